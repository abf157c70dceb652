// ptmi_mesh_update.h -- a mesh of the scene in force moved in place (pt_update_mesh_vertices, include/ptmi.h): the two kernels,
// thin wrappers around the functions of pt_mesh_update.h (ONE definition for the device, the host and the test program), the
// device storage they need, and the handle's side.  An update checks the new vertices on the device, writes the mesh's world
// frames (and corner normals) into the device paths' triangle-order copies (ptmi_mesh_build.h: DeviceBuild::world / corner), and
// then runs ONE mesh's body of refit_meshes or of the builder in force.  The other meshes, the uvs, the textures and the scene
// table are not touched.  Nothing is allocated after the first update of a scene.
#pragma once
#include "pt_mesh_update.h"

namespace ptupdate {

constexpr uint32_t kBlock = 256;
inline uint32_t blocks_for(uint32_t threads) { return (threads + kBlock - 1) / kBlock; }

// fault[0] / fault[1]: the first fault among the frames / among the corner normals (start kNoFault).  A wave reduces its words by
// their minimum and its first lane issues one atomicMin: integers, exact in any order.  normals == nullptr: the frames alone.
__global__ void mesh_update_check_kernel(uint32_t n, const uint32_t* __restrict__ indices, const float* __restrict__ vertices,
                                         const uint32_t* __restrict__ normal_indices, const float* __restrict__ normals,
                                         unsigned long long* fault) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  unsigned long long wf = kNoFault, wn = kNoFault;
  if (j < n) {
    float fr[kFrameFloats];
    wf = fault_word(j, frame_thread(j, indices, vertices, fr));
    if (normals) {
      float cn[9];
      wn = fault_word(j, corner_normals_thread(j, normal_indices, normals, cn));
    }
  }
  for (int m = warpSize / 2; m >= 1; m >>= 1) {
    wf = combine(wf, __shfl_xor(wf, m));
    wn = combine(wn, __shfl_xor(wn, m));
  }
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (wf != kNoFault) atomicMin(&fault[0], wf);
    if (wn != kNoFault) atomicMin(&fault[1], wn);
  }
}

// world / corner: the mesh's own part of the triangle-order copies (48 / 36 bytes per triangle).  Launched only after the check
// found no fault.
__global__ void mesh_update_commit_kernel(uint32_t n, const uint32_t* __restrict__ indices, const float* __restrict__ vertices,
                                          const uint32_t* __restrict__ normal_indices, const float* __restrict__ normals,
                                          float* __restrict__ world, float* __restrict__ corner) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  float fr[kFrameFloats];
  (void)frame_thread(j, indices, vertices, fr);
  ptmesh::F4* out = reinterpret_cast<ptmesh::F4*>(world) + 3u * (size_t)j;   // (48 bytes per triangle from a 256-byte aligned base)
  out[0] = ptmesh::F4{fr[0], fr[1], fr[2], fr[3]};
  out[1] = ptmesh::F4{fr[4], fr[5], fr[6], fr[7]};
  out[2] = ptmesh::F4{fr[8], fr[9], fr[10], fr[11]};
  if (normals) {
    float cn[9];
    (void)corner_normals_thread(j, normal_indices, normals, cn);
    for (int k = 0; k < 9; ++k) corner[9u * (size_t)j + k] = cn[k];
  }
}

}  // namespace ptupdate

// ---- the handle's side
namespace {

// What an update needs beside ensure_mesh_device's storage, allocated unless it is there already: the scene's triangle indices,
// a staging buffer for the mesh with the most vertices, the two fault words and, for the scene's meshes with normals, the
// per-corner normal indices and a staging buffer for the most normals.  A failed allocation leaves M with what it had.
int ensure_mesh_update(pt_handle h, pt_context::MeshSet& M) {
  pt_context::MeshSet::Update& U = M.upd;
  size_t total = 0, vertices = 0, normals = 0;
  bool per_corner = false;
  for (const pt_context::MeshSet::One& m : M.mesh) {
    total += m.n_triangles;
    vertices = std::max<size_t>(vertices, m.n_vertices);
    if (!m.normals.empty()) { normals = std::max<size_t>(normals, m.n_normals); per_corner = per_corner || m.per_corner; }
  }
  const auto oom = [&](hipError_t e, size_t bytes) {
    return fail(h, hip_status(e), "mesh update storage: allocating " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  };
  hipError_t e;
  if (!U.indices) {
    DevBuf<uint32_t> indices;
    DevBuf<float> staging;
    DevBuf<uint64_t> fault;
    if ((e = dev_alloc(indices, 3 * total)) != hipSuccess) return oom(e, 12 * total);
    if ((e = dev_alloc(staging, 3 * vertices)) != hipSuccess) return oom(e, 12 * vertices);
    if ((e = dev_alloc(fault, 2)) != hipSuccess) return oom(e, 16);
    PT_HIP(hipMemcpy(indices, M.indices.data(), 12 * total, hipMemcpyHostToDevice));
    U.indices = std::move(indices); U.vertices = std::move(staging); U.fault = std::move(fault);
    U.cap_vertices = vertices;
    U.bytes += 12 * total + 12 * vertices + 16;
  }
  if (normals > U.cap_normals || (per_corner && !U.normal_indices)) {   // (the first update, or normals attached since: drop_mesh_update_normals)
    DevBuf<float> staging;
    DevBuf<uint32_t> nidx;
    if ((e = dev_alloc(staging, 3 * normals)) != hipSuccess) return oom(e, 12 * normals);
    if (per_corner) {
      if ((e = dev_alloc(nidx, 3 * total)) != hipSuccess) return oom(e, 12 * total);
      for (const pt_context::MeshSet::One& m : M.mesh)
        if (!m.normals.empty() && m.per_corner)
          PT_HIP(hipMemcpy(nidx + 3 * (size_t)m.tri_base, m.normal_indices.data(), 12 * (size_t)m.n_triangles, hipMemcpyHostToDevice));
    }
    U.bytes -= 12 * (uint64_t)U.cap_normals + 4 * (uint64_t)U.normal_indices.count();
    U.normals = std::move(staging); U.normal_indices = std::move(nidx);
    U.cap_normals = normals;
    U.bytes += 12 * (uint64_t)normals + 4 * (uint64_t)U.normal_indices.count();
  }
  if (!h->mesh_update_event[0])
    for (hipEvent_t& ev : h->mesh_update_event) PT_HIP(hipEventCreate(&ev));
  return PT_OK;
}

// pt_set_mesh_normals changed which normals the scene's meshes have: the update path sizes and fills its normal buffers again at
// the next update.
inline void drop_mesh_update_normals(pt_context::MeshSet& M) {
  pt_context::MeshSet::Update& U = M.upd;
  U.bytes -= 12 * (uint64_t)U.cap_normals + 4 * (uint64_t)U.normal_indices.count();
  U.normals.reset(); U.normal_indices.reset();
  U.cap_normals = 0;
}

// The message of a rejected update, by the code pt_set_scene_meshes / pt_set_mesh_normals name the same data with: the one
// triangle's vertices (36 bytes), or its three normals, come back from the staging buffers.
int mesh_update_rejection(pt_handle h, pt_context::MeshSet& M, uint32_t mesh, uint64_t frames_fault, uint64_t normals_fault) {
  const pt_context::MeshSet::One& m = M.mesh[mesh];
  if (frames_fault != ptupdate::kNoFault) {
    const uint32_t j = ptupdate::fault_triangle(frames_fault);
    if (j >= m.n_triangles) return fail(h, PT_ERR_HIP, "pt_update_mesh_vertices: a fault at triangle " + std::to_string(j) + " of " + std::to_string(m.n_triangles));
    const uint32_t* ix = M.indices.data() + 3 * ((size_t)m.tri_base + j);
    float v[3][3];
    for (int c = 0; c < 3; ++c) PT_HIP(hipMemcpy(v[c], M.upd.vertices + 3 * (size_t)ix[c], 12, hipMemcpyDeviceToHost));
    return fail(h, PT_ERR_INVALID_ARGUMENT, "scene object " + std::to_string(m.object_index) + ", mesh " + std::to_string(mesh) + ", triangle " +
                                                std::to_string(j) + ": " + ptmesh::triangle_fault(ix, v));
  }
  const uint32_t j = ptupdate::fault_triangle(normals_fault);
  if (j >= m.n_triangles) return fail(h, PT_ERR_HIP, "pt_update_mesh_vertices: a fault at triangle " + std::to_string(j) + " of " + std::to_string(m.n_triangles));
  const uint32_t* ix = (m.per_corner ? m.normal_indices.data() : M.indices.data() + 3 * (size_t)m.tri_base) + 3 * (size_t)j;
  for (int c = 0; c < 3; ++c) {
    float v[3];
    PT_HIP(hipMemcpy(v, M.upd.normals + 3 * (size_t)ix[c], 12, hipMemcpyDeviceToHost));
    const std::string fault = ptmesh::normal_fault(ix[c], v);
    if (!fault.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, "mesh " + std::to_string(mesh) + ": triangle " + std::to_string(j) + ": " + fault);
  }
  return fail(h, PT_ERR_HIP, "pt_update_mesh_vertices: the device rejected normals the host accepts");   // (cannot happen: one rule)
}

// The tree pass after a commit, for mesh k alone where the trees of the scene are valid: a refit in the frame they are built for,
// or a build by the builder in force.  Stale trees (or another builder's or kind's topology) are built whole, for the camera in force, as
// the next trace would have built them.  kind: the PT_MESH_LAST_* of what ran.
int mesh_update_tree(pt_handle h, pt_context::MeshSet& M, size_t k, int32_t mode, int& kind, bool& fallback) {
  fallback = false;
  if (!M.built || !mesh_topology_in_force(h, M)) {
    const ptcamera::Basis& cb = h->camera_basis;
    const uint64_t refits = h->mesh_refits;
    if (int rc = update_meshes(h, M, cb.identity ? nullptr : &cb)) return rc;
    kind = h->mesh_last_kind;
    fallback = mode == PT_MESH_UPDATE_REFIT && h->mesh_refits == refits;
    return PT_OK;
  }
  const ptcamera::Basis frame = M.built_for;
  const ptcamera::Basis* cam = M.built_world ? nullptr : &frame;
  M.built = false;
  if (mode == PT_MESH_UPDATE_REFIT) {
    if (int rc = refit_mesh(h, M, k, ptlbvh::pose_of(cam))) return rc;
    kind = PT_MESH_LAST_REFIT;
  } else if (h->mesh_builder == PT_MESH_BUILDER_DEVICE) {
    if (int rc = build_mesh_device_of_kind(h, M, k, ptlbvh::pose_of(cam))) return rc;
    kind = PT_MESH_LAST_DEVICE_BUILD;
    note_sah_build(h, M.mesh[k].build_ms);
  } else {
    try {
      if (int rc = refresh_mesh_host(h, M)) return rc;
      MeshHostScratch X;
      if (int rc = build_mesh_host(h, M, M.mesh[k], cam, X)) return rc;
    } catch (const std::bad_alloc&) {   // the trees stay marked stale: the next call that traces builds them
      return fail(h, PT_ERR_OUT_OF_MEMORY, "pt_update_mesh_vertices: out of host memory while building the tree");
    }
    kind = PT_MESH_LAST_HOST_BUILD;
  }
  const int topo = M.topo_builder;
  mesh_finish_pass(M, cam);
  M.topo_builder = topo;
  note_mesh_pass(h, kind, M.mesh[k].build_ms);
  return PT_OK;
}

}  // namespace
