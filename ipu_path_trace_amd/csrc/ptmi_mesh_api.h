// ptmi_mesh_api.h -- the meshes' entry points (include/ptmi.h): pt_set_scene_meshes, the trees' options and read-back, vertex
// updates, normals, textures and the three hooks.  Their host logic is in ptmi_mesh*.h, their kernels in pt_mesh*.h.  Part of the
// one translation unit ptmi.hip, included at its end, ahead of ptmi_film_comm.h.
#pragma once

// A scene without a mesh takes over: the MESH instances stop running and the meshes' memory goes back (hipFree waits for the device).
static void drop_meshes(pt_handle h) {
  if (!h->scene_mesh && h->mesh.mesh.empty()) return;
  h->scene_mesh = false;
  (void)hipSetDevice(h->cfg.device);
  h->mesh = pt_context::MeshSet{};
}

// Mesh `mesh` of the scene in force, or null with the error of entry point `who` set: the scene has no such mesh.
static pt_context::MeshSet::One* mesh_at(pt_handle h, uint32_t mesh, const char* who) {
  const size_t count = (h->scene_n && h->scene_mesh) ? h->mesh.mesh.size() : 0;
  if (mesh < count) return &h->mesh.mesh[mesh];
  h->error = std::string(who) + ": mesh " + std::to_string(mesh) + " of " + std::to_string(count) + " in the scene in force";
  return nullptr;
}

// What pt_mesh_tree and the hooks need first: a scene in force that holds a mesh.
static int need_mesh_scene(pt_handle h, const char* who) {
  if (h->scene_n && h->scene_mesh) return PT_OK;
  return fail(h, PT_ERR_NOT_READY, std::string(who) + ": the scene in force holds no mesh (pt_set_scene_meshes)");
}

// The hooks' limit: origin and direction are three floats per ray.
constexpr ProbeLimit kMeshProbeRays{(1ull << 31) / 3, "too many rays"};

extern "C" {

// pt_set_scene_ex with meshes.  Everything is checked, copied, built and on the device before the scene in force changes: a
// rejection or a failed allocation leaves it as it was.
int pt_set_scene_meshes(pt_handle h, const pt_scene_object_ex* objects, uint32_t n, uint32_t stride, const pt_mesh* meshes,
                        uint32_t n_meshes) {
  if (!objects && n == 0 && stride == sizeof(pt_scene_object_ex) && !meshes && n_meshes == 0) {   // the built-in scene
    if (!h) { g_create_error = "pt_set_scene_meshes: null handle"; return PT_ERR_INVALID_ARGUMENT; }
    return pt_set_scene(h, nullptr, 0);
  }
  const std::string bad = ptmesh::check(objects, n, stride, meshes, n_meshes);
  if (!bad.empty()) {   // the scene in force stays
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_set_scene_meshes: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  if (n_meshes == 0) return pt_set_scene_ex(h, objects, n, stride);   // no mesh row: pt_set_scene_ex's scene, on its kernels
  PT_HIP(hipSetDevice(h->cfg.device));
  try {   // (the host copies are large -- 48 bytes per triangle and the builder's arrays: no exception crosses the C boundary)
  pt_context::MeshSet M;
  size_t triangles = 0, nodes = 0;
  for (uint32_t i = 0, m = 0; i < n; ++i) {
    if (objects[i].shape != PT_SHAPE_MESH) continue;
    pt_context::MeshSet::One one{};
    one.object_index = i;
    one.n_triangles = meshes[m].n_triangles;
    one.n_vertices = meshes[m].n_vertices;
    M.indices.insert(M.indices.end(), meshes[m].indices, meshes[m].indices + 3 * (size_t)meshes[m].n_triangles);
    one.tri_base = (uint32_t)triangles;
    one.node_base = (uint32_t)nodes;
    ptmesh::world_frames(meshes[m], M.world);
    M.mesh.push_back(one);
    triangles += one.n_triangles;
    nodes += 2 * (size_t)one.n_triangles - 1;
    m += 1;
  }
  PT_HIP(dev_alloc(M.d_nodes, nodes));
  PT_HIP(dev_alloc(M.d_tris, 3 * triangles));
  PT_HIP(dev_alloc(M.d_orig, triangles));
  const ptcamera::Basis& cb = h->camera_basis;
  if (mesh_device_option(h))   // (pt_set_mesh_build: the options outlive the scene, so their storage comes with every scene)
    if (int rc = ensure_mesh_device(h, M)) return rc;
  if (int rc = update_meshes(h, M, cb.identity ? nullptr : &cb)) return rc;
  // commit: the table as stored -- a mesh row with shape 4, its material and colour, and zeros
  pt_scene_object_ex stored[PT_MAX_SCENE_OBJECTS];
  std::copy(objects, objects + n, stored);
  for (uint32_t i = 0; i < n; ++i)
    if (stored[i].shape == PT_SHAPE_MESH) { stored[i].radius = 0.f; for (int k = 0; k < 3; ++k) stored[i].centre[k] = 0.f; }
  ptscene::normalise_ex(stored, n);   // (a mesh row: normal and vertex 0, as a sphere's)
  bool poly = false;
  for (uint32_t i = 0; i < n; ++i) {
    memcpy(&h->scene[i], &stored[i], sizeof(pt_scene_object));
    memcpy(h->scene_vertex[i], stored[i].vertex, sizeof(stored[i].vertex));
    poly = poly || ptscene::is_polygon(stored[i].shape);
  }
  h->scene_n = n;
  h->scene_poly = poly;   // (which rows are polygons: the light guide's polygon lamps and pt_get_scene_ex ask; the MESH instances run)
  h->mesh = std::move(M);
  h->scene_mesh = true;
  h->feature_gen += 1;
  rebuild_light_guide(h);
  return PT_OK;
  } catch (const std::bad_alloc&) {   // nothing of the scene in force has changed yet
    return fail(h, PT_ERR_OUT_OF_MEMORY, "pt_set_scene_meshes: out of host memory for the meshes' copies");
  }
}

int pt_get_mesh_info(pt_handle h, uint32_t mesh, pt_mesh_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_info")) return rc;
  const pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_get_mesh_info");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  const pt_context::MeshSet::One& m = *pm;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->object_index = m.object_index;
  out->n_triangles = m.n_triangles;
  out->n_nodes = m.n_nodes;
  out->max_leaf = m.max_leaf;
  out->depth = m.depth;
  out->device_bytes = (2 * (uint64_t)m.n_triangles - 1) * sizeof(ptmesh::Node) + (uint64_t)m.n_triangles * (3 * sizeof(ptmesh::F4) + sizeof(uint32_t));
  out->build_ms = m.build_ms;
  out->pad = m.pad;
  return PT_OK;
}

// Who builds the trees and what a pose change does to them (include/ptmi.h).  Everything the device paths need is allocated here,
// before the options change: a failed allocation leaves them as they were.
int pt_set_mesh_build(pt_handle h, const pt_mesh_build_options* o) {
  const pt_mesh_build_options defaults{sizeof(pt_mesh_build_options), PT_MESH_BUILDER_HOST, PT_MESH_POSE_REBUILD};
  const pt_mesh_build_options& O = o ? *o : defaults;
  std::string bad;
  if (O.struct_size != sizeof(pt_mesh_build_options))
    bad = "pt_set_mesh_build: struct_size must be " + std::to_string(sizeof(pt_mesh_build_options)) + " (got " + std::to_string(O.struct_size) + ")";
  else if (O.builder != PT_MESH_BUILDER_HOST && O.builder != PT_MESH_BUILDER_DEVICE)
    bad = "pt_set_mesh_build: builder must be 0 (host) or 1 (device) (got " + std::to_string(O.builder) + ")";
  else if (O.on_pose != PT_MESH_POSE_REBUILD && O.on_pose != PT_MESH_POSE_REFIT)
    bad = "pt_set_mesh_build: on_pose must be 0 (rebuild) or 1 (refit) (got " + std::to_string(O.on_pose) + ")";
  if (!bad.empty()) {
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_set_mesh_build: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  const bool device = O.builder == PT_MESH_BUILDER_DEVICE || O.on_pose == PT_MESH_POSE_REFIT;
  if (device && h->scene_n && h->scene_mesh)
    if (int rc = ensure_mesh_device(h, h->mesh)) return rc;
  if (O.builder != h->mesh_builder) {   // the trees of the scene in force are the other builder's: stale, and no refit may keep them
    h->mesh.built = false;
    h->mesh.topo_builder = -1;
  }
  h->mesh_builder = O.builder;
  h->mesh_on_pose = O.on_pose;
  return PT_OK;
}

int pt_get_mesh_build_info(pt_handle h, pt_mesh_build_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_build_info")) return rc;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->builder = h->mesh_builder;
  out->on_pose = h->mesh_on_pose;
  out->sort_on_device = PT_LBVH_DEVICE_SORT;
  out->host_builds = h->mesh_host_builds;
  out->device_builds = h->mesh_device_builds;
  out->refits = h->mesh_refits;
  out->last_kind = h->mesh_last_kind;
  out->last_ms = h->mesh_last_ms;
  out->device_bytes = (h->scene_n && h->scene_mesh) ? h->mesh.dev.bytes + h->mesh.dev.sah_bytes : 0u;
  return PT_OK;
}

// Which tree PT_MESH_BUILDER_DEVICE builds (include/ptmi.h).  The SAH builder's arrays are allocated here, before the kind
// changes: a failed allocation leaves it as it was.
static_assert(sizeof(pt_mesh_device_tree_info) == 40, "pt_mesh_device_tree_info layout");
int pt_set_mesh_device_tree(pt_handle h, int32_t kind) {
  if (kind != PT_MESH_DEVICE_TREE_LINEAR && kind != PT_MESH_DEVICE_TREE_SAH) {
    const std::string bad = "pt_set_mesh_device_tree: kind must be 0 (linear) or 1 (sah) (got " + std::to_string(kind) + ")";
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_set_mesh_device_tree: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  if (kind == PT_MESH_DEVICE_TREE_SAH && mesh_device_option(h) && h->scene_n && h->scene_mesh)
    if (int rc = ensure_mesh_device(h, h->mesh, false, false, true)) return rc;
  if (kind != h->mesh_device_tree && h->mesh_builder == PT_MESH_BUILDER_DEVICE) {   // the other kind's trees: stale, and no refit may keep them
    h->mesh.built = false;
    h->mesh.topo_builder = -1;
  }
  h->mesh_device_tree = kind;
  return PT_OK;
}

int pt_get_mesh_device_tree_info(pt_handle h, pt_mesh_device_tree_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_device_tree_info")) return rc;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->kind = h->mesh_device_tree;
  out->sah_builds = h->mesh_sah_builds;
  out->last_levels = h->mesh_sah_last_levels;
  out->last_ms = h->mesh_sah_last_ms;
  out->device_bytes = (h->scene_n && h->scene_mesh) ? h->mesh.dev.sah_bytes : 0u;
  return PT_OK;
}

static_assert(sizeof(pt_mesh_node) == sizeof(ptmesh::Node) && sizeof(pt_mesh_build_options) == 12 && sizeof(pt_mesh_build_info) == 64,
              "pt_mesh_node / pt_mesh_build_* layout");
int pt_mesh_tree(pt_handle h, uint32_t mesh, pt_mesh_node* nodes, uint32_t node_capacity, uint32_t* orig, uint32_t orig_capacity) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = need_mesh_scene(h, "pt_mesh_tree")) return rc;
  const pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_mesh_tree");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  if ((!nodes && node_capacity) || (!orig && orig_capacity)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_mesh_tree: a null buffer with a capacity");
  if (int rc = ensure_meshes(h)) return rc;   // the camera in force, exactly as a render
  const pt_context::MeshSet::One& m = *pm;
  if (nodes && node_capacity < m.n_nodes)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_mesh_tree: node_capacity must be >= " + std::to_string(m.n_nodes) + " (got " + std::to_string(node_capacity) + ")");
  if (orig && orig_capacity < m.n_triangles)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_mesh_tree: orig_capacity must be >= " + std::to_string(m.n_triangles) + " (got " + std::to_string(orig_capacity) + ")");
  if (nodes) PT_HIP(hipMemcpy(nodes, h->mesh.d_nodes + m.node_base, m.n_nodes * sizeof(ptmesh::Node), hipMemcpyDeviceToHost));
  if (orig) PT_HIP(hipMemcpy(orig, h->mesh.d_orig + m.tri_base, m.n_triangles * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return PT_OK;
}

// New vertices (and normals) for mesh `mesh` of the scene in force (include/ptmi.h; ptmi_mesh_update.h).  Everything is allocated,
// copied into staging and checked on the device before a byte of the geometry in force changes.
static_assert(sizeof(pt_mesh_update) == 40 && offsetof(pt_mesh_update, vertices) == 16 && offsetof(pt_mesh_update, normals) == 32 &&
              sizeof(pt_mesh_update_info) == 64, "pt_mesh_update* layout");
int pt_update_mesh_vertices(pt_handle h, uint32_t mesh, const pt_mesh_update* u) {
  std::string bad;
  if (!u) bad = "pt_update_mesh_vertices: null update";
  else if (u->struct_size != sizeof(pt_mesh_update))
    bad = "pt_update_mesh_vertices: struct_size must be " + std::to_string(sizeof(pt_mesh_update)) + " (got " + std::to_string(u->struct_size) + ")";
  else if (u->mode != PT_MESH_UPDATE_REFIT && u->mode != PT_MESH_UPDATE_REBUILD)
    bad = "pt_update_mesh_vertices: mode must be 0 (refit) or 1 (rebuild) (got " + std::to_string(u->mode) + ")";
  else if (u->memory != PT_MESH_UPDATE_HOST_MEMORY && u->memory != PT_MESH_UPDATE_DEVICE_MEMORY)
    bad = "pt_update_mesh_vertices: memory must be 0 (host) or 1 (device) (got " + std::to_string(u->memory) + ")";
  else if (!u->vertices) bad = "pt_update_mesh_vertices: null vertices";
  else if (!u->normals && u->n_normals != 0) bad = "pt_update_mesh_vertices: null normals with n_normals = " + std::to_string(u->n_normals);
  else if (u->normals && u->n_normals == 0) bad = "pt_update_mesh_vertices: normals with n_normals = 0";
  if (!bad.empty()) {
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_update_mesh_vertices: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_update_mesh_vertices");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  pt_context::MeshSet& M = h->mesh;
  pt_context::MeshSet::One& m = *pm;
  const std::string at = "pt_update_mesh_vertices: mesh " + std::to_string(mesh) + ": ";
  if (u->n_vertices != m.n_vertices)
    return fail(h, PT_ERR_INVALID_ARGUMENT, at + "n_vertices must equal the mesh's " + std::to_string(m.n_vertices) + " (got " + std::to_string(u->n_vertices) + ")");
  if (u->normals && m.normals.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, at + "normals for a mesh without normals (pt_set_mesh_normals)");
  if (u->normals && u->n_normals != m.n_normals)
    return fail(h, PT_ERR_INVALID_ARGUMENT, at + "n_normals must equal the attached " + std::to_string(m.n_normals) + " (got " + std::to_string(u->n_normals) + ")");
  // storage: nothing of the scene changes here
  if (int rc = drain_for_meshes(h, M)) return rc;
  const uint64_t dev_before = M.dev.bytes;
  if (int rc = ensure_mesh_device(h, M)) return rc;
  M.upd.bytes += M.dev.bytes - dev_before;
  if (int rc = ensure_mesh_update(h, M)) return rc;
  // staging, the check, and the commit
  pt_context::MeshSet::Update& U = M.upd;
  const hipMemcpyKind kind = u->memory == PT_MESH_UPDATE_DEVICE_MEMORY ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const uint32_t T = m.n_triangles;
  const uint32_t* indices = U.indices + 3 * (size_t)m.tri_base;
  const float* normals = u->normals ? (const float*)U.normals : nullptr;
  const uint32_t* normal_indices = !u->normals ? nullptr : m.per_corner ? U.normal_indices + 3 * (size_t)m.tri_base : indices;
  const dim3 grid(ptupdate::blocks_for(T)), block(ptupdate::kBlock);
  unsigned long long* fault = reinterpret_cast<unsigned long long*>((uint64_t*)U.fault);
  uint64_t fault_host[2] = {ptupdate::kNoFault, ptupdate::kNoFault};
  PT_HIP(hipEventRecord(h->mesh_update_event[0], h->stream));
  PT_HIP(hipMemcpyAsync(U.vertices, u->vertices, 12 * (size_t)m.n_vertices, kind, h->stream));
  if (normals) PT_HIP(hipMemcpyAsync(U.normals, u->normals, 12 * (size_t)m.n_normals, kind, h->stream));
  PT_HIP(hipMemsetAsync(U.fault, 0xff, sizeof(fault_host), h->stream));
  hipLaunchKernelGGL(ptupdate::mesh_update_check_kernel, grid, block, 0, h->stream, T, indices, (const float*)U.vertices, normal_indices, normals, fault);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpyAsync(fault_host, U.fault, sizeof(fault_host), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  if (fault_host[0] != ptupdate::kNoFault || fault_host[1] != ptupdate::kNoFault)   // the geometry in force stands
    return mesh_update_rejection(h, M, mesh, fault_host[0], fault_host[1]);
  hipLaunchKernelGGL(ptupdate::mesh_update_commit_kernel, grid, block, 0, h->stream, T, indices, (const float*)U.vertices, normal_indices, normals,
                     M.dev.world + ptlbvh::kFrameFloats * (size_t)m.tri_base, normals ? M.dev.corner + 9 * (size_t)m.tri_base : (float*)nullptr);
  PT_HIP(hipGetLastError());
  PT_HIP(hipEventRecord(h->mesh_update_event[1], h->stream));
  PT_HIP(hipEventSynchronize(h->mesh_update_event[1]));
  float frames_ms = 0.f;
  PT_HIP(hipEventElapsedTime(&frames_ms, h->mesh_update_event[0], h->mesh_update_event[1]));
  m.world_stale = true;
  m.normals_stale = m.normals_stale || normals != nullptr;
  h->feature_gen += 1;
  // the tree (a pass that fails leaves the trees marked stale: the next call that traces builds them from the new frames)
  int tree_kind = PT_MESH_LAST_NONE;
  bool fallback = false;
  if (int rc = mesh_update_tree(h, M, mesh, u->mode, tree_kind, fallback)) return rc;
  h->mesh_updates += 1;
  (tree_kind == PT_MESH_LAST_REFIT ? h->mesh_update_refits : h->mesh_update_rebuilds) += 1;
  h->mesh_update_fallbacks += fallback ? 1 : 0;
  h->mesh_update_last_kind = tree_kind;
  h->mesh_update_frames_ms = frames_ms;
  h->mesh_update_tree_ms = h->mesh_last_ms;
  return PT_OK;
}

int pt_get_mesh_update_info(pt_handle h, pt_mesh_update_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_update_info")) return rc;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->last_kind = h->mesh_update_last_kind;
  out->updates = h->mesh_updates;
  out->refits = h->mesh_update_refits;
  out->rebuilds = h->mesh_update_rebuilds;
  out->fallbacks = h->mesh_update_fallbacks;
  out->last_frames_ms = h->mesh_update_frames_ms;
  out->last_tree_ms = h->mesh_update_tree_ms;
  out->device_bytes = (h->scene_n && h->scene_mesh) ? h->mesh.upd.bytes : 0u;
  return PT_OK;
}

int pt_mesh_intersect(pt_handle h, const float* origin, const float* dir, size_t n, int32_t mode, float* out_t, int32_t* out_object,
                      int32_t* out_triangle) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = need_mesh_scene(h, "pt_mesh_intersect")) return rc;
  if (mode != PT_MESH_INTERSECT_BVH && mode != PT_MESH_INTERSECT_BRUTE)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_mesh_intersect: mode must be 0 (BVH) or 1 (brute force) (got " + std::to_string(mode) + ")");
  return probe(h, n, kMeshProbeRays, std::tuple{in(origin, 3), in(dir, 3), out(out_t), out(out_object), out(out_triangle)},
               [&](const float* o, const float* d, float* t, int32_t* object, int32_t* triangle) -> int {
    ptd::TraceParams P;
    if (int rc = mesh_probe_params(h, P)) return rc;
    hipLaunchKernelGGL(mode == PT_MESH_INTERSECT_BRUTE ? ptd::mesh_intersect_brute_kernel : ptd::mesh_intersect_kernel, probe_grid(n),
                       dim3(kProbeBlock), 0, h->stream, P, o, d, (uint32_t)n, t, object, triangle);
    return PT_OK;
  });
}

// Vertex normals of mesh `mesh` of the scene in force.  Checked and copied on the host, and the device buffer allocated, before
// anything of the mesh changes; the trees are then marked stale, so that the next call that traces re-expands the normals into the
// slot order of the frame it traces in (build_meshes), exactly as after a pose change.
int pt_set_mesh_normals(pt_handle h, uint32_t mesh, const float* normals, uint32_t n_normals, const uint32_t* normal_indices) {
  if (!h) { g_create_error = "pt_set_mesh_normals: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_set_mesh_normals");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  pt_context::MeshSet& M = h->mesh;
  pt_context::MeshSet::One& m = *pm;
  try {
  if (!normals && n_normals == 0 && !normal_indices) {   // remove: the mesh is flat again
    if (m.normals.empty()) return PT_OK;
    std::vector<float>().swap(m.normals);
    std::vector<uint32_t>().swap(m.normal_indices);
    m.n_normals = 0; m.per_corner = false; m.normals_stale = false;
  } else {
    const std::string bad = ptmesh::check_normals(mesh, m.n_vertices, m.n_triangles, M.indices.data() + 3 * (size_t)m.tri_base, normals,
                                                  n_normals, normal_indices);
    if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);   // the mesh keeps what it had
    std::vector<float> corner;
    ptmesh::corner_normals(m.n_triangles, M.indices.data() + 3 * (size_t)m.tri_base, normals, normal_indices, corner);
    std::vector<uint32_t> kept;   // (pt_update_mesh_vertices looks new per-corner normals up by the caller's indices)
    if (normal_indices) kept.assign(normal_indices, normal_indices + 3 * (size_t)m.n_triangles);
    if (!M.d_normals) {
      PT_HIP(hipSetDevice(h->cfg.device));
      const size_t triangles = M.triangles();
      const hipError_t e = dev_alloc(M.d_normals, 3 * triangles);
      if (e != hipSuccess)
        return fail(h, hip_status(e), "pt_set_mesh_normals: allocating " + std::to_string(3 * triangles * sizeof(ptmesh::F4)) + " bytes: " + hipGetErrorString(e));
    }
    if (mesh_device_option(h))   // (pt_set_mesh_build: the triangle-order copy the device paths expand from)
      if (int rc = ensure_mesh_device(h, M, true, false)) return rc;
    m.normals.swap(corner);
    m.normal_indices.swap(kept);
    m.n_normals = n_normals; m.per_corner = normal_indices != nullptr; m.normals_stale = false;
    if (int rc = upload_mesh_corners(h, M, mesh)) return rc;
  }
  drop_mesh_update_normals(M);
  } catch (const std::bad_alloc&) {
    return fail(h, PT_ERR_OUT_OF_MEMORY, "pt_set_mesh_normals: out of host memory for the normals' copy");
  }
  M.built = false;        // the next trace rebuilds: rows' flags and the normals in slot order
  M.topo_builder = -1;    // (a build, never a refit: pt_set_mesh_build)
  h->feature_gen += 1;
  return PT_OK;
}

int pt_get_mesh_normals_info(pt_handle h, uint32_t mesh, pt_mesh_normals_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_normals_info")) return rc;
  const pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_get_mesh_normals_info");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  const pt_context::MeshSet::One& m = *pm;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  out->has_normals = m.normals.empty() ? 0u : 1u;
  out->per_corner = m.per_corner ? 1u : 0u;
  out->n_normals = m.n_normals;
  out->device_bytes = m.normals.empty() ? 0u : (uint64_t)m.n_triangles * 3 * sizeof(ptmesh::F4);
  return PT_OK;
}

int pt_mesh_shade(pt_handle h, const float* origin, const float* dir, size_t n, float* out_t, int32_t* out_object, int32_t* out_triangle,
                  float* out_bary, float* out_normal) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = need_mesh_scene(h, "pt_mesh_shade")) return rc;
  return probe(h, n, kMeshProbeRays,
               std::tuple{in(origin, 3), in(dir, 3), out(out_t), out(out_object), out(out_triangle), out(out_bary, 2), out(out_normal, 3)},
               [&](const float* o, const float* d, float* t, int32_t* object, int32_t* triangle, float* bary, float* normal) -> int {
    ptd::TraceParams P;
    if (int rc = mesh_probe_params(h, P)) return rc;
    hipLaunchKernelGGL(ptd::mesh_shade_kernel, probe_grid(n), dim3(kProbeBlock), 0, h->stream, P, o, d, (uint32_t)n, t, object, triangle,
                       bary, normal);
    return PT_OK;
  });
}

// The texture of mesh `mesh` of the scene in force.  Checked and copied on the host, and every device buffer allocated and filled,
// before anything of the mesh changes; the trees are then marked stale, so that the next call that traces re-expands the uvs into
// the slot order of the frame it traces in (build_meshes), exactly as after a pose change.
int pt_set_mesh_texture(pt_handle h, uint32_t mesh, const pt_mesh_texture* t) {
  if (!h) { g_create_error = "pt_set_mesh_texture: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_set_mesh_texture");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  pt_context::MeshSet& M = h->mesh;
  pt_context::MeshSet::One& m = *pm;
  const auto drain = [&]() -> hipError_t {   // a step in flight may still read the image and the descriptors
    for (hipStream_t s : {h->stream, h->trace_stream, h->acc_stream})
      if (s) if (hipError_t e = hipStreamSynchronize(s)) return e;
    return hipSuccess;
  };
  try {
  if (!t) {   // remove: the mesh has its one colour again
    if (m.uvs.empty()) return PT_OK;
    PT_HIP(hipSetDevice(h->cfg.device));
    PT_HIP(drain());
    ptmesh::TexDesc table[PT_MAX_SCENE_OBJECTS];   // the new table in a temporary: committed only once it is on the device
    memcpy(table, M.desc, sizeof(table));
    table[m.object_index] = ptmesh::TexDesc{};
    PT_HIP(hipMemcpy(M.d_desc, table, sizeof(table), hipMemcpyHostToDevice));
    memcpy(M.desc, table, sizeof(table));
    M.d_texels[mesh].reset();
    std::vector<float>().swap(m.uvs);
    m.n_uvs = 0; m.tex_w = m.tex_h = 0; m.tex_filter = m.tex_wrap = 0; m.uv_per_corner = false;
  } else {
    const std::string bad = ptmesh::check_texture(mesh, m.n_vertices, m.n_triangles, M.indices.data() + 3 * (size_t)m.tri_base, t);
    if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);   // the mesh keeps what it had
    std::vector<float> corner;
    ptmesh::corner_uvs(m.n_triangles, M.indices.data() + 3 * (size_t)m.tri_base, t->uvs, t->uv_indices, corner);
    std::vector<ptmesh::F4> texels;
    ptmesh::texel_vectors(t, texels);
    if (M.d_texels.size() < M.mesh.size()) M.d_texels.resize(M.mesh.size());
    PT_HIP(hipSetDevice(h->cfg.device));
    if (!M.d_uvs) {
      const size_t triangles = M.triangles();
      DevBuf<float> uvs;
      DevBuf<ptmesh::TexDesc> desc;
      hipError_t e = dev_alloc(uvs, 6 * triangles);
      if (e == hipSuccess) e = dev_alloc(desc, PT_MAX_SCENE_OBJECTS);
      if (e == hipSuccess) e = hipMemset(uvs, 0, 6 * triangles * sizeof(float));
      if (e != hipSuccess)
        return fail(h, hip_status(e), "pt_set_mesh_texture: allocating " + std::to_string(6 * triangles * sizeof(float) + sizeof(M.desc)) + " bytes: " + hipGetErrorString(e));
      M.d_uvs = std::move(uvs);
      M.d_desc = std::move(desc);
    }
    DevBuf<ptmesh::F4> image;
    hipError_t e = dev_alloc(image, texels.size());
    if (e == hipSuccess) e = hipMemcpy(image, texels.data(), texels.size() * sizeof(ptmesh::F4), hipMemcpyHostToDevice);
    if (e != hipSuccess)
      return fail(h, hip_status(e), "pt_set_mesh_texture: allocating " + std::to_string(texels.size() * sizeof(ptmesh::F4)) + " bytes: " + hipGetErrorString(e));
    if (mesh_device_option(h))   // (pt_set_mesh_build: the triangle-order copy the device builder expands from)
      if (int rc = ensure_mesh_device(h, M, false, true)) return rc;
    PT_HIP(drain());
    ptmesh::TexDesc d{};
    d.texels = image; d.width = t->width; d.height = t->height; d.filter = t->filter; d.wrap = t->wrap;
    ptmesh::TexDesc table[PT_MAX_SCENE_OBJECTS];   // the new table in a temporary: a failed copy leaves the host's table, and with it
    memcpy(table, M.desc, sizeof(table));          // every later upload, without a pointer into the image freed on the way out
    table[m.object_index] = d;
    PT_HIP(hipMemcpy(M.d_desc, table, sizeof(table), hipMemcpyHostToDevice));
    memcpy(M.desc, table, sizeof(table));
    M.d_texels[mesh] = std::move(image);   // (frees the image it replaces)
    m.uvs.swap(corner);
    m.n_uvs = t->n_uvs; m.tex_w = t->width; m.tex_h = t->height; m.tex_filter = t->filter; m.tex_wrap = t->wrap;
    m.uv_per_corner = t->uv_indices != nullptr;
    if (int rc = upload_mesh_corners(h, M, mesh)) return rc;
  }
  } catch (const std::bad_alloc&) {
    return fail(h, PT_ERR_OUT_OF_MEMORY, "pt_set_mesh_texture: out of host memory for the texture's copy");
  }
  M.built = false;        // the next trace rebuilds: rows' flags and the uvs in slot order
  M.topo_builder = -1;    // (a build, never a refit: pt_set_mesh_build)
  h->feature_gen += 1;
  return PT_OK;
}

int pt_get_mesh_texture_info(pt_handle h, uint32_t mesh, pt_mesh_texture_info* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = check_info(h, out, "pt_get_mesh_texture_info")) return rc;
  const pt_context::MeshSet::One* pm = mesh_at(h, mesh, "pt_get_mesh_texture_info");
  if (!pm) return PT_ERR_INVALID_ARGUMENT;
  const pt_context::MeshSet::One& m = *pm;
  memset(out, 0, sizeof(*out));
  out->struct_size = sizeof(*out);
  if (m.uvs.empty()) return PT_OK;
  out->has_texture = 1u;
  out->per_corner = m.uv_per_corner ? 1u : 0u;
  out->width = m.tex_w; out->height = m.tex_h;
  out->filter = m.tex_filter; out->wrap = m.tex_wrap;
  out->n_uvs = m.n_uvs;
  out->device_bytes = (uint64_t)m.n_triangles * 6 * sizeof(float) + (uint64_t)m.tex_w * m.tex_h * sizeof(ptmesh::F4);
  return PT_OK;
}

int pt_mesh_texel(pt_handle h, const float* origin, const float* dir, size_t n, float* out_t, int32_t* out_object, int32_t* out_triangle,
                  float* out_uv, float* out_bgr) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = need_mesh_scene(h, "pt_mesh_texel")) return rc;
  return probe(h, n, kMeshProbeRays,
               std::tuple{in(origin, 3), in(dir, 3), out(out_t), out(out_object), out(out_triangle), out(out_uv, 2), out(out_bgr, 3)},
               [&](const float* o, const float* d, float* t, int32_t* object, int32_t* triangle, float* uv, float* bgr) -> int {
    ptd::TraceParams P;
    if (int rc = mesh_probe_params(h, P)) return rc;
    const ptd::TexParams X = tex_params(h);   // (no textured mesh: every row's flag is 0 and the kernel reads neither pointer)
    hipLaunchKernelGGL(ptd::mesh_texel_kernel, probe_grid(n), dim3(kProbeBlock), 0, h->stream, P, X, o, d, (uint32_t)n, t, object, triangle,
                       uv, bgr);
    return PT_OK;
  });
}

}  // extern "C"
