// ptmi_mesh_build.h -- mesh trees built and refitted on the device (pt_set_mesh_build, include/ptmi.h): the kernels, which are
// thin wrappers around the functions of pt_mesh_build.h (ONE definition for the device, the host reference and the test
// program), the device storage they need, and the two passes build_meshes_device / refit_meshes that stand beside build_meshes
// (ptmi_context.h), each a loop over the one-mesh body that pt_update_mesh_vertices (ptmi_mesh_update.h) runs alone.  Nothing here allocates during a build or a refit: ensure_mesh_device sizes everything for the largest mesh
// when the option is set and at every pt_set_scene_meshes under it.  No kernel waits on another workgroup: the bottom-up passes
// use arrival counters, the first thread to arrive returns (pt_mesh_build.h: arrive).
#pragma once
#include "pt_mesh_build.h"
#include "pt_mesh_sah.h"

// The keys are sorted by the radix sort below (pt_mesh_build_info.sort_on_device = 1).  rocprim's radix sort is not used: its
// host side reads an environment variable, which the product library must not do, and its one-sweep kernels look back at other
// workgroups' flags.
#define PT_LBVH_DEVICE_SORT 1

namespace ptlbvh {

constexpr uint32_t kBlock = 256;
inline uint32_t blocks_for(uint32_t threads) { return (threads + kBlock - 1) / kBlock; }

// float <-> a word whose unsigned order is the float's order
__device__ __forceinline__ uint32_t ordered(float f) { const uint32_t u = float_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float unordered(uint32_t u) { return bits_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// bounds[0..2]: min of the centroids as ordered words (start 0xffffffff), bounds[3..5]: max (start 0)
__global__ void lbvh_bounds_kernel(const float* __restrict__ world, uint32_t n, Pose P, uint32_t* bounds) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (j < n) {
    float fr[kFrameFloats];
    kernel_frame(P, world + (size_t)kFrameFloats * j, fr);
    centroid(fr, lo);
    for (int k = 0; k < 3; ++k) hi[k] = lo[k];
  }
  for (int m = warpSize / 2; m >= 1; m >>= 1)
    for (int k = 0; k < 3; ++k) { lo[k] = min2(lo[k], __shfl_xor(lo[k], m)); hi[k] = max2(hi[k], __shfl_xor(hi[k], m)); }
  if ((threadIdx.x & (warpSize - 1)) == 0 && lo[0] <= hi[0])
    for (int k = 0; k < 3; ++k) { atomicMin(&bounds[k], ordered(lo[k])); atomicMax(&bounds[3 + k], ordered(hi[k])); }
}
__global__ void lbvh_codes_kernel(const float* __restrict__ world, uint32_t n, Pose P, const uint32_t* __restrict__ bounds,
                                  uint64_t* __restrict__ codes, uint32_t* __restrict__ index) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  float b[6];
  for (int k = 0; k < 6; ++k) b[k] = unordered(bounds[k]);
  float fr[kFrameFloats], c[3];
  kernel_frame(P, world + (size_t)kFrameFloats * j, fr);
  centroid(fr, c);
  codes[j] = morton(c, b);
  index[j] = j;
}
// ---- a stable least-significant-digit radix sort of (code, index) pairs, eight bits a pass: per pass a histogram per tile of
// kSortTile keys (hist[digit][tile]), an exclusive scan of every digit's row (one workgroup per digit, totals[digit]), and a
// scatter in which a key's place is its digit's base + its tile's offset + its rank among the tile's earlier keys of that digit.
// Equal digits keep their order, so equal codes stay ordered by triangle index.  No kernel looks at another workgroup's progress.
constexpr uint32_t kSortRounds = 4, kSortTile = kSortRounds * kBlock, kSortDigits = 256, kSortPasses = 8;
static_assert(kBlock == kSortDigits, "one thread per digit");
inline uint32_t sort_tiles(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }
inline size_t sort_words(uint32_t n) { return (size_t)kSortDigits * sort_tiles(n) + kSortDigits; }   // hist, then totals

__global__ void lbvh_sort_hist_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t tiles, uint32_t* __restrict__ hist) {
  __shared__ uint32_t counts[kSortDigits];
  const uint32_t t = threadIdx.x;
  counts[t] = 0u;
  __syncthreads();
  for (uint32_t r = 0; r < kSortRounds; ++r) {
    const uint32_t i = blockIdx.x * kSortTile + r * kBlock + t;
    if (i < n) atomicAdd(&counts[(uint32_t)(keys[i] >> shift) & (kSortDigits - 1u)], 1u);
  }
  __syncthreads();
  hist[(size_t)t * tiles + blockIdx.x] = counts[t];
}
// workgroup d: row d of hist becomes its exclusive prefix sums, totals[d] its sum
__global__ void lbvh_sort_scan_kernel(uint32_t* hist, uint32_t tiles, uint32_t* __restrict__ totals) {
  __shared__ uint32_t sums[kBlock];
  const uint32_t t = threadIdx.x;
  uint32_t* row = hist + (size_t)blockIdx.x * tiles;
  const uint32_t per = (tiles + kBlock - 1u) / kBlock;
  const uint32_t begin = t * per < tiles ? t * per : tiles, end = begin + per < tiles ? begin + per : tiles;
  uint32_t mine = 0u;
  for (uint32_t i = begin; i < end; ++i) mine += row[i];
  sums[t] = mine;
  __syncthreads();
  for (uint32_t off = 1u; off < kBlock; off <<= 1) {
    const uint32_t v = t >= off ? sums[t - off] : 0u;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint32_t run = sums[t] - mine;
  for (uint32_t i = begin; i < end; ++i) { const uint32_t x = row[i]; row[i] = run; run += x; }
  if (t == kBlock - 1u) totals[blockIdx.x] = sums[t];
}
__global__ void lbvh_sort_scatter_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ values, uint32_t n, uint32_t shift,
                                         uint32_t tiles, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ totals,
                                         uint64_t* __restrict__ keys_out, uint32_t* __restrict__ values_out) {
  __shared__ uint32_t offs[kSortDigits], base[kSortDigits], dig[kBlock];
  const uint32_t t = threadIdx.x;
  offs[t] = totals[t];
  __syncthreads();
  if (t == 0u) {
    uint32_t acc = 0u;
    for (uint32_t d = 0; d < kSortDigits; ++d) { const uint32_t x = offs[d]; offs[d] = acc; acc += x; }
  }
  __syncthreads();
  offs[t] += hist[(size_t)t * tiles + blockIdx.x];
  base[t] = 0u;
  __syncthreads();
  for (uint32_t r = 0; r < kSortRounds; ++r) {
    const uint32_t i = blockIdx.x * kSortTile + r * kBlock + t;
    const bool valid = i < n;
    const uint64_t key = valid ? keys[i] : 0ull;
    const uint32_t d = valid ? (uint32_t)(key >> shift) & (kSortDigits - 1u) : kSortDigits;   // (no key has digit 256)
    dig[t] = d;
    __syncthreads();
    uint32_t rank = 0u;
    for (uint32_t u = 0; u < t; ++u) rank += dig[u] == d ? 1u : 0u;
    const uint32_t dst = valid ? offs[d] + base[d] + rank : 0u;
    __syncthreads();
    if (valid && dst < n) {   // (dst < n by construction: the histogram counted these very keys)
      keys_out[dst] = key;
      values_out[dst] = values[i];
      atomicAdd(&base[d], 1u);
    }
    __syncthreads();
  }
}

__global__ void lbvh_tree_kernel(const uint64_t* __restrict__ codes, uint32_t n, Scratch S) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) tree_thread(codes, n, i, S);
}
__global__ void lbvh_count_kernel(uint32_t n, Scratch S) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < n) count_thread(p, S);
}
__global__ void lbvh_emit_kernel(uint32_t n, Scratch S, Node* nodes, uint32_t* stats) {
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x < 2u * n - 1u) emit_thread(n, x, S, nodes, stats);
}
// Slot s takes triangle order[s].  orig / uvs: written when not null (a build); a refit leaves both as they are.
__global__ void lbvh_slots_kernel(uint32_t n, const uint32_t* __restrict__ order, Pose P, const float* __restrict__ world,
                                  const float* __restrict__ corner, const float* __restrict__ corner_uv, F4* __restrict__ tris,
                                  F4* __restrict__ normals, uint32_t* orig, float* __restrict__ uvs) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n) return;
  const uint32_t tri = order[s];
  slot_thread(s, tri, P, world, corner, tris, normals);
  if (orig) orig[s] = tri;
  if (uvs && corner_uv)
    for (int k = 0; k < 6; ++k) uvs[6u * (size_t)s + k] = corner_uv[6u * (size_t)tri + k];
}
__global__ void lbvh_box_leaf_kernel(uint32_t threads, Node* nodes, const F4* __restrict__ tris, Scratch S, uint32_t* stats, float pad_scale) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < threads) box_leaf_thread(i, nodes, tris, S, stats, pad_scale);
}
__global__ void lbvh_box_climb_kernel(uint32_t threads, Node* nodes, Scratch S, uint32_t* stats, float pad_scale) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < threads) box_climb_thread(i, nodes, S, stats, pad_scale);
}
__global__ void lbvh_pad_kernel(uint32_t threads, Node* nodes, const uint32_t* __restrict__ stats) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < threads) pad_thread(i, nodes, stats);
}

}  // namespace ptlbvh

// ---- the handle's side
namespace {

inline bool mesh_device_option(pt_handle h) { return h->mesh_builder == PT_MESH_BUILDER_DEVICE || h->mesh_on_pose == PT_MESH_POSE_REFIT; }
// Do the trees on the device (if any) have the topology a build by the options in force would give them: the builder's and, on
// the device, the kind's (pt_set_mesh_device_tree).  Only then may a refit keep them.
inline bool mesh_topology_in_force(pt_handle h, const pt_context::MeshSet& M) {
  return M.topo_builder == h->mesh_builder && (h->mesh_builder != PT_MESH_BUILDER_DEVICE || M.topo_kind == h->mesh_device_tree);
}

inline ptlbvh::Scratch mesh_scratch(const pt_context::MeshSet::DeviceBuild& D) {
  uint32_t* w = D.words;
  const size_t n = D.cap;
  return ptlbvh::Scratch{w, w + n, w + 2 * n, w + 3 * n, w + 4 * n, w + 5 * n, w + 6 * n, w + 7 * n, w + 9 * n};
}

// mesh m's world corner normals / uvs (triangle order) onto the device, where it has any
int upload_mesh_corners(pt_handle h, pt_context::MeshSet& M, size_t mesh) {
  const pt_context::MeshSet::One& m = M.mesh[mesh];
  pt_context::MeshSet::DeviceBuild& D = M.dev;
  if (!m.normals.empty() && D.corner && !m.normals_stale)   // (stale: the device holds the newer ones, pt_update_mesh_vertices)
    PT_HIP(hipMemcpy(D.corner + 9 * (size_t)m.tri_base, m.normals.data(), m.normals.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!m.uvs.empty() && D.corner_uv)
    PT_HIP(hipMemcpy(D.corner_uv + 6 * (size_t)m.tri_base, m.uvs.data(), m.uvs.size() * sizeof(float), hipMemcpyHostToDevice));
  return PT_OK;
}

// Everything the device paths need for the meshes of M, allocated and filled unless it is there already: the world frames, the
// triangle-order corner normals and uvs (where a mesh has them, or is about to: want_normals / want_uvs), and the builder's
// arrays for the largest mesh -- the SAH builder's too while that kind is in force, or about to be (want_sah).  A failed
// allocation leaves M with what it had (a part that did get allocated stays, unused).
int ensure_mesh_device(pt_handle h, pt_context::MeshSet& M, bool want_normals = false, bool want_uvs = false, bool want_sah = false) {
  PT_HIP(hipSetDevice(h->cfg.device));
  pt_context::MeshSet::DeviceBuild& D = M.dev;
  size_t total = 0, cap = 0;
  for (const pt_context::MeshSet::One& m : M.mesh) { total += m.n_triangles; cap = std::max<size_t>(cap, m.n_triangles); }
  const auto oom = [&](hipError_t e, size_t bytes) {
    return fail(h, hip_status(e), "mesh build storage: allocating " + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
  };
  hipError_t e;
  if (!D.world) {
    if ((e = dev_alloc(D.world, ptlbvh::kFrameFloats * total)) != hipSuccess) return oom(e, ptlbvh::kFrameFloats * total * 4);
    PT_HIP(hipMemcpy(D.world, M.world.data(), M.world.size() * sizeof(float), hipMemcpyHostToDevice));
    D.bytes += ptlbvh::kFrameFloats * total * 4;
  }
  if (!D.words) {
    const size_t sort_bytes = ptlbvh::sort_words((uint32_t)cap) * sizeof(uint32_t);
    DevBuf<uint64_t> code[2];
    DevBuf<uint32_t> index[2], words, stats;
    DevBuf<uint8_t> sort_tmp;
    const size_t n_words = (size_t)ptlbvh::kScratchWords * cap + 8;
    for (int k = 0; k < 2; ++k) {
      if ((e = dev_alloc(code[k], cap)) != hipSuccess) return oom(e, cap * 8);
      if ((e = dev_alloc(index[k], cap)) != hipSuccess) return oom(e, cap * 4);
    }
    if ((e = dev_alloc(words, n_words)) != hipSuccess) return oom(e, n_words * 4);
    if ((e = dev_alloc(stats, ptlbvh::kStats * M.mesh.size())) != hipSuccess) return oom(e, ptlbvh::kStats * M.mesh.size() * 4);
    if ((e = dev_alloc(sort_tmp, sort_bytes)) != hipSuccess) return oom(e, sort_bytes);
    for (int k = 0; k < 2; ++k) { D.code[k] = std::move(code[k]); D.index[k] = std::move(index[k]); }
    D.words = std::move(words); D.stats = std::move(stats); D.sort_tmp = std::move(sort_tmp);
    D.cap = cap;
    D.bytes += 2 * cap * 12 + n_words * 4 + ptlbvh::kStats * M.mesh.size() * 4 + sort_bytes;
  }
  if ((want_sah || h->mesh_device_tree == PT_MESH_DEVICE_TREE_SAH) && !D.sah_words) {
    const size_t words = ptsah::work_words((uint32_t)D.cap);
    if ((e = dev_alloc(D.sah_words, words)) != hipSuccess) return oom(e, words * 4);
    D.sah_bytes = words * 4;
  }
  bool fresh = false;
  if ((want_normals || M.smooth()) && !D.corner) {
    if ((e = dev_alloc(D.corner, 9 * total)) != hipSuccess) return oom(e, 9 * total * 4);
    D.bytes += 9 * total * 4;
    fresh = true;
  }
  if ((want_uvs || M.textured()) && !D.corner_uv) {
    if ((e = dev_alloc(D.corner_uv, 6 * total)) != hipSuccess) return oom(e, 6 * total * 4);
    D.bytes += 6 * total * 4;
    fresh = true;
  }
  if (fresh)
    for (size_t k = 0; k < M.mesh.size(); ++k)
      if (int rc = upload_mesh_corners(h, M, k)) return rc;
  if (!h->mesh_event[0])
    for (hipEvent_t& ev : h->mesh_event) PT_HIP(hipEventCreate(&ev));
  return PT_OK;
}

inline void note_mesh_pass(pt_handle h, int kind, double ms) {
  (kind == PT_MESH_LAST_HOST_BUILD ? h->mesh_host_builds : kind == PT_MESH_LAST_DEVICE_BUILD ? h->mesh_device_builds : h->mesh_refits) += 1;
  h->mesh_last_kind = kind;
  h->mesh_last_ms = ms;
}

// The box pass on mesh m's tree (skips, leaf words and slots in place), then its four words back to the host.
static int mesh_fit_and_read(pt_handle h, pt_context::MeshSet& M, size_t k, uint32_t threads, uint32_t* stats_host) {
  pt_context::MeshSet::One& m = M.mesh[k];
  const ptlbvh::Scratch S = mesh_scratch(M.dev);
  uint32_t* stats = M.dev.stats + ptlbvh::kStats * k;
  ptmesh::Node* nodes = M.d_nodes + m.node_base;
  const ptmesh::F4* tris = M.d_tris + 3 * (size_t)m.tri_base;
  const uint32_t grid = ptlbvh::blocks_for(threads);
  hipLaunchKernelGGL(ptlbvh::lbvh_box_leaf_kernel, dim3(grid), dim3(ptlbvh::kBlock), 0, h->stream, threads, nodes, tris, S, stats, ptlbvh::kPadScale);
  hipLaunchKernelGGL(ptlbvh::lbvh_box_climb_kernel, dim3(grid), dim3(ptlbvh::kBlock), 0, h->stream, threads, nodes, S, stats, ptlbvh::kPadScale);
  hipLaunchKernelGGL(ptlbvh::lbvh_pad_kernel, dim3(grid), dim3(ptlbvh::kBlock), 0, h->stream, threads, nodes, (const uint32_t*)stats);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpyAsync(stats_host, stats, ptlbvh::kStats * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipEventRecord(h->mesh_event[1], h->stream));
  PT_HIP(hipEventSynchronize(h->mesh_event[1]));
  float ms = 0.f;
  PT_HIP(hipEventElapsedTime(&ms, h->mesh_event[0], h->mesh_event[1]));
  m.build_ms = ms;
  if (stats_host[ptlbvh::kStatNodes] == 0 || stats_host[ptlbvh::kStatNodes] > 2 * m.n_triangles - 1)
    return fail(h, PT_ERR_HIP, "mesh builder (device): a tree of " + std::to_string(stats_host[ptlbvh::kStatNodes]) + " nodes over " + std::to_string(m.n_triangles) + " triangles");
  m.n_nodes = stats_host[ptlbvh::kStatNodes];
  m.depth = stats_host[ptlbvh::kStatDepth];
  m.max_leaf = stats_host[ptlbvh::kStatMaxLeaf];
  m.pad = ptlbvh::bits_float(stats_host[ptlbvh::kStatPad]);
  return PT_OK;
}

static void mesh_finish_pass(pt_context::MeshSet& M, const ptcamera::Basis* cam) {
  for (pt_context::MeshSet::One& m : M.mesh) {
    const ptd::MeshRow row{m.node_base, m.tri_base, m.n_nodes, m.n_triangles, m.normals.empty() ? 0u : 1u, m.uvs.empty() ? 0u : 1u};
    memcpy(&M.row[m.object_index], &row, sizeof(row));
  }
  M.built = true;
  M.built_world = cam == nullptr;
  if (cam) M.built_for = *cam;
}

static int drain_for_meshes(pt_handle h, pt_context::MeshSet& M) {
  PT_HIP(hipSetDevice(h->cfg.device));
  if (&M == &h->mesh)   // (a set that is not in force yet has no reader)
    for (hipStream_t s : {h->stream, h->trace_stream, h->acc_stream})
      if (s) PT_HIP(hipStreamSynchronize(s));
  return PT_OK;
}

// Mesh k of M built on the device in the frame of P, from the device copy of its world frames, on the handle's stream (drained
// by the caller).  No per-triangle data crosses to or from the host.
static int build_mesh_device(pt_handle h, pt_context::MeshSet& M, size_t k, const ptlbvh::Pose& P) {
  pt_context::MeshSet::DeviceBuild& D = M.dev;
  const ptlbvh::Scratch S = mesh_scratch(D);
  uint32_t* bounds = D.words + (size_t)ptlbvh::kScratchWords * D.cap;
  pt_context::MeshSet::One& m = M.mesh[k];
  const uint32_t T = m.n_triangles;
  if (T > D.cap) return fail(h, PT_ERR_HIP, "mesh builder (device): storage smaller than the mesh");   // (cannot happen)
  const float* world = D.world + ptlbvh::kFrameFloats * (size_t)m.tri_base;
  uint32_t* stats = D.stats + ptlbvh::kStats * k;
  const dim3 block(ptlbvh::kBlock), per_tri(ptlbvh::blocks_for(T)), per_node(ptlbvh::blocks_for(2 * T - 1));
  PT_HIP(hipEventRecord(h->mesh_event[0], h->stream));
  PT_HIP(hipMemsetAsync(bounds, 0xff, 3 * sizeof(uint32_t), h->stream));
  PT_HIP(hipMemsetAsync(bounds + 3, 0, 3 * sizeof(uint32_t), h->stream));
  PT_HIP(hipMemsetAsync(stats, 0, ptlbvh::kStats * sizeof(uint32_t), h->stream));
  hipLaunchKernelGGL(ptlbvh::lbvh_bounds_kernel, per_tri, block, 0, h->stream, world, T, P, bounds);
  hipLaunchKernelGGL(ptlbvh::lbvh_codes_kernel, per_tri, block, 0, h->stream, world, T, P, (const uint32_t*)bounds, (uint64_t*)D.code[0], (uint32_t*)D.index[0]);
  PT_HIP(hipGetLastError());
  {
    const uint32_t tiles = ptlbvh::sort_tiles(T);
    uint32_t* hist = reinterpret_cast<uint32_t*>((uint8_t*)D.sort_tmp);
    uint32_t* totals = hist + (size_t)ptlbvh::kSortDigits * tiles;
    for (uint32_t p = 0; p < ptlbvh::kSortPasses; ++p) {   // an even number of passes: the sorted pairs end in code[0], index[0]
      const uint64_t* kin = D.code[p & 1u];
      const uint32_t* vin = D.index[p & 1u];
      hipLaunchKernelGGL(ptlbvh::lbvh_sort_hist_kernel, dim3(tiles), block, 0, h->stream, kin, T, 8u * p, tiles, hist);
      hipLaunchKernelGGL(ptlbvh::lbvh_sort_scan_kernel, dim3(ptlbvh::kSortDigits), block, 0, h->stream, hist, tiles, totals);
      hipLaunchKernelGGL(ptlbvh::lbvh_sort_scatter_kernel, dim3(tiles), block, 0, h->stream, kin, vin, T, 8u * p, tiles, (const uint32_t*)hist,
                         (const uint32_t*)totals, (uint64_t*)D.code[(p + 1u) & 1u], (uint32_t*)D.index[(p + 1u) & 1u]);
    }
    PT_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(ptlbvh::lbvh_tree_kernel, per_tri, block, 0, h->stream, (const uint64_t*)D.code[0], T, S);
  hipLaunchKernelGGL(ptlbvh::lbvh_count_kernel, per_tri, block, 0, h->stream, T, S);
  hipLaunchKernelGGL(ptlbvh::lbvh_emit_kernel, per_node, block, 0, h->stream, T, S, M.d_nodes + m.node_base, stats);
  hipLaunchKernelGGL(ptlbvh::lbvh_slots_kernel, per_tri, block, 0, h->stream, T, (const uint32_t*)D.index[0], P, world,
                     m.normals.empty() ? (const float*)nullptr : (const float*)(D.corner + 9 * (size_t)m.tri_base),
                     m.uvs.empty() ? (const float*)nullptr : (const float*)(D.corner_uv + 6 * (size_t)m.tri_base),
                     M.d_tris + 3 * (size_t)m.tri_base, m.normals.empty() ? (ptmesh::F4*)nullptr : M.d_normals + 3 * (size_t)m.tri_base,
                     M.d_orig + m.tri_base, m.uvs.empty() ? (float*)nullptr : M.d_uvs + 6 * (size_t)m.tri_base);
  PT_HIP(hipGetLastError());
  uint32_t stats_host[ptlbvh::kStats] = {};
  return mesh_fit_and_read(h, M, k, 2 * T - 1, stats_host);
}

}  // (namespace: ptmi_mesh_sah.h opens its own)
#include "ptmi_mesh_sah.h"
namespace {

// build_meshes on the device: every mesh of M in the frame of `cam`, by the kind of tree in force.
int build_meshes_device(pt_handle h, pt_context::MeshSet& M, const ptcamera::Basis* cam) {
  if (int rc = drain_for_meshes(h, M)) return rc;
  M.built = false;
  M.topo_builder = -1;
  const ptlbvh::Pose P = ptlbvh::pose_of(cam);
  double total_ms = 0;
  for (size_t k = 0; k < M.mesh.size(); ++k) {
    if (int rc = build_mesh_device_of_kind(h, M, k, P)) return rc;
    total_ms += M.mesh[k].build_ms;
  }
  mesh_finish_pass(M, cam);
  M.topo_builder = PT_MESH_BUILDER_DEVICE;
  M.topo_kind = h->mesh_device_tree;
  note_mesh_pass(h, PT_MESH_LAST_DEVICE_BUILD, total_ms);
  note_sah_build(h, total_ms);
  return PT_OK;
}

// Mesh k of M refitted to the frame of P: topology, slot order and orig stand (whichever builder made them); the frames are
// formed again from the device copy of the world frames, the corner normals go through the direction transform into their slots,
// and the boxes and the pad follow.  uvs are not touched.
static int refit_mesh(pt_handle h, pt_context::MeshSet& M, size_t k, const ptlbvh::Pose& P) {
  pt_context::MeshSet::DeviceBuild& D = M.dev;
  pt_context::MeshSet::One& m = M.mesh[k];
  const uint32_t T = m.n_triangles;
  uint32_t* stats = D.stats + ptlbvh::kStats * k;
  uint32_t stats_host[ptlbvh::kStats] = {m.n_nodes, m.depth, m.max_leaf, 0u};
  PT_HIP(hipEventRecord(h->mesh_event[0], h->stream));
  PT_HIP(hipMemcpyAsync(stats, stats_host, sizeof(stats_host), hipMemcpyHostToDevice, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));   // (stats_host is written again below)
  hipLaunchKernelGGL(ptlbvh::lbvh_slots_kernel, dim3(ptlbvh::blocks_for(T)), dim3(ptlbvh::kBlock), 0, h->stream, T,
                     (const uint32_t*)(M.d_orig + m.tri_base), P, (const float*)(D.world + ptlbvh::kFrameFloats * (size_t)m.tri_base),
                     m.normals.empty() ? (const float*)nullptr : (const float*)(D.corner + 9 * (size_t)m.tri_base), (const float*)nullptr,
                     M.d_tris + 3 * (size_t)m.tri_base, m.normals.empty() ? (ptmesh::F4*)nullptr : M.d_normals + 3 * (size_t)m.tri_base,
                     (uint32_t*)nullptr, (float*)nullptr);
  PT_HIP(hipGetLastError());
  return mesh_fit_and_read(h, M, k, m.n_nodes, stats_host);
}

// A pose change under PT_MESH_POSE_REFIT: every mesh of M refitted to the frame of `cam`.
int refit_meshes(pt_handle h, pt_context::MeshSet& M, const ptcamera::Basis* cam) {
  if (int rc = drain_for_meshes(h, M)) return rc;
  M.built = false;
  const ptlbvh::Pose P = ptlbvh::pose_of(cam);
  double total_ms = 0;
  for (size_t k = 0; k < M.mesh.size(); ++k) {
    if (int rc = refit_mesh(h, M, k, P)) return rc;
    total_ms += M.mesh[k].build_ms;
  }
  mesh_finish_pass(M, cam);
  note_mesh_pass(h, PT_MESH_LAST_REFIT, total_ms);
  return PT_OK;
}

}  // namespace
