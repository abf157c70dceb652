// ptmi_mesh_sah.h -- SAH mesh trees built on the device (pt_set_mesh_device_tree, include/ptmi.h): the kernels, thin wrappers
// around the *_thread functions of pt_mesh_sah.h (ONE definition for the device, the host's thread-by-thread form and the test
// program), and the one-mesh body that stands beside build_mesh_device (ptmi_mesh_build.h, which includes this file).  The
// wrappers add only what cannot change a result: bounds_kernel reduces a wave that lies in one range by min / max before its
// first lane touches memory, bins_kernel keeps the bins of the workgroup's first range in LDS and flushes them with the same
// integer atomics, and the prefix sum of the goes-left flags is written here -- tile sums, a scan of the sums, and the partition
// adds the two (rocprim is not used: ptmi_mesh_build.h says why).  No kernel waits on another workgroup; a build allocates
// nothing; the host reads two words per level (the next level's open and large ranges) to size its launches and to know when
// to stop.
#pragma once
#include "pt_mesh_sah.h"

namespace ptsah {

constexpr uint32_t kBlock = ptlbvh::kBlock;
static_assert(kTile == 4u * kBlock, "four positions per thread of a tile");
using ptlbvh::blocks_for;

__global__ void sah_prep_kernel(uint32_t n, const float* __restrict__ world, ptlbvh::Pose P, Work W) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) prep_thread(i, n, world, P, W);
}
__global__ void sah_clear_kernel(uint32_t words, Work W) {
  const uint32_t w = blockIdx.x * kBlock + threadIdx.x;
  if (w < words) clear_thread(w, W);
}
__global__ void sah_bounds_kernel(uint32_t n, Work W, uint32_t parity) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  uint32_t tri = 0u, table = kNone;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n && large_position(i, W, parity, tri, table))
    for (int k = 0; k < 3; ++k) lo[k] = hi[k] = centre(W, tri, k);
  else table = kNone;
  const uint32_t first = __shfl(table, 0);
  if (__all(table == first)) {   // the whole wave in one range (or in none): one min / max per wave
    if (first == kNone) return;
    for (int m = warpSize / 2; m >= 1; m >>= 1)
      for (int k = 0; k < 3; ++k) { lo[k] = min2(lo[k], __shfl_xor(lo[k], m)); hi[k] = max2(hi[k], __shfl_xor(hi[k], m)); }
    if ((threadIdx.x & (warpSize - 1)) == 0) bounds_store(W.tables + (size_t)kLargeWords * first, lo, hi);
  } else if (table != kNone) {
    bounds_store(W.tables + (size_t)kLargeWords * table, lo, hi);
  }
}
__global__ void sah_bins_kernel(uint32_t n, Work W, uint32_t parity) {
  __shared__ uint32_t bins[kTableWords];
  __shared__ uint32_t own;
  const uint32_t t = threadIdx.x, i = blockIdx.x * kBlock + t;
  if (t == 0u) {   // the range of the workgroup's first position (blockIdx.x * kBlock < n: the grid is blocks_for(n))
    uint32_t tri, table;
    own = large_position(blockIdx.x * kBlock, W, parity, tri, table) ? table : kNone;
  }
  for (uint32_t w = t; w < kTableWords; w += kBlock) bins[w] = table_start(w);
  __syncthreads();
  const uint32_t mine = own;
  if (i < n) bin_thread(i, W, parity, bins, mine);
  __syncthreads();
  if (mine != kNone)
    for (uint32_t w = t; w < kTableWords; w += kBlock) flush_word(W.tables + (size_t)kLargeWords * mine + 6u, w, bins[w]);
}
__global__ void sah_split_kernel(uint32_t n_open, Work W, uint32_t parity, uint32_t depth, uint32_t max_depth, uint32_t next_base) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < n_open) split_thread(r, W, parity, depth, max_depth, next_base);
}
// workgroup t: tile t's flags, S = the flags before a position within the tile | its own flag, sums[t] = the tile's flags
__global__ void sah_flags_kernel(uint32_t n, Work W, uint32_t parity) {
  __shared__ uint32_t sums[kBlock];
  const uint32_t t = threadIdx.x, base = blockIdx.x * kTile + 4u * t;
  uint32_t f[4], mine = 0u;
  for (uint32_t q = 0; q < 4u; ++q) { f[q] = base + q < n ? flag_thread(base + q, W, parity) : 0u; mine += f[q]; }
  sums[t] = mine;
  __syncthreads();
  for (uint32_t off = 1u; off < kBlock; off <<= 1) {
    const uint32_t v = t >= off ? sums[t - off] : 0u;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint32_t run = sums[t] - mine;
  for (uint32_t q = 0; q < 4u; ++q)
    if (base + q < n) { W.S[base + q] = run | (f[q] ? kFlagBit : 0u); run += f[q]; }
  if (t == kBlock - 1u) W.sums[blockIdx.x] = sums[t];
}
// one workgroup: sums becomes its exclusive prefix sums
__global__ void sah_scan_sums_kernel(uint32_t tiles, Work W) {
  __shared__ uint32_t sums[kBlock];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (tiles + kBlock - 1u) / kBlock;
  const uint32_t begin = t * per < tiles ? t * per : tiles, end = begin + per < tiles ? begin + per : tiles;
  uint32_t mine = 0u;
  for (uint32_t i = begin; i < end; ++i) mine += W.sums[i];
  sums[t] = mine;
  __syncthreads();
  for (uint32_t off = 1u; off < kBlock; off <<= 1) {
    const uint32_t v = t >= off ? sums[t - off] : 0u;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint32_t run = sums[t] - mine;
  for (uint32_t i = begin; i < end; ++i) { const uint32_t x = W.sums[i]; W.sums[i] = run; run += x; }
}
__global__ void sah_partition_kernel(uint32_t n, Work W, uint32_t parity) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) partition_thread(i, n, W, parity);
}
__global__ void sah_count_kernel(uint32_t n_nodes, Work W) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k < n_nodes) count_thread(k, W);
}
__global__ void sah_emit_kernel(uint32_t n_nodes, Work W, Node* nodes, uint32_t* stats) {
  const uint32_t k = blockIdx.x * kBlock + threadIdx.x;
  if (k < n_nodes) emit_thread(k, n_nodes, W, nodes, stats);
}

}  // namespace ptsah

// ---- the handle's side
namespace {

// Mesh k of M built by binned SAH on the device in the frame of P: ptmesh::build's tree of the same kernel-frame triangles, byte
// for byte.  On the handle's stream (drained by the caller); no per-triangle data crosses to or from the host.
static int build_mesh_device_sah(pt_handle h, pt_context::MeshSet& M, size_t k, const ptlbvh::Pose& P) {
  pt_context::MeshSet::DeviceBuild& D = M.dev;
  pt_context::MeshSet::One& m = M.mesh[k];
  const uint32_t T = m.n_triangles;
  if (T > D.cap || !D.sah_words || D.sah_words.count() < ptsah::work_words((uint32_t)D.cap))
    return fail(h, PT_ERR_HIP, "mesh builder (device, SAH): storage smaller than the mesh");   // (cannot happen)
  const ptsah::Work W = ptsah::work_view(D.sah_words, T);
  const float* world = D.world + ptlbvh::kFrameFloats * (size_t)m.tri_base;
  uint32_t* stats = D.stats + ptlbvh::kStats * k;
  const dim3 block(ptsah::kBlock), per_tri(ptsah::blocks_for(T));
  const uint32_t tiles = ptsah::tiles_for(T);
  hipStream_t s = h->stream;
  PT_HIP(hipEventRecord(h->mesh_event[0], s));
  PT_HIP(hipMemsetAsync(stats, 0, ptlbvh::kStats * sizeof(uint32_t), s));
  hipLaunchKernelGGL(ptsah::sah_prep_kernel, per_tri, block, 0, s, T, world, P, W);
  PT_HIP(hipGetLastError());
  uint32_t n_open = T > ptmesh::kMaxLeaf ? 1u : 0u, n_large = T > ptsah::kSeq ? 1u : 0u, parity = 0u, level = 0u, next_base = 1u;
  while (n_open) {
    if (level >= ptsah::kMaxLevels || n_open > W.cap_open || n_large > W.cap_large || (uint64_t)next_base + 2ull * n_open > 2ull * T - 1ull)
      return fail(h, PT_ERR_HIP, "mesh builder (device, SAH): level " + std::to_string(level) + " with " + std::to_string(n_open) + " open ranges over " +
                                     std::to_string(T) + " triangles");   // (cannot happen)
    if (n_large) {
      const uint32_t words = n_large * ptsah::kLargeWords;
      hipLaunchKernelGGL(ptsah::sah_clear_kernel, dim3(ptsah::blocks_for(words)), block, 0, s, words, W);
      hipLaunchKernelGGL(ptsah::sah_bounds_kernel, per_tri, block, 0, s, T, W, parity);
      hipLaunchKernelGGL(ptsah::sah_bins_kernel, per_tri, block, 0, s, T, W, parity);
    }
    uint32_t* next_ctr = W.ctr + 2u * (parity ^ 1u);
    PT_HIP(hipMemsetAsync(next_ctr, 0, 2 * sizeof(uint32_t), s));
    hipLaunchKernelGGL(ptsah::sah_split_kernel, dim3(ptsah::blocks_for(n_open)), block, 0, s, n_open, W, parity, level + 1u, ptsah::kMaxDepthSah, next_base);
    hipLaunchKernelGGL(ptsah::sah_flags_kernel, dim3(tiles), block, 0, s, T, W, parity);
    hipLaunchKernelGGL(ptsah::sah_scan_sums_kernel, dim3(1), block, 0, s, tiles, W);
    hipLaunchKernelGGL(ptsah::sah_partition_kernel, per_tri, block, 0, s, T, W, parity);
    PT_HIP(hipGetLastError());
    uint32_t next[2] = {0u, 0u};   // the one small read per level: how many ranges the next level holds
    PT_HIP(hipMemcpyAsync(next, next_ctr, sizeof(next), hipMemcpyDeviceToHost, s));
    PT_HIP(hipStreamSynchronize(s));
    next_base += 2u * n_open;
    n_open = next[0]; n_large = next[1];
    parity ^= 1u;
    level += 1u;
  }
  uint32_t error = 0u;
  const dim3 per_node(ptsah::blocks_for(next_base));
  hipLaunchKernelGGL(ptsah::sah_count_kernel, per_node, block, 0, s, next_base, W);
  hipLaunchKernelGGL(ptsah::sah_emit_kernel, per_node, block, 0, s, next_base, W, M.d_nodes + m.node_base, stats);
  hipLaunchKernelGGL(ptlbvh::lbvh_slots_kernel, per_tri, block, 0, s, T, (const uint32_t*)W.idx[parity], P, world,
                     m.normals.empty() ? (const float*)nullptr : (const float*)(D.corner + 9 * (size_t)m.tri_base),
                     m.uvs.empty() ? (const float*)nullptr : (const float*)(D.corner_uv + 6 * (size_t)m.tri_base),
                     M.d_tris + 3 * (size_t)m.tri_base, m.normals.empty() ? (ptmesh::F4*)nullptr : M.d_normals + 3 * (size_t)m.tri_base,
                     M.d_orig + m.tri_base, m.uvs.empty() ? (float*)nullptr : M.d_uvs + 6 * (size_t)m.tri_base);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpyAsync(&error, W.ctr + ptsah::kCtrError, sizeof(error), hipMemcpyDeviceToHost, s));
  uint32_t stats_host[ptlbvh::kStats] = {};
  if (int rc = mesh_fit_and_read(h, M, k, next_base, stats_host)) return rc;
  if (error || stats_host[ptlbvh::kStatNodes] != next_base)
    return fail(h, PT_ERR_HIP, "mesh builder (device, SAH): " + std::to_string(stats_host[ptlbvh::kStatNodes]) + " nodes emitted of " + std::to_string(next_base));
  h->mesh_sah_last_levels = level;
  return PT_OK;
}

// Mesh k by the device builder's kind in force (pt_set_mesh_device_tree).
static int build_mesh_device_of_kind(pt_handle h, pt_context::MeshSet& M, size_t k, const ptlbvh::Pose& P) {
  return h->mesh_device_tree == PT_MESH_DEVICE_TREE_SAH ? build_mesh_device_sah(h, M, k, P) : build_mesh_device(h, M, k, P);
}
// A device build pass under the SAH kind counts in pt_mesh_device_tree_info as well.
inline void note_sah_build(pt_handle h, double ms) {
  if (h->mesh_device_tree != PT_MESH_DEVICE_TREE_SAH) return;
  h->mesh_sah_builds += 1;
  h->mesh_sah_last_ms = ms;
}

}  // namespace
