// pt_mesh_sah.h -- the binned-SAH builder of ptmi_mesh.h (ptmesh::Builder) in a parallel form (pt_set_mesh_device_tree,
// include/ptmi.h), written ONCE for the kernels and for the host: the functions behind PT_MESH_HD hold no HIP type, so
// tests/mesh_sah_main.cpp compiles them with g++ alone.  Compile with -ffp-contract=off like everything else here: every operation
// below is one rounded binary32.
//
// THE RULE is ptmesh::Builder's, and "the same tree" means its bytes:
//   * a triangle's box is ptmesh::tri_box's, its centroid 0.5f * (lo + hi) per axis;
//   * a range of at most kMaxLeaf triangles is a leaf; a larger one at depth < max_depth (the root has depth 1; kMaxDepthSah = 48
//     in the library -- 48 levels are out of reach of small valid fixtures in binary32, so the cap is a parameter and the test
//     program exercises it at 2 and 3) looks for a split: over the centroids' bounds cb of the range, for the axes 0, 1, 2 in
//     this order with ext = cb.hi - cb.lo > 0 and finite, the triangles fall into kBins bins by bin_of; a right-to-left scan
//     gives every split's right box and count, a left-to-right scan its left ones, splits with an empty side are skipped, the
//     cost is half_area(left) * (float)n_left + half_area(right) * (float)n_right and a split wins by strict <, so the first of
//     equal costs stands (scan_axis);
//   * the range is partitioned STABLY by bin_of(...) < the winning bin; where no axis offers a split, or at the depth cap, the
//     range is halved as it lies (the first count / 2 positions go left);
//   * layout, boxes and pad are ptmi_mesh.h's, by the box pass of pt_mesh_build.h.
// Every reduction is a min / max or an integer count, so it is exact in any order; nothing else is reduced.
//
// THE PARALLEL FORM builds breadth-first over the open ranges of one index array.  Nodes are numbered in creation order: the
// children of the r-th open range of a level are nodes base + 2 r and base + 2 r + 1 of the next, so numbering needs no atomic;
// which slot of the next level's open list a child takes is decided by an integer counter, and nothing depends on it.  A level:
//   bounds_thread     position i of a LARGE open range (more than kSeq triangles): its centroid into the range's bounds
//   bin_thread        position i of a large open range: its box into 3 x kBins bins of the range (count; min / max words)
//   split_thread      open range r: the scans over its bins -- a small range bins its triangles itself, in registers --, then
//                     its two children: their ranges, and for a child that stays open its slot in the next level's lists
//   flag_thread       position i: does it go left; a prefix sum over the whole array follows (tile sums, a scan of the sums)
//   partition_thread  position i to b + (S[i] - S[b]) or mid + (i - b) - (S[i] - S[b]) of the other index array
// When no range is open the index array is the slot order (the host emits leaves depth-first, left to right).  count_thread
// climbs from every leaf over arrival counters and gives each node its subtree's node count; emit_thread walks to the root for a
// node's depth-first index (+ 1 for a left turn, + 1 + count(left sibling) for a right turn), its skip and its leaf word.  Slots,
// boxes and pad are pt_mesh_build.h's slot_thread, box_leaf_thread, box_climb_thread and pad_thread.
#pragma once
#include <cmath>
#include <cstdint>

#include "pt_mesh.h"
#include "pt_mesh_build.h"

namespace ptsah {

using ptlbvh::kNone;
using ptlbvh::max2;
using ptlbvh::min2;
using ptmesh::Node;

constexpr int kBins = 16;                   // = ptmesh::kBins
constexpr uint32_t kMaxDepthSah = 48;       // = ptmesh::kMaxDepthSah
constexpr uint32_t kSeq = 32;               // a range of at most kSeq triangles is binned by its split thread alone
constexpr uint32_t kBinWords = 7;           // count, lo[3], hi[3] (floats as order-preserving words)
constexpr uint32_t kTableWords = 3 * kBins * kBinWords;   // 336 words = 1344 bytes
constexpr uint32_t kLargeWords = 6 + kTableWords;         // a large range's centroid bounds (lo[3], hi[3]), then its bins
constexpr uint32_t kTileShift = 10, kTile = 1u << kTileShift;   // the prefix sum's tile
constexpr uint32_t kFlagBit = 0x80000000u;
constexpr uint32_t kMaxLevels = 96;         // depth cap + log2(PT_MAX_MESH_TRIANGLES) halvings, with room
enum { kCtrOpen = 0, kCtrLarge = 1, kCtrError = 4, kCtrWords = 8 };   // ctr[2 * parity + ...]: the level's open / large ranges

// float <-> a word whose unsigned order is the float's order
PT_MESH_HD uint32_t ordered(float f) { const uint32_t u = ptlbvh::float_bits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
PT_MESH_HD float unordered(uint32_t u) { return ptlbvh::bits_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// The only reductions: integer min / max / add on a word (LDS or global on the device).
PT_MESH_HD void word_min(uint32_t* w, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(w, v);
#else
  if (v < *w) *w = v;
#endif
}
PT_MESH_HD void word_max(uint32_t* w, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(w, v);
#else
  if (v > *w) *w = v;
#endif
}
PT_MESH_HD uint32_t word_add(uint32_t* w, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicAdd(w, v);
#else
  const uint32_t before = *w;
  *w += v;
  return before;
#endif
}

// ---- the per-range arithmetic, expression for expression ptmesh::Builder's
PT_MESH_HD int bin_of(float c, float lo, float ext) {
  const int k = (int)((float)kBins * ((c - lo) / ext));
  return k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
}
PT_MESH_HD float half_area(const float* lo, const float* hi) {
  const float x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
  return ((x * y) + (y * z)) + (z * x);
}
PT_MESH_HD void grow_point(float* lo, float* hi, const float* p) {   // ptmesh::Box::grow(const float*)
  for (int k = 0; k < 3; ++k) { lo[k] = min2(lo[k], p[k]); hi[k] = max2(hi[k], p[k]); }
}
PT_MESH_HD void grow_box(float* lo, float* hi, const float* blo, const float* bhi) { grow_point(lo, hi, blo); grow_point(lo, hi, bhi); }
PT_MESH_HD void clear_box(float* lo, float* hi) { for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; } }
PT_MESH_HD bool axis_splits(float ext) { return ext > 0.f && ext < INFINITY; }   // !( !(ext > 0) || !isfinite(ext) )

struct Split {
  float cost = INFINITY;
  int32_t axis = -1;
  uint32_t bin = 0, left = 0;   // bins < bin go left: `left` triangles
  float lo = 0.f, ext = 0.f;    // of the winning axis: what bin_of takes
};
// One axis' bins (count, box; an empty bin's box is never read): the two scans.  lo, ext: the centroid bounds of that axis.
PT_MESH_HD void scan_axis(int axis, const uint32_t* bin_n, const float (*bin_lo)[3], const float (*bin_hi)[3], float lo, float ext, Split& best) {
  float right_area[kBins];
  uint32_t right_n[kBins];
  float alo[3], ahi[3];
  clear_box(alo, ahi);
  uint32_t cnt = 0;
  for (int k = kBins - 1; k > 0; --k) {
    if (bin_n[k]) grow_box(alo, ahi, bin_lo[k], bin_hi[k]);
    cnt += bin_n[k];
    right_area[k] = cnt ? half_area(alo, ahi) : 0.f;
    right_n[k] = cnt;
  }
  clear_box(alo, ahi);
  cnt = 0;
  for (int k = 1; k < kBins; ++k) {   // split: bins < k to the left
    if (bin_n[k - 1]) grow_box(alo, ahi, bin_lo[k - 1], bin_hi[k - 1]);
    cnt += bin_n[k - 1];
    if (cnt == 0 || right_n[k] == 0) continue;
    const float cost = half_area(alo, ahi) * (float)cnt + right_area[k] * (float)right_n[k];
#if defined(PT_SAH_MUTATE_LE)   // (tests/mesh_sah_main.cpp: the mutation must fail the test)
    if (cost <= best.cost) {
#else
    if (cost < best.cost) {
#endif
      best.cost = cost; best.axis = axis; best.bin = (uint32_t)k; best.left = cnt; best.lo = lo; best.ext = ext;
    }
  }
}

// ---- the arrays of one build, every one sized for T triangles (work_words(T) words in all)
struct Work {
  uint32_t cap_open, cap_large;
  float* box;                  // [T][6]   the triangles' boxes in the frame to build in, triangle order
  uint32_t* idx[2];            // [T]      the index array, this level's and the next's
  uint32_t* rid[2];            // [T]      position -> its range's slot in the level's open list (kNone: in a leaf)
  uint32_t* S;                 // [T]      goes-left flags before position i within its tile | its own flag << 31
  uint32_t* sums;              // [tiles]  goes-left flags before the tile
  uint32_t *nb, *ne;           // [2T]     node -> its range [nb, ne)                            (nodes in creation order)
  uint32_t *nparent, *nleft;   // [2T]     its parent (kNone: the root), its left child (kNone: a leaf; the right one is + 1)
  uint32_t *ncount, *ncounter; // [2T]     nodes of its subtree, arrivals (count_thread)
  uint32_t* open[2];           // [cap_open]  open slot -> node
  uint32_t* large[2];          // [cap_open]  open slot -> its table in `tables` (kNone: at most kSeq triangles)
  int32_t* sp_axis;            // [cap_open]  the split of the level's open slot: axis (-1: halved), bin, the right part's first
  uint32_t *sp_bin, *sp_mid;   //             position, the winning axis' lo and ext, and the children's open slots in the next
  float *sp_lo, *sp_ext;       //             level (kNone: a leaf)
  uint32_t* sp_child[2];
  uint32_t* tables;            // [cap_large][kLargeWords]
  uint32_t* ctr;               // [kCtrWords]
};
inline uint32_t cap_open(uint32_t T) { return T / (ptmesh::kMaxLeaf + 1u) + 1u; }   // open ranges are disjoint, more than kMaxLeaf each
inline uint32_t cap_large(uint32_t T) { return T / (kSeq + 1u) + 1u; }
inline uint32_t tiles_for(uint32_t T) { return (T + kTile - 1u) >> kTileShift; }
inline size_t work_words(uint32_t T) {
  return 6 * (size_t)T + 5 * (size_t)T + tiles_for(T) + 12 * (size_t)T + 11 * (size_t)cap_open(T) + (size_t)kLargeWords * cap_large(T) + kCtrWords;
}
inline Work work_view(uint32_t* base, uint32_t T) {
  Work W{};
  W.cap_open = cap_open(T); W.cap_large = cap_large(T);
  uint32_t* w = base;
  const auto take = [&](size_t words) { uint32_t* p = w; w += words; return p; };
  W.box = reinterpret_cast<float*>(take(6 * (size_t)T));
  for (int k = 0; k < 2; ++k) W.idx[k] = take(T);
  for (int k = 0; k < 2; ++k) W.rid[k] = take(T);
  W.S = take(T);
  W.sums = take(tiles_for(T));
  W.nb = take(2 * (size_t)T); W.ne = take(2 * (size_t)T); W.nparent = take(2 * (size_t)T); W.nleft = take(2 * (size_t)T);
  W.ncount = take(2 * (size_t)T); W.ncounter = take(2 * (size_t)T);
  for (int k = 0; k < 2; ++k) W.open[k] = take(W.cap_open);
  for (int k = 0; k < 2; ++k) W.large[k] = take(W.cap_open);
  W.sp_axis = reinterpret_cast<int32_t*>(take(W.cap_open));
  W.sp_bin = take(W.cap_open); W.sp_mid = take(W.cap_open);
  W.sp_lo = reinterpret_cast<float*>(take(W.cap_open)); W.sp_ext = reinterpret_cast<float*>(take(W.cap_open));
  for (int k = 0; k < 2; ++k) W.sp_child[k] = take(W.cap_open);
  W.tables = take((size_t)kLargeWords * W.cap_large);
  W.ctr = take(kCtrWords);
  return W;
}

PT_MESH_HD float centre(const Work& W, uint32_t tri, int axis) { return 0.5f * (W.box[6u * (size_t)tri + axis] + W.box[6u * (size_t)tri + 3 + axis]); }
// What a word of a large range's kLargeWords starts as: bounds lo / hi, then per bin count, lo[3], hi[3].
PT_MESH_HD uint32_t table_start(uint32_t w) { return w % kBinWords == 0u ? 0u : (w % kBinWords <= 3u ? 0xffffffffu : 0u); }
PT_MESH_HD uint32_t large_start(uint32_t w) { return w < 3u ? 0xffffffffu : (w < 6u ? 0u : table_start(w - 6u)); }

// thread i of T, once per build: triangle i's box in the frame of P, the index array, and (thread 0) the root.  world: the
// mesh's frames in triangle order.
PT_MESH_HD void prep_thread(uint32_t i, uint32_t T, const float* world, const ptlbvh::Pose& P, const Work& W) {
  float fr[ptlbvh::kFrameFloats];
  ptlbvh::kernel_frame(P, world + (size_t)ptlbvh::kFrameFloats * i, fr);
  ptlbvh::tri_box(fr, W.box + 6u * (size_t)i, W.box + 6u * (size_t)i + 3);
  const bool open = T > ptmesh::kMaxLeaf;
  W.idx[0][i] = i;
  W.rid[0][i] = open ? 0u : kNone;
  if (i != 0u) return;
  W.nb[0] = 0u; W.ne[0] = T; W.nparent[0] = kNone; W.nleft[0] = kNone; W.ncount[0] = 1u; W.ncounter[0] = 0u;
  W.open[0][0] = 0u;
  W.large[0][0] = T > kSeq ? 0u : kNone;
  for (uint32_t k = 0; k < kCtrWords; ++k) W.ctr[k] = 0u;
  W.ctr[kCtrOpen] = open ? 1u : 0u;
  W.ctr[kCtrLarge] = T > kSeq ? 1u : 0u;
}
// thread w of n_large * kLargeWords: the level's tables as they start
PT_MESH_HD void clear_thread(uint32_t w, const Work& W) { W.tables[w] = large_start(w % kLargeWords); }

// Position i of the level: its triangle and its range's table (false: not in a large open range).
PT_MESH_HD bool large_position(uint32_t i, const Work& W, uint32_t parity, uint32_t& tri, uint32_t& table) {
  const uint32_t r = W.rid[parity][i];
  if (r == kNone) return false;
  table = W.large[parity][r];
  if (table == kNone || table >= W.cap_large) return false;
  tri = W.idx[parity][i];
  return true;
}
PT_MESH_HD void bounds_store(uint32_t* words, const float* lo, const float* hi) {
  for (int k = 0; k < 3; ++k) { word_min(&words[k], ordered(lo[k])); word_max(&words[3 + k], ordered(hi[k])); }
}
PT_MESH_HD void bounds_thread(uint32_t i, const Work& W, uint32_t parity) {
  uint32_t tri, table;
  if (!large_position(i, W, parity, tri, table)) return;
  const float c[3] = {centre(W, tri, 0), centre(W, tri, 1), centre(W, tri, 2)};
  bounds_store(W.tables + (size_t)kLargeWords * table, c, c);
}
// own / own_table: a private copy of table `own`'s bins (a workgroup's, in LDS), flushed by the caller; kNone: none
PT_MESH_HD void bin_thread(uint32_t i, const Work& W, uint32_t parity, uint32_t* own_table, uint32_t own) {
  uint32_t tri, table;
  if (!large_position(i, W, parity, tri, table)) return;
  const uint32_t* cb = W.tables + (size_t)kLargeWords * table;
  uint32_t* bins = table == own ? own_table : W.tables + (size_t)kLargeWords * table + 6u;
  const float* b = W.box + 6u * (size_t)tri;
  for (int axis = 0; axis < 3; ++axis) {
    const float lo = unordered(cb[axis]), ext = unordered(cb[3 + axis]) - lo;
    if (!axis_splits(ext)) continue;
    uint32_t* t = bins + (size_t)kBinWords * (axis * kBins + bin_of(centre(W, tri, axis), lo, ext));
    word_add(&t[0], 1u);
    for (int q = 0; q < 3; ++q) { word_min(&t[1 + q], ordered(b[q])); word_max(&t[4 + q], ordered(b[3 + q])); }
  }
}
// word w of a private table into the range's own: what it holds beyond its start
PT_MESH_HD void flush_word(uint32_t* bins, uint32_t w, uint32_t v) {
  if (v == table_start(w)) return;
  const uint32_t q = w % kBinWords;
  if (q == 0u) word_add(&bins[w], v); else if (q <= 3u) word_min(&bins[w], v); else word_max(&bins[w], v);
}

// The split of idx[b, e) by its own triangles alone (a range of at most kSeq): ptmesh::Builder::sah_split up to the partition.
PT_MESH_HD void choose_alone(const Work& W, const uint32_t* idx, uint32_t b, uint32_t e, Split& best) {
  float clo[3], chi[3];
  clear_box(clo, chi);
  for (uint32_t i = b; i < e; ++i) {
    const float c[3] = {centre(W, idx[i], 0), centre(W, idx[i], 1), centre(W, idx[i], 2)};
    grow_point(clo, chi, c);
  }
  for (int axis = 0; axis < 3; ++axis) {
    const float ext = chi[axis] - clo[axis];
    if (!axis_splits(ext)) continue;
    float bin_lo[kBins][3], bin_hi[kBins][3];
    uint32_t bin_n[kBins];
    for (int k = 0; k < kBins; ++k) { clear_box(bin_lo[k], bin_hi[k]); bin_n[k] = 0u; }
    for (uint32_t i = b; i < e; ++i) {
      const int k = bin_of(centre(W, idx[i], axis), clo[axis], ext);
      const float* bx = W.box + 6u * (size_t)idx[i];
      grow_box(bin_lo[k], bin_hi[k], bx, bx + 3);
      bin_n[k] += 1u;
    }
    scan_axis(axis, bin_n, bin_lo, bin_hi, clo[axis], ext, best);
  }
}
// The split of a large range from its table.
PT_MESH_HD void choose_table(const uint32_t* words, Split& best) {
  for (int axis = 0; axis < 3; ++axis) {
    const float lo = unordered(words[axis]), ext = unordered(words[3 + axis]) - lo;
    if (!axis_splits(ext)) continue;
    float bin_lo[kBins][3], bin_hi[kBins][3];
    uint32_t bin_n[kBins];
    for (int k = 0; k < kBins; ++k) {
      const uint32_t* t = words + 6u + (size_t)kBinWords * (axis * kBins + k);
      bin_n[k] = t[0];
      for (int q = 0; q < 3; ++q) { bin_lo[k][q] = unordered(t[1 + q]); bin_hi[k][q] = unordered(t[4 + q]); }
    }
    scan_axis(axis, bin_n, bin_lo, bin_hi, lo, ext, best);
  }
}
// thread r of the level's open ranges.  depth: of the level's nodes (the root's is 1); next_base: the next level's first node.
PT_MESH_HD void split_thread(uint32_t r, const Work& W, uint32_t parity, uint32_t depth, uint32_t max_depth, uint32_t next_base) {
  const uint32_t n = W.open[parity][r], b = W.nb[n], e = W.ne[n], count = e - b;
  Split s;
  if (depth < max_depth) {
    const uint32_t table = W.large[parity][r];
    if (table == kNone) choose_alone(W, W.idx[parity], b, e, s);
    else choose_table(W.tables + (size_t)kLargeWords * table, s);
  }
  if (s.axis < 0 || s.left == 0u || s.left >= count) { s.axis = -1; s.left = count / 2u; }   // no split by SAH: halve the range as it lies
  const uint32_t mid = b + s.left, child = next_base + 2u * r, next = parity ^ 1u;
  W.nleft[n] = child;
  for (uint32_t side = 0; side < 2u; ++side) {
    const uint32_t c = child + side, cb = side ? mid : b, ce = side ? e : mid;
    W.nb[c] = cb; W.ne[c] = ce; W.nparent[c] = n; W.nleft[c] = kNone; W.ncount[c] = 1u; W.ncounter[c] = 0u;
    uint32_t slot = kNone;
    if (ce - cb > ptmesh::kMaxLeaf) {
      slot = word_add(&W.ctr[2u * next + kCtrOpen], 1u);
      if (slot >= W.cap_open) { W.ctr[kCtrError] = 1u; slot = kNone; }   // (cannot happen: open ranges are disjoint)
      else {
        W.open[next][slot] = c;
        uint32_t table = kNone;
        if (ce - cb > kSeq) {
          table = word_add(&W.ctr[2u * next + kCtrLarge], 1u);
          if (table >= W.cap_large) { W.ctr[kCtrError] = 1u; table = kNone; }
        }
        W.large[next][slot] = table;
      }
    }
    W.sp_child[side][r] = slot;
  }
  W.sp_axis[r] = s.axis; W.sp_bin[r] = s.bin; W.sp_mid[r] = mid; W.sp_lo[r] = s.lo; W.sp_ext[r] = s.ext;
}
// position i: 1 if it goes to the left part of its range
PT_MESH_HD uint32_t flag_thread(uint32_t i, const Work& W, uint32_t parity) {
  const uint32_t r = W.rid[parity][i];
  if (r == kNone) return 0u;
  const int32_t axis = W.sp_axis[r];
  if (axis < 0) return i < W.sp_mid[r] ? 1u : 0u;
  return (uint32_t)bin_of(centre(W, W.idx[parity][i], axis), W.sp_lo[r], W.sp_ext[r]) < W.sp_bin[r] ? 1u : 0u;
}
PT_MESH_HD uint32_t flags_before(const Work& W, uint32_t i) { return (W.S[i] & ~kFlagBit) + W.sums[i >> kTileShift]; }
// position i of T into the other index array: the stable partition of its range
PT_MESH_HD void partition_thread(uint32_t i, uint32_t T, const Work& W, uint32_t parity) {
  const uint32_t r = W.rid[parity][i], next = parity ^ 1u;
  if (r == kNone) { W.idx[next][i] = W.idx[parity][i]; W.rid[next][i] = kNone; return; }
  const uint32_t n = W.open[parity][r], b = W.nb[n], mid = W.sp_mid[r];
  const bool left = (W.S[i] & kFlagBit) != 0u;
  const uint32_t before = flags_before(W, i) - flags_before(W, b);
#if defined(PT_SAH_MUTATE_UNSTABLE)   // (tests/mesh_sah_main.cpp: the right part reversed must fail the test)
  const uint32_t to = left ? b + before : W.ne[n] - 1u - ((i - b) - before);
#else
  const uint32_t to = left ? b + before : mid + (i - b) - before;
#endif
  if (to >= T) { W.ctr[kCtrError] = 1u; return; }   // (cannot happen: the flags counted these very positions)
  W.idx[next][to] = W.idx[parity][i];
  W.rid[next][to] = W.sp_child[left ? 0 : 1][r];
}
// thread n of the tree's nodes: from a leaf upwards, every node's subtree count
PT_MESH_HD void count_thread(uint32_t n, const Work& W) {
  if (W.nleft[n] != kNone) return;
  uint32_t p = W.nparent[n];
  while (p != kNone) {
    if (ptlbvh::arrive(&W.ncounter[p]) == 0u) return;
    const uint32_t l = W.nleft[p];
    W.ncount[p] = 1u + W.ncount[l] + W.ncount[l + 1u];
    p = W.nparent[p];
  }
}
// thread n of the tree's n_nodes nodes: skip and leaf word at its depth-first index.  stats: zeroed before the launch.
PT_MESH_HD void emit_thread(uint32_t n, uint32_t n_nodes, const Work& W, Node* nodes, uint32_t* stats) {
  uint32_t index = 0u, depth = 1u, cur = n, p = W.nparent[n];
  while (p != kNone) {
    const uint32_t l = W.nleft[p];
    index += cur == l ? 1u : 1u + W.ncount[l];
    depth += 1u;
    cur = p;
    p = W.nparent[p];
  }
  if (index >= n_nodes) { W.ctr[kCtrError] = 1u; return; }   // (cannot happen: the counts are those of this very tree)
  const bool leaf = W.nleft[n] == kNone;
  const uint32_t count = W.ne[n] - W.nb[n];
  nodes[index].skip = index + W.ncount[n];
  nodes[index].leaf = leaf ? (W.nb[n] << ptmesh::kLeafCountBits | count) : 0u;
  ptlbvh::stat_max(&stats[ptlbvh::kStatDepth], depth);
  if (leaf) ptlbvh::stat_max(&stats[ptlbvh::kStatMaxLeaf], count);
  if (n == 0u) stats[ptlbvh::kStatNodes] = W.ncount[0];
}

}  // namespace ptsah

// ---- the host: the parallel form run thread by thread
namespace ptsah {

static_assert(kBins == ptmesh::kBins && kMaxDepthSah == ptmesh::kMaxDepthSah, "one rule for both builders");

// The prefix sum of a level's flags as the kernels lay it out: within each tile, then over the tiles' sums.
inline void scan_flags_host(uint32_t T, const Work& W, uint32_t parity, bool reverse) {
  const uint32_t tiles = tiles_for(T);
  std::vector<uint32_t> flag(T);
  for (uint32_t k = 0; k < T; ++k) { const uint32_t i = reverse ? T - 1u - k : k; flag[i] = flag_thread(i, W, parity); }
  for (uint32_t t = 0; t < tiles; ++t) {
    uint32_t run = 0u;
    for (uint32_t i = t << kTileShift; i < T && i < (t + 1u) << kTileShift; ++i) { W.S[i] = run | (flag[i] ? kFlagBit : 0u); run += flag[i]; }
    W.sums[t] = run;
  }
  uint32_t run = 0u;
  for (uint32_t t = 0; t < tiles; ++t) { const uint32_t x = W.sums[t]; W.sums[t] = run; run += x; }
}

// ptmesh::build's tree of n frames by the parallel form, every kernel's threads one after the other in index order (reverse: in
// reversed order, so every atomic arrives the other way round).  levels: the breadth-first levels it ran.
inline bool build_threads(const float* frames, uint32_t n, ptmesh::Built& out, float pad_scale = ptlbvh::kPadScale,
                          uint32_t max_depth = kMaxDepthSah, bool reverse = false, uint32_t* levels = nullptr) {
  out = ptmesh::Built{};
  std::vector<uint32_t> words(work_words(n), 0u);
  const Work W = work_view(words.data(), n);
  const auto each = [&](uint32_t threads, auto&& f) {
    for (uint32_t k = 0; k < threads; ++k) f(reverse ? threads - 1u - k : k);
  };
  const ptlbvh::Pose world{};
  each(n, [&](uint32_t i) { prep_thread(i, n, frames, world, W); });
  uint32_t parity = 0u, level = 0u, next_base = 1u;
  while (W.ctr[2u * parity + kCtrOpen] != 0u) {
    if (level >= kMaxLevels) return false;
    const uint32_t n_open = W.ctr[2u * parity + kCtrOpen], n_large = W.ctr[2u * parity + kCtrLarge];
    if (n_large) {
      each(n_large * kLargeWords, [&](uint32_t w) { clear_thread(w, W); });
      each(n, [&](uint32_t i) { bounds_thread(i, W, parity); });
      each(n, [&](uint32_t i) { bin_thread(i, W, parity, nullptr, kNone); });
    }
    W.ctr[2u * (parity ^ 1u) + kCtrOpen] = 0u; W.ctr[2u * (parity ^ 1u) + kCtrLarge] = 0u;
    each(n_open, [&](uint32_t r) { split_thread(r, W, parity, level + 1u, max_depth, next_base); });
    scan_flags_host(n, W, parity, reverse);
    each(n, [&](uint32_t i) { partition_thread(i, n, W, parity); });
    next_base += 2u * n_open;
    parity ^= 1u;
    level += 1u;
  }
  if (levels) *levels = level;
  if (W.ctr[kCtrError]) return false;
  const std::vector<uint32_t> order(W.idx[parity], W.idx[parity] + n);
  ptlbvh::fill_slots(frames, order, out);
  uint32_t stats[ptlbvh::kStats] = {};
  out.nodes.assign(next_base, Node{});
  each(next_base, [&](uint32_t k) { count_thread(k, W); });
  each(next_base, [&](uint32_t k) { emit_thread(k, next_base, W, out.nodes.data(), stats); });
  if (stats[ptlbvh::kStatNodes] != next_base) return false;
  out.depth = stats[ptlbvh::kStatDepth]; out.max_leaf = stats[ptlbvh::kStatMaxLeaf];
  ptlbvh::HostScratch H;
  const ptlbvh::Scratch S = H.view(n);
  ptlbvh::fit_boxes_threads(out, S, stats, pad_scale);
  return true;
}

}  // namespace ptsah
