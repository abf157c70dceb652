// pt_mesh_build.h -- the linear BVH builder and the refit of a mesh's tree (pt_set_mesh_build, include/ptmi.h), written ONCE for
// the kernels and for the host: the functions behind PT_MESH_HD hold no HIP type, so tests/mesh_lbvh_main.cpp compiles them with
// g++ alone.  Compile with -ffp-contract=off like everything else here: every operation below is one rounded binary32.
//
// THE RULE (what "the same tree" means; the kernels of ptmi_mesh_build.h, the sequential reference builder at the end of this
// file and the test program all call the functions of this file, so there is one definition):
//   * a triangle's box is ptmesh::tri_box's (min / max of v0, v0 + e1, v0 + e2, one rounded add each), its centroid
//     0.5f * (lo + hi) per axis; the centroids' bounds are their min / max;
//   * per axis, ext = hi - lo and q = ext > 0 ? min(2097151, (uint)(((c - lo) / ext) * 2097152.0f)) : 0, the division IEEE-correct;
//   * the code is the 63-bit Morton code of (qx, qy, qz), x most significant; the sort key is (code, triangle index), so keys
//     are unique and any correct sort gives one order; slot s of the mesh holds the s-th triangle of that order;
//   * a range [a, b] of more than kMaxLeaf keys splits at the highest differing bit of its first and last key, at the first key
//     with that bit set -- for equal codes the "key" continues with the sorted POSITION (Karras' tie-break), so such a range
//     splits at the first position in (a, b] that has the highest differing bit of a and b set; a range of <= kMaxLeaf keys is a
//     leaf;
//   * layout, boxes and pad are ptmi_mesh.h's: depth-first order, left child at node + 1, skip, leaf word; a leaf's box is the
//     union of its triangles' boxes, an inner node's the union of its two children's (min / max only: exact, in any order);
//     pad = kPadScale x the largest absolute coordinate of the root's box, applied as lo - pad and hi + pad.
//
// THE PARALLEL FORM.  Over the sorted keys the split rule is Karras' binary radix tree (2012) with n - 1 inner nodes, inner node
// i having key i at one end of its range; each is found on its own (tree_thread).  The tree of the rule is that tree PRUNED: a
// radix node is emitted when its parent's range holds more than kMaxLeaf keys (or it is the root), as a leaf when its own range
// holds at most kMaxLeaf.  A bottom-up pass over arrival counters (count_thread: the first thread to arrive at a node returns,
// the second goes on; nobody waits) gives every radix node its number of emitted leaves L.  An emitted node then finds its
// depth-first index by walking to the root (emit_thread): + 1 for a left turn, + 2 L(left sibling) for a right turn; its skip is
// index + 2 L - 1; a leaf's first slot is the first key of its range.  The boxes come from the pass the refit uses as well
// (box_leaf_thread, box_climb_thread, pad_thread), which needs only the depth-first layout: the children of inner node i are
// i + 1 and skip(i + 1).  So a refit serves a host-built (SAH) tree and a device-built one alike.
#pragma once
#include <cmath>
#include <cstdint>

#include "pt_mesh.h"

namespace ptlbvh {

using ptmesh::F4;
using ptmesh::Node;

constexpr float kPadScale = 1.52587890625e-05f;   // 2^-16 = ptmesh::kPadScale (ptmi_mesh.h)
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kFrameFloats = 12;             // v0, e1, e2, n
enum { kStatNodes = 0, kStatDepth = 1, kStatMaxLeaf = 2, kStatPad = 3, kStats = 4 };   // a mesh's four words on the device

// ptcamera::Basis without its host-only neighbours: what a kernel takes by value.  posed == 0: the world frame, no transform at all.
struct Pose { float r[3], u[3], f[3], position[3]; int32_t posed; };

PT_MESH_HD float min2(float a, float b) { return b < a ? b : a; }   // std::min / std::max, as ptmesh::Box::grow uses them
PT_MESH_HD float max2(float a, float b) { return a < b ? b : a; }
PT_MESH_HD uint32_t float_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
PT_MESH_HD float bits_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// ---- frames: ptcamera::to_camera_direction / to_camera_point and ptmesh::kernel_frames, expression for expression
PT_MESH_HD float dot3(const float* a, const float* b) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }
PT_MESH_HD void to_direction(const Pose& P, const float* n, float* out) {
  const float x = dot3(P.r, n), y = dot3(P.u, n), z = 0.f - dot3(P.f, n);
  out[0] = x; out[1] = y; out[2] = z;
}
PT_MESH_HD void to_point(const Pose& P, const float* p, float* out) {
  const float d[3] = {p[0] - P.position[0], p[1] - P.position[1], p[2] - P.position[2]};
  to_direction(P, d, out);
}
PT_MESH_HD void kernel_frame(const Pose& P, const float* w, float* o) {
  if (!P.posed) { for (uint32_t k = 0; k < kFrameFloats; ++k) o[k] = w[k]; return; }
  to_point(P, w, o);
  to_direction(P, w + 3, o + 3);
  to_direction(P, w + 6, o + 6);
  to_direction(P, w + 9, o + 9);
}

// ---- boxes, centroids, codes
PT_MESH_HD void tri_box(const float* fr, float* lo, float* hi) {   // = ptmesh::tri_box
  for (int k = 0; k < 3; ++k) {
    const float p0 = fr[k], p1 = fr[k] + fr[3 + k], p2 = fr[k] + fr[6 + k];
    float l = INFINITY, h = -INFINITY;
    l = min2(l, p0); h = max2(h, p0);
    l = min2(l, p1); h = max2(h, p1);
    l = min2(l, p2); h = max2(h, p2);
    lo[k] = l; hi[k] = h;
  }
}
PT_MESH_HD void centroid(const float* fr, float* c) {
  float lo[3], hi[3];
  tri_box(fr, lo, hi);
  for (int k = 0; k < 3; ++k) c[k] = 0.5f * (lo[k] + hi[k]);
}
PT_MESH_HD uint32_t quantise(float c, float lo, float hi) {
  const float ext = hi - lo;
  if (!(ext > 0.f) || !(ext < INFINITY)) return 0u;
  const uint32_t q = (uint32_t)(((c - lo) / ext) * 2097152.0f);
  return q < 2097151u ? q : 2097151u;
}
PT_MESH_HD uint64_t spread3(uint32_t v) {   // 21 bits, two zeros after each
  uint64_t x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// bounds: the centroids' lo[3], hi[3]
PT_MESH_HD uint64_t morton(const float* c, const float* bounds) {
  return spread3(quantise(c[0], bounds[0], bounds[3])) << 2 | spread3(quantise(c[1], bounds[1], bounds[4])) << 1 |
         spread3(quantise(c[2], bounds[2], bounds[5]));
}

// ---- the radix tree over n sorted codes
struct Scratch {   // per mesh under construction; every array for the largest mesh of the scene (T keys)
  uint32_t* kparent;       // [T]   radix inner node -> its parent (kNone: the root)
  uint32_t* leaf_parent;   // [T]   key -> the radix inner node above it
  uint32_t* kfirst;        // [T]   radix inner node's range [kfirst, klast] and the last key of its left part
  uint32_t* klast;
  uint32_t* ksplit;
  uint32_t* outl;          // [T]   emitted leaves below a radix inner node
  uint32_t* kcounter;      // [T]   arrivals (count_thread)
  uint32_t* parent;        // [2T]  depth-first node -> its parent (the box pass)
  uint32_t* counter;       // [2T]  arrivals (box_climb_thread)
};
constexpr uint32_t kScratchWords = 11;   // per key

// The length of the common prefix of keys i and j (code, then position), -1 outside the array.
PT_MESH_HD int prefix(const uint64_t* codes, uint32_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= (int64_t)n) return -1;
  const uint64_t a = codes[i], b = codes[j];
  if (a != b) return __builtin_clzll(a ^ b);
  return 64 + __builtin_clz((uint32_t)i ^ (uint32_t)j);   // (i != j wherever this is called)
}
// Radix inner node i of n >= 2 keys: its range and the last key of its left part (Karras 2012, figure 4).
PT_MESH_HD void radix_node(const uint64_t* codes, uint32_t n, uint32_t i, uint32_t& first, uint32_t& last, uint32_t& split) {
  const int64_t I = i;
  const int64_t d = prefix(codes, n, I, I + 1) > prefix(codes, n, I, I - 1) ? 1 : -1;
  const int dmin = prefix(codes, n, I, I - d);
  int64_t lmax = 2;
  while (prefix(codes, n, I, I + lmax * d) > dmin) lmax *= 2;
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (prefix(codes, n, I, I + (l + t) * d) > dmin) l += t;
  const int64_t j = I + l * d;
  const int dnode = prefix(codes, n, I, j);
  int64_t s = 0;
  for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
    if (prefix(codes, n, I, I + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int64_t g = I + s * d + (d < 0 ? -1 : 0);
  first = (uint32_t)(d > 0 ? I : j);
  last = (uint32_t)(d > 0 ? j : I);
  split = (uint32_t)g;
}

// One arrival at a node with two children: what the counter held before.  On the device the fences make what this thread wrote
// visible to the thread that arrives second, and what the first wrote visible to this one.
PT_MESH_HD uint32_t arrive(uint32_t* counter) {
#if defined(__HIP_DEVICE_COMPILE__)
  __threadfence();
  const uint32_t before = atomicAdd(counter, 1u);
  __threadfence();
  return before;
#else
  return (*counter)++;
#endif
}
PT_MESH_HD void stat_max(uint32_t* word, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(word, v);
#else
  if (v > *word) *word = v;
#endif
}

// thread i of n: radix inner node i (i < n - 1), its range, and its children's parent links
PT_MESH_HD void tree_thread(const uint64_t* codes, uint32_t n, uint32_t i, const Scratch& S) {
  if (i == 0) { S.kparent[0] = kNone; if (n == 1) S.leaf_parent[0] = kNone; }
  if (i + 1 >= n) return;
  uint32_t first, last, g;
  radix_node(codes, n, i, first, last, g);
  S.kfirst[i] = first; S.klast[i] = last; S.ksplit[i] = g; S.kcounter[i] = 0u;
  if (first == g) S.leaf_parent[g] = i; else S.kparent[g] = i;
  if (last == g + 1) S.leaf_parent[g + 1] = i; else S.kparent[g + 1] = i;
}
// thread p of n: from key p upwards, the emitted leaves below every radix inner node
PT_MESH_HD void count_thread(uint32_t p, const Scratch& S) {
  uint32_t node = S.leaf_parent[p];
  while (node != kNone) {
    if (arrive(&S.kcounter[node]) == 0u) return;
    const uint32_t first = S.kfirst[node], last = S.klast[node], g = S.ksplit[node];
    uint32_t leaves = 1u;
    if (last - first + 1u > ptmesh::kMaxLeaf)
      leaves = (g - first + 1u <= ptmesh::kMaxLeaf ? 1u : S.outl[g]) + (last - g <= ptmesh::kMaxLeaf ? 1u : S.outl[g + 1u]);
    S.outl[node] = leaves;
    node = S.kparent[node];
  }
}
// thread x of 2 n - 1: radix inner node x (x < n - 1) or key x - (n - 1); writes skip and leaf word of the node it emits, if any.
// stats: zeroed before the launch.
PT_MESH_HD void emit_thread(uint32_t n, uint32_t x, const Scratch& S, Node* nodes, uint32_t* stats) {
  const bool inner = x < n - 1u;
  const uint32_t first = inner ? S.kfirst[x] : x - (n - 1u), last = inner ? S.klast[x] : first;
  const uint32_t count = last - first + 1u;
  uint32_t p = inner ? S.kparent[x] : S.leaf_parent[first];
  if (p != kNone && S.klast[p] - S.kfirst[p] + 1u <= ptmesh::kMaxLeaf) return;   // inside a leaf
  uint32_t index = 0u, depth = 1u, cur_first = first;
  while (p != kNone) {
    const uint32_t pf = S.kfirst[p], g = S.ksplit[p];
    if (cur_first == g + 1u) index += 2u * (g - pf + 1u <= ptmesh::kMaxLeaf ? 1u : S.outl[g]);   // a right turn: past the left sibling
    else index += 1u;
    depth += 1u;
    cur_first = pf;
    p = S.kparent[p];
  }
  const bool leaf = count <= ptmesh::kMaxLeaf;
  const uint32_t leaves = leaf ? 1u : S.outl[x];
  nodes[index].skip = index + 2u * leaves - 1u;
  nodes[index].leaf = leaf ? (first << ptmesh::kLeafCountBits | count) : 0u;
  stat_max(&stats[kStatDepth], depth);
  if (leaf) stat_max(&stats[kStatMaxLeaf], count);
  if (index == 0u) stats[kStatNodes] = 2u * leaves - 1u;
}

// ---- slots: triangle `tri` of the mesh into slot s, in the frame of P
// world: the mesh's frames in triangle order; corner / corner_uv: its world corner normals (nine floats per triangle) and uvs
// (six), or null; the outputs are the mesh's own parts of the slot arrays.
PT_MESH_HD void slot_thread(uint32_t s, uint32_t tri, const Pose& P, const float* world, const float* corner, F4* tris, F4* normals) {
  float fr[kFrameFloats];
  kernel_frame(P, world + (size_t)kFrameFloats * tri, fr);
  tris[3u * (size_t)s] = F4{fr[0], fr[1], fr[2], fr[3]};
  tris[3u * (size_t)s + 1u] = F4{fr[4], fr[5], fr[6], fr[7]};
  tris[3u * (size_t)s + 2u] = F4{fr[8], fr[9], fr[10], fr[11]};
  if (corner)
    for (int c = 0; c < 3; ++c) {   // = ptmesh::slot_normals
      const float* w = corner + 9u * (size_t)tri + 3 * c;
      float o[3] = {w[0], w[1], w[2]};
      if (P.posed) to_direction(P, w, o);
      normals[3u * (size_t)s + c] = F4{o[0], o[1], o[2], 0.f};
    }
}

// ---- the box pass over a depth-first tree (nodes: skip and leaf word valid; tris: the slots in the frame to fit)
PT_MESH_HD float pad_of(const Node& root, float pad_scale) {
  float big = 0.f;
  for (int k = 0; k < 3; ++k) big = max2(big, max2(fabsf(root.lo[k]), fabsf(root.hi[k])));
  return pad_scale * big;
}
// thread i of stats[kStatNodes]: a leaf's box without the pad; an inner node's links
PT_MESH_HD void box_leaf_thread(uint32_t i, Node* nodes, const F4* tris, const Scratch& S, uint32_t* stats, float pad_scale) {
  if (i >= stats[kStatNodes]) return;
  if (i == 0u) S.parent[0] = kNone;
  const uint32_t leaf = nodes[i].leaf;
  if (leaf == 0u) {
    const uint32_t l = i + 1u, r = nodes[l].skip;
    S.counter[i] = 0u;
    S.parent[l] = i; S.parent[r] = i;
    return;
  }
  const uint32_t first = leaf >> ptmesh::kLeafCountBits, count = leaf & ((1u << ptmesh::kLeafCountBits) - 1u);
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t s = first; s < first + count; ++s) {
    const F4 a = tris[3u * (size_t)s], b = tris[3u * (size_t)s + 1u], c = tris[3u * (size_t)s + 2u];
    const float fr[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
    float tl[3], th[3];
    tri_box(fr, tl, th);
    for (int k = 0; k < 3; ++k) { lo[k] = min2(lo[k], tl[k]); hi[k] = max2(hi[k], th[k]); }
  }
  for (int k = 0; k < 3; ++k) { nodes[i].lo[k] = lo[k]; nodes[i].hi[k] = hi[k]; }
  if (stats[kStatNodes] == 1u) stats[kStatPad] = float_bits(pad_of(nodes[0], pad_scale));
}
// thread i of stats[kStatNodes], after box_leaf_thread has run for all: from leaf i upwards, each inner box from its two children
PT_MESH_HD void box_climb_thread(uint32_t i, Node* nodes, const Scratch& S, uint32_t* stats, float pad_scale) {
  if (i >= stats[kStatNodes] || nodes[i].leaf == 0u) return;
  uint32_t p = S.parent[i];
  while (p != kNone) {
    if (arrive(&S.counter[p]) == 0u) return;
    const uint32_t l = p + 1u, r = nodes[l].skip;
    for (int k = 0; k < 3; ++k) {
      const float lo = min2(nodes[l].lo[k], nodes[r].lo[k]), hi = max2(nodes[l].hi[k], nodes[r].hi[k]);
      nodes[p].lo[k] = lo; nodes[p].hi[k] = hi;
    }
    if (p == 0u) stats[kStatPad] = float_bits(pad_of(nodes[0], pad_scale));
    p = S.parent[p];
  }
}
// thread i of stats[kStatNodes], after box_climb_thread has run for all: the pad, by the builder's own two expressions
PT_MESH_HD void pad_thread(uint32_t i, Node* nodes, const uint32_t* stats) {
  if (i >= stats[kStatNodes]) return;
#if defined(PT_LBVH_MUTATE_NO_PAD)   // (tests/mesh_lbvh_main.cpp: the mutation must fail the test)
  return;
#endif
  const float pad = bits_float(stats[kStatPad]);
  for (int k = 0; k < 3; ++k) {
    const float lo = nodes[i].lo[k] - pad, hi = nodes[i].hi[k] + pad;
    nodes[i].lo[k] = lo; nodes[i].hi[k] = hi;
  }
}

}  // namespace ptlbvh

// ---- the host: the sequential reference builder and refit, and the parallel form run thread by thread
#include <algorithm>
#include <vector>

#include "ptmi_mesh.h"

namespace ptlbvh {

static_assert(kPadScale == ptmesh::kPadScale && kFrameFloats == ptmesh::kFrameFloats, "one pad and one frame for both builders");

inline Pose pose_of(const ptcamera::Basis* cam) {
  Pose P{};
  if (!cam) return P;
  for (int k = 0; k < 3; ++k) { P.r[k] = cam->r[k]; P.u[k] = cam->u[k]; P.f[k] = cam->f[k]; P.position[k] = cam->position[k]; }
  P.posed = 1;
  return P;
}

// The sorted keys of n frames: codes[s] and order[s], the triangle in slot s.
inline void sorted_keys(const float* frames, uint32_t n, std::vector<uint64_t>& codes, std::vector<uint32_t>& order) {
  std::vector<float> c(3 * (size_t)n);
  float bounds[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (uint32_t j = 0; j < n; ++j) {
    centroid(frames + (size_t)kFrameFloats * j, &c[3 * (size_t)j]);
    for (int k = 0; k < 3; ++k) { bounds[k] = min2(bounds[k], c[3 * (size_t)j + k]); bounds[3 + k] = max2(bounds[3 + k], c[3 * (size_t)j + k]); }
  }
  std::vector<uint64_t> code(n);
  for (uint32_t j = 0; j < n; ++j) code[j] = morton(&c[3 * (size_t)j], bounds);
  order.resize(n);
  for (uint32_t j = 0; j < n; ++j) order[j] = j;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return code[a] != code[b] ? code[a] < code[b] : a < b; });
  codes.resize(n);
  for (uint32_t s = 0; s < n; ++s) codes[s] = code[order[s]];
}

inline void fill_slots(const float* frames, const std::vector<uint32_t>& order, ptmesh::Built& out) {
  out.orig = order;
  out.tris.resize(3 * order.size());
  for (size_t s = 0; s < order.size(); ++s) {
    const float* f = frames + (size_t)kFrameFloats * order[s];
    out.tris[3 * s] = F4{f[0], f[1], f[2], f[3]};
    out.tris[3 * s + 1] = F4{f[4], f[5], f[6], f[7]};
    out.tris[3 * s + 2] = F4{f[8], f[9], f[10], f[11]};
  }
}

inline void slot_box(const ptmesh::Built& B, uint32_t s, float* lo, float* hi) {
  const F4 a = B.tris[3 * (size_t)s], b = B.tris[3 * (size_t)s + 1], c = B.tris[3 * (size_t)s + 2];
  const float fr[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
  tri_box(fr, lo, hi);
}

// The boxes of a tree whose skips, leaf words and slots stand: each leaf from its triangles, each inner node from its two
// children, then the pad from the new root.  keep_pad (a mutation the test program must catch): the pad is left as it was.
inline void fit_boxes(ptmesh::Built& B, float pad_scale, bool keep_pad = false) {
  for (size_t i = B.nodes.size(); i-- > 0;) {   // depth-first order: every child lies after its parent
    Node& N = B.nodes[i];
    if (N.leaf != 0u) {
      const uint32_t first = N.leaf >> ptmesh::kLeafCountBits, count = N.leaf & ((1u << ptmesh::kLeafCountBits) - 1u);
      for (int k = 0; k < 3; ++k) { N.lo[k] = INFINITY; N.hi[k] = -INFINITY; }
      for (uint32_t s = first; s < first + count; ++s) {
        float lo[3], hi[3];
        slot_box(B, s, lo, hi);
        for (int k = 0; k < 3; ++k) { N.lo[k] = min2(N.lo[k], lo[k]); N.hi[k] = max2(N.hi[k], hi[k]); }
      }
    } else {
      const Node& L = B.nodes[i + 1];
      const Node& R = B.nodes[L.skip];
      for (int k = 0; k < 3; ++k) { N.lo[k] = min2(L.lo[k], R.lo[k]); N.hi[k] = max2(L.hi[k], R.hi[k]); }
    }
  }
  if (!keep_pad) B.pad = pad_of(B.nodes[0], pad_scale);
#if defined(PT_LBVH_MUTATE_NO_PAD)
  return;
#endif
  for (Node& N : B.nodes)
    for (int k = 0; k < 3; ++k) {
      const float lo = N.lo[k] - B.pad, hi = N.hi[k] + B.pad;
      N.lo[k] = lo; N.hi[k] = hi;
    }
}

// THE REFERENCE BUILDER: the rule at the head of this file, one range after the other.
inline void emit_range(const std::vector<uint64_t>& codes, uint32_t a, uint32_t b, uint32_t depth, ptmesh::Built& out) {
  const uint32_t self = (uint32_t)out.nodes.size(), count = b - a + 1u;
  out.nodes.push_back(Node{});
  out.depth = std::max(out.depth, depth);
  if (count <= ptmesh::kMaxLeaf) {
    out.max_leaf = std::max(out.max_leaf, count);
    out.nodes[self].leaf = a << ptmesh::kLeafCountBits | count;
    out.nodes[self].skip = self + 1u;
    return;
  }
  uint32_t split;   // the first key of the right part
  if (codes[a] != codes[b]) {
    const uint64_t bit = 1ull << (63 - __builtin_clzll(codes[a] ^ codes[b]));
    split = (uint32_t)(std::partition_point(codes.begin() + a, codes.begin() + b + 1, [&](uint64_t c) { return !(c & bit); }) - codes.begin());
  } else {
    const int bit = 31 - __builtin_clz(a ^ b);
    split = (b >> bit) << bit;
  }
  emit_range(codes, a, split - 1u, depth + 1u, out);
  emit_range(codes, split, b, depth + 1u, out);
  out.nodes[self].skip = (uint32_t)out.nodes.size();
}
// frames: in the kernel's frame, triangle order (n >= 1)
inline void build(const float* frames, uint32_t n, ptmesh::Built& out, float pad_scale = kPadScale) {
  out = ptmesh::Built{};
  std::vector<uint64_t> codes;
  std::vector<uint32_t> order;
  sorted_keys(frames, n, codes, order);
  fill_slots(frames, order, out);
  emit_range(codes, 0u, n - 1u, 1u, out);
  fit_boxes(out, pad_scale);
}

// THE REFERENCE REFIT of any tree (SAH or linear) to the frame of P: topology, slot order and orig stand.
inline void refit(ptmesh::Built& B, const float* world, const Pose& P, float pad_scale = kPadScale, bool keep_pad = false) {
  for (size_t s = 0; s < B.orig.size(); ++s) slot_thread((uint32_t)s, B.orig[s], P, world, nullptr, B.tris.data(), nullptr);
  fit_boxes(B, pad_scale, keep_pad);
}

// The parallel form, its threads run one after the other in index order (the kernels run the same functions): the test program
// holds it against the reference above, byte for byte.
struct HostScratch {
  std::vector<uint32_t> words;
  Scratch view(uint32_t n) {
    words.assign((size_t)kScratchWords * n + 2, 0u);
    uint32_t* w = words.data();
    return Scratch{w, w + n, w + 2 * (size_t)n, w + 3 * (size_t)n, w + 4 * (size_t)n, w + 5 * (size_t)n, w + 6 * (size_t)n, w + 7 * (size_t)n, w + 9 * (size_t)n};
  }
};
inline void fit_boxes_threads(ptmesh::Built& B, const Scratch& S, uint32_t* stats, float pad_scale) {
  const uint32_t nn = stats[kStatNodes];
  for (uint32_t i = 0; i < nn; ++i) box_leaf_thread(i, B.nodes.data(), B.tris.data(), S, stats, pad_scale);
  for (uint32_t i = 0; i < nn; ++i) box_climb_thread(i, B.nodes.data(), S, stats, pad_scale);
  for (uint32_t i = 0; i < nn; ++i) pad_thread(i, B.nodes.data(), stats);
  B.pad = bits_float(stats[kStatPad]);
}
inline void build_threads(const float* frames, uint32_t n, ptmesh::Built& out, float pad_scale = kPadScale) {
  out = ptmesh::Built{};
  std::vector<uint64_t> codes;
  std::vector<uint32_t> order;
  sorted_keys(frames, n, codes, order);
  fill_slots(frames, order, out);
  HostScratch H;
  const Scratch S = H.view(n);
  uint32_t stats[kStats] = {};
  out.nodes.assign(2 * (size_t)n - 1, Node{});
  for (uint32_t i = 0; i < n; ++i) tree_thread(codes.data(), n, i, S);
  for (uint32_t p = 0; p < n; ++p) count_thread(p, S);
  for (uint32_t x = 0; x < 2 * n - 1; ++x) emit_thread(n, x, S, out.nodes.data(), stats);
  out.nodes.resize(stats[kStatNodes]);
  out.depth = stats[kStatDepth]; out.max_leaf = stats[kStatMaxLeaf];
  fit_boxes_threads(out, S, stats, pad_scale);
}
inline void refit_threads(ptmesh::Built& B, const float* world, const Pose& P, float pad_scale = kPadScale) {
  for (size_t s = 0; s < B.orig.size(); ++s) slot_thread((uint32_t)s, B.orig[s], P, world, nullptr, B.tris.data(), nullptr);
  HostScratch H;
  const Scratch S = H.view((uint32_t)B.orig.size());
  uint32_t stats[kStats] = {(uint32_t)B.nodes.size(), B.depth, B.max_leaf, 0u};
  fit_boxes_threads(B, S, stats, pad_scale);
}

}  // namespace ptlbvh
