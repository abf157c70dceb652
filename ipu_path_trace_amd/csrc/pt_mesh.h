// pt_mesh.h -- the walk of a mesh's stackless BVH and its box test (pt_set_scene_meshes, include/ptmi.h), written ONCE for the
// kernels and for the host: no HIP intrinsic, no HIP type, so tests/mesh_bvh_main.cpp compiles it with g++ alone.  Compile
// with -ffp-contract=off like everything else here: every operation below is one rounded binary32.
//
// Layout (built by ptmi_mesh.h).  Nodes lie in depth-first order, the left child of an inner node at node + 1; `skip` is the
// node to continue at when a node's box is missed and also what follows a leaf; skip == n_nodes ends the walk, so the walk
// keeps no stack.  Triangles lie in leaf order ("slots"), three 16-byte vectors each holding v0, e1, e2, n as twelve floats;
// orig[slot] is the triangle's index in the caller's mesh.
//
// Ties.  The smallest t wins and, among equal t INSIDE one mesh, the lowest original index, so the result does not depend on
// the tree: the node test uses <= against the best t so far, and the triangle loop accepts t == tbest from a lower index.
// Against a hit of an earlier object the rule stays the scene's strict < (best_orig starts at 0: no index is lower).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_MESH_HD __host__ __device__ __forceinline__
#else
#define PT_MESH_HD inline
#endif

namespace ptmesh {

constexpr float kEps = 1e-5f;              // = ptd::kEps: the scene's intersection epsilon
constexpr float kFarWiden = 1.0000004f;    // tfar is widened by a few ulps before it is compared
constexpr uint32_t kMaxLeaf = 4;           // triangles per leaf at most
constexpr uint32_t kLeafCountBits = 3;     // leaf word: first slot << 3 | count; 0 = an inner node

struct alignas(16) F4 { float x, y, z, w; };
struct alignas(16) Node {                  // 32 bytes
  float lo[3], hi[3];
  uint32_t skip;
  uint32_t leaf;
};
static_assert(sizeof(F4) == 16 && sizeof(Node) == 32, "mesh node / vector layout");

// A triangle's twelve floats from its three vectors.
struct Tri { float v0[3], e1[3], e2[3]; };
PT_MESH_HD Tri load_tri(const F4* t) {
  const F4 a = t[0], b = t[1];
  const float e2z = t[2].x;
  return Tri{{a.x, a.y, a.z}, {a.w, b.x, b.y}, {b.z, b.w, e2z}};
}

// poly_intersect (pt_trace.h) for SHAPE_TRIANGLE, expression for expression: Moeller-Trumbore, two-sided.  0 for a miss.
PT_MESH_HD float tri_intersect(const float* o, const float* d, const Tri& T) {
  const float* e1 = T.e1;
  const float* e2 = T.e2;
  const float pvx = d[1] * e2[2] - d[2] * e2[1], pvy = d[2] * e2[0] - d[0] * e2[2], pvz = d[0] * e2[1] - d[1] * e2[0];   // cross(d, e2)
  const float det = e1[0] * pvx + e1[1] * pvy + e1[2] * pvz;
  if (det == 0.0f) return 0.0f;
  const float inv = 1.0f / det;
  const float tvx = o[0] - T.v0[0], tvy = o[1] - T.v0[1], tvz = o[2] - T.v0[2];
  const float a = (tvx * pvx + tvy * pvy + tvz * pvz) * inv;
  if (!(a >= 0.0f) || a > 1.0f) return 0.0f;
  const float qvx = tvy * e1[2] - tvz * e1[1], qvy = tvz * e1[0] - tvx * e1[2], qvz = tvx * e1[1] - tvy * e1[0];         // cross(tv, e1)
  const float b = (d[0] * qvx + d[1] * qvy + d[2] * qvz) * inv;
  if (!(b >= 0.0f)) return 0.0f;
  if (a + b > 1.0f) return 0.0f;
  const float t = (e2[0] * qvx + e2[1] * qvy + e2[2] * qvz) * inv;
  return t > kEps ? t : 0.0f;
}

// 1 / d per component; a zero component gives +-inf.
PT_MESH_HD void ray_inverse(const float* d, float* inv) {
  inv[0] = 1.0f / d[0]; inv[1] = 1.0f / d[1]; inv[2] = 1.0f / d[2];
}

// The slab test.  Two products per axis.  A NaN among them is 0 x inf: the origin lies ON a slab plane and the direction is
// parallel to it, so the ray runs inside the closed slab -- a triangle with an edge in that plane is hit -- and the axis is
// DROPPED: it constrains nothing, instead of rejecting the node.  (The other product of that axis is then +-inf or NaN too;
// taking it as the axis' near and far value would reject as well, so the whole axis goes.)  Visit when tnear <= tfar, tfar > 0
// and tnear <= tbest (<=: an equal-t triangle of a lower index is still reached).
PT_MESH_HD bool box_hit(const Node& N, const float* o, const float* inv, float tbest) {
  float tnear = -INFINITY, tfar = INFINITY;
  for (int k = 0; k < 3; ++k) {
    const float t0 = (N.lo[k] - o[k]) * inv[k], t1 = (N.hi[k] - o[k]) * inv[k];
#ifdef PT_MESH_MUTATE_NAN   // (tests/mesh_bvh_main.cpp: the mutation must fail the test)
    if (t0 != t0 || t1 != t1) return false;
#endif
    const bool on_plane = t0 != t0 || t1 != t1;
    tnear = on_plane ? tnear : fmaxf(tnear, fminf(t0, t1));
    tfar = on_plane ? tfar : fminf(tfar, fmaxf(t0, t1));
  }
  tfar = tfar * kFarWiden;
#ifdef PT_MESH_MUTATE_CULL
  return tnear <= tfar && tfar > 0.0f && tnear < tbest;
#else
  return tnear <= tfar && tfar > 0.0f && tnear <= tbest;
#endif
}

// One candidate against the best so far.
PT_MESH_HD void consider(float t, uint32_t slot, uint32_t index, float& tbest, int& best_slot, uint32_t& best_orig) {
  if (t > kEps && (t < tbest || (t == tbest && index < best_orig))) { tbest = t; best_slot = (int)slot; best_orig = index; }
}

// The nearest triangle of one mesh in front of tbest: its slot, or -1 when the best so far stands.  tbest is carried in and out,
// so the walk culls against the best hit of the objects before it.
PT_MESH_HD int walk(const Node* nodes, uint32_t n_nodes, const F4* tris, const uint32_t* orig, const float* o, const float* d,
                    const float* inv, float& tbest) {
  int best_slot = -1;
  uint32_t best_orig = 0;
  uint32_t node = 0;
  while (node < n_nodes) {
    const Node N = nodes[node];
    if (!box_hit(N, o, inv, tbest)) { node = N.skip; continue; }
    if (N.leaf == 0u) { node += 1u; continue; }
    const uint32_t first = N.leaf >> kLeafCountBits, count = N.leaf & ((1u << kLeafCountBits) - 1u);
    for (uint32_t s = first; s < first + count; ++s)
      consider(tri_intersect(o, d, load_tri(tris + 3u * s)), s, orig[s], tbest, best_slot, best_orig);
    node = N.skip;
  }
  return best_slot;
}

// The yardstick: the same triangle function and the same tie rule over every triangle of the mesh, no tree.
PT_MESH_HD int brute(const F4* tris, const uint32_t* orig, uint32_t n_triangles, const float* o, const float* d, float& tbest) {
  int best_slot = -1;
  uint32_t best_orig = 0;
  for (uint32_t s = 0; s < n_triangles; ++s)
    consider(tri_intersect(o, d, load_tri(tris + 3u * s)), s, orig[s], tbest, best_slot, best_orig);
  return best_slot;
}

// ---- vertex normals (pt_set_mesh_normals, include/ptmi.h): the shading normal of a hit on a triangle of a mesh with normals.
//
// The barycentrics are formed AGAIN, here, by tri_intersect's own expressions (pv, det, inv, tv, a, qv, b) on the ray that hit:
// the same bits as the walk computed, without two more registers alive across the walk.  vn: the triangle slot's three corner
// normals (unit to rounding, in the kernel's frame; .w unused).  ng: the triangle's stored geometric normal.  Steps, every
// operation one rounded binary32:
//   c = (1 - a) - b;  m = ((c n0) + (a n1)) + (b n2) per component;  l2 = dot(m, m)
//   ns = m * (1 / sqrtf(l2)) when l2 > 1e-12 (the kernels' normalise), else ng
//   orientation: dot(ns, ng) < 0 -> ns = -ns      (normals wound against the triangle shade as if wound with it)
//   side: (dot(ns, d) > 0) != (dot(ng, d) > 0) -> ns = ng   (a shading normal that puts the ray on the other side is dropped)
constexpr float kSmoothMinLen2 = 1e-12f;
PT_MESH_HD float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
PT_MESH_HD void tri_bary(const float* o, const float* d, const Tri& T, float& a, float& b) {
  const float* e1 = T.e1;
  const float* e2 = T.e2;
  const float pvx = d[1] * e2[2] - d[2] * e2[1], pvy = d[2] * e2[0] - d[0] * e2[2], pvz = d[0] * e2[1] - d[1] * e2[0];   // cross(d, e2)
  const float det = e1[0] * pvx + e1[1] * pvy + e1[2] * pvz;
  const float inv = 1.0f / det;
  const float tvx = o[0] - T.v0[0], tvy = o[1] - T.v0[1], tvz = o[2] - T.v0[2];
  a = (tvx * pvx + tvy * pvy + tvz * pvz) * inv;
  const float qvx = tvy * e1[2] - tvz * e1[1], qvy = tvz * e1[0] - tvx * e1[2], qvz = tvx * e1[1] - tvy * e1[0];         // cross(tv, e1)
  b = (d[0] * qvx + d[1] * qvy + d[2] * qvz) * inv;
}
// Steps 2-4 from the barycentrics (the kernels call the two halves one after the other, so that the corner normals are fetched
// once the triangle's twelve floats are dead).
PT_MESH_HD void blend_normal(float a, float b, const float* d, const float* ng, const F4* vn, float* ns) {
  const float c = (1.0f - a) - b;
  const F4 n0 = vn[0], n1 = vn[1], n2 = vn[2];
  const float mx = ((c * n0.x) + (a * n1.x)) + (b * n2.x), my = ((c * n0.y) + (a * n1.y)) + (b * n2.y),
              mz = ((c * n0.z) + (a * n1.z)) + (b * n2.z);
  const float l2 = mx * mx + my * my + mz * mz;
  const bool ok = l2 > kSmoothMinLen2;
  const float inv = 1.0f / sqrtf(ok ? l2 : 1.0f);
  float x = ok ? mx * inv : ng[0], y = ok ? my * inv : ng[1], z = ok ? mz * inv : ng[2];
  if (x * ng[0] + y * ng[1] + z * ng[2] < 0.0f) { x = -x; y = -y; z = -z; }
  const bool drop = (x * d[0] + y * d[1] + z * d[2] > 0.0f) != (ng[0] * d[0] + ng[1] * d[1] + ng[2] * d[2] > 0.0f);
  ns[0] = drop ? ng[0] : x; ns[1] = drop ? ng[1] : y; ns[2] = drop ? ng[2] : z;
}
// Step 6, specular only: v = d - 2 dot(d, n) n was formed with the (flipped) shading normal; if it points into the surface --
// dot(v, ng_f) <= 0 with ng_f the geometric normal flipped to face the ray -- it is formed again with ng_f in place of n.
PT_MESH_HD void mirror_guard(const float* d, const float* ng, float* v) {
  const bool back = ng[0] * d[0] + ng[1] * d[1] + ng[2] * d[2] > 0.0f;
  const float fx = back ? -ng[0] : ng[0], fy = back ? -ng[1] : ng[1], fz = back ? -ng[2] : ng[2];
  if (v[0] * fx + v[1] * fy + v[2] * fz <= 0.0f) {
    const float cost = d[0] * fx + d[1] * fy + d[2] * fz;
    v[0] = d[0] - fx * (cost * 2.0f); v[1] = d[1] - fy * (cost * 2.0f); v[2] = d[2] - fz * (cost * 2.0f);
  }
}
PT_MESH_HD void shading_normal(const float* o, const float* d, const Tri& T, const float* ng, const F4* vn, float& a, float& b,
                               float* ns) {
  tri_bary(o, d, T, a, b);
  blend_normal(a, b, d, ng, vn, ns);
}

// ---- texture coordinates and image textures (pt_set_mesh_texture, include/ptmi.h): the texel of a hit on a triangle of a
// textured mesh.  The barycentrics are tri_bary's, on the ray that hit.  Every operation one rounded binary32; the lerp is
// spelled with fmaf, as the environment map's is, so that no contraction setting changes it.
//   c = (1 - a) - b;  s = ((c s0) + (a s1)) + (b s2), t likewise                            (rule 2)
//   REPEAT: x' = x - floorf(x);  CLAMP: x' = fminf(fmaxf(x, 0), 1);  not (x' >= 0) -> 0      (rule 3)
//   (s, t) = (0, 0) is the image's bottom-left corner; rows are stored top to bottom         (rule 4)
constexpr int kTexNearest = 0, kTexBilinear = 1;   // PT_TEX_FILTER_NEAREST / _BILINEAR
constexpr int kTexRepeat = 0, kTexClamp = 1;       // PT_TEX_WRAP_REPEAT / _CLAMP
// What a textured mesh's row looks its image up by: one per scene row in a device table (a row without a texture: all zero).
struct alignas(16) TexDesc {
  const F4* texels;          // [height][width] (B, G, R, 0), rows top to bottom
  uint32_t width, height;
  int32_t filter, wrap;
  uint32_t pad[2];
};
static_assert(sizeof(TexDesc) == 32, "texture descriptor layout");
// uv: the slot's three corners (s0, t0, s1, t1, s2, t2)
PT_MESH_HD void blend_uv(float a, float b, const float* uv, float& s, float& t) {
  const float c = (1.0f - a) - b;
  s = ((c * uv[0]) + (a * uv[2])) + (b * uv[4]);
  t = ((c * uv[1]) + (a * uv[3])) + (b * uv[5]);
}
PT_MESH_HD float tex_wrap(float x, int wrap) {
  const float w = wrap == kTexClamp ? fminf(fmaxf(x, 0.0f), 1.0f) : x - floorf(x);
  return w >= 0.0f ? w : 0.0f;   // (inf - inf, or a NaN that came in)
}
// An index in [-1, size] into [0, size): wrapped or clamped by the mode.  Whatever comes in, what goes out is inside the image.
PT_MESH_HD uint32_t tex_index(int i, uint32_t size, int wrap) {
  const int n = (int)size;
  if (wrap == kTexClamp) i = i < 0 ? 0 : (i >= n ? n - 1 : i);
  else i = i < 0 ? i + n : (i >= n ? i - n : i);
  return (uint32_t)(i < 0 ? 0 : (i >= n ? n - 1 : i));
}
PT_MESH_HD float tex_lerp(float f, float p, float q) { return fmaf(f, q - p, p); }
PT_MESH_HD void texel(const TexDesc& D, float s, float t, float* bgr) {
  const float sw = tex_wrap(s, D.wrap), tw = tex_wrap(t, D.wrap);
  const float fw = (float)D.width, fh = (float)D.height;
  const float tv = 1.0f - tw;
  if (D.filter == kTexNearest) {
    const float X = sw * fw, Y = tv * fh;
    const uint32_t c0 = tex_index((int)floorf(X), D.width, D.wrap), r0 = tex_index((int)floorf(Y), D.height, D.wrap);
    const F4 q = D.texels[(size_t)r0 * D.width + c0];
    bgr[0] = q.x; bgr[1] = q.y; bgr[2] = q.z;
    return;
  }
  const float X = sw * fw - 0.5f, Y = tv * fh - 0.5f;
  const float xf = floorf(X), yf = floorf(Y);
  const float fx = X - xf, fy = Y - yf;
  const int ci = (int)xf, ri = (int)yf;
  const uint32_t c0 = tex_index(ci, D.width, D.wrap), c1 = tex_index(ci + 1, D.width, D.wrap);
  const uint32_t r0 = tex_index(ri, D.height, D.wrap), r1 = tex_index(ri + 1, D.height, D.wrap);
  const F4* row0 = D.texels + (size_t)r0 * D.width;
  const F4* row1 = D.texels + (size_t)r1 * D.width;
  const F4 t00 = row0[c0], t01 = row0[c1], t10 = row1[c0], t11 = row1[c1];   // four loads in flight
  bgr[0] = tex_lerp(fy, tex_lerp(fx, t00.x, t01.x), tex_lerp(fx, t10.x, t11.x));
  bgr[1] = tex_lerp(fy, tex_lerp(fx, t00.y, t01.y), tex_lerp(fx, t10.y, t11.y));
  bgr[2] = tex_lerp(fy, tex_lerp(fx, t00.z, t01.z), tex_lerp(fx, t10.z, t11.z));
}

}  // namespace ptmesh
