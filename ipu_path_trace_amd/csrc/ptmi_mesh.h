// ptmi_mesh.h -- host side of triangle meshes in runtime scenes (pt_set_scene_meshes, include/ptmi.h): validation, the
// triangles' frames, and the builder of the stackless BVH that pt_mesh.h walks.  Plain C++ on purpose, no HIP type: the library
// (ptmi.hip) and the stand-alone test program (tests/mesh_bvh_main.cpp) include it.
//
// Builder.  A binary tree by binned SAH (16 bins per axis over the centroids' bounds, the cheapest of the three axes); where SAH
// finds no split -- every centroid in one bin, or a tree already 48 levels deep -- the range is halved in its current order.
// Leaves hold at most four triangles.  Nothing depends on addresses, threads or time: the same triangles give the same tree.
// The tree is written in depth-first order as it is built (pt_mesh.h: the layout and the skip links).
//
// Boxes.  A triangle's box is the min / max of v0, v0 + e1, v0 + e2 (one rounded add each) in the kernel's frame; a node's box
// is the union of its triangles', then padded outward by ONE value per mesh, pad = kPadScale x (largest absolute coordinate of
// the root box).  It is absolute, like the tracer's epsilon.  The pad is a SAFETY MARGIN, NOT A PROOF: Moeller-Trumbore's a, b
// and t carry rounding that grows at grazing incidence, and a triangle the test accepts may have its computed hit point a
// little outside its exact box.  The contract is only that the walk finds what the loop over all triangles finds on the
// fixtures and rays of tests/mesh_bvh_main.cpp and tests/test_gpu_scene_meshes.py (counts: DESIGN.md section 4.16).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pt_mesh.h"
#include "ptmi_camera.h"
#include "ptmi_scene.h"

namespace ptmesh {

constexpr float kPadScale = 1.52587890625e-05f;   // 2^-16
constexpr int kBins = 16;
constexpr uint32_t kMaxDepthSah = 48;

// ---- validation (include/ptmi.h: the order is part of the contract)

// What is wrong with one triangle -- its corners' vertex indices ix and their values v --, "" if nothing: checks 10..12 of
// pt_set_scene_meshes, lowest corner first, lowest component first.  pt_update_mesh_vertices names a rejected triangle by this.
inline std::string triangle_fault(const uint32_t* ix, const float (&v)[3][3]) {
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(v[c][k])) return "vertices[" + std::to_string(ix[c]) + "] must be finite (got " + ptscene::num(v[c][k]) + ")";
  const ptscene::PolyFrame f = ptscene::poly_frame(v);
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(f.e1[k]) || !std::isfinite(f.e2[k]) || !std::isfinite(f.c[k]))
      return "vertex differences and their cross product must be finite";
  if (!(f.cc > 0.f) || !std::isfinite(f.cc)) return "vertices are collinear";
  return "";
}

// Checks 1..12 of pt_set_scene_meshes; "" if the call is valid.
inline std::string check(const pt_scene_object_ex* objs, uint32_t n, uint32_t stride, const pt_mesh* meshes, uint32_t n_meshes) {
  const std::string bad = ptscene::check_ex(objs, n, stride, PT_SHAPE_MESH);
  if (!bad.empty()) return bad;
  uint32_t rows = 0;
  for (uint32_t i = 0; i < n; ++i) rows += objs[i].shape == PT_SHAPE_MESH ? 1u : 0u;
  if (rows != n_meshes)
    return "scene: " + std::to_string(rows) + " object(s) of shape 4 (mesh) but n_meshes = " + std::to_string(n_meshes);
  if (n_meshes && !meshes) return "scene: null mesh table";
  uint64_t total = 0;
  for (uint32_t m = 0; m < n_meshes; ++m) {
    const pt_mesh& M = meshes[m];
    const std::string at = "mesh " + std::to_string(m) + ": ";
    if (M.struct_size != sizeof(pt_mesh))
      return at + "struct_size must be " + std::to_string(sizeof(pt_mesh)) + " (got " + std::to_string(M.struct_size) + ")";
    if (!M.vertices) return at + "null vertices";
    if (!M.indices) return at + "null indices";
    if (M.n_triangles == 0) return at + "n_triangles must be > 0";
    total += M.n_triangles;
  }
  if (total > PT_MAX_MESH_TRIANGLES)
    return "scene: " + std::to_string(total) + " mesh triangles in all, " + std::to_string(PT_MAX_MESH_TRIANGLES) + " at most";
  for (uint32_t m = 0, row = 0; m < n_meshes; ++m, ++row) {
    while (objs[row].shape != PT_SHAPE_MESH) ++row;
    const pt_mesh& M = meshes[m];
    for (uint32_t j = 0; j < M.n_triangles; ++j) {
      const std::string at = "scene object " + std::to_string(row) + ", mesh " + std::to_string(m) + ", triangle " + std::to_string(j) + ": ";
      float v[3][3];
      for (int c = 0; c < 3; ++c) {
        const uint32_t ix = M.indices[3 * (size_t)j + c];
        if (ix >= M.n_vertices)
          return at + "indices[" + std::to_string(c) + "] must be < n_vertices = " + std::to_string(M.n_vertices) + " (got " + std::to_string(ix) + ")";
      }
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) v[c][k] = M.vertices[3 * (size_t)M.indices[3 * (size_t)j + c] + k];
      const std::string fault = triangle_fault(M.indices + 3 * (size_t)j, v);
      if (!fault.empty()) return at + fault;
    }
  }
  return "";
}

// ---- vertex normals (pt_set_mesh_normals, include/ptmi.h)

// What is wrong with normal k of value v, "" if nothing: the last two checks of pt_set_mesh_normals (pt_update_mesh_vertices
// names a rejected normal by this).
inline std::string normal_fault(uint32_t k, const float* v) {
  for (int q = 0; q < 3; ++q)
    if (!std::isfinite(v[q])) return "normals[" + std::to_string(k) + "] must be finite (got " + ptscene::num(v[q]) + ")";
  volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  volatile float d0 = xx + yy, d1 = d0 + zz;
  if (!(d1 > 0.f) || !std::isfinite(d1)) return "normals[" + std::to_string(k) + "] must have a finite dot(n, n) > 0 (got " + ptscene::num(d1) + ")";
  return "";
}

// The checks of pt_set_mesh_normals that need no device, in the contract's order; "" if the normals are valid.  indices: the
// mesh's own [n_triangles][3] (used when normal_indices is null: per-vertex normals).  Only referenced normals are examined.
inline std::string check_normals(uint32_t mesh, uint32_t n_vertices, uint32_t n_triangles, const uint32_t* indices, const float* normals,
                                 uint32_t n_normals, const uint32_t* normal_indices) {
  const std::string at = "mesh " + std::to_string(mesh) + ": ";
  if (!normals) return at + "null normals with n_normals = " + std::to_string(n_normals);
  if (!normal_indices && n_normals != n_vertices)
    return at + "n_normals must equal n_vertices = " + std::to_string(n_vertices) + " when normal_indices is null (got " + std::to_string(n_normals) + ")";
  const uint32_t* ix = normal_indices ? normal_indices : indices;
  for (uint32_t j = 0; j < n_triangles; ++j)
    for (int c = 0; c < 3; ++c) {
      const std::string tri = at + "triangle " + std::to_string(j) + ": ";
      const uint32_t k = ix[3 * (size_t)j + c];
      if (k >= n_normals)
        return tri + (normal_indices ? "normal_indices[" : "indices[") + std::to_string(c) + "] must be < n_normals = " + std::to_string(n_normals) + " (got " + std::to_string(k) + ")";
      const std::string fault = normal_fault(k, normals + 3 * (size_t)k);
      if (!fault.empty()) return tri + fault;
    }
  return "";
}

// The world normals per corner in triangle order, nine floats per triangle: each n / sqrtf(dot(n, n)) by a disc normal's
// expressions (ptscene::normalise).  Call on normals check_normals() accepted.
inline void corner_normals(uint32_t n_triangles, const uint32_t* indices, const float* normals, const uint32_t* normal_indices,
                           std::vector<float>& out) {
  const uint32_t* ix = normal_indices ? normal_indices : indices;
  out.resize(9 * (size_t)n_triangles);
  for (size_t e = 0; e < 3 * (size_t)n_triangles; ++e) {
    const float* v = normals + 3 * (size_t)ix[e];
    volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    volatile float d0 = xx + yy, d1 = d0 + zz;
    volatile float len = sqrtf(d1);
    for (int k = 0; k < 3; ++k) out[3 * e + k] = v[k] / len;
  }
}

// The corner normals as the kernel reads them: three vectors per slot in leaf order (orig: slot -> triangle), each a direction
// through the camera's transform from its world value (cam == nullptr: the world value as it is).
inline void slot_normals(const float* corner, const uint32_t* orig, size_t n_triangles, const ptcamera::Basis* cam, F4* out) {
  for (size_t s = 0; s < n_triangles; ++s)
    for (int c = 0; c < 3; ++c) {
      const float* w = corner + 9 * (size_t)orig[s] + 3 * c;
      float o[3] = {w[0], w[1], w[2]};
      if (cam) ptcamera::to_camera_direction(*cam, w, o);
      out[3 * s + c] = F4{o[0], o[1], o[2], 0.f};
    }
}

// ---- textures (pt_set_mesh_texture, include/ptmi.h)

// The checks of pt_set_mesh_texture that need no device, in the contract's order; "" if the texture is valid.  indices: the mesh's
// own [n_triangles][3] (used when uv_indices is null: per-vertex uvs).  Only referenced uvs are examined.
inline std::string check_texture(uint32_t mesh, uint32_t n_vertices, uint32_t n_triangles, const uint32_t* indices, const pt_mesh_texture* t) {
  const std::string at = "mesh " + std::to_string(mesh) + ": ";
  if (t->struct_size != sizeof(pt_mesh_texture))
    return at + "texture: struct_size must be " + std::to_string(sizeof(pt_mesh_texture)) + " (got " + std::to_string(t->struct_size) + ")";
  if (t->width < 1 || t->width > PT_MESH_TEXTURE_MAX_SIZE || t->height < 1 || t->height > PT_MESH_TEXTURE_MAX_SIZE)
    return at + "texture: width and height must be in 1.." + std::to_string(PT_MESH_TEXTURE_MAX_SIZE) + " (got " + std::to_string(t->width) + " x " + std::to_string(t->height) + ")";
  if (t->filter != PT_TEX_FILTER_NEAREST && t->filter != PT_TEX_FILTER_BILINEAR)
    return at + "texture: filter must be 0 (nearest) or 1 (bilinear) (got " + std::to_string(t->filter) + ")";
  if (t->wrap != PT_TEX_WRAP_REPEAT && t->wrap != PT_TEX_WRAP_CLAMP)
    return at + "texture: wrap must be 0 (repeat) or 1 (clamp) (got " + std::to_string(t->wrap) + ")";
  if (!t->bgr) return at + "texture: null bgr";
  if (!t->uvs) return at + "texture: null uvs with n_uvs = " + std::to_string(t->n_uvs);
  if (!t->uv_indices && t->n_uvs != n_vertices)
    return at + "texture: n_uvs must equal n_vertices = " + std::to_string(n_vertices) + " when uv_indices is null (got " + std::to_string(t->n_uvs) + ")";
  for (uint32_t r = 0; r < t->height; ++r)
    for (uint32_t c = 0; c < t->width; ++c)
      for (int k = 0; k < 3; ++k) {
        const float v = t->bgr[3 * ((size_t)r * t->width + c) + k];
        if (!std::isfinite(v) || v < 0.f)
          return at + "texture: texel (row " + std::to_string(r) + ", column " + std::to_string(c) + ") channel " + std::to_string(k) +
                 " must be finite and >= 0 (got " + ptscene::num(v) + ")";
      }
  const uint32_t* ix = t->uv_indices ? t->uv_indices : indices;
  for (uint32_t j = 0; j < n_triangles; ++j)
    for (int c = 0; c < 3; ++c) {
      const std::string tri = at + "triangle " + std::to_string(j) + ": ";
      const uint32_t k = ix[3 * (size_t)j + c];
      if (k >= t->n_uvs)
        return tri + (t->uv_indices ? "uv_indices[" : "indices[") + std::to_string(c) + "] must be < n_uvs = " + std::to_string(t->n_uvs) + " (got " + std::to_string(k) + ")";
      for (int q = 0; q < 2; ++q)
        if (!std::isfinite(t->uvs[2 * (size_t)k + q])) return tri + "uvs[" + std::to_string(k) + "] must be finite (got " + ptscene::num(t->uvs[2 * (size_t)k + q]) + ")";
    }
  return "";
}

// The (s, t) per corner in triangle order, six floats per triangle.  Call on a texture check_texture() accepted.
inline void corner_uvs(uint32_t n_triangles, const uint32_t* indices, const float* uvs, const uint32_t* uv_indices, std::vector<float>& out) {
  const uint32_t* ix = uv_indices ? uv_indices : indices;
  out.resize(6 * (size_t)n_triangles);
  for (size_t e = 0; e < 3 * (size_t)n_triangles; ++e) {
    out[2 * e] = uvs[2 * (size_t)ix[e]];
    out[2 * e + 1] = uvs[2 * (size_t)ix[e] + 1];
  }
}

// The corner uvs as the kernel reads them: six floats per slot in leaf order (orig: slot -> triangle).  No frame applies to them.
inline void slot_uvs(const float* corner, const uint32_t* orig, size_t n_triangles, float* out) {
  for (size_t s = 0; s < n_triangles; ++s)
    for (int k = 0; k < 6; ++k) out[6 * s + k] = corner[6 * (size_t)orig[s] + k];
}

// The image as the kernel reads it: one (B, G, R, 0) vector per texel.
inline void texel_vectors(const pt_mesh_texture* t, std::vector<F4>& out) {
  const size_t n = (size_t)t->width * t->height;
  out.resize(n);
  for (size_t i = 0; i < n; ++i) out[i] = F4{t->bgr[3 * i], t->bgr[3 * i + 1], t->bgr[3 * i + 2], 0.f};
}

// ---- frames: twelve floats per triangle, v0, e1, e2, n

constexpr size_t kFrameFloats = 12;

// World space, exactly as a PT_SHAPE_TRIANGLE object's: e1 = v1 - v0, e2 = v2 - v0 and n = c / sqrtf(dot(c, c)) from
// ptscene::poly_frame (every intermediate a rounded binary32).  Appends M.n_triangles frames; call on a mesh check() accepted.
inline void world_frames(const pt_mesh& M, std::vector<float>& out) {
  for (uint32_t j = 0; j < M.n_triangles; ++j) {
    float v[3][3];
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k) v[c][k] = M.vertices[3 * (size_t)M.indices[3 * (size_t)j + c] + k];
    const ptscene::PolyFrame f = ptscene::poly_frame(v);
    volatile float len = sqrtf(f.cc);
    float fr[kFrameFloats];
    for (int k = 0; k < 3; ++k) { fr[k] = v[0][k]; fr[3 + k] = f.e1[k]; fr[6 + k] = f.e2[k]; fr[9 + k] = f.c[k] / len; }
    out.insert(out.end(), fr, fr + kFrameFloats);
  }
}

// The frames as the kernel sees them: v0 a point, e1, e2 and n directions through the camera's transform, from the world
// values -- what fill_scene does to a polygon.  cam == nullptr (the built-in camera): the world values as they are.
inline void kernel_frames(const float* world, size_t n_triangles, const ptcamera::Basis* cam, float* out) {
  if (!cam) { memcpy(out, world, n_triangles * kFrameFloats * sizeof(float)); return; }
  for (size_t j = 0; j < n_triangles; ++j) {
    const float* w = world + j * kFrameFloats;
    float* o = out + j * kFrameFloats;
    ptcamera::to_camera_point(*cam, w, o);
    ptcamera::to_camera_direction(*cam, w + 3, o + 3);
    ptcamera::to_camera_direction(*cam, w + 6, o + 6);
    ptcamera::to_camera_direction(*cam, w + 9, o + 9);
  }
}

// ---- the builder

struct Built {
  std::vector<Node> nodes;        // depth-first, boxes padded
  std::vector<F4> tris;           // three per slot
  std::vector<uint32_t> orig;     // slot -> triangle index
  uint32_t max_leaf = 0, depth = 0;
  float pad = 0.f;
};

struct Box {
  float lo[3], hi[3];
  void clear() { for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; } }
  void grow(const float* p) { for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); } }
  void grow(const Box& b) { grow(b.lo); grow(b.hi); }
  float half_area() const {
    const float x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
    return x * y + y * z + z * x;
  }
};

// A triangle's box: min / max of v0, v0 + e1, v0 + e2, one rounded add each.
inline Box tri_box(const float* fr) {
  Box b;
  b.clear();
  float p1[3], p2[3];
  for (int k = 0; k < 3; ++k) {
    volatile float a = fr[k] + fr[3 + k], c = fr[k] + fr[6 + k];
    p1[k] = a; p2[k] = c;
  }
  b.grow(fr); b.grow(p1); b.grow(p2);
  return b;
}

class Builder {
 public:
  Builder(const float* frames, uint32_t n_triangles, Built& out, float pad_scale, uint32_t max_depth = kMaxDepthSah)
      : fr_(frames), n_(n_triangles), out_(out), pad_scale_(pad_scale), max_depth_(max_depth) {}

  void run() {
    out_ = Built{};
    boxes_.resize(n_);
    centre_.resize(3 * (size_t)n_);
    idx_.resize(n_);
    for (uint32_t j = 0; j < n_; ++j) {
      boxes_[j] = tri_box(fr_ + kFrameFloats * (size_t)j);
      for (int k = 0; k < 3; ++k) centre_[3 * (size_t)j + k] = 0.5f * (boxes_[j].lo[k] + boxes_[j].hi[k]);
      idx_[j] = j;
    }
    out_.nodes.reserve(2 * (size_t)n_);
    out_.tris.reserve(3 * (size_t)n_);
    out_.orig.reserve(n_);
    node(0, n_, 1);
    // the pad, one value per mesh, from the root's box before padding
    float big = 0.f;
    for (int k = 0; k < 3; ++k) big = std::max(big, std::max(std::fabs(out_.nodes[0].lo[k]), std::fabs(out_.nodes[0].hi[k])));
    out_.pad = pad_scale_ * big;
    for (Node& N : out_.nodes)
      for (int k = 0; k < 3; ++k) {
        volatile float lo = N.lo[k] - out_.pad, hi = N.hi[k] + out_.pad;
        N.lo[k] = lo; N.hi[k] = hi;
      }
  }

 private:
  // Emits the subtree over idx_[b, e) and returns nothing: its nodes are out_.nodes[first .. size) when it comes back.
  void node(uint32_t b, uint32_t e, uint32_t depth) {
    const uint32_t self = (uint32_t)out_.nodes.size();
    out_.depth = std::max(out_.depth, depth);
    Box box;
    box.clear();
    for (uint32_t i = b; i < e; ++i) box.grow(boxes_[idx_[i]]);
    Node N{};
    for (int k = 0; k < 3; ++k) { N.lo[k] = box.lo[k]; N.hi[k] = box.hi[k]; }
    out_.nodes.push_back(N);
    const uint32_t count = e - b;
    if (count <= kMaxLeaf) {
      const uint32_t first = (uint32_t)out_.orig.size();
      for (uint32_t i = b; i < e; ++i) {
        const uint32_t j = idx_[i];
        const float* f = fr_ + kFrameFloats * (size_t)j;
        out_.tris.push_back(F4{f[0], f[1], f[2], f[3]});
        out_.tris.push_back(F4{f[4], f[5], f[6], f[7]});
        out_.tris.push_back(F4{f[8], f[9], f[10], f[11]});
        out_.orig.push_back(j);
      }
      out_.max_leaf = std::max(out_.max_leaf, count);
      out_.nodes[self].leaf = first << kLeafCountBits | count;
      out_.nodes[self].skip = self + 1u;
      return;
    }
    uint32_t mid = depth < max_depth_ ? sah_split(b, e) : b;
    if (mid <= b || mid >= e) mid = b + count / 2;   // no split by SAH: halve the range as it lies
    node(b, mid, depth + 1);
    node(mid, e, depth + 1);
    out_.nodes[self].leaf = 0u;
    out_.nodes[self].skip = (uint32_t)out_.nodes.size();
  }

  // Binned SAH over the centroids of idx_[b, e): partitions the range (stably) and returns the first index of the right part,
  // or b when no axis offers a split.
  uint32_t sah_split(uint32_t b, uint32_t e) {
    Box cb;
    cb.clear();
    for (uint32_t i = b; i < e; ++i) cb.grow(&centre_[3 * (size_t)idx_[i]]);
    float best_cost = INFINITY;
    int best_axis = -1, best_bin = 0;
    for (int axis = 0; axis < 3; ++axis) {
      const float ext = cb.hi[axis] - cb.lo[axis];
      if (!(ext > 0.f) || !std::isfinite(ext)) continue;
      Box bin_box[kBins];
      uint32_t bin_n[kBins] = {};
      for (auto& bb : bin_box) bb.clear();
      for (uint32_t i = b; i < e; ++i) {
        const int k = bin_of(centre_[3 * (size_t)idx_[i] + axis], cb.lo[axis], ext);
        bin_box[k].grow(boxes_[idx_[i]]);
        bin_n[k] += 1;
      }
      float right_area[kBins];
      uint32_t right_n[kBins];
      Box acc;
      acc.clear();
      uint32_t cnt = 0;
      for (int k = kBins - 1; k > 0; --k) {
        if (bin_n[k]) acc.grow(bin_box[k]);
        cnt += bin_n[k];
        right_area[k] = cnt ? acc.half_area() : 0.f;
        right_n[k] = cnt;
      }
      acc.clear();
      cnt = 0;
      for (int k = 1; k < kBins; ++k) {   // split: bins < k to the left
        if (bin_n[k - 1]) acc.grow(bin_box[k - 1]);
        cnt += bin_n[k - 1];
        if (cnt == 0 || right_n[k] == 0) continue;
        const float cost = acc.half_area() * (float)cnt + right_area[k] * (float)right_n[k];
        if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = k; }
      }
    }
    if (best_axis < 0) return b;
    const float lo = cb.lo[best_axis], ext = cb.hi[best_axis] - cb.lo[best_axis];
    auto mid = std::stable_partition(idx_.begin() + b, idx_.begin() + e, [&](uint32_t j) {
      return bin_of(centre_[3 * (size_t)j + best_axis], lo, ext) < best_bin;
    });
    return (uint32_t)(mid - idx_.begin());
  }

  static int bin_of(float c, float lo, float ext) {
    const int k = (int)((float)kBins * ((c - lo) / ext));
    return k < 0 ? 0 : (k >= kBins ? kBins - 1 : k);
  }

  const float* fr_;
  uint32_t n_;
  Built& out_;
  float pad_scale_;
  uint32_t max_depth_;
  std::vector<Box> boxes_;
  std::vector<float> centre_;
  std::vector<uint32_t> idx_;
};

// The tree over n_triangles frames in the kernel's frame (n_triangles >= 1).  pad_scale: the library always takes the default;
// tests/mesh_bvh_main.cpp builds one exact fixture with 0, where boxes without a margin show the walk's NaN and tie rules.
// max_depth: the depth from which ranges are halved as they lie; the library always takes the default -- 48 levels are out of
// reach of small valid fixtures in binary32, so tests/mesh_sah_main.cpp exercises the cap at 2 and 3.
inline void build(const float* frames, uint32_t n_triangles, Built& out, float pad_scale = kPadScale, uint32_t max_depth = kMaxDepthSah) {
  Builder(frames, n_triangles, out, pad_scale, max_depth).run();
}

}  // namespace ptmesh
