// pt_mesh_update.h -- a mesh's world frames and corner normals made again from new vertices (pt_update_mesh_vertices,
// include/ptmi.h), written ONCE for the kernels (ptmi_mesh_update.h), the host and the test program: the functions behind
// PT_MESH_HD hold no HIP type, so tests/mesh_update_main.cpp compiles them with g++ alone.  Compile with -ffp-contract=off like
// everything else here: every operation below is one rounded binary32.
//
// THE RULE.  frame_thread is ptscene::poly_frame followed by ptmesh::world_frames, expression for expression:
//   e1 = v1 - v0, e2 = v2 - v0;  c[k] = e1[i] e2[j] - e1[j] e2[i] (i = k + 1, j = k + 2 mod 3), the two products rounded before
//   the difference;  cc = ((c0 c0 + c1 c1) + c2 c2);  n = c / sqrtf(cc).
// Its twelve floats are world_frames' bytes on the same input.  A triangle's status follows ptmesh::check's order: a referenced
// vertex that is not finite; then e1, e2 or c not finite; then cc not > 0 and finite.  corner_normals_thread is
// ptmesh::corner_normals for one triangle, its status ptmesh::check_normals': a referenced normal that is not finite, or whose
// dot(n, n) is not > 0 and finite -- the first offending corner decides.
//
// THE FIRST FAULT.  A pass over a mesh reports its LOWEST offending triangle, as a loop in index order would: each offending
// triangle gives the word index << 32 | status, a triangle without a fault gives kNoFault, and words combine by their minimum --
// an integer minimum, exact in any order.
#pragma once
#include <cmath>
#include <cstdint>

#include "pt_mesh.h"

namespace ptupdate {

enum : uint32_t {
  kStatusOk = 0,
  kVertexNotFinite = 1,    // "vertices[i] must be finite"
  kFrameNotFinite = 2,     // "vertex differences and their cross product must be finite"
  kCollinear = 3,          // "vertices are collinear"
  kNormalNotFinite = 4,    // "normals[i] must be finite"
  kNormalNoLength = 5,     // "normals[i] must have a finite dot(n, n) > 0"
};
constexpr uint64_t kNoFault = ~0ull;
constexpr uint32_t kFrameFloats = 12;   // v0, e1, e2, n = ptmesh::kFrameFloats

PT_MESH_HD bool finite32(float x) {   // std::isfinite, spelled on the bits: one answer on the host and the device
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return (u & 0x7f800000u) != 0x7f800000u;
}

PT_MESH_HD uint64_t fault_word(uint32_t triangle, uint32_t status) {
  return status == kStatusOk ? kNoFault : ((uint64_t)triangle << 32 | status);
}
PT_MESH_HD uint32_t fault_triangle(uint64_t word) { return (uint32_t)(word >> 32); }
PT_MESH_HD uint32_t fault_status(uint64_t word) { return (uint32_t)word; }
// Two passes' words into one: the lower triangle's.
PT_MESH_HD uint64_t combine(uint64_t a, uint64_t b) {
#if defined(PT_MESH_UPDATE_MUTATE_ANY)   // (tests/mesh_update_main.cpp: the mutation must fail the test)
  return b != kNoFault ? b : a;
#else
  return b < a ? b : a;
#endif
}

// Triangle j of a mesh with corner indices `indices` ([n_triangles][3], each < n_vertices) over `vertices` ([n_vertices][3]):
// its frame into fr[12], and its status.  The frame of a triangle with a fault is written too, and is never used.
PT_MESH_HD uint32_t frame_thread(uint32_t j, const uint32_t* indices, const float* vertices, float* fr) {
  float v[3][3];
  bool vertex_ok = true;
  for (int c = 0; c < 3; ++c) {
    const float* p = vertices + 3 * (size_t)indices[3 * (size_t)j + c];
    for (int k = 0; k < 3; ++k) { v[c][k] = p[k]; vertex_ok = vertex_ok && finite32(p[k]); }
  }
  float e1[3], e2[3], c[3];
  for (int k = 0; k < 3; ++k) {
    e1[k] = v[1][k] - v[0][k];
#if defined(PT_MESH_UPDATE_MUTATE_EDGE)
    e2[k] = v[2][k] - v[1][k];
#else
    e2[k] = v[2][k] - v[0][k];
#endif
  }
  bool frame_ok = true;
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, q = (k + 2) % 3;
    const float a = e1[i] * e2[q], b = e1[q] * e2[i];
    c[k] = a - b;
    frame_ok = frame_ok && finite32(e1[k]) && finite32(e2[k]);
  }
  for (int k = 0; k < 3; ++k) frame_ok = frame_ok && finite32(c[k]);
  const float xx = c[0] * c[0], yy = c[1] * c[1], zz = c[2] * c[2];
  const float d0 = xx + yy, cc = d0 + zz;
  const float len = sqrtf(cc);
  for (int k = 0; k < 3; ++k) { fr[k] = v[0][k]; fr[3 + k] = e1[k]; fr[6 + k] = e2[k]; fr[9 + k] = c[k] / len; }
  if (!vertex_ok) return kVertexNotFinite;
  if (!frame_ok) return kFrameNotFinite;
  if (!(cc > 0.f) || !finite32(cc)) return kCollinear;
  return kStatusOk;
}

// Triangle j's three corner normals, looked up by `normal_indices` ([n_triangles][3], each < n_normals: the mesh's own corner
// indices for per-vertex normals) in `normals` ([n_normals][3]): nine floats into out, each n / sqrtf(dot(n, n)), and the status.
PT_MESH_HD uint32_t corner_normals_thread(uint32_t j, const uint32_t* normal_indices, const float* normals, float* out) {
  uint32_t status = kStatusOk;
  for (int c = 0; c < 3; ++c) {
    const float* v = normals + 3 * (size_t)normal_indices[3 * (size_t)j + c];
    const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    const float d0 = xx + yy, d1 = d0 + zz;
    const float len = sqrtf(d1);
    for (int k = 0; k < 3; ++k) out[3 * c + k] = v[k] / len;
    if (status != kStatusOk) continue;
    if (!finite32(v[0]) || !finite32(v[1]) || !finite32(v[2])) status = kNormalNotFinite;
    else if (!(d1 > 0.f) || !finite32(d1)) status = kNormalNoLength;
  }
  return status;
}

// The passes one triangle after the other (the kernels run the same functions, one thread per triangle): the frames of all
// triangles into `frames`, and the first fault's word.
inline uint64_t frames_pass(uint32_t n_triangles, const uint32_t* indices, const float* vertices, float* frames) {
  uint64_t word = kNoFault;
  for (uint32_t j = 0; j < n_triangles; ++j)
    word = combine(word, fault_word(j, frame_thread(j, indices, vertices, frames + (size_t)kFrameFloats * j)));
  return word;
}
inline uint64_t corner_normals_pass(uint32_t n_triangles, const uint32_t* normal_indices, const float* normals, float* corner) {
  uint64_t word = kNoFault;
  for (uint32_t j = 0; j < n_triangles; ++j)
    word = combine(word, fault_word(j, corner_normals_thread(j, normal_indices, normals, corner + 9 * (size_t)j)));
  return word;
}

}  // namespace ptupdate
