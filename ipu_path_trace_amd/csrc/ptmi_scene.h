// ptmi_scene.h -- validation and host-side normalisation of a runtime scene table (pt_set_scene, pt_set_scene_ex, include/ptmi.h).
// Plain C++ on purpose: the library (ptmi.hip) and the CLI (host/PathTracerApp.cpp, --scene) both include it, so a bad
// scene file is refused before any device is attached with the very message the library would give.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "ptmi.h"

namespace ptscene {

inline std::string num(float v) {
  char buf[48];
  snprintf(buf, sizeof buf, "%.9g", (double)v);
  return buf;
}

// "" if the table is valid, else what is wrong, naming the object's index and the field.
inline std::string check(const pt_scene_object* objs, uint32_t n) {
  if (n < 1 || n > PT_MAX_SCENE_OBJECTS)
    return "scene: object count must be 1.." + std::to_string(PT_MAX_SCENE_OBJECTS) + " (got " + std::to_string(n) + ")";
  if (!objs) return "scene: null object table";
  for (uint32_t i = 0; i < n; ++i) {
    const pt_scene_object& o = objs[i];
    const std::string at = "scene object " + std::to_string(i) + ": ";
    if (o.shape != PT_SHAPE_SPHERE && o.shape != PT_SHAPE_DISC)
      return at + "shape must be 0 (sphere) or 1 (disc) (got " + std::to_string(o.shape) + ")";
    if (o.material < PT_MATERIAL_DIFFUSE || o.material > PT_MATERIAL_EMISSIVE)
      return at + "material must be 0 (diffuse), 1 (specular), 2 (refractive) or 3 (emissive) (got " + std::to_string(o.material) + ")";
    const struct { const char* name; const float* v; int k; } fields[] = {
        {"centre", o.centre, 3}, {"radius", &o.radius, 1}, {"normal", o.normal, 3}, {"colour", o.colour, 3}};
    for (const auto& f : fields)
      for (int k = 0; k < f.k; ++k)
        if (!std::isfinite(f.v[k])) return at + f.name + " must be finite (got " + num(f.v[k]) + ")";
    if (!(o.radius > 0.f)) return at + "radius must be > 0 (got " + num(o.radius) + ")";
    for (int k = 0; k < 3; ++k)
      if (o.colour[k] < 0.f) return at + "colour components must be >= 0 (got " + num(o.colour[k]) + ")";
    if (o.shape == PT_SHAPE_DISC) {
      const float nn = o.normal[0] * o.normal[0] + o.normal[1] * o.normal[1] + o.normal[2] * o.normal[2];
      if (!(nn > 0.f) || !std::isfinite(nn)) return at + "disc normal must have a non-zero finite length";
    }
  }
  return "";
}

// The table as stored: disc normals n / sqrtf(dot(n, n)) in binary32 (volatile: every intermediate a rounded float whatever
// the host's FLT_EVAL_METHOD), sphere normals 0.  Call on a table check() accepted.
inline void normalise(pt_scene_object* objs, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    float* v = objs[i].normal;
    if (objs[i].shape != PT_SHAPE_DISC) { v[0] = v[1] = v[2] = 0.f; continue; }
    volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    volatile float d0 = xx + yy, d1 = d0 + zz;
    volatile float len = sqrtf(d1);
    for (int k = 0; k < 3; ++k) v[k] = v[k] / len;
  }
}

// ---- pt_set_scene_ex: the same with triangles and parallelograms (include/ptmi.h)

inline bool is_polygon(int32_t shape) { return shape == PT_SHAPE_TRIANGLE || shape == PT_SHAPE_PARALLELOGRAM; }

// A polygon's edges e1 = v1 - v0, e2 = v2 - v0 and c = cross(e1, e2), cc = dot(c, c), in binary32 (volatile: every intermediate a
// rounded float, the sums left to right).
struct PolyFrame {
  float e1[3], e2[3], c[3], cc;
};
inline PolyFrame poly_frame(const float (&v)[3][3]) {
  PolyFrame f;
  for (int k = 0; k < 3; ++k) {
    volatile float a = v[1][k] - v[0][k], b = v[2][k] - v[0][k];
    f.e1[k] = a; f.e2[k] = b;
  }
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    volatile float p = f.e1[i] * f.e2[j], q = f.e1[j] * f.e2[i];
    volatile float d = p - q;
    f.c[k] = d;
  }
  volatile float xx = f.c[0] * f.c[0], yy = f.c[1] * f.c[1], zz = f.c[2] * f.c[2];
  volatile float d0 = xx + yy, d1 = d0 + zz;
  f.cc = d1;
  return f;
}

// "" if the ex table is valid, else what is wrong, in the order include/ptmi.h states.  max_shape = PT_SHAPE_MESH
// (pt_set_scene_meshes alone): a row of shape 4 passes, checked for its material and colour only.
inline std::string check_ex(const pt_scene_object_ex* objs, uint32_t n, uint32_t stride, int32_t max_shape = PT_SHAPE_PARALLELOGRAM) {
  if (stride != sizeof(pt_scene_object_ex))
    return "scene: stride must be " + std::to_string(sizeof(pt_scene_object_ex)) + " (sizeof(pt_scene_object_ex)) (got " + std::to_string(stride) + ")";
  if (n < 1 || n > PT_MAX_SCENE_OBJECTS)
    return "scene: object count must be 1.." + std::to_string(PT_MAX_SCENE_OBJECTS) + " (got " + std::to_string(n) + ")";
  if (!objs) return "scene: null object table";
  for (uint32_t i = 0; i < n; ++i) {
    const pt_scene_object_ex& o = objs[i];
    const std::string at = "scene object " + std::to_string(i) + ": ";
    if (o.shape < PT_SHAPE_SPHERE || o.shape > max_shape)
      return at + (max_shape == PT_SHAPE_MESH ? "shape must be 0 (sphere), 1 (disc), 2 (triangle), 3 (parallelogram) or 4 (mesh) (got "
                                              : "shape must be 0 (sphere), 1 (disc), 2 (triangle) or 3 (parallelogram) (got ") + std::to_string(o.shape) + ")";
    if (o.material < PT_MATERIAL_DIFFUSE || o.material > PT_MATERIAL_EMISSIVE)
      return at + "material must be 0 (diffuse), 1 (specular), 2 (refractive) or 3 (emissive) (got " + std::to_string(o.material) + ")";
    const bool poly = is_polygon(o.shape), mesh = o.shape == PT_SHAPE_MESH;
    const bool round = !poly && !mesh;   // a sphere or a disc
    const struct { const char* name; const float* v; int k; bool used; } fields[] = {
        {"centre", o.centre, 3, round}, {"radius", &o.radius, 1, round}, {"normal", o.normal, 3, round},
        {"vertex", &o.vertex[0][0], 9, poly}, {"colour", o.colour, 3, true}};
    for (const auto& f : fields)
      for (int k = 0; f.used && k < f.k; ++k)
        if (!std::isfinite(f.v[k])) return at + f.name + " must be finite (got " + num(f.v[k]) + ")";
    for (int k = 0; k < 3; ++k)
      if (o.colour[k] < 0.f) return at + "colour components must be >= 0 (got " + num(o.colour[k]) + ")";
    if (mesh) continue;   // its triangles are checked with the mesh table (ptmi_mesh.h)
    if (!poly) {
      if (!(o.radius > 0.f)) return at + "radius must be > 0 (got " + num(o.radius) + ")";
      if (o.shape == PT_SHAPE_DISC) {
        const float nn = o.normal[0] * o.normal[0] + o.normal[1] * o.normal[1] + o.normal[2] * o.normal[2];
        if (!(nn > 0.f) || !std::isfinite(nn)) return at + "disc normal must have a non-zero finite length";
      }
    } else {
      const PolyFrame f = poly_frame(o.vertex);
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(f.e1[k]) || !std::isfinite(f.e2[k]) || !std::isfinite(f.c[k]))
          return at + "vertex differences and their cross product must be finite";
      if (!(f.cc > 0.f) || !std::isfinite(f.cc)) return at + "vertices are collinear";
    }
  }
  return "";
}

// The ex table as stored: a sphere or disc as normalise() leaves it, with vertex = 0; a polygon with centre = v0, radius = 0
// and normal = c / sqrtf(dot(c, c)).  Call on a table check_ex() accepted.
inline void normalise_ex(pt_scene_object_ex* objs, uint32_t n) {
  for (uint32_t i = 0; i < n; ++i) {
    pt_scene_object_ex& o = objs[i];
    if (!is_polygon(o.shape)) {
      static_assert(offsetof(pt_scene_object_ex, vertex) == sizeof(pt_scene_object), "the first 48 bytes are pt_scene_object");
      pt_scene_object head;
      memcpy(&head, &o, sizeof head);
      normalise(&head, 1);
      memcpy(&o, &head, sizeof head);
      for (auto& v : o.vertex) v[0] = v[1] = v[2] = 0.f;
      continue;
    }
    const PolyFrame f = poly_frame(o.vertex);
    volatile float len = sqrtf(f.cc);
    for (int k = 0; k < 3; ++k) { o.centre[k] = o.vertex[0][k]; o.normal[k] = f.c[k] / len; }
    o.radius = 0.f;
  }
}

}  // namespace ptscene
