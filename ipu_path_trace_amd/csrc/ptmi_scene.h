// ptmi_scene.h -- validation and host-side normalisation of a runtime scene table (pt_set_scene, include/ptmi.h).
// Plain C++ on purpose: the library (ptmi.hip) and the CLI (host/PathTracerApp.cpp, --scene) both include it, so a bad
// scene file is refused before any device is attached with the very message the library would give.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
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

}  // namespace ptscene
