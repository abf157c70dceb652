// ptmi_camera.h -- validation of a runtime camera and its orthonormal basis (pt_set_camera, include/ptmi.h).
// Plain C++ on purpose, like ptmi_scene.h: the library (ptmi.hip) and the CLI (host/PathTracerApp.cpp, --scene with a "camera")
// both include it, so a bad file is refused before any device is attached with the very message the library would give.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "ptmi.h"
#include "ptmi_scene.h"

namespace ptcamera {

inline pt_camera default_camera() {
  pt_camera c{};
  c.struct_size = sizeof(pt_camera);
  c.position[0] = c.position[1] = c.position[2] = 0.f;
  c.look_at[0] = 0.f; c.look_at[1] = 0.f; c.look_at[2] = -1.f;
  c.up[0] = 0.f; c.up[1] = 1.f; c.up[2] = 0.f;
  c.lens_radius = 0.f;
  c.focus_distance = 1.f;
  return c;
}

// Every intermediate a rounded binary32 (volatile: whatever the host's FLT_EVAL_METHOD and contraction), left to right as the
// device's dot / cross / normalise (pt_device_math.h).
inline void normalise3(const float* v, float* out) {
  volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  volatile float d0 = xx + yy, d1 = d0 + zz;
  volatile float len = sqrtf(d1);
  for (int k = 0; k < 3; ++k) { volatile float q = v[k] / len; out[k] = q; }
}
inline void cross3(const float* a, const float* b, float* out) {
  volatile float p0 = a[1] * b[2], q0 = a[2] * b[1], r0 = p0 - q0;
  volatile float p1 = a[2] * b[0], q1 = a[0] * b[2], r1 = p1 - q1;
  volatile float p2 = a[0] * b[1], q2 = a[1] * b[0], r2 = p2 - q2;
  out[0] = r0; out[1] = r1; out[2] = r2;
}
inline float dot3(const float* a, const float* b) {
  volatile float xx = a[0] * b[0], yy = a[1] * b[1], zz = a[2] * b[2];
  volatile float d0 = xx + yy, d1 = d0 + zz;
  return d1;
}

// v times the power of two that brings its largest component into [0.5, 1).  Exact, and normalise(v 2^k) is normalise(v) bit for
// bit wherever the latter neither overflows nor underflows; so any finite vector of non-zero length can be squared in binary32.
// Returns false for the zero vector (out = v).
inline bool scale_pow2(const float* v, float* out) {
  float m = 0.f;
  for (int k = 0; k < 3; ++k) m = fabsf(v[k]) > m ? fabsf(v[k]) : m;
  int e = 0;
  if (m > 0.f) (void)frexpf(m, &e);
  for (int k = 0; k < 3; ++k) out[k] = ldexpf(v[k], -e);
  return m > 0.f;
}

// The camera's frame: a camera-space vector (x, y, z) is the world vector x r + y u - z f.
struct Basis {
  float r[3], u[3], f[3];
  float position[3];
  bool identity;   // r, u, f = +x, +y, -z and position = 0: the built-in camera, for which no transform is applied at all
};

// f = normalise(look_at - position), r = normalise(cross(f, up)), u = cross(r, f); look_at - position and up go through
// scale_pow2 first (the same bits, any length).  Call on a camera check() accepted.
inline Basis basis(const pt_camera& c) {
  Basis B;
  float d[3], up[3];
  for (int k = 0; k < 3; ++k) { volatile float s = c.look_at[k] - c.position[k]; d[k] = s; B.position[k] = c.position[k]; }
  scale_pow2(d, d);
  scale_pow2(c.up, up);
  normalise3(d, B.f);
  float x[3];
  cross3(B.f, up, x);
  normalise3(x, B.r);
  cross3(B.r, B.f, B.u);
  B.identity = B.r[0] == 1.f && B.r[1] == 0.f && B.r[2] == 0.f && B.u[0] == 0.f && B.u[1] == 1.f && B.u[2] == 0.f &&
               B.f[0] == 0.f && B.f[1] == 0.f && B.f[2] == -1.f && c.position[0] == 0.f && c.position[1] == 0.f && c.position[2] == 0.f;
  return B;
}

// World point -> camera space, R^T (p - position); world direction -> camera space, R^T n.
inline void to_camera_direction(const Basis& B, const float* n, float* out) {
  out[0] = dot3(B.r, n);
  out[1] = dot3(B.u, n);
  volatile float z = 0.f - dot3(B.f, n);
  out[2] = z;
}
inline void to_camera_point(const Basis& B, const float* p, float* out) {
  float d[3];
  for (int k = 0; k < 3; ++k) { volatile float s = p[k] - B.position[k]; d[k] = s; }
  to_camera_direction(B, d, out);
}

// "" if the camera is valid, else what is wrong, naming the field.
inline std::string check(const pt_camera* cam) {
  if (!cam) return "camera: null camera";
  const pt_camera& c = *cam;
  if (c.struct_size != sizeof(pt_camera))
    return "camera: struct_size must be " + std::to_string(sizeof(pt_camera)) + " (got " + std::to_string(c.struct_size) + ")";
  const struct { const char* name; const float* v; int k; } fields[] = {
      {"position", c.position, 3}, {"look_at", c.look_at, 3}, {"up", c.up, 3}, {"lens_radius", &c.lens_radius, 1},
      {"focus_distance", &c.focus_distance, 1}};
  for (const auto& f : fields)
    for (int k = 0; k < f.k; ++k)
      if (!std::isfinite(f.v[k])) return std::string("camera: ") + f.name + " must be finite (got " + ptscene::num(f.v[k]) + ")";
  float d[3];
  for (int k = 0; k < 3; ++k) { volatile float s = c.look_at[k] - c.position[k]; d[k] = s; }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(d[k])) return "camera: look_at - position must be finite (got " + ptscene::num(d[k]) + ")";
  float up[3];
  // lengths are taken after scaling by a power of two: no finite input overflows or underflows in the squares
  if (!scale_pow2(d, d)) return "camera: look_at must differ from position";
  if (!scale_pow2(c.up, up)) return "camera: up must have a non-zero length";
  float f[3], un[3], x[3];
  normalise3(d, f);
  normalise3(up, un);
  cross3(f, un, x);
  const float s = sqrtf(dot3(x, x));
  if (!(s >= 1e-3f)) return "camera: up must not be parallel to the view direction look_at - position (|cross(f, up/|up|)| = " + ptscene::num(s) + " < 1e-3)";
  if (c.lens_radius < 0.f) return "camera: lens_radius must be >= 0 (got " + ptscene::num(c.lens_radius) + ")";
  if (c.lens_radius > 0.f && !(c.focus_distance > 0.f))
    return "camera: focus_distance must be > 0 when lens_radius > 0 (got " + ptscene::num(c.focus_distance) + ")";
  return "";
}

}  // namespace ptcamera
