// ptmi_light_guide.h -- validation of an emitter guide and the construction of its table (pt_set_light_guide, include/ptmi.h).
// Plain C++ on purpose, like ptmi_scene.h and ptmi_env_guide.h: the library (ptmi.hip), the CLI (host/PathTracerApp.cpp,
// --light-guide-beta) and a stand-alone test program (tests/light_guide_main.cpp) all include it, so a bad beta is refused
// before any device is attached with the very message the library would give.
//
// The emitters are the objects of the scene in force with PT_MATERIAL_EMISSIVE, in declaration order (K <= 32).  Emitter k has
// the binary64 mass m_k = Y(colour_k) a_k, Y the Rec. 709 luminance and a_k = 4 r^2 (sphere) or 2 r^2 (disc: it emits from both
// faces; the common pi is dropped).  A 32-bit word g1 selects the first k with g1 < c_k, c_k = floor(2^32 sum_{j<=k} m_j / sum m),
// else the last emitter of positive mass, which takes the rest.  p_k is made from the QUANTISED thresholds, an integer
// difference / 2^32: the density the kernel divides by is exactly the distribution it draws from, and the p_k sum to 1.
//
// Polygon lamps (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS): build() given the vertices of pt_set_scene_ex's table lists an
// emissive triangle or parallelogram too, in declaration order with the spheres and discs, a_k = 2 A_p / pi (two faces; the pi
// the others dropped), A_p = (double)S (parallelogram) or 0.5 (double)S (triangle), S = sqrtf(dot(c, c)), c = cross(e1, e2),
// the binary32 value the stored normal was divided by (ptmi_scene.h, poly_frame; world space).  Without vertices -- the
// four-argument call, pt_set_light_guide -- a polygon is skipped.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "ptmi.h"
#include "ptmi_scene.h"

namespace ptlight {

constexpr double kTwo32 = 4294967296.0;
constexpr double kSumSlack = 1e-6;   // alpha + beta is compared in binary64: 0.6f + 0.3f is 0.90000004, above 0.9f by rounding alone

struct Table {
  uint32_t n = 0;                                    // emitters of the scene, K
  uint32_t n_draw = 0;                               // ranks that can be drawn: up to the last emitter of positive mass; 0 = inert
  uint32_t beta_thr = 0;                             // (uint32)(beta 2^32)
  double beta = 0;                                   // beta_thr / 2^32, the beta used everywhere afterwards
  uint32_t object_index[PT_MAX_SCENE_OBJECTS] = {};  // rank -> index into the scene
  uint32_t threshold[PT_MAX_SCENE_OBJECTS] = {};     // c_k; 0xffffffff from the last emitter of positive mass on
  uint64_t weight[PT_MAX_SCENE_OBJECTS] = {};        // p_k 2^32, an integer; the weights sum to 2^32
  float probability[PT_MAX_SCENE_OBJECTS] = {};      // (float)(weight / 2^32)
  double mass[PT_MAX_SCENE_OBJECTS] = {};
  bool polygons = false;                             // a polygon is listed: the polygon-lamp kernel instances run
  bool active() const { return n_draw != 0; }
};

inline std::string num(double v) { char b[40]; snprintf(b, sizeof(b), "%g", v); return b; }

// "" if the guide's fields are valid, else what is wrong, naming the field.  alpha: that of an environment guide already set (0
// without one); the two probabilities share the hemisphere's.
inline std::string check(const pt_light_guide* g, double alpha = 0.0) {
  if (!g) return "light guide: null guide";
  if (g->struct_size != sizeof(pt_light_guide))
    return "light guide: struct_size must be " + std::to_string(sizeof(pt_light_guide)) + " (got " + std::to_string(g->struct_size) + ")";
  if (!(g->beta >= 0.f && g->beta <= PT_LIGHT_GUIDE_MAX_BETA))
    return "light guide: beta must be in [0, " + num(PT_LIGHT_GUIDE_MAX_BETA) + "] (got " + num(g->beta) + ")";
  if ((double)g->beta + alpha > (double)PT_LIGHT_GUIDE_MAX_BETA + kSumSlack)
    return "light guide: alpha + beta must not exceed " + num(PT_LIGHT_GUIDE_MAX_BETA) + " (the environment guide's alpha " + num(alpha) +
           " + beta " + num(g->beta) + ")";
  return "";
}

// The same for pt_set_light_guide_ex, in the order include/ptmi.h states: struct_size, beta, flags, the sum.
inline std::string check_ex(const pt_light_guide_ex* g, double alpha = 0.0) {
  if (!g) return "light guide: null guide";
  if (g->struct_size != sizeof(pt_light_guide_ex))
    return "light guide: struct_size must be " + std::to_string(sizeof(pt_light_guide_ex)) + " (got " + std::to_string(g->struct_size) + ")";
  const pt_light_guide plain{(uint32_t)sizeof(pt_light_guide), g->beta};
  const std::string bad = check(&plain, 0.0);   // beta alone
  if (!bad.empty()) return bad;
  if (g->flags & ~(uint32_t)PT_LIGHT_GUIDE_POLYGONS)
    return "light guide: flags must be 0 or PT_LIGHT_GUIDE_POLYGONS (1) (got " + std::to_string(g->flags) + ")";
  return check(&plain, alpha);
}

// S of a polygon: sqrtf(dot(c, c)), c = cross(e1, e2), every operation one rounded binary32 -- the length normalise_ex divides by.
inline float poly_area_s(const float (&vertex)[3][3]) {
  const ptscene::PolyFrame f = ptscene::poly_frame(vertex);
  volatile float len = sqrtf(f.cc);
  return len;
}

// The same sum, seen from pt_set_env_guide while a light guide is set.
inline std::string check_alpha(double alpha, double beta) {
  if (alpha + beta > (double)PT_LIGHT_GUIDE_MAX_BETA + kSumSlack)
    return "env guide: alpha + beta must not exceed " + num(PT_LIGHT_GUIDE_MAX_BETA) + " (alpha " + num(alpha) + " + the light guide's beta " +
           num(beta) + ")";
  return "";
}

// The table of a guide check() accepted over a scene ptscene::check() accepted (n <= PT_MAX_SCENE_OBJECTS).  vertex: the
// polygons' vertices (pt_set_scene_ex's table as stored) when polygon lamps are asked for, else nullptr: polygons are skipped.
inline void build(float beta, const pt_scene_object* scene, uint32_t n_objects, Table& T, const float (*vertex)[3][3] = nullptr) {
  T = Table{};
  T.beta_thr = (uint32_t)((double)beta * kTwo32);
  T.beta = (double)T.beta_thr / kTwo32;
  double total = 0.0;
  int last = -1;
  for (uint32_t i = 0; i < n_objects && T.n < PT_MAX_SCENE_OBJECTS; ++i) {
    if (scene[i].material != PT_MATERIAL_EMISSIVE) continue;
    const bool poly = ptscene::is_polygon(scene[i].shape);
    if (poly && !vertex) continue;   // an emissive polygon (pt_set_scene_ex) is not drawn from unless pt_set_light_guide_ex asks
    if (!poly && scene[i].shape != PT_SHAPE_SPHERE && scene[i].shape != PT_SHAPE_DISC) continue;
    const float* c = scene[i].colour;
    const double y = 0.2126 * (double)c[0] + 0.7152 * (double)c[1] + 0.0722 * (double)c[2];
    const double r = (double)scene[i].radius;
    double m = y * (scene[i].shape == PT_SHAPE_DISC ? 2.0 : 4.0) * r * r;
    if (poly) {
      const double S = (double)poly_area_s(vertex[i]);
      m = y * 2.0 * (scene[i].shape == PT_SHAPE_TRIANGLE ? 0.5 * S : S) / 3.14159265358979323846;
    }
    if (!(m > 0.0) || !std::isfinite(m)) m = 0.0;
    T.object_index[T.n] = i;
    T.polygons = T.polygons || poly;
    T.mass[T.n] = m;
    if (m > 0.0) last = (int)T.n;
    total += m;
    T.n += 1;
  }
  if (last < 0 || !(total > 0.0) || !std::isfinite(total)) return;   // no emitter, or none with mass: inert
  T.n_draw = (uint32_t)last + 1u;
  double cum = 0.0;
  uint64_t prev = 0;
  for (uint32_t k = 0; k < T.n; ++k) {
    uint64_t c = 1ull << 32;
    if ((int)k < last) {
      cum += T.mass[k];
      const double f = std::floor(kTwo32 * (cum / total));
      c = f >= kTwo32 ? 0xffffffffull : (uint64_t)f;
      if (c < prev) c = prev;
    }
    T.weight[k] = T.mass[k] > 0.0 ? c - prev : 0;   // (an emitter without mass has c == prev already)
    T.threshold[k] = c > 0xffffffffull ? 0xffffffffu : (uint32_t)c;
    T.probability[k] = (float)((double)T.weight[k] / kTwo32);
    prev = c;
  }
}

}  // namespace ptlight
