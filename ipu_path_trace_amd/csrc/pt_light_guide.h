// pt_light_guide.h -- device side of the emitter guide (pt_set_light_guide, include/ptmi.h): drawing a direction towards an
// emissive sphere or disc of the scene (or, where asked for, a triangle or parallelogram: POLYGON LAMPS below) and evaluating the density of such draws for any direction.  The table (emitter rank ->
// object index, threshold, probability) comes from ptmi_light_guide.h (host) and travels at the end of the kernel arguments
// (TraceParams::lights); the guided diffuse bounce that uses these functions is in pt_trace.h (shade_hit<.., LIGHTS = true>).
// Included by pt_trace.h once SceneObject, TraceParams and basis_about exist.  The functions are frame-free: the trace kernels
// call them in camera space on P.obj[], the two hooks at the end in world space on the world-space scene table.
//
// Densities are in units of the hemisphere's 1 / 2 pi, as the environment guide's.  Eligibility of an emitter at (x, n) is a
// function of (x, n) alone, the same when sampling and when evaluating.
//
// THE RIM RULE.  A lane that drew its direction from emitter k takes that emitter's term by construction and does not run the
// inside test for k; the test is used for every other emitter, and for all emitters when the direction came from the hemisphere
// or the environment guide.  Without the rule, binary32 rounding at the rim of a small far lamp would drop a term of size
// ~ 1 / s^2 from the denominator on a share ~ 6e-8 / (1 - cm) of the draws: a bias of percent size.  With it a misjudged rim
// only affects hemisphere draws within an ulp of the rim, whose weights are bounded by cos rr / (1 - alpha - beta).
//
// POLYGON LAMPS (pt_set_light_guide_ex, PT_LIGHT_GUIDE_POLYGONS; the PLAMPS instances alone compile this).  An emissive triangle
// or parallelogram v0 + a e1 + b e2 with stored normal m: a uniform point of its area, density l^2 / (|m . w| A_p) in solid angle,
// 2 pi l^2 / (|m . w| A_p) in the hemisphere's units.  A_p = S (parallelogram) or 0.5 S (triangle), S = |e1 x e2| as the host
// formed it in WORLD space (ptmi_light_guide.h, poly_area_s): it travels in the polygon's otherwise unused `radius` slot, because
// recomputing it from rotated edges would change its bits under a camera.  The inside test is poly_intersect itself, epsilon
// included: the density is positive exactly where a ray would hit.
#pragma once
#include <type_traits>

namespace ptd {

constexpr float kTwoPi = 2.0f * kPi;

// How light_draw / light_mixture hold an emitter's constants: a reference into the kernel arguments, or -- the PLAMPS instances
// -- a copy, as nearest_hit holds its object.  With references to two tables of the arguments in flight the compiler gave up
// reading them where they lie and moved all 4 KiB of arguments to scratch (3968 bytes per lane in the pose and lens instances).
template <typename T, bool COPY>
using LightRow = std::conditional_t<COPY, const T, const T&>;

// Polygon emitter: eligible iff x is off its plane and some corner is above the horizon of (x, n).  aux = the signed height
// (v0 - x) . m of the plane over x.
__device__ __forceinline__ bool poly_light_eligible(const SceneObject& ob, const PolyEdges& pe, Vec3 x, Vec3 n, Vec3& v, float& aux) {
  v = sub(mk(ob.cx, ob.cy, ob.cz), x);
  aux = dot(v, mk(ob.nx, ob.ny, ob.nz));
  const float d0 = dot(v, n);
  const float d1 = dot(mk(pe.e1x, pe.e1y, pe.e1z), n);
  const float d2 = dot(mk(pe.e2x, pe.e2y, pe.e2z), n);
  const float reach = ob.is_disc == SHAPE_TRIANGLE ? fmaxf(0.0f, fmaxf(d1, d2)) : fmaxf(0.0f, d1) + fmaxf(0.0f, d2);
  return fabsf(aux) > kEps && d0 + reach > 0.0f;
}

__device__ __forceinline__ float poly_light_area(const SceneObject& ob) {
  return ob.is_disc == SHAPE_TRIANGLE ? 0.5f * ob.radius : ob.radius;   // (radius: S, see above)
}

__device__ __forceinline__ float poly_light_density(const SceneObject& ob, const PolyEdges& pe, Vec3 x, Vec3 w) {
  const float t = poly_intersect(x, w, ob, pe);
  if (t == 0.0f) return 0.0f;
  const float dn = dot(mk(ob.nx, ob.ny, ob.nz), w);
  if (dn == 0.0f) return 0.0f;
  return (kTwoPi * (t * t)) / (fabsf(dn) * poly_light_area(ob));
}

// The point y = v0 + (e1 a + e2 b), (a, b) = (x1, x2), folded into a + b <= 1 for a triangle; g = 2 pi l^3 / (|hgt| A_p).
__device__ __forceinline__ Vec3 poly_light_sample(const SceneObject& ob, const PolyEdges& pe, Vec3 x, float hgt, float x1, float x2,
                                                  float& g) {
  float a = x1, b = x2;
  if (ob.is_disc == SHAPE_TRIANGLE && a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
  const Vec3 y = add(mk(ob.cx, ob.cy, ob.cz), add(scale(mk(pe.e1x, pe.e1y, pe.e1z), a), scale(mk(pe.e2x, pe.e2y, pe.e2z), b)));
  const Vec3 e = sub(y, x);
  const float l2 = dot(e, e);
  const float l = sqrtf(l2);
  g = (kTwoPi * (l2 * l)) / (fabsf(hgt) * poly_light_area(ob));
  return scale(e, 1.0f / l);
}

// Is any part of emitter `ob` above the horizon of (x, n), seen from outside?  v = c - x; aux = |v|^2 (sphere) or the signed
// height (c - x) . m of the disc's plane over x (disc).  ob is wave-uniform: the shape test is a scalar branch.
template <bool PLAMPS = false>   // PLAMPS: the table may list polygons (shape codes 2, 3); every other instance compiles none of that
__device__ __forceinline__ bool light_eligible(const SceneObject& ob, const PolyEdges& pe, Vec3 x, Vec3 n, Vec3& v, float& aux) {
  if constexpr (PLAMPS) {
    if (ob.is_disc >= SHAPE_TRIANGLE) return poly_light_eligible(ob, pe, x, n, v, aux);
  }
  v = sub(mk(ob.cx, ob.cy, ob.cz), x);
  if (ob.is_disc) {
    const Vec3 m = mk(ob.nx, ob.ny, ob.nz);
    aux = dot(v, m);
    const float nm = dot(n, m);
    return fabsf(aux) > kEps && dot(v, n) + ob.radius * sqrtf(fmaxf(0.0f, 1.0f - nm * nm)) > 0.0f;
  }
  aux = dot(v, v);
  return aux > ob.r2 && dot(v, n) + ob.radius > 0.0f;
}

// g_k(w) of an eligible emitter for an arbitrary unit direction w (v, aux from light_eligible).  Sphere: (1 + cm) / s^2 inside
// the visible cone (w . a >= cm, a = v / D, s^2 = r^2 / D^2, cm = sqrt(1 - s^2)).  Disc: the disc test of nearest_hit on the ray
// (x, w), t = hgt / (m . w), then 2 t^2 / (|m . w| R^2).
template <bool PLAMPS = false>
__device__ __forceinline__ float light_density(const SceneObject& ob, const PolyEdges& pe, Vec3 x, Vec3 v, float aux, Vec3 w) {
  if constexpr (PLAMPS) {
    if (ob.is_disc >= SHAPE_TRIANGLE) return poly_light_density(ob, pe, x, w);
  }
  if (ob.is_disc) {
    const float dn = dot(mk(ob.nx, ob.ny, ob.nz), w);
    float g = 0.0f;
    if (dn != 0.0f) {
      const float t = aux / dn;
      if (t > kEps) {
        const Vec3 pc = sub(add(x, scale(w, t)), mk(ob.cx, ob.cy, ob.cz));
        if (!(dot(pc, pc) > ob.r2)) g = (2.0f * (t * t)) / (fabsf(dn) * ob.r2);
      }
    }
    return g;
  }
  const float s2 = ob.r2 / aux;
  const float cm = sqrtf(1.0f - s2);
  const Vec3 a = scale(v, 1.0f / sqrtf(aux));
  return dot(w, a) >= cm ? (1.0f + cm) / s2 : 0.0f;
}

// A direction drawn from an eligible emitter by two 32-bit words, and through `g` that emitter's own term for it (the rim rule:
// by construction, no inside test).  x1 = ((g2 >> 8) + 1/2) 2^-24, x2 = (g3 >> 8) 2^-24.
// Sphere: uniform in the visible cone about a, cos t = 1 - x1 s^2 / (1 + cm) (the cancellation-free 1 - x1 (1 - cm)).
// Disc: the point y = c + R sqrt(x1) (cos 2 pi x2 t1 + sin 2 pi x2 t2), uniform in area; g = 2 l^3 / (|hgt| R^2), l = |y - x|.
template <bool PLAMPS = false>
__device__ __forceinline__ Vec3 light_sample(const SceneObject& ob, const PolyEdges& pe, Vec3 x, Vec3 v, float aux, uint32_t g2, uint32_t g3,
                                             float& g) {
  const float x1 = ((float)(g2 >> 8) + 0.5f) * 5.9604644775390625e-08f;
  const float x2 = (float)(g3 >> 8) * 5.9604644775390625e-08f;
  if constexpr (PLAMPS) {
    if (ob.is_disc >= SHAPE_TRIANGLE) return poly_light_sample(ob, pe, x, aux, x1, x2, g);   // (wave-uniform: a scalar branch)
  }
  float sn, cs;
  dm_sincos2pi(x2, sn, cs);
  Vec3 rx, ry;
  if (ob.is_disc) {
    basis_about(mk(ob.nx, ob.ny, ob.nz), rx, ry);
    const float rho = ob.radius * sqrtf(x1);
    const Vec3 y = add(mk(ob.cx, ob.cy, ob.cz), add(scale(rx, rho * cs), scale(ry, rho * sn)));
    const Vec3 e = sub(y, x);
    const float l2 = dot(e, e);
    const float l = sqrtf(l2);
    g = (2.0f * (l2 * l)) / (fabsf(aux) * ob.r2);
    return scale(e, 1.0f / l);
  }
  const float s2 = ob.r2 / aux;
  const float cm = sqrtf(1.0f - s2);
  const Vec3 a = scale(v, 1.0f / sqrtf(aux));
  basis_about(a, rx, ry);
  const float ct = 1.0f - (x1 * s2) / (1.0f + cm);
  const float st = sqrtf(fmaxf(0.0f, 1.0f - ct * ct));
  const Vec3 h = mk(cs * st, sn * st, ct);
  g = (1.0f + cm) / s2;
  return mk(dot(mk(rx.x, ry.x, a.x), h), dot(mk(rx.y, ry.y, a.y), h), dot(mk(rx.z, ry.z, a.z), h));
}

// The light branch of a guided bounce: g1 selects the first rank k with g1 < threshold[k], else the last; if that emitter is
// eligible at (x, n), w is drawn from it and k returned (g = its own term), else -1 and nothing is written.  A wave-uniform
// loop: each emitter's constants are scalar loads, the lanes that selected it draw inside the loop.
template <bool PLAMPS = false>
__device__ __forceinline__ int light_draw(const TraceParams& P, Vec3 x, Vec3 n, uint32_t g1, uint32_t g2, uint32_t g3, Vec3& w, float& g) {
  const LightParams& L = P.lights;
  const int nl = (int)L.n;
  int sel = -1, drawn = -1;
#pragma unroll 1
  for (int j = 0; j < nl; ++j) {
    const bool pick = sel < 0 && (g1 < L.threshold[j] || j == nl - 1);
    if (pick) {
      sel = j;
      const uint32_t oi = L.index[j] & (uint32_t)(kMaxObjects - 1);   // (no bit pattern reads outside the tables)
      LightRow<SceneObject, PLAMPS> ob = P.obj[oi];
      LightRow<PolyEdges, PLAMPS> pe = P.poly[oi];
      Vec3 v;
      float aux;
      if (light_eligible<PLAMPS>(ob, pe, x, n, v, aux)) {
        w = light_sample<PLAMPS>(ob, pe, x, v, aux, g2, g3, g);
        drawn = j;
      }
    }
  }
  return drawn;
}

// Sum over the eligible emitters k, in declaration order, of p_k g_k(w), and through `pe` the sum of their p_k.  `drawn` is the
// rank w was drawn from (-1: none) and g_drawn that emitter's own term (the rim rule).
template <bool PLAMPS = false>
__device__ __forceinline__ float light_mixture(const TraceParams& P, Vec3 x, Vec3 n, Vec3 w, int drawn, float g_drawn, float& pe) {
  const LightParams& L = P.lights;
  const int nl = (int)L.n;
  float sum = 0.0f;
  pe = 0.0f;
#pragma unroll 1
  for (int j = 0; j < nl; ++j) {
    const float p = L.probability[j];
    if (p == 0.0f) continue;   // wave-uniform: never selected, adds nothing
    const uint32_t oi = L.index[j] & (uint32_t)(kMaxObjects - 1);
    LightRow<SceneObject, PLAMPS> ob = P.obj[oi];
    LightRow<PolyEdges, PLAMPS> edges = P.poly[oi];
    Vec3 v;
    float aux;
    if (light_eligible<PLAMPS>(ob, edges, x, n, v, aux)) {
      pe = pe + p;
      const float g = j == drawn ? g_drawn : light_density<PLAMPS>(ob, edges, x, v, aux, w);
      sum = sum + p * g;
    }
  }
  return sum;
}

// pt_light_guide_sample / pt_light_guide_eval: the functions above over caller data, P.obj[] being the world-space table.
template <bool PLAMPS>
__device__ __forceinline__ void light_guide_sample_body(const TraceParams& P, const float* origin, const float* normal, const uint32_t* g1,
                                                        const uint32_t* g2, const uint32_t* g3, uint32_t n, float* dir, int32_t* light) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t b = 3 * (size_t)t;
  Vec3 w = mk(0.f, 0.f, 0.f);
  float g = 0.f;
  const int k = light_draw<PLAMPS>(P, mk(origin[b], origin[b + 1], origin[b + 2]), mk(normal[b], normal[b + 1], normal[b + 2]), g1[t], g2[t],
                           g3[t], w, g);
  dir[b] = w.x; dir[b + 1] = w.y; dir[b + 2] = w.z;
  light[t] = k;
}
__global__ void light_guide_sample_kernel(const TraceParams P, const float* origin, const float* normal, const uint32_t* g1,
                                          const uint32_t* g2, const uint32_t* g3, uint32_t n, float* dir, int32_t* light) {
  light_guide_sample_body<false>(P, origin, normal, g1, g2, g3, n, dir, light);
}
// ... while the table in force lists a polygon (pt_set_light_guide_ex)
__global__ void light_guide_sample_plamps_kernel(const TraceParams P, const float* origin, const float* normal, const uint32_t* g1,
                                                 const uint32_t* g2, const uint32_t* g3, uint32_t n, float* dir, int32_t* light) {
  light_guide_sample_body<true>(P, origin, normal, g1, g2, g3, n, dir, light);
}

template <bool PLAMPS>
__device__ __forceinline__ void light_guide_eval_body(const TraceParams& P, const float* origin, const float* normal, const float* dir,
                                                      uint32_t n, float* sum, float* pe) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t b = 3 * (size_t)t;
  float e;
  sum[t] = light_mixture<PLAMPS>(P, mk(origin[b], origin[b + 1], origin[b + 2]), mk(normal[b], normal[b + 1], normal[b + 2]),
                         mk(dir[b], dir[b + 1], dir[b + 2]), -1, 0.f, e);
  pe[t] = e;
}
__global__ void light_guide_eval_kernel(const TraceParams P, const float* origin, const float* normal, const float* dir, uint32_t n,
                                        float* sum, float* pe) {
  light_guide_eval_body<false>(P, origin, normal, dir, n, sum, pe);
}
__global__ void light_guide_eval_plamps_kernel(const TraceParams P, const float* origin, const float* normal, const float* dir, uint32_t n,
                                               float* sum, float* pe) {
  light_guide_eval_body<true>(P, origin, normal, dir, n, sum, pe);
}

}  // namespace ptd
