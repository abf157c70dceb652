// pt_light_guide.h -- device side of the emitter guide (pt_set_light_guide, include/ptmi.h): drawing a direction towards an
// emissive sphere or disc of the scene and evaluating the density of such draws for any direction.  The table (emitter rank ->
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
#pragma once

namespace ptd {

// Is any part of emitter `ob` above the horizon of (x, n), seen from outside?  v = c - x; aux = |v|^2 (sphere) or the signed
// height (c - x) . m of the disc's plane over x (disc).  ob is wave-uniform: the shape test is a scalar branch.
__device__ __forceinline__ bool light_eligible(const SceneObject& ob, Vec3 x, Vec3 n, Vec3& v, float& aux) {
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
__device__ __forceinline__ float light_density(const SceneObject& ob, Vec3 x, Vec3 v, float aux, Vec3 w) {
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
__device__ __forceinline__ Vec3 light_sample(const SceneObject& ob, Vec3 x, Vec3 v, float aux, uint32_t g2, uint32_t g3, float& g) {
  const float x1 = ((float)(g2 >> 8) + 0.5f) * 5.9604644775390625e-08f;
  const float x2 = (float)(g3 >> 8) * 5.9604644775390625e-08f;
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
__device__ __forceinline__ int light_draw(const TraceParams& P, Vec3 x, Vec3 n, uint32_t g1, uint32_t g2, uint32_t g3, Vec3& w, float& g) {
  const LightParams& L = P.lights;
  const int nl = (int)L.n;
  int sel = -1, drawn = -1;
#pragma unroll 1
  for (int j = 0; j < nl; ++j) {
    const bool pick = sel < 0 && (g1 < L.threshold[j] || j == nl - 1);
    if (pick) {
      sel = j;
      const SceneObject& ob = P.obj[L.index[j] & (uint32_t)(kMaxObjects - 1)];   // (no bit pattern reads outside the table)
      Vec3 v;
      float aux;
      if (light_eligible(ob, x, n, v, aux)) {
        w = light_sample(ob, x, v, aux, g2, g3, g);
        drawn = j;
      }
    }
  }
  return drawn;
}

// Sum over the eligible emitters k, in declaration order, of p_k g_k(w), and through `pe` the sum of their p_k.  `drawn` is the
// rank w was drawn from (-1: none) and g_drawn that emitter's own term (the rim rule).
__device__ __forceinline__ float light_mixture(const TraceParams& P, Vec3 x, Vec3 n, Vec3 w, int drawn, float g_drawn, float& pe) {
  const LightParams& L = P.lights;
  const int nl = (int)L.n;
  float sum = 0.0f;
  pe = 0.0f;
#pragma unroll 1
  for (int j = 0; j < nl; ++j) {
    const float p = L.probability[j];
    if (p == 0.0f) continue;   // wave-uniform: never selected, adds nothing
    const SceneObject& ob = P.obj[L.index[j] & (uint32_t)(kMaxObjects - 1)];
    Vec3 v;
    float aux;
    if (light_eligible(ob, x, n, v, aux)) {
      pe = pe + p;
      const float g = j == drawn ? g_drawn : light_density(ob, x, v, aux, w);
      sum = sum + p * g;
    }
  }
  return sum;
}

// pt_light_guide_sample / pt_light_guide_eval: the functions above over caller data, P.obj[] being the world-space table.
__global__ void light_guide_sample_kernel(const TraceParams P, const float* origin, const float* normal, const uint32_t* g1,
                                          const uint32_t* g2, const uint32_t* g3, uint32_t n, float* dir, int32_t* light) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t b = 3 * (size_t)t;
  Vec3 w = mk(0.f, 0.f, 0.f);
  float g = 0.f;
  const int k = light_draw(P, mk(origin[b], origin[b + 1], origin[b + 2]), mk(normal[b], normal[b + 1], normal[b + 2]), g1[t], g2[t],
                           g3[t], w, g);
  dir[b] = w.x; dir[b + 1] = w.y; dir[b + 2] = w.z;
  light[t] = k;
}

__global__ void light_guide_eval_kernel(const TraceParams P, const float* origin, const float* normal, const float* dir, uint32_t n,
                                        float* sum, float* pe) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t b = 3 * (size_t)t;
  float e;
  sum[t] = light_mixture(P, mk(origin[b], origin[b + 1], origin[b + 2]), mk(normal[b], normal[b + 1], normal[b + 2]),
                         mk(dir[b], dir[b + 1], dir[b + 2]), -1, 0.f, e);
  pe[t] = e;
}

}  // namespace ptd
