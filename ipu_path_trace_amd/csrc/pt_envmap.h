// pt_envmap.h -- an equirectangular HDR image as the environment light (pt_set_env_map): the third kind of environment next
// to the NIF (pt_nif*.h) and the constant radiance.
//
// The kernel stands where the NIF kernels stand (stage N of enqueue_path_trace) and has their two modes: per path it reads
// the compacted queue of escaped paths the trace kernel wrote and stores rad_* = bgr * throughput -- the heads' own single
// fp32 multiply per channel --; with out_bgr set it stores the looked-up BGR of every queue entry instead (the form sharing,
// the memo and pt_env_map_lookup drive).
//
// Mapping (include/ptmi.h): u runs down the image, v across it (PreProcessEscapedRays, codelets.cpp:333-347); texel (r, c)
// sits at u = r / H, v = c / W with no half-texel offset (NifModel::makeGridCoordsUV, NifModel.cpp:474-490), so the map is
// the image a NIF would be trained to reproduce.  Rows clamp at the poles, columns wrap.  u and v are clamped into [0, 1]
// first (a NaN becomes 0), so no bit pattern of (u, v) reads outside the image.
//
// Texels are one float4 (B, G, R, 0) each, row-major: a corner is one 16-byte load, and the four corners of a bilinear
// lookup are four independent loads issued before the first use.  The kernel is a latency-bound gather.
#pragma once

namespace ptd {

constexpr int kEnvBlock = 256;
constexpr int kEnvNearest = 0, kEnvBilinear = 1;   // PT_ENV_FILTER_NEAREST / _BILINEAR

struct EnvMapParams {
  // queue of escaped paths as the trace kernel wrote it: one region per trace workgroup
  const float* q_u; const float* q_v; const float* q_tr; const float* q_tg; const float* q_tb;
  const uint32_t* q_path;
  const uint32_t* region_count;
  uint32_t region_cap;
  float* rad_r; float* rad_g; float* rad_b;   // per path: env(rgb) * throughput
  float* out_bgr;                             // not null: looked-up BGR [queue slot][3] instead
  const float4* texels;                       // [height][width] (B, G, R, 0)
  uint32_t width, height;
};

// out = a + t (b - a), spelled with fmaf so that no contraction setting changes it
__device__ __forceinline__ float env_lerp(float t, float a, float b) { return fmaf(t, b - a, a); }

// grid (ceil(region_cap / 256), n_regions): x = 256 entries of one region, y = region
template <int FILTER>
__global__ __launch_bounds__(kEnvBlock) void envmap_kernel(EnvMapParams E) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kEnvBlock + threadIdx.x;
  if (local >= E.region_count[r]) return;
  const size_t qi = (size_t)r * E.region_cap + local;
  const uint32_t W = E.width, H = E.height;
  const float u = fminf(fmaxf(E.q_u[qi], 0.f), 1.f), v = fminf(fmaxf(E.q_v[qi], 0.f), 1.f);
  const float y = u * (float)H, x = v * (float)W;
  const float y0 = floorf(y), x0 = floorf(x);
  const float fy = y - y0, fx = x - x0;
  uint32_t r0 = (uint32_t)(int)y0, c0 = (uint32_t)(int)x0;     // 0 <= y0 <= H, 0 <= x0 <= W
  r0 = r0 < H - 1u ? r0 : H - 1u;                               // rows clamp at the pole
  c0 = c0 >= W ? c0 - W : c0;                                   // columns wrap: v == 1 is column 0
  float b, g, rr;
  if (FILTER == kEnvNearest) {
    const float4 t = E.texels[(size_t)r0 * W + c0];
    b = t.x; g = t.y; rr = t.z;
  } else {
    const uint32_t r1 = r0 + 1u < H ? r0 + 1u : H - 1u;
    const uint32_t c1 = c0 + 1u >= W ? c0 + 1u - W : c0 + 1u;
    const float4* row0 = E.texels + (size_t)r0 * W;
    const float4* row1 = E.texels + (size_t)r1 * W;
    const float4 t00 = row0[c0], t01 = row0[c1], t10 = row1[c0], t11 = row1[c1];   // four loads in flight
    b = env_lerp(fy, env_lerp(fx, t00.x, t01.x), env_lerp(fx, t10.x, t11.x));
    g = env_lerp(fy, env_lerp(fx, t00.y, t01.y), env_lerp(fx, t10.y, t11.y));
    rr = env_lerp(fy, env_lerp(fx, t00.z, t01.z), env_lerp(fx, t10.z, t11.z));
  }
  if (E.out_bgr) {
    E.out_bgr[3 * qi + 0] = b;
    E.out_bgr[3 * qi + 1] = g;
    E.out_bgr[3 * qi + 2] = rr;
  } else {
    const uint32_t path = E.q_path[qi];
    E.rad_r[path] = rr * E.q_tr[qi];
    E.rad_g[path] = g * E.q_tg[qi];
    E.rad_b[path] = b * E.q_tb[qi];
  }
}

}  // namespace ptd
