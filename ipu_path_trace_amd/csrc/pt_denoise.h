// pt_denoise.h -- edge-avoiding A-trous wavelet filter over the finished film (pt_denoise, include/ptmi.h carries the
// definition in full; Dammertz et al., "Edge-Avoiding A-Trous Wavelet Transform for fast Global Illumination Filtering", HPG
// 2010).  An EXTENSION: the reference has no denoiser.  It runs after the sampling loop, on dense frames of its own, and touches
// no buffer the trace, NIF or accumulate kernels use.
//
// Frames: two float4 colour frames (ping-pong) c = (B, G, R, bits of the object index) and the two read-only feature frames of
// pt_features.h, f0 = (nx, ny, nz, depth), f1 = (albedo B, G, R, index bits).  The object index rides in the colour frame's
// fourth component so that a tap is two 16-byte gathers, c[q] and f0[q], not three.
//
// atrous_kernel<STEP, TILED>: one iteration, one thread per pixel, 32 x 8 pixel workgroups (a wave covers two rows of 32 pixels:
// 512 contiguous bytes per row and frame).
//   TILED   the tile plus its halo of 2 STEP pixels is staged in LDS first ((32 + 4 STEP) x (8 + 4 STEP) entries of 32 bytes: 13.5 KiB
//           at STEP 1, 20 KiB at STEP 2) and the 25 taps read LDS.  Only instantiated for STEP <= 2: the halo grows with the step
//           and the re-use between neighbours does not (at STEP >= 8 no two pixels of a tile row share a tap).
//   direct  the taps are global loads; the taps of neighbouring threads are neighbouring addresses (coalesced along x), and both
//           frames of an image a user renders sit in L2 / the Infinity Cache.
// Which variant runs at which step was decided by measurement: profiles/r11_denoise.txt (scripts/denoise_bench.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptd {

constexpr int kDenoiseTileW = 32, kDenoiseTileH = 8;
constexpr float kAlbedoFloor = 1e-3f;     // demodulation divides by max(albedo, 1e-3)
constexpr float kDepthFloor = 1e-6f;      // the depth stop is relative to max(d[p], 1e-6)

struct AtrousParams {
  uint32_t width, height;
  float inv_sc2;      // 1 / sigma_c_i^2 of this iteration; 0 = colour stop off
  float inv_sn2;      // 1 / sigma_normal^2; 0 = off
  float sigma_d;      // sigma_depth; 0 = off
  int32_t object_stop;
};

// The B3 spline 1/16 (1, 4, 6, 4, 1) as k[|d|] = (3/8, 1/4, 1/16): h(dx, dy) = k[|dx|] k[|dy|], every product exact in binary32.
__device__ __forceinline__ constexpr float b3(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

// One tap q of pixel p folded into (sum, wsum).  The three soft stops are ONE exponential of the summed arguments,
// exp(-(x_c + x_n + x_d)) = w_c w_n w_d; a stop whose squared difference is exactly 0 adds 0 (weight 1) without forming the
// quotient.  The object stop is a hard zero: the tap is not accumulated at all, its colour is never multiplied, so a
// non-finite neighbour on another object cannot leak (the select below discards a NaN weight too).
__device__ __forceinline__ void atrous_tap(const AtrousParams& A, float hk, float4 cp, float4 fp, float inv_sd2, float4 cq, float4 fq,
                                           float& sb, float& sg, float& sr, float& wsum) {
  const bool use = !A.object_stop || __float_as_uint(cq.w) == __float_as_uint(cp.w);
  const float db = cp.x - cq.x, dg = cp.y - cq.y, dr = cp.z - cq.z;
  const float nx = fp.x - fq.x, ny = fp.y - fq.y, nz = fp.z - fq.z;
  const float dd = fp.w - fq.w;
  const float d2c = db * db + dg * dg + dr * dr, d2n = nx * nx + ny * ny + nz * nz, d2d = dd * dd;
  float x = 0.f;
  if (A.inv_sc2 > 0.f && d2c != 0.f) x += d2c * A.inv_sc2;
  if (A.inv_sn2 > 0.f && d2n != 0.f) x += d2n * A.inv_sn2;
  if (A.sigma_d > 0.f && d2d != 0.f) x += d2d * inv_sd2;
  const float w = hk * expf(-x);   // expf: the OCML single-precision exponential, 1 ulp (HIP math API accuracy table)
  sb = use ? sb + w * cq.x : sb;
  sg = use ? sg + w * cq.y : sg;
  sr = use ? sr + w * cq.z : sr;
  wsum = use ? wsum + w : wsum;
}

template <int STEP, bool TILED>
__global__ __launch_bounds__(kDenoiseTileW * kDenoiseTileH) void atrous_kernel(const AtrousParams A, const float4* __restrict__ cin,
                                                                               const float4* __restrict__ f0, float4* __restrict__ cout) {
  constexpr int TW = kDenoiseTileW, TH = kDenoiseTileH, HALO = 2 * STEP;
  constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
  const int tx = (int)threadIdx.x % TW, ty = (int)threadIdx.x / TW;
  const int x0 = (int)blockIdx.x * TW, y0 = (int)blockIdx.y * TH;
  const int px = x0 + tx, py = y0 + ty;
  const int W = (int)A.width, H = (int)A.height;
  const bool inside = px < W && py < H;

  __shared__ float4 lc[TILED ? LW * LH : 1];
  __shared__ float4 lf[TILED ? LW * LH : 1];
  if constexpr (TILED) {
    // stage the tile and its halo; an entry outside the image is never read as a tap (the bounds test below) and is left unset
    for (int e = (int)threadIdx.x; e < LW * LH; e += TW * TH) {
      const int ly = e / LW, lx = e - ly * LW;
      const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
      if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
        const size_t g = (size_t)gy * A.width + (size_t)gx;
        lc[e] = cin[g];
        lf[e] = f0[g];
      }
    }
    __syncthreads();
  }
  if (!inside) return;

  const size_t p = (size_t)py * A.width + (size_t)px;
  float4 cp, fp;
  if constexpr (TILED) { cp = lc[(ty + HALO) * LW + tx + HALO]; fp = lf[(ty + HALO) * LW + tx + HALO]; }
  else { cp = cin[p]; fp = f0[p]; }
  float inv_sd2 = 0.f;
  if (A.sigma_d > 0.f) {
    const float s = A.sigma_d * fmaxf(fp.w, kDepthFloor);
    inv_sd2 = 1.0f / (s * s);
  }
  // the centre tap: weight 1 exactly, not computed through exp
  float sb = b3(0) * b3(0) * cp.x, sg = b3(0) * b3(0) * cp.y, sr = b3(0) * b3(0) * cp.z, wsum = b3(0) * b3(0);
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const int qy = py + dy * STEP;
    if (qy < 0 || qy >= H) continue;   // taps outside the image are skipped: no clamping, no wrap
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if (dx == 0 && dy == 0) continue;
      const int qx = px + dx * STEP;
      if (qx < 0 || qx >= W) continue;
      float4 cq, fq;
      if constexpr (TILED) {
        const int e = (ty + HALO + dy * STEP) * LW + tx + HALO + dx * STEP;
        cq = lc[e]; fq = lf[e];
      } else {
        const size_t q = (size_t)qy * A.width + (size_t)qx;
        cq = cin[q]; fq = f0[q];
      }
      atrous_tap(A, b3(dx) * b3(dy), cp, fp, inv_sd2, cq, fq, sb, sg, sr, wsum);
    }
  }
  cout[p] = make_float4(sb / wsum, sg / wsum, sr / wsum, cp.w);   // wsum >= 9/64: a convex combination of the inputs
}

// ---- the passes around the iterations, one thread per pixel (or work item)

// Host image [n][3] -> colour frame, with the object index of f1 and, if asked, demodulated: c / max(albedo, 1e-3) per channel.
__global__ void denoise_pack_kernel(uint32_t n, const float* __restrict__ bgr, const float4* __restrict__ f1, int demodulate,
                                    float4* __restrict__ c) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 a = f1[i];
  float b = bgr[3 * (size_t)i], g = bgr[3 * (size_t)i + 1], r = bgr[3 * (size_t)i + 2];
  if (demodulate) { b = b / fmaxf(a.x, kAlbedoFloor); g = g / fmaxf(a.y, kAlbedoFloor); r = r / fmaxf(a.z, kAlbedoFloor); }
  c[i] = make_float4(b, g, r, a.w);
}

// This handle's work items scattered into a dense [height][width][3] image by their (u, v); pixels the worklist does not hold and
// padding items stay 0 (the image is zeroed first).  film == nullptr: mean radiance of the accumulators, (b, g, r) * (1 /
// sampleCount) with the device's 32-bit count (0 samples -> 0), as export_hdr_kernel; else the resident film's running sum times
// inv_steps = 1 / film_steps.  A pixel the worklist holds twice gets one of the two values.
__global__ void denoise_scatter_kernel(uint32_t n, const uint32_t* __restrict__ pix, const float* __restrict__ ar,
                                       const float* __restrict__ ag, const float* __restrict__ ab, const uint32_t* __restrict__ count,
                                       const float* __restrict__ film, float inv_steps, uint32_t width, uint32_t height,
                                       float* __restrict__ bgr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t u = pix[i] & 0xffffu, v = pix[i] >> 16;
  if (u >= width || v >= height) return;
  float b, g, r;
  if (film) {
    b = film[3 * (size_t)i] * inv_steps; g = film[3 * (size_t)i + 1] * inv_steps; r = film[3 * (size_t)i + 2] * inv_steps;
  } else {
    const uint32_t cnt = count[i];
    const float s = cnt ? 1.f / (float)cnt : 0.f;
    b = ab[i] * s; g = ag[i] * s; r = ar[i] * s;
  }
  const size_t o = 3 * ((size_t)v * width + u);
  bgr[o] = b; bgr[o + 1] = g; bgr[o + 2] = r;
}

// Colour frame -> [n][3], re-modulated by the factor denoise_pack_kernel divided by.
__global__ void denoise_unpack_kernel(uint32_t n, const float4* __restrict__ c, const float4* __restrict__ f1, int demodulate,
                                      float* __restrict__ bgr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 v = c[i];
  if (demodulate) {
    const float4 a = f1[i];
    v.x = v.x * fmaxf(a.x, kAlbedoFloor); v.y = v.y * fmaxf(a.y, kAlbedoFloor); v.z = v.z * fmaxf(a.z, kAlbedoFloor);
  }
  bgr[3 * (size_t)i] = v.x; bgr[3 * (size_t)i + 1] = v.y; bgr[3 * (size_t)i + 2] = v.z;
}

}  // namespace ptd
