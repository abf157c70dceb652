// pt_env_guide.h -- device side of the environment guide (pt_set_env_guide, include/ptmi.h): drawing a direction from the
// guide's alias table and evaluating the guide's density for a direction.  The tables come from ptmi_env_guide.h (host); the
// guided diffuse bounce that uses these functions is in pt_trace.h (shade_hit<GUIDE = true>).  Both tables are read with plain
// global loads, 8 bytes per alias entry and 4 per density: no LDS, so a guided trace kernel keeps its place beside the NIF kernel.
#pragma once
#include "pt_device_math.h"

namespace ptd {

constexpr uint32_t kGuideBlock = 66u;   // Philox block of the guide draw of bounce d: 66 + d (0..64: AA noise and bounces, 65: lens)

struct GuideParams {
  const uint2* alias;      // [rows * cols] {threshold, alias}: cell k is kept when a 32-bit word is < threshold
  const float* q;          // [rows * cols] P(cell) n / pi
  uint32_t rows, cols;     // powers of two
  uint32_t log2n, log2cols;
  uint32_t alpha_thr;      // a word below it takes the guide branch
  float alpha, one_minus_alpha;   // alpha_thr / 2^32 and 1 - that, rounded once on the host
  float inv_rows, inv_cols;       // exact: powers of two
};

__device__ __forceinline__ void dir_to_uv(Vec3 d, float azimuth, float& u, float& v);   // pt_trace.h

// Three caller words -> the cell drawn and a point (u, v) inside it (16 bits of g3 each way, cell-centred).
__device__ __forceinline__ uint32_t guide_sample(const GuideParams& G, uint32_t g1, uint32_t g2, uint32_t g3, float& u, float& v) {
  const uint32_t k = (g1 >> 1) >> (31u - G.log2n);   // g1 >> (32 - log2 n), also for n = 1
  const uint2 e = G.alias[k];                         // k < n by construction
  uint32_t cell = g2 < e.x ? k : e.y;
  cell &= (G.rows * G.cols - 1u);                     // (the host's aliases are in range; no bit pattern reads outside the tables)
  const uint32_t i = cell >> G.log2cols, j = cell & (G.cols - 1u);
  u = ((float)i + ((float)(g3 >> 16) + 0.5f) * 1.52587890625e-05f) * G.inv_rows;
  v = ((float)j + ((float)(g3 & 0xffffu) + 0.5f) * 1.52587890625e-05f) * G.inv_cols;
  return cell;
}

// (u, v) -> world direction (sin t cos p, cos t, sin t sin p), t = pi u, p = 2 pi v - azimuth: the inverse of dir_to_uv.
__device__ __forceinline__ Vec3 guide_direction(float u, float v, float azimuth) {
  float st, ct, sp, cp;
  dm_sincos2pi(u * 0.5f, st, ct);
  float w = v - azimuth * 0.15915493667125701904296875f;   // turns; brought into [0, 1] for dm_sincos2pi
  w = w - floorf(w);
  dm_sincos2pi(w, sp, cp);
  return mk(st * cp, ct, st * sp);
}

// World direction -> its cell and g = 2 pi x the guide's solid-angle density = q[cell] / sin(theta).
__device__ __forceinline__ float guide_density(const GuideParams& G, Vec3 dw, float azimuth, uint32_t& cell) {
  float u, v;
  dir_to_uv(dw, azimuth, u, v);
  int i = (int)(u * (float)G.rows);
  i = i < (int)G.rows - 1 ? i : (int)G.rows - 1;
  i = i > 0 ? i : 0;                                        // (u >= 0 always; no bit pattern reads outside the table)
  const uint32_t j = (uint32_t)(int)(v * (float)G.cols) & (G.cols - 1u);
  cell = ((uint32_t)i << G.log2cols) | j;
  const float sint = fmaxf(sqrtf(1.0f - dw.y * dw.y), 1e-30f);
  return G.q[cell] / sint;
}

// pt_env_guide_sample / pt_env_guide_eval: the two functions above over caller data.
__global__ void env_guide_sample_kernel(const GuideParams G, const uint32_t* g1, const uint32_t* g2, const uint32_t* g3, uint32_t n,
                                        float* uv, uint32_t* cell) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  float u, v;
  cell[t] = guide_sample(G, g1[t], g2[t], g3[t], u, v);
  uv[2 * (size_t)t] = u;
  uv[2 * (size_t)t + 1] = v;
}

__global__ void env_guide_eval_kernel(const GuideParams G, float azimuth, const float* dir, uint32_t n, uint32_t* cell, float* g) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t c;
  g[t] = guide_density(G, mk(dir[3 * (size_t)t], dir[3 * (size_t)t + 1], dir[3 * (size_t)t + 2]), azimuth, c);
  cell[t] = c;
}

}  // namespace ptd
