// pt_env_guide_build.h -- device side of pt_set_env_guide_from_environment (include/ptmi.h): the cell masses of an environment
// guide summed from the environment in force, with no image in host memory.  The image the guide is defined over (height
// rows S, width cols S) is never formed: it is visited one sub-sample plane (sr, sc) at a time, a plane being one lookup per
// cell.  Per plane: env_guide_grid_kernel writes the dense queue (u, v), the NIF stage's own launcher decodes it to BGR
// (ptmi.hip: launch_nif, launch_envmap, or env_guide_fill_kernel for a constant), env_guide_mass_kernel adds the plane to the
// masses.  Binary64, no contraction (pt_device_math.h), one thread per cell and the planes in row-major (sr, sc) order: every
// mass is the sum ptguide::build() forms on the host over the same values, bit for bit.  No atomics anywhere.
#pragma once
#include <cfloat>

namespace ptd {

constexpr uint32_t kGuideBuildBlock = 256u;

struct GuideBuildParams {
  uint32_t n;                 // rows * cols
  uint32_t cols, log2cols;    // powers of two
  uint32_t S, sr, sc;         // samples per cell edge; the plane
  float inv_h, inv_w;         // 1 / (rows S), 1 / (cols S): exact, powers of two
};

// The plane's queue: cell k = (i, j) looks the environment up at u = (i S + sr + 0.5) / (rows S), v = (j S + sc + 0.5) / (cols S).
// Every operand is an integer + 0.5 below 2^13 and the scale is a power of two: the products are the quotients of the contract.
__global__ void env_guide_grid_kernel(const GuideBuildParams B, float* __restrict__ u, float* __restrict__ v, uint32_t* __restrict__ count) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) *count = B.n;
  if (k >= B.n) return;
  const uint32_t i = k >> B.log2cols, j = k & (B.cols - 1u);
  u[k] = ((float)(i * B.S + B.sr) + 0.5f) * B.inv_h;
  v[k] = ((float)(j * B.S + B.sc) + 0.5f) * B.inv_w;
}

// A constant environment in out_bgr form: the stage's "lookup" when there is nothing to look up.
__global__ void env_guide_fill_kernel(uint32_t n, float b, float g, float r, float* __restrict__ bgr) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  bgr[3 * (size_t)k] = b;
  bgr[3 * (size_t)k + 1] = g;
  bgr[3 * (size_t)k + 2] = r;
}

// x >= 0 ? fminf(x, FLT_MAX) : 0 -- NaN and negative values become 0, +inf becomes FLT_MAX; `replaced` counts the changes.
__device__ __forceinline__ float guide_clamp(float x, uint32_t& replaced) {
  if (x >= 0.f) {
    if (x > FLT_MAX) { replaced += 1u; return FLT_MAX; }
    return x;
  }
  replaced += 1u;
  return 0.f;
}

// mass[k] += ((0.0722 B + 0.7152 G) + 0.2126 R) sn[i S + sr], one thread per cell, consecutive threads on consecutive cells.
// clamp_partial[block] += the channel values this block replaced: each block owns its slot and the planes follow one another
// on one stream, so the plain read-modify-write of thread 0 is the whole reduction; the host adds the slots.
__global__ void __launch_bounds__(kGuideBuildBlock)
env_guide_mass_kernel(const GuideBuildParams B, const float* __restrict__ bgr, const double* __restrict__ sn, double* __restrict__ mass,
                      uint32_t* __restrict__ clamp_partial) {
  __shared__ uint32_t s_replaced[kGuideBuildBlock];
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t replaced = 0u;
  if (k < B.n) {
    const float b = guide_clamp(bgr[3 * (size_t)k], replaced);
    const float g = guide_clamp(bgr[3 * (size_t)k + 1], replaced);
    const float r = guide_clamp(bgr[3 * (size_t)k + 2], replaced);
    const uint32_t i = k >> B.log2cols;
    const double y = (0.0722 * (double)b + 0.7152 * (double)g) + 0.2126 * (double)r;
    mass[k] += y * sn[i * B.S + B.sr];
  }
  s_replaced[threadIdx.x] = replaced;
  __syncthreads();
  for (uint32_t w = kGuideBuildBlock / 2u; w > 0u; w >>= 1) {
    if (threadIdx.x < w) s_replaced[threadIdx.x] += s_replaced[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) clamp_partial[blockIdx.x] += s_replaced[0];
}

}  // namespace ptd
