// pt_nif_train.h -- kernels of the on-device NIF trainer (pt_nif_train_*, include/ptmi.h): an HDR environment map in, the
// weights of a Fourier-feature MLP out.  Everything here is float32; the matrix products run on v_mfma_f32_32x32x2_f32
// (an exact fp32 FMA chain in k order, pt_nif_f32.h).  Nothing of the sampling loop is touched: the trainer runs beside it.
//
// Buffers are plain row-major.  Layer l reads its input from its OWN buffer act[l], [batch][rows_l]: the previous layer
// writes its post-ReLU output into columns 0 .. cols_{l-1} of it, and where the layer takes concat(x, features)
// (NifModel.cpp:305-308) the encode kernel has written the features into the remaining 4 E columns -- one row, as the oracle
// lays it out, and no concat pass.
//
// Determinism: no float atomic anywhere.  Sums over the batch (dW, db) go into kTrainSlabs per-slab partials that a second
// pass adds in slab order; the loss and the image statistics are per-block tree sums added in block order.  The grid of
// every kernel depends on the shapes alone, so two runs with one seed on one device give the same bits.
#pragma once
#include "pt_device_math.h"
#include "pt_nif.h"

namespace ptd {

constexpr uint32_t kTrainSlabs = 32;         // batch slabs of the dW / db reduction
constexpr uint32_t kTrainStatBlocks = 256;   // partial blocks of the image statistics and of the loss
constexpr uint32_t kTrainBatchTag = 0x4e494642u, kTrainInitTag = 0x4e494657u;   // Philox counter word 3: "NIFB", "NIFW"

// ---- image statistics and the target image

// L of one texel channel (binary64 from the binary32 texel and eps): log(texel + eps) in log mode, the texel otherwise.
__device__ __forceinline__ double train_l(float texel, float eps, int log_mode) {
  return log_mode ? log((double)texel + (double)eps) : (double)texel;
}

// A block's tree sum / tree maximum over 256 values in LDS: a fixed order.
template <bool MAX>
__device__ __forceinline__ double train_block_reduce(double* s, double v) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) s[threadIdx.x] = MAX ? fmax(s[threadIdx.x], s[threadIdx.x + o]) : s[threadIdx.x] + s[threadIdx.x + o];
    __syncthreads();
  }
  const double r = s[0];
  __syncthreads();
  return r;
}

// MODE 0: partial[block][c] = sum of L over the block's texels; MODE 1: the largest |L - mean[c]| (enc = mean0..2, max).
template <int MODE>
__global__ __launch_bounds__(256) void train_stat_kernel(const float4* texels, uint32_t n, float eps, int log_mode, const float* enc,
                                                         double* partial) {
  __shared__ double s[256];
  double a[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const float4 t = texels[i];
    const float c[3] = {t.x, t.y, t.z};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double L = train_l(c[k], eps, log_mode);
      if (MODE == 0) a[k] += L; else a[k] = fmax(a[k], fabs(L - (double)enc[k]));
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double r = train_block_reduce<MODE == 1>(s, a[k]);
    if (threadIdx.x == 0) partial[blockIdx.x * 3u + k] = r;
  }
}

// One block: the kTrainStatBlocks partials in block order.  MODE 0: enc[c] = (float)(sum / n); MODE 1: enc[3] = (float)max.
template <int MODE>
__global__ __launch_bounds__(256) void train_stat_final_kernel(const double* partial, uint32_t n, float* enc) {
  __shared__ double s[256];
  double out[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = train_block_reduce<MODE == 1>(s, partial[threadIdx.x * 3u + k]);
  if (threadIdx.x == 0) {
    if (MODE == 0) { for (int k = 0; k < 3; ++k) enc[k] = (float)(out[k] / (double)n); }
    else enc[3] = (float)fmax(out[0], fmax(out[1], out[2]));
  }
}

// target[i] = (L - mean) / max per channel, binary64 from the binary32 mean and max, rounded once: what the net learns.
__global__ __launch_bounds__(256) void train_target_kernel(const float4* texels, uint32_t n, float eps, int log_mode, const float* enc,
                                                           float4* target) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 t = texels[i];
  const double mx = (double)enc[3];
  target[i] = make_float4((float)((train_l(t.x, eps, log_mode) - (double)enc[0]) / mx), (float)((train_l(t.y, eps, log_mode) - (double)enc[1]) / mx),
                          (float)((train_l(t.z, eps, log_mode) - (double)enc[2]) / mx), 0.f);
}

// ---- the batch of a step

// Sample i of step t: texel index floor(word0 * H W / 2^32) of Philox block (i, t_lo, t_hi, "NIFB") keyed by the seed;
// u = r / H, v = c / W by one fp32 division each (the map's own mapping, pt_envmap.h); t = the texel's target.
__global__ __launch_bounds__(256) void train_batch_kernel(const float4* target, uint32_t W, uint32_t H, uint32_t n, uint32_t seed_lo,
                                                          uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi, float* u, float* v, float* t) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t w[4];
  philox4x32_10(i, step_lo, step_hi, kTrainBatchTag, seed_lo, seed_hi, w);
  const uint32_t idx = (uint32_t)(((uint64_t)w[0] * (uint64_t)(W * H)) >> 32);   // < W H <= 2^28
  const uint32_t r = idx / W, c = idx - r * W;
  u[i] = (float)r / (float)H;
  v[i] = (float)c / (float)W;
  const float4 x = target[idx];
  t[3u * i] = x.x; t[3u * i + 1u] = x.y; t[3u * i + 2u] = x.z;
}

// Fourier features of the batch as float32, [sin u, sin v, cos u, cos v] x E, into columns col0 .. col0 + 4 E of up to two
// activation buffers (layer 0's input and the concat layer's).  Per value: a = half((coord - 1) 2 2^j), then the correctly
// rounded float sine / cosine of a (through binary64) rounded to half -- the oracle's definition (orc_nif_encode), bit for
// bit.  The inference kernels take v_sin_f32 / v_cos_f32 instead (fourier_group, fast_sincos).  Measured
// (scripts/nif_train_bench.py, profiles/r12_nif_train.txt): on a 64 x 64 texel grid the two agree in all 196608 values; at
// 4096 random (u, v) 112 of 196608 values (0.057 %) differ, each by one step of the half (4.9e-4).  Harmless under the
// inference tolerance of 2e-2, but no input for a gradient check against the float64 model, which takes the oracle's
// features and whose bound is 6.3e-6.  Features carry no gradient.
__global__ __launch_bounds__(256) void train_encode_kernel(const float* u, const float* v, uint32_t n, uint32_t E, float* x0, uint32_t ld0,
                                                           float* x1, uint32_t ld1, uint32_t col1) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n * 2u * E) return;
  const uint32_t s = i / (2u * E), j = i - s * 2u * E, h = j / E, f = j - h * E;
  const float coord = h ? v[s] : u[s];
  const float x = (coord - 1.0f) * 2.0f;
  const float a = (float)(_Float16)(x * (float)(1u << f));
  const float sn = (float)(_Float16)(float)sin((double)a), cs = (float)(_Float16)(float)cos((double)a);
  const uint32_t cs_col = h * E + f, cc_col = 2u * E + cs_col;
  x0[(size_t)s * ld0 + cs_col] = sn;
  x0[(size_t)s * ld0 + cc_col] = cs;
  if (x1) { x1[(size_t)s * ld1 + col1 + cs_col] = sn; x1[(size_t)s * ld1 + col1 + cc_col] = cs; }
}

// ---- one tiled GEMM, three operand forms
//
// C[m][n] = sum_k A(m, k) B(k, n) over k in this block's slab, A(m, k) = A[m a_rs + k a_cs], B(k, n) = B[k b_rs + n b_cs]:
//   forward          Y  = X W        A = X  (k contiguous)   B = W   (n contiguous)   epilogue + bias, ReLU
//   input gradient   dX = dY W^T     A = dY (k contiguous)   B = W^T (k contiguous)   epilogue . (x > 0) on the stored activation
//   weight gradient  dW = X^T dY     A = X^T (m contiguous)  B = dY  (n contiguous)   per-slab partials, no epilogue
// A workgroup of four waves owns a 128 x 64 tile of C, a wave 64 x 32 of it as two 32 x 32 accumulators.  K goes in tiles
// of 16 through LDS, zero-filled past M, N and the slab's end, so any shape runs: K = 3 (the head's dX), N = 3 (the head),
// M = 8 (dW of an E = 2 first layer).  The next tile's global loads are in flight while this one's 16 MFMAs per wave run.
// LDS rows are padded by 33 words: the two half-waves of an operand read (rows k and k + 1) fall on disjoint banks, and the
// k-contiguous tile writes spread over the banks as well.
constexpr int kTgBM = 128, kTgBN = 64, kTgBK = 16, kTgLdA = kTgBM + 33, kTgLdB = kTgBN + 33;
enum { kTrainEpiBias = 0, kTrainEpiMask = 1, kTrainEpiNone = 2 };

struct TrainGemm {
  const float* A; const float* B; float* C;
  uint32_t a_rs, a_cs, b_rs, b_cs, ldc;
  uint32_t M, N, K;
  uint32_t k_slab;             // k range of blockIdx.z: [z k_slab, min(K, (z + 1) k_slab)); C advances by c_slab floats per z
  uint32_t c_slab;
  const float* bias;           // kTrainEpiBias: [N]
  const float* mask;           // kTrainEpiMask: the stored post-ReLU activation, [M][ldmask]
  uint32_t ldmask, relu;
};

template <int EPI>
__global__ __launch_bounds__(256) void train_gemm_kernel(const TrainGemm G) {
  __shared__ float As[kTgBK][kTgLdA];
  __shared__ float Bs[kTgBK][kTgLdB];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t m0 = blockIdx.x * kTgBM, n0 = blockIdx.y * kTgBN;
  const uint32_t kb = blockIdx.z * G.k_slab, ke = min(G.K, kb + G.k_slab);
  const bool a_kfast = G.a_cs == 1u, b_nfast = G.b_cs == 1u;
  float ra[8], rb[4];
  auto load = [&](uint32_t k0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t e = tid + 256u * i;
      const uint32_t k = a_kfast ? (e & 15u) : (e >> 7), m = a_kfast ? (e >> 4) : (e & 127u);
      const bool in = m0 + m < G.M && k0 + k < ke;
      ra[i] = in ? G.A[(size_t)(m0 + m) * G.a_rs + (size_t)(k0 + k) * G.a_cs] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t e = tid + 256u * i;
      const uint32_t k = b_nfast ? (e >> 6) : (e & 15u), n = b_nfast ? (e & 63u) : (e >> 4);
      const bool in = n0 + n < G.N && k0 + k < ke;
      rb[i] = in ? G.B[(size_t)(k0 + k) * G.b_rs + (size_t)(n0 + n) * G.b_cs] : 0.f;
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t e = tid + 256u * i;
      const uint32_t k = a_kfast ? (e & 15u) : (e >> 7), m = a_kfast ? (e >> 4) : (e & 127u);
      As[k][m] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t e = tid + 256u * i;
      const uint32_t k = b_nfast ? (e >> 6) : (e & 15u), n = b_nfast ? (e & 63u) : (e >> 4);
      Bs[k][n] = rb[i];
    }
  };
  const uint32_t wm = 64u * (wave >> 1), wn = 32u * (wave & 1u), r = lane & 31u, kk = lane >> 5;
  f32x16 acc0 = (f32x16)(0.0f), acc1 = (f32x16)(0.0f);
  if (kb < ke) {
    load(kb);
    for (uint32_t k0 = kb; k0 < ke; k0 += kTgBK) {
      stage();
      __syncthreads();
      if (k0 + kTgBK < ke) load(k0 + kTgBK);
#pragma unroll
      for (int ks = 0; ks < kTgBK / 2; ++ks) {   // lane (r, kk): A[m = r][k = kk], B[k = kk][n = r] (cdna_hip_programming.md section 3)
        const float a0 = As[2 * ks + kk][wm + r], a1 = As[2 * ks + kk][wm + 32u + r], b = Bs[2 * ks + kk][wn + r];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc1, 0, 0, 0);
      }
      __syncthreads();
    }
  }
  // D: register i of lane (r, kk) is row 8 (i >> 2) + 4 kk + (i & 3), column r
  float* C = G.C + (size_t)blockIdx.z * G.c_slab;
  const uint32_t col = n0 + wn + r;
  if (col >= G.N) return;
  const float bias = EPI == kTrainEpiBias && G.bias ? G.bias[col] : 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t row = m0 + wm + 32u * t + 8u * (i >> 2) + 4u * kk + (i & 3);
      if (row >= G.M) continue;
      float y = t ? acc1[i] : acc0[i];
      if (EPI == kTrainEpiBias) { y = y + bias; if (G.relu) y = y > 0.f ? y : 0.f; }
      if (EPI == kTrainEpiMask) y = G.mask[(size_t)row * G.ldmask + col] > 0.f ? y : 0.f;
      C[(size_t)row * G.ldc + col] = y;
    }
  }
}

// ---- loss, bias gradient, the slab sum

// g[e] = 2 (y[e] - t[e]) / (3 n), the gradient of the mean squared error over n x 3 values, and per block the tree sum of
// (y - t)^2 in binary64.
__global__ __launch_bounds__(256) void train_loss_kernel(const float* y, const float* t, uint32_t count, float scale, float* g, double* partial) {
  __shared__ double s[256];
  double a = 0.0;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < count; e += gridDim.x * 256u) {
    const float d = y[e] - t[e];
    g[e] = d * scale;
    a += (double)d * (double)d;
  }
  const double r = train_block_reduce<false>(s, a);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}
__global__ __launch_bounds__(256) void train_loss_final_kernel(const double* partial, uint32_t count, float* loss) {
  __shared__ double s[256];
  const double r = train_block_reduce<false>(s, partial[threadIdx.x]);
  if (threadIdx.x == 0) *loss = (float)(r / (double)count);
}

// db partials: block (x, z) sums columns 64 x .. of the rows of slab z -- four row lanes each in row order, then lanes 0..3.
__global__ __launch_bounds__(256) void train_colsum_kernel(const float* g, uint32_t n, uint32_t N, uint32_t slab_rows, float* partial, uint32_t slab_stride) {
  __shared__ float s[4][64];
  const uint32_t c = blockIdx.x * 64u + (threadIdx.x & 63u), rl = threadIdx.x >> 6;
  const uint32_t r0 = blockIdx.y * slab_rows, r1 = min(n, r0 + slab_rows);
  float a = 0.f;
  if (c < N)
    for (uint32_t r = r0 + rl; r < r1; r += 4u) a += g[(size_t)r * N + c];
  s[rl][threadIdx.x & 63u] = a;
  __syncthreads();
  if (rl == 0 && c < N) partial[(size_t)blockIdx.y * slab_stride + c] = ((s[0][threadIdx.x] + s[1][threadIdx.x]) + s[2][threadIdx.x]) + s[3][threadIdx.x];
}

// out[e] = partial[0][e] + partial[1][e] + ... in slab order (dW and, right behind it, db of one layer).
__global__ __launch_bounds__(256) void train_slab_sum_kernel(const float* partial, uint32_t count, uint32_t slab_stride, float* out) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= count) return;
  float a = partial[e];
  for (uint32_t z = 1; z < kTrainSlabs; ++z) a += partial[(size_t)z * slab_stride + e];
  out[e] = a;
}

// ---- Adam, initialisation, export

// Bias-corrected Adam (Kingma & Ba, algorithm 1), c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t) from the host in binary64:
//   m = b1 m + (1 - b1) g,  v = b2 v + (1 - b2) g^2,  w -= lr (m c1) / (sqrt(v c2) + eps)
__global__ __launch_bounds__(256) void train_adam_kernel(float* w, float* m, float* v, const float* g, uint32_t count, float lr, float b1, float b2,
                                                         float eps, float c1, float c2) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= count) return;
  const float ge = g[e];
  const float me = b1 * m[e] + (1.0f - b1) * ge;
  const float ve = b2 * v[e] + ((1.0f - b2) * ge) * ge;
  m[e] = me;
  v[e] = ve;
  w[e] = w[e] - (lr * (me * c1)) / (sqrtf(ve * c2) + eps);
}

// Glorot-uniform kernel of layer `layer`: w[i] = (2 x - 1) limit, x = (word0 >> 8 + 1/2) 2^-24 of Philox block
// (i, layer, 0, "NIFW") keyed by the seed; limit = sqrt(6 / (rows + cols)) from the host.
__global__ __launch_bounds__(256) void train_init_kernel(float* w, uint32_t count, uint32_t layer, uint32_t seed_lo, uint32_t seed_hi, float limit) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  uint32_t r[4];
  philox4x32_10(i, layer, 0u, kTrainInitTag, seed_lo, seed_hi, r);
  const float x = ((float)(r[0] >> 8) + 0.5f) * 5.9604644775390625e-08f;
  w[i] = (2.0f * x - 1.0f) * limit;
}

// binary32 -> binary16, round to nearest even (v_cvt_f16_f32); *overflow = 1 when a finite value became infinite.
__global__ __launch_bounds__(256) void train_export_kernel(const float* w, uint32_t count, uint16_t* out, uint32_t* overflow) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  const float x = w[i];
  const _Float16 hx = (_Float16)x;
  out[i] = __builtin_bit_cast(uint16_t, hx);
  if (fabsf(x) <= 3.4028234663852886e38f && fabsf((float)hx) > 65504.0f) *overflow = 1u;
}

}  // namespace ptd
