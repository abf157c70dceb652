// pt_nif_train.h -- kernels of the on-device NIF trainer (pt_nif_train_*, include/ptmi.h): an HDR environment map in, the
// weights of a Fourier-feature MLP out.  The default path is float32 throughout; the matrix products run on
// v_mfma_f32_32x32x2_f32 (an exact fp32 FMA chain in k order, pt_nif_f32.h).  The opt-in mixed-precision path (binary16 MFMA
// inputs, loss scaling, binary32 masters) is the second half of this file.  Nothing of the sampling loop is touched: the
// trainer runs beside it.
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

// ---- mixed precision (PT_NIF_TRAIN_MIXED_F16, include/ptmi.h): binary16 MFMA inputs, binary32 sums, binary32 masters
//
// Nothing above is touched or called differently; the kernels below run only after pt_nif_train_set_precision asked for the
// mode.  Activations and gradients are halves in buffers whose leading dimension is a multiple of 32 halves, the padding zeroed
// once and never written: every 16-byte load is aligned and what it reads past a tensor's width adds exact zeros.  The weights
// exist three times: the binary32 masters, w16 = half(w) as [rows][ld] and its transpose [cols][ld], both written by the Adam
// kernel, so the forward pass (contraction over the rows of W) and the input gradient (over its columns) both find the
// contraction index contiguous.  The loss scale S and everything derived from it live in a device control block that one
// single-thread kernel updates per step: a step makes no host round trip.

struct TrainCtl {
  float S, inv_S, c;               // the scale, 1 / S (exact: S is a power of two), c = (float)(2 S / (3 n)) of the loss gradient
  float c1, c2;                    // Adam's bias corrections of step applied + 1, from binary64
  uint32_t flag;                   // 1 = a gradient of this pass was not finite (a plain idempotent store)
  uint32_t good;                   // applied steps since S last changed
  uint32_t pad;
  unsigned long long applied, skipped;
};
enum { kTrainCtlInit = 0, kTrainCtlCommit = 1, kTrainCtlPrepare = 2 };

// Init: S and the counters from the arguments.  Commit: the finished step's verdict -- skipped (S halves with `dynamic`, floor 1)
// or applied (S doubles when `good` reaches `growth`, cap 2^30).  Every form then prepares the next pass over n samples.
__global__ void train_ctl_kernel(TrainCtl* ctl, int op, float S0, unsigned long long applied0, int dynamic, uint32_t growth, uint32_t n,
                                 float b1, float b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  TrainCtl k = *ctl;
  if (op == kTrainCtlInit) { k.S = S0; k.good = 0u; k.applied = applied0; k.skipped = 0ull; k.pad = 0u; }
  if (op == kTrainCtlCommit) {
    if (k.flag) {
      k.skipped += 1ull;
      if (dynamic) { k.S = fmaxf(k.S * 0.5f, 1.0f); k.good = 0u; }
    } else {
      k.applied += 1ull;
      k.good += 1u;
      if (dynamic && k.good >= growth) { k.S = fminf(k.S * 2.0f, 1073741824.0f); k.good = 0u; }
    }
  }
  k.flag = 0u;
  k.inv_S = 1.0f / k.S;
  k.c = (float)(2.0 * (double)k.S / (3.0 * (double)n));
  const double t = (double)(k.applied + 1ull);
  k.c1 = (float)(1.0 / (1.0 - pow((double)b1, t)));
  k.c2 = (float)(1.0 / (1.0 - pow((double)b2, t)));
  *ctl = k;
}

// train_encode_kernel with half outputs (the values are halves already).
__global__ __launch_bounds__(256) void train_encode16_kernel(const float* u, const float* v, uint32_t n, uint32_t E, _Float16* x0, uint32_t ld0,
                                                             _Float16* x1, uint32_t ld1, uint32_t col1) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n * 2u * E) return;
  const uint32_t s = i / (2u * E), j = i - s * 2u * E, h = j / E, f = j - h * E;
  const float coord = h ? v[s] : u[s];
  const float x = (coord - 1.0f) * 2.0f;
  const float a = (float)(_Float16)(x * (float)(1u << f));
  const _Float16 sn = (_Float16)(float)sin((double)a), cs = (_Float16)(float)cos((double)a);
  const uint32_t cs_col = h * E + f, cc_col = 2u * E + cs_col;
  x0[(size_t)s * ld0 + cs_col] = sn;
  x0[(size_t)s * ld0 + cc_col] = cs;
  if (x1) { x1[(size_t)s * ld1 + col1 + cs_col] = sn; x1[(size_t)s * ld1 + col1 + cc_col] = cs; }
}

// ---- the half GEMM: C[m][n] = sum_k A(m, k) B(k, n) on v_mfma_f32_32x32x16_f16 (exact products, binary32 accumulation)
//
//   KSLOW = false   A[m lda + k], B[n ldb + k]   forward (X, w16^T) and input gradient (dZ, w16): k contiguous in both
//   KSLOW = true    A[k lda + m], B[k ldb + n]   weight gradient (X, dZ): k is the batch row, the slow index of both
// The tile is that of train_gemm_kernel: 128 x 64 per workgroup of four waves, 64 x 32 per wave as two accumulators; K goes in
// tiles of 32 through LDS in 16-byte chunks, the next tile's global loads in flight under this one's MFMAs, zero-filled past
// the rows of either operand and past the slab's end.  Lane (r, h) of an MFMA wants A[r][8 h + j], B[8 h + j][r], j = 0..7:
//   KSLOW = false: image [row][32 k], 80-byte rows; the fragment is one ds_read_b128 at byte 80 row + 32 ks + 16 h.  Row r
//     starts at dword 20 r, i.e. at 16-byte slot 5 r mod 16 of the 64 banks: a bijection over any 16 rows that differ mod 16.
//     Each of the read's four 16-lane groups (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32) holds such
//     rows at one h: no conflict.  The 16-byte stores (groups of 8 lanes = two rows, 32-bank rule) wrap one of their eight
//     slots onto another: 2-way on 4 banks of 32.
//   KSLOW = true: image [k][row] as it lies in memory, and two ds_read_b64_tr_b16 give the fragment: the 16-lane group g takes
//     the block of k rows 8 (g >> 1) + 4 t .. + 3 (t = 0, 1: elements 0..3, 4..7) and columns 16 (g & 1) .. + 15, its lane
//     4 q + p supplying row q, columns 4 p .. 4 p + 3.  A 32-lane half so reads 4 k rows x 64 contiguous bytes (16 dwords); with
//     rows of 320 bytes (A, 80 dwords) and 192 bytes (B, 48 dwords) the four rows start at banks 0 16 32 48 and 0 48 32 16:
//     disjoint, no conflict by the 64-bank rule; the 16-byte stores of 8 lanes cover 128 contiguous bytes of one row: no
//     conflict either.  Every address is a multiple of 8 bytes; all 64 lanes take part in every read: out-of-range chunks
//     were zero-filled, nothing is masked and no wave leaves before the last read.
constexpr int kHgBM = 128, kHgBN = 64, kHgBK = 32;
constexpr int kHgLdK = 40;                      // halves per row, KSLOW = false (both operands)
constexpr int kHgLdA = 160, kHgLdB = 96;        // halves per k row, KSLOW = true
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 fp16q4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

struct TrainGemm16 {
  const _Float16* A; const _Float16* B;
  void* C;                     // halves, or floats with out_f32 (the head's y) and in the weight gradient
  uint32_t lda, ldb, ldc;
  uint32_t a_rows, b_rows;     // KSLOW = false: rows of A (M) and of B (N) that exist; KSLOW = true: lda, ldb (columns that exist)
  uint32_t M, N, K;
  uint32_t k_slab, c_slab;     // as TrainGemm
  const float* bias;
  const _Float16* mask;
  uint32_t ldmask, relu, out_f32;
};

__device__ __forceinline__ f16x4 train_tr_read(const _Float16* p) {
  return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16q4*)p));
}

template <int EPI, bool KSLOW>
__global__ __launch_bounds__(256) void train_gemm16_kernel(const TrainGemm16 G) {
  __shared__ __attribute__((aligned(16))) _Float16 As[kHgBM * kHgLdK];   // = kHgBK * kHgLdA halves
  __shared__ __attribute__((aligned(16))) _Float16 Bs[kHgBK * kHgLdB];   // >= kHgBN * kHgLdK
  static_assert(kHgBM * kHgLdK == kHgBK * kHgLdA && kHgBK * kHgLdB >= kHgBN * kHgLdK, "one LDS size for both forms");
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t m0 = blockIdx.x * kHgBM, n0 = blockIdx.y * kHgBN;
  const uint32_t kb = blockIdx.z * G.k_slab, ke = min(G.K, kb + G.k_slab);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  uint4 ra[2], rb;
  auto load = [&](uint32_t k0) {
    if (!KSLOW) {   // chunk e: row e >> 2, k chunk e & 3
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t e = tid + 256u * i, row = m0 + (e >> 2), k = k0 + 8u * (e & 3u);
        ra[i] = row < G.a_rows && k < ke ? *(const uint4*)(G.A + (size_t)row * G.lda + k) : zero;
      }
      const uint32_t row = n0 + (tid >> 2), k = k0 + 8u * (tid & 3u);
      rb = row < G.b_rows && k < ke ? *(const uint4*)(G.B + (size_t)row * G.ldb + k) : zero;
    } else {        // A chunk e: k row e >> 4, column chunk e & 15; B chunk: k row tid >> 3, column chunk tid & 7
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t e = tid + 256u * i, k = k0 + (e >> 4), col = m0 + 8u * (e & 15u);
        ra[i] = k < ke && col < G.a_rows ? *(const uint4*)(G.A + (size_t)k * G.lda + col) : zero;
      }
      const uint32_t k = k0 + (tid >> 3), col = n0 + 8u * (tid & 7u);
      rb = k < ke && col < G.b_rows ? *(const uint4*)(G.B + (size_t)k * G.ldb + col) : zero;
    }
  };
  auto stage = [&]() {
    if (!KSLOW) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t e = tid + 256u * i;
        *(uint4*)(As + (e >> 2) * kHgLdK + 8u * (e & 3u)) = ra[i];
      }
      *(uint4*)(Bs + (tid >> 2) * kHgLdK + 8u * (tid & 3u)) = rb;
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t e = tid + 256u * i;
        *(uint4*)(As + (e >> 4) * kHgLdA + 8u * (e & 15u)) = ra[i];
      }
      *(uint4*)(Bs + (tid >> 3) * kHgLdB + 8u * (tid & 7u)) = rb;
    }
  };
  const uint32_t wm = 64u * (wave >> 1), wn = 32u * (wave & 1u), r = lane & 31u, h = lane >> 5;
  // transposed reads: this lane's address inside a 16 (k) x 32 (column) block
  const uint32_t tr_k = 8u * (lane >> 5) + ((lane & 15u) >> 2), tr_c = 16u * ((lane >> 4) & 1u) + 4u * (lane & 3u);
  f32x16 acc0 = (f32x16)(0.0f), acc1 = (f32x16)(0.0f);
  if (kb < ke) {
    load(kb);
    for (uint32_t k0 = kb; k0 < ke; k0 += kHgBK) {
      stage();
      __syncthreads();
      if (k0 + kHgBK < ke) load(k0 + kHgBK);
#pragma unroll
      for (int ks = 0; ks < kHgBK / 16; ++ks) {
        f16x8 a0, a1, b;
        if (!KSLOW) {
          a0 = *(const f16x8*)(As + (wm + r) * kHgLdK + 16 * ks + 8u * h);
          a1 = *(const f16x8*)(As + (wm + 32u + r) * kHgLdK + 16 * ks + 8u * h);
          b = *(const f16x8*)(Bs + (wn + r) * kHgLdK + 16 * ks + 8u * h);
        } else {
          const _Float16* pa = As + (16 * ks + tr_k) * kHgLdA + wm + tr_c;
          const _Float16* pb = Bs + (16 * ks + tr_k) * kHgLdB + wn + tr_c;
          a0 = __builtin_shufflevector(train_tr_read(pa), train_tr_read(pa + 4 * kHgLdA), 0, 1, 2, 3, 4, 5, 6, 7);
          a1 = __builtin_shufflevector(train_tr_read(pa + 32), train_tr_read(pa + 32 + 4 * kHgLdA), 0, 1, 2, 3, 4, 5, 6, 7);
          b = __builtin_shufflevector(train_tr_read(pb), train_tr_read(pb + 4 * kHgLdB), 0, 1, 2, 3, 4, 5, 6, 7);
        }
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b, acc1, 0, 0, 0);
      }
      __syncthreads();
    }
  }
  // D: register i of lane (r, h) is row 8 (i >> 2) + 4 h + (i & 3), column r (no transposed read follows: lanes may leave)
  const uint32_t col = n0 + wn + r;
  if (col >= G.N) return;
  const float bias = EPI == kTrainEpiBias && G.bias ? G.bias[col] : 0.f;
  float* Cf = (float*)G.C + (size_t)blockIdx.z * G.c_slab;
  _Float16* Ch = (_Float16*)G.C;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t row = m0 + wm + 32u * t + 8u * (i >> 2) + 4u * h + (i & 3);
      if (row >= G.M) continue;
      float y = t ? acc1[i] : acc0[i];
      if (EPI == kTrainEpiBias) { y = y + bias; if (G.relu) y = y > 0.f ? y : 0.f; }
      if (EPI == kTrainEpiMask) y = (float)G.mask[(size_t)row * G.ldmask + col] > 0.f ? y : 0.f;
      if (EPI == kTrainEpiNone || G.out_f32) Cf[(size_t)row * G.ldc + col] = y;
      else Ch[(size_t)row * G.ldc + col] = (_Float16)y;
    }
  }
}

// train_loss_kernel for the mixed pass: g[row][col] = half((y - t) c), c from the control block, into rows of 32 halves.
__global__ __launch_bounds__(256) void train_loss16_kernel(const float* y, const float* t, uint32_t count, const TrainCtl* ctl, _Float16* g,
                                                           double* partial) {
  __shared__ double s[256];
  const float c = ctl->c;
  double a = 0.0;
  for (uint32_t e = blockIdx.x * 256u + threadIdx.x; e < count; e += gridDim.x * 256u) {
    const float d = y[e] - t[e];
    const uint32_t row = e / 3u;
    g[(size_t)row * 32u + (e - 3u * row)] = (_Float16)(d * c);
    a += (double)d * (double)d;
  }
  const double r = train_block_reduce<false>(s, a);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// train_colsum_kernel over halves with a leading dimension: binary32 sums in the same order.
__global__ __launch_bounds__(256) void train_colsum16_kernel(const _Float16* g, uint32_t n, uint32_t N, uint32_t ld, uint32_t slab_rows, float* partial,
                                                             uint32_t slab_stride) {
  __shared__ float s[4][64];
  const uint32_t c = blockIdx.x * 64u + (threadIdx.x & 63u), rl = threadIdx.x >> 6;
  const uint32_t r0 = blockIdx.y * slab_rows, r1 = min(n, r0 + slab_rows);
  float a = 0.f;
  if (c < N)
    for (uint32_t r = r0 + rl; r < r1; r += 4u) a += (float)g[(size_t)r * ld + c];
  s[rl][threadIdx.x & 63u] = a;
  __syncthreads();
  if (rl == 0 && c < N) partial[(size_t)blockIdx.y * slab_stride + c] = ((s[0][threadIdx.x] + s[1][threadIdx.x]) + s[2][threadIdx.x]) + s[3][threadIdx.x];
}

// train_slab_sum_kernel, then the unscaling (exact) and the finite check of the scaled sum.
__global__ __launch_bounds__(256) void train_slab_sum_mixed_kernel(const float* partial, uint32_t count, uint32_t slab_stride, float* out, TrainCtl* ctl) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= count) return;
  float a = partial[e];
  for (uint32_t z = 1; z < kTrainSlabs; ++z) a += partial[(size_t)z * slab_stride + e];
  out[e] = a * ctl->inv_S;
  if (!(fabsf(a) <= 3.4028234663852886e38f)) ctl->flag = 1u;
}

// train_adam_kernel on one layer (kernel, then bias) with c1, c2 from the control block; nothing moves when the flag is set.
// The new kernel weights also go out as halves: w16 [rows][ldw] and its transpose [cols][ldt].
__global__ __launch_bounds__(256) void train_adam_mixed_kernel(float* w, float* m, float* v, const float* g, uint32_t rows, uint32_t cols, float lr,
                                                               float b1, float b2, float eps, const TrainCtl* ctl, _Float16* w16, uint32_t ldw,
                                                               _Float16* w16t, uint32_t ldt) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= rows * cols + cols || ctl->flag) return;
  const float c1 = ctl->c1, c2 = ctl->c2;
  const float ge = g[e];
  const float me = b1 * m[e] + (1.0f - b1) * ge;
  const float ve = b2 * v[e] + ((1.0f - b2) * ge) * ge;
  m[e] = me;
  v[e] = ve;
  const float we = w[e] - (lr * (me * c1)) / (sqrtf(ve * c2) + eps);
  w[e] = we;
  if (e < rows * cols) {
    const uint32_t r = e / cols, c = e - r * cols;
    const _Float16 hw = (_Float16)we;
    w16[(size_t)r * ldw + c] = hw;
    w16t[(size_t)c * ldt + r] = hw;
  }
}

// w16 and its transpose from the masters of one layer (set_weights, set_precision).
__global__ __launch_bounds__(256) void train_half_copy_kernel(const float* w, uint32_t rows, uint32_t cols, _Float16* w16, uint32_t ldw, _Float16* w16t,
                                                              uint32_t ldt) {
  const uint32_t e = blockIdx.x * 256u + threadIdx.x;
  if (e >= rows * cols) return;
  const uint32_t r = e / cols, c = e - r * cols;
  const _Float16 hw = (_Float16)w[e];
  w16[(size_t)r * ldw + c] = hw;
  w16t[(size_t)c * ldt + r] = hw;
}

}  // namespace ptd
