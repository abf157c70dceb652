// ptmi_nif_train.h -- host side of the NIF trainer (pt_nif_train_*, include/ptmi.h): the trainer's buffers and the launch
// sequence of a step (kernels: pt_nif_train.h).  Part of the one translation unit ptmi.hip, included last, after ptmi_denoise.h.
// Everything runs on the handle's stream; nothing here is reached by a process that never calls pt_nif_train_begin.
#pragma once

namespace {

inline uint32_t train_blocks(size_t n) { return (uint32_t)((n + 255) / 256); }
void train_draw_batch(pt_handle h, NifTrainState& st, uint64_t step);

template <int EPI>
void train_launch_gemm(pt_handle h, const ptd::TrainGemm& G, uint32_t slabs) {
  const dim3 grid((G.M + ptd::kTgBM - 1) / ptd::kTgBM, (G.N + ptd::kTgBN - 1) / ptd::kTgBN, slabs);
  hipLaunchKernelGGL((ptd::train_gemm_kernel<EPI>), grid, dim3(256), 0, h->stream, G);
}

// Fourier features of the n samples in d_u / d_vv into layer 0's input and into the concat layer's feature columns.
void train_encode(pt_handle h, NifTrainState& st, uint32_t n) {
  const uint32_t E = st.p.embedding_dim;
  float* x1 = st.skip ? (float*)st.d_act[st.skip] : nullptr;
  hipLaunchKernelGGL(ptd::train_encode_kernel, dim3(train_blocks((size_t)n * 2 * E)), dim3(256), 0, h->stream, st.d_u, st.d_vv, n, E,
                     st.d_act[0], st.layers[0].rows, x1, st.skip ? st.layers[st.skip].rows : 0u, st.p.hidden);
}

// Forward pass, loss (into d_enc[4]) and backward pass over the n samples whose features and targets are in place: every dW
// and db into the gradient blob.
int train_forward_backward(pt_handle h, NifTrainState& st, uint32_t n) {
  const size_t L = st.layers.size();
  for (size_t l = 0; l < L; ++l) {   // Y = X W + b, ReLU: straight into the next layer's input buffer
    const NifTrainState::Layer& Y = st.layers[l];
    ptd::TrainGemm G{};
    G.A = st.d_act[l]; G.a_rs = Y.rows; G.a_cs = 1;
    G.B = st.d_w + Y.w_off; G.b_rs = Y.cols; G.b_cs = 1;
    G.C = l + 1 < L ? (float*)st.d_act[l + 1] : (float*)st.d_y;
    G.ldc = l + 1 < L ? st.layers[l + 1].rows : 3u;
    G.M = n; G.N = Y.cols; G.K = Y.rows; G.k_slab = Y.rows;
    G.bias = st.d_w + Y.b_off; G.relu = Y.relu;
    train_launch_gemm<ptd::kTrainEpiBias>(h, G, 1);
  }
  hipLaunchKernelGGL(ptd::train_loss_kernel, dim3(ptd::kTrainStatBlocks), dim3(256), 0, h->stream, st.d_y, st.d_t, 3u * n,
                     (float)(2.0 / (3.0 * (double)n)), st.d_dz[0], st.d_red);
  hipLaunchKernelGGL(ptd::train_loss_final_kernel, dim3(1), dim3(256), 0, h->stream, st.d_red, 3u * n, st.d_enc + 4);
  const uint32_t slab_rows = ((n + ptd::kTrainSlabs - 1) / ptd::kTrainSlabs + ptd::kTgBK - 1) / ptd::kTgBK * ptd::kTgBK;
  int cur = 0;
  for (size_t l = L; l-- > 0;) {
    const NifTrainState::Layer& Y = st.layers[l];
    ptd::TrainGemm W{};   // dW = X^T dZ over the batch, one partial per slab
    W.A = st.d_act[l]; W.a_rs = 1; W.a_cs = Y.rows;
    W.B = st.d_dz[cur]; W.b_rs = Y.cols; W.b_cs = 1;
    W.C = st.d_partial; W.ldc = Y.cols;
    W.M = Y.rows; W.N = Y.cols; W.K = n; W.k_slab = slab_rows; W.c_slab = (uint32_t)st.partial_stride;
    train_launch_gemm<ptd::kTrainEpiNone>(h, W, ptd::kTrainSlabs);
    hipLaunchKernelGGL(ptd::train_colsum_kernel, dim3((Y.cols + 63) / 64, ptd::kTrainSlabs), dim3(256), 0, h->stream, st.d_dz[cur], n, Y.cols,
                       slab_rows, st.d_partial + (size_t)Y.rows * Y.cols, (uint32_t)st.partial_stride);
    const uint32_t count = Y.rows * Y.cols + Y.cols;
    hipLaunchKernelGGL(ptd::train_slab_sum_kernel, dim3(train_blocks(count)), dim3(256), 0, h->stream, st.d_partial, count,
                       (uint32_t)st.partial_stride, st.d_g + Y.w_off);
    if (l == 0) break;
    const NifTrainState::Layer& X = st.layers[l - 1];
    ptd::TrainGemm D{};   // dZ of the layer below = (dZ W^T)[:, :cols below] . (x > 0); the feature columns of a concat layer are dropped
    D.A = st.d_dz[cur]; D.a_rs = Y.cols; D.a_cs = 1;
    D.B = st.d_w + Y.w_off; D.b_rs = 1; D.b_cs = Y.cols;
    D.C = st.d_dz[cur ^ 1]; D.ldc = X.cols;
    D.M = n; D.N = X.cols; D.K = Y.cols; D.k_slab = Y.cols;
    D.mask = st.d_act[l]; D.ldmask = Y.rows;
    train_launch_gemm<ptd::kTrainEpiMask>(h, D, 1);
    cur ^= 1;
  }
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// ---- mixed precision (pt_nif_train_set_precision): the same sequence on the half kernels

inline uint32_t train_round32(uint32_t x) { return (x + 31u) / 32u * 32u; }
inline bool train_mixed(const NifTrainState& st) { return st.prec.mode == PT_NIF_TRAIN_MIXED_F16; }

template <int EPI, bool KSLOW>
void train_launch_gemm16(pt_handle h, const ptd::TrainGemm16& G, uint32_t slabs) {
  const dim3 grid((G.M + ptd::kHgBM - 1) / ptd::kHgBM, (G.N + ptd::kHgBN - 1) / ptd::kHgBN, slabs);
  hipLaunchKernelGGL((ptd::train_gemm16_kernel<EPI, KSLOW>), grid, dim3(256), 0, h->stream, G);
}

// The control block's kernel: kTrainCtlInit (S and the counters), kTrainCtlCommit (a finished step) or kTrainCtlPrepare; each
// leaves the block ready for a pass over n samples.
void train_ctl(pt_handle h, NifTrainState& st, int op, uint32_t n, float S0 = 0.f, uint64_t applied0 = 0) {
  hipLaunchKernelGGL(ptd::train_ctl_kernel, dim3(1), dim3(1), 0, h->stream, st.d_ctl, op, S0, (unsigned long long)applied0,
                     st.prec.dynamic, st.prec.growth_interval, n, st.p.beta1, st.p.beta2);
}

// w16 and its transpose from the masters.
void train_refresh_half(pt_handle h, NifTrainState& st) {
  for (size_t l = 0; l < st.layers.size(); ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    const NifTrainState::Layer16& H = st.layers16[l];
    hipLaunchKernelGGL(ptd::train_half_copy_kernel, dim3(train_blocks((size_t)Y.rows * Y.cols)), dim3(256), 0, h->stream, st.d_w + Y.w_off, Y.rows,
                       Y.cols, (_Float16*)(uint16_t*)st.d_w16 + H.w16_off, H.ldw, (_Float16*)(uint16_t*)st.d_w16t + H.w16t_off, H.ldt);
  }
}

void train_encode16(pt_handle h, NifTrainState& st, uint32_t n) {
  const uint32_t E = st.p.embedding_dim;
  _Float16* x1 = st.skip ? (_Float16*)(uint16_t*)st.d_act16[st.skip] : nullptr;
  hipLaunchKernelGGL(ptd::train_encode16_kernel, dim3(train_blocks((size_t)n * 2 * E)), dim3(256), 0, h->stream, st.d_u, st.d_vv, n, E,
                     (_Float16*)(uint16_t*)st.d_act16[0], st.layers16[0].ldx, x1, st.skip ? st.layers16[st.skip].ldx : 0u, st.p.hidden);
}

// train_forward_backward in mixed precision: the scaled loss gradient from the control block's c, every dW and db unscaled
// into the gradient blob, the control block's flag set where one is not finite.
int train_forward_backward_mixed(pt_handle h, NifTrainState& st, uint32_t n) {
  const size_t L = st.layers.size();
  auto act = [&](size_t l) { return (_Float16*)(uint16_t*)st.d_act16[l]; };
  _Float16* w16 = (_Float16*)(uint16_t*)st.d_w16;
  _Float16* w16t = (_Float16*)(uint16_t*)st.d_w16t;
  _Float16* dzh = (_Float16*)(uint16_t*)st.d_dzh16;
  _Float16* dz[2] = {(_Float16*)(uint16_t*)st.d_dz16[0], (_Float16*)(uint16_t*)st.d_dz16[1]};
  for (size_t l = 0; l < L; ++l) {   // Y = X w16 + b, ReLU, half: straight into the next layer's input buffer
    const NifTrainState::Layer& Y = st.layers[l];
    const NifTrainState::Layer16& H = st.layers16[l];
    ptd::TrainGemm16 G{};
    G.A = act(l); G.lda = H.ldx; G.a_rows = n;
    G.B = w16t + H.w16t_off; G.ldb = H.ldt; G.b_rows = Y.cols;
    G.C = l + 1 < L ? (void*)act(l + 1) : (void*)(float*)st.d_y;
    G.ldc = l + 1 < L ? st.layers16[l + 1].ldx : 3u;
    G.out_f32 = l + 1 < L ? 0u : 1u;
    G.M = n; G.N = Y.cols; G.K = Y.rows; G.k_slab = Y.rows;
    G.bias = st.d_w + Y.b_off; G.relu = Y.relu;
    train_launch_gemm16<ptd::kTrainEpiBias, false>(h, G, 1);
  }
  hipLaunchKernelGGL(ptd::train_loss16_kernel, dim3(ptd::kTrainStatBlocks), dim3(256), 0, h->stream, st.d_y, st.d_t, 3u * n, st.d_ctl, dzh, st.d_red);
  hipLaunchKernelGGL(ptd::train_loss_final_kernel, dim3(1), dim3(256), 0, h->stream, st.d_red, 3u * n, st.d_enc + 4);
  const uint32_t slab_rows = ((n + ptd::kTrainSlabs - 1) / ptd::kTrainSlabs + ptd::kHgBK - 1) / ptd::kHgBK * ptd::kHgBK;
  const _Float16* g = dzh;   // dZ of the layer at hand and its leading dimension
  uint32_t ldg = 32u;
  int next = 0;
  for (size_t l = L; l-- > 0;) {
    const NifTrainState::Layer& Y = st.layers[l];
    const NifTrainState::Layer16& H = st.layers16[l];
    ptd::TrainGemm16 W{};   // dW = X^T dZ over the batch, one binary32 partial per slab
    W.A = act(l); W.lda = H.ldx; W.a_rows = H.ldx;
    W.B = g; W.ldb = ldg; W.b_rows = ldg;
    W.C = (float*)st.d_partial; W.ldc = Y.cols;
    W.M = Y.rows; W.N = Y.cols; W.K = n; W.k_slab = slab_rows; W.c_slab = (uint32_t)st.partial_stride;
    train_launch_gemm16<ptd::kTrainEpiNone, true>(h, W, ptd::kTrainSlabs);
    hipLaunchKernelGGL(ptd::train_colsum16_kernel, dim3((Y.cols + 63) / 64, ptd::kTrainSlabs), dim3(256), 0, h->stream, g, n, Y.cols, ldg, slab_rows,
                       st.d_partial + (size_t)Y.rows * Y.cols, (uint32_t)st.partial_stride);
    const uint32_t count = Y.rows * Y.cols + Y.cols;
    hipLaunchKernelGGL(ptd::train_slab_sum_mixed_kernel, dim3(train_blocks(count)), dim3(256), 0, h->stream, st.d_partial, count,
                       (uint32_t)st.partial_stride, st.d_g + Y.w_off, st.d_ctl);
    if (l == 0) break;
    const NifTrainState::Layer& X = st.layers[l - 1];
    ptd::TrainGemm16 D{};   // dZ below = half((dZ w16^T)[:, :cols below] . (a > 0)); B(k, n) = w16[n][k], the rows below X.cols only
    D.A = g; D.lda = ldg; D.a_rows = n;
    D.B = w16 + H.w16_off; D.ldb = H.ldw; D.b_rows = X.cols;
    D.C = dz[next]; D.ldc = X.cols;
    D.M = n; D.N = X.cols; D.K = Y.cols; D.k_slab = Y.cols;
    D.mask = act(l); D.ldmask = H.ldx;
    train_launch_gemm16<ptd::kTrainEpiMask, false>(h, D, 1);
    g = dz[next]; ldg = X.cols;
    next ^= 1;
  }
  PT_HIP(hipGetLastError());
  return PT_OK;
}

// The half buffers and the control block of the model in st, into `to` (which may be st itself only through a temporary).
int train_alloc_mixed(pt_handle h, const NifTrainState& st, NifTrainState& to) {
  const size_t L = st.layers.size(), batch = st.p.batch;
  to.layers16.clear();
  size_t w16 = 0, w16t = 0;
  for (size_t l = 0; l < L; ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    NifTrainState::Layer16 H{train_round32(Y.rows), train_round32(Y.cols), train_round32(Y.rows), w16, w16t};
    w16 += (size_t)Y.rows * H.ldw;
    w16t += (size_t)Y.cols * H.ldt;
    to.layers16.push_back(H);
  }
  to.d_act16.clear();
  to.d_act16.resize(L);
  for (size_t l = 0; l < L; ++l) PT_HIP(dev_alloc(to.d_act16[l], batch * to.layers16[l].ldx));
  for (auto& g : to.d_dz16) PT_HIP(dev_alloc(g, batch * st.p.hidden));
  PT_HIP(dev_alloc(to.d_dzh16, batch * 32));
  PT_HIP(dev_alloc(to.d_w16, w16));
  PT_HIP(dev_alloc(to.d_w16t, w16t));
  PT_HIP(dev_alloc(to.d_ctl, 1));
  // the padding is zeroed here, once: no kernel writes it
  for (size_t l = 0; l < L; ++l) PT_HIP(hipMemsetAsync(to.d_act16[l], 0, batch * to.layers16[l].ldx * 2, h->stream));
  for (auto& g : to.d_dz16) PT_HIP(hipMemsetAsync(g, 0, batch * st.p.hidden * 2, h->stream));
  PT_HIP(hipMemsetAsync(to.d_dzh16, 0, batch * 32 * 2, h->stream));
  PT_HIP(hipMemsetAsync(to.d_w16, 0, w16 * 2, h->stream));
  PT_HIP(hipMemsetAsync(to.d_w16t, 0, w16t * 2, h->stream));
  PT_HIP(hipMemsetAsync(to.d_ctl, 0, sizeof(ptd::TrainCtl), h->stream));
  return PT_OK;
}

void train_free_mixed(NifTrainState& st) {
  st.layers16.clear();
  st.d_act16.clear();
  for (auto& g : st.d_dz16) g.reset();
  st.d_dzh16.reset(); st.d_w16.reset(); st.d_w16t.reset(); st.d_ctl.reset();
}

int train_read_ctl(pt_handle h, NifTrainState& st, ptd::TrainCtl* out) {
  PT_HIP(hipMemcpyAsync(out, st.d_ctl, sizeof(ptd::TrainCtl), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  return PT_OK;
}

// pt_nif_train_steps in mixed precision: per step one control-block kernel, no host round trip.
int train_steps_mixed(pt_handle h, NifTrainState& st, uint32_t n, float* last_loss) {
  auto run = [&]() -> int {
    for (uint32_t i = 0; i < n; ++i) {
      train_draw_batch(h, st, st.step);
      train_encode16(h, st, st.p.batch);
      if (int rc = train_forward_backward_mixed(h, st, st.p.batch)) return rc;
      for (size_t l = 0; l < st.layers.size(); ++l) {
        const NifTrainState::Layer& Y = st.layers[l];
        const NifTrainState::Layer16& H = st.layers16[l];
        hipLaunchKernelGGL(ptd::train_adam_mixed_kernel, dim3(train_blocks((size_t)Y.rows * Y.cols + Y.cols)), dim3(256), 0, h->stream, st.d_w + Y.w_off,
                           st.d_m + Y.w_off, st.d_v + Y.w_off, st.d_g + Y.w_off, Y.rows, Y.cols, st.p.learning_rate, st.p.beta1, st.p.beta2,
                           st.p.adam_eps, st.d_ctl, (_Float16*)(uint16_t*)st.d_w16 + H.w16_off, H.ldw, (_Float16*)(uint16_t*)st.d_w16t + H.w16t_off,
                           H.ldt);
      }
      train_ctl(h, st, ptd::kTrainCtlCommit, st.p.batch);
      st.step += 1;
    }
    PT_HIP(hipGetLastError());
    float loss = 0.f;
    PT_HIP(hipMemcpyAsync(&loss, st.d_enc + 4, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipStreamSynchronize(h->stream));
    if (last_loss) *last_loss = loss;
    return PT_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

void train_draw_batch(pt_handle h, NifTrainState& st, uint64_t step) {
  hipLaunchKernelGGL(ptd::train_batch_kernel, dim3(train_blocks(st.p.batch)), dim3(256), 0, h->stream, st.d_target, st.map_w, st.map_h,
                     st.p.batch, (uint32_t)st.p.seed, (uint32_t)(st.p.seed >> 32), (uint32_t)step, (uint32_t)(step >> 32), st.d_u, st.d_vv,
                     st.d_t);
}

int train_need(pt_handle h, const char* fn) {
  if (!h->train) return fail(h, PT_ERR_NOT_READY, std::string(fn) + ": no trainer (pt_nif_train_begin has not been called, or pt_nif_train_end has)");
  return PT_OK;
}

// The caller's pt_layer array against the model: count and shapes; "" = fine.
std::string train_check_layers(const NifTrainState& st, const pt_layer* layers, uint32_t n_layers, const char* fn, bool need_kernel) {
  if (!layers) return std::string(fn) + ": null layer array";
  if (n_layers != st.layers.size()) return std::string(fn) + ": n_layers must be " + std::to_string(st.layers.size()) + " (got " + std::to_string(n_layers) + ")";
  for (uint32_t l = 0; l < n_layers; ++l) {
    if (layers[l].rows != st.layers[l].rows || layers[l].cols != st.layers[l].cols)
      return std::string(fn) + ": layer " + std::to_string(l) + " must be " + std::to_string(st.layers[l].rows) + " x " + std::to_string(st.layers[l].cols) +
             " (got " + std::to_string(layers[l].rows) + " x " + std::to_string(layers[l].cols) + ")";
    if (need_kernel && !layers[l].kernel) return std::string(fn) + ": layer " + std::to_string(l) + " has a null kernel";
  }
  return "";
}

// A device blob of n_params elements out into the caller's per-layer buffers.
template <typename T>
int train_blob_out(pt_handle h, const NifTrainState& st, const T* d_blob, pt_layer* layers, int32_t dtype) {
  std::vector<T> host(st.n_params);
  PT_HIP(hipMemcpyAsync(host.data(), d_blob, st.n_params * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  for (size_t l = 0; l < st.layers.size(); ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    if (layers[l].kernel) memcpy(const_cast<void*>(layers[l].kernel), host.data() + Y.w_off, (size_t)Y.rows * Y.cols * sizeof(T));
    if (layers[l].bias) memcpy(const_cast<void*>(layers[l].bias), host.data() + Y.b_off, (size_t)Y.cols * sizeof(T));
    layers[l].dtype = dtype;
    layers[l].relu = (int32_t)Y.relu;
  }
  return PT_OK;
}

// The master weights rounded to binary16 into d_half; a finite weight that became infinite names its layer.
int train_round_to_half(pt_handle h, NifTrainState& st) {
  const size_t L = st.layers.size();
  PT_HIP(hipMemsetAsync(st.d_overflow, 0, L * sizeof(uint32_t), h->stream));
  for (size_t l = 0; l < L; ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    const uint32_t count = Y.rows * Y.cols + Y.cols;
    hipLaunchKernelGGL(ptd::train_export_kernel, dim3(train_blocks(count)), dim3(256), 0, h->stream, st.d_w + Y.w_off, count, st.d_half + Y.w_off,
                       st.d_overflow + l);
  }
  PT_HIP(hipGetLastError());
  std::vector<uint32_t> over(L);
  PT_HIP(hipMemcpyAsync(over.data(), st.d_overflow, L * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  for (size_t l = 0; l < L; ++l)
    if (over[l]) return fail(h, PT_ERR_UNSUPPORTED_MODEL, "pt_nif_train_export: layer " + std::to_string(l) + " has a weight that rounds to infinity in binary16");
  return PT_OK;
}

}  // namespace

extern "C" {

int pt_nif_train_default_params(pt_nif_train_params* p) {
  if (!p) return PT_ERR_INVALID_ARGUMENT;
  *p = ptniftrain::defaults();
  return PT_OK;
}

int pt_nif_train_begin(pt_handle h, const pt_nif_train_params* params) {
  // the checks that need no device come first; without a handle the message goes where pt_last_error(NULL) reads it
  const std::string bad = ptniftrain::check(params);
  if (!bad.empty()) {
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_nif_train_begin: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  if (!h->env_map) return fail(h, PT_ERR_NOT_READY, "pt_nif_train_begin: no environment map on the handle (pt_set_env_map has not been called, or a NIF or a constant has replaced the map)");
  PT_HIP(hipSetDevice(h->cfg.device));
  // the new trainer is built aside: whatever fails below, an earlier one stays in force
  auto fresh = std::make_unique<NifTrainState>();
  NifTrainState& st = *fresh;
  st.p = *params;
  st.prec = ptniftrain::default_precision();
  st.map_w = h->env_w; st.map_h = h->env_h;
  st.skip = params->layer_count / 2;
  size_t largest = 0;
  for (const ptniftrain::Shape& s : ptniftrain::shapes(*params)) {
    NifTrainState::Layer Y{s.rows, s.cols, s.relu ? 1u : 0u, st.n_params, st.n_params + (size_t)s.rows * s.cols};
    st.n_params += (size_t)s.rows * s.cols + s.cols;
    largest = std::max(largest, (size_t)s.rows * s.cols + s.cols);
    st.layers.push_back(Y);
  }
  const size_t L = st.layers.size(), batch = params->batch, texels = (size_t)st.map_w * st.map_h;
  st.partial_stride = largest;
  PT_HIP(dev_alloc(st.d_target, texels));
  for (DevBuf<float>* b : {&st.d_w, &st.d_g, &st.d_m, &st.d_v}) PT_HIP(dev_alloc(*b, st.n_params));
  PT_HIP(dev_alloc(st.d_u, batch));
  PT_HIP(dev_alloc(st.d_vv, batch));
  PT_HIP(dev_alloc(st.d_t, batch * 3));
  st.d_act.resize(L);
  for (size_t l = 0; l < L; ++l) PT_HIP(dev_alloc(st.d_act[l], batch * st.layers[l].rows));
  PT_HIP(dev_alloc(st.d_y, batch * 3));
  for (auto& g : st.d_dz) PT_HIP(dev_alloc(g, batch * params->hidden));
  PT_HIP(dev_alloc(st.d_partial, (size_t)ptd::kTrainSlabs * st.partial_stride));
  PT_HIP(dev_alloc(st.d_red, (size_t)ptd::kTrainStatBlocks * 3));
  PT_HIP(dev_alloc(st.d_enc, 8));
  PT_HIP(dev_alloc(st.d_half, st.n_params));
  PT_HIP(dev_alloc(st.d_overflow, L));
  // encode parameters: the mean first, then the largest deviation from it (rounded to binary32 as it is returned)
  const uint32_t n = (uint32_t)texels;
  hipLaunchKernelGGL(ptd::train_stat_kernel<0>, dim3(ptd::kTrainStatBlocks), dim3(256), 0, h->stream, h->d_env_texels, n, params->eps,
                     params->log_tone_map, st.d_enc, st.d_red);
  hipLaunchKernelGGL(ptd::train_stat_final_kernel<0>, dim3(1), dim3(256), 0, h->stream, st.d_red, n, st.d_enc);
  hipLaunchKernelGGL(ptd::train_stat_kernel<1>, dim3(ptd::kTrainStatBlocks), dim3(256), 0, h->stream, h->d_env_texels, n, params->eps,
                     params->log_tone_map, st.d_enc, st.d_red);
  hipLaunchKernelGGL(ptd::train_stat_final_kernel<1>, dim3(1), dim3(256), 0, h->stream, st.d_red, n, st.d_enc);
  hipLaunchKernelGGL(ptd::train_target_kernel, dim3(train_blocks(texels)), dim3(256), 0, h->stream, h->d_env_texels, n, params->eps,
                     params->log_tone_map, st.d_enc, st.d_target);
  PT_HIP(hipGetLastError());
  // Glorot-uniform kernels, zero biases and moments
  for (DevBuf<float>* b : {&st.d_w, &st.d_m, &st.d_v}) PT_HIP(hipMemsetAsync(*b, 0, st.n_params * sizeof(float), h->stream));
  for (size_t l = 0; l < L; ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    hipLaunchKernelGGL(ptd::train_init_kernel, dim3(train_blocks((size_t)Y.rows * Y.cols)), dim3(256), 0, h->stream, st.d_w + Y.w_off,
                       Y.rows * Y.cols, (uint32_t)l, (uint32_t)params->seed, (uint32_t)(params->seed >> 32),
                       sqrtf(6.0f / (float)(Y.rows + Y.cols)));
  }
  PT_HIP(hipGetLastError());
  float enc[4];
  const hipError_t e = hipMemcpyAsync(enc, st.d_enc, sizeof(enc), hipMemcpyDeviceToHost, h->stream);
  const hipError_t s = hipStreamSynchronize(h->stream);   // (also: no kernel reads the map's texels once this call has returned)
  PT_HIP(e);
  PT_HIP(s);
  if (!(enc[3] > 0.f) || !std::isfinite(enc[3]))
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_begin: the environment map is constant (max |L - mean| = 0): there is nothing to train on");
  memcpy(st.mean, enc, 12);
  st.max = enc[3];
  h->train = std::move(fresh);
  return PT_OK;
}

int pt_nif_train_layer_shapes(pt_handle h, pt_layer* layers, uint32_t n_layers) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_layer_shapes")) return rc;
  const NifTrainState& st = *h->train;
  if (!layers || n_layers != st.layers.size())
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_layer_shapes: n_layers must be " + std::to_string(st.layers.size()));
  for (uint32_t l = 0; l < n_layers; ++l) {
    layers[l].rows = st.layers[l].rows; layers[l].cols = st.layers[l].cols;
    layers[l].dtype = PT_DTYPE_F32; layers[l].relu = (int32_t)st.layers[l].relu;
  }
  return PT_OK;
}

int pt_nif_train_steps(pt_handle h, uint32_t n, float* last_loss) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_steps")) return rc;
  if (n == 0) return PT_OK;
  NifTrainState& st = *h->train;
  PT_HIP(hipSetDevice(h->cfg.device));
  if (train_mixed(st)) return train_steps_mixed(h, st, n, last_loss);
  auto run = [&]() -> int {
    for (uint32_t i = 0; i < n; ++i) {
      train_draw_batch(h, st, st.step);
      train_encode(h, st, st.p.batch);
      if (int rc = train_forward_backward(h, st, st.p.batch)) return rc;
      const double t = (double)(st.step + 1);
      const float c1 = (float)(1.0 / (1.0 - std::pow((double)st.p.beta1, t))), c2 = (float)(1.0 / (1.0 - std::pow((double)st.p.beta2, t)));
      hipLaunchKernelGGL(ptd::train_adam_kernel, dim3(train_blocks(st.n_params)), dim3(256), 0, h->stream, st.d_w, st.d_m, st.d_v, st.d_g,
                         (uint32_t)st.n_params, st.p.learning_rate, st.p.beta1, st.p.beta2, st.p.adam_eps, c1, c2);
      st.step += 1;
    }
    PT_HIP(hipGetLastError());
    float loss = 0.f;
    PT_HIP(hipMemcpyAsync(&loss, st.d_enc + 4, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipStreamSynchronize(h->stream));
    if (last_loss) *last_loss = loss;
    return PT_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

int pt_nif_train_get_weights(pt_handle h, pt_layer* layers, uint32_t n_layers) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_get_weights")) return rc;
  const std::string bad = train_check_layers(*h->train, layers, n_layers, "pt_nif_train_get_weights", true);
  if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);
  PT_HIP(hipSetDevice(h->cfg.device));
  return train_blob_out<float>(h, *h->train, h->train->d_w, layers, PT_DTYPE_F32);
}

int pt_nif_train_set_weights(pt_handle h, const pt_layer* layers, uint32_t n_layers) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_set_weights")) return rc;
  NifTrainState& st = *h->train;
  const std::string bad = train_check_layers(st, layers, n_layers, "pt_nif_train_set_weights", true);
  if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);
  for (uint32_t l = 0; l < n_layers; ++l)
    if (layers[l].dtype != PT_DTYPE_F32) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_set_weights: layer " + std::to_string(l) + " must be PT_DTYPE_F32");
  std::vector<float> host(st.n_params, 0.f);
  for (uint32_t l = 0; l < n_layers; ++l) {
    const NifTrainState::Layer& Y = st.layers[l];
    memcpy(host.data() + Y.w_off, layers[l].kernel, (size_t)Y.rows * Y.cols * sizeof(float));
    if (layers[l].bias) memcpy(host.data() + Y.b_off, layers[l].bias, (size_t)Y.cols * sizeof(float));
  }
  PT_HIP(hipSetDevice(h->cfg.device));
  PT_HIP(hipMemcpyAsync(st.d_w, host.data(), st.n_params * sizeof(float), hipMemcpyHostToDevice, h->stream));
  PT_HIP(hipMemsetAsync(st.d_m, 0, st.n_params * sizeof(float), h->stream));
  PT_HIP(hipMemsetAsync(st.d_v, 0, st.n_params * sizeof(float), h->stream));
  if (train_mixed(st)) {   // w16 follows the masters; applied and skipped steps return to 0, S stays
    ptd::TrainCtl now{};
    PT_HIP(hipMemcpyAsync(&now, st.d_ctl, sizeof(now), hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipStreamSynchronize(h->stream));
    train_refresh_half(h, st);
    train_ctl(h, st, ptd::kTrainCtlInit, st.p.batch, now.S, 0);
    PT_HIP(hipGetLastError());
  }
  PT_HIP(hipStreamSynchronize(h->stream));
  st.step = 0;
  return PT_OK;
}

int pt_nif_train_get_encode_params(pt_handle h, float* max, float mean[3]) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_get_encode_params")) return rc;
  if (!max || !mean) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_get_encode_params: null output");
  *max = h->train->max;
  memcpy(mean, h->train->mean, 12);
  return PT_OK;
}

int pt_nif_train_export(pt_handle h, pt_layer* layers, uint32_t n_layers) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_export")) return rc;
  const std::string bad = train_check_layers(*h->train, layers, n_layers, "pt_nif_train_export", true);
  if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);
  PT_HIP(hipSetDevice(h->cfg.device));
  if (int rc = train_round_to_half(h, *h->train)) return rc;
  return train_blob_out<uint16_t>(h, *h->train, h->train->d_half, layers, PT_DTYPE_F16);
}

int pt_nif_train_install(pt_handle h) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_install")) return rc;
  NifTrainState& st = *h->train;
  PT_HIP(hipSetDevice(h->cfg.device));
  if (int rc = train_round_to_half(h, st)) return rc;
  std::vector<uint16_t> host(st.n_params);
  PT_HIP(hipMemcpyAsync(host.data(), st.d_half, st.n_params * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  std::vector<pt_layer> layers(st.layers.size());
  for (size_t l = 0; l < layers.size(); ++l)
    layers[l] = pt_layer{st.layers[l].rows, st.layers[l].cols, host.data() + st.layers[l].w_off, host.data() + st.layers[l].b_off, PT_DTYPE_F16,
                         (int32_t)st.layers[l].relu};
  float mean[3];
  for (int k = 0; k < 3; ++k) {   // the loaders' fold (NifMetaData.cpp:48-53): mean - eps in binary32, log mode only
    const float folded = st.mean[k] - st.p.eps;
    mean[k] = st.p.log_tone_map ? folded : st.mean[k];
  }
  return pt_upload_nif(h, layers.data(), (uint32_t)layers.size(), st.p.embedding_dim, st.max, mean, st.p.log_tone_map);
}

int pt_nif_train_default_precision(pt_nif_train_precision* p) {
  if (!p) return PT_ERR_INVALID_ARGUMENT;
  *p = ptniftrain::default_precision();
  return PT_OK;
}

int pt_nif_train_set_precision(pt_handle h, const pt_nif_train_precision* p) {
  const std::string bad = ptniftrain::check_precision(p);
  if (!bad.empty()) {
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_nif_train_set_precision: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  if (int rc = train_need(h, "pt_nif_train_set_precision")) return rc;
  NifTrainState& st = *h->train;
  PT_HIP(hipSetDevice(h->cfg.device));
  uint64_t applied = st.step;   // PT_NIF_TRAIN_F32 skips nothing
  if (train_mixed(st)) {
    ptd::TrainCtl now{};
    if (int rc = train_read_ctl(h, st, &now)) return rc;
    applied = now.applied;
  } else {
    PT_HIP(hipStreamSynchronize(h->stream));
  }
  if (p->mode == PT_NIF_TRAIN_MIXED_F16 && !train_mixed(st)) {
    NifTrainState fresh;   // built aside: whatever fails, the mode in force stays
    const int rc = train_alloc_mixed(h, st, fresh);
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    st.layers16 = std::move(fresh.layers16);
    st.d_act16 = std::move(fresh.d_act16);
    for (int i = 0; i < 2; ++i) st.d_dz16[i] = std::move(fresh.d_dz16[i]);
    st.d_dzh16 = std::move(fresh.d_dzh16);
    st.d_w16 = std::move(fresh.d_w16);
    st.d_w16t = std::move(fresh.d_w16t);
    st.d_ctl = std::move(fresh.d_ctl);
  }
  if (p->mode == PT_NIF_TRAIN_F32 && train_mixed(st)) train_free_mixed(st);
  st.prec = *p;
  st.step = applied;
  if (train_mixed(st)) {
    train_refresh_half(h, st);
    train_ctl(h, st, ptd::kTrainCtlInit, st.p.batch, st.prec.loss_scale, applied);
    PT_HIP(hipGetLastError());
    PT_HIP(hipStreamSynchronize(h->stream));
  }
  return PT_OK;
}

int pt_nif_train_get_precision_state(pt_handle h, pt_nif_train_precision_state* s) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_get_precision_state")) return rc;
  if (!s || s->struct_size != sizeof(pt_nif_train_precision_state))
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_get_precision_state: pt_nif_train_precision_state.struct_size mismatch");
  NifTrainState& st = *h->train;
  s->mode = st.prec.mode;
  s->loss_scale = 1.0f; s->good_steps = 0; s->applied_steps = st.step; s->skipped_steps = 0;
  if (!train_mixed(st)) return PT_OK;
  PT_HIP(hipSetDevice(h->cfg.device));
  ptd::TrainCtl now{};
  if (int rc = train_read_ctl(h, st, &now)) return rc;
  s->loss_scale = now.S; s->good_steps = now.good; s->applied_steps = now.applied; s->skipped_steps = now.skipped;
  return PT_OK;
}

int pt_nif_train_end(pt_handle h) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!h->train) return PT_OK;
  PT_HIP(hipSetDevice(h->cfg.device));
  PT_HIP(hipStreamSynchronize(h->stream));
  h->train.reset();
  return PT_OK;
}

int pt_nif_train_batch(pt_handle h, uint64_t step, float* u, float* v, float* target) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_batch")) return rc;
  if (!u || !v || !target) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_batch: null buffer");
  NifTrainState& st = *h->train;
  PT_HIP(hipSetDevice(h->cfg.device));
  auto run = [&]() -> int {
    train_draw_batch(h, st, step);
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(u, st.d_u, (size_t)st.p.batch * 4, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipMemcpyAsync(v, st.d_vv, (size_t)st.p.batch * 4, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipMemcpyAsync(target, st.d_t, (size_t)st.p.batch * 12, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipStreamSynchronize(h->stream));
    return PT_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

int pt_nif_train_gradients(pt_handle h, const float* u, const float* v, const float* target, uint32_t n, float* loss, pt_layer* gradients,
                           uint32_t n_layers) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (int rc = train_need(h, "pt_nif_train_gradients")) return rc;
  NifTrainState& st = *h->train;
  if (!u || !v || !target || !loss) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_gradients: null buffer");
  if (n < 1 || n > st.p.batch) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_train_gradients: n must be 1.." + std::to_string(st.p.batch) + " (got " + std::to_string(n) + ")");
  const std::string bad = train_check_layers(st, gradients, n_layers, "pt_nif_train_gradients", true);
  if (!bad.empty()) return fail(h, PT_ERR_INVALID_ARGUMENT, bad);
  PT_HIP(hipSetDevice(h->cfg.device));
  auto run = [&]() -> int {
    PT_HIP(hipMemcpyAsync(st.d_u, u, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PT_HIP(hipMemcpyAsync(st.d_vv, v, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    PT_HIP(hipMemcpyAsync(st.d_t, target, (size_t)n * 12, hipMemcpyHostToDevice, h->stream));
    if (train_mixed(st)) {   // c for n samples, the pass, then the block as a step expects it: S and the counters stay
      train_ctl(h, st, ptd::kTrainCtlPrepare, n);
      train_encode16(h, st, n);
      if (int rc = train_forward_backward_mixed(h, st, n)) return rc;
      train_ctl(h, st, ptd::kTrainCtlPrepare, st.p.batch);
    } else {
      train_encode(h, st, n);
      if (int rc = train_forward_backward(h, st, n)) return rc;
    }
    PT_HIP(hipMemcpyAsync(loss, st.d_enc + 4, sizeof(float), hipMemcpyDeviceToHost, h->stream));
    return train_blob_out<float>(h, st, st.d_g, gradients, PT_DTYPE_F32);
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

}  // extern "C"
