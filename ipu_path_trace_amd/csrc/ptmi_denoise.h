// ptmi_denoise.h -- host side of pt_feature_buffers and pt_denoise (include/ptmi.h): the feature cache, the dense frames and the
// A-trous iterations.  Part of the one translation unit ptmi.hip, included last, after ptmi_film_comm.h.
#pragma once

namespace {

// Allocate `count` frames of width x height float4 into p[0 .. count) or none of them.
int alloc_frames(pt_handle h, DevBuf<float4>* p, int count, const char* what) {
  const size_t px = (size_t)h->cfg.width * h->cfg.height;
  for (int i = 0; i < count; ++i) {
    const hipError_t e = dev_alloc(p[i], px);
    if (e != hipSuccess) {
      for (int j = 0; j < i; ++j) p[j].reset();
      return fail(h, hip_status(e), std::string(what) + ": allocating " + std::to_string(px * sizeof(float4)) + " bytes: " + hipGetErrorString(e));
    }
  }
  return PT_OK;
}

// The feature cache holds the scene, camera and field of view in force: recomputed when their generation has moved.
int ensure_features(pt_handle h) {
  if (!h->settings_valid) return fail(h, PT_ERR_NOT_READY, "pt_set_render_settings has not been called (the field of view is a render setting)");
  PT_HIP(hipSetDevice(h->cfg.device));
  if (!h->d_feat[0]) {
    if (int rc = alloc_frames(h, h->d_feat, 2, "feature buffers")) return rc;
    h->feature_cached_gen = 0;
  }
  if (h->feature_cached_gen == h->feature_gen) return PT_OK;
  if (int rc = ensure_meshes(h)) return rc;
  ptd::TraceParams P;
  fill_trace_params(h, P);
  P.aa_scale = 0.f;      // the noise-free centre ray (pt_features.h)
  P.lens_a = 0.f;        // ... through a pinhole
  P.emitted = nullptr;
  const uint32_t px = h->cfg.width * h->cfg.height;
  const ptvariant::Variant var = variant_in_force(h, P);
  const int i = (int)var.geometry;   // the geometry level alone picks the instance
  note_variant(h->variant_features, var, i);   // (pt_get_trace_variant)
  if (i >= ptvariant::kFeatureTexFirst)   // pt_set_mesh_texture: albedo = colour x texel
    hipLaunchKernelGGL(ptd::features_kernel_tex, dim3((px + ptd::kFeatureBlock - 1) / ptd::kFeatureBlock), dim3(ptd::kFeatureBlock), 0,
                       h->stream, P, tex_params(h), h->d_feat[0], h->d_feat[1]);
  else
    hipLaunchKernelGGL(kFeatureKernels[i], dim3((px + ptd::kFeatureBlock - 1) / ptd::kFeatureBlock), dim3(ptd::kFeatureBlock), 0, h->stream, P,
                       h->d_feat[0], h->d_feat[1]);
  PT_HIP(hipGetLastError());
  h->feature_cached_gen = h->feature_gen;
  return PT_OK;
}

template <int STEP>
void launch_atrous(pt_handle h, const ptd::AtrousParams& A, const float4* in, float4* out) {
  const dim3 grid((A.width + ptd::kDenoiseTileW - 1) / ptd::kDenoiseTileW, (A.height + ptd::kDenoiseTileH - 1) / ptd::kDenoiseTileH);
  const dim3 block(ptd::kDenoiseTileW * ptd::kDenoiseTileH);
  if constexpr (STEP <= 2) {
    if ((uint32_t)STEP <= h->denoise_tiled_max_step) {
      hipLaunchKernelGGL((ptd::atrous_kernel<STEP, true>), grid, block, 0, h->stream, A, in, h->d_feat[0], out);
      return;
    }
  }
  hipLaunchKernelGGL((ptd::atrous_kernel<STEP, false>), grid, block, 0, h->stream, A, in, h->d_feat[0], out);
}

// Iteration i (step 2^i) of the filter from frame `in` to frame `out`.
void launch_atrous_iteration(pt_handle h, const pt_denoise_params& p, uint32_t i, const float4* in, float4* out) {
  ptd::AtrousParams A;
  A.width = h->cfg.width; A.height = h->cfg.height;
  const float sc = ldexpf(p.sigma_colour, -(int)i);     // sigma_colour 2^-i: exact
  A.inv_sc2 = p.sigma_colour > 0.f ? 1.0f / (sc * sc) : 0.f;
  A.inv_sn2 = p.sigma_normal > 0.f ? 1.0f / (p.sigma_normal * p.sigma_normal) : 0.f;
  A.sigma_d = p.sigma_depth > 0.f ? p.sigma_depth : 0.f;
  A.object_stop = p.object_stop ? 1 : 0;
  switch (i) {
    case 0: launch_atrous<1>(h, A, in, out); break;
    case 1: launch_atrous<2>(h, A, in, out); break;
    case 2: launch_atrous<4>(h, A, in, out); break;
    case 3: launch_atrous<8>(h, A, in, out); break;
    case 4: launch_atrous<16>(h, A, in, out); break;
    default: launch_atrous<32>(h, A, in, out); break;
  }
}

pt_denoise_params denoise_defaults() {
  pt_denoise_params p;
  p.struct_size = (uint32_t)sizeof(pt_denoise_params);
  p.iterations = 5;
  p.sigma_colour = 4.0f;
  p.sigma_normal = 0.5f;
  p.sigma_depth = 0.1f;
  p.object_stop = 1;
  p.demodulate = 1;
  return p;
}

// The checks of pt_denoise that need no device; empty = fine.
std::string denoise_check(const pt_denoise_params* p, int32_t source, const float* in, const float* out) {
  if (p) {
    if (p->struct_size != sizeof(pt_denoise_params)) return "pt_denoise: pt_denoise_params.struct_size mismatch";
    if (p->iterations < 1 || p->iterations > 6) return "pt_denoise: iterations must be 1..6 (got " + std::to_string(p->iterations) + ")";
    if (!std::isfinite(p->sigma_colour)) return "pt_denoise: sigma_colour must be finite";
    if (!std::isfinite(p->sigma_normal)) return "pt_denoise: sigma_normal must be finite";
    if (!std::isfinite(p->sigma_depth)) return "pt_denoise: sigma_depth must be finite";
  }
  if (source != PT_DENOISE_HOST_IMAGE && source != PT_DENOISE_ACCUMULATORS && source != PT_DENOISE_FILM)
    return "pt_denoise: source must be PT_DENOISE_HOST_IMAGE, PT_DENOISE_ACCUMULATORS or PT_DENOISE_FILM (got " + std::to_string(source) + ")";
  if (!out) return "pt_denoise: host_bgr_out is NULL";
  if (source == PT_DENOISE_HOST_IMAGE && !in) return "pt_denoise: host_bgr_in is NULL with PT_DENOISE_HOST_IMAGE";
  return std::string();
}

}  // namespace

extern "C" {

int pt_feature_buffers(pt_handle h, pt_features* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!out) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_feature_buffers: null pt_features");
  if (out->struct_size != sizeof(pt_features)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_feature_buffers: pt_features.struct_size mismatch");
  if (int rc = ensure_features(h)) return rc;
  const size_t px = (size_t)h->cfg.width * h->cfg.height;
  std::vector<float4> f0(px), f1(px);
  PT_HIP(hipMemcpyAsync(f0.data(), h->d_feat[0], px * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipMemcpyAsync(f1.data(), h->d_feat[1], px * sizeof(float4), hipMemcpyDeviceToHost, h->stream));
  PT_HIP(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < px; ++i) {
    if (out->object_id) out->object_id[i] = (int32_t)f2u(f1[i].w);
    if (out->depth) out->depth[i] = f0[i].w;
    if (out->normal) { out->normal[3 * i] = f0[i].x; out->normal[3 * i + 1] = f0[i].y; out->normal[3 * i + 2] = f0[i].z; }
    if (out->albedo) { out->albedo[3 * i] = f1[i].x; out->albedo[3 * i + 1] = f1[i].y; out->albedo[3 * i + 2] = f1[i].z; }
  }
  return PT_OK;
}

int pt_denoise_default_params(pt_denoise_params* p) {
  if (!p) return PT_ERR_INVALID_ARGUMENT;
  *p = denoise_defaults();
  return PT_OK;
}

int pt_denoise(pt_handle h, const pt_denoise_params* params, int32_t source, const float* host_bgr_in, float* host_bgr_out) {
  // the checks that need no device come first; without a handle the message goes where pt_last_error(NULL) reads it
  const std::string bad = denoise_check(params, source, host_bgr_in, host_bgr_out);
  if (!bad.empty()) {
    if (h) h->error = bad; else g_create_error = bad;
    return PT_ERR_INVALID_ARGUMENT;
  }
  if (!h) { g_create_error = "pt_denoise: null handle"; return PT_ERR_INVALID_ARGUMENT; }
  const pt_denoise_params p = params ? *params : denoise_defaults();
  if (source != PT_DENOISE_HOST_IMAGE && h->n_items == 0) return fail(h, PT_ERR_NOT_READY, "pt_denoise: no worklist (pt_setup has not been called)");
  if (source == PT_DENOISE_FILM && (!h->d_film || h->film_steps == 0))
    return fail(h, PT_ERR_NOT_READY, "pt_denoise: no resident film (pt_film_accumulate has not been called since pt_setup)");
  if (int rc = ensure_features(h)) return rc;
  if (!h->d_dn_colour[0]) {
    if (int rc = alloc_frames(h, h->d_dn_colour, 2, "denoiser frames")) return rc;
  }
  const size_t px = (size_t)h->cfg.width * h->cfg.height;
  if (int rc = ensure_scratch(h, px * 12)) return rc;
  float* d_img = scratch_as<float>(h);
  const uint32_t n = (uint32_t)px, blocks = (n + 255) / 256;
  // whatever fails below, no copy from or to the caller's buffers is left pending when the call returns
  auto run = [&]() -> int {
    if (source == PT_DENOISE_HOST_IMAGE) {
      PT_HIP(hipMemcpyAsync(d_img, host_bgr_in, px * 12, hipMemcpyHostToDevice, h->stream));
    } else {
      PT_HIP(hipMemsetAsync(d_img, 0, px * 12, h->stream));
      const bool film = source == PT_DENOISE_FILM;
      hipLaunchKernelGGL(ptd::denoise_scatter_kernel, dim3((h->n_items + 255) / 256), dim3(256), 0, h->stream, h->n_items, h->acc.pix, h->acc.r,
                         h->acc.g, h->acc.b, h->acc.count, film ? h->d_film : nullptr, film ? 1.0f / (float)h->film_steps : 0.f,
                         h->cfg.width, h->cfg.height, d_img);
      PT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ptd::denoise_pack_kernel, dim3(blocks), dim3(256), 0, h->stream, n, d_img, h->d_feat[1], p.demodulate ? 1 : 0,
                       h->d_dn_colour[0]);
    PT_HIP(hipGetLastError());
    int cur = 0;
    for (uint32_t i = 0; i < p.iterations; ++i, cur ^= 1) {
      launch_atrous_iteration(h, p, i, h->d_dn_colour[cur], h->d_dn_colour[cur ^ 1]);
      PT_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ptd::denoise_unpack_kernel, dim3(blocks), dim3(256), 0, h->stream, n, h->d_dn_colour[cur], h->d_feat[1],
                       p.demodulate ? 1 : 0, d_img);
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(host_bgr_out, d_img, px * 12, hipMemcpyDeviceToHost, h->stream));
    PT_HIP(hipStreamSynchronize(h->stream));
    return PT_OK;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  return rc;
}

#ifdef PTMI_DIAG_BUILD
// profiling build only (scripts/denoise_bench.py): iteration `iteration` of the default filter, `launches` times back to back
// between two HIP events on the frames the last pt_denoise left, with the taps staged in LDS (tiled != 0, steps 1 and 2 only)
// or read from global memory.  Returns the average device milliseconds per launch.
int pt_diag_denoise_bench(pt_handle h, int32_t tiled, uint32_t iteration, uint32_t launches, double* ms_per_launch) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!ms_per_launch || launches == 0 || iteration > 5 || (tiled && iteration > 1)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_denoise_bench: bad argument");
  if (!h->d_dn_colour[0] || !h->d_feat[0]) return fail(h, PT_ERR_NOT_READY, "pt_diag_denoise_bench: pt_denoise has not run");
  PT_HIP(hipSetDevice(h->cfg.device));
  const uint32_t keep = h->denoise_tiled_max_step;
  h->denoise_tiled_max_step = tiled ? 2u : 0u;
  const pt_denoise_params p = denoise_defaults();
  hipEvent_t a = nullptr, b = nullptr;
  PT_HIP(hipEventCreate(&a));
  PT_HIP(hipEventCreate(&b));
  launch_atrous_iteration(h, p, iteration, h->d_dn_colour[0], h->d_dn_colour[1]);   // untimed
  (void)hipEventRecord(a, h->stream);
  for (uint32_t k = 0; k < launches; ++k) launch_atrous_iteration(h, p, iteration, h->d_dn_colour[k & 1], h->d_dn_colour[(k & 1) ^ 1]);
  (void)hipEventRecord(b, h->stream);
  const hipError_t e = hipStreamSynchronize(h->stream);
  h->denoise_tiled_max_step = keep;
  float ms = 0.f;
  if (e == hipSuccess) (void)hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  PT_HIP(e);
  PT_HIP(hipGetLastError());
  *ms_per_launch = (double)ms / launches;
  return PT_OK;
}
#endif

}  // extern "C"
