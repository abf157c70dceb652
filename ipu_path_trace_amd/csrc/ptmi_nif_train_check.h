// ptmi_nif_train_check.h -- defaults, validation and layer shapes of the NIF trainer (pt_nif_train_*, include/ptmi.h).
// Plain C++ on purpose, like ptmi_scene.h: the library (ptmi.hip), the CLI (host/PathTracerApp.cpp, --train-nif) and the
// sanitizer program of the tests include it, so bad arguments are refused before any device is attached with the very
// message the library would give.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "ptmi.h"

namespace ptniftrain {

constexpr uint32_t kMaxBatch = 1u << 20;

// The reference's train_command (nif_metadata.txt: embedding 12, 6 x 320, log tone map, eps 1e-8) and Keras's Adam.
inline pt_nif_train_params defaults() {
  pt_nif_train_params p{};
  p.struct_size = (uint32_t)sizeof(pt_nif_train_params);
  p.embedding_dim = 12;
  p.hidden = 320;
  p.layer_count = 6;
  p.batch = 65536;
  p.learning_rate = 1e-3f;
  p.beta1 = 0.9f;
  p.beta2 = 0.999f;
  p.adam_eps = 1e-7f;
  p.seed = 1;
  p.log_tone_map = 1;
  p.eps = 1e-8f;
  return p;
}

// "" if the parameters are valid, else what is wrong, naming the field.
inline std::string check(const pt_nif_train_params* p) {
  const std::string at = "pt_nif_train_begin: ";
  if (!p) return at + "null pt_nif_train_params";
  if (p->struct_size != sizeof(pt_nif_train_params)) return at + "pt_nif_train_params.struct_size mismatch";
  // 16 is refused: at u = 0 or v = 0 the argument of frequency 2^15 is half(-2 x 2^15) = -inf, its sine NaN, and one such texel
  // in a batch puts NaN into every weight (inference accepts 16; its oracle gives the same NaN there)
  if (p->embedding_dim < 1 || p->embedding_dim > 15) return at + "embedding_dim must be 1..15 (got " + std::to_string(p->embedding_dim) + ")";
  if (p->hidden < 32 || p->hidden > 1024 || p->hidden % 32 != 0)
    return at + "hidden must be a multiple of 32 in 32..1024 (got " + std::to_string(p->hidden) + ")";
  if (p->layer_count < 1 || p->layer_count > 15) return at + "layer_count must be 1..15 (got " + std::to_string(p->layer_count) + ")";
  if (p->batch < 256 || p->batch > kMaxBatch || p->batch % 256 != 0)
    return at + "batch must be a multiple of 256 in 256.." + std::to_string(kMaxBatch) + " (got " + std::to_string(p->batch) + ")";
  if (!std::isfinite(p->learning_rate) || !(p->learning_rate > 0.f)) return at + "learning_rate must be finite and > 0";
  if (!std::isfinite(p->beta1) || !(p->beta1 >= 0.f) || !(p->beta1 < 1.f)) return at + "beta1 must be in [0, 1)";
  if (!std::isfinite(p->beta2) || !(p->beta2 >= 0.f) || !(p->beta2 < 1.f)) return at + "beta2 must be in [0, 1)";
  if (!std::isfinite(p->adam_eps) || !(p->adam_eps > 0.f)) return at + "adam_eps must be finite and > 0";
  if (p->log_tone_map != 0 && p->log_tone_map != 1) return at + "log_tone_map must be 0 or 1 (got " + std::to_string(p->log_tone_map) + ")";
  if (!std::isfinite(p->eps) || !(p->eps >= 0.f)) return at + "eps must be finite and >= 0";
  if (p->log_tone_map && !(p->eps > 0.f)) return at + "eps must be > 0 with log_tone_map (a black texel has no logarithm)";
  return "";
}

// pt_nif_train_set_precision: the defaults and the check, in field order.
inline pt_nif_train_precision default_precision() {
  pt_nif_train_precision p{};
  p.struct_size = (uint32_t)sizeof(pt_nif_train_precision);
  p.mode = PT_NIF_TRAIN_F32;
  p.loss_scale = 65536.0f;
  p.dynamic = 1;
  p.growth_interval = 2000;
  return p;
}

inline std::string check_precision(const pt_nif_train_precision* p) {
  const std::string at = "pt_nif_train_set_precision: ";
  if (!p) return at + "null pt_nif_train_precision";
  if (p->struct_size != sizeof(pt_nif_train_precision)) return at + "pt_nif_train_precision.struct_size mismatch";
  if (p->mode != PT_NIF_TRAIN_F32 && p->mode != PT_NIF_TRAIN_MIXED_F16)
    return at + "mode must be PT_NIF_TRAIN_F32 (0) or PT_NIF_TRAIN_MIXED_F16 (1) (got " + std::to_string(p->mode) + ")";
  int exponent = 0;
  const bool power_of_two = std::isfinite(p->loss_scale) && p->loss_scale > 0.f && std::frexp(p->loss_scale, &exponent) == 0.5f;
  if (!power_of_two || p->loss_scale < 1.0f || p->loss_scale > 1073741824.0f) return at + "loss_scale must be a power of two in 1 .. 2^30";
  if (p->dynamic != 0 && p->dynamic != 1) return at + "dynamic must be 0 or 1 (got " + std::to_string(p->dynamic) + ")";
  if (p->growth_interval < 1u || p->growth_interval > 2147483648u)
    return at + "growth_interval must be 1 .. 2^31 (got " + std::to_string(p->growth_interval) + ")";
  return "";
}

// The stack synthetic_nif builds: layer_count ReLU layers of width hidden, the 4 E Fourier features concatenated to the input
// of layer layer_count / 2 (when that is not layer 0), and a linear head of 3 outputs.
struct Shape { uint32_t rows, cols; bool relu; };
inline std::vector<Shape> shapes(const pt_nif_train_params& p) {
  const uint32_t in = 4 * p.embedding_dim, skip = p.layer_count / 2;
  std::vector<Shape> s;
  for (uint32_t l = 0; l < p.layer_count; ++l) s.push_back({l == 0 ? in : p.hidden + (l == skip ? in : 0u), p.hidden, true});
  s.push_back({p.hidden, 3u, false});
  return s;
}

}  // namespace ptniftrain
