// ptmi_env_guide.h -- validation of an environment guide and the construction of its tables (pt_set_env_guide, include/ptmi.h).
// Plain C++ on purpose, like ptmi_scene.h and ptmi_camera.h: the library (ptmi.hip), the CLI (host/PathTracerApp.cpp,
// --env-guide) and a stand-alone test program (tests/env_guide_main.cpp) all include it, so a bad image or grid is refused
// before any device is attached with the very message the library would give.
//
// The guide is a piecewise-constant density over the unit square of (u, v) -- u down the image, v across it -- on a grid of
// rows x cols cells.  A cell's mass is the binary64 sum of luminance x sin(theta) over its texels; one alias table (Vose) over
// all n = rows x cols cells draws a cell from two 32-bit words.  The density table q is computed from the QUANTISED alias
// table, not from the ideal masses: the density the kernel divides by is exactly the distribution it draws from.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "ptmi.h"

namespace ptguide {

constexpr uint32_t kMaxRows = PT_ENV_GUIDE_MAX_ROWS, kMaxCols = PT_ENV_GUIDE_MAX_COLS;
constexpr double kTwo32 = 4294967296.0;
constexpr double kPi = 3.14159265358979323846;

struct Table {
  uint32_t rows = 0, cols = 0, log2n = 0, log2cols = 0;
  uint32_t alpha_thr = 0;            // (uint32)(alpha 2^32): a word below it takes the guide branch
  double alpha = 0;                  // alpha_thr / 2^32, the alpha used everywhere afterwards
  std::vector<uint32_t> threshold;   // [n]: cell k is kept when a 32-bit word is < threshold[k] ...
  std::vector<uint32_t> alias;       // [n]: ... and replaced by alias[k] otherwise
  std::vector<float> q;              // [n]: P(cell) n / pi, P from the quantised table
  std::vector<double> ideal;         // [n]: the normalised binary64 masses (what the table approximates)
  std::vector<double> P;             // [n]: the probability the table really draws each cell with
};

// What a guide built from the environment answers when there is none (PT_ERR_NOT_READY; the CLI refuses with the same words).
constexpr const char* kNoEnvironment =
    "no environment has been set (none of pt_upload_nif, pt_set_env_map, pt_set_constant_env has been called)";

inline bool pow2(uint32_t x) { return x != 0 && (x & (x - 1)) == 0; }
inline uint32_t log2u(uint32_t x) { uint32_t l = 0; while ((1u << l) < x) ++l; return l; }
inline std::string num(double v) { char b[40]; snprintf(b, sizeof(b), "%g", v); return b; }

// The default grid: the largest powers of two not above the image size or the caps.
inline void default_grid(uint32_t width, uint32_t height, uint32_t& rows, uint32_t& cols) {
  rows = 1; cols = 1;
  while (rows * 2 <= height && rows * 2 <= kMaxRows) rows *= 2;
  while (cols * 2 <= width && cols * 2 <= kMaxCols) cols *= 2;
}

// "" if the guide's fields are valid, else what is wrong, naming the field.  The texels are checked too (as pt_set_env_map).
inline std::string check(const pt_env_guide* g) {
  if (!g) return "env guide: null guide";
  if (g->struct_size != sizeof(pt_env_guide))
    return "env guide: struct_size must be " + std::to_string(sizeof(pt_env_guide)) + " (got " + std::to_string(g->struct_size) + ")";
  if (!g->bgr) return "env guide: bgr is null";
  if (g->width == 0 || g->width > PT_ENV_MAP_MAX_SIZE)
    return "env guide: width must be in 1.." + std::to_string(PT_ENV_MAP_MAX_SIZE) + " (got " + std::to_string(g->width) + ")";
  if (g->height == 0 || g->height > PT_ENV_MAP_MAX_SIZE)
    return "env guide: height must be in 1.." + std::to_string(PT_ENV_MAP_MAX_SIZE) + " (got " + std::to_string(g->height) + ")";
  if (!pow2(g->rows) || g->rows > kMaxRows)
    return "env guide: rows must be a power of two in 1.." + std::to_string(kMaxRows) + " (got " + std::to_string(g->rows) + ")";
  if (!pow2(g->cols) || g->cols > kMaxCols)
    return "env guide: cols must be a power of two in 1.." + std::to_string(kMaxCols) + " (got " + std::to_string(g->cols) + ")";
  if (g->rows > g->height)
    return "env guide: rows must not exceed height (" + std::to_string(g->rows) + " > " + std::to_string(g->height) + ")";
  if (g->cols > g->width)
    return "env guide: cols must not exceed width (" + std::to_string(g->cols) + " > " + std::to_string(g->width) + ")";
  if (!(g->alpha >= 0.f && g->alpha <= PT_ENV_GUIDE_MAX_ALPHA))
    return "env guide: alpha must be in [0, " + num(PT_ENV_GUIDE_MAX_ALPHA) + "] (got " + num(g->alpha) + ")";
  const size_t texels = (size_t)g->width * g->height;
  for (size_t i = 0; i < 3 * texels; ++i)
    if (!(g->bgr[i] >= 0.f) || !std::isfinite(g->bgr[i])) {
      static const char* const kChannel[3] = {"B", "G", "R"};
      return "env guide: bgr texel at row " + std::to_string(i / 3 / g->width) + ", column " + std::to_string(i / 3 % g->width) +
             ", channel " + std::to_string(i % 3) + " (" + kChannel[i % 3] + ") is " + num(g->bgr[i]) +
             ": texels must be finite and not negative";
    }
  return "";
}

// Vose's alias method in binary64 over the masses m[0..n) (total > 0, finite), quantised to 32-bit thresholds.  A cell of zero
// mass ends with threshold 0 and no alias pointing at it; a column that keeps its cell with probability 1 names itself as its
// alias, so the 2^-32 its threshold cannot express comes back to it and the table's probabilities sum to 1 exactly.
inline void alias_table(const std::vector<double>& m, double total, std::vector<uint32_t>& threshold, std::vector<uint32_t>& alias) {
  const size_t n = m.size();
  threshold.assign(n, 0u);
  alias.assign(n, 0u);
  std::vector<double> p(n);
  std::vector<uint32_t> small, large;
  size_t heaviest = 0;
  for (size_t k = 0; k < n; ++k) {
    p[k] = m[k] / total * (double)n;
    if (m[k] > m[heaviest]) heaviest = k;
  }
  // the empty cells are taken first (they lie on top of the stack): each finds a donor while donors are certain to exist
  for (size_t k = 0; k < n; ++k) if (p[k] < 1.0 && m[k] > 0.0) small.push_back((uint32_t)k);
  for (size_t k = 0; k < n; ++k) if (m[k] == 0.0) small.push_back((uint32_t)k);
  for (size_t k = 0; k < n; ++k) if (p[k] >= 1.0) large.push_back((uint32_t)k);
  auto quantise = [](double x) { return x >= 1.0 ? 0xffffffffu : (uint32_t)std::floor(x * kTwo32); };
  while (!small.empty() && !large.empty()) {
    const uint32_t s = small.back(), l = large.back();
    small.pop_back();
    threshold[s] = quantise(p[s]);
    alias[s] = l;
    p[l] = (p[l] + p[s]) - 1.0;
    if (p[l] < 1.0) { large.pop_back(); small.push_back(l); }
  }
  // what is left is 1 up to rounding: the column keeps its own cell (an empty cell cannot be left, but must never gain mass)
  for (uint32_t k : large) { threshold[k] = 0xffffffffu; alias[k] = k; }
  for (uint32_t k : small) {
    if (m[k] > 0.0) { threshold[k] = 0xffffffffu; alias[k] = k; }
    else { threshold[k] = 0u; alias[k] = (uint32_t)heaviest; }
  }
}

// The tables from the cell masses (cell order, binary64): the total, the alias table, P and q.  Both routes to a guide end here --
// build() below over an image in host memory, and pt_set_env_guide_from_environment over the masses its kernels summed on the
// device (csrc/pt_env_guide_build.h) -- so one set of masses gives one set of tables.  "" on success, else the reason (no mass).
inline std::string build_from_masses(uint32_t rows, uint32_t cols, float alpha, const std::vector<double>& mass, Table& T,
                                     const char* what = "bgr") {
  const size_t n = (size_t)rows * cols;
  T.rows = rows; T.cols = cols;
  T.log2cols = log2u(cols);
  T.log2n = log2u(rows) + T.log2cols;
  T.alpha_thr = (uint32_t)((double)alpha * kTwo32);
  T.alpha = (double)T.alpha_thr / kTwo32;
  double total = 0.0;
  for (double m : mass) total += m;
  if (!(total > 0.0) || !std::isfinite(total))
    return std::string("env guide: ") + what + " has a total mass (luminance x sin theta) of " + num(total) + ": the image must not be black";
  alias_table(mass, total, T.threshold, T.alias);
  std::vector<uint64_t> acc(n, 0);   // P(cell) n 2^32, an integer: at most n 2^32 <= 2^53
  for (size_t k = 0; k < n; ++k) {
    acc[k] += T.threshold[k];
    acc[T.alias[k]] += (1ull << 32) - T.threshold[k];
  }
  T.q.resize(n); T.P.resize(n); T.ideal.resize(n);
  for (size_t k = 0; k < n; ++k) {
    T.P[k] = (double)acc[k] / ((double)n * kTwo32);
    T.q[k] = (float)((double)acc[k] / kTwo32 / kPi);
    T.ideal[k] = mass[k] / total;
  }
  return "";
}

// sin(pi (r + 0.5) / height) for every image row, as build() weighs them: the device build takes this table from the host.
inline std::vector<double> row_sines(uint32_t height) {
  std::vector<double> sn(height);
  for (uint32_t r = 0; r < height; ++r) sn[r] = std::sin(kPi * ((double)r + 0.5) / (double)height);
  return sn;
}

// The tables of a guide check() accepted.  "" on success, else the reason (an image without mass), naming the field.
inline std::string build(const pt_env_guide& g, Table& T) {
  const uint32_t rows = g.rows, cols = g.cols, W = g.width, H = g.height;
  const size_t n = (size_t)rows * cols;
  std::vector<double> mass(n, 0.0);
  for (uint32_t r = 0; r < H; ++r) {
    const size_t i = (size_t)((uint64_t)r * rows / H);
    const double sn = std::sin(kPi * ((double)r + 0.5) / (double)H);
    for (uint32_t c = 0; c < W; ++c) {
      const size_t j = (size_t)((uint64_t)c * cols / W);
      const float* t = g.bgr + 3 * ((size_t)r * W + c);
      mass[i * cols + j] += (0.0722 * (double)t[0] + 0.7152 * (double)t[1] + 0.2126 * (double)t[2]) * sn;
    }
  }
  return build_from_masses(rows, cols, g.alpha, mass, T);
}

// "" if the fields of a guide built from the environment in force are valid, else what is wrong, naming the field; checked in
// the order of the struct (pt_set_env_guide_from_environment, include/ptmi.h).
inline std::string check_auto(const pt_env_guide_auto* a) {
  if (!a) return "env guide: null pt_env_guide_auto";
  if (a->struct_size != sizeof(pt_env_guide_auto))
    return "env guide: struct_size must be " + std::to_string(sizeof(pt_env_guide_auto)) + " (got " + std::to_string(a->struct_size) + ")";
  if (!pow2(a->rows) || a->rows > kMaxRows)
    return "env guide: rows must be a power of two in 1.." + std::to_string(kMaxRows) + " (got " + std::to_string(a->rows) + ")";
  if (!pow2(a->cols) || a->cols > kMaxCols)
    return "env guide: cols must be a power of two in 1.." + std::to_string(kMaxCols) + " (got " + std::to_string(a->cols) + ")";
  if (a->supersample != 1 && a->supersample != 2 && a->supersample != 4)
    return "env guide: supersample must be 1, 2 or 4 (got " + std::to_string(a->supersample) + ")";
  if (!(a->alpha >= 0.f && a->alpha <= PT_ENV_GUIDE_MAX_ALPHA))
    return "env guide: alpha must be in [0, " + num(PT_ENV_GUIDE_MAX_ALPHA) + "] (got " + num(a->alpha) + ")";
  if (a->follow != 0 && a->follow != 1)
    return "env guide: follow must be 0 or 1 (got " + std::to_string(a->follow) + ")";
  return "";
}

}  // namespace ptguide
