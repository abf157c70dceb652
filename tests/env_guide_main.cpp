// env_guide_main.cpp -- stand-alone checks of csrc/ptmi_env_guide.h (validation and table construction of pt_set_env_guide).
// Built with -fsanitize=address,undefined and run by tests/test_env_guide_model.py; it also prints a table on request so that the
// numpy model can be compared with the library's own construction entry for entry.
//
//   env_guide_main check                      the seeded images and every rejection; prints "ok <cases>" and exits 0
//   env_guide_main dump W H ROWS COLS SEED    prints threshold, alias, q bits of a seeded image, one cell per line
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ptmi_env_guide.h"

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                                      \
  do {                                                                        \
    if (!(cond)) {                                                            \
      ++g_failures;                                                           \
      std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);          \
      std::printf(__VA_ARGS__);                                               \
      std::printf("\n");                                                      \
    }                                                                         \
  } while (0)

// splitmix64: the seeded images (tests/test_env_guide_model.py makes the same ones)
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
};

// kind 0: seeded noise with a wide range; 1: all texels equal; 2: one hot texel on black; 3: noise with a black band
std::vector<float> image(uint32_t w, uint32_t h, uint64_t seed, int kind) {
  Rng rng{seed};
  std::vector<float> img((size_t)w * h * 3);
  for (size_t t = 0; t < (size_t)w * h; ++t)
    for (int c = 0; c < 3; ++c) {
      const float x = rng.unit();
      float v = x * x * x * 50.f;
      if (kind == 1) v = 0.75f;
      if (kind == 2) v = 0.f;
      if (kind == 3 && (t / w) % 2 == 0) v = 0.f;
      img[3 * t + c] = v;
    }
  if (kind == 2) { const size_t t = ((size_t)(h / 2) * w + w / 3); img[3 * t] = img[3 * t + 1] = img[3 * t + 2] = 1000.f; }
  return img;
}

pt_env_guide request(const std::vector<float>& img, uint32_t w, uint32_t h, uint32_t rows, uint32_t cols, float alpha) {
  pt_env_guide g{};
  g.struct_size = sizeof(pt_env_guide);
  g.width = w; g.height = h; g.rows = rows; g.cols = cols; g.alpha = alpha;
  g.bgr = img.data();
  return g;
}

void check_table(const char* name, uint32_t w, uint32_t h, uint32_t rows, uint32_t cols, int kind, uint64_t seed) {
  const std::vector<float> img = image(w, h, seed, kind);
  const pt_env_guide g = request(img, w, h, rows, cols, 0.5f);
  const std::string bad = ptguide::check(&g);
  CHECK(bad.empty(), "%s: %s", name, bad.c_str());
  if (!bad.empty()) return;
  ptguide::Table T;
  const std::string why = ptguide::build(g, T);
  CHECK(why.empty(), "%s: %s", name, why.c_str());
  if (!why.empty()) return;
  const size_t n = (size_t)rows * cols;
  CHECK(T.threshold.size() == n && T.alias.size() == n && T.q.size() == n, "%s: table sizes", name);
  CHECK((1u << T.log2n) == n && (1u << T.log2cols) == cols, "%s: log2", name);
  // every alias in range (every uint32 is a valid threshold); P recomputed here from the table alone
  std::vector<long double> P(n, 0.0L);
  for (size_t k = 0; k < n; ++k) {
    CHECK(T.alias[k] < n, "%s: alias[%zu] = %u out of range", name, k, T.alias[k]);
    if (T.alias[k] >= n) return;
    P[k] += (long double)T.threshold[k];
    P[T.alias[k]] += 4294967296.0L - (long double)T.threshold[k];
  }
  // the ideal masses, summed independently of build()
  std::vector<double> mass(n, 0.0);
  double total = 0.0;
  for (uint32_t r = 0; r < h; ++r)
    for (uint32_t c = 0; c < w; ++c) {
      const float* t = &img[3 * ((size_t)r * w + c)];
      const size_t cell = (size_t)((uint64_t)r * rows / h) * cols + (size_t)((uint64_t)c * cols / w);
      mass[cell] += (0.0722 * t[0] + 0.7152 * t[1] + 0.2126 * t[2]) * std::sin(ptguide::kPi * (r + 0.5) / h);
    }
  for (double m : mass) total += m;
  long double sum = 0.0L;
  const double tol = std::ldexp((double)n, -32);
  for (size_t k = 0; k < n; ++k) {
    const double p = (double)(P[k] / (4294967296.0L * (long double)n));
    sum += P[k] / (4294967296.0L * (long double)n);
    CHECK(std::fabs(p - T.P[k]) <= 1e-15, "%s: P[%zu] %.17g, build() says %.17g", name, k, p, T.P[k]);
    CHECK(std::fabs(p - mass[k] / total) <= tol, "%s: P[%zu] = %.12g, ideal %.12g, tolerance %.3g", name, k, p, mass[k] / total, tol);
    if (mass[k] == 0.0) CHECK(P[k] == 0.0L, "%s: empty cell %zu has P = %.12g", name, k, p);
    CHECK(T.q[k] == (float)(p * (double)n / ptguide::kPi), "%s: q[%zu]", name, k);
  }
  CHECK(std::fabs((double)(sum - 1.0L)) <= 1e-12, "%s: P sums to 1 %+.3g", name, (double)(sum - 1.0L));
  CHECK(T.alpha_thr == 0x80000000u && T.alpha == 0.5, "%s: alpha", name);
}

void expect_rejected(const char* what, const pt_env_guide& g, const char* field) {
  std::string msg = ptguide::check(&g);
  if (msg.empty()) { ptguide::Table T; msg = ptguide::build(g, T); }
  CHECK(!msg.empty(), "%s was accepted", what);
  CHECK(msg.find(field) != std::string::npos, "%s: the message does not name '%s': %s", what, field, msg.c_str());
}

int run_checks() {
  int cases = 0;
  const struct { const char* name; uint32_t w, h, rows, cols; } shapes[] = {
      {"3x5 on 2x4", 5, 3, 2, 4}, {"64x32 on 32x64", 64, 32, 32, 64}, {"one row", 16, 8, 1, 16}, {"one column", 16, 8, 8, 1},
      {"one cell", 7, 5, 1, 1}, {"ragged", 37, 19, 16, 32}};
  for (const auto& s : shapes)
    for (int kind = 0; kind < 4; ++kind)
      for (uint64_t seed = 1; seed <= 3; ++seed) {
        if (kind == 3 && s.h < 2) continue;
        check_table(s.name, s.w, s.h, s.rows, s.cols, kind, seed * 7919 + (uint64_t)kind);
        ++cases;
      }
  // rejections: each names its field
  const std::vector<float> img = image(8, 4, 11, 0);
  expect_rejected("null guide", pt_env_guide{}, "struct_size");
  CHECK(!ptguide::check(nullptr).empty(), "null pointer accepted");
  { pt_env_guide g = request(img, 8, 4, 4, 8, 0.5f); g.struct_size = 12; expect_rejected("struct_size", g, "struct_size"); }
  { pt_env_guide g = request(img, 8, 4, 4, 8, 0.5f); g.bgr = nullptr; expect_rejected("null image", g, "bgr"); }
  expect_rejected("width 0", request(img, 0, 4, 4, 8, 0.5f), "width");
  expect_rejected("height too large", request(img, 8, PT_ENV_MAP_MAX_SIZE + 1, 4, 8, 0.5f), "height");
  expect_rejected("rows not a power of two", request(img, 8, 4, 3, 8, 0.5f), "rows");
  expect_rejected("rows zero", request(img, 8, 4, 0, 8, 0.5f), "rows");
  expect_rejected("cols not a power of two", request(img, 8, 4, 4, 6, 0.5f), "cols");
  expect_rejected("rows above the image", request(img, 8, 4, 8, 8, 0.5f), "rows");
  expect_rejected("cols above the image", request(img, 8, 4, 4, 16, 0.5f), "cols");
  expect_rejected("alpha negative", request(img, 8, 4, 4, 8, -0.1f), "alpha");
  expect_rejected("alpha above the cap", request(img, 8, 4, 4, 8, 0.95f), "alpha");
  expect_rejected("alpha NaN", request(img, 8, 4, 4, 8, std::numeric_limits<float>::quiet_NaN()), "alpha");
  { std::vector<float> bad = img; bad[3 * (2 * 8 + 5) + 1] = -1.f; expect_rejected("negative texel", request(bad, 8, 4, 4, 8, 0.5f), "row 2, column 5, channel 1"); }
  { std::vector<float> bad = img; bad[7] = std::numeric_limits<float>::quiet_NaN(); expect_rejected("NaN texel", request(bad, 8, 4, 4, 8, 0.5f), "bgr"); }
  { std::vector<float> bad = img; bad[0] = std::numeric_limits<float>::infinity(); expect_rejected("infinite texel", request(bad, 8, 4, 4, 8, 0.5f), "bgr"); }
  { std::vector<float> black(img.size(), 0.f); expect_rejected("black image", request(black, 8, 4, 4, 8, 0.5f), "bgr"); }
  { std::vector<float> big(3u * 2048 * 4, 1.f); expect_rejected("rows above the cap", request(big, 4, 2048, 2048, 4, 0.5f), "rows"); }
  { std::vector<float> big(3u * 4096 * 2, 1.f); expect_rejected("cols above the cap", request(big, 4096, 2, 2, 4096, 0.5f), "cols"); }
  // the caps themselves and alpha's ends are accepted; alpha as used
  { std::vector<float> big(3u * 2048 * 2, 1.f); const pt_env_guide g = request(big, 2048, 2, 2, 2048, 0.9f); CHECK(ptguide::check(&g).empty(), "cols = 2048 refused"); }
  {
    ptguide::Table T;
    const pt_env_guide g0 = request(img, 8, 4, 4, 8, 0.f), g9 = request(img, 8, 4, 4, 8, 0.9f);
    CHECK(ptguide::check(&g0).empty() && ptguide::build(g0, T).empty() && T.alpha_thr == 0 && T.alpha == 0.0, "alpha 0");
    CHECK(ptguide::check(&g9).empty() && ptguide::build(g9, T).empty() && T.alpha_thr == (uint32_t)((double)0.9f * 4294967296.0), "alpha 0.9");
  }
  // the default grid: the largest powers of two not above the image or the caps
  uint32_t r = 0, c = 0;
  ptguide::default_grid(64, 32, r, c); CHECK(r == 32 && c == 64, "default grid 64 x 32: %u x %u", r, c);
  ptguide::default_grid(5, 3, r, c); CHECK(r == 2 && c == 4, "default grid 5 x 3: %u x %u", r, c);
  ptguide::default_grid(16384, 8192, r, c); CHECK(r == 1024 && c == 2048, "default grid 16384 x 8192: %u x %u", r, c);
  ptguide::default_grid(1, 1, r, c); CHECK(r == 1 && c == 1, "default grid 1 x 1: %u x %u", r, c);
  if (g_failures) { std::printf("%d check(s) failed\n", g_failures); return 1; }
  std::printf("ok %d\n", cases);
  return 0;
}

int dump(uint32_t w, uint32_t h, uint32_t rows, uint32_t cols, uint64_t seed) {
  const std::vector<float> img = image(w, h, seed, 0);
  const pt_env_guide g = request(img, w, h, rows, cols, 0.5f);
  const std::string bad = ptguide::check(&g);
  ptguide::Table T;
  const std::string why = bad.empty() ? ptguide::build(g, T) : bad;
  if (!why.empty()) { std::printf("%s\n", why.c_str()); return 1; }
  for (float v : img) { uint32_t b; std::memcpy(&b, &v, 4); std::printf("t %u\n", b); }
  for (size_t k = 0; k < T.q.size(); ++k) {
    uint32_t b; std::memcpy(&b, &T.q[k], 4);
    std::printf("c %u %u %u\n", T.threshold[k], T.alias[k], b);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "check")) return run_checks();
  if (argc == 7 && !std::strcmp(argv[1], "dump"))
    return dump((uint32_t)std::atoi(argv[2]), (uint32_t)std::atoi(argv[3]), (uint32_t)std::atoi(argv[4]), (uint32_t)std::atoi(argv[5]),
                (uint64_t)std::atoll(argv[6]));
  std::printf("usage: env_guide_main check | dump W H ROWS COLS SEED\n");
  return 2;
}
