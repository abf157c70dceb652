// env_guide_masses_main.cpp -- stand-alone checks of the split of csrc/ptmi_env_guide.h into the mass loop and
// build_from_masses (the entry the device build of pt_set_env_guide_from_environment ends in), and of check_auto.
// Built with -fsanitize=address,undefined and run by tests/test_env_guide_masses.py; tests/test_env_guide_auto_abi.py uses
// the `auto` mode to compare the library's messages with check_auto's.
//
//   env_guide_masses_main check                                    prints "ok <cases>" and exits 0
//   env_guide_masses_main auto SIZE ROWS COLS S ALPHA FOLLOW       prints check_auto's message (empty line: accepted)
//   env_guide_masses_main auto null                                ... for a NULL struct
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Rng {   // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
};

struct Image { uint32_t w, h; std::vector<float> bgr; };

// tests/env_guide_model.py::sun_map: 64 wide, 32 high, radiance `base`, a 2 x 2-texel source of `sun` at rows and columns 15, 16
Image sun_map(float base, float sun) {
  Image I{64, 32, std::vector<float>(64u * 32u * 3u, base)};
  for (uint32_t r = 15; r <= 16; ++r)
    for (uint32_t c = 15; c <= 16; ++c)
      for (int k = 0; k < 3; ++k) I.bgr[3 * ((size_t)r * 64 + c) + k] = sun;
  return I;
}

Image random_image(uint32_t h, uint32_t w, uint64_t seed) {
  Rng rng{seed};
  Image I{w, h, std::vector<float>((size_t)w * h * 3)};
  for (float& v : I.bgr) { const float x = rng.unit(); v = x * x * x * 50.f; }
  return I;
}

// The cell masses summed by hand: per texel ((0.0722 B + 0.7152 G) + 0.2126 R) sin(pi (r + 0.5) / H), row-major into the cells.
std::vector<double> masses(const Image& I, uint32_t rows, uint32_t cols) {
  std::vector<double> mass((size_t)rows * cols, 0.0);
  const std::vector<double> sn = ptguide::row_sines(I.h);
  for (uint32_t r = 0; r < I.h; ++r)
    for (uint32_t c = 0; c < I.w; ++c) {
      const float* t = &I.bgr[3 * ((size_t)r * I.w + c)];
      const double y = (0.0722 * (double)t[0] + 0.7152 * (double)t[1]) + 0.2126 * (double)t[2];
      mass[(size_t)((uint64_t)r * rows / I.h) * cols + (size_t)((uint64_t)c * cols / I.w)] += y * sn[r];
    }
  return mass;
}

void compare(const char* name, const Image& I, uint32_t rows, uint32_t cols, float alpha) {
  pt_env_guide g{};
  g.struct_size = sizeof(pt_env_guide);
  g.width = I.w; g.height = I.h; g.rows = rows; g.cols = cols; g.alpha = alpha; g.bgr = I.bgr.data();
  const std::string bad = ptguide::check(&g);
  CHECK(bad.empty(), "%s: %s", name, bad.c_str());
  if (!bad.empty()) return;
  ptguide::Table A, B;
  const std::string why_a = ptguide::build(g, A);
  const std::vector<double> mass = masses(I, rows, cols);
  const std::string why_b = ptguide::build_from_masses(rows, cols, alpha, mass, B);
  CHECK(why_a.empty() && why_b.empty(), "%s: build '%s', build_from_masses '%s'", name, why_a.c_str(), why_b.c_str());
  if (!why_a.empty() || !why_b.empty()) return;
  const size_t n = (size_t)rows * cols;
  CHECK(A.rows == B.rows && A.cols == B.cols && A.log2n == B.log2n && A.log2cols == B.log2cols, "%s: geometry", name);
  CHECK(A.alpha_thr == B.alpha_thr && A.alpha == B.alpha, "%s: alpha", name);
  CHECK(B.threshold.size() == n && B.alias.size() == n && B.q.size() == n && B.P.size() == n && B.ideal.size() == n, "%s: sizes", name);
  if (B.threshold.size() != n || A.threshold.size() != n) return;
  std::vector<int> pointed(n, 0);
  for (size_t k = 0; k < n; ++k) {
    CHECK(A.threshold[k] == B.threshold[k], "%s: threshold[%zu] %u != %u", name, k, A.threshold[k], B.threshold[k]);
    CHECK(A.alias[k] == B.alias[k], "%s: alias[%zu] %u != %u", name, k, A.alias[k], B.alias[k]);
    CHECK(std::memcmp(&A.q[k], &B.q[k], 4) == 0, "%s: q[%zu] %.9g != %.9g", name, k, A.q[k], B.q[k]);
    CHECK(std::memcmp(&A.P[k], &B.P[k], 8) == 0 && std::memcmp(&A.ideal[k], &B.ideal[k], 8) == 0, "%s: P / ideal [%zu]", name, k);
    CHECK(B.alias[k] < n, "%s: alias[%zu] out of range", name, k);
    if (B.alias[k] < n && B.threshold[k] != 0xffffffffu && B.alias[k] != k) pointed[B.alias[k]] += 1;
  }
  // a cell without mass is never drawn: threshold 0 and no column hands its remainder to it
  for (size_t k = 0; k < n; ++k)
    if (mass[k] == 0.0) {
      CHECK(B.threshold[k] == 0u, "%s: empty cell %zu has threshold %u", name, k, B.threshold[k]);
      CHECK(pointed[k] == 0, "%s: %d aliases point at the empty cell %zu", name, pointed[k], k);
      for (size_t j = 0; j < n; ++j)
        CHECK(!(B.alias[j] == k && j != k), "%s: alias[%zu] names the empty cell %zu", name, j, k);
      CHECK(B.P[k] == 0.0 && B.q[k] == 0.f, "%s: empty cell %zu has P %.12g", name, k, B.P[k]);
    }
}

int run_checks() {
  int cases = 0;
  const Image images[] = {sun_map(0.25f, 4000.f), random_image(24, 40, 2024), sun_map(0.f, 4000.f)};   // the last: mass in a few cells only
  const char* names[] = {"sun_map", "random 24 x 40", "sun on black"};
  const uint32_t grids[][2] = {{8, 16}, {1, 2}};
  for (int i = 0; i < 3; ++i)
    for (const auto& gr : grids)
      for (float alpha : {0.5f, 0.f, 0.9f}) {
        compare(names[i], images[i], gr[0], gr[1], alpha);
        ++cases;
      }
  {   // sun on black, 8 x 16: the 2 x 2 source straddles rows 15, 16 (cells 3, 4) and columns 15, 16 (cell 3, 4): 4 cells have mass
    const std::vector<double> mass = masses(images[2], 8, 16);
    int with_mass = 0;
    for (double m : mass) with_mass += m > 0.0;
    CHECK(with_mass == 4, "sun on black: %d cells with mass", with_mass);
  }
  {   // no mass at all is refused, naming the total, and `what` names the source
    ptguide::Table T;
    const std::string why = ptguide::build_from_masses(2, 2, 0.5f, std::vector<double>(4, 0.0), T, "the environment");
    CHECK(why.find("total mass") != std::string::npos && why.find("the environment") != std::string::npos, "black: %s", why.c_str());
    const std::string inf = ptguide::build_from_masses(1, 2, 0.5f, std::vector<double>{1.0, HUGE_VAL}, T);
    CHECK(inf.find("total mass") != std::string::npos, "infinite total: %s", inf.c_str());
  }
  {   // the sine table is build()'s expression
    const std::vector<double> sn = ptguide::row_sines(48);
    bool same = sn.size() == 48;
    for (uint32_t r = 0; same && r < 48; ++r) same = sn[r] == std::sin(ptguide::kPi * ((double)r + 0.5) / 48.0);
    CHECK(same, "row_sines");
  }
  if (g_failures) { std::printf("%d check(s) failed\n", g_failures); return 1; }
  std::printf("ok %d\n", cases);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "check")) return run_checks();
  if (argc == 3 && !std::strcmp(argv[1], "auto") && !std::strcmp(argv[2], "null")) {
    std::printf("%s\n", ptguide::check_auto(nullptr).c_str());
    return 0;
  }
  if (argc == 8 && !std::strcmp(argv[1], "auto")) {
    pt_env_guide_auto a{};
    a.struct_size = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    a.rows = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    a.cols = (uint32_t)std::strtoul(argv[4], nullptr, 10);
    a.supersample = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    a.alpha = std::strtof(argv[6], nullptr);
    a.follow = (int32_t)std::strtol(argv[7], nullptr, 10);
    std::printf("%s\n", ptguide::check_auto(&a).c_str());
    return 0;
  }
  std::printf("usage: env_guide_masses_main check | auto SIZE ROWS COLS S ALPHA FOLLOW | auto null\n");
  return 2;
}
