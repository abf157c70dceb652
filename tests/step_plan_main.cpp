// Exercises ipu_path_trace_amd/csrc/ptmi_step_plan.h -- the integer arithmetic of a step -- on the CPU (tests/test_step_plan.py
// builds it with -fsanitize=address,undefined):
//  1. the batch deal: sizes sum to the step, fit the capacity, a short first batch exactly when the step is long enough and
//     has a NIF stage, the rest dealt evenly over as few batches as possible, larger ones first;
//  2. item_divider: (x * magic) >> shift == x / n for x < 2^31, the product formed in 64 bits as the trace kernel forms it;
//  3. trace_grid: the regions of a batch hold its paths.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ptmi_step_plan.h"

using namespace ptplan;

static int failures = 0;
#define CHECK(cond, ...)                                             \
  do {                                                               \
    if (!(cond)) {                                                   \
      if (++failures <= 20) {                                        \
        std::printf("FAILED line %d: %s  [", __LINE__, #cond);       \
        std::printf(__VA_ARGS__);                                    \
        std::printf("]\n");                                          \
      }                                                              \
    }                                                                \
  } while (0)

static void check_deal(uint32_t spp, uint32_t ipb, uint32_t fbi, bool env_const) {
  const std::vector<uint32_t> it = batch_iterations(spp, ipb, fbi, env_const);
  uint64_t sum = 0;
  bool fit = true;
  for (uint32_t x : it) { sum += x; fit = fit && x >= 1 && x <= ipb; }
  CHECK(sum == spp, "spp %u ipb %u first %u const %d: sum %llu", spp, ipb, fbi, (int)env_const, (unsigned long long)sum);
  CHECK(fit, "spp %u ipb %u first %u const %d: a size outside 1..ipb", spp, ipb, fbi, (int)env_const);
  const bool want_first = !env_const && spp > 2 * ipb;
  const uint32_t first = want_first ? (fbi < ipb ? fbi : ipb) : 0;
  size_t r0 = 0;
  if (want_first) {
    CHECK(!it.empty() && it[0] == first, "spp %u ipb %u first %u: first batch %u", spp, ipb, fbi, it.empty() ? 0u : it[0]);
    r0 = 1;
  }
  const uint32_t rest = spp - first;
  CHECK(it.size() - r0 == (rest + ipb - 1) / ipb, "spp %u ipb %u first %u const %d: %zu batches for %u iterations", spp, ipb, fbi,
        (int)env_const, it.size() - r0, rest);
  bool even = true;
  for (size_t i = r0; i < it.size(); ++i) even = even && it[i] <= it[r0] && it[i] + 1 >= it[r0] && (i == r0 || it[i] <= it[i - 1]);
  CHECK(even, "spp %u ipb %u first %u const %d: not dealt evenly, larger first", spp, ipb, fbi, (int)env_const);
}

static void check_divider(uint32_t n, uint64_t& rng) {
  uint32_t magic = 0, shift = 0;
  item_divider(n, magic, shift);
  const uint32_t top = 0x7fffffffu;   // x < 2^31
  const uint32_t fixed[8] = {0u, 1u, n - 1u, n, n + 1u, (1u << 31) - n, top - 1u, top};
  auto one = [&](uint32_t x) {
    if (x > top) return;   // (n + 1 at the largest n)
    const uint32_t q = (uint32_t)(((uint64_t)x * magic) >> shift);
    CHECK(q == x / n, "n %u x %u: %u, not %u (magic %u shift %u)", n, x, q, x / n, magic, shift);
  };
  for (uint32_t x : fixed) one(x);
  for (int i = 0; i < 1000; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;   // Knuth's MMIX LCG, fixed seed
    one((uint32_t)(rng >> 33));
  }
}

static void check_grid(uint32_t total, uint32_t cap) {
  const TraceGrid g = trace_grid(total, cap);
  CHECK(g.blocks >= 1 && g.blocks <= cap, "total %u cap %u: blocks %u", total, cap, g.blocks);
  CHECK(g.n_waves == 4 * g.blocks, "total %u cap %u: n_waves %u", total, cap, g.n_waves);
  CHECK(g.region_cap % 256 == 0, "total %u cap %u: region_cap %u", total, cap, g.region_cap);
  CHECK((uint64_t)g.blocks * g.region_cap >= total, "total %u cap %u: %u x %u slots", total, cap, g.blocks, g.region_cap);
}

int main() {
  for (uint32_t s = 1; s <= 201; ++s) {
    const uint32_t spp = s <= 200 ? s : 65535u;
    for (uint32_t ipb = 1; ipb <= 32; ++ipb)
      for (uint32_t fbi = 1; fbi <= ipb; ++fbi)
        for (int env_const = 0; env_const < 2; ++env_const) check_deal(spp, ipb, fbi, env_const != 0);
  }

  uint64_t rng = 0x9e3779b97f4a7c15ull;
  for (uint32_t n = 1; n <= 4096; ++n) check_divider(n, rng);
  for (uint32_t k = 1; k <= 30; ++k)
    for (uint32_t n = (1u << k) - 1u; n <= (1u << k) + 1u; ++n) check_divider(n, rng);
  check_divider(0x7fffffffu, rng);   // the largest n for which pt_create can yield one iteration per batch

  for (uint32_t cap : {1u, 6u, 1536u}) {
    for (uint32_t total = 1; total <= 70000; ++total) check_grid(total, cap);
    const uint64_t m = 64ull * 4 * cap;   // the paths one round of the grid takes
    for (uint64_t k = 1; k * m < (1ull << 31); k = k < 64 ? k + 1 : k * 2 + 1)
      for (int d = -2; d <= 2; ++d) {
        const uint64_t total = k * m + d;
        if (total >= 1 && total < (1ull << 31)) check_grid((uint32_t)total, cap);
      }
  }

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("STEP_PLAN_OK\n");
  return 0;
}
