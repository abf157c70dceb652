// The claim pass's tiles (ipu_path_trace_amd/csrc/ptmi_share_plan.h: claim_tiles, claim_tile_idle, claim_entry,
// claim_wave_offset) on the CPU: tests/test_claim_plan.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ptmi_share_plan.h"

using namespace ptshare;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// One region of `cap` slots with `count` live entries, walked as the claim grid walks it: every tile, thread and k.
static void check_region(uint32_t count, uint32_t cap) {
  CHECK(count <= cap);
  const uint32_t tiles = claim_tiles(cap);
  CHECK((uint64_t)tiles * kClaimTile >= cap && (tiles == 0 || (uint64_t)(tiles - 1) * kClaimTile < cap));
  std::vector<uint32_t> taken(count, 0);
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    const bool idle = claim_tile_idle(tile, count);   // one answer per workgroup: it takes nothing thread-specific
    uint32_t live = 0;
    for (uint32_t t = 0; t < kClaimBlock; ++t)
      for (uint32_t k = 0; k < kClaimK; ++k) {
        const uint32_t e = claim_entry(tile, t, k);
        CHECK(e >= tile * kClaimTile && e < (tile + 1) * kClaimTile);
        CHECK(e / 64 == claim_entry(tile, t & ~63u, k) / 64);   // a wave's k-th entries are 64 consecutive ones
        if (e < count) { taken[e] += 1; live += 1; }            // (an index at or above the count is never taken)
      }
    CHECK(idle == (live == 0));
    CHECK(idle == (tile * kClaimTile >= count));
  }
  for (uint32_t e = 0; e < count; ++e) CHECK(taken[e] == 1);
}

int main() {
  static_assert(kClaimTile == kClaimBlock * kClaimK && kClaimWaves * 64 == kClaimBlock, "tile geometry");
  CHECK(claim_tiles(0) == 0 && claim_tiles(1) == 1 && claim_tiles(kClaimTile) == 1 && claim_tiles(kClaimTile + 1) == 2);
  CHECK(claim_tiles(0xffffffffu) == 0xffffffffu / kClaimTile + 1);   // no wrap at the top of the range
  CHECK(!claim_tile_idle(0, 1) && claim_tile_idle(0, 0) && claim_tile_idle(1, kClaimTile) && !claim_tile_idle(1, kClaimTile + 1));
  CHECK(!claim_tile_idle(0xffffffffu / kClaimTile, 0xffffffffu - 5));
  CHECK(claim_tile_idle((uint32_t)((1ull << 32) / kClaimTile), 0xffffffffu));   // the product is taken in 64 bits: no wrap to 0

  const uint32_t counts[] = {0, 1, 255, 256, 257, kClaimTile - 1, kClaimTile, kClaimTile + 1, 3 * kClaimTile + 17};
  for (uint32_t count : counts) {
    // capacities: the count itself, the next multiple of the tile, and some that are no multiple of it
    const uint32_t caps[] = {count, count + 1, count + 63, (count / kClaimTile + 1) * kClaimTile, count + kClaimTile + 5, 4 * kClaimTile + 333};
    for (uint32_t cap : caps)
      if (cap >= count) check_region(count, cap);
  }

  // per-wave offsets: an exclusive scan of the waves' append counts whose total is the reservation
  const uint32_t full = 64 * kClaimK;
  uint32_t cases[][kClaimWaves] = {{0, 0, 0, 0}, {full, full, full, full}, {1, 0, 0, 0}, {0, 0, 0, 1}, {3, 0, full, 7}, {full, 0, 1, 0}, {17, 511, 2, 64}};
  static_assert(kClaimWaves == 4, "the cases above are for four waves");
  for (auto& c : cases) {
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kClaimWaves; ++w) {
      CHECK(claim_wave_offset(c, w) == sum);
      sum += c[w];
    }
    CHECK(claim_wave_offset(c, kClaimWaves) == sum && sum <= kClaimTile);
    // the waves' ranges [offset, offset + count) tile [0, total) without a gap or an overlap
    std::vector<uint32_t> used(sum, 0);
    for (uint32_t w = 0; w < kClaimWaves; ++w)
      for (uint32_t i = 0; i < c[w]; ++i) used[claim_wave_offset(c, w) + i] += 1;
    for (uint32_t x : used) CHECK(x == 1);
  }
  // a pseudo-random sweep of counts in 0 .. 64 * K
  uint32_t rng = 12345u;
  for (int it = 0; it < 1000; ++it) {
    uint32_t c[kClaimWaves], sum = 0;
    for (uint32_t w = 0; w < kClaimWaves; ++w) {
      rng = rng * 1664525u + 1013904223u;
      c[w] = (rng >> 8) % (full + 1);
    }
    for (uint32_t w = 0; w <= kClaimWaves; ++w) {
      CHECK(claim_wave_offset(c, w) == sum);
      if (w < kClaimWaves) sum += c[w];
    }
  }

  std::printf("CLAIM_PLAN_OK\n");
  return 0;
}
