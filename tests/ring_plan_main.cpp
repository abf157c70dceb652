// The ring of batch-buffer sets (ipu_path_trace_amd/csrc/ptmi_step_plan.h: ring_slot, ring_predecessor, store_region) and the
// owner-map count of the automatic sharing budget (ptmi_share_plan.h: auto_bytes, auto_fits) on the CPU: tests/test_ring_plan.py
// builds this with -fsanitize=address,undefined and runs it.  For depths 2 and 3 and steps of 1 to 40 batches:
//  1. a batch and the one `depth` before it use the same set, and no two batches closer than `depth` do;
//  2. ring_predecessor(b) is exactly the set's previous user -- found by replaying the step, not by the formula -- and none
//     for the first `depth` batches;
//  3. the batch-scope store region is the set's, the step-scope one the batch's own.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ptmi_share_plan.h"
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

static void check_ring(uint32_t depth, uint32_t batches) {
  std::vector<uint32_t> last_user(depth, kNoBatch);   // per set: the batch that used it last, as the step goes
  for (uint32_t b = 0; b < batches; ++b) {
    const uint32_t slot = ring_slot(b, depth);
    CHECK(slot < depth, "depth %u batch %u: slot %u", depth, b, slot);
    if (slot >= depth) return;
    if (b >= depth) CHECK(slot == ring_slot(b - depth, depth), "depth %u batch %u: slot %u, batch %u had %u", depth, b, slot, b - depth, ring_slot(b - depth, depth));
    for (uint32_t near = 1; near < depth && near <= b; ++near)
      CHECK(slot != ring_slot(b - near, depth), "depth %u: batches %u and %u share set %u", depth, b, b - near, slot);
    const uint32_t pred = ring_predecessor(b, depth);
    CHECK(pred == last_user[slot], "depth %u batch %u: predecessor %u, the set's previous user is %u", depth, b, pred, last_user[slot]);
    CHECK((b < depth) == (pred == kNoBatch), "depth %u batch %u: predecessor %u", depth, b, pred);
    last_user[slot] = b;
    CHECK(store_region(b, depth, false) == slot, "depth %u batch %u: batch-scope region %u, set %u", depth, b, store_region(b, depth, false), slot);
    CHECK(store_region(b, depth, true) == b, "depth %u batch %u: step-scope region %u", depth, b, store_region(b, depth, true));
  }
}

int main() {
  for (uint32_t depth = 2; depth <= 3; ++depth)
    for (uint32_t batches = 1; batches <= 40; ++batches) check_ring(depth, batches);

  // auto_bytes / auto_fits with the number of owner maps: two by default (unchanged), three for a ring of three sets
  using namespace ptshare;
  const uint64_t q = 30105600ull, table = kMaxSlots;   // the headline step: 11 batches
  const Held nothing;
  CHECK(auto_bytes(table, 11, q, nothing) == table * 12 + 11 * q * 20 + 2 * q * 4, "two-map default");
  CHECK(auto_bytes(table, 11, q, nothing, 2) == auto_bytes(table, 11, q, nothing), "explicit two maps");
  const uint64_t need3 = auto_bytes(table, 11, q, nothing, 3);
  CHECK(need3 == table * 12 + 11 * q * 20 + 3 * q * 4, "three maps needed: %llu", (unsigned long long)need3);
  CHECK(auto_fits(table, 11, q, nothing, 4 * need3, 3) && !auto_fits(table, 11, q, nothing, 4 * need3 - 1, 3), "the budget counts three maps");
  CHECK(auto_fits(table, 11, q, nothing, 4 * need3 - 1), "the two-map default is unchanged");
  for (uint64_t have = 0; have <= 4; ++have) {
    Held held;
    held.table_slots = table; held.store_regions = 11; held.owner_maps = have;
    const uint64_t missing3 = have < 3 ? 3 - have : 0, missing2 = have < 2 ? 2 - have : 0;
    CHECK(auto_bytes(table, 11, q, held, 3) == missing3 * q * 4, "%llu maps held of 3", (unsigned long long)have);
    CHECK(auto_bytes(table, 11, q, held) == missing2 * q * 4, "%llu maps held of 2", (unsigned long long)have);
    CHECK(auto_fits(table, 11, q, held, 0, 3) == (missing3 == 0), "%llu maps held of 3, no memory free", (unsigned long long)have);
    CHECK(auto_fits(table, 11, q, held, kFreeUnknown, 3) == (missing3 == 0), "%llu maps held of 3, free memory unknown", (unsigned long long)have);
  }
  Held two;   // a handle that held the two maps of a two-set ring: the third is what it has to find
  two.owner_maps = 2;
  CHECK(auto_bytes(1024, 1, 100, two, 3) == 1024 * 12 + 100 * 20 + 100 * 4, "third map of a small step");

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("RING_PLAN_OK\n");
  return 0;
}
