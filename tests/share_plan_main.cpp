// The arithmetic of NIF sharing and the memo (ipu_path_trace_amd/csrc/ptmi_share_plan.h) on the CPU: tests/test_share_plan.py
// builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "ptmi_share_plan.h"

using namespace ptshare;

#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

int main() {
  const uint64_t kBig = (1ull << 31) - 1;
  const uint64_t counts[] = {0, 1, 2, 511, 512, 513, 1023, 1024, 1025, 65535, 65536, 65537, 84000000ull, 331200000ull,
                             (1ull << 29) - 1, 1ull << 29, (1ull << 29) + 1, 1ull << 30, kBig};

  uint64_t prev = 0;
  // worst_case_slots: a power of two, load <= 1/2 below the cap, monotone in the entries and in the free memory, within 1/8
  // of the memory; entry counts of 0, 1 and 2^31 - 1
  for (uint64_t e : counts) {
    const uint64_t w = worst_case_slots(e, kFreeUnknown);
    CHECK(pow2(w) && w >= kMinSlots && w <= kMaxSlots && w >= prev);
    CHECK(w >= 2 * e || w == kMaxSlots);
    prev = w;
    uint64_t prev_m = 0;
    for (uint64_t free_b : {0ull, 1ull, 4096ull, 1ull << 20, 1ull << 30, 16ull << 30, 288ull << 30, ~0ull - 1}) {
      const uint64_t m = worst_case_slots(e, free_b);
      CHECK(pow2(m) && m >= kMinSlots && m <= w && m >= prev_m);
      CHECK(m == kMinSlots || m * kSlotBytes <= free_b / kTableMemoryDivisor);
      prev_m = m;
    }
  }
  CHECK(worst_case_slots(0, kFreeUnknown) == 1024 && worst_case_slots(1, kFreeUnknown) == 1024);
  CHECK(worst_case_slots(512, kFreeUnknown) == 1024 && worst_case_slots(513, kFreeUnknown) == 2048);
  CHECK(worst_case_slots(kBig, kFreeUnknown) == kMaxSlots);
  CHECK(worst_case_slots(331200000ull, kFreeUnknown) == kMaxSlots);          // the headline step: 2^30 slots
  CHECK(worst_case_slots(331200000ull, 64ull << 30) == (1ull << 29));        // ... 8 GiB allowed: 2^29 x 12 B = 6 GiB

  // the automatic default's memory budget
  const Held nothing;
  const uint64_t q = 30105600ull, table = kMaxSlots;                           // the headline step: 11 batches
  const uint64_t need = auto_bytes(table, 11, q, nothing);
  CHECK(need == table * 12 + 11 * q * 20 + 2 * q * 4);
  CHECK(auto_fits(table, 11, q, nothing, 4 * need) && !auto_fits(table, 11, q, nothing, 4 * need - 1));
  CHECK(!auto_fits(table, 11, q, nothing, kFreeUnknown) && !auto_fits(table, 11, q, nothing, 0));
  CHECK(!auto_fits(table, 0, q, nothing, ~0ull - 1) && !auto_fits(table, 11, 0, nothing, ~0ull - 1));
  Held all;
  all.table_slots = table; all.store_regions = 11; all.owner_maps = 2;
  CHECK(auto_bytes(table, 11, q, all) == 0 && auto_fits(table, 11, q, all, 0) && auto_fits(table, 11, q, all, kFreeUnknown));
  CHECK(auto_bytes(table, 12, q, all) == 12 * q * 20);                         // a store that has to grow is allocated anew
  Held some;
  some.owner_maps = 1;
  CHECK(auto_bytes(1024, 1, 100, some) == 1024 * 12 + 100 * 20 + 100 * 4);
  // the step store is indexed below 2^31: a step whose store would not be is declined whatever the memory
  CHECK(auto_fits(1024, 2, (1ull << 30) - 1, nothing, ~0ull - 1) && !auto_fits(1024, 2, 1ull << 30, nothing, ~0ull - 1));
  CHECK(auto_fits(1024, 1, kBig, nothing, ~0ull - 1) && !auto_fits(1024, 1, kBig + 1, nothing, ~0ull - 1));
  CHECK(!auto_fits(kMaxSlots, 251, 33177600ull, nothing, 288ull << 30));      // 4K, 1000 samples per step: declined
  CHECK(!auto_fits(1024, kBig, kBig, nothing, ~0ull - 1));

  // the owner word: a store index, a served slot or a pending slot -- exactly one of the three, and the payload comes back
  const uint32_t kLastStore = 0x7fffffffu, kLastSlot = 0x3fffffffu;
  for (uint32_t g : {0u, 1u, kLastSlot, kLastSlot + 1u, kLastStore}) {
    CHECK(owner_is_store(g) && !owner_is_served(g) && !owner_is_pending(g));
  }
  for (uint32_t s : {0u, 1u, kLastSlot - 1u, kLastSlot}) {
    const uint32_t sv = owner_served(s), pd = owner_pending(s);
    CHECK(!owner_is_store(sv) && owner_is_served(sv) && !owner_is_pending(sv) && owner_slot(sv) == s);
    CHECK(!owner_is_store(pd) && !owner_is_served(pd) && owner_is_pending(pd) && owner_slot(pd) == s);
    CHECK(sv != pd);
  }
  CHECK(kMaxSlots == (uint64_t)kLastSlot + 1 && kMaxStoreEntries == (uint64_t)kLastStore + 1);
  CHECK(!owner_is_store((uint32_t)kMaxStoreEntries));   // the first index that is none

  // memo_slots_for: 48 bytes per slot (table + retain list), a power of two in kMinSlots .. kMaxSlots or 0 (refused), within
  // max_bytes, monotone
  CHECK(kMemoBytesPerSlot == 48);
  const unsigned long long k48 = 48 * 1024;
  CHECK(memo_slots_for(0) == 0 && memo_slots_for(k48 - 1) == 0 && memo_slots_for(k48) == 1024 && memo_slots_for(k48 + 1) == 1024);
  CHECK(memo_slots_for(2 * k48 - 1) == 1024 && memo_slots_for(2 * k48) == 2048 && memo_slots_for(2 * k48 + 1) == 2048);
  CHECK(memo_slots_for((48ull << 30) - 1) == (1ull << 29) && memo_slots_for(48ull << 30) == kMaxSlots);
  CHECK(memo_slots_for((48ull << 30) + 1) == kMaxSlots && memo_slots_for((48ull << 31) + 1) == kMaxSlots);
  CHECK(memo_slots_for(~0ull) == kMaxSlots);
  uint64_t prev_slots = 0;
  for (uint64_t bytes : {0ull, 1ull, 47ull, 48ull, k48 - 1, k48, k48 + 1, 2 * k48 - 1, 2 * k48, 2 * k48 + 1, 1ull << 20, (1ull << 30) - 1,
                         1ull << 30, (1ull << 30) + 1, 6ull << 30, (48ull << 30) - 1, 48ull << 30, (48ull << 30) + 1, 1ull << 40, ~0ull - 1,
                         ~0ull}) {
    const uint64_t m = memo_slots_for(bytes);
    CHECK(m == 0 || (pow2(m) && m >= kMinSlots && m <= kMaxSlots));
    CHECK(m * kMemoBytesPerSlot <= bytes);
    CHECK(m == kMaxSlots || 2 * m * kMemoBytesPerSlot > bytes || m == 0);   // the largest that fits
    CHECK(m >= prev_slots);
    prev_slots = m;
  }

  std::printf("SHARE_PLAN_OK\n");
  return 0;
}
