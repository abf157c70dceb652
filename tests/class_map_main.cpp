// The class map of a mapped step (ipu_path_trace_amd/csrc/ptmi_share_plan.h: class_axis_index, class_map_index, the words of the
// map, map_clear_skippable, map_mark_after_step) on the CPU: tests/test_class_map.py builds this with
// -fsanitize=address,undefined and runs it.  Every float coordinate of [0, 2] goes through the axis index; a sequential model of
// C(b), E(b)'s hop and the release (pt_nif_group.h: class_map_claim, group_expand, class_map_release_kernel) runs over
// generated queues; the mark rule runs over every sequence of step kinds.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <unordered_map>
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

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

// ---- regular and irregular, as the header states it, written out once more
static bool regular_by_rule(float coord) {
  const uint32_t c = class_coord(coord), mag = c & 0x7fffffffu;
  return (c & 0x80000000u) && (c & 0x1fffu) == 0 && mag >= kClassMinMag && mag <= kClassMaxMag;
}
// ... and by value: x = (coord - 1) * 2 in [-2, -2^-14]
static bool regular_by_value(float coord) {
  const float x = (coord - 1.0f) * 2.0f;
  return x >= -2.0f && x <= -0x1p-14f;   // false for NaN
}

static void check_coord(float coord) {
  const uint32_t i = class_axis_index(class_coord(coord));
  CHECK(regular_by_rule(coord) == regular_by_value(coord));
  CHECK((i != kClassIrregular) == regular_by_rule(coord));
  if (i != kClassIrregular) {
    CHECK(i <= 15360u && i < kClassAxis);
    CHECK(kClassMinMag + (i << 13) == (class_coord(coord) & 0x7fffffffu));   // the index names the class's bits
  }
}

// Every float of [0, 2] (stride 1): class_of[i] is the one class_coord seen with axis index i, so two regular coordinates share
// an index exactly when their class_coord bits are equal -- the index is a function of the bits, and no two classes meet in one
// entry of the table.
static void sweep() {
  const uint32_t first = bits(0.0f), last = bits(2.0f);
  const unsigned hw = std::thread::hardware_concurrency();
  const unsigned T = hw == 0 ? 1 : hw > 8 ? 8 : hw;
  std::vector<std::vector<uint32_t>> class_of(T, std::vector<uint32_t>(kClassAxis, 0u));
  std::atomic<uint64_t> bad{0}, regular{0};
  std::vector<std::thread> pool;
  const uint64_t n = (uint64_t)last - first + 1, per = (n + T - 1) / T;
  for (unsigned t = 0; t < T; ++t)
    pool.emplace_back([=, &bad, &regular, &class_of] {
      const uint64_t i0 = (uint64_t)t * per, i1 = std::min<uint64_t>(n, i0 + per);
      uint64_t mine = 0, reg = 0;
      std::vector<uint32_t>& seen = class_of[t];
      for (uint64_t k = i0; k < i1; ++k) {
        const float coord = from_bits((uint32_t)(first + k));
        const uint32_t c = class_coord(coord), i = class_axis_index(c);
        const bool want = coord < 1.0f && (coord - 1.0f) * 2.0f <= -0x1p-14f;   // in [0, 2]: x in [-2, -2^-14]
        mine += (i != kClassIrregular) != want;
        if (i == kClassIrregular) continue;
        reg += 1;
        if (i > 15360u) { mine += 1; continue; }
        if (seen[i] == 0u) seen[i] = c;
        mine += seen[i] != c;
      }
      bad += mine; regular += reg;
    });
  for (auto& th : pool) th.join();
  CHECK(bad.load() == 0);
  uint32_t hit = 0, last_class = 0;
  for (uint32_t i = 0; i < kClassAxis; ++i) {   // the threads agree, and every index has a class
    uint32_t c = 0;
    for (unsigned t = 0; t < T; ++t)
      if (class_of[t][i]) { CHECK(c == 0 || c == class_of[t][i]); c = class_of[t][i]; }
    hit += c != 0;
    if (c) { CHECK(last_class < c); last_class = c; }   // ... and distinct indices, distinct classes: the classes rise with the index
  }
  CHECK(hit == kClassAxis - 512u);   // every class that has a coordinate (main: every other one of the first 1024 has none)
  std::printf("swept %llu coordinates of [0, 2] (%u threads): %llu regular, %u axis indices\n", (unsigned long long)n, T,
              (unsigned long long)regular.load(), hit);
}

// ---- a sequential model of a mapped step
constexpr uint32_t kMaxProbes = 32;   // kShareMaxProbes
constexpr uint64_t kEmptyKey = ~0ull;  // kShareEmpty
static uint32_t hash64(uint64_t k) {   // share_hash
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

struct Step {
  std::unordered_map<uint32_t, uint32_t> words;   // the map and the tail's values: a word that is not here is kMapEmpty
  std::vector<uint64_t> tail_keys;
  std::vector<float> c_u, c_v;                    // the class store: row = position
  uint64_t alone = 0;
  explicit Step(uint32_t tail_slots) : tail_keys(tail_slots, kEmptyKey) {}
  uint32_t word(uint32_t slot) const { auto it = words.find(slot); return it == words.end() ? kMapEmpty : it->second; }

  // C(b) over one batch's queue.  `lag`: a winner stores its row only after this many later entries have looked, as the lanes of
  // a tile do (they look first and append together): those entries see kMapClaimed and write a pending class word.
  std::vector<uint32_t> claim(const std::vector<float>& u, const std::vector<float>& v, uint32_t lag) {
    std::vector<uint32_t> owner(u.size());
    std::vector<std::pair<size_t, std::pair<uint32_t, uint32_t>>> due;   // (entry at which it lands, (slot, row))
    auto land = [&](size_t now) {
      for (auto it = due.begin(); it != due.end();)
        if (it->first <= now) { words[it->second.first] = it->second.second; it = due.erase(it); } else ++it;
    };
    for (size_t q = 0; q < u.size(); ++q) {
      land(q);
      uint32_t slot = class_map_index(u[q], v[q]);
      bool none = false;
      if (slot == kClassIrregular) {
        const uint64_t key = class_key(u[q], v[q]);
        none = true;
        if (key != kEmptyKey) {
          const uint32_t mask = (uint32_t)tail_keys.size() - 1u;
          uint32_t s = hash64(key) & mask;
          for (uint32_t p = 0; p < kMaxProbes; ++p, s = (s + 1u) & mask) {
            if (tail_keys[s] == kEmptyKey) tail_keys[s] = key;
            if (tail_keys[s] == key) { none = false; slot = kClassMapWords + s; break; }
          }
        }
      }
      if (none) {   // evaluated alone: a row of its own
        owner[q] = (uint32_t)c_u.size();
        c_u.push_back(u[q]); c_v.push_back(v[q]);
        alone += 1;
        continue;
      }
      CHECK(slot <= kOwnerSlotBits && owner_is_class(owner_class(slot)) && owner_slot(owner_class(slot)) == slot);
      const uint32_t w = word(slot);
      if (w == kMapEmpty) {
        const uint32_t row = (uint32_t)c_u.size();
        c_u.push_back(u[q]); c_v.push_back(v[q]);
        words[slot] = kMapClaimed;
        due.push_back({q + 1 + lag, {slot, row}});
        owner[q] = row;
      } else {
        owner[q] = owner_is_store(w) ? w : owner_class(slot);
      }
    }
    land(~(size_t)0);
    return owner;
  }
  // E(b)'s hop
  uint32_t row_of(uint32_t o) const { return owner_is_store(o) ? o : word(owner_slot(o)); }
  // the release: the word of every regular row, and the tail as a whole
  void release() {
    for (size_t i = 0; i < c_u.size(); ++i) {
      const uint32_t slot = class_map_index(c_u[i], c_v[i]);
      if (slot != kClassIrregular) words.erase(slot);
    }
    for (uint32_t s = 0; s < tail_keys.size(); ++s) { tail_keys[s] = kEmptyKey; words.erase(kClassMapWords + s); }
  }
};

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

// a queue of n entries: a few values per axis (so that classes repeat, some of them two floats of one class), and irregular
// entries of every kind mixed in
static void make_queue(size_t n, uint32_t values, uint32_t irregular_every, std::vector<float>& u, std::vector<float>& v) {
  const float odd[] = {1.0f, 1.5f, std::nanf(""), from_bits(0xffffffffu), 1.0f - 0x1p-16f, 1.0f - 0x1p-17f, 2.0f, from_bits(0x7fc00001u)};
  u.resize(n); v.resize(n);
  for (size_t i = 0; i < n; ++i) {
    u[i] = (float)(rnd() % values) / (float)values + (rnd() & 1u ? 0x1p-20f : 0.0f);
    v[i] = (float)(rnd() % values) / (float)values;
    if (irregular_every && rnd() % irregular_every == 0) {
      const uint32_t which = rnd() % 8u;
      if (rnd() & 1u) u[i] = odd[which]; else v[i] = odd[which];
      if (which == 3 && (rnd() & 1u)) u[i] = v[i] = odd[3];   // the empty marker itself
    }
  }
}

static void model(uint32_t tail_slots, uint32_t batches, size_t n, uint32_t values, uint32_t irregular_every, uint32_t lag) {
  Step step(tail_slots);
  for (int round = 0; round < 2; ++round) {   // twice: the second finds what the release left
    std::map<uint64_t, uint32_t> class_rows;   // class_key -> the row every entry of the class must end at
    uint64_t entries_alone = 0;
    step.c_u.clear(); step.c_v.clear(); step.alone = 0;
    for (uint32_t b = 0; b < batches; ++b) {
      std::vector<float> u, v;
      make_queue(n, values, irregular_every, u, v);
      const uint64_t alone_before = step.alone;
      const size_t rows_before = step.c_u.size();
      const std::vector<uint32_t> owner = step.claim(u, v, lag);
      for (size_t q = 0; q < n; ++q) {
        const uint32_t row = step.row_of(owner[q]);
        CHECK(owner_is_store(row) && row < step.c_u.size());
        // the row holds a pair of the entry's class: the NIF kernels compute the entry's own output from it
        const uint64_t key = class_key(u[q], v[q]);
        CHECK(class_key(step.c_u[row], step.c_v[row]) == key);
        auto it = class_rows.find(key);
        if (it == class_rows.end()) class_rows[key] = row;
        else if (it->second != row) entries_alone += 1;   // only an entry evaluated alone leaves its class's row
      }
      if (tail_slots >= n * batches * 2 && irregular_every == 0) CHECK(step.alone == 0);
    }
    // rows = distinct classes + alone; an entry that left its class's row was evaluated alone (its class's first entry may have been too)
    CHECK(step.c_u.size() <= class_rows.size() + step.alone);
    CHECK(step.c_u.size() >= class_rows.size());
    CHECK(entries_alone <= step.alone);
    {   // exactly: every class that has a word owns one row; every alone entry one more
      size_t taken = 0;
      for (const auto& w : step.words) { CHECK(owner_is_store(w.second)); taken += 1; }   // no word is left claimed
      CHECK(step.c_u.size() == taken + step.alone);
    }
    step.release();
    CHECK(step.words.empty());   // nothing is left behind
    for (uint64_t k : step.tail_keys) CHECK(k == kEmptyKey);
  }
}

// ---- the mark against a model of the map itself
enum Op { kOpMapped, kOpOther, kOpMappedFailed, kOpOtherFailed, kOpRealloc, kOps };
struct MapModel {
  bool dirty = true;   // a fresh allocation holds anything
  bool mark = false;
  uint32_t clears = 0, skips = 0;
};
static void run(MapModel& m, Op op) {
  if (op == kOpRealloc) { m.dirty = true; m.mark = false; return; }   // alloc_class_map drops the mark where it happens
  const bool used = op == kOpMapped || op == kOpMappedFailed, ok = op == kOpMapped || op == kOpOther;
  if (used) {
    if (map_clear_skippable(m.mark)) m.skips += 1;
    else { m.dirty = false; m.clears += 1; }
    CHECK(!m.dirty);   // C(0) starts on an empty map
    m.dirty = true;    // the step's claims
    if (ok) m.dirty = false;   // the release; a failed step may have stopped ahead of it
  }
  m.mark = map_mark_after_step(m.mark, used, ok);
  CHECK(!m.mark || !m.dirty);   // the mark never says more than is true
}

int main() {
  static_assert(kClassAxis == 15361u && kClassMapWords == 235960321u, "the class space of [0, 1)^2");
  static_assert(kMapEmpty != kMapClaimed && !owner_is_store(kMapEmpty) && !owner_is_store(kMapClaimed), "a row is neither");
  static_assert(class_map_bytes(kClassTailSlots) < (1ull << 30), "under a GiB");

  // the ends: coord = 0 (x = -2) and the last float below 1 - 2^-15 that still rounds to -2^-14; -0 is 0's class
  CHECK(class_axis_index(class_coord(0.0f)) == 15360u && class_axis_index(class_coord(-0.0f)) == 15360u);
  CHECK(class_axis_index(class_coord(1.0f - 0x1p-15f)) == 0u);
  CHECK(class_axis_index(class_coord(1.0f)) == kClassIrregular);               // x = 0
  CHECK(class_axis_index(class_coord(1.0f - 0x1p-16f)) == kClassIrregular);    // |x| = 2^-15 < 2^-14
  CHECK(class_axis_index(class_coord(from_bits(bits(1.0f) - 1u))) == kClassIrregular);
  for (float c : {1.5f, 2.0f, 3.0f, 1e30f, -0.25f, -1e30f, std::nanf(""), from_bits(0xffffffffu), from_bits(0x7f800000u), from_bits(0xff800000u)})
    CHECK(class_axis_index(class_coord(c)) == kClassIrregular);
  // +- 4 ulps round every rounding boundary of the range, as coordinates: x = -(h + 1/2 ulp of a half) <=> coord = 1 + x / 2
  for (uint32_t h = kClassMinMag; h < kClassMaxMag; h += 0x2000u)
    for (int d = -4; d <= 4; ++d) {
      const float xm = from_bits(0x80000000u | (h + 0x1000u)), xh = from_bits(0x80000000u | h);
      for (float x : {xm, xh}) {
        const float coord = 1.0f + x * 0.5f;
        check_coord(from_bits(bits(coord) + (uint32_t)d));
      }
    }
  for (float c : {0.0f, 1.0f, 2.0f, 0.5f, 1.5f, 0.25f, 0.999999f, 1.000001f, -0.0f, -0.25f, -3.0f, 2.5f, 1e30f, -1e30f, 1e-30f, 1.0f - 0x1p-15f})
    for (int d = -4; d <= 4; ++d) check_coord(from_bits(bits(c) + (uint32_t)d));
  check_coord(std::nanf(""));
  check_coord(from_bits(0xffffffffu));

  // the pair index: row-major over the two axis indices covers [0, 15361^2) once each (the expression, written out here), and
  // class_map_index is that expression of the two axis indices on a sample of pairs (the axis index itself is swept in full
  // below); irregular if either coordinate is
  {
    std::vector<float> axis(kClassAxis);
    for (uint32_t i = 0; i < kClassAxis; ++i) {
      // the coordinate whose x is the class's own half.  Below 1 a float steps by 2^-24, so x steps by 2^-23; the halves below
      // 2^-13 step by 2^-24: every other one of the first 1024 classes has no coordinate at all (its word is never used)
      axis[i] = 1.0f + from_bits(0x80000000u | (kClassMinMag + (i << 13))) * 0.5f;
      if (i >= 1024u || !(i & 1u)) CHECK(class_axis_index(class_coord(axis[i])) == i);
      else axis[i] = axis[i - 1];
    }
    std::vector<bool> seen(kClassMapWords, false);
    uint64_t count = 0;
    for (uint32_t iu = 0; iu < kClassAxis; ++iu)
      for (uint32_t iv = 0; iv < kClassAxis; ++iv) {
        const uint32_t m = iu * kClassAxis + iv;   // what class_map_index computes from the two indices ...
        CHECK(m < kClassMapWords && !seen[m]);
        seen[m] = true;
        count += 1;
      }
    CHECK(count == kClassMapWords);
    for (uint32_t k = 0; k < 200000; ++k) {   // ... checked through the floats on a sample, the corners included
      const uint32_t iu = k < 4 ? (k & 1u) * 15360u : rnd() % kClassAxis, iv = k < 4 ? (k >> 1) * 15360u : rnd() % kClassAxis;
      const uint32_t ju = class_axis_index(class_coord(axis[iu])), jv = class_axis_index(class_coord(axis[iv]));
      CHECK((ju == iu || (iu < 1024u && ju == iu - 1u)) && (jv == iv || (iv < 1024u && jv == iv - 1u)));
      CHECK(class_map_index(axis[iu], axis[iv]) == ju * kClassAxis + jv);
    }
    CHECK(class_map_index(1.0f, 0.5f) == kClassIrregular && class_map_index(0.5f, 1.0f) == kClassIrregular);
    CHECK(class_map_index(std::nanf(""), 0.5f) == kClassIrregular && class_map_index(0.5f, 1.5f) == kClassIrregular);
    CHECK(class_map_index(from_bits(0xffffffffu), from_bits(0xffffffffu)) == kClassIrregular);
    CHECK(class_key(from_bits(0xffffffffu), from_bits(0xffffffffu)) == kEmptyKey);   // the empty marker is its own class key
  }

  sweep();

  // the model: a 4-slot tail that fills, a tail with room, no irregular entry at all; with and without pending words
  for (uint32_t lag : {0u, 3u, 64u}) {
    model(4, 3, 5000, 40, 7, lag);
    model(1u << 16, 3, 5000, 40, 7, lag);
    model(4, 2, 3000, 8, 0, lag);
    model(4, 1, 2049, 3, 2, lag);
    model(2, 4, 100, 1, 1, lag);
  }

  // whether the map may be taken: held, or its bytes and what the step allocates besides within a quarter of the free memory
  {
    const uint64_t need = class_map_bytes(kClassTailSlots);
    CHECK(need == ((uint64_t)kClassMapWords + kClassTailSlots) * 4 + (uint64_t)kClassTailSlots * 8);
    CHECK(class_map_fits(true, kClassTailSlots, 0) && class_map_fits(true, kClassTailSlots, kFreeUnknown, ~0ull >> 1));
    CHECK(!class_map_fits(false, kClassTailSlots, kFreeUnknown));
    CHECK(class_map_fits(false, kClassTailSlots, 4 * need) && !class_map_fits(false, kClassTailSlots, 4 * need - 4));
    CHECK(class_map_fits(false, kClassTailSlots, 4 * (need + 1000), 1000) && !class_map_fits(false, kClassTailSlots, 4 * (need + 1000), 1001));
  }

  // the mark rule, case by case, then over every sequence of four steps behind each history of one
  CHECK(!map_clear_skippable(false) && map_clear_skippable(true));
  for (bool mark : {false, true}) {
    CHECK(map_mark_after_step(mark, true, true) && !map_mark_after_step(mark, true, false));
    CHECK(map_mark_after_step(mark, false, true) == mark && map_mark_after_step(mark, false, false) == mark);   // the map was not touched
  }
  uint32_t sequences = 0, skips = 0;
  for (int first = 0; first < kOps; ++first)
    for (int a = 0; a < kOps; ++a)
      for (int b = 0; b < kOps; ++b)
        for (int c = 0; c < kOps; ++c)
          for (int d = 0; d < kOps; ++d) {
            MapModel m;
            run(m, (Op)first);
            const uint32_t before = m.skips;
            run(m, (Op)a); run(m, (Op)b); run(m, (Op)c); run(m, (Op)d);
            skips += m.skips - before;
            sequences += 1;
          }
  CHECK(sequences == kOps * kOps * kOps * kOps * kOps && skips > 0);
  {
    MapModel m;
    run(m, kOpMapped); run(m, kOpMapped); run(m, kOpOther); run(m, kOpOtherFailed); run(m, kOpMapped);
    CHECK(m.clears == 1 && m.skips == 2);
    run(m, kOpMappedFailed); run(m, kOpMapped);   // the failed step itself skipped; the step behind it clears
    CHECK(m.clears == 2 && m.skips == 3);
    run(m, kOpRealloc); run(m, kOpMapped); run(m, kOpMapped);
    CHECK(m.clears == 3 && m.skips == 4);
  }

  std::printf("CLASS_MAP_OK %u mark sequences, %u skipped clears\n", sequences, skips);
  return 0;
}
