// The owner words and the two-hop resolve of the fused claim (ipu_path_trace_amd/csrc/ptmi_share_plan.h: owner_class,
// resolve_two_hops) on the CPU, and a sequential model of the fused claim + resolve of pt_nif_group.h (ShareClassTable) over
// generated queues.  tests/test_fused_claim.py builds this with -fsanitize=address,undefined and runs it.
//
// The model keeps the order of the device passes where it matters: every key of the queue is looked up (raw table, then, for
// an entry that appends, the class table) before any value is written, so a class found claimed leaves a pending class word
// exactly as a claim whose owner has not written its value yet does; then the values; then the resolve, in an order of its own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
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

constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kMaxProbes = 32;   // kShareMaxProbes
static uint32_t hash64(uint64_t k) {   // share_hash
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}
static uint64_t raw_key(float u, float v) { return ((uint64_t)bits(u) << 32) | bits(v); }

// ---- the owner format: three kinds, disjoint; slots round-trip
static void owner_words() {
  const uint32_t slots[] = {0u, 1u, 2u, 1023u, (1u << 29) - 1u, 1u << 29, (1u << 30) - 1u};
  for (uint32_t s : slots) {
    const uint32_t c = owner_class(s), p = owner_pending(s);
    CHECK(owner_slot(c) == s && owner_slot(p) == s);
    CHECK(owner_is_class(c) && !owner_is_pending(c) && !owner_is_store(c));
    CHECK(owner_is_pending(p) && !owner_is_class(p) && !owner_is_store(p));
  }
  const uint32_t stores[] = {0u, 1u, (1u << 29) - 1u, (1u << 30) - 1u, 1u << 30, 0x7fffffffu};
  for (uint32_t g : stores) CHECK(owner_is_store(g) && !owner_is_class(g) && !owner_is_pending(g));
  CHECK(kClassMaxSlots - 1 <= kOwnerSlotBits && kMaxStoreEntries == kOwnerTagged);
  for (uint64_t o = 0; o <= 0xffffffffull; o += 0x0fffffffull) {   // every word is exactly one kind
    const uint32_t w = (uint32_t)o;
    CHECK((int)owner_is_store(w) + (int)owner_is_class(w) + (int)owner_is_pending(w) == 1);
  }
}

// ---- the two-hop rule
static void two_hops() {
  std::vector<uint32_t> raw(8, 0xffffffffu), cls(8, 0xffffffffu);
  raw[1] = 77;                 // a raw slot that holds a class-store index
  raw[2] = owner_class(5);     // ... and one that holds a pending class word
  cls[5] = 91; cls[6] = 13;
  uint32_t back = 0;
  CHECK(resolve_two_hops(42u, raw, cls, &back) == 42u && back == kNoWriteBack);                   // a store index stays
  CHECK(resolve_two_hops(owner_pending(1), raw, cls, &back) == 77u && back == kNoWriteBack);      // one hop
  CHECK(resolve_two_hops(owner_pending(2), raw, cls, &back) == 91u && back == 2u);                // two hops, through a raw slot
  CHECK(resolve_two_hops(owner_class(6), raw, cls, &back) == 13u && back == kNoWriteBack);        // the class slot alone
  CHECK(resolve_two_hops(owner_pending(2), raw, cls) == 91u);                                     // (no write-back asked for)
  raw[2] = 91;                                                                                    // after the write-back: one hop
  CHECK(resolve_two_hops(owner_pending(2), raw, cls, &back) == 91u && back == kNoWriteBack);
}

// ---- the sequential model
struct Table {
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals;
  explicit Table(uint32_t slots) : keys(slots, kEmpty), vals(slots, 0xdeadbeefu) {}
  // the slot of `key`, claimed if it was free (fresh); false: no slot within the probe limit, or the key is the empty marker
  bool lookup(uint64_t key, uint32_t& slot, bool& fresh) {
    fresh = false;
    if (key == kEmpty) return false;
    const uint32_t mask = (uint32_t)keys.size() - 1u;
    uint32_t s = hash64(key) & mask;
    for (uint32_t p = 0; p < kMaxProbes; ++p, s = (s + 1u) & mask) {
      if (keys[s] == kEmpty) { keys[s] = key; fresh = true; slot = s; return true; }
      if (keys[s] == key) { slot = s; return true; }
    }
    return false;
  }
  size_t held() const { size_t n = 0; for (uint64_t k : keys) n += k != kEmpty; return n; }
};

struct Queue { std::vector<float> u, v; };

static void run_model(const Queue& q, uint32_t raw_slots, uint32_t class_slots, bool expect_exact, const char* name) {
  const size_t n = q.u.size();
  Table raw(raw_slots), cls(class_slots);
  struct Entry { bool append = false, fresh = false, c_append = false, c_fresh = false; uint32_t slot = 0, c_slot = 0; };
  std::vector<Entry> e(n);
  uint64_t over = 0, alone = 0;
  for (size_t i = 0; i < n; ++i) {   // every key first
    bool fresh = false;
    const bool found = raw.lookup(raw_key(q.u[i], q.v[i]), e[i].slot, fresh);
    e[i].fresh = fresh;
    e[i].append = fresh || !found;
    over += !found;
    if (!e[i].append) continue;
    bool c_fresh = false;
    const bool c_found = cls.lookup(class_key(q.u[i], q.v[i]), e[i].c_slot, c_fresh);
    e[i].c_fresh = c_fresh;
    e[i].c_append = c_fresh || !c_found;
    alone += !c_found;
  }
  std::vector<uint32_t> owner(n), dq, cq;   // the queues, as indices of their entries
  for (size_t i = 0; i < n; ++i) {   // then the values
    if (!e[i].append) { owner[i] = owner_pending(e[i].slot); continue; }
    dq.push_back((uint32_t)i);
    uint32_t word = owner_class(e[i].c_slot);
    if (e[i].c_append) {
      word = (uint32_t)cq.size();
      cq.push_back((uint32_t)i);
      if (e[i].c_fresh) cls.vals[e[i].c_slot] = word;
    }
    if (e[i].fresh) raw.vals[e[i].slot] = word;
    owner[i] = word;
  }
  size_t second_hops = 0;
  for (size_t j = n; j-- > 0;) {   // the resolve, last entry first, with the write-back
    uint32_t back = 0;
    owner[j] = resolve_two_hops(owner[j], raw.vals, cls.vals, &back);
    if (back != kNoWriteBack) { raw.vals[back] = owner[j]; ++second_hops; }
  }
  // every final owner is the row of a class-queue entry of the same class
  for (size_t i = 0; i < n; ++i) {
    CHECK(owner_is_store(owner[i]) && owner[i] < cq.size());
    const uint32_t row = cq[owner[i]];
    CHECK(class_key(q.u[row], q.v[row]) == class_key(q.u[i], q.v[i]));
  }
  // the raw appends: the keys that hold a slot, and the overflows; the class queue: the classes that hold a slot, and the rows alone
  CHECK(dq.size() == raw.held() + over && cq.size() == cls.held() + alone && cq.size() <= dq.size());
  std::set<uint64_t> pairs, classes;
  for (size_t i = 0; i < n; ++i) { pairs.insert(raw_key(q.u[i], q.v[i])); classes.insert(class_key(q.u[i], q.v[i])); }
  if (expect_exact) {
    CHECK(over == 0 && alone == 0);
    CHECK(dq.size() == pairs.size());       // the raw appends equal the distinct raw pairs
    CHECK(cq.size() == classes.size());     // the class queue holds a row per class
  } else {
    CHECK(dq.size() >= pairs.size() && cq.size() >= classes.size());
  }
  // a second pass over the resolved table takes one hop everywhere
  for (size_t i = 0; i < n; ++i)
    if (!e[i].append) {
      uint32_t back = 0;
      CHECK(resolve_two_hops(owner_pending(e[i].slot), raw.vals, cls.vals, &back) == owner[i]);
    }
  std::printf("%-22s raw %6u class %6u: %zu entries, %zu distinct (%zu pairs), %zu rows (%zu classes), over %llu alone %llu, %zu second hops\n",
              name, raw_slots, class_slots, n, dq.size(), pairs.size(), cq.size(), classes.size(), (unsigned long long)over,
              (unsigned long long)alone, second_hops);
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static Queue make_queue(const char* kind, size_t n) {
  Queue q;
  for (size_t i = 0; i < n; ++i) {
    float u, v;
    if (!std::strcmp(kind, "equal")) { u = 0.3125f; v = 0.75f; }
    else if (!std::strcmp(kind, "distinct")) { u = (float)(i % 1000) / 1024.0f + 0.001f; v = (float)(i / 1000) / 1024.0f + 0.002f; }
    else {   // mixed: a few hundred classes, a few raw pairs in each, each several times; and the special coordinates
      const uint32_t c = rnd() % 300u, j = rnd() % 4u;
      u = from_bits(bits(0.1f + (float)(c % 20u) * 0.04f) + j);
      v = from_bits(bits(0.2f + (float)(c / 20u) * 0.05f) + (j >> 1));
      if (i % 97 == 0) u = 1.0f;                                     // x = 0: out of the class range, its own bits
      if (i % 101 == 0) { u = 1.0f; v = 1.0f; }
      if (i % 211 == 0) { u = from_bits(0xffffffffu); v = u; }       // the empty marker itself: evaluated alone at both levels
    }
    q.u.push_back(u); q.v.push_back(v);
  }
  return q;
}

int main() {
  owner_words();
  two_hops();
  const size_t lengths[] = {1, 2047, 2048, 2049, 3 * 2048 + 5};
  for (const char* kind : {"mixed", "equal", "distinct"})
    for (size_t n : lengths) {
      const Queue q = make_queue(kind, n);
      const bool marker = !std::strcmp(kind, "mixed");   // (the empty-marker entries are alone by rule: not exact)
      run_model(q, 1u << 14, 1u << 14, !marker, kind);
      run_model(q, 16, 1u << 14, false, kind);
      run_model(q, 1u << 14, 4, false, kind);
      run_model(q, 16, 4, false, kind);
    }
  {   // mixed without the marker: exact
    Queue q = make_queue("mixed", 3 * 2048 + 5);
    for (size_t i = 0; i < q.u.size(); ++i)
      if (bits(q.u[i]) == 0xffffffffu) { q.u[i] = 1.0f; q.v[i] = 0.5f; }
    run_model(q, 1u << 14, 1u << 14, true, "mixed, no marker");
  }
  std::printf("FUSED_CLAIM_OK\n");
  return 0;
}
