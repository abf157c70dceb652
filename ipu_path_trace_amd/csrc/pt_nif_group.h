// pt_nif_group.h -- exact sharing of NIF evaluations between queue entries with bit-identical (u, v), within a batch or a step
// (pt_set_nif_sharing) and across steps (pt_set_nif_memo, pt_nif_memo.h): the three passes both run, over either table.
//
// The NIF output of an escaped path depends on its (u, v) alone: the azimuth is folded in by dir_to_uv and the path's
// throughput is applied after the decode, as one fp32 multiply per channel (the heads of pt_nif.h, pt_nif_gemm.h and
// pt_nif_f32.h: rad_r[path] = bgr[2] * q_tr[qi] ...).  Per batch, between the trace kernel T(b) and the NIF launch N(b):
//
//   S(b)  claim + resolve (trace stream): every entry of the queue T(b) wrote claims its 64-bit key (bits of u : bits of v) in
//         an open-addressed device table.  The entry that claims a key appends (u, v) to the batch's DISTINCT queue; every
//         entry records an owner word (ptmi_share_plan.h): the index of its owner in the step's BGR store, or the table slot
//         it is served from.  (Step scope and the memo run the resolve pass at the head of N(b), on the NIF stream:
//         ptmi_nif_group.h, resolve_on_nif_stream.)
//   N(b)  the unmodified NIF kernels in their out_bgr mode (as pt_nif_infer drives them) over the distinct queue.
//   E(b)  expand (accumulate stream, ahead of the accumulate kernel): rad_r[q_path[q]] = bgr_owner[2] * q_tr[q], and likewise
//         for g and b -- the head's own expressions, so every per-path radiance is the per-path mode's bit for bit.
//
// A key that finds no slot within kShareMaxProbes (full table), or that equals the empty marker, takes a distinct-queue
// entry of its own and is counted in `overflowed`: it is evaluated alone, never dropped.
//
// The table is a compile-time policy of the passes.  ShareTable lives for a batch or a step and holds, per key, the store
// index of its owner; MemoTable outlives the step and holds the decoded value itself.  What a table gives the passes is
// exactly where the two differ; the one other difference, of schedule, is named at group_expand:
//   key(s)               the address of slot s's key
//   kServes, served(s)   whether a hit on slot s is served from the table (ShareTable: never, at compile time -- the passes
//                        never ask a table that does not serve for served(s) or served_bgr(s))
//   append(g, fresh, s)  what an append to the distinct queue at store index g records
//   claim(s, g)          what a fresh claim of slot s writes
//   stamp(s)             what a served hit stamps
//   store_index(s)       the owner's store index of a slot claimed in this step, for resolve
//   served_bgr(s)        the BGR of a served slot, for expand
//   count(served, fresh) the table's own counters, a claim tile's sums at a time (only a table that serves has any)
//   key_of(u, v)         the key an entry claims: the 64 raw bits for ShareTable and MemoTable
//   kCountsOnly          the claim pass appends and counts but writes no owner word and no value (RawCountTable)
//   kMapped              expand follows a pending class word through the class map itself (ClassMap)
//
// The class level of N(b).  ClassTable is ShareTable with another key_of: ptshare::class_key, under which two entries are
// equal when the NIF kernels compute the same output for them (ptmi_share_plan.h).  That is a property of the kernels'
// encoder, not of (u, v), so it sits one layer down: on the NIF stream, claim and resolve run once more, over the batch's
// distinct queue as one region; the NIF kernels then run over the class queue, and class_spread_kernel copies every distinct
// entry's BGR from its class owner, so that E(b) and the memo's publish pass read the step store as before.
//
// The fused step (step scope, no memo).  ShareClassTable is ShareTable plus the step's class table and the batch's class queue: the raw table
// claims and counts raw pairs exactly as ShareTable does, but an entry that appends to the distinct queue looks its class up in
// the same pass, and what its raw slot's value and its owner word get is a CLASS-store index, or a pending class word
// (ptmi_share_plan.h: owner_class).  Resolve takes up to two hops, the NIF kernels run over the class queue, and E(b) gathers
// from the class store: no class pass of its own on the NIF stream, no spread, and no BGR in the step store.
//
// The mapped step (the fused step wherever the class map is held or fits; ptmi_share_plan.h).  ClassMap indexes the class of a
// regular (u, v) directly: S(b) is C(b), class_map_claim, which touches no raw table; the raw pairs are claimed and counted by
// R(b), group_claim over RawCountTable, behind A(b) on the accumulate stream, for the statistics alone; E(b) follows a pending class
// word itself, so no resolve pass runs; class_map_release_kernel gives the step's words back at its end.  Over a worklist of a
// multiple of four items E(b) is inside A(b), accumulate_mapped_kernel: the per-path radiance of an escaped path is never
// written.
#pragma once

#include "ptmi_share_plan.h"

namespace ptd {

constexpr unsigned long long kShareEmpty = ~0ull;     // empty slot: u and v both the all-ones NaN pattern
constexpr uint32_t kShareMaxProbes = 32;              // linear probes before a key is evaluated alone
constexpr int kShareBlock = 256;
constexpr uint32_t kClassInFlight = 2;                // class lookups a lane of the fused claim has in flight (of its kClaimK entries)
static_assert(kShareBlock == (int)ptshare::kClaimBlock, "the claim tiles of ptmi_share_plan.h are for this workgroup");

// 64-bit finaliser of MurmurHash3: neighbouring (u, v) bit patterns land on unrelated slots
__device__ __forceinline__ uint32_t share_hash(unsigned long long k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ void wave_count(bool pred, unsigned long long* ctr) {
  const uint64_t m = __ballot(pred);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

}  // namespace ptd

#include "pt_nif_memo.h"   // MemoSlot and the memo's own passes

namespace ptd {

// What claim and resolve read of a batch: the queue of escaped paths as the trace kernel wrote it (one region per trace
// workgroup), its owner map and its distinct queue in the store.
struct GroupQueue {
  const float* q_u; const float* q_v;
  const uint32_t* region_count;
  uint32_t region_cap;
  uint32_t* owner;           // [queue slot]: the entry's owner word
  float* d_u; float* d_v;    // the batch's distinct queue (store index base + i)
  uint32_t* d_count;         // the batch's distinct-queue length
  uint32_t base;             // store index of d_u[0]
  unsigned long long* overflowed;
};

// ... and what expand reads.
struct GroupExpand {
  const uint32_t* region_count;
  uint32_t region_cap;
  const uint32_t* owner;
  const float* bgr;          // the step's BGR store [index][3], written by the NIF kernels' out_bgr mode
  const float* q_tr; const float* q_tg; const float* q_tb;
  const uint32_t* q_path;
  float* rad_r; float* rad_g; float* rad_b;
};

__device__ __forceinline__ unsigned long long raw_key(float u, float v) {
  return ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)__float_as_uint(v);
}

// slot_mask + 1 slots, a power of two <= 2^30: key and store index of its owner
struct ShareTable {
  unsigned long long* keys;
  uint32_t* vals;
  uint32_t slot_mask;
  static constexpr bool kServes = false;
  static constexpr bool kClasses = false;
  static constexpr bool kCountsOnly = false;
  static constexpr bool kMapped = false;
  static __device__ __forceinline__ unsigned long long key_of(float u, float v) { return raw_key(u, v); }
  __device__ __forceinline__ unsigned long long* key(uint32_t s) const { return keys + s; }
  __device__ __forceinline__ void append(uint32_t, bool, uint32_t) const {}
  __device__ __forceinline__ void claim(uint32_t s, uint32_t g) const { vals[s] = g; }
  __device__ __forceinline__ void stamp(uint32_t) const {}
  __device__ __forceinline__ uint32_t store_index(uint32_t s) const { return vals[s]; }
};

// the class level's table (ptmi_share_plan.h: class_slots): key = the class of (u, v), value = the class-store index of its owner
struct ClassTable : ShareTable {
  static __device__ __forceinline__ unsigned long long key_of(float u, float v) { return ptshare::class_key(u, v); }
};

// the fused claim's table: the raw table, whose values are class-store indices or pending class words, the step's class table
// and the batch's class queue (c_u / c_v: class-store index c_base + i; *c_count its length; *c_alone: rows that found no class slot)
struct ShareClassTable : ShareTable {
  ClassTable classes;
  float* c_u; float* c_v;
  uint32_t* c_count;
  uint32_t c_base;
  unsigned long long* c_alone;
  static constexpr bool kClasses = true;
};

// R(b) of a mapped step: the raw table as the raw-pair pass sees it.  The pass claims keys, appends to the batch's distinct queue
// and counts overflows exactly as ShareTable's claim does -- evaluations, overflowed and what pt_calibrate_nif replays keep their
// values -- and writes neither owner[q] nor a slot's value: nothing in the step reads what it produces.
struct RawCountTable : ShareTable {
  static constexpr bool kCountsOnly = true;
};

// The class map of a mapped step (ptmi_share_plan.h): words[0 .. kClassMapWords) one word per regular class, behind them the
// values of the hashed tail, whose keys are tail_keys[0 .. tail_mask]; the batch's class queue as in ShareClassTable.  As a table
// of group_expand: an owner word that is not a row is a pending class word, and the word it names is a row by then.
struct ClassMap {
  uint32_t* words;
  unsigned long long* tail_keys;
  uint32_t tail_mask;
  float* c_u; float* c_v;
  uint32_t* c_count;
  uint32_t c_base;
  unsigned long long* c_alone;
  static constexpr bool kServes = false;
  static constexpr bool kMapped = true;
};

// slot_mask + 1 slots of pt_nif_memo.h
struct MemoTable {
  MemoSlot* slots;
  uint32_t slot_mask;
  uint32_t step;             // stamp of this step
  uint32_t* d_slot;          // [store index]: memo slot to publish the entry into, or kMemoNoSlot
  unsigned long long* counters;   // kMemoCounters
  static constexpr bool kServes = true;
  static constexpr bool kClasses = false;
  static constexpr bool kCountsOnly = false;
  static constexpr bool kMapped = false;
  static __device__ __forceinline__ unsigned long long key_of(float u, float v) { return raw_key(u, v); }
  __device__ __forceinline__ unsigned long long* key(uint32_t s) const { return &slots[s].key; }
  // valid only if published by an earlier step (publish runs after every lookup of its step): a claim of this step whose
  // state is not written yet reads kMemoFree or the stamp, never kMemoValid.  A plain load, no atomic operation.
  __device__ __forceinline__ bool served(uint32_t s) const {
    return __hip_atomic_load(&slots[s].state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kMemoValid;
  }
  __device__ __forceinline__ void append(uint32_t g, bool fresh, uint32_t s) const { d_slot[g] = fresh ? s : kMemoNoSlot; }
  __device__ __forceinline__ void claim(uint32_t s, uint32_t g) const { slots[s].idx = g; slots[s].state = step; }
  __device__ __forceinline__ void stamp(uint32_t s) const { if (slots[s].last_hit != step) slots[s].last_hit = step; }
  __device__ __forceinline__ uint32_t store_index(uint32_t s) const { return slots[s].idx; }
  __device__ __forceinline__ const float* served_bgr(uint32_t s) const { return &slots[s].b; }
  // a claim tile's sums, by one thread of its workgroup
  __device__ __forceinline__ void count(uint32_t served, uint32_t fresh) const {
    if (served) atomicAdd(counters + kMemoServedCount, (unsigned long long)served);
    if (fresh) {
      atomicAdd(counters + kMemoInserted, (unsigned long long)fresh);
      atomicAdd(counters + kMemoOccupied, (unsigned long long)fresh);
    }
  }
};
static_assert(offsetof(MemoSlot, g) == offsetof(MemoSlot, b) + 4 && offsetof(MemoSlot, r) == offsetof(MemoSlot, b) + 8,
              "a memo slot holds its BGR as the store does");

// grid (claim_tiles(region_cap), n_regions): x = one tile of kClaimTile entries of one region, y = region.  A thread takes
// kClaimK entries of the tile (ptmi_share_plan.h: claim_entry) and looks all of them up before anything is appended, so
// kClaimK table loads are in flight per lane; then the workgroup reserves the tile's places in the distinct queue with ONE
// returning atomic on d_count (the waves' append counts meet in LDS, each wave starts behind the waves before it), and the
// tile's overflow and table counters go out once each, non-returning, where they are not zero.  One word takes about 88
// returning atomics per microsecond; a reservation per wave of 64 entries made that rate the cost of the whole pass
// (profiles/r20_claim_counter.txt).
template <class Table>
__device__ __forceinline__ void group_claim(const GroupQueue& Q, const Table& T) {
  constexpr uint32_t K = ptshare::kClaimK, W = ptshare::kClaimWaves;
  __shared__ uint32_t s_appends[W], s_alone[W], s_served[W], s_fresh[W];
  __shared__ uint32_t s_first;
  const uint32_t r = blockIdx.y, tile = blockIdx.x;
  const uint32_t count = Q.region_count[r];
  if (ptshare::claim_tile_idle(tile, count)) return;   // uniform over the workgroup
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t q0 = (size_t)r * Q.region_cap;
  // bit k of each: entry k is below the count / fresh: claimed a new key / alone: no slot (evaluated on its own) / served:
  // the table holds the key's value
  uint32_t valid = 0, fresh = 0, alone = 0, served = 0;
  float u[K], v[K];
  uint32_t slot[K];
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t local = ptshare::claim_entry(tile, threadIdx.x, k);
    // no branch around the loads, so that they go out together: an entry at or above the count reads the region's last
    // live one (the tile is not idle, so there is one) and is not looked at again
    const uint32_t at = local < count ? local : count - 1u;
    u[k] = Q.q_u[q0 + at]; v[k] = Q.q_v[q0 + at];
    valid |= (local < count ? 1u : 0u) << k;
  }
  // a plain look at every key's first slot, all of them in flight together: most entries find their key already there and
  // need no atomic (a stale EMPTY only costs the CAS, and a slot that holds a key keeps it)
  unsigned long long cur[K];
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    const unsigned long long key = Table::key_of(u[k], v[k]);
    slot[k] = share_hash(key) & T.slot_mask;
    cur[k] = __hip_atomic_load(T.key(slot[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (no branch, as above)
  }
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    if (!((valid >> k) & 1u)) continue;
    const unsigned long long key = Table::key_of(u[k], v[k]);
    bool none = true;
    if (key != kShareEmpty) {
      uint32_t s = slot[k];
      unsigned long long c = cur[k];
#pragma unroll 1
      for (uint32_t p = 0;;) {
        if (c == kShareEmpty) c = atomicCAS(T.key(s), kShareEmpty, key);
        if (c == kShareEmpty) { fresh |= 1u << k; none = false; slot[k] = s; break; }
        if (c == key) {
          if constexpr (Table::kServes) { if (T.served(s)) served |= 1u << k; }
          none = false; slot[k] = s; break;
        }
        if (++p == kShareMaxProbes) break;
        s = (s + 1u) & T.slot_mask;
        c = __hip_atomic_load(T.key(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    if (none) alone |= 1u << k;
  }
  const uint32_t append = fresh | alone;
  // The class phase (ShareClassTable): every entry that appends looks its class up in the class table, by the same probe rule.
  // c_append: claimed a class, or found no class slot -- a row of the class queue; otherwise c_slot[k] holds the class.
  [[maybe_unused]] uint32_t c_append = 0, c_fresh = 0, c_slot[K];
  if constexpr (Table::kClasses) {
    __shared__ uint32_t s_c_appends[W], s_c_alone[W];
    __shared__ uint32_t s_c_first;
    uint32_t c_alone = 0;
    // kClassInFlight lookups at a time, not kClaimK: about a quarter of a tile's entries append, and eight more key words
    // beside (u, v), the raw slots and the class slots of eight entries do not fit the step's register budget
    static_assert(K % kClassInFlight == 0, "the class phase takes a lane's entries in whole groups");
#pragma unroll
    for (uint32_t k0 = 0; k0 < K; k0 += kClassInFlight) {
      unsigned long long c_key[kClassInFlight], c_cur[kClassInFlight];
#pragma unroll
      for (uint32_t j = 0; j < kClassInFlight; ++j) {   // the first slots of the group's appending entries, in flight together
        const uint32_t k = k0 + j;
        c_slot[k] = 0u;
        c_key[j] = c_cur[j] = kShareEmpty;
        if ((append >> k) & 1u) {   // key and hash for the entries that append alone: the others never look at theirs
          c_key[j] = ptshare::class_key(u[k], v[k]);
          c_slot[k] = share_hash(c_key[j]) & T.classes.slot_mask;
          c_cur[j] = __hip_atomic_load(T.classes.key(c_slot[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kClassInFlight; ++j) {
        const uint32_t k = k0 + j;
        if (!((append >> k) & 1u)) continue;
        const unsigned long long key = c_key[j];
        bool none = true;
        if (key != kShareEmpty) {
          uint32_t s = c_slot[k];
          unsigned long long c = c_cur[j];
#pragma unroll 1
          for (uint32_t p = 0;;) {
            if (c == kShareEmpty) c = atomicCAS(T.classes.key(s), kShareEmpty, key);
            if (c == kShareEmpty) { c_fresh |= 1u << k; none = false; c_slot[k] = s; break; }
            if (c == key) { none = false; c_slot[k] = s; break; }
            if (++p == kShareMaxProbes) break;
            s = (s + 1u) & T.classes.slot_mask;
            c = __hip_atomic_load(T.classes.key(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        if (none) c_alone |= 1u << k;
      }
    }
    c_append = c_fresh | c_alone;
    // a second reservation per tile, in the class queue
    uint32_t n_c_append = 0, n_c_alone = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
      n_c_append += (uint32_t)__popcll(__ballot((c_append >> k) & 1u));
      n_c_alone += (uint32_t)__popcll(__ballot((c_alone >> k) & 1u));
    }
    if (lane == 0) { s_c_appends[wave] = n_c_append; s_c_alone[wave] = n_c_alone; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t total = ptshare::claim_wave_offset(s_c_appends, W);
      s_c_first = total ? atomicAdd(T.c_count, total) : 0u;
      const uint32_t over = ptshare::claim_wave_offset(s_c_alone, W);
      if (over) atomicAdd(T.c_alone, (unsigned long long)over);
    }
    __syncthreads();
    uint32_t c_next = s_c_first + ptshare::claim_wave_offset(s_c_appends, wave);
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {   // c_slot[k] becomes the entry's word: its row of the class store, or its pending class
      const uint32_t bit = 1u << k;
      const uint64_t m = __ballot((c_append & bit) != 0);
      if (c_append & bit) {
        const uint32_t i = c_next + lane_rank(m);
        T.c_u[i] = u[k]; T.c_v[i] = v[k];
        const uint32_t g = T.c_base + i;
        if (c_fresh & bit) T.classes.claim(c_slot[k], g);
        c_slot[k] = g;
      } else {
        c_slot[k] = ptshare::owner_class(c_slot[k]);
      }
      c_next += (uint32_t)__popcll(m);
    }
  }
  // the wave's counts (wave ballots: scalar work), then the workgroup's through LDS
  uint32_t n_append = 0, n_alone = 0, n_served = 0, n_fresh = 0;
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    n_append += (uint32_t)__popcll(__ballot((append >> k) & 1u));
    n_alone += (uint32_t)__popcll(__ballot((alone >> k) & 1u));
    if constexpr (Table::kServes) {
      n_served += (uint32_t)__popcll(__ballot((served >> k) & 1u));
      n_fresh += (uint32_t)__popcll(__ballot((fresh >> k) & 1u));
    }
  }
  if (lane == 0) {
    s_appends[wave] = n_append; s_alone[wave] = n_alone;
    if constexpr (Table::kServes) { s_served[wave] = n_served; s_fresh[wave] = n_fresh; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = ptshare::claim_wave_offset(s_appends, W);
    s_first = total ? atomicAdd(Q.d_count, total) : 0u;
    const uint32_t over = ptshare::claim_wave_offset(s_alone, W);
    if (over) atomicAdd(Q.overflowed, (unsigned long long)over);
    if constexpr (Table::kServes) T.count(ptshare::claim_wave_offset(s_served, W), ptshare::claim_wave_offset(s_fresh, W));
  }
  __syncthreads();
  uint32_t next = s_first + ptshare::claim_wave_offset(s_appends, wave);   // the wave's next place in the distinct queue
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t bit = 1u << k;
    const size_t q = q0 + ptshare::claim_entry(tile, threadIdx.x, k);
    const uint64_t m = __ballot((append & bit) != 0);
    if (append & bit) {
      const uint32_t i = next + lane_rank(m);
      Q.d_u[i] = u[k]; Q.d_v[i] = v[k];
      uint32_t g = Q.base + i;
      if constexpr (Table::kClasses) g = c_slot[k];   // what the slot and the owner word name is the class row, not the raw one
      if constexpr (!Table::kCountsOnly) {
        T.append(g, (fresh & bit) != 0, slot[k]);
        if (fresh & bit) T.claim(slot[k], g);
        Q.owner[q] = g;
      }
    } else if constexpr (Table::kCountsOnly) {   // (the raw-pair pass: no owner word)
    } else if (served & bit) {
      T.stamp(slot[k]);
      Q.owner[q] = ptshare::owner_served(slot[k]);
    } else if (valid & bit) {
      Q.owner[q] = ptshare::owner_pending(slot[k]);   // the key's owner may not have written its store index yet: resolved by the next pass
    }
    next += (uint32_t)__popcll(m);
  }
}

// owner[q] = the store index of the slot's owner, for the entries that found their key claimed by another in this step (every
// store index of the batch is written now)
template <class Table>
__device__ __forceinline__ void group_resolve(const GroupQueue& Q, const Table& T) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= Q.region_count[r]) return;
  const uint32_t q = r * Q.region_cap + local;
  const uint32_t o = Q.owner[q];
  if constexpr (Table::kClasses) {
    // two hops (ptmi_share_plan.h): raw slot -> pending class word -> class slot.  The final index goes back into the raw slot,
    // so that hits of later batches take one hop: every writer stores the same word, and readers accept either form.
    uint32_t back;
    const uint32_t w = ptshare::resolve_two_hops(o, T.vals, T.classes.vals, &back);
    if (back != ptshare::kNoWriteBack) T.vals[back] = w;
    if (w != o) Q.owner[q] = w;
  } else {
    if (ptshare::owner_is_pending(o)) Q.owner[q] = T.store_index(ptshare::owner_slot(o));
  }
}

// the per-path radiance of the NIF heads' per-path mode, from the owner's decoded BGR in the step store or the served slot
// (resolve has left no pending word: whatever is not a store index is served).  The three values, the throughputs and the
// path are read ahead of the stores with either table: nothing tells the compiler that rad_* and the store do not alias, and
// three reads that each wait for the store before them cost the memo's passes a sixth more time per step
// (profiles/r18_nif_group.txt); the sharing pass has read ahead since round 25 (profiles/r25_step_head_tail.txt).
template <class Table>
__device__ __forceinline__ void group_expand(const GroupExpand& E, const Table& T) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= E.region_count[r]) return;
  const uint32_t q = r * E.region_cap + local;
  uint32_t o = E.owner[q];
  if constexpr (Table::kMapped) {   // a pending class word: its class's word holds the row since the C(b) that claimed it, which N(b) is behind
    if (!ptshare::owner_is_store(o)) o = T.words[ptshare::owner_slot(o)];
  }
  const float* bgr = E.bgr + 3 * (size_t)o;
  if constexpr (Table::kServes) {
    if (!ptshare::owner_is_store(o)) bgr = T.served_bgr(ptshare::owner_slot(o));
  }
  const float held[3] = {bgr[0], bgr[1], bgr[2]};
  const uint32_t path = E.q_path[q];
  const float tr = E.q_tr[q], tg = E.q_tg[q], tb = E.q_tb[q];
  E.rad_r[path] = held[2] * tr;
  E.rad_g[path] = held[1] * tg;
  E.rad_b[path] = held[0] * tb;
}

__global__ __launch_bounds__(kShareBlock) void share_claim_kernel(GroupQueue Q, ShareTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_resolve_kernel(GroupQueue Q, ShareTable T) { group_resolve(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_expand_kernel(GroupExpand E, ShareTable T) { group_expand(E, T); }
__global__ __launch_bounds__(kShareBlock) void memo_lookup_kernel(GroupQueue Q, MemoTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void memo_resolve_kernel(GroupQueue Q, MemoTable T) { group_resolve(Q, T); }
__global__ __launch_bounds__(kShareBlock) void memo_expand_kernel(GroupExpand E, MemoTable T) { group_expand(E, T); }

// The fused step: raw claim with the class lookup inside, two-hop resolve, and the expand from the class store (E.bgr).  The
// claim states its occupancy: six waves per SIMD are the 80 registers of the step's budget (scripts/kernel_resources.py
// --step-budget), which the allocator keeps without scratch with kClassInFlight lookups at a time and not with more.
__global__ __launch_bounds__(kShareBlock) __attribute__((amdgpu_waves_per_eu(6))) void share_class_claim_kernel(GroupQueue Q, ShareClassTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_class_resolve_kernel(GroupQueue Q, ShareClassTable T) { group_resolve(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_class_expand_kernel(GroupExpand E, ShareClassTable T) { group_expand(E, T); }

// ---- the mapped step (ptmi_share_plan.h: the class map).  C(b): one lane per queue entry, in the claim pass's tiles.  An entry
// computes its class slot and looks at the word: a row goes straight into owner[q]; kMapEmpty is taken with a 32-bit CAS to
// kMapClaimed, and the winner appends its (u, v) to the batch's class queue (one reservation per tile) and stores the row into
// the word and into owner[q]; whoever sees kMapClaimed writes a pending class word, which E(b) follows.  An irregular entry finds
// its slot through the tail's keys first, by the tables' probe rule; one that finds none, or whose key is the empty marker, is a
// row of its own, counted in *c_alone.  No raw table is touched.
__device__ __forceinline__ void class_map_claim(const GroupQueue& Q, const ClassMap& M) {
  constexpr uint32_t K = ptshare::kClaimK, W = ptshare::kClaimWaves;
  __shared__ uint32_t s_appends[W], s_alone[W];
  __shared__ uint32_t s_first;
  const uint32_t r = blockIdx.y, tile = blockIdx.x;
  const uint32_t count = Q.region_count[r];
  if (ptshare::claim_tile_idle(tile, count)) return;   // uniform over the workgroup
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const size_t q0 = (size_t)r * Q.region_cap;
  uint32_t valid = 0, fresh = 0, alone = 0;
  float u[K], v[K];
  uint32_t slot[K], word[K];
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {   // (no branch around the loads, as in group_claim)
    const uint32_t local = ptshare::claim_entry(tile, threadIdx.x, k);
    const uint32_t at = local < count ? local : count - 1u;
    u[k] = Q.q_u[q0 + at]; v[k] = Q.q_v[q0 + at];
    valid |= (local < count ? 1u : 0u) << k;
  }
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {   // the words of the regular entries, all in flight together
    slot[k] = ptshare::class_map_index(u[k], v[k]);
    word[k] = ptshare::kMapEmpty;
    if (slot[k] != ptshare::kClassIrregular) word[k] = __hip_atomic_load(M.words + slot[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    if (!((valid >> k) & 1u)) continue;
    if (slot[k] == ptshare::kClassIrregular) {   // the tail: the key's slot first, then its word as for a regular entry
      const unsigned long long key = ptshare::class_key(u[k], v[k]);
      bool none = true;
      if (key != kShareEmpty) {
        uint32_t s = share_hash(key) & M.tail_mask;
#pragma unroll 1
        for (uint32_t p = 0;;) {
          unsigned long long c = __hip_atomic_load(M.tail_keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (c == kShareEmpty) c = atomicCAS(M.tail_keys + s, kShareEmpty, key);
          if (c == kShareEmpty || c == key) { none = false; break; }
          if (++p == kShareMaxProbes) break;
          s = (s + 1u) & M.tail_mask;
        }
        if (!none) {
          slot[k] = ptshare::kClassMapWords + s;
          word[k] = __hip_atomic_load(M.words + slot[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (none) { alone |= 1u << k; continue; }
    }
    if (word[k] == ptshare::kMapEmpty) {
      word[k] = atomicCAS(M.words + slot[k], ptshare::kMapEmpty, ptshare::kMapClaimed);
      if (word[k] == ptshare::kMapEmpty) fresh |= 1u << k;
    }
  }
  const uint32_t append = fresh | alone;
  uint32_t n_append = 0, n_alone = 0;
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    n_append += (uint32_t)__popcll(__ballot((append >> k) & 1u));
    n_alone += (uint32_t)__popcll(__ballot((alone >> k) & 1u));
  }
  if (lane == 0) { s_appends[wave] = n_append; s_alone[wave] = n_alone; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t total = ptshare::claim_wave_offset(s_appends, W);
    s_first = total ? atomicAdd(M.c_count, total) : 0u;
    const uint32_t over = ptshare::claim_wave_offset(s_alone, W);
    if (over) atomicAdd(M.c_alone, (unsigned long long)over);
  }
  __syncthreads();
  uint32_t next = s_first + ptshare::claim_wave_offset(s_appends, wave);
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) {
    const uint32_t bit = 1u << k;
    const size_t q = q0 + ptshare::claim_entry(tile, threadIdx.x, k);
    const uint64_t m = __ballot((append & bit) != 0);
    if (append & bit) {
      const uint32_t i = next + lane_rank(m);
      M.c_u[i] = u[k]; M.c_v[i] = v[k];
      const uint32_t g = M.c_base + i;
      if (fresh & bit) __hip_atomic_store(M.words + slot[k], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      Q.owner[q] = g;
    } else if (valid & bit) {
      Q.owner[q] = ptshare::owner_is_store(word[k]) ? word[k] : ptshare::owner_class(slot[k]);
    }
    next += (uint32_t)__popcll(m);
  }
}

__global__ __launch_bounds__(kShareBlock) void class_map_claim_kernel(GroupQueue Q, ClassMap M) { class_map_claim(Q, M); }
__global__ __launch_bounds__(kShareBlock) void class_map_expand_kernel(GroupExpand E, ClassMap M) { group_expand(E, M); }
// R(b): the raw-pair pass (RawCountTable)
__global__ __launch_bounds__(kShareBlock) void share_raw_claim_kernel(GroupQueue Q, RawCountTable T) { group_claim(Q, T); }

// A(b) of a mapped step with E(b) inside (n % 4 == 0; other worklists keep class_map_expand_kernel and accumulate_kernel): what
// accumulate4_kernel does, but the radiance of an escaped path is formed here, from the class store, and never written.  The
// trace kernel has left the inverse slot map in q_path (ptmi_share_plan.h: kNoQueueSlot): a contributing path (bit 7 of its
// record) reads its slot q; with a slot, its row is owner[q] -- through the map, if that is a pending class word, exactly as
// group_expand goes for kMapped -- and it adds held[2] * q_tr[q], held[1] * q_tg[q], held[0] * q_tb[q]: group_expand's own
// expressions, the products rounded to fp32 before the add (no contraction), so film and records are the bytes of E(b) + A(b).
// Without a slot it ended on an emitter and adds rad_*[path], which the trace kernel wrote.  Nothing is read for a path that does
// not contribute: what an earlier batch left in its q_path word may be no slot of this batch.
struct MappedGather {
  const uint32_t* slot;      // [path]: the inverse map (the set's q_path)
  const uint32_t* owner;     // [queue slot]
  const uint32_t* words;     // the class map and, behind it, the tail's values
  const float* bgr;          // the step's class store
  const float* q_tr; const float* q_tg; const float* q_tb;
  const float* rad_r; const float* rad_g; const float* rad_b;   // emitters
};
// A path's chain is three dependent loads -- slot, owner word, row and throughputs -- and a thread keeps three groups' chains
// in flight, one stage apart.  A group is two CONSECUTIVE work items in two consecutive iterations: four paths, like an iteration
// of accumulate4_kernel, but six accumulators instead of twelve.  While the 24 values of group j are on their way, so are the
// owner words of group j + 1 and the records and slots of group j + 2, and the thread waits for memory once per group.  (Four
// items a thread and two whole iterations side by side, 48 values, took 112 VGPRs; four items, three stages, 85; either held to
// the 80 of the step's budget had scratch: scripts/kernel_resources.py --step-budget.)  A pixel's adds stay in iteration order.
// The arrays indexed by a path or a queue slot are read at 32-bit BYTE offsets from their uniform base: one register of address
// per load, not two.  The host launches the kernel only where that holds (ptshare::kMaxSlotsAt32: 4 * queue_cap < 2^32; a
// batch's path indices are below its queue_cap).  Row indices of the class store reach further and keep 64-bit addresses.
struct MappedStage {
  uint32_t pl;      // the group's path records, iteration k in the low half; 0 past the batch's last iteration
  uint32_t q[4];    // the slots of the contributing paths (2 * iteration + item); kNoQueueSlot for every other path and for one that ended on an emitter
  uint32_t o[4];    // owner[q] (of slot 0 for a path without one: not looked at)
  __device__ __forceinline__ bool has(uint32_t c) const { return q[c] != ptshare::kNoQueueSlot; }
  __device__ __forceinline__ uint32_t slot(uint32_t c) const { return has(c) ? q[c] : 0u; }   // a slot to read in any case
};
template <class T>
__device__ __forceinline__ T at32(const T* base, uint32_t index) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4-byte elements, one or two of them");
  return *reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + (uint32_t)(index * 4u));
}
// records and slots of the group that starts at iteration k (no branch around the loads: an iteration past the last reads the last)
__device__ __forceinline__ void mapped_load_slots(const MappedGather& G, const uint8_t* plen, uint32_t n, uint32_t iters, uint32_t i,
                                                  uint32_t k, MappedStage& s) {
  uint32_t w[2];
  uint2 v[2];
#pragma unroll
  for (uint32_t j = 0; j < 2; ++j) {
    const uint32_t p = (k + j < iters ? k + j : iters - 1u) * n + i;   // a batch's path indices stay below 2^31 (pt_create): 32-bit index arithmetic
    w[j] = *reinterpret_cast<const uint16_t*>(plen + p);
    v[j] = at32(reinterpret_cast<const uint2*>(G.slot), p);
    if (k + j >= iters) w[j] = 0u;
  }
  s.pl = w[0] | (w[1] << 16);
  const uint32_t q[4] = {v[0].x, v[0].y, v[1].x, v[1].y};
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) s.q[c] = ((s.pl >> (8u * c + 7u)) & 1u) ? q[c] : ptshare::kNoQueueSlot;   // whatever else the word holds is no slot of this batch
}
__device__ __forceinline__ void mapped_load_owners(const MappedGather& G, MappedStage& s) {
#pragma unroll
  for (uint32_t c = 0; c < 4; ++c) s.o[c] = at32(G.owner, s.slot(c));
}
__global__ __launch_bounds__(256) void accumulate_mapped_kernel(uint32_t n, uint32_t iters, const uint8_t* plen, MappedGather G, Accum A,
                                                                 unsigned long long* counters) {
  const uint32_t i = 2u * (blockIdx.x * blockDim.x + threadIdx.x);
  uint32_t segs = 0, esc = 0;
  if (i < n) {
    float2 r = *reinterpret_cast<const float2*>(A.r + i), g = *reinterpret_cast<const float2*>(A.g + i),
           b = *reinterpret_cast<const float2*>(A.b + i);
    uint32_t len[2] = {0, 0};
    MappedStage sa, sb, sc;   // the groups at iterations k, k + 2, k + 4
    mapped_load_slots(G, plen, n, iters, i, 0u, sa);
    mapped_load_slots(G, plen, n, iters, i, 2u, sb);
    mapped_load_owners(G, sa);
    float* const rc[2] = {&r.x, &r.y};
    float* const gc[2] = {&g.x, &g.y};
    float* const bc[2] = {&b.x, &b.y};
    for (uint32_t k = 0; k < iters; k += 2u) {
      mapped_load_slots(G, plen, n, iters, i, k + 4u, sc);
      mapped_load_owners(G, sb);
      // the group at k: x = the blue, green and red of a path's row, t = its throughputs.  No branch around the loads (a path
      // without a slot reads row 0 and slot 0, and nothing of it is looked at), so that they go out with the two above.
      float x[4][3], t[4][3];
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {
        uint32_t o = sa.has(c) ? sa.o[c] : 0u;
        if (!ptshare::owner_is_store(o)) o = G.words[ptshare::owner_slot(o)];   // a pending class word: rare, and the one load that is waited for
        const float* held = G.bgr + 3 * (size_t)o;
        x[c][0] = held[0]; x[c][1] = held[1]; x[c][2] = held[2];
        t[c][0] = at32(G.q_tr, sa.slot(c)); t[c][1] = at32(G.q_tg, sa.slot(c)); t[c][2] = at32(G.q_tb, sa.slot(c));
      }
      const uint32_t w = sa.pl;
      len[0] += (w & 0x7fu) + ((w >> 16) & 0x7fu); len[1] += ((w >> 8) & 0x7fu) + ((w >> 24) & 0x7fu);
#pragma unroll
      for (uint32_t c = 0; c < 4; ++c) {   // iteration k's two items, then iteration k + 1's
        if (!((w >> (8u * c + 7u)) & 1u)) continue;
        float vr = x[c][2] * t[c][0], vg = x[c][1] * t[c][1], vb = x[c][0] * t[c][2];   // held[2] * tr, held[1] * tg, held[0] * tb
        if (!sa.has(c)) {   // ended on an emitter: what the trace kernel wrote
          const uint32_t p = (k + (c >> 1)) * n + i + (c & 1u);
          vr = G.rad_r[p]; vg = G.rad_g[p]; vb = G.rad_b[p];
        }
        *rc[c & 1u] += vr; *gc[c & 1u] += vg; *bc[c & 1u] += vb;
      }
      esc += (uint32_t)__popc(w & 0x80808080u);
      sa = sb; sb = sc;
    }
    *reinterpret_cast<float2*>(A.r + i) = r;
    *reinterpret_cast<float2*>(A.g + i) = g;
    *reinterpret_cast<float2*>(A.b + i) = b;
    uint2 cnt = *reinterpret_cast<const uint2*>(A.count + i), ln = *reinterpret_cast<const uint2*>(A.length + i);
    cnt.x += iters; cnt.y += iters;
    ln.x += len[0]; ln.y += len[1];
    *reinterpret_cast<uint2*>(A.count + i) = cnt;
    *reinterpret_cast<uint2*>(A.length + i) = ln;
    segs = len[0] + len[1];
  }
  accumulate_counters(segs, esc, counters);
}

// The release at the end of a mapped step: the word of every regular row of the step's class store goes back to kMapEmpty, so
// that the map is never cleared as a whole (about 6.6 M stores at 1104 x 1000 x 300 spp against a memset of 944 MB).  Rows of
// irregular classes live in the tail, which batch 0's workgroups clear whole in the same launch: its tail_slots values behind
// the map and its keys.  Grid (x, batches): batch y's class queue is c_u / c_v + y * region with c_count[y] rows; grid-stride
// over them.
__global__ __launch_bounds__(kShareBlock) void class_map_release_kernel(const float* c_u, const float* c_v, const uint32_t* c_count,
                                                                        uint32_t region, uint32_t* words, unsigned long long* tail_keys,
                                                                        uint32_t tail_slots) {
  const uint32_t n = c_count[blockIdx.y];
  const size_t base = (size_t)blockIdx.y * region;
  for (uint32_t i = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kShareBlock) {
    const uint32_t slot = ptshare::class_map_index(c_u[base + i], c_v[base + i]);
    if (slot != ptshare::kClassIrregular) words[slot] = ptshare::kMapEmpty;
  }
  if (blockIdx.y == 0) {
    for (uint32_t i = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x; i < tail_slots; i += gridDim.x * (uint32_t)kShareBlock) {
      words[ptshare::kClassMapWords + i] = ptshare::kMapEmpty;
      tail_keys[i] = kShareEmpty;
    }
  }
}

// The class level: claim and resolve over a batch's distinct queue (one region; Q.owner: [position in the distinct queue], the
// class-store index of the entry's class owner; Q.d_u / d_v: the batch's class queue), and the spread behind the NIF launch.
__global__ __launch_bounds__(kShareBlock) void class_claim_kernel(GroupQueue Q, ClassTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void class_resolve_kernel(GroupQueue Q, ClassTable T) { group_resolve(Q, T); }

// bgr[i] = class_bgr[owner[i]] for the *count entries of a batch's distinct queue: 12-byte copies, no arithmetic.  bgr: the
// batch's region of the step store; class_bgr: the step's class store from index 0.  Grid-stride over `cap` >= *count.
__global__ __launch_bounds__(kShareBlock) void class_spread_kernel(const uint32_t* count, const uint32_t* owner, const float* class_bgr,
                                                                   float* bgr) {
  const uint32_t n = *count;
  for (uint32_t i = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kShareBlock) {
    const float* from = class_bgr + 3 * (size_t)owner[i];
    const float b = from[0], g = from[1], r = from[2];
    float* to = bgr + 3 * (size_t)i;
    to[0] = b; to[1] = g; to[2] = r;
  }
}

}  // namespace ptd
