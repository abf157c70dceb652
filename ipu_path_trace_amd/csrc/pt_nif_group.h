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
//         it is served from.
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
//   count(...)           the table's own counters
#pragma once

#include "ptmi_share_plan.h"

namespace ptd {

constexpr unsigned long long kShareEmpty = ~0ull;     // empty slot: u and v both the all-ones NaN pattern
constexpr uint32_t kShareMaxProbes = 32;              // linear probes before a key is evaluated alone
constexpr int kShareBlock = 256;

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

// slot_mask + 1 slots, a power of two <= 2^30: key and store index of its owner
struct ShareTable {
  unsigned long long* keys;
  uint32_t* vals;
  uint32_t slot_mask;
  static constexpr bool kServes = false;
  __device__ __forceinline__ unsigned long long* key(uint32_t s) const { return keys + s; }
  __device__ __forceinline__ void append(uint32_t, bool, uint32_t) const {}
  __device__ __forceinline__ void claim(uint32_t s, uint32_t g) const { vals[s] = g; }
  __device__ __forceinline__ void stamp(uint32_t) const {}
  __device__ __forceinline__ uint32_t store_index(uint32_t s) const { return vals[s]; }
  __device__ __forceinline__ void count(bool, bool) const {}
};

// slot_mask + 1 slots of pt_nif_memo.h
struct MemoTable {
  MemoSlot* slots;
  uint32_t slot_mask;
  uint32_t step;             // stamp of this step
  uint32_t* d_slot;          // [store index]: memo slot to publish the entry into, or kMemoNoSlot
  unsigned long long* counters;   // kMemoCounters
  static constexpr bool kServes = true;
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
  __device__ __forceinline__ void count(bool served, bool fresh) const {
    wave_count(served, counters + kMemoServedCount);
    wave_count(fresh, counters + kMemoInserted);
    wave_count(fresh, counters + kMemoOccupied);
  }
};
static_assert(offsetof(MemoSlot, g) == offsetof(MemoSlot, b) + 4 && offsetof(MemoSlot, r) == offsetof(MemoSlot, b) + 8,
              "a memo slot holds its BGR as the store does");

// grid (ceil(region_cap / 256), n_regions): x = 256 entries of one region, y = region
template <class Table>
__device__ __forceinline__ void group_claim(const GroupQueue& Q, const Table& T) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  const uint32_t count = Q.region_count[r];
  if (blockIdx.x * (uint32_t)kShareBlock >= count) return;   // uniform over the workgroup
  const bool valid = local < count;
  const uint32_t q = r * Q.region_cap + local;
  // fresh: claimed a new key; alone: no slot (evaluated on its own); served: the table holds the key's value
  bool fresh = false, alone = false, served = false;
  uint32_t slot = 0;
  float u = 0.f, v = 0.f;
  if (valid) {
    u = Q.q_u[q]; v = Q.q_v[q];
    const unsigned long long key = ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)__float_as_uint(v);
    alone = true;
    if (key != kShareEmpty) {
      uint32_t s = share_hash(key) & T.slot_mask;
      for (uint32_t p = 0; p < kShareMaxProbes; ++p, s = (s + 1u) & T.slot_mask) {
        // a plain look first: most entries find their key already there and need no atomic (a stale EMPTY only costs the CAS)
        unsigned long long cur = __hip_atomic_load(T.key(s), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kShareEmpty) cur = atomicCAS(T.key(s), kShareEmpty, key);
        if (cur == kShareEmpty) { fresh = true; alone = false; slot = s; break; }
        if (cur == key) { if constexpr (Table::kServes) served = T.served(s); alone = false; slot = s; break; }
      }
    }
  }
  const bool append = fresh || alone;
  // one atomic per wave for the distinct-queue entries it appends (wave ballot + prefix count, as the trace kernel's queue)
  const uint64_t m = __ballot(append);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t first = 0;
  if (m) {
    const int leader = __ffsll((long long)m) - 1;
    if (lane == (uint32_t)leader) first = atomicAdd(Q.d_count, (uint32_t)__popcll(m));
    first = __shfl(first, leader, 64);
  }
  if (append) {
    const uint32_t i = first + lane_rank(m);
    Q.d_u[i] = u; Q.d_v[i] = v;
    const uint32_t g = Q.base + i;
    T.append(g, fresh, slot);
    if (fresh) T.claim(slot, g);
    Q.owner[q] = g;
  } else if (served) {
    T.stamp(slot);
    Q.owner[q] = ptshare::owner_served(slot);
  } else if (valid) {
    Q.owner[q] = ptshare::owner_pending(slot);   // the key's owner may not have written its store index yet: resolved by the next pass
  }
  wave_count(alone, Q.overflowed);
  T.count(served, fresh);
}

// owner[q] = the store index of the slot's owner, for the entries that found their key claimed by another in this step (every
// store index of the batch is written now)
template <class Table>
__device__ __forceinline__ void group_resolve(const GroupQueue& Q, const Table& T) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= Q.region_count[r]) return;
  const uint32_t q = r * Q.region_cap + local;
  const uint32_t o = Q.owner[q];
  if (ptshare::owner_is_pending(o)) Q.owner[q] = T.store_index(ptshare::owner_slot(o));
}

// the per-path radiance of the NIF heads' per-path mode, from the owner's decoded BGR in the step store or the served slot
// (resolve has left no pending word: whatever is not a store index is served).  A table that serves reads the three values
// in one go ahead of the stores -- a sixth difference, of schedule alone: its slots lie anywhere in a table of gigabytes,
// and with three reads that each wait for the store before them the memo's passes took a sixth more time per step
// (profiles/r18_nif_group.txt).  Without one the reads stay where share_expand_kernel always had them.
template <class Table>
__device__ __forceinline__ void group_expand(const GroupExpand& E, const Table& T) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= E.region_count[r]) return;
  const uint32_t q = r * E.region_cap + local;
  const uint32_t o = E.owner[q];
  const float* bgr = E.bgr + 3 * (size_t)o;
  float held[3];
  if constexpr (Table::kServes) {
    if (!ptshare::owner_is_store(o)) bgr = T.served_bgr(ptshare::owner_slot(o));
    held[0] = bgr[0]; held[1] = bgr[1]; held[2] = bgr[2];
    bgr = held;
  }
  const uint32_t path = E.q_path[q];
  E.rad_r[path] = bgr[2] * E.q_tr[q];
  E.rad_g[path] = bgr[1] * E.q_tg[q];
  E.rad_b[path] = bgr[0] * E.q_tb[q];
}

__global__ __launch_bounds__(kShareBlock) void share_claim_kernel(GroupQueue Q, ShareTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_resolve_kernel(GroupQueue Q, ShareTable T) { group_resolve(Q, T); }
__global__ __launch_bounds__(kShareBlock) void share_expand_kernel(GroupExpand E, ShareTable T) { group_expand(E, T); }
__global__ __launch_bounds__(kShareBlock) void memo_lookup_kernel(GroupQueue Q, MemoTable T) { group_claim(Q, T); }
__global__ __launch_bounds__(kShareBlock) void memo_resolve_kernel(GroupQueue Q, MemoTable T) { group_resolve(Q, T); }
__global__ __launch_bounds__(kShareBlock) void memo_expand_kernel(GroupExpand E, MemoTable T) { group_expand(E, T); }

}  // namespace ptd
