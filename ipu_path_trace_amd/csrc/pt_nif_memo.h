// pt_nif_memo.h -- a persistent device memo of decoded NIF values across steps (pt_set_nif_memo).
//
// The decoded BGR of an escaped path depends on its (u, v) and the uploaded model only (pt_nif_share.h): a value stays valid
// until pt_upload_nif.  With the memo on, the step-scope sharing table of pt_nif_share.h is replaced by a table that outlives
// the step.  One 32-byte slot per entry (one cache line per lookup): key, state, last-hit step, the decoded BGR as the NIF
// kernels' out_bgr mode wrote it, and the step-store index of the entry's owner while it is claimed.  Per batch:
//
//   S(b)  memo_lookup_kernel + memo_resolve_kernel (trace stream).  A key that is VALID (published by an earlier step) is
//         served from its slot: a plain load, no atomic.  A key claimed earlier in this step goes through the owner / store-
//         index path of step-scope sharing.  An absent key is claimed with the 64-bit CAS and appended to the batch's distinct
//         queue, whose index it records for the publish pass.
//   N(b)  the unmodified NIF kernels in their out_bgr mode over the distinct queue (as with sharing).
//   E(b)  memo_expand_kernel: rad_r[q_path[q]] = bgr[2] * q_tr[q] ..., bgr from the step store or the memo slot -- the heads'
//         own single fp32 multiply per channel, so every per-path radiance is the per-path mode's bit for bit.
//
// At the end of the step (after every E(b) and every N(b)), memo_publish_kernel copies the BGR of every newly claimed key into
// its slot and marks it valid: the memo is never read while it is written, and within a step later batches reach this step's
// keys through the step store.  When the occupancy passes 1/2 of the slots, the next step starts with a retain pass:
// memo_compact_kernel lists the valid entries hit in the last step, the table is cleared, memo_reinsert_kernel puts them back.
#pragma once

namespace ptd {

constexpr uint32_t kMemoFree = 0xffffffffu;       // state of a cleared slot (the table is cleared with all-ones bytes)
constexpr uint32_t kMemoValid = 0xfffffffeu;      // state of a published slot: bgr holds the decoded value
constexpr uint32_t kMemoMaxStamp = 0xfffffffdu;   // step stamps run 1 .. kMemoMaxStamp (then wrap to 1)
// owner[q] with the memo on: a step-store index (< 2^31), a served memo slot, or a slot claimed this step still to be resolved
constexpr uint32_t kMemoServed = 0x80000000u;
constexpr uint32_t kMemoResolve = 0xc0000000u;
constexpr uint32_t kMemoSlotBits = 0x3fffffffu;   // slots < 2^30
constexpr uint32_t kMemoNoSlot = 0xffffffffu;     // publish index of a distinct-queue entry that is evaluated alone

struct alignas(32) MemoSlot {
  unsigned long long key;   // bits of u : bits of v, kShareEmpty = free
  uint32_t state;           // kMemoFree, a step stamp (claimed in that step), or kMemoValid
  uint32_t last_hit;        // stamp of the last step that looked the key up
  float b, g, r;            // decoded BGR (valid slots)
  uint32_t idx;             // step-store index of the owner (claimed slots)
};
static_assert(sizeof(MemoSlot) == 32, "one memo slot = 32 bytes");

// counters of the memo passes, cleared at the start of every step (occupied only when the table is cleared)
enum { kMemoOccupied = 0, kMemoServedCount = 1, kMemoInserted = 2, kMemoRetained = 3, kMemoCounters = 4 };

struct MemoParams {
  const float* q_u; const float* q_v;
  const uint32_t* region_count;
  uint32_t region_cap;
  MemoSlot* slots;
  uint32_t slot_mask;
  uint32_t step;             // stamp of this step
  uint32_t* owner;           // [queue slot]
  float* d_u; float* d_v;    // the batch's distinct queue (store index base + i)
  uint32_t* d_slot;          // [store index]: memo slot to publish the entry into, or kMemoNoSlot
  uint32_t* d_count;
  uint32_t base;
  unsigned long long* overflowed;
  unsigned long long* counters;   // kMemoCounters
};

struct MemoExpandParams {
  const uint32_t* region_count;
  uint32_t region_cap;
  const uint32_t* owner;
  const float* bgr;          // the step store [index][3]
  const MemoSlot* slots;
  const float* q_tr; const float* q_tg; const float* q_tb;
  const uint32_t* q_path;
  float* rad_r; float* rad_g; float* rad_b;
};

__device__ __forceinline__ void wave_count(bool pred, unsigned long long* ctr) {
  const uint64_t m = __ballot(pred);
  if (m && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)m) - 1)) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

// grid (ceil(region_cap / 256), n_regions), as share_claim_kernel
__global__ __launch_bounds__(kShareBlock) void memo_lookup_kernel(MemoParams M) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  const uint32_t count = M.region_count[r];
  if (blockIdx.x * (uint32_t)kShareBlock >= count) return;   // uniform over the workgroup
  const bool valid = local < count;
  const uint32_t q = r * M.region_cap + local;
  bool fresh = false, alone = false, served = false;
  uint32_t slot = 0;
  float u = 0.f, v = 0.f;
  if (valid) {
    u = M.q_u[q]; v = M.q_v[q];
    const unsigned long long key = ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)__float_as_uint(v);
    alone = true;
    if (key != kShareEmpty) {
      uint32_t s = share_hash(key) & M.slot_mask;
      for (uint32_t p = 0; p < kShareMaxProbes; ++p, s = (s + 1u) & M.slot_mask) {
        unsigned long long cur = __hip_atomic_load(&M.slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kShareEmpty) cur = atomicCAS(&M.slots[s].key, kShareEmpty, key);
        if (cur == kShareEmpty) { fresh = true; alone = false; slot = s; break; }
        if (cur == key) {
          // valid only if published by an earlier step (publish runs after every lookup of its step): a claim of this step
          // whose state is not written yet reads kMemoFree or the stamp, never kMemoValid
          served = __hip_atomic_load(&M.slots[s].state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kMemoValid;
          alone = false; slot = s;
          break;
        }
      }
    }
  }
  const bool append = fresh || alone;
  const uint64_t m = __ballot(append);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t first = 0;
  if (m) {
    const int leader = __ffsll((long long)m) - 1;
    if (lane == (uint32_t)leader) first = atomicAdd(M.d_count, (uint32_t)__popcll(m));
    first = __shfl(first, leader, 64);
  }
  if (append) {
    const uint32_t i = first + lane_rank(m);
    M.d_u[i] = u; M.d_v[i] = v;
    const uint32_t g = M.base + i;
    M.d_slot[g] = fresh ? slot : kMemoNoSlot;
    if (fresh) { M.slots[slot].idx = g; M.slots[slot].state = M.step; }
    M.owner[q] = g;
  } else if (served) {
    if (M.slots[slot].last_hit != M.step) M.slots[slot].last_hit = M.step;
    M.owner[q] = kMemoServed | slot;
  } else if (valid) {
    M.owner[q] = kMemoResolve | slot;   // claimed in this step by another entry, whose idx may not be written yet
  }
  wave_count(alone, M.overflowed);
  wave_count(served, M.counters + kMemoServedCount);
  wave_count(fresh, M.counters + kMemoInserted);
  wave_count(fresh, M.counters + kMemoOccupied);
}

__global__ __launch_bounds__(kShareBlock) void memo_resolve_kernel(MemoParams M) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= M.region_count[r]) return;
  const uint32_t q = r * M.region_cap + local;
  const uint32_t o = M.owner[q];
  if ((o & kMemoResolve) == kMemoResolve) M.owner[q] = M.slots[o & kMemoSlotBits].idx;
}

__global__ __launch_bounds__(kShareBlock) void memo_expand_kernel(MemoExpandParams E) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= E.region_count[r]) return;
  const uint32_t q = r * E.region_cap + local;
  const uint32_t o = E.owner[q];
  float b, g, rr;
  if (o & kMemoServed) {
    const MemoSlot& s = E.slots[o & kMemoSlotBits];
    b = s.b; g = s.g; rr = s.r;
  } else {
    const float* bgr = E.bgr + 3 * (size_t)o;
    b = bgr[0]; g = bgr[1]; rr = bgr[2];
  }
  const uint32_t path = E.q_path[q];
  E.rad_r[path] = rr * E.q_tr[q];
  E.rad_g[path] = g * E.q_tg[q];
  E.rad_b[path] = b * E.q_tb[q];
}

// Grid-stride passes: a fixed grid (kMemoGrid workgroups, or per batch) walks the whole range, so a 2^30-slot table is not
// 4 M workgroups.  The loop bounds are uniform over a workgroup, so the wave ballots below see every lane.
constexpr uint32_t kMemoGrid = 2048;

// grid (kMemoGrid, batches): region b of the step store holds batch b's distinct queue, d_count[b] entries
__global__ __launch_bounds__(kShareBlock) void memo_publish_kernel(MemoSlot* slots, const uint32_t* d_slot, const float* bgr,
                                                                   const uint32_t* d_count, uint32_t region_cap, uint32_t step) {
  const uint32_t b = blockIdx.y, count = d_count[b];
  for (uint32_t local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x; local < count; local += gridDim.x * (uint32_t)kShareBlock) {
    const uint32_t g = b * region_cap + local;
    const uint32_t s = d_slot[g];
    if (s == kMemoNoSlot) continue;
    MemoSlot& m = slots[s];
    m.b = bgr[3 * (size_t)g]; m.g = bgr[3 * (size_t)g + 1]; m.r = bgr[3 * (size_t)g + 2];
    m.last_hit = step;
    m.state = kMemoValid;
  }
}

// retain pass, 1 of 2: the valid entries hit in step `last` into list[0 .. list_cap); the rest are dropped (a memo may forget)
__global__ __launch_bounds__(kShareBlock) void memo_compact_kernel(const MemoSlot* slots, uint32_t n_slots, uint32_t last,
                                                                   MemoSlot* list, uint32_t list_cap, unsigned long long* counters) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t s0 = blockIdx.x * (uint32_t)kShareBlock; s0 < n_slots; s0 += gridDim.x * (uint32_t)kShareBlock) {
    const uint32_t s = s0 + threadIdx.x;
    bool keep = false;
    MemoSlot e{};
    if (s < n_slots) {
      e = slots[s];
      keep = e.state == kMemoValid && e.last_hit == last;
    }
    const uint64_t m = __ballot(keep);
    unsigned long long first = 0;
    if (m) {
      const int leader = __ffsll((long long)m) - 1;
      if (lane == (uint32_t)leader) first = atomicAdd(counters + kMemoRetained, (unsigned long long)__popcll(m));
      first = __shfl(first, leader, 64);
    }
    if (keep) {
      const unsigned long long i = first + lane_rank(m);
      if (i < list_cap) list[i] = e;
    }
  }
}

// retain pass, 2 of 2 (after the table is cleared): every listed entry back into the table, still valid.  The keys are
// distinct, so a CAS that fails has met another key; an entry with no slot within the probe limit is dropped.
__global__ __launch_bounds__(kShareBlock) void memo_reinsert_kernel(MemoSlot* slots, uint32_t slot_mask, const MemoSlot* list,
                                                                    uint32_t list_cap, unsigned long long* counters) {
  const unsigned long long retained = counters[kMemoRetained];
  const uint32_t n = (uint32_t)(retained < list_cap ? retained : list_cap);
  for (uint32_t i0 = blockIdx.x * (uint32_t)kShareBlock; i0 < n; i0 += gridDim.x * (uint32_t)kShareBlock) {
    const uint32_t i = i0 + threadIdx.x;
    bool placed = false;
    if (i < n) {
      const MemoSlot e = list[i];
      uint32_t s = share_hash(e.key) & slot_mask;
      for (uint32_t p = 0; p < kShareMaxProbes; ++p, s = (s + 1u) & slot_mask) {
        if (atomicCAS(&slots[s].key, kShareEmpty, e.key) == kShareEmpty) {
          MemoSlot& m = slots[s];
          m.b = e.b; m.g = e.g; m.r = e.r;
          m.last_hit = e.last_hit;
          m.state = kMemoValid;
          placed = true;
          break;
        }
      }
    }
    wave_count(placed, counters + kMemoOccupied);
  }
}

}  // namespace ptd
