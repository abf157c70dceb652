// pt_nif_memo.h -- a persistent device memo of decoded NIF values across steps (pt_set_nif_memo): its slot and the passes that
// are the memo's own.  Included by pt_nif_group.h, whose three passes run over the memo as MemoTable.
//
// The decoded BGR of an escaped path depends on its (u, v) and the uploaded model only (pt_nif_group.h): a value stays valid
// until pt_upload_nif.  With the memo on, the step-scope sharing table is replaced by a table that outlives the step.  One
// 32-byte slot per entry (one cache line per lookup): key, state, last-hit step, the decoded BGR as the NIF kernels' out_bgr
// mode wrote it, and the step-store index of the entry's owner while it is claimed.  Per batch:
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
constexpr uint32_t kMemoNoSlot = 0xffffffffu;     // publish index of a distinct-queue entry that is evaluated alone

struct alignas(32) MemoSlot {
  unsigned long long key;   // bits of u : bits of v, kShareEmpty = free
  uint32_t state;           // kMemoFree, a step stamp (claimed in that step), or kMemoValid
  uint32_t last_hit;        // stamp of the last step that looked the key up
  float b, g, r;            // decoded BGR (valid slots)
  uint32_t idx;             // step-store index of the owner (claimed slots)
};
static_assert(sizeof(MemoSlot) == ptshare::kMemoSlotBytes, "one memo slot = 32 bytes, as pt_set_nif_memo counts them");
static_assert(offsetof(MemoSlot, state) == 8 && offsetof(MemoSlot, last_hit) == 12, "memo_compact_kernel reads them as words 2 and 3");

// counters of the memo passes, cleared at the start of every step (occupied only when the table is cleared)
enum { kMemoOccupied = 0, kMemoServedCount = 1, kMemoInserted = 2, kMemoRetained = 3, kMemoCounters = 4 };

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

// retain pass, 1 of 2: the valid entries hit in step `last` into list[0 .. list_cap); the rest are dropped (a memo may forget).
// A workgroup holds kCompactTrips trips of its grid-stride loop in registers and reserves their places in the list with one
// atomic: with one per wave and trip, the single counter was the pass's time (profiles/r07_nif_memo.txt).  The list stays
// dense (memo_reinsert_kernel reads list[0 .. retained)); the LDS words alternate between two sets, so a wave that is a
// round ahead writes beside what a slower wave still reads.
constexpr uint32_t kCompactTrips = 8;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(kShareBlock) void memo_compact_kernel(const MemoSlot* slots, uint32_t n_slots, uint32_t last,
                                                                   MemoSlot* list, uint32_t list_cap, unsigned long long* counters) {
  constexpr uint32_t W = ptshare::kClaimWaves;
  __shared__ uint32_t s_kept[2][W];
  __shared__ unsigned long long s_first[2];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t stride = (uint64_t)gridDim.x * kShareBlock;
  uint32_t round = 0;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kShareBlock; s0 < n_slots; s0 += stride * kCompactTrips, round ^= 1u) {
    u32x4 lo[kCompactTrips], hi[kCompactTrips];   // the trips' slots as two 16-byte halves: key, state, last_hit | b, g, r, idx
    uint32_t keep = 0, n_kept = 0;                // bit j: trip j's slot stays
#pragma unroll
    for (uint32_t j = 0; j < kCompactTrips; ++j) {
      const uint64_t s = s0 + j * stride + threadIdx.x;
      const u32x4* from = reinterpret_cast<const u32x4*>(slots + (s < n_slots ? s : n_slots - 1u));   // (no branch round the loads)
      lo[j] = from[0]; hi[j] = from[1];
      keep |= (s < n_slots && lo[j].z == kMemoValid && lo[j].w == last ? 1u : 0u) << j;
    }
#pragma unroll
    for (uint32_t j = 0; j < kCompactTrips; ++j) n_kept += (uint32_t)__popcll(__ballot((keep >> j) & 1u));
    if (lane == 0) s_kept[round][wave] = n_kept;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t total = ptshare::claim_wave_offset(s_kept[round], W);
      s_first[round] = total ? atomicAdd(counters + kMemoRetained, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    unsigned long long next = s_first[round] + ptshare::claim_wave_offset(s_kept[round], wave);
#pragma unroll
    for (uint32_t j = 0; j < kCompactTrips; ++j) {
      const uint64_t m = __ballot((keep >> j) & 1u);
      if ((keep >> j) & 1u) {
        const unsigned long long i = next + lane_rank(m);
        if (i < list_cap) { u32x4* to = reinterpret_cast<u32x4*>(list + i); to[0] = lo[j]; to[1] = hi[j]; }
      }
      next += (unsigned long long)__popcll(m);
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
