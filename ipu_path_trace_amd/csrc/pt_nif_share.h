// pt_nif_share.h -- exact sharing of NIF evaluations between queue entries with bit-identical (u, v) (pt_set_nif_sharing).
//
// The NIF output of an escaped path depends on its (u, v) alone: the azimuth is folded in by dir_to_uv and the path's
// throughput is applied after the decode, as one fp32 multiply per channel (the heads of pt_nif.h, pt_nif_gemm.h and
// pt_nif_f32.h: rad_r[path] = bgr[2] * q_tr[qi] ...).  Per batch, between the trace kernel T(b) and the NIF launch N(b):
//
//   S(b)  share_claim_kernel + share_resolve_kernel (trace stream): every entry of the queue T(b) wrote claims its 64-bit
//         key (bits of u : bits of v) in an open-addressed device table.  The entry that claims a key appends (u, v) to
//         the batch's DISTINCT queue; every entry records the index of its owner in the step's BGR store.
//   N(b)  the unmodified NIF kernels in their out_bgr mode (as pt_nif_infer drives them) over the distinct queue.
//   E(b)  share_expand_kernel (accumulate stream, ahead of the accumulate kernel): rad_r[q_path[q]] = bgr_owner[2] * q_tr[q],
//         and likewise for g and b -- the head's own expressions, so every per-path radiance is the per-path mode's bit for bit.
//
// A key that finds no slot within kShareMaxProbes (full table), or that equals the empty marker, takes a distinct-queue
// entry of its own and is counted in `overflowed`: it is evaluated alone, never dropped.
#pragma once

namespace ptd {

constexpr unsigned long long kShareEmpty = ~0ull;     // empty slot: u and v both the all-ones NaN pattern
constexpr uint32_t kShareSlotFlag = 0x80000000u;      // owner[q] holds a table slot still to be resolved (share_resolve_kernel)
constexpr uint32_t kShareMaxProbes = 32;              // linear probes before a key is evaluated alone
constexpr int kShareBlock = 256;

struct ShareParams {
  // queue of escaped paths as the trace kernel wrote it: one region per trace workgroup
  const float* q_u; const float* q_v;
  const uint32_t* region_count;
  uint32_t region_cap;
  // open-addressed table (slot_mask + 1 slots, a power of two <= 2^30): key and store index of its owner
  unsigned long long* keys;
  uint32_t* vals;
  uint32_t slot_mask;
  uint32_t* owner;           // [queue slot]: store index of the entry's owner
  float* d_u; float* d_v;    // the batch's distinct queue (store index base + i)
  uint32_t* d_count;         // the batch's distinct-queue length
  uint32_t base;             // store index of d_u[0]
  unsigned long long* overflowed;
};

struct ExpandParams {
  const uint32_t* region_count;
  uint32_t region_cap;
  const uint32_t* owner;
  const float* bgr;          // the step's BGR store [index][3], written by the NIF kernels' out_bgr mode
  const float* q_tr; const float* q_tg; const float* q_tb;
  const uint32_t* q_path;
  float* rad_r; float* rad_g; float* rad_b;
};

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

// grid (ceil(region_cap / 256), n_regions): x = 256 entries of one region, y = region
__global__ __launch_bounds__(kShareBlock) void share_claim_kernel(ShareParams S) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  const uint32_t count = S.region_count[r];
  if (blockIdx.x * (uint32_t)kShareBlock >= count) return;   // uniform over the workgroup
  const bool valid = local < count;
  const uint32_t q = r * S.region_cap + local;
  bool fresh = false, alone = false;   // fresh: claimed a new key; alone: no slot (evaluated on its own)
  uint32_t slot = 0;
  float u = 0.f, v = 0.f;
  if (valid) {
    u = S.q_u[q]; v = S.q_v[q];
    const unsigned long long key = ((unsigned long long)__float_as_uint(u) << 32) | (unsigned long long)__float_as_uint(v);
    alone = true;
    if (key != kShareEmpty) {
      uint32_t s = share_hash(key) & S.slot_mask;
      for (uint32_t p = 0; p < kShareMaxProbes; ++p, s = (s + 1u) & S.slot_mask) {
        // a plain look first: most entries find their key already there and need no atomic (a stale EMPTY only costs the CAS)
        unsigned long long cur = __hip_atomic_load(&S.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kShareEmpty) cur = atomicCAS(&S.keys[s], kShareEmpty, key);
        if (cur == kShareEmpty) { fresh = true; alone = false; slot = s; break; }
        if (cur == key) { alone = false; slot = s; break; }
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
    if (lane == (uint32_t)leader) first = atomicAdd(S.d_count, (uint32_t)__popcll(m));
    first = __shfl(first, leader, 64);
  }
  if (append) {
    const uint32_t i = first + lane_rank(m);
    S.d_u[i] = u; S.d_v[i] = v;
    const uint32_t g = S.base + i;
    if (fresh) S.vals[slot] = g;
    S.owner[q] = g;
  } else if (valid) {
    S.owner[q] = kShareSlotFlag | slot;   // the key's owner may not have written vals[slot] yet: resolved by the next pass
  }
  const uint64_t om = __ballot(alone);
  if (om && lane == (uint32_t)(__ffsll((long long)om) - 1)) atomicAdd(S.overflowed, (unsigned long long)__popcll(om));
}

// owner[q] = vals[slot] for the entries that found their key claimed by another (every vals[] of the batch is written now)
__global__ __launch_bounds__(kShareBlock) void share_resolve_kernel(ShareParams S) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= S.region_count[r]) return;
  const uint32_t q = r * S.region_cap + local;
  const uint32_t o = S.owner[q];
  if (o & kShareSlotFlag) S.owner[q] = S.vals[o & ~kShareSlotFlag];
}

// the per-path radiance of the NIF heads' per-path mode, from the owner's decoded BGR
__global__ __launch_bounds__(kShareBlock) void share_expand_kernel(ExpandParams E) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= E.region_count[r]) return;
  const uint32_t q = r * E.region_cap + local;
  const float* bgr = E.bgr + 3 * (size_t)E.owner[q];
  const uint32_t path = E.q_path[q];
  E.rad_r[path] = bgr[2] * E.q_tr[q];
  E.rad_g[path] = bgr[1] * E.q_tg[q];
  E.rad_b[path] = bgr[0] * E.q_tb[q];
}

}  // namespace ptd
