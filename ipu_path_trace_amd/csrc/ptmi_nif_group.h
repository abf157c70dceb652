// ptmi_nif_group.h -- host side of NIF sharing and the memo (pt_set_nif_sharing, pt_set_nif_memo; kernels: pt_nif_group.h,
// pt_nif_memo.h; arithmetic: ptmi_share_plan.h): the buffers of pt_context::group, the mode a step runs in, the stages S(b) and
// E(b) and the memo's publish pass, the class level of N(b), the entry points and the test build's hooks.  Part of the one translation unit ptmi.hip,
// included there behind `Batch` and ahead of the other stages of a step, which take the StepMode.
#pragma once

static int resolve_stage_times(pt_handle h);   // ptmi.hip

// ---- exact sharing of NIF evaluations: buffers (pt_set_nif_sharing allocates them, a step-scope step with more batches
// than store regions grows the store) and the S / E launches of one batch (pt_nif_group.h)

static uint64_t free_device_bytes() {
  size_t free_b = 0, total_b = 0;
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (uint64_t)free_b : ptshare::kFreeUnknown;
}

// Table capacity: the worst case of the table's scope -- one batch, or every batch of a step (ptmi_share_plan.h: load factor
// <= 1/2 even if every entry is distinct, at most 1/8 of the free device memory and 2^30 slots).  A full table is not an
// error: the keys that find no slot are evaluated alone.
static uint32_t share_table_slots(pt_handle h, uint64_t entries, uint64_t free_b) {
  if (h->group.share_diag_slots) return h->group.share_diag_slots;   // test build: exactly the forced size
  return ptshare::worst_case_slots(entries, free_b);
}

static int ensure_share_counts(pt_handle h, size_t batches) {
  if (batches <= h->group.share_count_cap) return PT_OK;
  h->group.share_count_cap = 0;
  PT_HIP(dev_alloc(h->group.d_share_count, batches));
  PT_HIP(dev_alloc(h->group.h_share_count, batches));
  h->group.share_count_cap = batches;
  return PT_OK;
}

// store regions of queue_cap entries each: (u, v) of the distinct queue and its decoded BGR.  Store indices stay below 2^31.
static int ensure_share_store(pt_handle h, size_t regions) {
  if (regions <= h->group.share_regions) return PT_OK;
  if (regions * h->queue_cap >= ptshare::kMaxStoreEntries)
    return fail(h, PT_ERR_OUT_OF_MEMORY, "NIF sharing: the step's distinct queues would exceed 2^31 entries (fewer samples per step)");
  PT_HIP(hipStreamSynchronize(h->stream));
  h->group.d_share_u.reset(); h->group.d_share_v.reset(); h->group.d_share_bgr.reset();   // all three go before the first comes back: they are large
  h->group.share_regions = 0;
  PT_HIP(dev_alloc(h->group.d_share_u, regions * h->queue_cap));
  PT_HIP(dev_alloc(h->group.d_share_v, regions * h->queue_cap));
  PT_HIP(dev_alloc(h->group.d_share_bgr, 3 * regions * h->queue_cap));
  h->group.share_regions = regions;
  return PT_OK;
}

// The table with exactly `slots` slots, the stream drained first.
static int alloc_share_table(pt_handle h, uint32_t slots) {
  PT_HIP(hipStreamSynchronize(h->stream));
  h->group.d_share_keys.reset(); h->group.d_share_vals.reset();
  h->group.share_slots = 0;
  h->group.share_clean_slots = 0;   // new memory: nothing is known of it
  if (!slots) return PT_OK;
  PT_HIP(dev_alloc(h->group.d_share_keys, slots));
  PT_HIP(dev_alloc(h->group.d_share_vals, slots));
  h->group.share_slots = slots;
  return PT_OK;
}

// (re)allocates the table if its scope needs more slots than it has (never for a capacity forced by the test build)
static int ensure_share_table(pt_handle h, uint64_t entries) {
  const uint32_t slots = share_table_slots(h, entries, free_device_bytes());
  if (h->group.d_share_keys && (slots <= h->group.share_slots || h->group.share_diag_slots)) return PT_OK;
  return alloc_share_table(h, slots);
}

// What sharing and the memo both need besides their table: the owner maps, the overflow counter, counts and a store.
static int alloc_group_buffers(pt_handle h) {
  for (auto& o : h->group.d_share_owner)
    if (!o) PT_HIP(dev_alloc(o, h->queue_cap));
  if (!h->group.d_share_over) {
    PT_HIP(dev_alloc(h->group.d_share_over, 1));
    PT_HIP(dev_alloc(h->group.h_share_over, 1));
  }
  if (int rc = ensure_share_counts(h, 64)) return rc;
  return ensure_share_store(h, pt_context::kBatchSets);   // what batch scope needs: a region per set
}

static int alloc_share_buffers(pt_handle h) {
  if (int rc = ensure_share_table(h, h->queue_cap)) return rc;
  return alloc_group_buffers(h);
}

static void free_share_buffers(pt_handle h) {   // (the counts and the overflow counter are a few bytes: they stay)
  h->group.d_share_keys.reset(); h->group.d_share_vals.reset();
  h->group.share_slots = 0;
  h->group.share_clean_slots = 0;
  h->group.d_share_u.reset(); h->group.d_share_v.reset(); h->group.d_share_bgr.reset();
  h->group.share_regions = 0;
  for (auto& o : h->group.d_share_owner) o.reset();
}

static int ensure_memo_slot_map(pt_handle h);

// The buffers of a grouped step at the step's size (the table's only without the memo, which has its own).
static int ensure_group_buffers(pt_handle h, bool memo, bool step_scope, size_t batches) {
  if (int rc = ensure_share_counts(h, batches)) return rc;
  if (int rc = ensure_share_store(h, step_scope ? batches : pt_context::kBatchSets)) return rc;
  if (memo) return ensure_memo_slot_map(h);
  return ensure_share_table(h, (step_scope ? batches : 1) * (uint64_t)h->queue_cap);
}

// ---- persistent memo of decoded NIF values (pt_set_nif_memo, pt_nif_memo.h): buffers, generations, the per-step passes
static void free_memo_buffers(pt_handle h) {
  h->group.d_memo.reset(); h->group.d_memo_list.reset(); h->group.d_memo_slot.reset(); h->group.d_memo_ctr.reset(); h->group.h_memo_ctr.reset();
  h->group.memo_slots = 0; h->group.memo_slot_regions = 0; h->group.memo_occupied = 0;
}

// every value in the memo is forgotten: the table is cleared before the next lookup
static void memo_new_generation(pt_handle h) {
  h->group.memo_generation += 1;
  h->group.memo_clear = true;
  h->group.memo_occupied = 0;
}

// the publish map follows the step store (one entry per store index)
static int ensure_memo_slot_map(pt_handle h) {
  if (h->group.memo_slot_regions >= h->group.share_regions) return PT_OK;
  PT_HIP(hipStreamSynchronize(h->stream));
  h->group.memo_slot_regions = 0;
  PT_HIP(dev_alloc(h->group.d_memo_slot, h->group.share_regions * h->queue_cap));
  h->group.memo_slot_regions = h->group.share_regions;
  return PT_OK;
}

static int alloc_memo_buffers(pt_handle h, uint32_t slots) {
  PT_HIP(dev_alloc(h->group.d_memo, slots));
  PT_HIP(dev_alloc(h->group.d_memo_list, std::max<size_t>(1, slots / 2)));
  PT_HIP(dev_alloc(h->group.d_memo_ctr, ptd::kMemoCounters));
  PT_HIP(dev_alloc(h->group.h_memo_ctr, ptd::kMemoCounters));
  if (int rc = alloc_group_buffers(h)) return rc;
  return ensure_memo_slot_map(h);
}

// A memo of `slots` slots (a power of two <= 2^30), its retain list and what the step-scope path needs besides the sharing
// table; a failure leaves the memo off (h->error names the failing call).
static int alloc_memo(pt_handle h, uint32_t slots) {
  PT_HIP(hipStreamSynchronize(h->stream));
  free_memo_buffers(h);
  if (int rc = alloc_memo_buffers(h, slots)) { free_memo_buffers(h); return rc; }
  h->group.memo_slots = slots;
  h->group.memo_clear = true;   // cleared on the stream ahead of the first lookup
  return PT_OK;
}

// Memo prologue of a step, on the trace stream ahead of the first lookup: the step's counters, and the table cleared (new
// generation) or thinned out (retain pass: occupancy above 1/2 of the slots after the last step).
static int enqueue_memo_prologue(pt_handle h) {
  hipStream_t s = h->trace_stream;
  PT_HIP(hipMemsetAsync(h->group.d_memo_ctr + ptd::kMemoServedCount, 0, (ptd::kMemoCounters - 1) * 8, s));
  const uint32_t last = h->group.memo_step;
  h->group.memo_step = h->group.memo_step >= ptd::kMemoMaxStamp ? 1u : h->group.memo_step + 1u;
  const size_t table_bytes = (size_t)h->group.memo_slots * sizeof(ptd::MemoSlot);
  if (h->group.memo_clear) {
    PT_HIP(hipMemsetAsync(h->group.d_memo, 0xff, table_bytes, s));
    PT_HIP(hipMemsetAsync(h->group.d_memo_ctr + ptd::kMemoOccupied, 0, 8, s));
    h->group.memo_clear = false;
  } else if (2 * h->group.memo_occupied > h->group.memo_slots) {
    const uint32_t list_cap = std::max<uint32_t>(1, h->group.memo_slots / 2);
    const uint32_t grid = std::min<uint32_t>(ptd::kMemoGrid, (h->group.memo_slots + ptd::kShareBlock - 1) / ptd::kShareBlock);
    hipLaunchKernelGGL(ptd::memo_compact_kernel, dim3(grid), dim3(ptd::kShareBlock), 0, s, h->group.d_memo, h->group.memo_slots, last,
                       h->group.d_memo_list, list_cap, h->group.d_memo_ctr);
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemsetAsync(h->group.d_memo, 0xff, table_bytes, s));
    PT_HIP(hipMemsetAsync(h->group.d_memo_ctr + ptd::kMemoOccupied, 0, 8, s));
    const uint32_t rgrid = std::min<uint32_t>(ptd::kMemoGrid, (list_cap + ptd::kShareBlock - 1) / ptd::kShareBlock);
    hipLaunchKernelGGL(ptd::memo_reinsert_kernel, dim3(rgrid), dim3(ptd::kShareBlock), 0, s, h->group.d_memo, h->group.memo_slots - 1u,
                       h->group.d_memo_list, list_cap, h->group.d_memo_ctr);
    PT_HIP(hipGetLastError());
    h->group.memo_retains += 1;
  }
  return PT_OK;
}

// ---- the mode of a step and its stages S(b), E(b) and the memo's publish pass (schedule: ptmi.hip, "one step")
// NIF sharing (off: S and E do not run, and the step is exactly the unshared one) puts S(b) behind T(b) and E(b) ahead of
// A(b).  Batch scope: the distinct queue of batch b in the store region of its buffer set, b mod depth
// (ptmi_step_plan.h: store_region).  N(b + depth) writes region b mod depth only after A(b), hence E(b), has read it: N(b + depth)
// is behind S(b + depth), that behind T(b + depth), and T(b + depth) waits for the set's B.accumulated, which A(b) recorded.
// The same chain keeps the set's owner map, which S(b + depth) rewrites, for E(b).  Step scope: region b, every batch's
// results live until the step ends.  The memo
// (pt_set_nif_memo) replaces the sharing table whatever the sharing mode: keys it does not hold are shared at step scope,
// through the same store.
struct StepMode {
  int32_t share;   // sharing mode in force (off for a constant environment)
  bool memo;
  bool classes = false;   // N(b) evaluates a row per class of its distinct queue (prepare_class_level)
  // the class is claimed inside S(b) and E(b) gathers from the class store (pt_nif_group.h: ShareClassTable): a step-scope step
  // with the class level and without the memo, whose publish pass reads the raw BGR store.  Batch scope keeps the level's own
  // passes in N(b) as the memo does: its tables forget a pair from batch to batch, so 2.5 times as many entries append, and
  // their class lookups on the trace stream cost it more than the NIF stream saves (profiles/r29_class_in_claim.txt)
  bool fused() const { return classes && !memo && share == PT_NIF_SHARE_STEP; }
  // a fused step that indexes its classes in the class map (prepare_class_level; pt_nif_group.h: ClassMap): S(b) is C(b), the
  // class claim alone; the raw-pair pass R(b) runs behind A(b) on the accumulate stream, off the step's critical path; E(b) follows a
  // pending class word itself and no resolve pass runs; the step ends with the release of the words it took
  bool mapped = false;
  // a mapped step over a worklist of a multiple of four items: no E(b); the trace kernels write the inverse slot map and A(b)
  // forms the escaped paths' radiance itself (pt_nif_group.h: accumulate_mapped_kernel).  Other worklists keep E(b) + A(b).
  bool expand_in_accumulate = false;
  bool grouped() const { return share || memo; }   // N runs over distinct queues in the step store
  bool step_scope() const { return memo || share == PT_NIF_SHARE_STEP; }
  ptshare::StepKind kind() const {   // what the step does to the sharing table (ptmi_share_plan.h: the clean-table hand-off)
    return memo ? ptshare::StepKind::kMemo : share == PT_NIF_SHARE_STEP ? ptshare::StepKind::kStep
           : share == PT_NIF_SHARE_BATCH ? ptshare::StepKind::kBatch : ptshare::StepKind::kOff;
  }
};

// The mode of a handle on which neither pt_set_nif_sharing nor pt_set_nif_memo was ever called: step scope if the environment
// is a NIF, the memo is off and what the step would allocate fits the budget of ptmi_share_plan.h (a quarter of the free
// device memory); otherwise, and if an allocation fails all the same, off -- exactly the unshared step, and no error.
// Buffers the handle already holds (an earlier step, the test build's forced capacity) count as held.
static int32_t auto_share_mode(pt_handle h, size_t batches) {
  if (h->env_const || h->env_map || h->group.memo_slots || h->group.share_auto_failed) return PT_NIF_SHARE_OFF;   // (memo_slots: the test build's hook; pt_set_nif_memo ends the choice)
  const uint64_t free_b = free_device_bytes();
  const uint64_t slots = share_table_slots(h, batches * (uint64_t)h->queue_cap, free_b);
  ptshare::Held held;
  held.table_slots = h->group.d_share_keys ? (h->group.share_diag_slots ? slots : h->group.share_slots) : 0;
  held.store_regions = h->group.share_regions;
  for (const auto& o : h->group.d_share_owner) held.owner_maps += o ? 1 : 0;
  if (!ptshare::auto_fits(slots, batches, h->queue_cap, held, free_b, pt_context::kBatchSets)) return PT_NIF_SHARE_OFF;
  if (ensure_group_buffers(h, false, true, batches) == PT_OK && alloc_group_buffers(h) == PT_OK) return PT_NIF_SHARE_STEP;   // (the step's sizes first: nothing is allocated twice)
  (void)hipGetLastError();   // an allocation failed: give back what was taken and run unshared from now on
  free_share_buffers(h);
  h->group.share_auto_failed = true;
  h->error.clear();
  return PT_NIF_SHARE_OFF;
}

// Before the first batch of a grouped step: the buffers at the step's size, and the counts, the overflow counter and a
// step-scope table cleared on the trace stream, where S runs (after e_begin: part of the step) -- unless the step before
// handed the table over clean (enqueue_table_handoff; the mark is checked after the buffers have their size).
static int prepare_group_store(pt_handle h, const StepMode& mode, size_t batches) {
  if (int rc = ensure_group_buffers(h, mode.memo, mode.step_scope(), batches)) return rc;
  PT_HIP(hipMemsetAsync(h->group.d_share_count, 0, batches * 4, h->trace_stream));
  PT_HIP(hipMemsetAsync(h->group.d_share_over, 0, 8, h->trace_stream));
  if (mode.kind() == ptshare::StepKind::kStep &&   // one table for the step
      !ptshare::clear_skippable(h->group.share_clean_slots, mode.kind(), h->group.share_slots))
    PT_HIP(hipMemsetAsync(h->group.d_share_keys, 0xff, (size_t)h->group.share_slots * 8, h->trace_stream));
  return PT_OK;
}

// ---- the class level of N(b) (pt_nif_group.h: ClassTable; sizes: ptmi_share_plan.h).  All of it runs on the NIF stream.
static void free_class_buffers(pt_handle h) {
  h->group.d_class_keys.reset(); h->group.d_class_vals.reset();
  h->group.class_slots = 0;
  h->group.d_class_u.reset(); h->group.d_class_v.reset(); h->group.d_class_bgr.reset();
  h->group.class_regions = 0;
  h->group.d_class_owner.reset();
  h->group.d_class_map.reset(); h->group.d_class_tail_keys.reset();
  h->group.class_tail_slots = 0;
  h->group.class_map_clean = false;
}

// The class map and its tail (ptmi_share_plan.h), the stream drained first.  New memory: nothing is known of it.
static int alloc_class_map(pt_handle h, uint32_t tail_slots) {
  PT_HIP(hipStreamSynchronize(h->stream));
  h->group.d_class_map.reset(); h->group.d_class_tail_keys.reset();
  h->group.class_tail_slots = 0;
  h->group.class_map_clean = false;
  PT_HIP(dev_alloc(h->group.d_class_map, (size_t)ptshare::kClassMapWords + tail_slots));
  PT_HIP(dev_alloc(h->group.d_class_tail_keys, tail_slots));
  h->group.class_tail_slots = tail_slots;
  return PT_OK;
}

// (slots = 0: a mapped step, which needs no hashed table -- one it holds stays)
static int alloc_class_buffers(pt_handle h, uint32_t slots, size_t batches) {
  PT_HIP(hipStreamSynchronize(h->stream));
  if (!slots) {
  } else if (!h->group.d_class_keys || (h->group.class_diag_slots ? slots != h->group.class_slots : slots > h->group.class_slots)) {
    h->group.d_class_keys.reset(); h->group.d_class_vals.reset();
    h->group.class_slots = 0;
    PT_HIP(dev_alloc(h->group.d_class_keys, slots));
    PT_HIP(dev_alloc(h->group.d_class_vals, slots));
    h->group.class_slots = slots;
  }
  if (batches > h->group.class_regions) {
    h->group.d_class_u.reset(); h->group.d_class_v.reset(); h->group.d_class_bgr.reset();
    h->group.class_regions = 0;
    PT_HIP(dev_alloc(h->group.d_class_u, batches * h->queue_cap));
    PT_HIP(dev_alloc(h->group.d_class_v, batches * h->queue_cap));
    PT_HIP(dev_alloc(h->group.d_class_bgr, 3 * batches * h->queue_cap));
    h->group.class_regions = batches;
  }
  if (!h->group.d_class_owner) PT_HIP(dev_alloc(h->group.d_class_owner, h->queue_cap));
  if (!h->group.d_class_over) {
    PT_HIP(dev_alloc(h->group.d_class_over, 1));
    PT_HIP(dev_alloc(h->group.h_class_over, 1));
  }
  if (batches > h->group.class_count_cap) {
    h->group.class_count_cap = 0;
    PT_HIP(dev_alloc(h->group.d_class_count, batches));
    PT_HIP(dev_alloc(h->group.h_class_count, batches));
    h->group.class_count_cap = batches;
  }
  return PT_OK;
}

// Before the first batch of a grouped step, behind prepare_group_store (the sharing buffers come first): whether the step
// runs the class level -- the environment is a NIF, and the level's buffers at the step's size are held or fit the budget
// (ptshare::class_fits) and could be allocated -- and, if it does, the table, the counts and the alone counter cleared on the
// NIF stream, where they overlap T(0).  Declining is no error: the step is then the one without the level.  In a fused step
// the first to touch what is cleared here is S(0), on the trace stream: `cleared` is recorded behind the clears, and
// stage_group makes the trace stream wait for it ahead of S(0) -- not ahead of T(0), which the clears still overlap.  Every
// other step touches them on the NIF stream alone and records no event.
static int prepare_class_level(pt_handle h, StepEvents& ev, size_t batches, StepMode& mode, hipEvent_t& cleared) {
  bool& classes = mode.classes;
  classes = false;
  if (h->env_map || h->group.class_failed) return PT_OK;
  const uint64_t free_b = free_device_bytes();
  ptshare::ClassHeld held;
  held.store_regions = h->group.class_regions;
  held.owner_maps = h->group.d_class_owner ? 1 : 0;
  // the class map: a step-scope step without the memo and without a capacity the test build forced on either table, if the map is
  // held or fits together with the class store the step is about to take; such a step needs no hashed class table
  const bool mapped = mode.share == PT_NIF_SHARE_STEP && !mode.memo && !h->group.class_diag_slots && !h->group.share_diag_slots &&
                      !h->group.class_map_failed &&
                      ptshare::class_map_fits(h->group.class_tail_slots != 0, ptshare::kClassTailSlots, free_b,
                                              ptshare::class_bytes(0, batches, h->queue_cap, held));
  const uint32_t slots = mapped ? 0u : h->group.class_diag_slots ? h->group.class_diag_slots : ptshare::class_slots(batches * (uint64_t)h->queue_cap, free_b);
  held.table_slots = h->group.d_class_keys ? (h->group.class_diag_slots ? (h->group.class_slots == slots ? slots : 0) : h->group.class_slots) : 0;
  if (!ptshare::class_fits(slots, batches, h->queue_cap, held, free_b)) return PT_OK;
  if (alloc_class_buffers(h, slots, batches) != PT_OK) {   // give back what was taken and run without the level from now on
    (void)hipGetLastError();
    free_class_buffers(h);
    h->group.class_failed = true;
    h->error.clear();
    return PT_OK;
  }
  if (mapped && !h->group.class_tail_slots && alloc_class_map(h, ptshare::kClassTailSlots) != PT_OK) {   // the hashed table from now on
    (void)hipGetLastError();
    h->group.d_class_map.reset(); h->group.d_class_tail_keys.reset();
    h->group.class_map_failed = true;
    h->error.clear();
    return prepare_class_level(h, ev, batches, mode, cleared);
  }
  if (mapped) {
    if (!ptshare::map_clear_skippable(h->group.class_map_clean)) {   // the first step on this map, or the one behind a failed step
      PT_HIP(hipMemsetAsync(h->group.d_class_map, 0xff, ((size_t)ptshare::kClassMapWords + h->group.class_tail_slots) * 4, h->stream));
      PT_HIP(hipMemsetAsync(h->group.d_class_tail_keys, 0xff, (size_t)h->group.class_tail_slots * 8, h->stream));
    }
    mode.mapped = h->group.class_map_ran = true;
  } else {
    PT_HIP(hipMemsetAsync(h->group.d_class_keys, 0xff, (size_t)h->group.class_slots * 8, h->stream));
  }
  PT_HIP(hipMemsetAsync(h->group.d_class_count, 0, batches * 4, h->stream));
  PT_HIP(hipMemsetAsync(h->group.d_class_over, 0, 8, h->stream));
  classes = true;
  if (!mode.fused()) return PT_OK;
  size_t at = 0;
  return ev.record(h->stream, cleared, at);
}

static ptd::ClassTable class_table(pt_handle h) { return {{h->group.d_class_keys, h->group.d_class_vals, h->group.class_slots - 1u}}; }

// The head of N(b) with the class level: claim and resolve over the batch's distinct queue, one region whose count S(b) left
// on the device.  An entry that claims a class appends its own (u, v) to the batch's class queue (class region b).
static int stage_class_claim(pt_handle h, StepEvents& ev, const Batch& b) {
  return ev.timed(h->stream, pt_context::kSpanClass, [&]() -> int {
    ptd::GroupQueue Q;
    Q.q_u = h->group.d_share_u + b.store_base; Q.q_v = h->group.d_share_v + b.store_base;
    Q.region_count = h->group.d_share_count + b.index;
    Q.region_cap = b.store_cap;
    Q.owner = h->group.d_class_owner;
    Q.d_u = h->group.d_class_u + b.class_base; Q.d_v = h->group.d_class_v + b.class_base;
    Q.d_count = h->group.d_class_count + b.index;
    Q.base = b.class_base;
    Q.overflowed = h->group.d_class_over;
    const dim3 tiles(ptshare::claim_tiles(b.store_cap), 1), grid((b.store_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock, 1), block(ptd::kShareBlock);
    hipLaunchKernelGGL(ptd::class_claim_kernel, tiles, block, 0, h->stream, Q, class_table(h));
    PT_HIP(hipGetLastError());
    hipLaunchKernelGGL(ptd::class_resolve_kernel, grid, block, 0, h->stream, Q, class_table(h));
    PT_HIP(hipGetLastError());
    return PT_OK;
  });
}

// ... and its tail: every entry of the distinct queue gets the BGR of its class owner, into the step store.
static int stage_class_spread(pt_handle h, StepEvents& ev, const Batch& b, hipEvent_t* done) {
  return ev.timed(h->stream, pt_context::kSpanClass, [&]() -> int {
    const uint32_t grid = std::min<uint32_t>(ptd::kMemoGrid, (b.store_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock);
    hipLaunchKernelGGL(ptd::class_spread_kernel, dim3(grid), dim3(ptd::kShareBlock), 0, h->stream, h->group.d_share_count + b.index,
                       h->group.d_class_owner, h->group.d_class_bgr, h->group.d_share_bgr + 3 * (size_t)b.store_base);
    PT_HIP(hipGetLastError());
    return PT_OK;
  }, done);
}

// Behind the last S(b) of a step-scope step, which is the table's last reader: the clear for the NEXT step, on the trace
// stream, where it runs beside the last NIF launches instead of ahead of the next step's T(0).  `clean` is recorded behind
// it; the step's end waits for it, and pt_path_trace sets the mark (ptshare::mark_after_step) once the step has returned.
// A mapped step's last reader of the table is R(b) of its last batch, on the accumulate stream: the clear follows it there.
// (The last R(b) and the clear on the trace stream, behind C(b), lost an alternating A/B: profiles/r34_expand_in_accumulate.txt.)
static int enqueue_table_handoff(pt_handle h, StepEvents& ev, hipEvent_t& clean, hipStream_t s) {
  PT_HIP(hipMemsetAsync(h->group.d_share_keys, 0xff, (size_t)h->group.share_slots * 8, s));
  size_t at = 0;
  return ev.record(s, clean, at);
}

static ptd::ShareTable share_table(pt_handle h) { return {h->group.d_share_keys, h->group.d_share_vals, h->group.share_slots - 1u}; }
// the fused step's table for batch b: the raw table, the step's class table and the batch's class queue (class region b)
static ptd::ShareClassTable share_class_table(pt_handle h, const Batch& b) {
  ptd::ShareClassTable T;
  static_cast<ptd::ShareTable&>(T) = share_table(h);
  T.classes = class_table(h);
  T.c_u = h->group.d_class_u + b.class_base; T.c_v = h->group.d_class_v + b.class_base;
  T.c_count = h->group.d_class_count + b.index;
  T.c_base = b.class_base;
  T.c_alone = h->group.d_class_over;
  return T;
}
// the mapped step's class map for batch b: the map, the tail and the batch's class queue (class region b)
static ptd::ClassMap class_map(pt_handle h, const Batch& b) {
  ptd::ClassMap M;
  M.words = h->group.d_class_map;
  M.tail_keys = h->group.d_class_tail_keys;
  M.tail_mask = h->group.class_tail_slots - 1u;
  M.c_u = h->group.d_class_u + b.class_base; M.c_v = h->group.d_class_v + b.class_base;
  M.c_count = h->group.d_class_count + b.index;
  M.c_base = b.class_base;
  M.c_alone = h->group.d_class_over;
  return M;
}
static ptd::MemoTable memo_table(pt_handle h) {
  return {h->group.d_memo, h->group.memo_slots - 1u, h->group.memo_step, h->group.d_memo_slot, h->group.d_memo_ctr};
}

// The batch's queue, its owner map and its distinct queue in the store, as claim and resolve take them.
static ptd::GroupQueue group_queue(pt_handle h, const Batch& b) {
  ptd::GroupQueue Q;
  Q.q_u = b.B->q_u; Q.q_v = b.B->q_v;
  Q.region_count = b.B->region_count;
  Q.region_cap = b.g.region_cap;
  Q.owner = h->group.d_share_owner[b.set()];
  Q.d_u = h->group.d_share_u + b.store_base; Q.d_v = h->group.d_share_v + b.store_base;
  Q.d_count = h->group.d_share_count + b.index;
  Q.base = b.store_base;
  Q.overflowed = h->group.d_share_over;
  return Q;
}

// The resolve pass of S(b) on stream `s`: the owners claimed in this step get their store index.
static int stage_resolve(pt_handle h, StepEvents& ev, const StepMode& mode, const Batch& b, hipStream_t s) {
  return ev.timed(s, mode.memo ? pt_context::kSpanMemo : pt_context::kSpanShare, [&]() -> int {
    const ptd::GroupQueue Q = group_queue(h, b);
    if (mode.memo) hipLaunchKernelGGL(ptd::memo_resolve_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, s, Q, memo_table(h));
    else if (mode.fused()) hipLaunchKernelGGL(ptd::share_class_resolve_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, s, Q, share_class_table(h, b));
    else hipLaunchKernelGGL(ptd::share_resolve_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, s, Q, share_table(h));
    PT_HIP(hipGetLastError());
    return PT_OK;
  });
}

// Since the class level the NIF stream has room and the trace stream is what a step waits for (profiles/r28_nif_classes.txt),
// so a step-scope step (the memo included) resolves at the head of N(b), on the NIF stream.  Nothing on the trace stream
// writes what the pass reads: claims of later batches write the value of slots they claim fresh, the pass reads the values
// of slots claimed up to its own batch, and the table's clears touch the keys alone.  Batch scope reuses its table from batch
// to batch and resolves where it claims.  The fused step's two-hop resolve stands on the same argument, for both tables: a
// claim writes the value of a raw or a class slot only if it claimed the slot fresh, every slot the pass reaches (a raw slot
// through an owner word, a class slot through a pending class word) was claimed up to its own batch, and both tables' clears
// touch keys alone.  Its write-back stores into raw slots claimed up to its own batch, which no claim writes again; the only
// other readers and writers of those values are resolve passes, which follow each other on one stream.
static bool resolve_on_nif_stream(const StepMode& mode) { return mode.step_scope(); }

// S(b), right behind T(b) (it hides under N(b - 1) as T(b) does): claim a slot per key -- in the sharing table, or with the
// memo look the key up -- then (batch scope) resolve the owners claimed in this batch.
static int stage_group(pt_handle h, StepEvents& ev, const StepMode& mode, const Batch& b, hipEvent_t class_cleared) {
  if (mode.fused() && b.index == 0) PT_HIP(hipStreamWaitEvent(h->trace_stream, class_cleared, 0));   // prepare_class_level's clears
  if (int rc = ev.timed(h->trace_stream, mode.memo ? pt_context::kSpanMemo : pt_context::kSpanShare, [&]() -> int {
        const ptd::GroupQueue Q = group_queue(h, b);
        const dim3 tiles = b.claim_grid(), block(ptd::kShareBlock);
        if (mode.memo) {
          hipLaunchKernelGGL(ptd::memo_lookup_kernel, tiles, block, 0, h->trace_stream, Q, memo_table(h));
        } else {
          if (mode.share == PT_NIF_SHARE_BATCH)   // one table per batch
            PT_HIP(hipMemsetAsync(h->group.d_share_keys, 0xff, (size_t)h->group.share_slots * 8, h->trace_stream));
          if (mode.mapped) hipLaunchKernelGGL(ptd::class_map_claim_kernel, tiles, block, 0, h->trace_stream, Q, class_map(h, b));   // C(b)
          else if (mode.fused()) hipLaunchKernelGGL(ptd::share_class_claim_kernel, tiles, block, 0, h->trace_stream, Q, share_class_table(h, b));
          else hipLaunchKernelGGL(ptd::share_claim_kernel, tiles, block, 0, h->trace_stream, Q, share_table(h));
        }
        PT_HIP(hipGetLastError());
        return PT_OK;
      })) return rc;
  return resolve_on_nif_stream(mode) ? PT_OK : stage_resolve(h, ev, mode, b, h->trace_stream);
}

// E(b), ahead of A(b) (it overlaps N(b + 1) as A(b) does): per-path radiance from the owners' BGR in the step store, or with
// the memo from the memo slot.
static int stage_expand(pt_handle h, StepEvents& ev, const StepMode& mode, const Batch& b) {
  return ev.timed(h->acc_stream, mode.memo ? pt_context::kSpanMemo : pt_context::kSpanShare, [&]() -> int {
    const pt_context::BatchBuffers& B = *b.B;
    ptd::GroupExpand X;
    X.region_count = B.region_count;
    X.region_cap = b.g.region_cap;
    X.owner = h->group.d_share_owner[b.set()];
    X.bgr = mode.fused() ? h->group.d_class_bgr : h->group.d_share_bgr;   // (fused: the owner words are class-store indices)
    X.q_tr = B.q_tr; X.q_tg = B.q_tg; X.q_tb = B.q_tb; X.q_path = B.q_path;
    X.rad_r = B.rad_r; X.rad_g = B.rad_g; X.rad_b = B.rad_b;
    if (mode.memo) hipLaunchKernelGGL(ptd::memo_expand_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, h->acc_stream, X, memo_table(h));
    else if (mode.mapped) hipLaunchKernelGGL(ptd::class_map_expand_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, h->acc_stream, X, class_map(h, b));
    else if (mode.fused()) hipLaunchKernelGGL(ptd::share_class_expand_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, h->acc_stream, X, share_class_table(h, b));
    else hipLaunchKernelGGL(ptd::share_expand_kernel, b.group_grid(), dim3(ptd::kShareBlock), 0, h->acc_stream, X, share_table(h));
    PT_HIP(hipGetLastError());
    h->group.expand_launches += 1;
    return PT_OK;
  });
}

// R(b) of a mapped step, behind A(b) on the accumulate stream: the raw pairs of the batch's queue, claimed and counted in the raw
// table (pt_nif_group.h: RawCountTable).  Nothing in the step reads what it leaves -- the distinct queue and the counts are for
// the statistics and pt_calibrate_nif -- so the trace stream does not carry it; but it reads the set's q_u / q_v, which
// T(b + depth) rewrites: the set's raw_read is recorded behind it, and T(b + depth) waits for that as for B.accumulated (which
// A(b) has recorded ahead of it: R(b) holds back no one who waits for the accumulated film alone).  Behind N(b) on the NIF stream
// the pass made that stream the busiest of the three (97.9 % of a step) and a step 3.7 % longer (profiles/r32_class_map.txt).
static int stage_raw_pairs(pt_handle h, StepEvents& ev, const Batch& b) {
  if (int rc = ev.timed(h->acc_stream, pt_context::kSpanShare, [&]() -> int {
        hipLaunchKernelGGL(ptd::share_raw_claim_kernel, b.claim_grid(), dim3(ptd::kShareBlock), 0, h->acc_stream, group_queue(h, b),
                           ptd::RawCountTable{share_table(h)});
        PT_HIP(hipGetLastError());
        return PT_OK;
      })) return rc;
  PT_HIP(hipEventRecord(b.B->raw_read, h->acc_stream));
  return PT_OK;
}

// The end of a mapped step, on the accumulate stream behind the last A(b): the words of the step's class rows go back to
// kMapEmpty (counts on the device), and the tail is cleared, in one launch.  pt_path_trace sets the mark once the step has returned.
static int stage_map_release(pt_handle h, StepEvents& ev, uint32_t store_cap, uint32_t batches) {
  return ev.timed(h->acc_stream, pt_context::kSpanShare, [&]() -> int {
    const dim3 grid(std::min<uint32_t>(ptd::kMemoGrid, (store_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock), batches);
    hipLaunchKernelGGL(ptd::class_map_release_kernel, grid, dim3(ptd::kShareBlock), 0, h->acc_stream, h->group.d_class_u, h->group.d_class_v,
                       h->group.d_class_count, (uint32_t)h->queue_cap, h->group.d_class_map, h->group.d_class_tail_keys, h->group.class_tail_slots);
    PT_HIP(hipGetLastError());
    return PT_OK;
  });
}

// The memo's publish pass on `stream`: after every N(b) (same stream) and every E(b) (the caller has made `stream` wait for
// the accumulate stream), so no lookup or expand reads what it writes.  store_cap: the largest distinct-queue bound of the step.
static int stage_memo_publish(pt_handle h, StepEvents& ev, uint32_t store_cap, uint32_t batches) {
  return ev.timed(h->stream, pt_context::kSpanMemo, [&]() -> int {
    const dim3 grid(std::min<uint32_t>(ptd::kMemoGrid, (store_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock), batches);
    hipLaunchKernelGGL(ptd::memo_publish_kernel, grid, dim3(ptd::kShareBlock), 0, h->stream, h->group.d_memo, h->group.d_memo_slot,
                       h->group.d_share_bgr, h->group.d_share_count, (uint32_t)h->queue_cap, h->group.memo_step);
    PT_HIP(hipGetLastError());
    return PT_OK;
  });
}

extern "C" {

int pt_set_nif_sharing(pt_handle h, int32_t mode) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (mode != PT_NIF_SHARE_OFF && mode != PT_NIF_SHARE_BATCH && mode != PT_NIF_SHARE_STEP)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_set_nif_sharing: mode must be PT_NIF_SHARE_OFF, _BATCH or _STEP");
  if (mode != PT_NIF_SHARE_OFF) {
    PT_HIP(hipSetDevice(h->cfg.device));
    if (int rc = alloc_share_buffers(h)) { h->group.share_mode = PT_NIF_SHARE_OFF; h->group.share_mode_set = true; return rc; }
  }
  h->group.share_mode = mode;
  h->group.share_mode_set = true;
  return PT_OK;
}

int pt_get_nif_sharing_stats(pt_handle h, pt_nif_sharing_stats* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!out || out->struct_size != sizeof(pt_nif_sharing_stats)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_sharing_stats.struct_size mismatch");
  if (int rc = resolve_stage_times(h)) return rc;
  out->mode = h->group.share_mode_last;
  out->escaped = h->stats.escaped;
  out->evaluations = h->group.share_evals;
  out->overflowed = h->group.share_overflowed;
  out->table_slots = h->group.share_mode_last && !h->group.memo_ran ? h->group.share_slots : 0;
  out->share_ms = h->group.share_ms;
  return PT_OK;
}

int pt_get_nif_class_stats(pt_handle h, pt_nif_class_stats* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!out || out->struct_size != sizeof(pt_nif_class_stats)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_class_stats.struct_size mismatch");
  if (int rc = resolve_stage_times(h)) return rc;
  out->ran = h->group.class_ran;
  out->mlp_rows = h->group.class_ran ? h->group.class_rows : h->group.share_evals;
  out->alone = h->group.class_ran ? h->group.class_alone : 0;
  out->table_slots = !h->group.class_ran ? 0 : h->group.class_map_ran ? ptshare::kClassMapWords + h->group.class_tail_slots : h->group.class_slots;
  out->class_ms = h->group.class_ms;
  return PT_OK;
}

int pt_set_nif_memo(pt_handle h, uint64_t max_bytes) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  PT_HIP(hipSetDevice(h->cfg.device));
  if (max_bytes == 0) {
    PT_HIP(hipStreamSynchronize(h->stream));
    free_memo_buffers(h);
    h->group.share_mode_set = true;   // a caller that manages the memo has chosen: the sharing mode is what pt_set_nif_sharing said (off)
    return PT_OK;
  }
  const uint64_t slots = ptshare::memo_slots_for(max_bytes);   // table + retain list = 48 bytes per slot
  if (!slots)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_set_nif_memo: max_bytes must be 0 or at least 48 KiB (1024 slots of 48 bytes)");
  h->group.share_mode_set = true;   // as above: with or without the memo, this handle no longer chooses its sharing mode itself
  if (slots == h->group.memo_slots) return PT_OK;   // same capacity: the entries stay
  return alloc_memo(h, (uint32_t)slots);
}

int pt_clear_nif_memo(pt_handle h) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  memo_new_generation(h);
  return PT_OK;
}

int pt_get_nif_memo_stats(pt_handle h, pt_nif_memo_stats* out) {
  if (!h) return PT_ERR_INVALID_ARGUMENT;
  if (!out || out->struct_size != sizeof(pt_nif_memo_stats)) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_nif_memo_stats.struct_size mismatch");
  if (int rc = resolve_stage_times(h)) return rc;
  out->enabled = h->group.memo_slots != 0;
  out->slots = h->group.memo_slots;
  out->occupied = h->group.memo_slots ? h->group.memo_occupied : 0;
  out->escaped = h->stats.escaped;
  out->served = h->group.memo_ran ? h->group.memo_served : 0;
  out->evaluations = h->group.share_evals;
  out->inserted = h->group.memo_ran ? h->group.memo_inserted : 0;
  out->overflowed = h->group.memo_ran ? h->group.share_overflowed : 0;
  out->generation = h->group.memo_generation;
  out->retains = h->group.memo_retains;
  out->memo_ms = h->group.memo_ms;
  return PT_OK;
}

#ifdef PTMI_DIAG_BUILD
// test build only: the NIF-sharing table gets `slots` slots (rounded up to a power of two; 0 = sized from memory again), so that
// a test reaches the overflow path with a small image
int pt_diag_set_nif_share_capacity(pt_handle h, uint32_t slots) {
  if (!h || slots > ptshare::kMaxSlots) return PT_ERR_INVALID_ARGUMENT;
  PT_HIP(hipSetDevice(h->cfg.device));
  h->group.share_diag_slots = 0;
  uint32_t p = slots ? 1 : 0;   // exactly the forced size (the sizing rule's minimum and memory bound do not apply)
  while (p < slots) p <<= 1;
  if (int rc = alloc_share_table(h, p)) return rc;
  h->group.share_diag_slots = p;
  if (int rc = alloc_share_buffers(h)) { h->group.share_mode = PT_NIF_SHARE_OFF; return rc; }
  return PT_OK;
}

// test build only: the NIF memo gets exactly `slots` slots (rounded up to a power of two, at least 2), whatever pt_set_nif_memo
// would size, so that a test reaches the overflow and retain paths with a small image; 0 turns the memo off
int pt_diag_set_nif_memo_slots(pt_handle h, uint32_t slots) {
  if (!h || slots > ptshare::kMaxSlots) return PT_ERR_INVALID_ARGUMENT;
  PT_HIP(hipSetDevice(h->cfg.device));
  if (slots == 0) return pt_set_nif_memo(h, 0);
  uint32_t p = 2;
  while (p < slots) p <<= 1;
  return alloc_memo(h, p);
}

// test build only: the claim and resolve passes over a queue the caller supplies, with buffers of its own (the handle gives
// the device and the stream; nothing of its sharing state is touched).  u, v: [n_regions x region_cap] as the trace kernel
// lays its queue out; region_count[r] <= region_cap entries of region r are live.  memo = 0: a ShareTable of table_slots
// slots (a power of two).  memo = 2: the same table through the raw-pair pass of a mapped step (RawCountTable), which leaves the
// owner map as it was filled, 0xff in every byte, and runs no resolve.  memo = 1: a MemoTable, `passes` times (1 or 2) over the same queue with a publish of zeros between
// them, as two steps would run; the outputs are the last pass's.  Out, on the host: owner [n_regions x region_cap] (live
// entries), the distinct queue d_u / d_v (same capacity; store index = position), its length, the overflow count, the memo's
// four counters (memo = 1; may be null) and the table's keys [table_slots] (may be null).
int pt_diag_claim_resolve(pt_handle h, int32_t memo, uint32_t passes, const float* u, const float* v, const uint32_t* region_count,
                          uint32_t n_regions, uint32_t region_cap, uint32_t table_slots, uint32_t* owner, float* d_u, float* d_v,
                          uint32_t* d_count, uint64_t* overflowed, uint64_t* memo_counters, uint64_t* table_keys) {
  if (!h || !u || !v || !region_count || !owner || !d_u || !d_v || !d_count || !overflowed) return PT_ERR_INVALID_ARGUMENT;
  const uint64_t n64 = (uint64_t)n_regions * region_cap;
  if (n_regions == 0 || region_cap == 0 || n64 >= ptshare::kMaxStoreEntries || table_slots < 2 || table_slots > ptshare::kMaxSlots ||
      (table_slots & (table_slots - 1u)) || passes < 1 || passes > (memo == 1 ? 2u : 1u) || memo < 0 || memo > 2)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_claim_resolve: sizes out of range");
  for (uint32_t r = 0; r < n_regions; ++r)
    if (region_count[r] > region_cap) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_claim_resolve: a region's count exceeds its capacity");
  const size_t n = (size_t)n64;
  PT_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  DevBuf<float> q_u, q_v, du, dv, bgr;
  DevBuf<uint32_t> counts, own, len, vals, d_slot;
  DevBuf<unsigned long long> over, keys, ctr;
  DevBuf<ptd::MemoSlot> slots;
  PT_HIP(dev_alloc(q_u, n)); PT_HIP(dev_alloc(q_v, n)); PT_HIP(dev_alloc(du, n)); PT_HIP(dev_alloc(dv, n));
  PT_HIP(dev_alloc(counts, n_regions)); PT_HIP(dev_alloc(own, n)); PT_HIP(dev_alloc(len, 1)); PT_HIP(dev_alloc(over, 1));
  PT_HIP(hipMemcpyAsync(q_u, u, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(q_v, v, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(counts, region_count, (size_t)n_regions * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemsetAsync(own, 0xff, n * 4, s));   // an entry no pass writes reads as pending
  PT_HIP(hipMemsetAsync(over, 0, 8, s));
  ptd::GroupQueue Q;
  Q.q_u = q_u; Q.q_v = q_v; Q.region_count = counts; Q.region_cap = region_cap; Q.owner = own;
  Q.d_u = du; Q.d_v = dv; Q.d_count = len; Q.base = 0; Q.overflowed = over;
  const dim3 grid((region_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock, n_regions), tiles(ptshare::claim_tiles(region_cap), n_regions);
  const dim3 block(ptd::kShareBlock);
  if (memo == 1) {
    PT_HIP(dev_alloc(slots, table_slots)); PT_HIP(dev_alloc(d_slot, n)); PT_HIP(dev_alloc(ctr, ptd::kMemoCounters)); PT_HIP(dev_alloc(bgr, 3 * n));
    PT_HIP(hipMemsetAsync(slots, 0xff, (size_t)table_slots * sizeof(ptd::MemoSlot), s));
    PT_HIP(hipMemsetAsync(ctr, 0, ptd::kMemoCounters * 8, s));
    PT_HIP(hipMemsetAsync(bgr, 0, 3 * n * 4, s));
    for (uint32_t pass = 1; pass <= passes; ++pass) {
      const ptd::MemoTable T{slots, table_slots - 1u, pass, d_slot, ctr};
      PT_HIP(hipMemsetAsync(len, 0, 4, s));
      PT_HIP(hipMemsetAsync(over, 0, 8, s));
      PT_HIP(hipMemsetAsync(ctr + ptd::kMemoServedCount, 0, (ptd::kMemoCounters - 1) * 8, s));   // as the step's prologue
      hipLaunchKernelGGL(ptd::memo_lookup_kernel, tiles, block, 0, s, Q, T);
      PT_HIP(hipGetLastError());
      hipLaunchKernelGGL(ptd::memo_resolve_kernel, grid, block, 0, s, Q, T);
      PT_HIP(hipGetLastError());
      if (pass < passes) {
        const dim3 pgrid(std::min<uint32_t>(ptd::kMemoGrid, (uint32_t)((n + ptd::kShareBlock - 1u) / ptd::kShareBlock)), 1);
        hipLaunchKernelGGL(ptd::memo_publish_kernel, pgrid, block, 0, s, slots, d_slot, bgr, len, (uint32_t)n, pass);
        PT_HIP(hipGetLastError());
      }
    }
  } else {
    PT_HIP(dev_alloc(keys, table_slots)); PT_HIP(dev_alloc(vals, table_slots));
    PT_HIP(hipMemsetAsync(keys, 0xff, (size_t)table_slots * 8, s));
    PT_HIP(hipMemsetAsync(len, 0, 4, s));
    const ptd::ShareTable T{keys, vals, table_slots - 1u};
    if (memo == 2) {
      hipLaunchKernelGGL(ptd::share_raw_claim_kernel, tiles, block, 0, s, Q, ptd::RawCountTable{T});
      PT_HIP(hipGetLastError());
    } else {
      hipLaunchKernelGGL(ptd::share_claim_kernel, tiles, block, 0, s, Q, T);
      PT_HIP(hipGetLastError());
      hipLaunchKernelGGL(ptd::share_resolve_kernel, grid, block, 0, s, Q, T);
      PT_HIP(hipGetLastError());
    }
  }
  PT_HIP(hipMemcpyAsync(owner, own, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(d_u, du, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(d_v, dv, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(d_count, len, 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(overflowed, over, 8, hipMemcpyDeviceToHost, s));
  if (memo == 1 && memo_counters) PT_HIP(hipMemcpyAsync(memo_counters, ctr, ptd::kMemoCounters * 8, hipMemcpyDeviceToHost, s));
  if (table_keys) {
    if (memo == 1) PT_HIP(hipMemcpy2DAsync(table_keys, 8, slots, sizeof(ptd::MemoSlot), 8, table_slots, hipMemcpyDeviceToHost, s));
    else PT_HIP(hipMemcpyAsync(table_keys, keys, (size_t)table_slots * 8, hipMemcpyDeviceToHost, s));
  }
  PT_HIP(hipStreamSynchronize(s));
  return PT_OK;
}

// test build only: the class table gets exactly `slots` slots (rounded up to a power of two; 0 = sized by the rule again), so that
// a test reaches the evaluated-alone path with a small image
int pt_diag_set_nif_class_capacity(pt_handle h, uint32_t slots) {
  if (!h || slots > ptshare::kClassMaxSlots) return PT_ERR_INVALID_ARGUMENT;
  uint32_t p = slots ? 2 : 0;
  while (p < slots) p <<= 1;
  h->group.class_diag_slots = p;
  h->group.class_failed = false;
  return PT_OK;
}

// test build only: how many E(b) the last pt_path_trace launched -- 0 in a mapped step whose accumulate passes expand
int pt_diag_expand_launches(pt_handle h, uint32_t* launches) {
  if (!h || !launches) return PT_ERR_INVALID_ARGUMENT;
  *launches = h->group.expand_launches;
  return PT_OK;
}

// test build only: the class level's claim and resolve over a distinct queue the caller supplies -- one region of n rows --
// with buffers of its own and a ClassTable of table_slots slots (a power of two).  Out, on the host: owner [n] (the position
// in the class queue of every row's class owner), the class queue c_u / c_v [n], its length and the rows evaluated alone.
int pt_diag_class_claim(pt_handle h, const float* u, const float* v, uint32_t n, uint32_t table_slots, uint32_t* owner, float* c_u,
                        float* c_v, uint32_t* c_count, uint64_t* alone) {
  if (!h || !u || !v || !owner || !c_u || !c_v || !c_count || !alone) return PT_ERR_INVALID_ARGUMENT;
  if (n == 0 || n >= ptshare::kMaxStoreEntries || table_slots < 2 || table_slots > ptshare::kClassMaxSlots || (table_slots & (table_slots - 1u)))
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_class_claim: sizes out of range");
  PT_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  DevBuf<float> q_u, q_v, du, dv;
  DevBuf<uint32_t> count, own, len, vals;
  DevBuf<unsigned long long> over, keys;
  PT_HIP(dev_alloc(q_u, n)); PT_HIP(dev_alloc(q_v, n)); PT_HIP(dev_alloc(du, n)); PT_HIP(dev_alloc(dv, n));
  PT_HIP(dev_alloc(count, 1)); PT_HIP(dev_alloc(own, n)); PT_HIP(dev_alloc(len, 1)); PT_HIP(dev_alloc(over, 1));
  PT_HIP(dev_alloc(keys, table_slots)); PT_HIP(dev_alloc(vals, table_slots));
  PT_HIP(hipMemcpyAsync(q_u, u, (size_t)n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(q_v, v, (size_t)n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(count, &n, 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemsetAsync(own, 0xff, (size_t)n * 4, s));   // an entry no pass writes reads as pending
  PT_HIP(hipMemsetAsync(over, 0, 8, s));
  PT_HIP(hipMemsetAsync(len, 0, 4, s));
  PT_HIP(hipMemsetAsync(keys, 0xff, (size_t)table_slots * 8, s));
  ptd::GroupQueue Q;
  Q.q_u = q_u; Q.q_v = q_v; Q.region_count = count; Q.region_cap = n; Q.owner = own;
  Q.d_u = du; Q.d_v = dv; Q.d_count = len; Q.base = 0; Q.overflowed = over;
  const ptd::ClassTable T{{keys, vals, table_slots - 1u}};
  const dim3 grid((n + ptd::kShareBlock - 1u) / ptd::kShareBlock, 1), tiles(ptshare::claim_tiles(n), 1), block(ptd::kShareBlock);
  hipLaunchKernelGGL(ptd::class_claim_kernel, tiles, block, 0, s, Q, T);
  PT_HIP(hipGetLastError());
  hipLaunchKernelGGL(ptd::class_resolve_kernel, grid, block, 0, s, Q, T);
  PT_HIP(hipGetLastError());
  PT_HIP(hipMemcpyAsync(owner, own, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_u, du, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_v, dv, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_count, len, 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(alone, over, 8, hipMemcpyDeviceToHost, s));
  PT_HIP(hipStreamSynchronize(s));
  return PT_OK;
}

// test build only: the fused claim and the two-hop resolve over a queue the caller supplies (laid out as for
// pt_diag_claim_resolve), with buffers of its own: a raw table of raw_slots and a class table of class_slots slots (powers of
// two).  Out, on the host: owner [n_regions x region_cap] (live entries: positions in the class queue), the distinct queue
// d_u / d_v and the class queue c_u / c_v (same capacity each), and counters[4]: the distinct queue's length, the raw
// overflows, the class queue's length, the rows that found no class slot.
int pt_diag_share_class_claim(pt_handle h, const float* u, const float* v, const uint32_t* region_count, uint32_t n_regions,
                              uint32_t region_cap, uint32_t raw_slots, uint32_t class_slots, uint32_t* owner, float* d_u, float* d_v,
                              float* c_u, float* c_v, uint64_t* counters) {
  if (!h || !u || !v || !region_count || !owner || !d_u || !d_v || !c_u || !c_v || !counters) return PT_ERR_INVALID_ARGUMENT;
  const uint64_t n64 = (uint64_t)n_regions * region_cap;
  if (n_regions == 0 || region_cap == 0 || n64 >= ptshare::kMaxStoreEntries || raw_slots < 2 || raw_slots > ptshare::kMaxSlots ||
      (raw_slots & (raw_slots - 1u)) || class_slots < 2 || class_slots > ptshare::kClassMaxSlots || (class_slots & (class_slots - 1u)))
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_share_class_claim: sizes out of range");
  for (uint32_t r = 0; r < n_regions; ++r)
    if (region_count[r] > region_cap) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_share_class_claim: a region's count exceeds its capacity");
  const size_t n = (size_t)n64;
  PT_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  DevBuf<float> q_u, q_v, du, dv, cu, cv;
  DevBuf<uint32_t> counts, own, len, vals, c_vals;   // len: [0] the distinct queue's length, [1] the class queue's
  DevBuf<unsigned long long> over, keys, c_keys;     // over: [0] raw overflows, [1] rows alone
  PT_HIP(dev_alloc(q_u, n)); PT_HIP(dev_alloc(q_v, n)); PT_HIP(dev_alloc(du, n)); PT_HIP(dev_alloc(dv, n));
  PT_HIP(dev_alloc(cu, n)); PT_HIP(dev_alloc(cv, n));
  PT_HIP(dev_alloc(counts, n_regions)); PT_HIP(dev_alloc(own, n)); PT_HIP(dev_alloc(len, 2)); PT_HIP(dev_alloc(over, 2));
  PT_HIP(dev_alloc(keys, raw_slots)); PT_HIP(dev_alloc(vals, raw_slots));
  PT_HIP(dev_alloc(c_keys, class_slots)); PT_HIP(dev_alloc(c_vals, class_slots));
  PT_HIP(hipMemcpyAsync(q_u, u, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(q_v, v, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(counts, region_count, (size_t)n_regions * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemsetAsync(own, 0xff, n * 4, s));   // an entry no pass writes reads as pending
  PT_HIP(hipMemsetAsync(over, 0, 16, s));
  PT_HIP(hipMemsetAsync(len, 0, 8, s));
  PT_HIP(hipMemsetAsync(keys, 0xff, (size_t)raw_slots * 8, s));
  PT_HIP(hipMemsetAsync(c_keys, 0xff, (size_t)class_slots * 8, s));
  ptd::GroupQueue Q;
  Q.q_u = q_u; Q.q_v = q_v; Q.region_count = counts; Q.region_cap = region_cap; Q.owner = own;
  Q.d_u = du; Q.d_v = dv; Q.d_count = len; Q.base = 0; Q.overflowed = over;
  ptd::ShareClassTable T;
  static_cast<ptd::ShareTable&>(T) = ptd::ShareTable{keys, vals, raw_slots - 1u};
  T.classes = ptd::ClassTable{{c_keys, c_vals, class_slots - 1u}};
  T.c_u = cu; T.c_v = cv; T.c_count = len + 1; T.c_base = 0; T.c_alone = over + 1;
  const dim3 grid((region_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock, n_regions), tiles(ptshare::claim_tiles(region_cap), n_regions);
  const dim3 block(ptd::kShareBlock);
  hipLaunchKernelGGL(ptd::share_class_claim_kernel, tiles, block, 0, s, Q, T);
  PT_HIP(hipGetLastError());
  hipLaunchKernelGGL(ptd::share_class_resolve_kernel, grid, block, 0, s, Q, T);
  PT_HIP(hipGetLastError());
  uint32_t h_len[2] = {0, 0};
  unsigned long long h_over[2] = {0, 0};
  PT_HIP(hipMemcpyAsync(owner, own, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(d_u, du, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(d_v, dv, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_u, cu, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_v, cv, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(h_len, len, 8, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(h_over, over, 16, hipMemcpyDeviceToHost, s));
  PT_HIP(hipStreamSynchronize(s));
  counters[0] = h_len[0]; counters[1] = h_over[0]; counters[2] = h_len[1]; counters[3] = h_over[1];
  return PT_OK;
}

// test build only: C(b) of a mapped step over a queue the caller supplies (laid out as for pt_diag_claim_resolve), with a class
// map and a tail of tail_slots slots (a power of two) of its own, `launches` times (1 or 2) over the same queue and the same
// class queue.  release_between: a release (and the counts reset) between the two launches, as two steps would run; otherwise
// the second launch finds what the first left, as a later batch of one step would.  A release follows the last launch.
// Out, on the host, of the last launch: owner [n_regions x region_cap] (live entries: the words C wrote), rows (the same after
// E(b)'s hop: positions in the class queue), the class queue c_u / c_v (same capacity, twice over: rows evaluated alone append
// per launch) and counters[4]: the class queue's length, the rows evaluated alone, the words of map and tail that are not
// kMapEmpty before the last release, and after it.
}  // extern "C"
namespace ptd {
__global__ __launch_bounds__(kShareBlock) void diag_map_hop_kernel(const uint32_t* region_count, uint32_t region_cap, const uint32_t* owner,
                                                                   const uint32_t* words, uint32_t* rows) {
  const uint32_t r = blockIdx.y, local = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x;
  if (local >= region_count[r]) return;
  const size_t q = (size_t)r * region_cap + local;
  const uint32_t o = owner[q];
  rows[q] = ptshare::owner_is_store(o) ? o : words[ptshare::owner_slot(o)];
}
__global__ __launch_bounds__(kShareBlock) void diag_map_count_kernel(const uint32_t* words, uint32_t n, unsigned long long* taken) {
  uint32_t mine = 0;
  for (uint32_t i = blockIdx.x * (uint32_t)kShareBlock + threadIdx.x; i < n; i += gridDim.x * (uint32_t)kShareBlock)
    mine += words[i] != ptshare::kMapEmpty ? 1u : 0u;
  if (mine) atomicAdd(taken, (unsigned long long)mine);   // (few words are taken: few atomics)
}
}  // namespace ptd
extern "C" {
int pt_diag_class_map_claim(pt_handle h, const float* u, const float* v, const uint32_t* region_count, uint32_t n_regions,
                            uint32_t region_cap, uint32_t tail_slots, uint32_t launches, int32_t release_between, uint32_t* owner,
                            uint32_t* rows, float* c_u, float* c_v, uint64_t* counters) {
  if (!h || !u || !v || !region_count || !owner || !rows || !c_u || !c_v || !counters) return PT_ERR_INVALID_ARGUMENT;
  const uint64_t n64 = (uint64_t)n_regions * region_cap;
  if (n_regions == 0 || region_cap == 0 || 2 * n64 >= ptshare::kMaxStoreEntries || tail_slots < 2 || tail_slots > ptshare::kClassTailMaxSlots ||
      (tail_slots & (tail_slots - 1u)) || launches < 1 || launches > 2)
    return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_class_map_claim: sizes out of range");
  for (uint32_t r = 0; r < n_regions; ++r)
    if (region_count[r] > region_cap) return fail(h, PT_ERR_INVALID_ARGUMENT, "pt_diag_class_map_claim: a region's count exceeds its capacity");
  const size_t n = (size_t)n64, n_words = (size_t)ptshare::kClassMapWords + tail_slots;
  PT_HIP(hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  DevBuf<float> q_u, q_v, cu, cv;
  DevBuf<uint32_t> counts, own, row, len, words;
  DevBuf<unsigned long long> over, tail_keys;   // over: [0] rows alone, [1] and [2] words taken before and after the last release
  PT_HIP(dev_alloc(q_u, n)); PT_HIP(dev_alloc(q_v, n)); PT_HIP(dev_alloc(cu, 2 * n)); PT_HIP(dev_alloc(cv, 2 * n));
  PT_HIP(dev_alloc(counts, n_regions)); PT_HIP(dev_alloc(own, n)); PT_HIP(dev_alloc(row, n)); PT_HIP(dev_alloc(len, 1)); PT_HIP(dev_alloc(over, 3));
  PT_HIP(dev_alloc(words, n_words)); PT_HIP(dev_alloc(tail_keys, tail_slots));
  PT_HIP(hipMemcpyAsync(q_u, u, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(q_v, v, n * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemcpyAsync(counts, region_count, (size_t)n_regions * 4, hipMemcpyHostToDevice, s));
  PT_HIP(hipMemsetAsync(over, 0, 24, s));
  PT_HIP(hipMemsetAsync(len, 0, 4, s));
  PT_HIP(hipMemsetAsync(words, 0xff, n_words * 4, s));
  PT_HIP(hipMemsetAsync(tail_keys, 0xff, (size_t)tail_slots * 8, s));
  ptd::GroupQueue Q;
  Q.q_u = q_u; Q.q_v = q_v; Q.region_count = counts; Q.region_cap = region_cap; Q.owner = own;
  Q.d_u = nullptr; Q.d_v = nullptr; Q.d_count = nullptr; Q.base = 0; Q.overflowed = nullptr;   // (C touches no distinct queue)
  const ptd::ClassMap M{words, tail_keys, tail_slots - 1u, cu, cv, len, 0u, over};
  const dim3 grid((region_cap + ptd::kShareBlock - 1u) / ptd::kShareBlock, n_regions), tiles(ptshare::claim_tiles(region_cap), n_regions);
  const dim3 block(ptd::kShareBlock), count_grid(ptd::kMemoGrid);
  auto release = [&]() -> int {   // as stage_map_release: one batch, whose class queue is the whole store
    hipLaunchKernelGGL(ptd::class_map_release_kernel, dim3(std::min<uint32_t>(ptd::kMemoGrid, (uint32_t)((2 * n + ptd::kShareBlock - 1u) / ptd::kShareBlock)), 1),
                       block, 0, s, cu, cv, len, 0u, words, tail_keys, tail_slots);
    PT_HIP(hipGetLastError());
    return PT_OK;
  };
  for (uint32_t launch = 0; launch < launches; ++launch) {
    if (launch && release_between) {
      if (int rc = release()) return rc;
      PT_HIP(hipMemsetAsync(len, 0, 4, s));
      PT_HIP(hipMemsetAsync(over, 0, 8, s));
    }
    PT_HIP(hipMemsetAsync(own, 0xff, n * 4, s));
    hipLaunchKernelGGL(ptd::class_map_claim_kernel, tiles, block, 0, s, Q, M);
    PT_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(ptd::diag_map_hop_kernel, grid, block, 0, s, counts, region_cap, own, words, row);
  PT_HIP(hipGetLastError());
  hipLaunchKernelGGL(ptd::diag_map_count_kernel, count_grid, block, 0, s, words, (uint32_t)n_words, over + 1);
  PT_HIP(hipGetLastError());
  if (int rc = release()) return rc;
  hipLaunchKernelGGL(ptd::diag_map_count_kernel, count_grid, block, 0, s, words, (uint32_t)n_words, over + 2);
  PT_HIP(hipGetLastError());
  uint32_t h_len = 0;
  unsigned long long h_over[3] = {0, 0, 0};
  PT_HIP(hipMemcpyAsync(owner, own, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(rows, row, n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_u, cu, 2 * n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(c_v, cv, 2 * n * 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(&h_len, len, 4, hipMemcpyDeviceToHost, s));
  PT_HIP(hipMemcpyAsync(h_over, over, 24, hipMemcpyDeviceToHost, s));
  PT_HIP(hipStreamSynchronize(s));
  counters[0] = h_len; counters[1] = h_over[0]; counters[2] = h_over[1]; counters[3] = h_over[2];
  return PT_OK;
}
#endif


}  // extern "C"
