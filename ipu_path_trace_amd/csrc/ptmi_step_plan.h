// ptmi_step_plan.h -- the integer arithmetic of a step: how its sample iterations are dealt into batches, the trace grid of a
// batch, the reciprocal of the work-item count.  Plain C++ (nothing from HIP), so that tests/step_plan_main.cpp checks it on
// a CPU; ptmi.hip includes it ahead of ptmi_context.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ptplan {

// Round-up reciprocal of the work-item count: (x * magic) >> shift == x / n for every x < 2^31 (Granlund & Montgomery: with
// s = ceil(log2 n) and magic = floor(2^(31+s) / n) + 1 the error magic * n - 2^(31+s) lies in (0, 2^s], so the product's excess
// over x / n stays below 1 / n).  The batch size keeps path indices below 2^31 (pt_create).
inline void item_divider(uint32_t n, uint32_t& magic, uint32_t& shift) {
  uint32_t s = 0;
  while ((1ull << s) < n) ++s;
  const uint64_t m = ((1ull << (31 + s)) / n) + 1ull;
  magic = (uint32_t)m;     // < 2^32: n > 2^(s-1)
  shift = 31 + s;
}

// Trace-grid geometry for a batch of `total` paths.
struct TraceGrid {
  uint32_t blocks, n_waves, region_cap;
};
// `cap` = pt_context::trace_blocks: the workgroups of the persistent trace kernel that are resident at once (pt_create).
inline TraceGrid trace_grid(uint32_t total, uint32_t cap) {
  const uint32_t n_chunks = (total + 63u) / 64u;
  uint32_t blocks = (n_chunks + 3u) / 4u;
  if (blocks > cap) blocks = cap;
  if (blocks == 0) blocks = 1;
  TraceGrid g;
  g.blocks = blocks;
  g.n_waves = blocks * 4u;
  g.region_cap = 4u * ((n_chunks + g.n_waves - 1u) / g.n_waves) * 64u;
  return g;
}

// The sample iterations of every batch of a step, in order.  The first batch is kept short when the step has several: its
// trace kernel is the only one with no NIF kernel to hide under, so the sooner it ends the sooner the MFMA pipes start (a
// constant environment has no NIF stage to start).  The remaining iterations are dealt EVENLY over as few batches as the
// capacity allows (sizes differ by one at most, the larger ones first), so no step ends on a stub of a batch whose launch
// tails weigh as much as a full one's.  Per-pixel sums stay in iteration order whatever the split.
inline std::vector<uint32_t> batch_iterations(uint32_t samples_per_step, uint32_t iters_per_batch, uint32_t first_batch_iters,
                                              bool env_const) {
  const uint32_t first =
      (!env_const && samples_per_step > 2u * iters_per_batch) ? std::min(first_batch_iters, iters_per_batch) : 0u;
  const uint32_t rest = samples_per_step - first;
  const uint32_t rest_batches = (rest + iters_per_batch - 1u) / iters_per_batch;
  const uint32_t base = rest_batches ? rest / rest_batches : 0u, longer = rest_batches ? rest % rest_batches : 0u;
  std::vector<uint32_t> iters;
  iters.reserve((first ? 1u : 0u) + rest_batches);
  if (first) iters.push_back(first);
  for (uint32_t r = 0; r < rest_batches; ++r) iters.push_back(base + (r < longer ? 1u : 0u));
  return iters;
}

// The ring of batch-buffer sets.  Batch b of a step uses set b mod depth; before it may overwrite the set, the batch that used
// the set last -- b - depth -- must have been accumulated.  With `depth` sets, `depth` batches travel the dependency cycle
// N -> E -> A -> T -> S -> N at once.
constexpr uint32_t kNoBatch = ~0u;
inline uint32_t ring_slot(uint32_t batch, uint32_t depth) { return batch % depth; }
// The batch whose `accumulated` event T(batch) waits for, or kNoBatch: the first `depth` batches of a step find their set free.
inline uint32_t ring_predecessor(uint32_t batch, uint32_t depth) { return batch >= depth ? batch - depth : kNoBatch; }
// Store region of a batch's distinct queue (NIF sharing): its own at step scope, the one that goes with its set at batch scope.
inline uint32_t store_region(uint32_t batch, uint32_t depth, bool step_scope) { return step_scope ? batch : ring_slot(batch, depth); }

}  // namespace ptplan
