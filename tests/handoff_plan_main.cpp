// The clean-table hand-off (ipu_path_trace_amd/csrc/ptmi_share_plan.h: clear_skippable, mark_after_step) on the CPU:
// tests/test_handoff_plan.py builds this with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstdlib>
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

// ---- the clean mark against a model of the table itself
// What a step of the sequences is.  kResized: a step-scope step whose table is reallocated at another size before it runs;
// kFailed: a step-scope step that returns an error.
enum Op { kOpStep, kOpBatch, kOpMemo, kOpOff, kOpFailed, kOpResized, kOps };

// The table as the device sees it: its size and whether any key is in it.  A fresh allocation holds anything.
struct Model {
  uint32_t slots = 0;
  bool dirty = true;
  uint32_t mark = 0;       // the handle's mark, kept by the rule under test
  uint32_t clears = 0, skips = 0;
};

static void reallocate(Model& m, uint32_t slots) {   // alloc_share_table: the host drops the mark where it happens
  m.slots = slots;
  m.dirty = true;
  m.mark = 0;
}

// One step through the rule; checks that a step-scope step never claims into a table that holds a key.
static void run(Model& m, Op op) {
  if (op == kOpResized) reallocate(m, m.slots == 1024 ? 2048 : 1024);
  const StepKind kind = op == kOpBatch ? StepKind::kBatch : op == kOpMemo ? StepKind::kMemo : op == kOpOff ? StepKind::kOff : StepKind::kStep;
  const bool ok = op != kOpFailed;
  if (kind == StepKind::kStep) {
    if (clear_skippable(m.mark, kind, m.slots)) m.skips += 1;
    else { m.dirty = false; m.clears += 1; }
    CHECK(!m.dirty);        // S(0) starts on an empty table
    m.dirty = true;         // the step's claims
    if (ok) m.dirty = false;   // the clear behind the last S(b); a failed step may have stopped ahead of it
  } else if (kind == StepKind::kBatch) {
    CHECK(!clear_skippable(m.mark, kind, m.slots));   // batch scope clears per batch, whatever the mark
    m.dirty = true;         // the last batch's keys stay
  } else {
    CHECK(!clear_skippable(m.mark, kind, m.slots));
  }
  m.mark = mark_after_step(m.mark, kind, m.slots, ok);
  CHECK(m.mark == 0 || (m.mark == m.slots && !m.dirty));   // the mark never says more than is true
}

int main() {
  // the rule, case by case
  CHECK(!clear_skippable(0, StepKind::kStep, 1024) && clear_skippable(1024, StepKind::kStep, 1024));
  CHECK(!clear_skippable(1024, StepKind::kStep, 2048) && !clear_skippable(2048, StepKind::kStep, 1024));   // another size
  CHECK(!clear_skippable(0, StepKind::kStep, 0));                                                          // no table
  CHECK(!clear_skippable(1024, StepKind::kBatch, 1024) && !clear_skippable(1024, StepKind::kMemo, 1024) && !clear_skippable(1024, StepKind::kOff, 1024));
  CHECK(clear_skippable(1u << 30, StepKind::kStep, 1u << 30) && !clear_skippable(1u << 30, StepKind::kStep, 1u << 29));
  for (uint32_t mark : {0u, 1024u, 1u << 30}) {
    CHECK(mark_after_step(mark, StepKind::kStep, 4096, true) == 4096);
    CHECK(mark_after_step(mark, StepKind::kOff, 4096, true) == mark);   // the table was not touched
    CHECK(mark_after_step(mark, StepKind::kBatch, 4096, true) == 0);
    CHECK(mark_after_step(mark, StepKind::kMemo, 4096, true) == 0);
    for (StepKind k : {StepKind::kOff, StepKind::kBatch, StepKind::kStep, StepKind::kMemo}) CHECK(mark_after_step(mark, k, 4096, false) == 0);
  }

  // every sequence of three steps, behind each possible history of one step (so that the first of the three meets every mark)
  uint32_t sequences = 0, skips = 0;
  for (int first = 0; first < kOps; ++first)
    for (int a = 0; a < kOps; ++a)
      for (int b = 0; b < kOps; ++b)
        for (int c = 0; c < kOps; ++c) {
          Model m;
          reallocate(m, 1024);
          run(m, (Op)first);
          const uint32_t before = m.skips;
          run(m, (Op)a); run(m, (Op)b); run(m, (Op)c);
          skips += m.skips - before;
          sequences += 1;
        }
  CHECK(sequences == kOps * kOps * kOps * kOps);
  // ... and the hand-off is taken where it may be: step after step, and across a step with sharing off
  {
    Model m;
    reallocate(m, 1024);
    run(m, kOpStep); run(m, kOpStep); run(m, kOpOff); run(m, kOpStep);
    CHECK(m.clears == 1 && m.skips == 2);
    run(m, kOpBatch); run(m, kOpStep);          // batch scope drops the mark
    CHECK(m.clears == 2 && m.skips == 2);
    run(m, kOpMemo); run(m, kOpStep);           // so does the memo
    CHECK(m.clears == 3 && m.skips == 2);
    run(m, kOpFailed); run(m, kOpStep);         // the failed step itself skipped; the step behind it clears
    CHECK(m.clears == 4 && m.skips == 3);
    run(m, kOpResized); run(m, kOpStep);        // the resized step clears, the one behind it skips
    CHECK(m.clears == 5 && m.skips == 4);
  }
  CHECK(skips > 0);

  std::printf("HANDOFF_PLAN_OK %u sequences, %u skipped clears\n", sequences, skips);
  return 0;
}
