// When a graphable call is launched eagerly, captured into a hipGraph, or replayed from the one that is live: the decision
// state of plan.hip's forward and backward graph routes (which own the hipGraphExec_t handles, the staging copies, the captures
// and the "is this call graphable" predicates).  No HIP dependency, so that tests/host/graph_replay_test.cpp, built with
// g++ -fsanitize=address,undefined, walks every sequence of forwards, backwards and drops against the logic this replaced.
//
// A call shape is a key.  Training graphs: eager the first time a key is seen, captured when the same key comes
// again straight away, replayed while it stands — one-off shapes stay eager, and every kernel has run eagerly once before it is
// captured.  Each capture is paid from a budget the forward and the backward policy of a plan share: a caller that keeps
// alternating call shapes would otherwise re-capture (milliseconds of host time) every other step.  With the budget spent
// nothing is graphed any more, a live graph included.  The eval-mode forward is the same type without a budget, capturing at
// first sight.  Key 0 is the value `seen` has after reset(): the first graphable call with key 0 counts as seen before and
// is captured at once.  plan.hip's forward keys are never 0; its backward key is — a per-stage backward without loss mask and
// perm behind a mimo_plan_bind that dropped the forward's graph — and the logic this replaced behaved the same way.
#pragma once

#include <cstdint>

namespace mimo {
namespace sched {

struct CaptureBudget {
  int max = 0, spent = 0;
  bool left() const { return spent < max; }
};

struct GraphReplayPolicy {
  enum Decision { Eager, Capture, Replay };

  CaptureBudget* budget = nullptr;  // captures are paid from it (shared between policies); null: not counted, never exhausted
  bool at_first_sight = false;      // capture a key the first time it is seen (else: the second time in a row)
  // a replay counts as the last sighting.  The two training routes differ in exactly this, and both are kept as they were: after
  // keys A A B A, the forward (false) captures the next B — B is still the key seen last — the backward (true) runs it eagerly.
  bool replay_is_sighting = false;

  bool have = false;  // an executable exists
  uint64_t live = 0;  // ... captured for this key
  uint64_t seen = 0;  // key seen last (0 after reset)

  // the three routes of a plan (plan.hip and tests/host/graph_replay_test.cpp build theirs here)
  static GraphReplayPolicy training_forward(CaptureBudget* b) { return GraphReplayPolicy{b, false, false}; }
  static GraphReplayPolicy training_backward(CaptureBudget* b) { return GraphReplayPolicy{b, false, true}; }
  static GraphReplayPolicy eval_forward() { return GraphReplayPolicy{nullptr, true, false}; }

  // for a graphable call only (any other call is eager and leaves no trace here).  Capture: the caller destroys what it has,
  // captures `key` and replays it — or reports capture_failed().
  Decision decide(uint64_t key) {
    if (budget && !budget->left()) return Eager;
    if (have && live == key) {
      if (replay_is_sighting) seen = key;
      return Replay;
    }
    if (!at_first_sight && seen != key) {
      seen = key;
      return Eager;
    }
    have = true;
    live = key;
    if (budget) ++budget->spent;
    return Capture;
  }
  // the capture just decided did not produce an executable: none is live, nothing was spent
  void capture_failed() {
    have = false;
    if (budget) --budget->spent;
  }
  // the executables are gone (other parameter or gradient tensors bound).  Spent captures are not refunded.
  void reset() {
    have = false;
    live = seen = 0;
  }
};

}  // namespace sched
}  // namespace mimo
