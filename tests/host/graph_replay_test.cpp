// Host-only model test of the graph replay policy in mimo_unet_amd/csrc/graph_replay.h, built with -fsanitize=address,undefined
// by tests/test_sched_cpu.py.  The reference (struct Parent) is the capture decision as plan.hip's forward() and backward() held
// it in line before the policy existed, transcribed with a bool for each hipGraphExec_t: tg_fwd / tg_fwd_key / tg_fwd_seen,
// tg_bwd[] / tg_bwd_key / tg_bwd_seen and the one tg_captures counter, and graph_exec / graph_key of the eval-mode forward.
// Every sequence of kDepth events of
//   a b  training forward with call shape A / B        A B  backward (stage 0), whole / per stage, no loss mask, no perm: its
//                                                            key is formed from the forward's live key, as plan.hip forms it
//   n    a call that is not graphable (no trace)       d    drop graphs (mimo_plan_bind with other tensors)
// is walked with a budget of kBudget captures, from the clean state and from every state a drop can leave (captures spent
// are not refunded), and at every step the policy's decision and the captures spent must be the reference's.  Checked on the
// policy directly as well:
//   * Replay is only returned for the key of an executable that exists
//   * a key is not captured at its first sighting (training routes) — but for key 0, which a per-stage backward has behind a
//     drop (no forward graph is live then) and which both the former logic and the policy take for "seen" after a reset: that
//     sequence (a a d B B: capture, replay) is pinned in main()
//   * no Capture once the budget is spent, and from then on no Replay either — a live graph included
// The eval-mode form (capture at first sight, no budget) is walked the same way against graph_exec / graph_key.
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "../../mimo_unet_amd/csrc/graph_replay.h"

using mimo::sched::CaptureBudget;
using mimo::sched::GraphReplayPolicy;
typedef GraphReplayPolicy::Decision Decision;

static constexpr int kDepth = 9, kBudget = 3;
static constexpr uint64_t kFwdA = 1 | 2 | 16, kFwdB = 1 | 4 | 16;
// backward(): key = (key of the live forward graph << 3) | (lmask ? 4 : 0) | (lperm ? 2 : 0) | (whole ? 1 : 0)
static constexpr uint64_t kWhole = 1, kPerStage = 0;

// ---- the former in-line logic ----
struct Parent {
  static constexpr int kBwdStages = 8, kBwdGraphs = 9, kMaxTrainCaptures = kBudget;
  bool graph_exec = false;
  uint64_t graph_key = 0;
  bool tg_fwd = false;
  uint64_t tg_fwd_key = 0, tg_fwd_seen = 0;
  bool tg_bwd[kBwdGraphs] = {};
  uint64_t tg_bwd_key = 0, tg_bwd_seen = 0;
  bool tg_bwd_live = false;
  int tg_captures = 0;

  void drop_train_graphs() {
    tg_fwd = false;
    tg_fwd_key = tg_fwd_seen = 0;
    for (auto& e : tg_bwd) e = false;
    tg_bwd_key = tg_bwd_seen = 0;
  }
  void drop_graphs() {
    graph_exec = false;
    drop_train_graphs();
  }
  // forward(): every other term of `graphable` holds (profiler off, x4 / x5, no element-wise masks, rows <= N, train_graph
  // for a training call, !need_derive for an eval one)
  Decision forward(uint64_t key, bool training_call) {
    const bool graphable = training_call ? tg_captures < kMaxTrainCaptures : true;
    bool eager = !graphable;
    if (graphable && training_call && !(tg_fwd && key == tg_fwd_key) && key != tg_fwd_seen) {
      tg_fwd_seen = key;  // first sighting of this call shape: eager (captured when it comes again)
      eager = true;
    }
    if (eager) return GraphReplayPolicy::Eager;
    bool* exec = training_call ? &tg_fwd : &graph_exec;
    uint64_t* ekey = training_call ? &tg_fwd_key : &graph_key;
    Decision d = GraphReplayPolicy::Replay;
    if (!*exec || key != *ekey) {
      if (*exec) *exec = false;
      *exec = true;  // capture
      *ekey = key;
      if (training_call) ++tg_captures;
      d = GraphReplayPolicy::Capture;
    }
    return d;
  }
  // backward() at stage 0: train_graph && !ready && fwd_graphed && loss_staged && ... && (whole || single) hold
  Decision backward(uint64_t key) {
    Decision d = GraphReplayPolicy::Eager;
    tg_bwd_live = false;
    const bool whole = (key & 1) != 0;
    if (tg_captures < kMaxTrainCaptures) {
      bool have_graphs = tg_bwd_key == key && (whole ? tg_bwd[kBwdStages] : tg_bwd[0]);
      if (have_graphs) d = GraphReplayPolicy::Replay;
      if (!have_graphs && tg_bwd_seen == key) {
        for (auto& e : tg_bwd) e = false;
        tg_bwd_key = 0;
        if (whole) {
          tg_bwd[kBwdStages] = true;
        } else {
          for (int stage = 0; stage < kBwdStages; ++stage) tg_bwd[stage] = true;
        }
        tg_bwd_key = key;
        ++tg_captures;
        have_graphs = true;
        d = GraphReplayPolicy::Capture;
      }
      tg_bwd_seen = key;
      tg_bwd_live = have_graphs;
    }
    return d;
  }
};

// ---- the policy as plan.hip holds it, with the test's own ledger ----
struct Route {
  GraphReplayPolicy policy;
  bool exists = false;           // an executable exists (made by a Capture, gone with a drop)
  uint64_t sighted[6] = {};      // keys decided since the last drop (at most six per route: {none, A, B} live x whole / per stage)
  int nsighted = 0;
  bool sighting(uint64_t key) const {
    for (int i = 0; i < nsighted; ++i)
      if (sighted[i] == key) return true;
    return false;
  }
  void note(uint64_t key) {
    if (!sighting(key)) sighted[nsighted++] = key;
  }
};

struct Model {
  Parent parent;
  CaptureBudget budget{kBudget, 0};
  Route fwd, bwd, eval;
  Model() {  // the header's own constructors, as in mimo_plan
    fwd.policy = GraphReplayPolicy::training_forward(&budget);
    bwd.policy = GraphReplayPolicy::training_backward(&budget);
    eval.policy = GraphReplayPolicy::eval_forward();
  }
  Model(const Model& o) : parent(o.parent), budget(o.budget), fwd(o.fwd), bwd(o.bwd), eval(o.eval) {
    fwd.policy.budget = bwd.policy.budget = &budget;  // (this copy's own budget)
  }
  Model& operator=(const Model&) = delete;
};

static long failures = 0, decisions = 0;
static std::vector<char> trail;

static void fail(const char* what, uint64_t key, int got, int want) {
  if (failures++ < 10) {
    std::printf("FAIL %s: key %llu decision %d (reference %d) after \"", what, (unsigned long long)key, got, want);
    for (char c : trail) std::putchar(c);
    std::printf("\"\n");
  }
}

static void decide(Model& m, Route& r, uint64_t key, Decision want) {
  const bool budgeted = r.policy.budget != nullptr;
  const bool spent_before = budgeted && m.budget.spent >= m.budget.max;
  const uint64_t live_before = r.policy.live;
  const Decision got = r.policy.decide(key);
  ++decisions;
  if (got != want) fail("decision differs from the former logic", key, got, want);
  if (m.budget.spent != m.parent.tg_captures) fail("captures spent differ from the former logic", key, m.budget.spent, m.parent.tg_captures);
  if (got == GraphReplayPolicy::Replay && !(r.exists && live_before == key)) fail("replay of a key that is not the live executable's", key, got, want);
  if (got == GraphReplayPolicy::Capture && !r.policy.at_first_sight && key != 0 && !r.sighting(key)) fail("captured at first sight", key, got, want);
  if (spent_before && got != GraphReplayPolicy::Eager) fail("graphed with the budget spent", key, got, want);
  if (m.budget.spent > m.budget.max) fail("budget overdrawn", key, m.budget.spent, m.budget.max);
  if (got == GraphReplayPolicy::Capture) r.exists = true;
  r.note(key);
}

static void drop(Model& m) {  // (plan.hip drop_graphs)
  m.parent.drop_graphs();
  for (Route* r : {&m.fwd, &m.bwd, &m.eval}) {
    r->policy.reset();
    r->exists = false;
    r->nsighted = 0;
  }
}

static void apply(Model& m, char op) {
  switch (op) {
    case 'a': decide(m, m.fwd, kFwdA, m.parent.forward(kFwdA, true)); break;
    case 'b': decide(m, m.fwd, kFwdB, m.parent.forward(kFwdB, true)); break;
    case 'A':
    case 'B': {
      const uint64_t bits = op == 'A' ? kWhole : kPerStage;
      const uint64_t key = (m.fwd.policy.live << 3) | bits, parent_key = (m.parent.tg_fwd_key << 3) | bits;
      if (key != parent_key) fail("backward key differs from the former logic's", key, 0, 0);
      decide(m, m.bwd, key, m.parent.backward(parent_key));
      break;
    }
    case 'e': decide(m, m.eval, kFwdA & ~16ull, m.parent.forward(kFwdA & ~16ull, false)); break;
    case 'f': decide(m, m.eval, kFwdB & ~16ull, m.parent.forward(kFwdB & ~16ull, false)); break;
    case 'd': drop(m); break;
    default: break;  // 'n': not graphable — neither the former logic nor plan.hip asks anything
  }
}

static void walk(const Model& m, const char* ops, int depth) {
  if (depth == kDepth) return;
  for (const char* op = ops; *op; ++op) {
    Model n(m);
    trail.push_back(*op);
    apply(n, *op);
    walk(n, ops, depth + 1);
    trail.pop_back();
  }
}

static auto key(const Model& m) {
  return std::make_tuple(m.fwd.policy.have, m.fwd.policy.live, m.fwd.policy.seen, m.bwd.policy.have, m.bwd.policy.live, m.bwd.policy.seen,
                         m.budget.spent);
}

int main() {
  static const char kTrainOps[] = "abABnd", kEvalOps[] = "efabd";
  // start states: the clean one and whatever a drop leaves behind (reachable states first, then a drop on each)
  std::vector<Model> reach;
  reach.emplace_back();
  std::set<decltype(key(Model{}))> seen{key(reach[0])};
  for (size_t i = 0; i < reach.size(); ++i)
    for (const char* op = kTrainOps; *op; ++op) {
      Model n(reach[i]);
      apply(n, *op);
      if (seen.insert(key(n)).second) reach.push_back(n);
    }
  std::vector<Model> starts;
  starts.emplace_back();
  std::set<int> spent{0};
  for (const Model& r : reach) {
    Model n(r);
    drop(n);
    if (spent.insert(n.budget.spent).second) starts.push_back(n);
  }
  for (const Model& s : starts) walk(s, kTrainOps, 0);
  const long train_decisions = decisions;
  {  // key 0: a per-stage backward behind a drop of the forward's graph is captured at once and then replayed, as it was
    Model m;
    for (char op : {'a', 'a', 'd'}) apply(m, op);
    const int before = m.budget.spent;
    apply(m, 'B');
    if (!(m.bwd.policy.have && m.bwd.policy.live == 0 && m.budget.spent == before + 1 && m.bwd.exists)) fail("key 0 behind a drop not captured", 0, 0, 1);
    apply(m, 'B');
    if (m.budget.spent != before + 1) fail("key 0 captured twice", 0, 0, 2);
  }
  // eval-mode replay beside the training routes (it shares nothing with them, budget included)
  for (const Model& s : starts) walk(s, kEvalOps, 0);
  std::printf("%zu reachable states, %zu start states, %ld + %ld decisions\n", reach.size(), starts.size(), train_decisions,
              decisions - train_decisions);
  if ((int)starts.size() != kBudget + 1) {
    std::printf("FAIL expected a start state for each number of captures spent\n");
    ++failures;
  }
  if (failures) {
    std::printf("%ld failures\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
