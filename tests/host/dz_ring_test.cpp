// Host-only model test of the dz ring policy in mimo_unet_amd/csrc/dz_ring.h, built with -fsanitize=address,undefined by
// tests/test_sched_cpu.py.  Every sequence of {layer, join, rewind} of kDepth operations (three trips round the ring when all
// of them are layers) is walked from a clean ring and from every state an abandoned staged backward can leave (any run of
// layers and joins that stops short of the final join).  Next to the policy the test keeps its own account of the two
// streams: the side stream is in order, so a wait for slot w's release event orders every reader issued up to w's before
// the main stream.  Checked at every acquire():
//   * the slot handed out has no reader that the main stream is not ordered behind
//   * the wait is the one the former in-line logic of plan.hip's convbn_backward chose (kParentWait below), and that
//     logic's branch for an odd slot with its own bit set ("cannot happen in cyclic order") is never reached
#include <algorithm>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "../../mimo_unet_amd/csrc/dz_ring.h"

using mimo::sched::DzRingPolicy;

static constexpr int kSlots = DzRingPolicy::kSlots;
static constexpr int kDepth = 3 * kSlots;

// The wait of the former logic, as an offset from the acquired slot b (-1: none), by [b odd][pending[b]][pending[b + 1]]:
//   even b: the odd slot behind it when that one is pending (covers both), else b itself when pending
//   odd b : its own event when pending — the branch that was kept "as the safe path"; its column for b + 1 is not looked at
static constexpr int kParentWait[2][2][2] = {{{-1, 1}, {0, 1}}, {{-1, -1}, {0, 0}}};

struct Model {
  DzRingPolicy ring;
  // the former logic's own state, stepped beside the policy
  int p_next = 0;
  bool p_pending[kSlots] = {};
  // the streams: readers are numbered in the order they are issued on the side stream
  long issued = 0;              // readers issued so far
  long reader[kSlots] = {};     // number of the slot's last reader (0: none yet)
  long event[kSlots] = {};      // the reader its release event was last recorded behind
  long covered = 0;             // every reader up to this one is ordered before the main stream
};

static long failures = 0, acquires = 0, odd_pending_reached = 0;
static std::vector<char> trail;

static void fail(const char* what, const Model& m, int slot, int got, int want) {
  if (failures++ < 10) {
    std::printf("FAIL %s: slot %d wait %d (expected %d), reader %ld covered %ld, after \"", what, slot, got, want, m.reader[slot], m.covered);
    for (char c : trail) std::putchar(c);
    std::printf("\"\n");
  }
}

static void layer(Model& m) {
  const DzRingPolicy::Acquired a = m.ring.acquire();
  ++acquires;
  // the former logic
  const int b = m.p_next;
  m.p_next = (m.p_next + 1) % kSlots;
  const bool odd = (b & 1) != 0;
  const int off = kParentWait[odd][m.p_pending[b]][odd ? 0 : m.p_pending[b + 1]];
  const int want = off < 0 ? -1 : b + off;
  if (odd && m.p_pending[b]) ++odd_pending_reached;
  if (!odd) m.p_pending[b] = m.p_pending[b + 1] = false;
  if (a.slot != b || a.wait_on != want) fail("wait differs from the former logic", m, a.slot, a.wait_on, want);
  // the streams
  if (a.wait_on >= 0) m.covered = std::max(m.covered, m.event[a.wait_on]);
  if (m.reader[a.slot] > m.covered) fail("slot handed out under a reader", m, a.slot, a.wait_on, want);
  m.reader[a.slot] = m.event[a.slot] = ++m.issued;  // weight gradient + reduction, the release event behind them
  m.ring.released(a.slot);
  m.p_pending[b] = true;
}

static void join(Model& m) {  // (plan.hip DzRing::join: nothing is issued when no bit is set)
  bool p_any = false;
  for (bool p : m.p_pending) p_any |= p;
  if (m.ring.any_pending() != p_any) fail("join differs from the former logic", m, 0, m.ring.any_pending(), p_any);
  if (!m.ring.any_pending()) return;
  m.covered = m.issued;
  m.ring.joined();
  for (bool& p : m.p_pending) p = false;
}

static void rewind(Model& m) {
  m.ring.rewind();
  m.p_next = 0;
}

static void walk(const Model& m, int depth) {
  if (depth == kDepth) return;
  for (char op : {'L', 'J', 'R'}) {
    Model n = m;
    trail.push_back(op);
    if (op == 'L') layer(n);
    if (op == 'J') join(n);
    if (op == 'R') rewind(n);
    walk(n, depth + 1);
    trail.pop_back();
  }
}

// what distinguishes two models for everything that follows: the policy's state and the order of the numbers
static auto key(const Model& m) {
  long v[2 * kSlots + 1];
  for (int i = 0; i < kSlots; ++i) {
    v[i] = m.reader[i];
    v[kSlots + i] = m.event[i];
  }
  v[2 * kSlots] = m.covered;
  std::vector<long> sorted(v, v + 2 * kSlots + 1);
  std::sort(sorted.begin(), sorted.end());
  sorted.erase(std::unique(sorted.begin(), sorted.end()), sorted.end());
  std::vector<int> rank;
  for (long x : v) rank.push_back((int)(std::lower_bound(sorted.begin(), sorted.end(), x) - sorted.begin()));
  int bits = 0;
  for (int i = 0; i < kSlots; ++i) bits |= (m.ring.pending[i] ? 1 : 0) << i;
  return std::make_tuple(m.ring.next, bits, rank);
}

int main() {
  // start states: the clean ring and whatever a backward given up between two stages leaves — layers, joins in between
  std::vector<Model> starts{Model{}};
  std::set<decltype(key(Model{}))> seen{key(Model{})};
  for (size_t i = 0; i < starts.size(); ++i)
    for (char op : {'L', 'J'}) {
      Model n = starts[i];
      if (op == 'L') layer(n);
      if (op == 'J') join(n);
      if (seen.insert(key(n)).second) starts.push_back(n);
    }
  for (const Model& s : starts) walk(s, 0);
  std::printf("%zu start states, %ld acquires, odd slot pending at its acquire: %ld times\n", starts.size(), acquires, odd_pending_reached);
  if (odd_pending_reached) {
    std::printf("FAIL the policy has no wait for an odd slot, but the former logic's branch for it was reached\n");
    ++failures;
  }
  if (failures) {
    std::printf("%ld failures\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
