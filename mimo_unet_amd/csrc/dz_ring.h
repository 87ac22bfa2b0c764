// Which dz buffer the BatchNorm backward of the next layer writes, and which release event the caller's stream has to wait for
// first: the decision state of plan.hip's DzRing (which owns the buffers, the events and the HIP calls).  No HIP dependency, so
// that tests/host/dz_ring_test.cpp, built with g++ -fsanitize=address,undefined, walks every sequence of layers, joins and rewinds.
//
// The side stream's weight gradients may lag kSlots dz buffers (with their max |dz| slots) behind the caller's stream.
// Round 6: 4 buffers, released in PAIRS — the main stream waits for the side stream once per two layers (in front of an even
// buffer, for the event of the odd one behind it: the side stream is in order, so that covers both) instead of once per layer.
// A cross-stream wait in front of a kernel costs the waiting stream ~4 us on this stack even when it is already satisfied
// (scripts/micro/event_cost.hip).  (2 buffers with a wait per layer, rounds 2-5: measured and settled)
#pragma once

namespace mimo {
namespace sched {

struct DzRingPolicy {
  static constexpr int kSlots = 4;
  static_assert(kSlots >= 4 && kSlots % 2 == 0, "slots are released in pairs");

  int next = 0;                  // slot the next layer writes
  bool pending[kSlots] = {};     // the slot's last reader was issued on the side stream and is not yet ordered before the main one

  // slot: the dz buffer to write; wait_on: the slot whose release event the main stream waits for first, -1: none
  struct Acquired {
    int slot, wait_on;
  };
  // An odd slot never needs a wait of its own: `next` only ever steps by one or returns to 0, so the acquire in front of an
  // odd slot is the one of the even slot below it, which cleared both bits (dz_ring_test.cpp walks every sequence).
  Acquired acquire() {
    const int b = next;
    next = (next + 1) % kSlots;
    int w = -1;
    if ((b & 1) == 0) {
      // last reader of this dz buffer (and, released in pairs, of the one after it)
      if (pending[b + 1])
        w = b + 1;
      else if (pending[b])
        w = b;
      pending[b] = pending[b + 1] = false;  // (their last readers are behind this wait)
    }
    return Acquired{b, w};
  }
  // the slot's last reader (the weight gradient's reduction) has been issued, its release event follows it
  void released(int slot) { pending[slot] = true; }
  bool any_pending() const {
    bool any = false;
    for (bool p : pending) any |= p;
    return any;
  }
  // the main stream has waited for everything issued on the side stream
  void joined() {
    for (bool& p : pending) p = false;
  }
  // a graph capture starts every graph at slot 0 (the bits stay: readers issued before the capture are still in flight)
  void rewind() { next = 0; }
};

}  // namespace sched
}  // namespace mimo
