// follow_lists.h — what travels between the kernels of the certified search (launch_nn), defined
// once: the four follow-up lists, their counters, the entry encodings, the lists' layout inside one
// allocation with its capacities, and the three sizes an iteration's record publishes.
//
//   k_nn_wave  --exact-->  k_nn_ball   queries whose result the wave could not certify: the exact
//                                      reference-order DFS
//              --ball--->  k_nn_ball   queries no wave box took or settled, with a distance guess:
//                                      the ball search (which finishes some per lane or by DFS)
//              --halves->  k_nn_half   overflowed waves (their box holds more than kWaveCandCap
//                                      candidates) as two 32-query halves; a source's first iterate
//              --wide--->  k_nn_wide   overflowed waves or halves, searched again in segments
//   k_nn_half and k_nn_wide append to the exact and ball lists too (and k_nn_half to the wide list):
//   k_nn_ball runs last and reads both complete.
//
// A list is an array plus its counter in FollowCounts; every kernel of the chain starts after the
// one before it ended, so a consumer reads a complete list. The counters are zero at launch_nn:
// the iterate's publish (reduce_kernels.hip finalize_cov_publish) clears them after reading, any
// other caller with a memset of sizeof(FollowCounts).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "icp_common.h"

namespace icp {

// The counters, one device allocation of the context. The first two and halves / wide are list
// sizes (the producers' atomicAdd returns the slot); the others only count.
struct FollowCounts {
  unsigned int exact;          // entries of FollowLists::exact
  unsigned int ball;           // entries of FollowLists::ball (and ball_u)
  unsigned int lane_searches;  // queries the ball search finished by a per-lane / cooperative search
  unsigned int dfs_finishes;   // queries the ball search finished by the exact DFS
  unsigned int halves;         // entries of FollowLists::halves
  unsigned int wide;           // entries of FollowLists::wide
  unsigned int overflowed;     // waves of k_nn_wave whose candidate set overflowed (IterDev::n_wide)
  unsigned int pad;            // never written: stays zero
};
static_assert(sizeof(FollowCounts) == 32, "eight words");

// The publish's reset: every counter a kernel writes, member by member.
ICP_HD void clear_counts(FollowCounts* c) {
  c->exact = 0u;
  c->ball = 0u;
  c->lane_searches = 0u;
  c->dfs_finishes = 0u;
  c->halves = 0u;
  c->wide = 0u;
  c->overflowed = 0u;
}

// The sizes an iteration's record carries (IterDev::lists, LoopRec::lists, icp_iter_stats
// n_fallback / n_ball_search / n_lane_search), in that order.
struct PublishedLists {
  unsigned int exact;  // exact DFS searches: the wave search's exact list + the ball search's DFS finishes
  unsigned int ball;   // the ball list
  unsigned int lane;   // per-lane searches
};
ICP_HD PublishedLists published_lists(const FollowCounts& c) {
  return PublishedLists{c.exact + c.dfs_finishes, c.ball, c.lane_searches};
}

// The lists as the kernels see them: six consecutive fields of NNLaunch (kernels.h).
struct FollowLists {
  int32_t* exact;   // queries sent to the exact reference-order DFS
  int32_t* ball;    // queries a wave did not take or settle -> ball search
  double* ball_u;   // the distance guess u of each ball entry
  FollowCounts* n;  // zero at the launch
  int32_t* halves;  // HalfEntry records (push_half / read_half); null: no half pass
  int32_t* wide;    // WideEntry records (push_wide / read_wide); null: no wide pass, overflowed
                    // lanes take the ball search
};

// A 32-query half of an overflowed wave: queries 32 * half + lane for the lanes set in `lanes`.
struct HalfEntry {
  int32_t half;
  uint32_t lanes;
};
// An overflowed wave or half for the wide pass: queries first + lane for the lanes set in the mask.
struct WideEntry {
  int32_t first;
  uint32_t lanes_lo, lanes_hi;
};
constexpr int kHalfEntryInts = (int)(sizeof(HalfEntry) / sizeof(int32_t));
constexpr int kWideEntryInts = (int)(sizeof(WideEntry) / sizeof(int32_t));
static_assert(kHalfEntryInts == 2 && kWideEntryInts == 3, "entries are whole ints, no padding");

#if defined(__HIPCC__)
// Entry `at` of a list, stored and loaded int by int (4-byte accesses: the lists are only
// int-aligned, and the records of one wave are written by one lane).
__device__ __forceinline__ void push_half(int32_t* list, unsigned at, HalfEntry e) {
  list[2 * at] = e.half;
  list[2 * at + 1] = (int32_t)e.lanes;
}
__device__ __forceinline__ HalfEntry read_half(const int32_t* list, unsigned at) {
  return HalfEntry{list[2 * at], (uint32_t)list[2 * at + 1]};
}
__device__ __forceinline__ void push_wide(int32_t* list, unsigned at, WideEntry e) {
  list[3 * at] = e.first;
  list[3 * at + 1] = (int32_t)e.lanes_lo;
  list[3 * at + 2] = (int32_t)e.lanes_hi;
}
__device__ __forceinline__ WideEntry read_wide(const int32_t* list, unsigned at) {
  return WideEntry{list[3 * at], (uint32_t)list[3 * at + 1], (uint32_t)list[3 * at + 2]};
}
#endif

// --- The layout: the four lists in one allocation of follow_list_ints(n) ints for n queries.
// Capacities, per list:
//   exact, ball  n entries: a query is appended to each at most once per search (a wave appends
//                only queries it does not defer; a second pass only the queries deferred to it).
//   halves       two entries per wave: k_nn_wave pushes the non-empty halves of an overflowed wave.
//   wide         three entries per wave: an overflowed wave pushes either itself (no half pass, or
//                the cache instance) or its two halves, each of which pushes itself if it overflows
//                again: two at most as wave_search stands. The capacity counts the wave and both
//                halves so that it does not depend on that either-or.
constexpr int64_t follow_waves(int64_t n) { return (n + 63) / 64; }
constexpr int64_t kHalvesPerWave = 2, kWidePerWave = 3;
struct FollowLayout {
  int64_t exact, ball, halves, wide, end;  // first int of each list; end: one past the last list
};
constexpr FollowLayout follow_layout(int64_t n) {
  FollowLayout l{};
  l.exact = 0;
  l.ball = l.exact + n;
  l.halves = l.ball + n;
  l.wide = l.halves + follow_waves(n) * kHalvesPerWave * kHalfEntryInts;
  l.end = l.wide + follow_waves(n) * kWidePerWave * kWideEntryInts;
  return l;
}
constexpr int64_t follow_list_ints(int64_t n) { return follow_layout(n).end; }

// The regions in order, each as long as its capacity, all inside follow_list_ints(n), which stays
// within 3 n + 64 ints (12 B per query).
constexpr bool follow_layout_ok(int64_t n) {
  const FollowLayout l = follow_layout(n);
  const int64_t w = follow_waves(n);
  return l.exact >= 0 && l.exact + n <= l.ball && l.ball + n <= l.halves &&
         l.halves + w * kHalvesPerWave * kHalfEntryInts <= l.wide &&
         l.wide + w * kWidePerWave * kWideEntryInts <= l.end && l.end == follow_list_ints(n) && 64 * w >= n &&
         l.end <= 3 * n + 64;
}
static_assert(follow_layout_ok(1) && follow_layout_ok(63) && follow_layout_ok(64) && follow_layout_ok(65),
              "follow-up lists overlap or overrun");
static_assert(follow_layout_ok(((int64_t)1 << 28) - 1) && follow_layout_ok((int64_t)1 << 28),
              "follow-up lists overlap or overrun at a full slice");

// The lists of a search over n queries inside `ints` (follow_list_ints(n) ints) and `guesses` (n
// doubles). Which pass is on is the caller's rule; an off pass has no list.
inline FollowLists carve_follow_lists(int32_t* ints, double* guesses, FollowCounts* counts, int64_t n, bool halves_on,
                                      bool wide_on) {
  const FollowLayout l = follow_layout(n);
  FollowLists f;
  f.exact = ints + l.exact;
  f.ball = ints + l.ball;
  f.ball_u = guesses;
  f.n = counts;
  f.halves = halves_on ? ints + l.halves : nullptr;
  f.wide = wide_on ? ints + l.wide : nullptr;
  return f;
}

}  // namespace icp
