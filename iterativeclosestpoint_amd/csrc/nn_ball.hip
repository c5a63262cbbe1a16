// nn_ball.hip — the searches around the wave search (nn_kernels.hip), all fp64, no FMA:
//  k_nn_ref      one thread per query, the literal reference-order DFS (the parity kernel, and the
//                work counter of the roofline's "reference work" figure).
//  k_nn_ball     the follow-up search: the queries a wave did not take, four per wave (16-lane
//                groups), sphere walks; what those cannot decide, and the wave search's exact list:
//                per-lane certified search, else the reference-order DFS.
//  k_target_sep  once per target: every point's separation from the others (TgtPt::sep).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "nn_device.h"

namespace icp {
namespace {
using namespace dev;

// The reference-order kernel.
template <bool APPLY, bool COUNT>
__global__ void __launch_bounds__(256) k_nn_ref(NNLaunch a) {
  if (a.loop && a.loop->core.done) return;  // the device loop's session finished
  extern __shared__ __attribute__((aligned(16))) unsigned long long lds_stack[];
  const int bs = blockDim.x;
  const int64_t i = (int64_t)blockIdx.x * bs + threadIdx.x;
  const bool active = i < a.n;

  double qx = 0.0, qy = 0.0, qz = 0.0;
  load_query<APPLY>(a, i, active, qx, qy, qz);

  double best_d2 = a.init_best;
  int32_t best = -1;
  double visits = 0.0, scanned = 0.0;
  // A NaN coordinate makes every leaf distance NaN, so the reference never updates best_idx
  // (octree.cpp:146): skipping the search is exact. (Its box distances stay finite: max(0,NaN)=0.)
  const bool nan_q = (qx != qx) || (qy != qy) || (qz != qz);
  if (active && !nan_q && a.n_nodes > 0)
    exact_dfs<COUNT>(a, qx, qy, qz, lds_stack + threadIdx.x, bs, best, best_d2, visits, scanned);
  if (active) {
    const int32_t pos = best >= 0 ? best : a.pos0;
    a.pos_out[i] = pos;
    a.dist_out[i] = best >= 0 ? __builtin_sqrt(best_d2)  // == computeDistance bit for bit
                              : residual_to(a.pts, a.pos0, qx, qy, qz);
  }
  if (COUNT) {
    __syncthreads();  // every traversal is done: reuse the stack LDS for the reduction
    double c[2] = {visits, scanned};
    block_sum<2>(c, reinterpret_cast<double*>(lds_stack));
    if (threadIdx.x == 0) {
      atomicAdd(&a.counters[0], (unsigned long long)c[0]);
      atomicAdd(&a.counters[1], (unsigned long long)c[1]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The ball search: four queries per wave, one 16-lane group (a DPP row) each. The list's queries
// are latency-bound walks of a few dependent rounds, so four in flight per wave hide four times
// the latency of one. A group collects, breadth-first from the cell tables of the query's box,
// every leaf whose box distance s <= u (1 + 2^-47) (a sphere test) and scans their points one per
// lane. Leaves with s > u (1 + 2^-47) only hold points with fl(d2) > best (1 + 2^-48) (monotone
// rounding), so nothing in the certificate window is missed. Certification as in the wave search
// (best <= u and the window test). A query the group cannot decide (no usable guess, an
// overflowing candidate set, or no certificate) is finished right there by the group's first lane:
// the per-lane certified search, else the reference-order DFS (stack in the group's LDS).
// Before that, the kernel's threads take the exact list the wave search left, one query each
// (the reference-order DFS). One launch for all the follow-up searches.
constexpr int kBallGroups = 4;
constexpr int kBallGL = 64 / kBallGroups;  // lanes per query
constexpr int kBallStack = 512;
constexpr int kBallPoints = 1024;
constexpr int kBallGStack = kBallStack / kBallGroups;
constexpr int kBallGPoints = kBallPoints / kBallGroups;
constexpr int kBallLdsBytes = kBallStack * 4 + kBallPoints * 4;

// The reference-order DFS for query i (octree.cpp:128-184), its result written.
__device__ __forceinline__ void exact_query(const NNLaunch& a, int64_t i, unsigned long long* st, int bs) {
  const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
  double best_d2 = a.init_best, visits = 0.0, scanned = 0.0;
  int32_t best = -1;
  exact_dfs<false>(a, qx, qy, qz, st, bs, best, best_d2, visits, scanned);
  a.pos_out[i] = best >= 0 ? best : a.pos0;
  a.dist_out[i] = best >= 0 ? __builtin_sqrt(best_d2) : residual_to(a.pts, a.pos0, qx, qy, qz);
}

// The per-lane certified search for query i; a query it cannot certify gets the reference-order
// DFS right away. budget > 0: a search that needs more node visits gives up (returns false, nothing
// written: the wave-cooperative search takes it).
// *found: the best fl(d2) it had found when it gave up (a point's: an upper bound for the next search).
// u: an upper bound of the nearest fl(d2) (inf: none), the search's initial prune bound.
__device__ __forceinline__ bool lane_query(const NNLaunch& a, int64_t i, unsigned long long* st, int bs,
                                           int budget = 0, double* found = nullptr, double u = __builtin_inf()) {
  const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
  double best = __builtin_inf(), second = __builtin_inf();
  int32_t bpos = -1;
  const double thr0 = u <= 0x1p900 ? u * (1.0 + kFastPrune) : __builtin_inf();
  if (!fast_dfs(a, qx, qy, qz, st, bs, best, second, bpos, budget, thr0)) {
    if (found) *found = best;
    return false;
  }
  if (certified(best, second, a.init_best)) {
    a.pos_out[i] = bpos;
    a.dist_out[i] = __builtin_sqrt(best);
  } else {
    exact_query(a, i, st, bs);
    atomicAdd(&a.follow.n->dfs_finishes, 1u);  // a DFS finish of the ball search
    if (a.dbg) atomicAdd(&a.dbg[ICP_DBG_LANE_EXACT], 1ull);
  }
  return true;
}

// Node visits a per-lane follow-up search may take before the wave-cooperative search takes over.
// A query far (relative to the local point spacing) from a dense surface needs every leaf whose
// box comes within its nearest distance: on the scene workload's outliers (metres above a ground
// sampled every few mm) up to ~30k visits of one lane, ~1 us of dependent loads each (the
// reference's DFS needs as many: tools/scene_probe.py). A wave's queue runs its lanes' searches
// together, so the longest one sets its time: the budget bounds that, and the cooperative search
// (64 nodes a step) takes the rest. Measured (profiles/r21/ab_lane_budget.txt, scene 20/5): 768
// -> 64 visits: 1M 320 -> 635 Mcorr/s, 10M 600 -> 677; config 4 and config 3 unchanged.
#ifndef ICP_LANE_BUDGET
#define ICP_LANE_BUDGET 64
#endif
constexpr int kLaneBudget = ICP_LANE_BUDGET;
constexpr int kBBStack = 2048;  // the cooperative search's node stack (int32 in LDS), the last
constexpr int kBBPts = 256;     // kBBPts entries of which hold a step's leaf points

// The wave-cooperative certified search of one query (every lane of the wave): branch and bound
// over the octree, up to 64 nodes per step (one per lane, LIFO), each node re-tested against the
// prune bound thr = best (1 + 2^-47) of the wave's best so far (exact as fast_dfs: a node is
// skipped only when its squared box distance s exceeds thr, so every point of the certificate
// window is scanned), leaves scanned by their lane, the best reduced over the wave every step.
// u: an upper bound of the query's nearest fl(d2) (inf: none). A frontier that outgrows the stack
// (a far query under a loose bound: every node within the bound is live) is searched again from
// the root with the best point found so far as the bound, which prunes the frontier to the nodes
// within the nearest distance (up to kBBPasses times while the bound shrinks). Returns false when
// it still overflows and 2 for a tie (nothing written either way: the caller runs the
// reference-order DFS), 1 after writing the certified result.
constexpr int kBBPasses = 4;
constexpr int kBBDone = 1;
__device__ __forceinline__ int wave_bb(const NNLaunch& a, int64_t i, double u, int32_t* stack, int lane) {
  const double qx = a.x[i], qy = a.y[i], qz = a.z[i];
  double best = __builtin_inf(), second = __builtin_inf();
  int32_t bpos = 0x7fffffff;
  int32_t* plist = stack + (kBBStack - kBBPts);
  double thr = (u <= 0x1p900) ? u * (1.0 + kFastPrune) : __builtin_inf();
  int steps = 0, passes = 0;
  bool over = false;
  while (true) {
    // a pass: every point it scans is counted once (best, second from this pass only)
    best = __builtin_inf();
    second = __builtin_inf();
    bpos = 0x7fffffff;
    const double thr0 = thr;
    // the start nodes: the cell-table nodes of the box q +- sqrt(thr) (every point within the
    // bound lies in it: the ball search's radius), else the root; the descent's levels skipped
    int tail = 1;
    if (a.cells && thr <= 0x1p900) {
      const double amax = __builtin_fmax(__builtin_fabs(qx), __builtin_fmax(__builtin_fabs(qy), __builtin_fabs(qz)));
      const double r = __builtin_sqrt(thr) * (1.0 + 0x1p-40) + amax * 0x1p-45;
      tail = cell_starts<64, 2>(a, qx - r, qy - r, qz - r, qx + r, qy + r, qz + r, lane, 0, stack);
    } else if (lane == 0) {
      stack[0] = 0;
    }
    over = false;
    ++passes;
    wave_lds_fence();
    while (tail > 0) {
      const int batch = tail < 64 ? tail : 64;
      const bool has = lane < batch;
      const int32_t nid = has ? stack[tail - batch + lane] : 0;
      tail -= batch;
      const NodeRec* rr = a.nodes + nid;
      const int2 topo = *reinterpret_cast<const int2*>(&rr->first);
      const uint32_t meta = (uint32_t)topo.y;
      // pushed against an older (larger) bound, and pushed by its cell: test the node's tight box
      const float4 tb0 = *reinterpret_cast<const float4*>(&a.tbox[nid].lo[0]);
      const float2 tb1 = *reinterpret_cast<const float2*>(&a.tbox[nid].hi[1]);
      const bool live = has && !(box_s(tb0.x, tb0.y, tb0.z, tb0.w, tb1.x, tb1.y, qx, qy, qz) > thr);
      const bool lf = live && (meta & kLeafBit);
      const uint32_t kids = (live && !lf) ? children_in_ball(rr, meta & 0xffu, qx, qy, qz, thr) : 0u;
      // The step's leaf points, flat: listed in LDS kBBPts at a time and scanned kBBPts / 64 per
      // lane with all their loads in flight together (a leaf scanned by its own lane was ~10
      // dependent round trips per step). Each point is scanned by one lane: the per-lane best and
      // second reduce to the wave's exactly as before.
      const int lcnt = lf ? (int)(meta & ~kLeafBit) : 0;
      int ltot;
      const int lfirst = wave_incl_scan(lcnt, &ltot) - lcnt;
      for (int base = 0; base < ltot; base += kBBPts) {
        for (int k = 0; k < lcnt; k++) {
          const int f = lfirst + k - base;
          if (f >= 0 && f < kBBPts) plist[f] = topo.x + k;
        }
        wave_lds_fence();
        const int m = ltot - base < kBBPts ? ltot - base : kBBPts;
        constexpr int P = kBBPts / 64;
        double px[P], py[P], pz[P];
        int32_t pid[P];
#pragma unroll
        for (int t = 0; t < P; t++) {
          pid[t] = t * 64 + lane < m ? plist[t * 64 + lane] : -1;
          const TgtPt* p = a.pts + (pid[t] >= 0 ? pid[t] : 0);
          const double2 pxy = *reinterpret_cast<const double2*>(&p->x);
          const double2 pzw = *reinterpret_cast<const double2*>(&p->z);
          px[t] = pxy.x;
          py[t] = pxy.y;
          pz[t] = pzw.x;
          pid[t] = tgt_copy_word(pzw.y) ? -1 : pid[t];  // a copy: its earlier twin is scanned
        }
#pragma unroll
        for (int t = 0; t < P; t++) {
          const double dx = px[t] - qx, dy = py[t] - qy, dz = pz[t] - qz;
          const double d2 = dx * dx + dy * dy + dz * dz;
          if (pid[t] >= 0) {
            if (d2 < best) {
              second = best;
              best = d2;
              bpos = pid[t];
            } else if (d2 < second) {
              second = d2;
            }
          }
        }
        wave_lds_fence();  // the list's reads are done before the next round rewrites it
      }
      const int nch = __builtin_popcount(kids);
      int tot;
      const int incl = wave_incl_scan(nch, &tot);
      if (tail + tot > kBBStack - kBBPts) {
        over = true;
        break;
      }
      wave_lds_fence();  // this step's pops are read before the pushes overwrite them
      int off = tail + incl - nch;
      uint32_t kk = kids;
      while (kk) {
        const uint32_t o = (uint32_t)__builtin_ctz(kk);
        kk &= kk - 1u;
        stack[off++] = topo.x + __builtin_popcount((meta & 0xffu) & ((1u << o) - 1u));
      }
      tail += tot;
      const double gb = wave_min_d(best);
      const double t2 = gb * (1.0 + kFastPrune);
      thr = t2 < thr ? t2 : thr;
      ++steps;
      wave_lds_fence();
    }
    wave_lds_fence();
    // again with the tighter bound (thr holds the best so far), while it shrinks
    if (!over || passes >= kBBPasses || !(thr < thr0)) break;
  }
  if (a.dbg && lane == 0) {
    atomicAdd(&a.dbg[ICP_DBG_BB_QUERIES], 1ull);
    atomicAdd(&a.dbg[ICP_DBG_BB_STEPS], (unsigned long long)steps);
    if (over) atomicAdd(&a.dbg[ICP_DBG_BB_OVERFLOW], 1ull);
  }
  if (over) return 0;
  // the wave's best, and its second: the smallest of the other lanes' bests and the best lane's
  // second (a best held by two lanes is its own second: a tie)
  const double gb = wave_min_d(best);
  const unsigned long long at = wballot(best == gb);
  const double gs = __popcll(at) > 1 ? gb : wave_min_d(best == gb ? second : best);
  const int32_t gp = (int32_t)__builtin_amdgcn_readlane(bpos, __builtin_ctzll(at ? at : 1ull));
  if (!certified(gb, gs, a.init_best)) return 2;
  if (lane == 0) {
    a.pos_out[i] = gp;
    a.dist_out[i] = __builtin_sqrt(gb);
  }
  return kBBDone;
}

__global__ void __launch_bounds__(64) k_nn_ball(NNLaunch a) {
  if (a.loop && a.loop->core.done) return;
  const FollowLists& L = a.follow;
  extern __shared__ __attribute__((aligned(16))) unsigned long long lds_raw[];
  const int lane = threadIdx.x, g = lane / kBallGL, gl = lane % kBallGL, gbase = g * kBallGL;
  int32_t* stack = reinterpret_cast<int32_t*>(lds_raw) + g * kBallGStack;
  int32_t* plist = reinterpret_cast<int32_t*>(lds_raw) + kBallStack + g * kBallGPoints;
  // The exact list (queries the wave search could not certify): complete when this kernel starts,
  // one thread each, a DFS stack of `levels` entries per thread in LDS.
  {
    const unsigned n0 = L.n->exact;
    for (unsigned j = blockIdx.x * 64u + (unsigned)lane; j < n0; j += gridDim.x * 64u)
      exact_query(a, L.exact[j], lds_raw + lane, 64);
    wave_lds_fence();
  }
  // The follow-ups of the ball queries (a per-lane certified search, or the reference-order DFS)
  // are queued per wave and run 64 at a time, one query per lane with its own DFS stack column
  // (the exact list's layout), once the queue is nearly full and at the end. (One lane of the
  // query's group ran each inline before: 1 lane in 16 busy. On a dense 2.5-D scan early in a
  // registration the queries sit ~0.3 m off surfaces sampled every few mm, every ball overflows,
  // and that serial tail took 21 ms per iterate at 1M points.)
  int32_t* fq = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(lds_raw) + a.ball_queue_off);
  double* fqu = reinterpret_cast<double*>(fq + 64);  // each entry's guess u (an upper bound, or inf)
  int qn = 0;  // wave-uniform
  // A per-lane search that exceeds kLaneBudget node visits is handed to the wave-cooperative
  // search (the whole wave on one query), one after the other once the lanes are done.
  auto flush = [&]() {
    wave_lds_fence();
    bool handed = false;
    int32_t e = 0;
    double qu = __builtin_inf();
    if (lane < qn) {
      e = fq[lane];
      qu = fqu[lane];
      const int64_t iq = e & 0x3fffffff;
      // an abandoned search's best so far (a point's fl(d2)) bounds the cooperative search
      double found = __builtin_inf();
      if ((e >> 30) == 1) handed = !lane_query(a, iq, lds_raw + lane, 64, kLaneBudget, &found, qu);
      else exact_query(a, iq, lds_raw + lane, 64);
      qu = found < qu ? found : qu;
    }
    wave_lds_fence();
    const unsigned long long handed_m = wballot(handed);
    if (a.dbg && lane == 0) atomicAdd(&a.dbg[ICP_DBG_LANE_HANDED], (unsigned long long)__popcll(handed_m));
    for (unsigned long long hm = wballot(handed); hm; hm &= hm - 1) {
      const int k = __builtin_ctzll(hm);
      const int64_t iq = __builtin_amdgcn_readlane(e, k) & 0x3fffffff;
      const double uq = readlane_d(qu, k);
      // the stack in the DFS columns' area (free now); a tie or an overflow: the reference-order
      // DFS on lane 0, in the same area
      if (wave_bb(a, iq, uq, reinterpret_cast<int32_t*>(lds_raw), lane) != kBBDone && lane == 0) {
        exact_query(a, iq, lds_raw, 1);
        atomicAdd(&L.n->dfs_finishes, 1u);
        if (a.dbg) atomicAdd(&a.dbg[ICP_DBG_LANE_EXACT], 1ull);
      }
      wave_lds_fence();
    }
    qn = 0;
    wave_lds_fence();
  };
  const unsigned cnt = L.n->ball;
  // Direct mode: each wave takes whole queries, one after the other, with all its lanes: the
  // cooperative search started from the cell tables of the query's bound (a few 64-node steps
  // instead of the 16-lane ball walk and the follow-ups after it). Used for a long list (over four
  // per wave: an unconverged registration on surface data, where most balls overflow) and after
  // the wide pass; the four-queries-per-wave ball walk takes the shorter lists, whose queries are
  // mostly easy. (Short lists, at most one query per wave, went to the direct mode too until r23:
  // since the flat leaf scans of r22 the ball walk settles them faster, config 3 6.2k -> 7.4k,
  // config 2 1.35k -> 1.41k Mcorr/s, profiles/r23/ab_ball_mode_configs23.txt.) Measured (profiles/r21/ab_ball_direct.txt): scene 10M 678 -> 1215 Mcorr/s,
  // scene 1M 624 -> 1254 (driver window), config 4 unchanged; direct at every size cost config
  // 4's window 4 % (its 15k-query lists of easy balls).
  // (icp_hip_config.ball_mode: 0 this rule, 1 the ball walk always, 2 direct always)
  if (a.ball_mode == 2 || (a.ball_mode == 0 && cnt > 4u * gridDim.x)) {
    // A query the cooperative search leaves (a tie, an overflow) is queued for the reference-order
    // DFS; the queue runs 64 at a time, one per lane, each with its DFS stack column in LDS (ties
    // come in numbers where both clouds sit on the LAS grid: the source's first iterate)
    unsigned taken = 0;
    int dq = 0;  // wave-uniform
    auto dfs_flush = [&]() {
      wave_lds_fence();
      if (lane < dq) exact_query(a, fq[lane], lds_raw + lane, 64);
      if (lane == 0) {
        atomicAdd(&L.n->dfs_finishes, (unsigned)dq);
        if (a.dbg) atomicAdd(&a.dbg[ICP_DBG_LANE_EXACT], (unsigned long long)dq);
      }
      dq = 0;
      wave_lds_fence();
    };
    for (unsigned j = blockIdx.x; j < cnt; j += gridDim.x, ++taken) {
      const int64_t i = L.ball[j];
      const double u = L.ball_u[j];
      if (wave_bb(a, i, u, reinterpret_cast<int32_t*>(lds_raw), lane) != kBBDone) {
        wave_lds_fence();
        if (lane == 0) fq[dq] = (int32_t)i;
        if (++dq == 64) dfs_flush();
      }
      wave_lds_fence();
    }
    if (dq > 0) dfs_flush();
    // the queries taken by the cooperative search count as follow-up searches, as after the ball
    // walk (icp_iter_stats.n_lane_search)
    if (lane == 0 && taken > 0) atomicAdd(&L.n->lane_searches, taken);
    return;
  }
  for (unsigned j0 = blockIdx.x * kBallGroups; j0 < cnt; j0 += gridDim.x * kBallGroups) {
    const unsigned j = j0 + g;
    bool live = j < cnt;  // group-uniform
    int follow = 0;       // group-uniform: 1 the per-lane search, 2 the reference-order DFS
    int64_t i = 0;
    double u = 0.0, qx = 0.0, qy = 0.0, qz = 0.0;
    if (live) {
      i = L.ball[j];
      u = L.ball_u[j];
      qx = a.x[i];
      qy = a.y[i];
      qz = a.z[i];
      if (!(u <= 0x1p900)) {
        follow = 1;
        live = false;
      }
    }
    const double thr = u * (1.0 + kFastPrune);
    int tail = 0, npts = 0;
    bool overflow = false;
    wave_lds_fence();
    {
      // every point with fl(d2) <= thr lies in the box q +- r (see the wave search's radius)
      const double amax = __builtin_fmax(__builtin_fabs(qx), __builtin_fmax(__builtin_fabs(qy), __builtin_fabs(qz)));
      const double r = live ? __builtin_sqrt(thr) * (1.0 + 0x1p-40) + amax * 0x1p-45 : 0.0;
      if (a.cells) {
        const int t = cell_starts<kBallGL, 1>(a, qx - r, qy - r, qz - r, qx + r, qy + r, qz + r, gl, gbase, stack);
        tail = live ? t : 0;
      } else {
        if (gl == 0) stack[0] = 0;
        tail = live ? 1 : 0;
      }
    }
    wave_lds_fence();
    // LIFO batches of up to 16 nodes per group, sphere test s <= thr on the children
    while (wballot(tail > 0) != 0) {
      const int batch = tail < kBallGL ? tail : kBallGL;
      const bool has = gl < batch;
      bool leaf = false;
      int32_t first = 0;
      uint32_t meta = 0, kids = 0;
      if (has) {
        const NodeRec* rr = a.nodes + stack[tail - batch + gl];
        const int2 topo = *reinterpret_cast<const int2*>(&rr->first);
        first = topo.x;
        meta = (uint32_t)topo.y;
        leaf = (meta & kLeafBit) != 0;
        if (!leaf) kids = children_in_ball(rr, meta & 0xffu, qx, qy, qz, thr);
      }
      const int lcnt = (has && leaf) ? (int)(meta & ~kLeafBit) : 0;
      int ltot;
      const int lincl = row_incl_scan(lcnt, gbase, &ltot);
      const int lpos = npts + lincl - lcnt;
      if (lcnt > 0 && lpos + lcnt <= kBallGPoints)
        for (int c = 0; c < lcnt; c++) plist[lpos + c] = first + c;
      const int nch = __builtin_popcount(kids);
      int tot;
      const int incl = row_incl_scan(nch, gbase, &tot);
      if (tail > 0) {
        npts += ltot;
        tail -= batch;
        if (npts > kBallGPoints || tail + tot > kBallGStack) {
          overflow = true;
          tail = 0;
        } else {
          int off = tail + incl - nch;
          const uint32_t mask = meta & 0xffu;
          uint32_t kk = kids;
          while (kk) {
            const uint32_t o = (uint32_t)__builtin_ctz(kk);
            kk &= kk - 1u;
            stack[off++] = first + __builtin_popcount(mask & ((1u << o) - 1u));
          }
          tail += tot;
        }
      }
      wave_lds_fence();
    }
    if (a.dbg && gl == 0 && live) {
      atomicAdd(&a.dbg[ICP_DBG_BALL_OVERFLOW], overflow ? 1ull : 0ull);
      atomicAdd(&a.dbg[ICP_DBG_BALL_POINTS], (unsigned long long)npts);
    }
    if (live && overflow) follow = 1;
    if (overflow) live = false;
    wave_lds_fence();
    double best = __builtin_inf(), second = __builtin_inf();
    int32_t bpos = 0x7fffffff;
    if (live) {
      for (int k = gl; k < npts; k += kBallGL) {
        const int32_t pg = plist[k];
        const double d2 = d2_to(a.pts + pg, qx, qy, qz);
        if (d2 < best) {
          second = best;
          best = d2;
          bpos = pg;
        } else if (d2 < second) {
          second = d2;
        }
      }
    }
#pragma unroll
    for (int o = kBallGL / 2; o >= 1; o >>= 1) {
      const double ob = __shfl_xor(best, o, kWave);
      const double os = __shfl_xor(second, o, kWave);
      const int32_t op = __shfl_xor(bpos, o, kWave);
      const double lo_ = ob < best ? ob : best;
      const double hi_ = ob < best ? best : ob;
      const double ss = os < second ? os : second;
      second = hi_ < ss ? hi_ : ss;
      bpos = (ob < best || (ob == best && op < bpos)) ? op : bpos;
      best = lo_;
    }
    if (live) {
      if (!(best <= u)) {
        follow = 1;
      } else if (certified(best, second, a.init_best)) {
        if (gl == 0) {
          a.pos_out[i] = bpos;
          a.dist_out[i] = __builtin_sqrt(best);
        }
      } else {
        follow = 2;
      }
    }
    // queue the follow-ups (one entry per group: its leader lane)
    const bool fol = follow != 0 && gl == 0;
    const unsigned long long fm = wballot(fol);
    if (fol) {
      atomicAdd(follow == 1 ? &L.n->lane_searches : &L.n->dfs_finishes, 1u);  // counted for the iteration record
      fq[qn + mask_rank(fm)] = (int32_t)i | (follow << 30);
      // an overflowing ball's guess bounds the nearest distance (a guess the ball did not cover
      // does not, nor does an unusable one)
      fqu[qn + mask_rank(fm)] = (overflow && u <= 0x1p900) ? u : __builtin_inf();
    }
    qn += __popcll(fm);
    if (qn > 64 - kBallGroups) flush();
    wave_lds_fence();
  }
  if (qn > 0) flush();
}

// ---------------------------------------------------------------------------------------------
// Separation of the target points (once per target): for every point p_j a lower bound S_j of its
// exact distance to every OTHER target point, stored in TgtPt::sep (fp32, rounded down; 0 when
// p_j has an exact duplicate). It turns the previous match into a certificate (k_nn_wave,
// icp_hip_config.certify_prev): a moved query q' with exact distance D* to its previous match p*
// has D(q', p) >= S - D* for every other point p (triangle inequality), so p* is the nearest with
// the reference's own certificate (nn_device.h) whenever (S - D*)^2 clears fl(d2(q', p*)) by the
// window. One thread per point (leaf order: neighbours in flight together), a branch-and-bound
// DFS for the nearest point other than itself: nearest child first, the remaining siblings of a
// level kept as one stack entry with a 16-bit lower-bound key (fast_dfs's encoding); a node is
// skipped when its squared box distance s exceeds the best (monotone rounding: every point inside
// has fl(d2) >= s), so the result is the exact minimum fl(d2) over the other points.
__global__ void __launch_bounds__(256) k_target_sep(const NodeRec* __restrict__ nodes, TgtPt* __restrict__ pts,
                                                    int64_t n) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sep_stack[];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;  // no barriers below
  unsigned long long* st = sep_stack + threadIdx.x;
  const int bs = blockDim.x;
  const double2 qxy = *reinterpret_cast<const double2*>(&pts[j].x);
  const double qx = qxy.x, qy = qxy.y, qz = pts[j].z;
  double best = __builtin_inf();
  uint32_t thr_key = key16(best);
  int sp = 0;
  int32_t node = 0;
  double lx = nodes[0].lo[0], ly = nodes[0].lo[1], lz = nodes[0].lo[2];
  double hx = nodes[0].hi[0], hy = nodes[0].hi[1], hz = nodes[0].hi[2];
  double s = box_s(lx, ly, lz, hx, hy, hz, qx, qy, qz);
  while (true) {
    bool entered = false;
    if (!(s > best)) {
      const int2 topo = *reinterpret_cast<const int2*>(&nodes[node].first);
      const int32_t first = topo.x;
      const uint32_t meta = (uint32_t)topo.y;
      if (meta & kLeafBit) {
        const int32_t cnt = (int32_t)(meta & ~kLeafBit);
        for (int32_t k = 0; k < cnt; k++) {
          if ((int64_t)first + k == j) continue;
          const double d2 = d2_to(pts + first + k, qx, qy, qz);
          if (d2 < best) {
            best = d2;
            thr_key = key16(best);
          }
        }
      } else {
        const OctantDist od = octant_dist(lx, ly, lz, hx, hy, hz, qx, qy, qz);
        const uint32_t mask = meta & 0xffu;
        double bs_ = __builtin_inf();
        uint32_t o1 = 0;
#pragma unroll
        for (int o = 0; o < 8; o++) {
          const double c = od.of(o);
          const bool take = ((mask >> o) & 1u) && c < bs_;
          bs_ = take ? c : bs_;
          o1 = take ? (uint32_t)o : o1;
        }
        const uint32_t rem = mask & ~(1u << o1);
        uint32_t kmin = 0xffffu;
#pragma unroll
        for (int o = 0; o < 8; o++) {
          const uint32_t kk = key16(od.of(o));
          kmin = ((rem >> o) & 1u) && kk < kmin ? kk : kmin;
        }
        if (rem) {
          st[sp * bs] = ((unsigned long long)kmin << 48) | ((unsigned long long)mask << 40) |
                        ((unsigned long long)rem << 32) | (uint32_t)first;
          sp++;
        }
        node = first + __builtin_popcount(mask & ((1u << o1) - 1u));
        if (o1 & 1u) lx = od.mx; else hx = od.mx;
        if (o1 & 2u) ly = od.my; else hy = od.my;
        if (o1 & 4u) lz = od.mz; else hz = od.mz;
        s = bs_;
        entered = true;
      }
    }
    if (entered) continue;
    bool found = false;
    while (sp > 0) {
      const unsigned long long e = st[(sp - 1) * bs];
      if ((uint32_t)(e >> 48) > thr_key) {  // key16 is monotone: every remaining child has s > best
        sp--;
        continue;
      }
      uint32_t rem = (uint32_t)(e >> 32) & 0xffu;
      const uint32_t pmask = (uint32_t)(e >> 40) & 0xffu;
      const int32_t first = (int32_t)(uint32_t)e;
      const uint32_t o = (uint32_t)__builtin_ctz(rem);
      rem &= rem - 1u;
      if (rem == 0) sp--;
      else st[(sp - 1) * bs] = (e & ~(0xffull << 32)) | ((unsigned long long)rem << 32);
      node = first + __builtin_popcount(pmask & ((1u << o) - 1u));
      const NodeBox nb = load_node_box(nodes + node);
      lx = nb.l01.x; ly = nb.l01.y; lz = nb.l2h0.x; hx = nb.l2h0.y; hy = nb.h12.x; hz = nb.h12.y;
      s = box_s(lx, ly, lz, hx, hy, hz, qx, qy, qz);
      found = true;
      break;
    }
    if (!found) break;
  }
  // fl(d2) <= D^2 (1 + 5 2^-53), so D >= sqrt(best) (1 - 2^-50) (the fp64 sqrt within an ulp);
  // the fp32 conversion rounds by <= 2^-24, covered by the 2^-22 factor: sep <= D
  float sep = __builtin_inff();
  if (best < __builtin_inf()) sep = (float)(__builtin_sqrt(best) * ((1.0 - 0x1p-50) * (1.0 - 0x1p-22)));
  if (!(sep >= 0.0f)) sep = 0.0f;
  pts[j].sep = sep;
}

inline unsigned grid_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace

int nn_block_threads(int levels) {
  // LDS stack of the per-thread kernels: levels x threads x 8 B. Keep <= 64 KiB per block.
  if (levels <= 32) return 256;
  if (levels <= 64) return 128;
  return 64;
}

hipError_t launch_target_sep(const NodeRec* nodes, TgtPt* pts, int64_t n, int levels, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int lv = levels < 1 ? 1 : levels;
  const int bs = nn_block_threads(lv);
  const size_t shmem = (size_t)lv * bs * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_target_sep, dim3(grid_for(n, bs)), dim3(bs), shmem, s, nodes, pts, n);
  return hipGetLastError();
}

hipError_t launch_nn_ref(const NNLaunch& a, hipStream_t s) {
  const int levels = a.levels < 1 ? 1 : a.levels;
  const int bs = nn_block_threads(levels);
  size_t shmem = (size_t)levels * bs * sizeof(unsigned long long);
  if (shmem < 1024) shmem = 1024;  // also hosts the block reduction
  const unsigned grid = grid_for(a.n, bs);
  if (a.ev_start) (void)hipEventRecord(a.ev_start, s);
  if (a.apply) {
    if (a.count) hipLaunchKernelGGL((k_nn_ref<true, true>), dim3(grid), dim3(bs), shmem, s, a);
    else hipLaunchKernelGGL((k_nn_ref<true, false>), dim3(grid), dim3(bs), shmem, s, a);
  } else {
    if (a.count) hipLaunchKernelGGL((k_nn_ref<false, true>), dim3(grid), dim3(bs), shmem, s, a);
    else hipLaunchKernelGGL((k_nn_ref<false, false>), dim3(grid), dim3(bs), shmem, s, a);
  }
  if (a.ev_fast_done) (void)hipEventRecord(a.ev_fast_done, s);
  return hipGetLastError();
}

hipError_t launch_nn_follow(const NNLaunch& a, hipStream_t s) {
  // the follow-up lists are short (the ball list ~0.1 % of the queries, the exact list usually
  // empty): one launch of 64-thread blocks, grid-stride over them; LDS for the group stacks and
  // lists or, before them, one DFS stack of `levels` entries per thread
  const int levels = a.levels < 1 ? 1 : a.levels;
  const int64_t bq = (a.n + kBallGroups - 1) / kBallGroups;
  size_t bshm = (size_t)levels * 64 * sizeof(unsigned long long);
  if (bshm < (size_t)kBallLdsBytes) bshm = kBallLdsBytes;
  NNLaunch b = a;
  if (bshm < (size_t)kBBStack * sizeof(int32_t)) bshm = (size_t)kBBStack * sizeof(int32_t);  // wave_bb's stack
  b.ball_queue_off = (int32_t)bshm;  // the follow-up queue (64 entries + guesses) after the stacks and lists
  // after the wide pass the list holds what it left: far queries (lanes that joined no box, and
  // lanes the wide pass could not certify, with its bounds): whole queries per wave
  if (a.follow.wide && b.ball_mode == 0) b.ball_mode = 2;
  bshm += 64 * (sizeof(int32_t) + sizeof(double));
  hipExtLaunchKernelGGL(k_nn_ball, dim3((unsigned)(bq < 8192 ? bq : 8192)), dim3(64), (uint32_t)bshm, s, nullptr,
                        nullptr, 0u, b);
  return hipGetLastError();
}

}  // namespace icp
