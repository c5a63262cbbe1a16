// kernels.h — launch wrappers of the gfx950 kernels (nn_kernels.hip, nn_ball.hip,
// reduce_kernels.hip, util_kernels.hip). Internal C++ API used by the C-ABI context (icp_ctx.hip); no torch types.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/icp_hip.h"
#include "follow_lists.h"
#include "icp_common.h"
#include "session_step.h"

namespace icp {

// The device-resident loop's state (device memory): the session (engine.cpp's decisions,
// session_step.h) stepped by each iteration's last kernel; every kernel of a later iteration
// reads `done` and returns at once after the session finished, and the search applies core.T.
struct LoopDev {
  SessionCore core;
  SessionParams p;
};

// Per-iteration record. Device-resident copy written by the merge/finalize kernels (the cull
// kernel reads the threshold from it); the last kernel of the iteration stores the finished
// record into pinned host memory (IterPublish), the one host read of the iteration.
struct IterDev {
  Moments m_local;      // this rank's residual moments
  Moments m_global;     // merged over ranks (rank order)
  CovMoments c_local;   // this rank's valid-pair moments
  CovMoments c_global;  // merged over ranks
  double mean, sd, thr, rmse;
  double cshift[6];  // this iteration's shift of the pair sums (set with the threshold)
  // The band of the fused covariance sums (wave_stats.h), set at the end of every iterate for the
  // next one's search: it sums the pairs with d <= fz_lo with the shift fz_sh and marks those in
  // (fz_lo, fz_hi]. fz_ok = 0: no band (a new source, a non-finite threshold): full cull pass.
  double fz_lo, fz_hi, fz_thr, fz_ok;
  double fz_sh[6];
  double cull_mode;  // this iterate: 1 = the search's wave records + the band pairs, 0 = full cull
  double n_wide;     // this iterate: waves of the wave search whose candidate set overflowed
  double lists[3];   // this iterate: published_lists (follow_lists.h) of the search: exact, ball, per-lane
  double seq;        // host copy only: IterPublish::seq, stored last (the host polls this word)
};
static_assert(sizeof(IterDev) == 656, "82 doubles");
static_assert(offsetof(IterDev, seq) + sizeof(double) == sizeof(IterDev), "seq is the record's last word");

// One wave's covariance record, written by the wave search's epilogue when the band is set
// (wave_stats.h): the canonical sums of its pairs with d <= fz_lo (s: d^2, a - s, b - t, the 9
// products), their count, the mask of its band lanes; flag = 1: the wave did not settle every
// query itself (ball / exact / per-lane searches finish them): the cull kernel recomputes it.
struct WaveStat {
  double s[16];
  double cnt;
  unsigned long long bm;
  unsigned long long flag;
  double pad;
};
static_assert(sizeof(WaveStat) == 160, "WaveStat is 20 doubles");

// The wave search's candidate cache (one record per wave of 64 queries): the box B+ whose leaves'
// points were collected, their count and the generation (target / source upload) it belongs to.
// The entries are the points inside B+ as fp32 offsets from B+'s centre (the scan's own staging
// values) with the point's id in the fourth word: a reusing wave streams them, no gathers.
constexpr int kWaveCandCap = 1008;  // candidate points per wave (the walk's list in LDS; the cache)
// One wave's candidate-cache record: its stored box B+ (the scan frame is B+'s centre), the count
// of entries, the generation, and vmin = vol(B+) / candidate_loose (the loose test: reused only
// while vol(B) >= vmin). One 64-B line, loaded by lanes 0..7 of the wave with its query.
struct WaveBox {
  double lo[3];
  double hi[3];
  int32_t count;
  uint32_t gen;
  float vmin;
  uint32_t pad;
};
static_assert(sizeof(WaveBox) == 64, "one line, eight words");

struct NNLaunch {
  const LoopDev* loop;      // device loop (null: the host drives the iterate); T from loop->core.T
  const NodeRec* nodes;
  const TBox* tbox;         // tight boxes of the nodes (prune tests of the certified searches)
  const TgtPt* pts;
  double* x;
  double* y;
  double* z;
  int32_t* pos_out;
  double* dist_out;
  unsigned long long* counters;  // [node entries, leaf points] (count mode only)
  int64_t n;
  int32_t n_nodes;
  int32_t pos0;
  int32_t levels;
  double init_best;
  double T[12];             // row-major 3x4, used when apply != 0
  int apply;
  int count;                // reference-order kernel counting the reference DFS's work
  int search;               // ICP_SEARCH_CERTIFIED (wave search) / ICP_SEARCH_REFERENCE
  FollowLists follow;       // the follow-up lists and their counters (follow_lists.h)
  hipEvent_t ev_start;      // optional: the main search kernel's start and end, recorded by its
  hipEvent_t ev_fast_done;  // own dispatch (hipExtLaunchKernel: no marker packets between kernels)
  int have_prev;            // dist_out holds the previous residuals of these queries
  int scan32;               // fp32 filter scan with fp64 certification (0: fp64 scan)
  const int32_t* cells;     // per-level cell tables (octree_gpu.h), null = root descent
  int cell_lmax;            // deepest table level
  double root_lo[3], root_hi[3];  // root box (the octree's midpoint recursion starts here)
  unsigned long long* dbg;  // optional diagnostics of the wave search (ICP_DBG_* slots)
  double join_factor;       // a lane joins the wave box if its radius <= this x the mean radius
  int xcd_blocks;           // renumber the wave search's blocks XCD-contiguously
  int scan_groups;          // lane groups of the fp32 filter scan (1, 2, 4)
  WaveBox* wc_box;          // candidate cache (iterate only; null: every wave walks)
  float4* wc_ents;          // kWaveCandCap entries per wave: (x, y, z) - centre of B+ in fp32, id
  uint32_t wc_gen;          // records of this generation are valid
  double wc_margin;         // a walk collects the leaves of B enlarged by this x B's half-extent
  double wc_loose;          // a record is reused only while vol(B+) <= this x vol(B)
  double wc_lead;           // a stored B+ leads the wave's motion by this many iterates' displacement
  int certify_prev;         // previous-match certificate mode (icp_hip_config.certify_prev)
  WaveStat* wstat;          // per-wave covariance records (null: none; the cull pass does it all)
  const IterDev* fz;        // the band of this iterate (IterDev::fz_*)
  int32_t ball_queue_off;   // k_nn_ball: byte offset of its follow-up queue in LDS
  int32_t ball_mode;        // icp_hip_config.ball_mode (k_nn_ball's direct mode)
  // The prewalk (launch_prewalk): a wave that reuses its record leaves its box B here, as the
  // fp32 keys of its reduction in the record's frame (lo x, y, z, hi x, y, z, the iterate's stamp,
  // 0: two int4 per wave); null: no prewalk after this search.
  int4* wc_req;
  uint32_t wc_stamp;        // request records of this iterate carry this stamp
  hipEvent_t ev_fork;       // optional: recorded once the wave search and its second passes are enqueued
  double pw_look;           // a wave asks when B leaves B+ within this many iterates of this motion
  double* pw_list;          // the requests k_prewalk_filter kept: (B lo, hi in fp64, wave id, 0)
  unsigned int* pw_count;   // their number (may exceed pw_cap: entries past it were dropped)
  unsigned int pw_cap;      // capacity of pw_list
};
// (the launch record is a kernel argument: its layout is part of every search kernel's code)
static_assert(sizeof(NNLaunch) == 520 && offsetof(NNLaunch, ev_start) == 272,
              "NNLaunch's layout moved");

// Threads per block of the per-thread search kernels for a given stack depth.
int nn_block_threads(int levels);
// The correspondence search of one iterate (nn_kernels.hip): the reference-order kernel, or the
// wave search, its second passes and the follow-up search.
hipError_t launch_nn(const NNLaunch& a, hipStream_t s);
// The prewalk of the candidate cache (nn_kernels.hip), enqueued on a side stream `ps` after `fork`
// (the search of this iterate is done) and followed by `done`: the waves that reused their record
// but whose box is about to leave it (within a.pw_look iterates of this iterate's motion, on the
// side they move to) get a fresh record around their current box, as a walking wave would store
// it, before the next iterate's search is launched (which waits for `done`). a: the search's own
// launch record (host-driven iterates: a.loop is null).
hipError_t launch_prewalk(const NNLaunch& a, hipStream_t ps, hipEvent_t fork, hipEvent_t done);
// launch_nn's parts in nn_ball.hip: the reference-order kernel (k_nn_ref), and the follow-up search
// of the lists the wave search left (k_nn_ball; owns its LDS sizing and the ball_mode rule).
hipError_t launch_nn_ref(const NNLaunch& a, hipStream_t s);
hipError_t launch_nn_follow(const NNLaunch& a, hipStream_t s);
// TgtPt::sep of every target point (lower bound of its distance to every other point).
hipError_t launch_target_sep(const NodeRec* nodes, TgtPt* pts, int64_t n, int levels, hipStream_t s);
hipError_t launch_mark_copies(TgtPt* pts, int64_t n, hipStream_t s);
// TBox of every node (icp_common.h), deepest level first; max_depth: the deepest node's depth.
hipError_t launch_tight_boxes(const NodeRec* nodes, const TgtPt* pts, TBox* tb, int64_t n_nodes, int max_depth,
                              hipStream_t s);

struct CullLaunch {
  const LoopDev* loop;  // device loop: nothing to do once the session is done
  const double* x;
  const double* y;
  const double* z;
  const int32_t* pos;
  const TgtPt* pts;
  const IterDev* it;
  CovMoments* part;
  int64_t n;
  const double* dist;       // the residuals (the band's and the recomputed waves' pairs)
  const WaveStat* wstat;    // the search's wave records (null: it wrote none this iterate)
  int wpb;                  // search waves per cull block (set by launch_cull_tail)
};

// Residual moments of the settled queries in fixed parts (deterministic), then the merges.
int64_t moments_num_parts(int64_t n);
// Partial buffers need merge_scratch_entries(nparts) entries of fold scratch behind the partials.
int64_t merge_scratch_entries(int64_t nparts);

struct MomentsFinalize {
  double k_sigma;
  int iter;
  int engine_rules;
};
// Residual moments of the rank's queries (part sums) and their last merge level into it->m_local;
// with fin (no communicator) also mean/std/threshold and the cull's pair shift (it->cshift, from
// cl's first 64 queries). With a ticket counter (zero between launches) and at most 4096 parts
// the last block of the moments launch runs the last level itself (one launch instead of two).
// uints of the two "last block done" counters (moments, cull), zero-initialised once
int ticket_words();
hipError_t launch_moments_tail(const double* dist, int64_t n, Moments* part, const LoopDev* loop, unsigned* ticket,
                               IterDev* it, const MomentsFinalize* fin, const CullLaunch& cl, hipStream_t s);
// Merge `nranks` gathered moments in rank order and compute mean/std/threshold.
hipError_t launch_finalize_moments(const Moments* gathered, int nranks, IterDev* it, MomentsFinalize fin,
                                   const CullLaunch& cl, hipStream_t s);

// Where the finished record goes: a device-visible pinned host IterDev (the search's
// published_lists in IterDev::lists); the search's counters are cleared for the next search.
struct IterPublish {
  IterDev* host;
  FollowCounts* lists;
  double seq;  // stored last into host->seq: the record is complete
  // device loop (host null): the session steps on the device and the iteration's LoopRec goes
  // to `rec` (pinned host memory, read after the batch)
  LoopDev* loop;
  LoopRec* rec;
};


int64_t cull_num_blocks(int64_t n);
// 3-sigma cull + covariance part sums (from the search's wave records and the band pairs, or a
// full pass; wave_stats.h) and their last merge level into it->c_local; with pub (no
// communicator) also RMSE + publish. With a ticket counter and a small grid the last block runs
// the last level and the publish itself (one launch instead of two).
hipError_t launch_cull_tail(const CullLaunch& a, unsigned* ticket, const IterPublish* pub, hipStream_t s);
// Merge `nranks` gathered covariance moments in rank order, RMSE, publish.
hipError_t launch_finalize_cov(const CovMoments* gathered, int nranks, IterDev* it, IterPublish pub, hipStream_t s);

// --- knn_kernels.hip: k nearest neighbours through the octree, the target's normals from them.
// Threads per block of the k-NN kernels: the DFS stack (levels x 8 B) and the k-entry list
// (k x 12 B) of every thread in LDS, at most 64 KiB per block.
int knn_block_threads(int levels, int k);
// The k nearest target points of n queries (AoS) under (fl(d2), original index), ascending:
// idx_out / d2_out are n x k (either may be null).
hipError_t launch_knn(const NodeRec* nodes, const TgtPt* pts, int levels, const double* q_aos, int64_t n, int k,
                      int32_t* idx_out, double* d2_out, hipStream_t s);
// One normal per target point (leaf order, 3 x fp64) from its k nearest target points; view: the
// viewpoint of the sign rule (has_view = 0: largest component positive).
hipError_t launch_target_normals(const NodeRec* nodes, const TgtPt* pts, int levels, int64_t n, int k, int has_view,
                                 const double view[3], double* normals, hipStream_t s);
// Normals between the caller's target order (aos) and leaf order (leaf). to_leaf also counts in *bad
// the rows that are neither of unit length nor zero.
hipError_t launch_normals_to_leaf(const TgtPt* pts, const double* aos, double* leaf, int64_t n, unsigned* bad,
                                  hipStream_t s);
hipError_t launch_normals_from_leaf(const TgtPt* pts, const double* leaf, double* aos, int64_t n, hipStream_t s);

// --- plane_kernels.hip: the point-to-plane sums of the last iterate's valid pairs.
constexpr int kPlaneSums = 32;  // 21 of J J^T (upper triangle, row by row), 6 of J r, r^2, n, skipped, 2 pad
struct PlaneLaunch {
  const double* x;
  const double* y;
  const double* z;
  const int32_t* pos;
  const double* dist;
  const TgtPt* pts;
  const double* normals;  // leaf order
  const IterDev* it;      // the threshold
  double origin[3];
  int64_t n;
  double* parts;  // plane_num_parts(n) x kPlaneSums
  double* out;    // kPlaneSums
  double thr;     // launch_plane_sums_at: the caller's threshold (it is not read)
};
int64_t plane_num_parts(int64_t n);
hipError_t launch_plane_sums(const PlaneLaunch& a, hipStream_t s);
// The same sums over the pairs with a finite d <= a.thr.
hipError_t launch_plane_sums_at(const PlaneLaunch& a, hipStream_t s);

// --- gicp_kernels.hip: the generalized-ICP sums of the last iterate's valid pairs
// and the source normals between the caller's order and slot order.
constexpr int kGicpSums = 32;  // 21 of J^T M J (upper triangle, row by row), 6 of J^T M r, r^T M r, n,
                               // zero source normals, zero target normals, 1 pad
struct GicpLaunch {
  const double* x;
  const double* y;
  const double* z;
  const int32_t* pos;
  const double* dist;
  const TgtPt* pts;
  const double* normals;      // the target's, leaf order
  const double* src_normals;  // the source's, slot order, in the frame they were made in
  const IterDev* it;          // the threshold
  double origin[3];
  double R[9];  // row-major: takes a source normal to the moved source's frame
  double f;     // 1 - epsilon
  int64_t n;
  double* parts;  // gicp_num_parts(n) x kGicpSums
  double* out;    // kGicpSums
  double thr;     // launch_gicp_sums_at: the caller's threshold (it is not read)
};
int64_t gicp_num_parts(int64_t n);
hipError_t launch_gicp_sums(const GicpLaunch& a, hipStream_t s);
// The same sums over the pairs with a finite d <= a.thr.
hipError_t launch_gicp_sums_at(const GicpLaunch& a, hipStream_t s);
// slot[k] = aos[perm[k]] (3 x fp64 rows). With bad (null: no check) it also counts in *bad the rows
// that are neither of unit length nor zero.
hipError_t launch_src_normals_to_slot(const int32_t* perm, const double* aos, double* slot, int64_t n, unsigned* bad,
                                      hipStream_t s);
hipError_t launch_src_normals_from_slot(const int32_t* perm, const double* slot, double* aos, int64_t n,
                                        hipStream_t s);
// *bad += the points of an AoS cloud with a non-finite coordinate.
hipError_t launch_count_nonfinite(const double* aos, int64_t n, unsigned* bad, hipStream_t s);

// --- reject_kernels.hip: the rank select over the residuals and the pair sums at a caller's
// threshold.
constexpr int kSelectPasses = 6;   // 11-bit digits of the 64-bit key, the last one 9 bits
constexpr int kSelectBins = 2048;
enum : unsigned { kSelectOk = 0, kSelectEmpty = 1, kSelectRange = 2 };  // no finite residual; rank > n_finite
// The select's device-resident record: the state after each digit, and after the last the result.
struct SelectState {
  unsigned long long key;        // the selected key's resolved digits (after the last: the value's bits)
  unsigned long long rank_left;  // the rank inside the bucket of the resolved digits (1-based)
  unsigned long long n_less;     // finite residuals below that bucket
  unsigned long long n_finite;
  unsigned long long rank;       // the rank the call selects
  unsigned long long n_equal;    // residuals in the bucket (after the last digit: equal to the value)
  unsigned long long status;     // kSelect*
  unsigned long long pad;
};
size_t select_scratch_bytes();  // the histograms and the states of one call
const SelectState* select_result(const void* scratch);  // where the finished call's record lies (device)
int select_full_reads();        // passes over the residuals of one call
// The rank-th smallest finite residual of dist[0, n): rank >= 1, or (rank 0) trim_rank(fraction,
// n_finite) computed on the device once the first pass has counted n_finite. Chained on s, no host
// wait; the result is *select_result(scratch).
hipError_t launch_residual_select(const double* dist, int64_t n, double fraction, int64_t rank, void* scratch,
                                  hipStream_t s);

constexpr int kPairRec = 20;  // doubles per part of the pair sums (the CovMoments record's size)
struct PairLaunch {
  const double* x;
  const double* y;
  const double* z;
  const int32_t* pos;
  const double* dist;
  const TgtPt* pts;
  double thr;
  int64_t n;
  unsigned* first;  // scratch: the lowest index of a valid pair
  double* parts;    // pair_num_parts(n) x kPairRec
  double* out;      // kPairRec + 1: the valid pairs' CovMoments, then the finite residuals
};
int64_t pair_num_parts(int64_t n);
hipError_t launch_pair_sums(const PairLaunch& a, hipStream_t s);

// --- voxel_kernels.hip: voxel-grid down-sampling (the definition: voxel_host.h).
struct VoxelOrigin {
  double o[3];
};
// The call's device-resident record: what the host reads back (once after the keys, once after the runs).
struct VoxelHead {
  double origin[3];            // the origin in use (phase 1)
  unsigned long long n_bad;    // non-finite coordinates (phase 1)
  unsigned long long max_key;  // the largest key (phase 2): the sort's end bit
  unsigned flags;              // kVoxelBelow | kVoxelBeyond: a cell index outside [0, 2^21) (phase 2)
  int32_t m;                   // runs = voxels (phase 4)
};
int voxel_bounds_parts(int64_t n);                      // parts of phase 1 (4 doubles each)
hipError_t voxel_temp_bytes(int64_t n, size_t* bytes);  // hipCUB's scratch for the sort and the scan
// Phase 1: head->origin = origin, or (null) the cloud's per-axis minimum; head->n_bad; the rest cleared.
hipError_t launch_voxel_bounds(const double* xyz, int64_t n, const double* origin, double* parts, VoxelHead* head,
                               hipStream_t s);
// Phase 2: keys[i] and idx[i] = i of every point; head->max_key, head->flags.
hipError_t launch_voxel_keys(const double* xyz, int64_t n, double h, VoxelHead* head, uint64_t* keys, int32_t* idx,
                             hipStream_t s);
// Phase 3: the stable radix sort of (key, index) over the bits of max_key.
hipError_t launch_voxel_sort(void* tmp, size_t tmp_bytes, const uint64_t* keys, uint64_t* keys_out, const int32_t* idx,
                             int32_t* idx_out, int64_t n, uint64_t max_key, hipStream_t s);
// Phase 4: flag / pos (n ints each, scratch), starts (n + 1 ints: run r begins at slot starts[r],
// starts[m] = n) and head->m.
hipError_t launch_voxel_runs(void* tmp, size_t tmp_bytes, const uint64_t* sorted_keys, int64_t n, int32_t* flag,
                             int32_t* pos, int32_t* starts, VoxelHead* head, hipStream_t s);
// Phase 5: per run its first index, count and point (any output may be null).
hipError_t launch_voxel_reduce(const double* xyz, const int32_t* idx, const int32_t* starts, const VoxelHead* head,
                               int64_t m, int mode, double* xyz_out, int32_t* first_out, int32_t* count_out,
                               hipStream_t s);

// --- outlier_kernels.hip: statistical and radius outlier removal (the definition:
// icp_hip.h) over a private octree of the cloud (nodes, pts: gpu_build_octree's arrays).
// The call's device-resident record: what the host reads back (once after the statistics, once
// after the flags' sum).
struct OutlierHead {
  double mean, sd, threshold;  // of the scores (statistics)
  int32_t m;                   // kept points (compaction)
  int32_t pad;
};
int outlier_num_parts(int64_t n);                         // parts of the statistics (2 doubles each)
hipError_t outlier_temp_bytes(int64_t n, size_t* bytes);  // hipCUB's scratch for the scan
// score[original index] of every point: the mean distance to its k nearest other points
// (ICP_OUTLIER_STATISTICAL; param unused), or the number of other points within the radius param,
// saturated at k (ICP_OUTLIER_RADIUS). knn_block_threads sizes the blocks (the radius mode: no list).
hipError_t launch_outlier_scores(const NodeRec* nodes, const TgtPt* pts, int levels, int64_t n, int mode, int k,
                                 double param, double* score, hipStream_t s);
// head->mean, sd, threshold from the scores in index order (parts: scratch); head->m cleared.
hipError_t launch_outlier_stats(const double* score, int64_t n, int mode, int k, double param, double* parts,
                                OutlierHead* head, hipStream_t s);
// flag / pos (n ints each): the kept points' flags from head->threshold and their exclusive sum; head->m.
hipError_t launch_outlier_flags(void* tmp, size_t tmp_bytes, const double* score, int64_t n, int mode, int32_t* flag,
                                int32_t* pos, OutlierHead* head, hipStream_t s);
// The kept points' coordinates and original indices at their ranks (either output may be null).
hipError_t launch_outlier_gather(const double* xyz, int64_t n, const int32_t* flag, const int32_t* pos, double* xyz_out,
                                 int32_t* index_out, hipStream_t s);

hipError_t launch_apply(const double T[12], double* x, double* y, double* z, int64_t n, hipStream_t s);
hipError_t launch_scatter_aos(const int32_t* perm, const double* x, const double* y, const double* z,
                              double* aos, int64_t n, hipStream_t s);
hipError_t launch_scatter_corr(const int32_t* perm, const int32_t* pos, const TgtPt* pts,
                               int32_t* idx_out, const double* dist_in, double* dist_out, int64_t n,
                               hipStream_t s);
hipError_t launch_deinterleave(const double* aos, double* x, double* y, double* z, int64_t n, hipStream_t s);
hipError_t launch_gather_deinterleave(const double* aos, const int32_t* perm, double* x, double* y, double* z,
                                      int64_t n, hipStream_t s);

}  // namespace icp
