// reject_kernels.hip — the correspondence rejectors beside the reference's cull:
// an exact rank select over the last iterate's residuals and the valid-pair sums at a caller's
// threshold. Calls of their own after the iterate: they read what it left resident (the moved
// source, the matches, the residuals, the target records) and write none of it. fp64, no FMA.
//
//  k_select_pass<P>  digit P of a radix select, most significant digit first (11-bit digits, the
//                    last one 9: 6 passes over the 64-bit key). A finite residual is sqrt of a
//                    non-negative fp64, so its bit pattern orders as an unsigned integer: that is
//                    the key; NaN and +-inf are not ranked. Every block first resolves the previous
//                    digit from its finished histogram (the bucket that holds the rank; all blocks
//                    compute the same state, block 0 stores it), then counts the keys under that
//                    prefix into a histogram in LDS and merges it into the global one: integer
//                    adds, so the counts do not depend on the order. The passes chain on the
//                    stream; a kernel boundary is the only hand-over between them.
//  k_select_finish   resolves the last digit: the value and its counts.
//  k_pair_first      the lowest index of a valid pair (d finite, d <= threshold): the shift.
//  k_pair_sums       fixed parts of 4096 queries (as k_moments): thread t of a part adds its queries
//                    t + 256 j (j < 16) in order, then the block's fixed tree (block_sum); plain sums
//                    of values shifted by the first valid pair, as the cull's (reduce_kernels.hip).
//  k_pair_merge      the parts added in index order, one thread per sum, then (count, means,
//                    co-moment) as the cull's last level.
// The bits depend neither on the run nor on which search path settled which query.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "nn_device.h"

namespace icp {
namespace {
using namespace dev;

constexpr int kSelBlock = 256;
constexpr int kSelPairs = 2048;      // 16-byte loads per block and trip (4096 residuals)
constexpr int kSelMaxBlocks = 1024;  // 4 per CU: a block's trips depend on n only

__host__ __device__ constexpr int sel_shift(int p) { return p < 5 ? 53 - 11 * p : 0; }
__host__ __device__ constexpr int sel_width(int p) { return p < 5 ? 11 : 9; }
static_assert(sel_shift(0) + sel_width(0) == 64 && sel_shift(4) == sel_width(5) && kSelectPasses == 6, "six digits");

struct SelArgs {
  const double* dist;
  int64_t n;
  unsigned* hist;    // kSelectPasses x kSelectBins, zero at the first pass
  SelectState* st;   // [p]: the state once digits 0 .. p-1 are resolved (p = 1 .. kSelectPasses)
  double fraction;
  int64_t rank;
};

// The bucket of a finished histogram that holds rank r (1-based), by all 256 threads of the
// block: thread t sums bins 8 t .. 8 t + 7, an inclusive scan over the threads, and the one
// thread whose range holds r walks its 8 bins. first: r is not known yet; it follows from the
// total (the finite residuals) by the call's rule. sm: 256 words of LDS.
struct SelPick {
  unsigned digit, below, count, total;
  unsigned long long r;
  unsigned status;
};
__device__ SelPick sel_pick(const unsigned* hist, unsigned long long r, bool first, double fraction, int64_t rank,
                            unsigned* sm) {
  const int t = threadIdx.x;
  const uint4 a = reinterpret_cast<const uint4*>(hist)[2 * t], b = reinterpret_cast<const uint4*>(hist)[2 * t + 1];
  const unsigned c[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  unsigned local = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) local += c[k];
  sm[t] = local;
  __syncthreads();
#pragma unroll
  for (int s = 1; s < kSelBlock; s <<= 1) {
    const unsigned v = t >= s ? sm[t - s] : 0u;
    __syncthreads();
    sm[t] += v;
    __syncthreads();
  }
  const unsigned incl = sm[t], excl = incl - local, total = sm[kSelBlock - 1];
  __syncthreads();
  SelPick p;
  p.total = total;
  p.status = kSelectOk;
  if (first) {
    r = rank >= 1 ? (unsigned long long)rank : (unsigned long long)trim_rank(fraction, (int64_t)total);
    p.status = total == 0 ? kSelectEmpty : (r > total ? kSelectRange : kSelectOk);
  }
  p.r = r;
  if (p.status == kSelectOk && r > excl && r <= incl) {  // one thread: 1 <= r <= total
    unsigned cum = excl, dg = 0, bl = 0, ct = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      if (!found && r <= (unsigned long long)cum + c[k]) {
        dg = 8u * t + k;
        bl = cum;
        ct = c[k];
        found = true;
      }
      cum += c[k];
    }
    sm[0] = dg;
    sm[1] = bl;
    sm[2] = ct;
  }
  __syncthreads();
  p.digit = sm[0];
  p.below = sm[1];
  p.count = sm[2];
  __syncthreads();
  return p;
}

// The state once digit P - 1 is resolved, from the state before it and that digit's histogram
// (the same in every block).
template <int P>
__device__ SelectState sel_advance(const SelArgs& a, unsigned* sm) {
  SelectState s;
  if (P == 1) {
    s.key = s.rank_left = s.n_less = s.n_finite = s.rank = s.n_equal = s.status = s.pad = 0ull;
  } else {
    s = a.st[P - 1];
    if (s.status != kSelectOk) return s;  // block-uniform
  }
  const SelPick p = sel_pick(a.hist + (P - 1) * kSelectBins, s.rank_left, P == 1, a.fraction, a.rank, sm);
  if (P == 1) {
    s.n_finite = p.total;
    s.rank = p.r;
    s.status = p.status;
    if (s.status != kSelectOk) return s;
  }
  s.key = (s.key << sel_width(P - 1)) | p.digit;
  s.n_less += p.below;
  s.rank_left = p.r - p.below;
  s.n_equal = p.count;
  return s;
}

template <int P>
__global__ void __launch_bounds__(kSelBlock) k_select_pass(SelArgs a) {
  __shared__ unsigned h[kSelectBins];
  __shared__ unsigned sm[kSelBlock];
  unsigned long long prefix = 0ull;
  if (P > 0) {
    const SelectState s = sel_advance<(P > 0 ? P : 1)>(a, sm);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.st[P] = s;
    if (s.status != kSelectOk) return;  // nothing to rank: the later passes only hand the status on
    prefix = s.key;
  }
  for (int k = threadIdx.x; k < kSelectBins; k += kSelBlock) h[k] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  // One residual into the block's histogram. The lanes that share the first counted lane's digit
  // add once for all of them (a pass whose keys agree in this digit would otherwise queue 64 adds
  // on one word); the others add for themselves.
  auto tally = [&](double d) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(d);
    bool mine = ((key >> 52) & 0x7ffull) != 0x7ffull;  // finite
    if (P > 0) mine = mine && (key >> (sel_shift(P) + sel_width(P))) == prefix;
    const unsigned digit = (unsigned)(key >> sel_shift(P)) & ((1u << sel_width(P)) - 1u);
    const unsigned long long m = wballot(mine);
    if (m == 0ull) return;
    const int lead = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(m));
    const unsigned ld = (unsigned)__builtin_amdgcn_readlane((int)digit, lead);
    const unsigned long long same = wballot(mine && digit == ld);
    if (lane == lead) {
      atomicAdd(&h[ld], (unsigned)__popcll(same));
    } else if (mine && digit != ld) {
      atomicAdd(&h[digit], 1u);
    }
  };
  // 16-byte loads from the first 16-byte boundary; the residual before it (the array is 8-byte
  // aligned) and the last one of an odd count go the scalar way. Nothing is read past n.
  const int64_t head = (a.n > 0 && (reinterpret_cast<uintptr_t>(a.dist) & 8u) != 0) ? 1 : 0;
  const int64_t npair = (a.n - head) / 2;
  const double2* v = reinterpret_cast<const double2*>(a.dist + head);
  const double nan = __builtin_nan("");
  for (int64_t c = blockIdx.x; c * kSelPairs < npair; c += gridDim.x) {
    double2 d[kSelPairs / kSelBlock];
#pragma unroll
    for (int j = 0; j < kSelPairs / kSelBlock; j++) {
      const int64_t q = c * kSelPairs + j * kSelBlock + threadIdx.x;
      d[j] = q < npair ? v[q] : make_double2(nan, nan);  // a NaN is not counted
    }
#pragma unroll
    for (int j = 0; j < kSelPairs / kSelBlock; j++) {
      tally(d[j].x);
      tally(d[j].y);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < kWave) {
    const bool lo = head != 0 && lane == 0, hi = head + 2 * npair < a.n && lane == 1;
    tally(lo ? a.dist[0] : (hi ? a.dist[a.n - 1] : nan));
  }
  __syncthreads();
  unsigned* g = a.hist + P * kSelectBins;
  for (int k = threadIdx.x; k < kSelectBins; k += kSelBlock) {
    const unsigned cnt = h[k];
    if (cnt != 0u) atomicAdd(&g[k], cnt);
  }
}

__global__ void __launch_bounds__(kSelBlock) k_select_finish(SelArgs a) {
  __shared__ unsigned sm[kSelBlock];
  const SelectState s = sel_advance<kSelectPasses>(a, sm);
  if (threadIdx.x == 0) a.st[kSelectPasses] = s;
}

// ---- the pair sums

constexpr int kPairPart = 4096;
constexpr int kPairBlock = 256;
constexpr int kPairSums = 18;  // CovSums' 17 (n, sum d^2, sa[3], sb[3], sab[9]) and the finite residuals
constexpr unsigned kNoPair = 0xffffffffu;

__device__ __forceinline__ bool pair_valid(double d, double thr) { return __builtin_isfinite(d) && d <= thr; }

// The lowest index of a valid pair into *first (kNoPair before the launch): a minimum, so the
// order of the blocks does not matter. A block whose part lies above a pair already found returns
// at once.
__global__ void __launch_bounds__(kPairBlock) k_pair_first(const double* __restrict__ dist, int64_t n, double thr,
                                                           unsigned* first) {
  __shared__ unsigned smin;
  const int64_t base = (int64_t)blockIdx.x * kPairPart;
  if (threadIdx.x == 0) smin = kNoPair;
  const unsigned known = __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  unsigned mine = kNoPair;
  if ((int64_t)known > base) {
    for (int j = kPairPart / kPairBlock - 1; j >= 0; j--) {
      const int64_t i = base + threadIdx.x + (int64_t)j * kPairBlock;
      if (i < n && pair_valid(dist[i], thr)) mine = (unsigned)i;
    }
  }
  if (mine != kNoPair) atomicMin(&smin, mine);
  __syncthreads();
  if (threadIdx.x == 0 && smin != kNoPair &&
      smin < __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMin(first, smin);
}

// The shift of the sums: the first valid pair's source point and match (zeros without one: no
// pair is summed then).
__device__ __forceinline__ void pair_shift(const PairLaunch& a, double sh[6]) {
  const unsigned f = *a.first;
#pragma unroll
  for (int k = 0; k < 6; k++) sh[k] = 0.0;
  if (f == kNoPair) return;
  const TgtPt* p = a.pts + a.pos[f];
  sh[0] = a.x[f];
  sh[1] = a.y[f];
  sh[2] = a.z[f];
  sh[3] = p->x;
  sh[4] = p->y;
  sh[5] = p->z;
}

__global__ void __launch_bounds__(kPairBlock) k_pair_sums(PairLaunch a) {
  __shared__ double red[(kPairBlock / kWave) * kPairSums];
  const int64_t base = (int64_t)blockIdx.x * kPairPart;
  const double thr = a.thr;
  double sh[6];
  pair_shift(a, sh);
  double v[kPairSums];
#pragma unroll
  for (int k = 0; k < kPairSums; k++) v[k] = 0.0;
  for (int j = 0; j < kPairPart / kPairBlock; j++) {
    const int64_t i = base + threadIdx.x + (int64_t)j * kPairBlock;
    if (i >= a.n) break;
    const double d = a.dist[i];
    if (!__builtin_isfinite(d)) continue;
    v[17] += 1.0;
    if (!(d <= thr)) continue;
    const TgtPt* p = a.pts + a.pos[i];
    const double2 bxy = *reinterpret_cast<const double2*>(&p->x);
    const double da[3] = {a.x[i] - sh[0], a.y[i] - sh[1], a.z[i] - sh[2]};
    const double db[3] = {bxy.x - sh[3], bxy.y - sh[4], p->z - sh[5]};
    v[0] += 1.0;
    v[1] += d * d;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      v[2 + r] += da[r];
      v[5 + r] += db[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) v[8 + 3 * r + c] += da[r] * db[c];
  }
  block_sum<kPairSums>(v, red);
  if (threadIdx.x < kPairRec) {
    // v[] is indexed by a constant below: every thread holds the block's sums
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < kPairSums; k++) out = threadIdx.x == k ? v[k] : out;
    a.parts[(int64_t)blockIdx.x * kPairRec + threadIdx.x] = out;
  }
}

// out: the CovMoments record of the valid pairs (20 doubles), then the finite residuals.
__global__ void __launch_bounds__(64) k_pair_merge(PairLaunch a, int64_t nparts) {
  __shared__ double col[kPairSums];
  const int k = threadIdx.x;
  if (k < kPairSums) {
    double s = 0.0;
    for (int64_t p = 0; p < nparts; p++) s += a.parts[p * kPairRec + k];
    col[k] = s;
  }
  __syncthreads();
  if (k != 0) return;
  double sh[6];
  pair_shift(a, sh);
  CovMoments m = cov_identity();
  const double n = col[0];
  if (n > 0.0) {  // the cull's last level (reduce_kernels.hip cov_last)
    m.n = n;
    m.sum_d2 = col[1];
    double da[3], db[3];
    for (int q = 0; q < 3; q++) {
      da[q] = col[2 + q] / n;
      db[q] = col[5 + q] / n;
      m.ma[q] = sh[q] + da[q];
      m.mb[q] = sh[3 + q] + db[q];
    }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) m.c[3 * i + j] = col[8 + 3 * i + j] - n * (da[i] * db[j]);
  }
  const double* mw = reinterpret_cast<const double*>(&m);
  for (int q = 0; q < kPairRec; q++) a.out[q] = mw[q];
  a.out[kPairRec] = col[17];
}

template <int P>
void launch_pass(const SelArgs& a, unsigned blocks, hipStream_t s) {
  hipLaunchKernelGGL(k_select_pass<P>, dim3(blocks), dim3(kSelBlock), 0, s, a);
}

}  // namespace

size_t select_scratch_bytes() {
  return sizeof(unsigned) * kSelectPasses * kSelectBins + sizeof(SelectState) * (kSelectPasses + 1);
}

const SelectState* select_result(const void* scratch) {
  return reinterpret_cast<const SelectState*>(static_cast<const unsigned*>(scratch) + kSelectPasses * kSelectBins) +
         kSelectPasses;
}

int select_full_reads() { return kSelectPasses; }

hipError_t launch_residual_select(const double* dist, int64_t n, double fraction, int64_t rank, void* scratch,
                                  hipStream_t s) {
  SelArgs a;
  a.dist = dist;
  a.n = n;
  a.hist = static_cast<unsigned*>(scratch);
  a.st = reinterpret_cast<SelectState*>(a.hist + kSelectPasses * kSelectBins);
  a.fraction = fraction;
  a.rank = rank;
  const hipError_t e = hipMemsetAsync(a.hist, 0, sizeof(unsigned) * kSelectPasses * kSelectBins, s);
  if (e != hipSuccess) return e;
  const int64_t trips = (n / 2 + kSelPairs - 1) / kSelPairs;
  const unsigned blocks = (unsigned)(trips < 1 ? 1 : trips > kSelMaxBlocks ? kSelMaxBlocks : trips);
  launch_pass<0>(a, blocks, s);
  launch_pass<1>(a, blocks, s);
  launch_pass<2>(a, blocks, s);
  launch_pass<3>(a, blocks, s);
  launch_pass<4>(a, blocks, s);
  launch_pass<5>(a, blocks, s);
  hipLaunchKernelGGL(k_select_finish, dim3(1), dim3(kSelBlock), 0, s, a);
  return hipGetLastError();
}

int64_t pair_num_parts(int64_t n) { return (n + kPairPart - 1) / kPairPart; }

hipError_t launch_pair_sums(const PairLaunch& a, hipStream_t s) {
  const int64_t nparts = pair_num_parts(a.n);
  const hipError_t e = hipMemsetAsync(a.first, 0xff, sizeof(unsigned), s);
  if (e != hipSuccess) return e;
  if (nparts > 0) {
    hipLaunchKernelGGL(k_pair_first, dim3((unsigned)nparts), dim3(kPairBlock), 0, s, a.dist, a.n, a.thr, a.first);
    hipLaunchKernelGGL(k_pair_sums, dim3((unsigned)nparts), dim3(kPairBlock), 0, s, a);
  }
  hipLaunchKernelGGL(k_pair_merge, dim3(1), dim3(64), 0, s, a, nparts);
  return hipGetLastError();
}

}  // namespace icp
