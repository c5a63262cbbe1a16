// ctx_clouds.cpp — the clouds resident on the device: the target's octree, this rank's source shard
// in query order, and the calls that read them back or search the target outside an iterate.
#include <cfloat>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "icp_ctx_internal.h"
#include "octree_build.h"
#include "octree_gpu.h"
#include "query_order.h"

using namespace icp;

void free_source(icp_hip_ctx* c) {
  prewalk_free_source(c);
  gicp_free_source(c);  // normals name the points of this source
  dfree(c->x);
  dfree(c->y);
  dfree(c->z);
  dfree(c->perm);
  dfree(c->pos);
  dfree(c->dist);
  c->follow.release(false);
  dfree(c->wc_box);
  dfree(c->wc_ents);
  dfree(c->mparts);
  dfree(c->cparts);
  dfree(c->wstat);
  c->n_src = 0;
}

// No band for the next iterate's search (a new source or target): its cull pass does it all.
static hipError_t reset_band(icp_hip_ctx* c) {
  c->last_cull_path = -1;
  char* base = reinterpret_cast<char*>(c->it);
  return hipMemsetAsync(base + offsetof(IterDev, fz_lo), 0, offsetof(IterDev, cull_mode) - offsetof(IterDev, fz_lo),
                        c->stream);
}

void free_target(icp_hip_ctx* c) {
  drain_prewalk(c);
  plane_free_target(c);  // normals name the points of this tree
  dfree(c->nodes);
  dfree(c->tbox);
  dfree(c->pts);
  dfree(c->cells);
  c->cell_lmax = -1;
  c->n_nodes = 0;
  c->n_tgt = 0;
}

NNLaunch base_launch(const icp_hip_ctx* c) {
  NNLaunch a;
  std::memset(&a, 0, sizeof(a));
  a.nodes = c->nodes;
  a.tbox = c->tbox;
  a.pts = c->pts;
  a.counters = c->counters;
  a.n_nodes = (int32_t)c->n_nodes;
  a.pos0 = c->pos0;
  a.levels = c->levels;
  a.init_best = c->init_best;
  a.search = c->cfg.search;
  a.scan32 = c->cfg.scan32;
  a.cells = c->cells;
  a.cell_lmax = c->cell_lmax;
  a.join_factor = c->cfg.join_factor;
  a.ball_mode = c->cfg.ball_mode;
  a.xcd_blocks = c->cfg.xcd_blocks;
  a.scan_groups = c->cfg.scan_groups;
  a.certify_prev = c->cfg.certify_prev;
  a.dbg = c->dbg;
  for (int k = 0; k < 3; k++) {
    a.root_lo[k] = c->root_box[k];
    a.root_hi[k] = c->root_box[3 + k];
  }
  return a;
}

// What the context keeps of a built tree besides its arrays (GpuOctree or FlatOctree).
template <class Tree>
static void keep_tree_info(icp_hip_ctx* c, const Tree& t, int64_t n_nodes) {
  c->n_nodes = n_nodes;
  c->n_leaves = t.n_leaves;
  c->pos0 = t.pos_of_orig0;
  c->max_depth = t.max_depth;
  c->max_inner_depth = t.max_inner_depth;
  c->levels = t.max_inner_depth + 1 > 0 ? t.max_inner_depth + 1 : 1;
}

// --- device-pointer entry points (icp_hip_*_device): the caller's buffer is checked by its
// attributes alone (never dereferenced on the host), then handed to the same device core the host
// variants run after their upload.

// A buffer a kernel of this context may read or write: device memory of the context's device, or
// managed memory. A group's host-staged routes only copy it, so any device's memory will do.
int check_device_ptr(const icp_hip_ctx* c, const void* p, const char* what, unsigned align) {
  if (!p) return fail(ICP_HIP_EINVAL, std::string(what) + ": null device pointer");
  if (reinterpret_cast<uintptr_t>(p) % align != 0)
    return fail(ICP_HIP_EINVAL, std::string(what) + ": pointer not " + std::to_string(align) + "-byte aligned");
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(ICP_HIP_EINVAL, std::string(what) + ": not a device pointer (" + hipGetErrorString(e) + ")");
  }
  if (at.type == hipMemoryTypeManaged) return ICP_HIP_OK;
  if (at.type != hipMemoryTypeDevice) return fail(ICP_HIP_EINVAL, std::string(what) + ": host memory, not a device pointer");
  if (!c->group && at.device != c->device)
    return fail(ICP_HIP_EINVAL, std::string(what) + ": device memory of another device than the context's");
  return ICP_HIP_OK;
}

int check_optional_device_ptr(const icp_hip_ctx* c, const void* p, const char* what, unsigned align) {
  return p ? check_device_ptr(c, p, what, align) : ICP_HIP_OK;
}

int fail_octree_build(int rc, const std::string& why) {
  return fail(rc == 1 ? ICP_HIP_EINVAL : rc == -2 ? ICP_HIP_ENOMEM : ICP_HIP_EDEVICE, why);
}

int last_timing(bool timed, const double* src, int count, const char* none_text, double* ms) {
  if (!timed) return fail(ICP_HIP_ENOTREADY, none_text);
  std::memcpy(ms, src, sizeof(double) * (size_t)count);
  return ICP_HIP_OK;
}

// set_target after the argument checks, from a host cloud (xyz) or a device cloud (d_in), one of
// them null. The device builder reads d_in in place; the host builder gets it staged down.
// Whole or not at all: a failure leaves the context without a target (as free_target leaves it);
// the source is untouched either way.
static int set_target_core(icp_hip_ctx* c, const double* xyz, const double* d_in, int64_t n, int max_points,
                           int max_depth, int rules) {
  HIP_TRY(hipSetDevice(c->device));
  free_target(c);
  ScopeExit undo([c] { free_target(c); });
  HIP_TRY(reset_band(c));
  hipEvent_t e0 = c->ev_it0, e1 = c->ev_it1;
  HIP_TRY(hipEventRecord(e0, c->stream));
  const bool on_device = max_depth <= kGpuBuildMaxDepth && c->cfg.octree_builder == ICP_BUILD_AUTO;
  if (on_device) {
    // device build straight from the AoS cloud in HBM (octree_gpu.hip): the caller's, or the upload
    DevScratch S;  // the upload: released with this block, before the boxes and tables are made
    double* d_xyz = nullptr;
    if (!d_in) HIP_TRY(call_upload(S, &d_xyz, xyz, 3 * (size_t)n, c->stream));
    ScopedOctree oct;
    std::string why;
    if (const int rc = gpu_build_octree(d_in ? d_in : d_xyz, n, max_points, max_depth, c->stream, &oct.t, &why))
      return fail_octree_build(rc, why);
    const GpuOctree t = oct.release();  // into the context (free_target)
    c->nodes = t.nodes;
    c->pts = t.pts;
    keep_tree_info(c, t, t.n_nodes);
  } else {
    std::vector<double> staged;
    if (!xyz) {
      HIP_TRY(stage_down(c, &staged, d_in, 3 * (size_t)n));
      xyz = staged.data();
    }
    FlatOctree t;
    const char* why = nullptr;
    if (!build_flat_octree(xyz, n, max_points, max_depth, &t, &why)) return fail(ICP_HIP_EINVAL, why ? why : "bad target");
    HIP_TRY(dalloc(&c->nodes, t.nodes.size()));
    HIP_TRY(dalloc(&c->pts, t.pts.size()));
    HIP_TRY(hipMemcpyAsync(c->nodes, t.nodes.data(), t.nodes.size() * sizeof(NodeRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->pts, t.pts.data(), t.pts.size() * sizeof(TgtPt), hipMemcpyHostToDevice, c->stream));
    keep_tree_info(c, t, (int64_t)t.nodes.size());
  }
  // separation of every target point (the previous-match certificate, certify_prev)
  if (c->cfg.certify_prev) HIP_TRY(launch_target_sep(c->nodes, c->pts, n, c->levels, c->stream));
  // after the separations (which a copy's flag overwrites: its separation is 0 either way)
  HIP_TRY(launch_mark_copies(c->pts, n, c->stream));
  HIP_TRY(dalloc(&c->tbox, (size_t)c->n_nodes));
  HIP_TRY(launch_tight_boxes(c->nodes, c->pts, c->tbox, c->n_nodes, c->max_depth, c->stream));
  // root box (host copy: the kernels' cell arithmetic starts from it) and the cell tables
  {
    NodeRec root;
    HIP_TRY(hipMemcpyAsync(&root, c->nodes, sizeof(NodeRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 3; k++) {
      c->root_box[k] = root.lo[k];
      c->root_box[3 + k] = root.hi[k];
    }
  }
  if (c->cfg.cell_starts && c->n_nodes < ((int64_t)1 << 26)) {
    const int lmax = cell_table_depth(c->n_leaves, c->max_inner_depth);  // a root leaf: level 0 alone
    // the tables only speed up the searches' start: without memory for them the searches start
    // from the root (identical results)
    if (dalloc(&c->cells, (size_t)cell_table_entries(lmax)) == hipSuccess) {
      HIP_TRY(build_cell_tables(c->nodes, lmax, c->cells, c->stream));
      c->cell_lmax = lmax;
    } else {
      (void)hipGetLastError();
      c->cells = nullptr;
    }
  }
  HIP_TRY(hipEventRecord(e1, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  c->target_build_ms = ms;
  c->target_on_device = on_device ? 1 : 0;
  c->n_tgt = n;
  c->init_best = (rules == ICP_RULES_CLI) ? 1e20 : DBL_MAX;  // icp_registration.cpp:201 / octree.cpp:180
  c->have_prev = false;
  c->wc_gen++;  // cached candidate lists name points of the previous tree
  c->have_results = false;
  undo.dismiss();
  return ICP_HIP_OK;
}

// get_correspondences after the argument checks, into host buffers or the caller's device buffers.
static int corr_core(icp_hip_ctx* c, bool to_host, int32_t* idx_out, double* dist_out) {
  if (!c->have_results) return fail(ICP_HIP_ENOTREADY, "no iteration has run on this source");
  if (c->n_src == 0 || (!idx_out && !dist_out)) return ICP_HIP_OK;
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  CallOut<int32_t> idx(idx_out, to_host);
  CallOut<double> dist(dist_out, to_host);
  HIP_TRY(idx.prepare(S, c->n_src));
  HIP_TRY(dist.prepare(S, c->n_src));
  HIP_TRY(launch_scatter_corr(c->perm, c->pos, c->pts, idx.dev(), c->dist, dist.dev(), c->n_src, c->stream));
  HIP_TRY(idx.download(c->n_src, c->stream));
  HIP_TRY(dist.download(c->n_src, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

// nn after the argument checks. to_host: q and the outputs are host buffers (uploaded, searched,
// downloaded); otherwise they are the caller's device buffers, read and written in place.
static int nn_core(icp_hip_ctx* c, bool to_host, const double* q, int64_t n, int32_t* idx_out, double* dist_out) {
  // the wave search addresses per-query arrays by 32-bit byte offsets (nn_device.h qat): launches
  // of fewer than 2^29 queries, so larger sets go in slices (the answers are per query)
  constexpr int64_t kSlice = (int64_t)1 << 28;
  if (n > kSlice) {
    PublishedLists lists{0, 0, 0};
    for (int64_t off = 0; off < n; off += kSlice) {
      const int64_t m = n - off < kSlice ? n - off : kSlice;
      const int rc = nn_core(c, to_host, q + 3 * off, m, idx_out ? idx_out + off : nullptr, dist_out ? dist_out + off : nullptr);
      if (rc != ICP_HIP_OK) return rc;
      lists.exact += c->follow.last.exact;
      lists.ball += c->follow.last.ball;
      lists.lane += c->follow.last.lane;
    }
    c->follow.last = lists;
    return ICP_HIP_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  FollowCounts counts{};  // before its source's owner: outlives the copy
  DevScratch S;           // the host form's upload and outputs, the query arrays, the follow-up lists
  CallOut<int32_t> idx(idx_out, to_host);
  CallOut<double> dist(dist_out, to_host);
  double *up = nullptr, *x = nullptr, *y = nullptr, *z = nullptr, *d = nullptr, *fbu = nullptr;
  int32_t *pos = nullptr, *fbl = nullptr;
  if (to_host) HIP_TRY(call_upload(S, &up, q, 3 * (size_t)n, c->stream));
  HIP_TRY(S.alloc(&x, n));
  HIP_TRY(S.alloc(&y, n));
  HIP_TRY(S.alloc(&z, n));
  HIP_TRY(S.alloc(&d, n));
  HIP_TRY(S.alloc(&pos, n));
  HIP_TRY(idx.prepare(S, n));
  HIP_TRY(dist.prepare(S, n));
  HIP_TRY(launch_deinterleave(to_host ? up : q, x, y, z, n, c->stream));
  HIP_TRY(S.alloc(&fbl, (size_t)follow_list_ints(n)));
  HIP_TRY(S.alloc(&fbu, (size_t)n));
  NNLaunch a = base_launch(c);
  a.x = x;
  a.y = y;
  a.z = z;
  a.pos_out = pos;
  a.dist_out = d;
  a.n = n;
  a.follow = carve_follow_lists(fbl, fbu, c->follow.counts, n, c->cfg.overflow_halves != 0,
                                c->cfg.scan32 && c->cfg.wide_pass != 1);
  HIP_TRY(c->follow.begin_search(c->stream));
  HIP_TRY(launch_nn(a, c->stream));
  HIP_TRY(hipMemcpyAsync(&counts, c->follow.counts, sizeof(FollowCounts), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->follow.last = published_lists(counts);
  if (idx.dev() || dist.dev())  // either may be null
    HIP_TRY(launch_scatter_corr(nullptr, pos, c->pts, idx.dev(), d, dist.dev(), n, c->stream));
  HIP_TRY(idx.download(n, c->stream));
  HIP_TRY(dist.download(n, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

extern "C" {

// HBM for the device entry points, so that a C caller needs no HIP toolchain. A group allocates on
// its first member's device.
int icp_hip_dev_alloc(icp_hip_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return fail(ICP_HIP_EINVAL, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(c->group ? group_member(c, 0)->device : c->device));
  HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return ICP_HIP_OK;
}

int icp_hip_dev_free(icp_hip_ctx* c, void* p) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (!p) return ICP_HIP_OK;
  HIP_TRY(hipSetDevice(c->group ? group_member(c, 0)->device : c->device));
  HIP_TRY(hipFree(p));
  return ICP_HIP_OK;
}

int icp_hip_dev_copy(icp_hip_ctx* c, void* dst, const void* src, size_t bytes, int dir) {
  if (!c || ((!dst || !src) && bytes > 0)) return fail(ICP_HIP_EINVAL, "null argument");
  if (dir != ICP_HIP_COPY_H2D && dir != ICP_HIP_COPY_D2H && dir != ICP_HIP_COPY_D2D)
    return fail(ICP_HIP_EINVAL, "dev_copy: unknown direction");
  if (bytes == 0) return ICP_HIP_OK;
  const hipMemcpyKind kind = dir == ICP_HIP_COPY_H2D   ? hipMemcpyHostToDevice
                             : dir == ICP_HIP_COPY_D2H ? hipMemcpyDeviceToHost
                                                       : hipMemcpyDeviceToDevice;
  icp_hip_ctx* m = c->group ? group_member(c, 0) : c;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  return ICP_HIP_OK;
}

int icp_hip_set_target(icp_hip_ctx* c, const double* xyz, int64_t n, int max_points, int max_depth, int rules) {
  if (!c || (!xyz && n > 0)) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return n <= 0 ? fail(ICP_HIP_EINVAL, "empty target cloud (icpengine.cpp:31-34 rejects it)")
                             : group_set_target(c, xyz, n, max_points, max_depth, rules);
  if (n <= 0) return fail(ICP_HIP_EINVAL, "empty target cloud (icpengine.cpp:31-34 rejects it)");
  if (max_depth < 0 || max_depth > 60) return fail(ICP_HIP_EINVAL, "max_depth out of range [0, 60]");
  if (n > (int64_t)0x7fffffff) return fail(ICP_HIP_EINVAL, "target size out of range (int32 indices, as the reference)");
  return set_target_core(c, xyz, nullptr, n, max_points, max_depth, rules);
}

int icp_hip_set_target_device(icp_hip_ctx* c, const double* d_xyz, int64_t n, int max_points, int max_depth, int rules) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (n <= 0) return fail(ICP_HIP_EINVAL, "empty target cloud (icpengine.cpp:31-34 rejects it)");
  if (max_depth < 0 || max_depth > 60) return fail(ICP_HIP_EINVAL, "max_depth out of range [0, 60]");
  if (n > (int64_t)0x7fffffff) return fail(ICP_HIP_EINVAL, "target size out of range (int32 indices, as the reference)");
  if (const int rc = check_device_ptr(c, d_xyz, "set_target_device")) return rc;
  if (c->group) {  // every member uploads its replica from host memory
    std::vector<double> staged;
    HIP_TRY(stage_down(c, &staged, d_xyz, 3 * (size_t)n));
    return group_set_target(c, staged.data(), n, max_points, max_depth, rules);
  }
  return set_target_core(c, nullptr, d_xyz, n, max_points, max_depth, rules);
}

int icp_hip_target_build_info(icp_hip_ctx* c, int32_t* on_device, double* build_ms) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (c->group) return group_target_build_info(c, on_device, build_ms);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (on_device) *on_device = c->target_on_device;
  if (build_ms) *build_ms = c->target_build_ms;
  return ICP_HIP_OK;
}

int icp_hip_copy_target(icp_hip_ctx* c, double* box6, int32_t* first, uint32_t* meta, int32_t* depth, double* xyz,
                        int32_t* orig) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (c->group) return icp_hip_copy_target(group_member(c, 0), box6, first, meta, depth, xyz, orig);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<NodeRec> nodes((size_t)c->n_nodes);
  std::vector<TgtPt> pts((size_t)c->n_tgt);
  HIP_TRY(hipMemcpyAsync(nodes.data(), c->nodes, nodes.size() * sizeof(NodeRec), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(pts.data(), c->pts, pts.size() * sizeof(TgtPt), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < nodes.size(); i++) {
    const NodeRec& r = nodes[i];
    if (box6)
      for (int k = 0; k < 3; k++) {
        box6[6 * i + k] = r.lo[k];
        box6[6 * i + 3 + k] = r.hi[k];
      }
    if (first) first[i] = r.first;
    if (meta) meta[i] = r.meta;
    if (depth) depth[i] = r.depth;
  }
  for (size_t i = 0; i < pts.size(); i++) {
    if (xyz) {
      xyz[3 * i] = pts[i].x;
      xyz[3 * i + 1] = pts[i].y;
      xyz[3 * i + 2] = pts[i].z;
    }
    if (orig) orig[i] = pts[i].orig;
  }
  return ICP_HIP_OK;
}

int icp_hip_target_separation(icp_hip_ctx* c, float* sep_out) {
  if (!c || !sep_out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return icp_hip_target_separation(group_member(c, 0), sep_out);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<TgtPt> pts((size_t)c->n_tgt);
  HIP_TRY(hipMemcpyAsync(pts.data(), c->pts, pts.size() * sizeof(TgtPt), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (const TgtPt& p : pts) sep_out[p.orig] = p.sep;
  return ICP_HIP_OK;
}

int icp_hip_copy_target_aux(icp_hip_ctx* c, float* tbox6, int32_t* cells, int64_t cells_cap, int32_t* cell_lmax) {
  if (!c) return fail(ICP_HIP_EINVAL, "null context");
  if (c->group) return icp_hip_copy_target_aux(group_member(c, 0), tbox6, cells, cells_cap, cell_lmax);
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  const int lmax = c->cells ? c->cell_lmax : -1;
  const int64_t nent = lmax >= 0 ? cell_table_entries(lmax) : 0;
  if (cells && cells_cap < nent) return fail(ICP_HIP_EINVAL, "copy_target_aux: cells_cap smaller than the cell tables");
  if (cell_lmax) *cell_lmax = lmax;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<TBox> tb(tbox6 ? (size_t)c->n_nodes : 0);
  if (tbox6) HIP_TRY(hipMemcpyAsync(tb.data(), c->tbox, tb.size() * sizeof(TBox), hipMemcpyDeviceToHost, c->stream));
  if (cells && nent > 0)
    HIP_TRY(hipMemcpyAsync(cells, c->cells, (size_t)nent * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < tb.size(); i++)
    for (int k = 0; k < 3; k++) {
      tbox6[6 * i + k] = tb[i].lo[k];
      tbox6[6 * i + 3 + k] = tb[i].hi[k];
    }
  return ICP_HIP_OK;
}

int icp_hip_target_info(icp_hip_ctx* c, int64_t* n_nodes, int64_t* n_leaves, int32_t* max_depth, int32_t* levels) {
  if (!c) return fail(ICP_HIP_EINVAL, "null ctx");
  if (c->group) return icp_hip_target_info(group_member(c, 0), n_nodes, n_leaves, max_depth, levels);
  if (n_nodes) *n_nodes = c->n_nodes;
  if (n_leaves) *n_leaves = c->n_leaves;
  if (max_depth) *max_depth = c->max_depth;
  if (levels) *levels = c->levels;
  return ICP_HIP_OK;
}

// set_source after the argument checks, from a host cloud (xyz) or a device cloud (d_in), one of
// them null when n > 0. The device query order and the gather read d_in in place; the host query
// order gets it staged down.
// Whole or not at all: a failure leaves the context without a source (as free_source leaves it,
// n_src = 0); the target is untouched either way.
static int set_source_core(icp_hip_ctx* c, const double* xyz, const double* d_in, int64_t n) {
  // the wave search addresses per-query arrays by 32-bit byte offsets (nn_device.h qat): < 2^29
  // points per shard (12 GB of coordinates; a larger cloud is sharded over a device group)
  if (n >= ((int64_t)1 << 29)) return fail(ICP_HIP_EINVAL, "source shard of 2^29 points or more");
  HIP_TRY(hipSetDevice(c->device));
  free_source(c);
  ScopeExit undo([c] { free_source(c); });
  c->n_src = n;  // the allocations below are sized by it (prewalk_new_source); the guard restores 0
  c->nb_mom = moments_num_parts(n);
  c->nb_cull = cull_num_blocks(n);
  HIP_TRY(dalloc(&c->x, n));
  HIP_TRY(dalloc(&c->y, n));
  HIP_TRY(dalloc(&c->z, n));
  HIP_TRY(dalloc(&c->perm, n));
  HIP_TRY(dalloc(&c->pos, n));
  HIP_TRY(dalloc(&c->dist, n));
  HIP_TRY(c->follow.alloc(n));
  if (c->cfg.candidate_cache && n > 0) {
    // the cache only saves walks: without memory for it every iterate walks (identical results)
    const size_t nw = (size_t)((n + 63) / 64);
    if (dalloc(&c->wc_box, nw) == hipSuccess && dalloc(&c->wc_ents, nw * icp::kWaveCandCap) == hipSuccess) {
      HIP_TRY(hipMemsetAsync(c->wc_box, 0, nw * sizeof(icp::WaveBox), c->stream));  // generation 0: invalid
      prewalk_new_source(c);
    } else {
      (void)hipGetLastError();
      dfree(c->wc_box);
      dfree(c->wc_ents);
    }
  }
  c->wc_gen++;
  HIP_TRY(dalloc(&c->mparts, (size_t)(c->nb_mom + merge_scratch_entries(c->nb_mom))));
  HIP_TRY(dalloc(&c->cparts, (size_t)(c->nb_cull + merge_scratch_entries(c->nb_cull))));
  if (n > 0 && c->cfg.fused_cull && dalloc(&c->wstat, (size_t)((n + 63) / 64)) != hipSuccess) {
    (void)hipGetLastError();  // without the records every cull is a full pass (identical results)
    dfree(c->wstat);
  }
  HIP_TRY(reset_band(c));
  if (n > 0) {
    // Spatially compact query order (kd buckets of 64 = one wave): on the device from the uploaded
    // cloud (query_order_gpu.hip), or on the host (config query_order = 1)
    DevScratch S;
    const double* aos = d_in;
    if (!d_in) {
      double* up = nullptr;
      HIP_TRY(call_upload(S, &up, xyz, 3 * (size_t)n, c->stream));
      aos = up;
    }
    if (c->cfg.query_order == 0) {
      HIP_TRY(gpu_kd_query_order(aos, n, 8, c->perm, c->stream));
    } else {
      std::vector<double> staged;
      if (!xyz) {
        HIP_TRY(stage_down(c, &staged, d_in, 3 * (size_t)n));
        xyz = staged.data();
      }
      std::vector<int32_t> perm;
      kd_query_order(xyz, n, 8, &perm);
      HIP_TRY(hipMemcpyAsync(c->perm, perm.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // the host order is read by the copy
    }
    HIP_TRY(launch_gather_deinterleave(aos, c->perm, c->x, c->y, c->z, n, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->have_results = false;
    c->have_prev = false;
  }
  undo.dismiss();
  return ICP_HIP_OK;
}

int icp_hip_set_source(icp_hip_ctx* c, const double* xyz, int64_t n) {
  if (!c || (!xyz && n > 0) || n < 0) return fail(ICP_HIP_EINVAL, "bad source arguments");
  if (c->group) return group_set_source(c, xyz, n);
  return set_source_core(c, xyz, nullptr, n);
}

int icp_hip_set_source_device(icp_hip_ctx* c, const double* d_xyz, int64_t n) {
  if (!c || n < 0) return fail(ICP_HIP_EINVAL, "bad source arguments");
  if (const int rc = check_device_ptr(c, d_xyz, "set_source_device")) return rc;
  if (c->group) {  // the shards are cut and uploaded from host memory
    if (n > (int64_t)0x7fffffff) return fail(ICP_HIP_EINVAL, "set_source: 2^31 points or more (int32 query order)");
    std::vector<double> staged;
    HIP_TRY(stage_down(c, &staged, d_xyz, 3 * (size_t)n));
    return group_set_source(c, staged.data(), n);
  }
  return set_source_core(c, nullptr, d_xyz, n);
}

int icp_hip_copy_query_order(icp_hip_ctx* c, int32_t* perm_out) {
  if (!c || !perm_out) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_copy_query_order(c, perm_out);
  if (c->n_src == 0 || !c->perm) return fail(ICP_HIP_ENOTREADY, "source not set");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(perm_out, c->perm, sizeof(int32_t) * c->n_src, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_apply(icp_hip_ctx* c, const double* T) {
  if (!c || !T) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_apply(c, T);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_apply(T, c->x, c->y, c->z, c->n_src, c->stream));
  c->src_moves++;
  c->have_prev = false;  // queries moved without a search: previous residuals are no guess
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_get_source(icp_hip_ctx* c, double* xyz_out) {
  if (c && c->group) return xyz_out ? group_get_source(c, xyz_out) : fail(ICP_HIP_EINVAL, "null argument");
  if (!c || (!xyz_out && c->n_src > 0)) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->n_src == 0) return ICP_HIP_OK;
  HIP_TRY(hipSetDevice(c->device));
  DevScratch S;
  double* aos = nullptr;
  HIP_TRY(S.alloc(&aos, 3 * (size_t)c->n_src));
  HIP_TRY(launch_scatter_aos(c->perm, c->x, c->y, c->z, aos, c->n_src, c->stream));
  HIP_TRY(hipMemcpyAsync(xyz_out, aos, 3 * sizeof(double) * c->n_src, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_get_source_device(icp_hip_ctx* c, double* d_xyz_out) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (const int rc = check_device_ptr(c, d_xyz_out, "get_source_device")) return rc;
  if (c->group) {  // the members' shards are put back in the caller's order on the host
    std::vector<double> staged(3 * (size_t)group_n_src(c));
    const int rc = group_get_source(c, staged.data());
    if (rc != ICP_HIP_OK) return rc;
    HIP_TRY(stage_up(c, d_xyz_out, staged));
    return ICP_HIP_OK;
  }
  if (c->n_src == 0) return ICP_HIP_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_scatter_aos(c->perm, c->x, c->y, c->z, d_xyz_out, c->n_src, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ICP_HIP_OK;
}

int icp_hip_get_correspondences(icp_hip_ctx* c, int32_t* idx_out, double* dist_out) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_get_correspondences(c, idx_out, dist_out);
  return corr_core(c, true, idx_out, dist_out);
}

int icp_hip_get_correspondences_device(icp_hip_ctx* c, int32_t* d_idx_out, double* d_dist_out) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  // int32 indices: 4-byte aligned
  if (const int rc = check_optional_device_ptr(c, d_idx_out, "get_correspondences_device", 4)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_dist_out, "get_correspondences_device")) return rc;
  if (c->group) {
    const size_t n = (size_t)group_n_src(c);
    RelayOut<int32_t> idx(d_idx_out, n);
    RelayOut<double> d(d_dist_out, n);
    if (const int rc = group_get_correspondences(c, idx.host(), d.host())) return rc;
    return relay_up(c, idx, d);
  }
  return corr_core(c, false, d_idx_out, d_dist_out);
}

int icp_hip_nn(icp_hip_ctx* c, const double* q, int64_t n, int32_t* idx_out, double* dist_out) {
  if (!c || n < 0 || (n > 0 && !q)) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (c->group) return icp_hip_nn(group_member(c, 0), q, n, idx_out, dist_out);  // the replicated octree
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (n == 0) return ICP_HIP_OK;
  return nn_core(c, true, q, n, idx_out, dist_out);
}

int icp_hip_nn_device(icp_hip_ctx* c, const double* d_q, int64_t n, int32_t* d_idx_out, double* d_dist_out) {
  if (!c || n < 0) return fail(ICP_HIP_EINVAL, "bad arguments");
  if (const int rc = check_device_ptr(c, d_q, "nn_device")) return rc;
  if (const int rc = check_optional_device_ptr(c, d_idx_out, "nn_device", 4)) return rc;
  if (const int rc = check_optional_device_ptr(c, d_dist_out, "nn_device")) return rc;
  if (c->group) {  // the first member's replica, through host memory (the buffers may be another device's)
    std::vector<double> hq;
    HIP_TRY(stage_down(c, &hq, d_q, 3 * (size_t)n));
    RelayOut<int32_t> idx(d_idx_out, (size_t)n);
    RelayOut<double> d(d_dist_out, (size_t)n);
    if (const int rc = icp_hip_nn(group_member(c, 0), hq.data(), n, idx.host(), d.host())) return rc;
    return relay_up(c, idx, d);
  }
  if (!c->nodes) return fail(ICP_HIP_ENOTREADY, "target not set");
  if (n == 0) return ICP_HIP_OK;
  return nn_core(c, false, d_q, n, d_idx_out, d_dist_out);
}

int icp_hip_traversal_counts(icp_hip_ctx* c, double* mean_entries, double* mean_points) {
  if (!c || !mean_entries || !mean_points) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->group) return group_traversal_counts(c, mean_entries, mean_points);
  if (!c->nodes || (!c->x && c->n_src > 0)) return fail(ICP_HIP_ENOTREADY, "target/source not set");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->counters, 0, 2 * sizeof(unsigned long long), c->stream));
  NNLaunch a = base_launch(c);
  a.x = c->x;
  a.y = c->y;
  a.z = c->z;
  a.pos_out = c->pos;  // same queries as the last iterate: identical outputs are rewritten
  a.dist_out = c->dist;
  a.n = c->n_src;
  a.dbg = nullptr;
  a.count = 1;
  HIP_TRY(launch_nn(a, c->stream));
  unsigned long long h[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(h, c->counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double n = c->n_src > 0 ? (double)c->n_src : 1.0;
  *mean_entries = (double)h[0] / n;
  *mean_points = (double)h[1] / n;
  return ICP_HIP_OK;
}

}  // extern "C"
