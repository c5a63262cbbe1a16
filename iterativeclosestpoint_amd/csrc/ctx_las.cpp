// ctx_las.cpp — LAS files to and from clouds resident on the device (include/icp_las.h, the
// icp_hip_*_las calls): the raw records cross PCIe through two pinned staging buffers and are
// decoded / encoded by las_kernels.hip; whatever those kernels would not reproduce byte for byte
// (a file shorter than its header claims, records without room for three coordinates, coordinates
// no int32 holds) goes through the host reader / writers of lasio.cpp instead.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/icp_las.h"
#include "icp_ctx_internal.h"
#include "las_chunks.h"
#include "las_format.h"
#include "las_kernels.h"

using namespace icp;

// Two chunks in flight: while chunk k is copied and decoded (or encoded and copied), the host
// reads chunk k + 1 from the file (or writes chunk k - 1 to it).
struct LasIo {
  size_t cap = 0;  // bytes of each staging buffer
  uint8_t* pinned[2] = {nullptr, nullptr};
  uint8_t* dev[2] = {nullptr, nullptr};
  hipEvent_t done[2] = {nullptr, nullptr};
  unsigned long long* count = nullptr;
};

static void las_release(LasIo* io) {
  for (int b = 0; b < 2; b++) {
    if (io->pinned[b]) (void)hipHostFree(io->pinned[b]);
    dfree(io->dev[b]);
    if (io->done[b]) (void)hipEventDestroy(io->done[b]);
    io->pinned[b] = nullptr;
    io->done[b] = nullptr;
  }
  dfree(io->count);
  io->cap = 0;
}

void las_destroy(icp_hip_ctx* c) {
  if (!c->las) return;
  las_release(c->las);
  delete c->las;
  c->las = nullptr;
}

// The context's staging buffers, at its current chunk size. The device buffers end 16 bytes past
// the chunk: the decode loads whole 16-byte granules.
static int las_io(icp_hip_ctx* m, LasIo** out) {
  if (!m->las) m->las = new LasIo;
  LasIo* io = m->las;
  if (io->cap != m->las_chunk_bytes) {
    las_release(io);
    for (int b = 0; b < 2; b++) {
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&io->pinned[b]), m->las_chunk_bytes, hipHostMallocDefault));
      HIP_TRY(dalloc(&io->dev[b], m->las_chunk_bytes + 16));
      HIP_TRY(hipEventCreateWithFlags(&io->done[b], hipEventDisableTiming));
    }
    HIP_TRY(dalloc(&io->count, 1));
    io->cap = m->las_chunk_bytes;
  }
  *out = io;
  return ICP_HIP_OK;
}

// The single-device context that does the device work of a call (a group: its first member).
static icp_hip_ctx* worker(icp_hip_ctx* c) { return c->group ? group_member(c, 0) : c; }

static int las_error(int rc, const char* path) {
  return fail(ICP_HIP_EINVAL, std::string(rc == -2 ? "bad LAS signature or point count: " : "cannot read LAS file: ") + path);
}

static int64_t kept(int64_t n, int64_t stride) { return n <= 0 ? 0 : (n - 1) / stride + 1; }

// The host reader, then the stride on the host, then one upload: every file the decode kernels
// would not reproduce byte for byte.
static int read_fallback(icp_hip_ctx* c, const char* path, int rules, int64_t max_points, int64_t stride, int64_t n,
                         double* d_out, icp_las_header* hdr, int64_t* n_out) {
  std::vector<double> xyz(3 * (size_t)(n > 0 ? n : 1));
  const int64_t got = icp_las_read(path, rules, rules == ICP_LAS_CORE ? max_points : 0, xyz.data(), hdr);
  if (got < 0) return las_error((int)got, path);
  int64_t m = 0;
  for (int64_t i = 0; i < got; i += stride, m++)  // the CLI's `i += sample_rate` loop
    if (m != i) std::memcpy(&xyz[3 * m], &xyz[3 * i], 3 * sizeof(double));
  if (m > 0) {
    const int rc = icp_hip_dev_copy(c, d_out, xyz.data(), 3 * sizeof(double) * (size_t)m, ICP_HIP_COPY_H2D);
    if (rc != ICP_HIP_OK) return rc;
  }
  *n_out = m;
  c->las_device_path = 0;
  return ICP_HIP_OK;
}

// Decodes the file into d_out (room for the kept points of the span). d_out = null: only the
// header and the count (*n_out = the kept points), so that a caller can size its buffer.
static int read_las(icp_hip_ctx* c, const char* path, int rules, int64_t max_points, int64_t stride, double* d_out,
                    icp_las_header* hdr_out, int64_t* n_out) {
  if (stride < 1) return fail(ICP_HIP_EINVAL, "LAS stride must be at least 1");
  if (rules != ICP_LAS_CORE && rules != ICP_LAS_CLI) return fail(ICP_HIP_EINVAL, "unknown LAS rules");
  LasSpan sp;
  const int orc = las_span_open(path, rules, max_points, &sp);
  if (orc != 0) return las_error(orc, path);
  if (hdr_out) *hdr_out = sp.hdr;
  if (!d_out) {
    *n_out = kept(sp.n, stride);
    las_span_close(&sp);
    return ICP_HIP_OK;
  }
  if (sp.n == 0) {
    las_span_close(&sp);
    *n_out = 0;
    c->las_device_path = 1;
    return ICP_HIP_OK;
  }
  if (!sp.well_formed) {
    las_span_close(&sp);
    icp_las_header h;
    return read_fallback(c, path, rules, max_points, stride, sp.n, d_out, hdr_out ? hdr_out : &h, n_out);
  }
  icp_hip_ctx* m = worker(c);
  LasIo* io = nullptr;
  hipError_t e = hipSetDevice(m->device);
  const int rc = e == hipSuccess ? las_io(m, &io) : fail_hip("hipSetDevice", e);
  if (rc != ICP_HIP_OK) {
    las_span_close(&sp);
    return rc;
  }
  LasAxes ax;
  for (int a = 0; a < 3; a++) {
    ax.scale[a] = sp.hdr.scale[a];
    ax.offset[a] = sp.hdr.offset[a];
  }
  const int rl = sp.hdr.record_length;
  bool short_file = false;
  for (int k = 0; e == hipSuccess; k++) {
    const int b = k & 1;
    if (k >= 2) e = hipEventSynchronize(io->done[b]);  // the buffer's previous chunk has left it
    if (e != hipSuccess) break;
    int64_t first = 0;
    const int64_t cnt = las_span_read(&sp, io->pinned[b], io->cap, &first);
    if (cnt == 0) break;
    if (cnt < 0) {  // the file shrank under us
      short_file = true;
      break;
    }
    int64_t j0 = 0, out0 = 0;
    const int64_t sel = las_chunk_selection(first, cnt, stride, &j0, &out0);
    if (sel > 0) {
      // up to the last kept record's coordinates: what the kernel reads
      const size_t bytes = (size_t)((j0 + (sel - 1) * stride) * rl + 12);
      e = hipMemcpyAsync(io->dev[b], io->pinned[b], bytes, hipMemcpyHostToDevice, m->stream);
      if (e == hipSuccess) e = launch_las_decode(io->dev[b], rl, stride, j0, sel, d_out + 3 * out0, ax, m->stream);
    }
    if (e == hipSuccess) e = hipEventRecord(io->done[b], m->stream);
  }
  const hipError_t es = hipStreamSynchronize(m->stream);
  if (e == hipSuccess) e = es;
  las_span_close(&sp);
  if (e != hipSuccess) return fail_hip("LAS decode", e);
  if (short_file) return fail(ICP_HIP_EINVAL, std::string("LAS file changed while it was read: ") + path);
  *n_out = kept(sp.n, stride);
  c->las_device_path = 1;
  return ICP_HIP_OK;
}

// The fp64 cloud down, then the host writer of the flavour: clouds with a coordinate the encode
// kernel would not convert as the host's cast does.
static int write_fallback(icp_hip_ctx* c, const char* path, const double* d_xyz, int64_t n, int flavour,
                          const double* scale, const double* offset, const double* bounds) {
  std::vector<double> xyz(3 * (size_t)n);
  const int rc = icp_hip_dev_copy(c, xyz.data(), d_xyz, xyz.size() * sizeof(double), ICP_HIP_COPY_D2H);
  if (rc != ICP_HIP_OK) return rc;
  const int wrc = flavour == ICP_LAS_CLI ? icp_las_write_cli(path, xyz.data(), n, scale, offset)
                  : bounds               ? icp_las_write_core_bounds(path, xyz.data(), n, bounds)
                                         : icp_las_write_core(path, xyz.data(), n);
  if (wrc != 0) return fail(ICP_HIP_EINVAL, std::string("cannot write LAS file: ") + path);
  c->las_device_path = 0;
  return ICP_HIP_OK;
}

static int write_las(icp_hip_ctx* c, const char* path, const double* d_xyz, int64_t n, int flavour, const double* scale,
                     const double* offset, const double* bounds) {
  icp_hip_ctx* m = worker(c);
  LasIo* io = nullptr;
  HIP_TRY(hipSetDevice(m->device));
  if (const int rc = las_io(m, &io)) return rc;
  // the header's min and max, as the host loops compute them (lasio.cpp): the caller's bounds
  // (core), or partials per run of points folded in index order
  double mn[3], mx[3];
  if (flavour == ICP_LAS_CORE && bounds) {
    for (int a = 0; a < 3; a++) {
      mn[a] = bounds[2 * a];
      mx[a] = bounds[2 * a + 1];
    }
  } else {
    const int64_t np = las_bounds_parts(n);
    std::vector<double> parts(6 * (size_t)np);  // before its source's owner: outlives the copy
    DevScratch S;
    double* d_parts = nullptr;
    HIP_TRY(S.alloc(&d_parts, parts.size()));
    HIP_TRY(launch_las_bounds(d_xyz, n, d_parts, m->stream));
    HIP_TRY(hipMemcpyAsync(parts.data(), d_parts, parts.size() * sizeof(double), hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    for (int a = 0; a < 3; a++) {
      if (flavour == ICP_LAS_CLI) {  // from points[0]: run 0 begins with it, and a repeat changes nothing
        mn[a] = parts[a];
        mx[a] = parts[3 + a];
      } else {  // computeBounds starts from the largest and the lowest double
        mn[a] = std::numeric_limits<double>::max();
        mx[a] = std::numeric_limits<double>::lowest();
      }
      for (int64_t k = 0; k < np; k++) {
        const double lo = parts[6 * k + a], hi = parts[6 * k + 3 + a];
        if (lo < mn[a]) mn[a] = lo;
        if (hi > mx[a]) mx[a] = hi;
      }
    }
  }
  LasAxes ax;
  for (int a = 0; a < 3; a++) {
    ax.scale[a] = flavour == ICP_LAS_CLI ? scale[a] : 0.001;
    ax.offset[a] = flavour == ICP_LAS_CLI ? offset[a] : mn[a];
  }
  unsigned long long bad = 0;
  HIP_TRY(hipMemsetAsync(io->count, 0, sizeof(unsigned long long), m->stream));
  HIP_TRY(launch_las_count_unencodable(d_xyz, n, ax, io->count, m->stream));
  HIP_TRY(hipMemcpyAsync(&bad, io->count, sizeof(bad), hipMemcpyDeviceToHost, m->stream));
  HIP_TRY(hipStreamSynchronize(m->stream));
  if (bad != 0) return write_fallback(c, path, d_xyz, n, flavour, scale, offset, bounds);

  std::FILE* f = std::fopen(path, "wb");
  if (!f) return fail(ICP_HIP_EINVAL, std::string("cannot write LAS file: ") + path);
  char h[227];
  if (flavour == ICP_LAS_CLI) las_header_cli(h, (uint32_t)n, scale, offset, mn, mx);
  else las_header_core(h, (uint32_t)n, mn, mx);
  bool ok = std::fwrite(h, 1, 227, f) == 227;
  const int64_t per = (int64_t)(io->cap / 20);
  hipError_t e = hipSuccess;
  int64_t pending_cnt[2] = {0, 0};
  auto drain = [&](int b) {  // chunk in buffer b: wait for its copy, write it
    if (pending_cnt[b] == 0) return;
    if (e == hipSuccess) e = hipEventSynchronize(io->done[b]);
    if (e == hipSuccess && ok) ok = std::fwrite(io->pinned[b], 20, (size_t)pending_cnt[b], f) == (size_t)pending_cnt[b];
    pending_cnt[b] = 0;
  };
  int k = 0;
  for (int64_t first = 0; first < n && e == hipSuccess && ok; first += per, k++) {
    const int b = k & 1;
    drain(b);
    if (e != hipSuccess) break;
    const int64_t cnt = n - first < per ? n - first : per;
    e = launch_las_encode(d_xyz + 3 * first, cnt, ax, reinterpret_cast<uint32_t*>(io->dev[b]), m->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(io->pinned[b], io->dev[b], (size_t)cnt * 20, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipEventRecord(io->done[b], m->stream);
    if (e == hipSuccess) pending_cnt[b] = cnt;
  }
  drain(k & 1);  // the older chunk first
  drain((k + 1) & 1);
  const hipError_t es = hipStreamSynchronize(m->stream);
  if (e == hipSuccess) e = es;
  ok = (std::fclose(f) == 0) && ok;
  if (e != hipSuccess) return fail_hip("LAS encode", e);
  if (!ok) return fail(ICP_HIP_EINVAL, std::string("cannot write LAS file: ") + path);
  c->las_device_path = 1;
  return ICP_HIP_OK;
}

static int check_write_args(const icp_hip_ctx* c, const char* path, int flavour, const double* scale, const double* offset) {
  if (!c || !path) return fail(ICP_HIP_EINVAL, "null argument");
  if (flavour != ICP_LAS_CORE && flavour != ICP_LAS_CLI) return fail(ICP_HIP_EINVAL, "unknown LAS flavour");
  if (flavour == ICP_LAS_CLI && (!scale || !offset)) return fail(ICP_HIP_EINVAL, "the CLI flavour needs a scale and an offset");
  return ICP_HIP_OK;
}

extern "C" {

int icp_hip_read_las_device(icp_hip_ctx* c, const char* path, int las_rules, int64_t max_points, int64_t stride,
                            double* d_xyz_out, icp_las_header* hdr, int64_t* n_out) {
  if (!c || !path || !n_out) return fail(ICP_HIP_EINVAL, "null argument");
  if (d_xyz_out)
    if (const int rc = check_device_ptr(c, d_xyz_out, "read_las_device")) return rc;
  return read_las(c, path, las_rules, max_points, stride, d_xyz_out, hdr, n_out);
}

int icp_hip_write_las_device(icp_hip_ctx* c, const char* path, const double* d_xyz, int64_t n, int flavour,
                             const double scale[3], const double offset[3], const double bounds[6]) {
  if (const int rc = check_write_args(c, path, flavour, scale, offset)) return rc;
  if (n <= 0 || n > (int64_t)0xffffffffu) return fail(ICP_HIP_EINVAL, "LAS point count out of range [1, 2^32)");
  if (const int rc = check_device_ptr(c, d_xyz, "write_las_device")) return rc;
  return write_las(c, path, d_xyz, n, flavour, scale, offset, bounds);
}

// The decoded cloud lives in a scratch buffer for the length of the call: the builders read it in
// place (icp_hip_set_target_device / _set_source_device), nothing of it is retained.
static int set_from_las(icp_hip_ctx* c, const char* path, int las_rules, int64_t max_points, int64_t stride, bool target,
                        int max_tree_points, int max_depth, int rules, icp_las_header* hdr, int64_t* n_out) {
  if (!c || !path) return fail(ICP_HIP_EINVAL, "null argument");
  int64_t cap = 0, n = 0;
  int rc = read_las(c, path, las_rules, max_points, stride, nullptr, hdr, &cap);
  if (rc != ICP_HIP_OK) return rc;
  void* d = nullptr;
  rc = icp_hip_dev_alloc(c, 3 * sizeof(double) * (size_t)(cap > 0 ? cap : 1), &d);
  if (rc != ICP_HIP_OK) return rc;
  ScopeExit release([c, d] { (void)icp_hip_dev_free(c, d); });
  rc = read_las(c, path, las_rules, max_points, stride, static_cast<double*>(d), hdr, &n);
  if (rc != ICP_HIP_OK) return rc;
  rc = target ? icp_hip_set_target_device(c, static_cast<double*>(d), n, max_tree_points, max_depth, rules)
              : icp_hip_set_source_device(c, static_cast<double*>(d), n);
  if (rc == ICP_HIP_OK && n_out) *n_out = n;
  return rc;
}

int icp_hip_set_target_las(icp_hip_ctx* c, const char* path, int las_rules, int64_t max_points, int64_t stride,
                           int max_tree_points, int max_depth, int rules, icp_las_header* hdr, int64_t* n_out) {
  return set_from_las(c, path, las_rules, max_points, stride, true, max_tree_points, max_depth, rules, hdr, n_out);
}

int icp_hip_set_source_las(icp_hip_ctx* c, const char* path, int las_rules, int64_t max_points, int64_t stride,
                           icp_las_header* hdr, int64_t* n_out) {
  return set_from_las(c, path, las_rules, max_points, stride, false, 0, 0, 0, hdr, n_out);
}

int icp_hip_write_source_las(icp_hip_ctx* c, const char* path, int flavour, const double scale[3], const double offset[3],
                             const double bounds[6]) {
  if (const int rc = check_write_args(c, path, flavour, scale, offset)) return rc;
  const int64_t n = c->group ? group_n_src(c) : c->n_src;
  if (n <= 0) return fail(ICP_HIP_EINVAL, "write_source_las: no source");
  void* d = nullptr;
  int rc = icp_hip_dev_alloc(c, 3 * sizeof(double) * (size_t)n, &d);
  if (rc != ICP_HIP_OK) return rc;
  ScopeExit release([c, d] { (void)icp_hip_dev_free(c, d); });
  rc = icp_hip_get_source_device(c, static_cast<double*>(d));
  if (rc != ICP_HIP_OK) return rc;
  return write_las(c, path, static_cast<double*>(d), n, flavour, scale, offset, bounds);
}

int icp_hip_last_las_path(icp_hip_ctx* c, int32_t* device_path) {
  if (!c || !device_path) return fail(ICP_HIP_EINVAL, "null argument");
  if (c->las_device_path < 0) return fail(ICP_HIP_ENOTREADY, "no LAS call has run on this context");
  *device_path = c->las_device_path;
  return ICP_HIP_OK;
}

int icp_hip_set_las_chunk_bytes(icp_hip_ctx* c, size_t bytes) {
  if (!c) return fail(ICP_HIP_EINVAL, "null argument");
  if (bytes < ((size_t)1 << 16) || bytes > ((size_t)1 << 28))
    return fail(ICP_HIP_EINVAL, "LAS chunk size out of range [64 KiB, 256 MiB]");
  worker(c)->las_chunk_bytes = bytes;
  return ICP_HIP_OK;
}

}  // extern "C"
