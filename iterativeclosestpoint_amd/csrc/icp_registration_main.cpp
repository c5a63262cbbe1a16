// icp_registration — the reference's standalone CLI (icp_registration.cpp:817-949) on the
// MI355X path: LAS in, stride down-sampling, ICP() with the CLI's rules on the GPU
// (icp_cli_icp), LAS + transformation report out. Same files, same order, same defaults;
// the reference's hard-coded names and parameters become flags with those defaults.
//
//   icp_registration [--source Scan_096_origin.las] [--target Scannew_099.las]
//                    [--sample-rate 50] [--max-iters 20] [--tolerance 1e-2]
//                    [--outdir .] [--device 0 | --devices 0,1,...] [--device-io] [--pause]
//                    [--metric point|plane|gicp] [--normals-k 16] [--gicp-epsilon 1e-3] [--voxel X]
//                    [--sor K,RATIO] [--radius-filter R,MIN] [--trim F | --max-dist D]
//
// --trim F registers with the trimmed rejector (icp_engine_run_options, ICP_REJECT_TRIM): each
// iteration keeps the fraction F, in (0, 1], of its pairs with the smallest residuals, for scans that
// overlap only partly. --max-dist D keeps the pairs no farther apart than D metres
// (ICP_REJECT_MAX_DIST). One of the two at most, alone or with --metric plane / gicp; one GPU only. The
// CLI's rules, decisions and files otherwise. Without the flags every output is unchanged.
//
// --voxel X (metres, > 0) reduces each cloud, after the stride sampling, to the centroids of the
// voxels of edge X of a grid of its own with the origin at the cloud's minimum
// (icp_voxel_downsample; with --device-io icp_hip_voxel_downsample_device, nothing comes down). The
// sampled files hold the voxel clouds and the registration runs on the fp64 centroids. Without
// --sample-rate the stride is then 1. Without the flag every output is unchanged.
//
// --sor K,RATIO drops from each cloud the points whose mean distance to their K nearest other points
// exceeds mean + RATIO * std of those scores; --radius-filter R,MIN those with fewer than MIN other
// points within R metres (icp_hip_outlier_filter; with --device-io its _device variant, nothing
// comes down). Each runs on each cloud after the stride and after --voxel, before the normals and
// the loop; with both flags the radius filter runs first. The sampled files hold the filtered
// clouds. Without the flags every output is unchanged.
//
// --metric plane registers with the point-to-plane step (icp_engine_run_metric, ICP_METRIC_PLANE):
// the target's normals are estimated from --normals-k neighbours once the target is set; the CLI's
// rules, decisions and files otherwise. One GPU only. Without the flag every output is unchanged.
//
// --metric gicp registers with the generalized-ICP ("plane-to-plane") step (ICP_METRIC_GICP): the
// normals of the target and of the source are estimated from --normals-k neighbours, after the
// thinning and the filters and before the loop; --gicp-epsilon E, in [2^-20, 1], is the covariance
// along a normal (default 1e-3). The CLI's rules, decisions and files otherwise. One GPU only.
//
// --devices runs one registration over several GPUs of this process (icp_cli_icp_devices: the
// source sharded over them, the octree replicated, RCCL all-gathers per iteration).
//
// --device-io keeps both clouds resident on the GPU from file to file: the LAS records are decoded
// and sampled by kernels (icp_hip_set_source_las, icp_hip_read_las_device), the registration runs
// on the resident clouds and the four LAS outputs are encoded on the device
// (icp_hip_write_source_las, icp_hip_write_las_device). The same five files byte for byte; one
// GPU only (with --devices of more than one it is a usage error).
//
// Exit code 255 (the reference's `return -1`) when an input cannot be read.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/icp_engine.h"
#include "../../include/icp_hip.h"
#include "../../include/icp_host.h"
#include "../../include/icp_las.h"

namespace {

struct Args {
  std::string source = "Scan_096_origin.las";  // :825
  std::string target = "Scannew_099.las";      // :826
  long sample_rate = 50;                        // :858
  int max_iters = 20;                           // :900
  double tolerance = 1e-2;                      // :901
  std::string outdir = ".";
  std::vector<int> devices{0};
  bool device_io = false;
  bool pause = false;
  int metric = ICP_METRIC_POINT;
  int normals_k = 16;
  double gicp_epsilon = 1e-3;
  bool with_normals() const { return metric == ICP_METRIC_PLANE || metric == ICP_METRIC_GICP; }
  double voxel = 0.0;  // 0: no voxel grid
  int sor_k = 0;       // 0: no statistical filter
  double sor_ratio = 0.0;
  double radius = 0.0;  // 0: no radius filter
  int radius_min = 0;
  int reject = ICP_REJECT_SIGMA;  // --trim / --max-dist
  double reject_param = 0.0;
  bool filtered() const { return sor_k > 0 || radius > 0.0; }
};

[[noreturn]] void usage(const char* prog, int code) {
  std::fprintf(code ? stderr : stdout,
               "usage: %s [--source F] [--target F] [--sample-rate N] [--max-iters N] [--tolerance X]\n"
               "          [--outdir D] [--device N | --devices N,M,...] [--device-io] [--pause]\n"
               "          [--metric point|plane|gicp] [--normals-k N] [--gicp-epsilon E] [--voxel X]\n"
               "          [--sor K,RATIO] [--radius-filter R,MIN] [--trim F | --max-dist D]\n",
               prog);
  std::exit(code);
}

Args parse(int argc, char** argv) {
  Args a;
  bool rate_given = false;
  for (int i = 1; i < argc; i++) {
    const std::string k = argv[i];
    auto val = [&]() -> const char* {
      if (i + 1 >= argc) usage(argv[0], 2);
      return argv[++i];
    };
    if (k == "--source") a.source = val();
    else if (k == "--target") a.target = val();
    else if (k == "--sample-rate") {
      a.sample_rate = std::strtol(val(), nullptr, 10);
      rate_given = true;
    }
    else if (k == "--voxel") {
      const char* v = val();
      char* end = nullptr;
      a.voxel = std::strtod(v, &end);
      if (end == v || *end != '\0' || !(a.voxel - a.voxel == 0.0) || !(a.voxel > 0.0)) {
        std::fprintf(stderr, "--voxel must be a finite edge > 0 (metres)\n");
        usage(argv[0], 2);
      }
    }
    else if (k == "--sor") {
      const char* v = val();
      char *e1 = nullptr, *e2 = nullptr;
      const long kk = std::strtol(v, &e1, 10);
      if (e1 != v && *e1 == ',') a.sor_ratio = std::strtod(e1 + 1, &e2);
      if (e1 == v || *e1 != ',' || e2 == e1 + 1 || *e2 != '\0' || !(a.sor_ratio - a.sor_ratio == 0.0) || kk < 1 ||
          kk > ICP_HIP_KNN_MAX) {
        std::fprintf(stderr, "--sor must be K,RATIO with K in [1, %d] and a finite RATIO\n", ICP_HIP_KNN_MAX);
        usage(argv[0], 2);
      }
      a.sor_k = (int)kk;
    }
    else if (k == "--radius-filter") {
      const char* v = val();
      char *e1 = nullptr, *e2 = nullptr;
      long mm = 0;
      a.radius = std::strtod(v, &e1);
      if (e1 != v && *e1 == ',') mm = std::strtol(e1 + 1, &e2, 10);
      if (e1 == v || *e1 != ',' || e2 == e1 + 1 || *e2 != '\0' || !(a.radius - a.radius == 0.0) || !(a.radius > 0.0) ||
          mm < 1 || mm > 0x7fffffffL) {
        std::fprintf(stderr, "--radius-filter must be R,MIN with a finite R > 0 (metres) and MIN >= 1\n");
        usage(argv[0], 2);
      }
      a.radius_min = (int)mm;
    }
    else if (k == "--trim" || k == "--max-dist") {
      const bool trim = k == "--trim";
      const char* v = val();
      char* end = nullptr;
      const double x = std::strtod(v, &end);
      if (a.reject != ICP_REJECT_SIGMA) {
        std::fprintf(stderr, "--trim and --max-dist: one rejector at most\n");
        usage(argv[0], 2);
      }
      if (end == v || *end != '\0' || !(x > 0.0) || (trim ? !(x <= 1.0) : !(x - x == 0.0))) {
        std::fprintf(stderr, trim ? "--trim must be a fraction in (0, 1]\n" : "--max-dist must be a finite distance > 0 (metres)\n");
        usage(argv[0], 2);
      }
      a.reject = trim ? ICP_REJECT_TRIM : ICP_REJECT_MAX_DIST;
      a.reject_param = x;
    }
    else if (k == "--max-iters") a.max_iters = (int)std::strtol(val(), nullptr, 10);
    else if (k == "--tolerance") a.tolerance = std::strtod(val(), nullptr);
    else if (k == "--outdir") a.outdir = val();
    else if (k == "--device") a.devices = {(int)std::strtol(val(), nullptr, 10)};
    else if (k == "--devices") {
      a.devices.clear();
      std::string list = val();
      size_t p = 0;
      while (p <= list.size()) {
        const size_t q = list.find(',', p);
        const std::string tok = list.substr(p, q == std::string::npos ? std::string::npos : q - p);
        char* end = nullptr;
        const long d = std::strtol(tok.c_str(), &end, 10);
        if (tok.empty() || *end != '\0' || d < 0) usage(argv[0], 2);
        a.devices.push_back((int)d);
        if (q == std::string::npos) break;
        p = q + 1;
      }
    }
    else if (k == "--device-io") a.device_io = true;
    else if (k == "--metric") {
      const std::string m = val();
      if (m == "point") a.metric = ICP_METRIC_POINT;
      else if (m == "plane") a.metric = ICP_METRIC_PLANE;
      else if (m == "gicp") a.metric = ICP_METRIC_GICP;
      else usage(argv[0], 2);
    }
    else if (k == "--normals-k") a.normals_k = (int)std::strtol(val(), nullptr, 10);
    else if (k == "--gicp-epsilon") {
      const char* v = val();
      char* end = nullptr;
      a.gicp_epsilon = std::strtod(v, &end);
      if (end == v || *end != '\0' || !(a.gicp_epsilon >= 0x1p-20 && a.gicp_epsilon <= 1.0)) {
        std::fprintf(stderr, "--gicp-epsilon must be in [2^-20, 1]\n");
        usage(argv[0], 2);
      }
    }
    else if (k == "--pause") a.pause = true;
    else if (k == "-h" || k == "--help") usage(argv[0], 0);
    else usage(argv[0], 2);
  }
  if (a.voxel > 0.0 && !rate_given) a.sample_rate = 1;
  if (a.sample_rate < 1) {
    std::fprintf(stderr, "--sample-rate must be >= 1\n");
    std::exit(2);
  }
  if (a.device_io && a.devices.size() > 1) {
    std::fprintf(stderr, "--device-io runs on one GPU (clouds resident across a device group: not supported)\n");
    usage(argv[0], 2);
  }
  if (a.metric == ICP_METRIC_PLANE && a.devices.size() > 1) {
    std::fprintf(stderr, "--metric plane runs on one GPU (the plane sums are not exchanged between devices)\n");
    usage(argv[0], 2);
  }
  if (a.metric == ICP_METRIC_GICP && a.devices.size() > 1) {
    std::fprintf(stderr, "--metric gicp runs on one GPU (the source is sharded, the sums are not exchanged between devices)\n");
    usage(argv[0], 2);
  }
  if (a.reject != ICP_REJECT_SIGMA && a.devices.size() > 1) {
    std::fprintf(stderr, "--trim and --max-dist run on one GPU (the residuals are not exchanged between devices)\n");
    usage(argv[0], 2);
  }
  if (a.with_normals() && (a.normals_k < 3 || a.normals_k > ICP_HIP_KNN_MAX)) {
    std::fprintf(stderr, "--normals-k must be in [3, %d]\n", ICP_HIP_KNN_MAX);
    std::exit(2);
  }
  return a;
}

void print_cloud(int64_t n, const icp_las_header& hdr) {
  std::cout << "  " << n << " points, scale (" << hdr.scale[0] << ", " << hdr.scale[1] << ", " << hdr.scale[2]
            << "), offset (" << hdr.offset[0] << ", " << hdr.offset[1] << ", " << hdr.offset[2] << ")" << std::endl;
}

bool read_cloud(const std::string& path, std::vector<double>& xyz, icp_las_header& hdr) {
  std::cout << "  reading " << path << std::endl;
  if (icp_las_read_header(path.c_str(), ICP_LAS_CLI, &hdr) != 0) return false;
  xyz.resize((size_t)hdr.num_points * 3);
  const int64_t got = icp_las_read(path.c_str(), ICP_LAS_CLI, 0, xyz.data(), &hdr);
  if (got <= 0) return false;  // readLASFile returns read_count > 0 (:377)
  xyz.resize((size_t)got * 3);
  print_cloud(got, hdr);
  return true;
}

int fail(const Args& a, const char* msg) {
  std::cout << "error: " << msg << std::endl;
  if (a.pause) std::cin.get();
  return -1;
}

std::string out_path(const Args& a, const char* name) { return a.outdir + "/" + name; }

void print_transform(const double R[9], const double t[3]) {
  std::cout << "\n========== transform ==========" << std::endl << "R:" << std::endl;
  for (int i = 0; i < 3; i++)
    std::cout << "  [" << R[3 * i] << ", " << R[3 * i + 1] << ", " << R[3 * i + 2] << "]" << std::endl;
  std::cout << "\nt:\n  [" << t[0] << ", " << t[1] << ", " << t[2] << "]" << std::endl;
  std::cout << "===============================" << std::endl;
}

void print_voxel(const Args& a, int64_t ns0, int64_t ns, int64_t nt0, int64_t nt) {
  std::cout << "\nvoxel grid (" << a.voxel << " m)..." << std::endl;
  std::cout << "source: " << ns0 << " -> " << ns << " points\ntarget: " << nt0 << " -> " << nt << " points" << std::endl;
}

// The host flow's reductions: the cloud replaced by what call(in, n, out, &m) keeps of it (m <= n
// points; false: it failed).
template <class Call>
bool replace_cloud(std::vector<double>& xyz, Call call) {
  std::vector<double> out(xyz.size());
  int64_t m = 0;
  if (!call(xyz.data(), (int64_t)xyz.size() / 3, out.data(), &m)) return false;
  out.resize((size_t)m * 3);
  xyz.swap(out);
  return true;
}

// The --device-io flow's: *d_xyz (n points, a buffer of icp_hip_dev_alloc) replaced by a buffer of
// what call(in, n, out, &m) keeps of it; the old buffer is freed.
template <class Call>
bool replace_device_cloud(icp_hip_ctx* ctx, void** d_xyz, int64_t* n, Call call) {
  void* d_out = nullptr;
  int64_t m = 0;
  if (icp_hip_dev_alloc(ctx, 3 * sizeof(double) * (size_t)*n, &d_out) != ICP_HIP_OK) return false;
  if (!call(static_cast<const double*>(*d_xyz), *n, static_cast<double*>(d_out), &m)) {
    (void)icp_hip_dev_free(ctx, d_out);
    return false;
  }
  (void)icp_hip_dev_free(ctx, *d_xyz);
  *d_xyz = d_out;
  *n = m;
  return true;
}

// --voxel: the cloud replaced by the centroids of its voxels (its own grid, the origin at its minimum).
bool voxel_reduce(const Args& a, std::vector<double>& xyz) {
  return replace_cloud(xyz, [&](const double* in, int64_t n, double* out, int64_t* m) {
    *m = icp_voxel_downsample(in, n, a.voxel, nullptr, ICP_VOXEL_CENTROID, n, out, nullptr, nullptr, nullptr);
    return *m >= 0;
  });
}

bool voxel_reduce_device(const Args& a, icp_hip_ctx* ctx, void** d_xyz, int64_t* n) {
  return replace_device_cloud(ctx, d_xyz, n, [&](const double* in, int64_t n_in, double* out, int64_t* m) {
    return icp_hip_voxel_downsample_device(ctx, in, n_in, a.voxel, nullptr, ICP_VOXEL_CENTROID, n_in, out, nullptr,
                                           nullptr, m, nullptr) == ICP_HIP_OK;
  });
}

// One outlier filter's line: the points before, the points kept and the threshold.
void print_outlier(const char* cloud, const char* what, const icp_outlier_stats& st) {
  std::cout << "  " << cloud << " (" << what << "): " << st.n << " -> " << st.kept << " points, threshold " << st.threshold
            << std::endl;
}

void print_outlier_head(const Args& a) {
  std::cout << "\noutlier removal (";
  if (a.radius > 0.0) std::cout << "radius " << a.radius << " m, at least " << a.radius_min << (a.sor_k > 0 ? "; " : "");
  if (a.sor_k > 0) std::cout << "statistical, k=" << a.sor_k << ", ratio " << a.sor_ratio;
  std::cout << ")..." << std::endl;
}

// The filters of the flags in their order (radius, then statistical) as (mode, k, param, name).
struct OutlierPass {
  int mode, k;
  double param;
  const char* what;
};
std::vector<OutlierPass> outlier_passes(const Args& a) {
  std::vector<OutlierPass> v;
  if (a.radius > 0.0) v.push_back({ICP_OUTLIER_RADIUS, a.radius_min, a.radius, "radius"});
  if (a.sor_k > 0) v.push_back({ICP_OUTLIER_STATISTICAL, a.sor_k, a.sor_ratio, "statistical"});
  return v;
}

// --sor / --radius-filter: the cloud replaced by its kept points, through the device call.
bool outlier_reduce(const Args& a, icp_hip_ctx* ctx, const char* cloud, std::vector<double>& xyz) {
  for (const OutlierPass& f : outlier_passes(a)) {
    icp_outlier_stats st{};
    if (!replace_cloud(xyz, [&](const double* in, int64_t n, double* out, int64_t* m) {
          return icp_hip_outlier_filter(ctx, in, n, f.mode, f.k, f.param, n, out, nullptr, nullptr, m, &st) == ICP_HIP_OK;
        }))
      return false;
    print_outlier(cloud, f.what, st);
  }
  return true;
}

bool outlier_reduce_device(const Args& a, icp_hip_ctx* ctx, const char* cloud, void** d_xyz, int64_t* n) {
  for (const OutlierPass& f : outlier_passes(a)) {
    icp_outlier_stats st{};
    if (!replace_device_cloud(ctx, d_xyz, n, [&](const double* in, int64_t n_in, double* out, int64_t* m) {
          return icp_hip_outlier_filter_device(ctx, in, n_in, f.mode, f.k, f.param, n_in, out, nullptr, nullptr, m, &st) ==
                 ICP_HIP_OK;
        }))
      return false;
    print_outlier(cloud, f.what, st);
  }
  return true;
}

// ICP()'s parameters as the CLI sets them: its flags and rules.
icp_params cli_params(const Args& a) {
  icp_params p;
  icp_params_default(&p);
  p.max_iterations = a.max_iters;
  p.tolerance = a.tolerance;
  p.rules = ICP_RULES_CLI;
  return p;
}

// The run's options of the flags, and the line that names a rejector.
icp_run_options cli_options(const Args& a) {
  icp_run_options o;
  icp_run_options_default(&o);
  o.metric = a.metric;
  o.reject = a.reject;
  o.reject_param = a.reject_param;
  return o;
}

void print_metric(const Args& a) {
  if (a.metric == ICP_METRIC_PLANE)
    std::cout << "metric: point-to-plane, normals from " << a.normals_k << " neighbours" << std::endl;
  if (a.metric == ICP_METRIC_GICP)
    std::cout << "metric: generalized ICP, epsilon " << a.gicp_epsilon << ", normals of both clouds from " << a.normals_k
              << " neighbours" << std::endl;
}

// The normals the metric needs: the target's once the target is set, the source's (and the
// epsilon) once the source is.
int target_normals(const Args& a, icp_hip_ctx* ctx) {
  return a.with_normals() ? icp_hip_estimate_target_normals(ctx, a.normals_k, nullptr) : ICP_HIP_OK;
}

int source_normals(const Args& a, icp_hip_ctx* ctx) {
  if (a.metric != ICP_METRIC_GICP) return ICP_HIP_OK;
  const int rc = icp_hip_estimate_source_normals(ctx, a.normals_k, nullptr);
  return rc == ICP_HIP_OK ? icp_hip_set_gicp_epsilon(ctx, a.gicp_epsilon) : rc;
}

void print_rejector(const Args& a) {
  if (a.reject == ICP_REJECT_TRIM) std::cout << "rejector: trimmed, keeps " << a.reject_param << " of the pairs" << std::endl;
  if (a.reject == ICP_REJECT_MAX_DIST) std::cout << "rejector: pairs within " << a.reject_param << " m" << std::endl;
}

// The per-iteration transforms of a run's history, the first cap of them into out; *n_tr counts all.
void collect_transforms(const icp_result& res, const std::vector<icp_iteration_record>& hist, int32_t cap, double* out,
                        int32_t* n_tr) {
  *n_tr = 0;
  for (int32_t k = 0; k < res.n_history; k++) {
    if (!hist[k].has_transform) continue;
    if (*n_tr < cap) std::memcpy(out + 16 * (size_t)*n_tr, hist[k].transform, 16 * sizeof(double));
    (*n_tr)++;
  }
}

// --device-io: the default flow's steps on clouds that stay in HBM (one context; the same files).
int run_device_io(const Args& a) {
  icp_hip_ctx* ctx = nullptr;
  void* d_tgt = nullptr;
  void* d_src = nullptr;  // --voxel and the outlier filters: the decoded source on its way through them
  const bool staged = a.voxel > 0.0 || a.filtered();
  auto bail = [&](const char* msg) {
    std::cerr << msg << ": " << icp_hip_last_error() << std::endl;
    if (ctx) (void)icp_hip_dev_free(ctx, d_tgt);
    if (ctx) (void)icp_hip_dev_free(ctx, d_src);
    icp_hip_destroy(ctx);
    return fail(a, msg);
  };
  if (icp_hip_create(&ctx, a.devices[0]) != ICP_HIP_OK) return bail("cannot create the GPU context");

  // Read + stride down-sampling in one pass per file; readLASFile rejects an empty file (:377).
  icp_las_header hs{}, ht{};
  int64_t ns = 0, nt = 0;
  std::cout << "\nsource: " << a.source << std::endl << "  reading " << a.source << std::endl;
  if (staged) {  // into a buffer of ours first: the source is set from its reduced cloud below
    if (icp_hip_read_las_device(ctx, a.source.c_str(), ICP_LAS_CLI, 0, a.sample_rate, nullptr, &hs, &ns) != ICP_HIP_OK ||
        ns <= 0 || icp_hip_dev_alloc(ctx, 3 * sizeof(double) * (size_t)ns, &d_src) != ICP_HIP_OK ||
        icp_hip_read_las_device(ctx, a.source.c_str(), ICP_LAS_CLI, 0, a.sample_rate, static_cast<double*>(d_src), &hs,
                                &ns) != ICP_HIP_OK)
      return bail("cannot read the source point cloud");
  } else if (icp_hip_set_source_las(ctx, a.source.c_str(), ICP_LAS_CLI, 0, a.sample_rate, &hs, &ns) != ICP_HIP_OK || ns <= 0)
    return bail("cannot read the source point cloud");
  print_cloud((int64_t)hs.num_points, hs);
  std::cout << "\ntarget: " << a.target << std::endl << "  reading " << a.target << std::endl;
  // the decoded target stays in a buffer of ours: the octree is built from it and both target files written
  if (icp_hip_read_las_device(ctx, a.target.c_str(), ICP_LAS_CLI, 0, a.sample_rate, nullptr, &ht, &nt) != ICP_HIP_OK ||
      nt <= 0 || icp_hip_dev_alloc(ctx, 3 * sizeof(double) * (size_t)nt, &d_tgt) != ICP_HIP_OK ||
      icp_hip_read_las_device(ctx, a.target.c_str(), ICP_LAS_CLI, 0, a.sample_rate, static_cast<double*>(d_tgt), &ht,
                              &nt) != ICP_HIP_OK)
    return bail("cannot read the target point cloud");
  print_cloud((int64_t)ht.num_points, ht);
  std::cout << "\ndown-sampling (1/" << a.sample_rate << ")..." << std::endl;
  std::cout << "source: " << ns << " points\ntarget: " << nt << " points" << std::endl;
  if (a.voxel > 0.0) {
    const int64_t ns0 = ns, nt0 = nt;
    if (!voxel_reduce_device(a, ctx, &d_src, &ns) || !voxel_reduce_device(a, ctx, &d_tgt, &nt))
      return bail("cannot reduce the clouds to the voxel grid");
    print_voxel(a, ns0, ns, nt0, nt);
  }
  if (a.filtered()) {
    print_outlier_head(a);
    if (!outlier_reduce_device(a, ctx, "source", &d_src, &ns) || !outlier_reduce_device(a, ctx, "target", &d_tgt, &nt))
      return bail("cannot filter the clouds");
  }
  if (staged) {
    if (icp_hip_set_source_device(ctx, static_cast<double*>(d_src), ns) != ICP_HIP_OK)
      return bail(a.voxel > 0.0 ? "cannot reduce the clouds to the voxel grid" : "cannot filter the clouds");
    (void)icp_hip_dev_free(ctx, d_src);
    d_src = nullptr;
  }

  // both sampled clouds carry the SOURCE's scale/offset (:862-876)
  if (icp_hip_write_source_las(ctx, out_path(a, "sampled_source.las").c_str(), ICP_LAS_CLI, hs.scale, hs.offset, nullptr) !=
          ICP_HIP_OK ||
      icp_hip_write_las_device(ctx, out_path(a, "sampled_target.las").c_str(), static_cast<double*>(d_tgt), nt, ICP_LAS_CLI,
                               hs.scale, hs.offset, nullptr) != ICP_HIP_OK)
    return bail("cannot write the sampled clouds");

  std::cout << "\nparameters: max iterations=" << a.max_iters << ", tolerance=" << a.tolerance << std::endl;
  // ICP() (icp_cli_icp_devices) on the resident clouds: the CLI's octree (10 points, depth 20) and rules
  const icp_params p = cli_params(a);
  const int cap = a.max_iters > 0 ? a.max_iters : 1;
  std::vector<icp_iteration_record> hist((size_t)cap);
  icp_result res;
  if (icp_hip_set_target_device(ctx, static_cast<double*>(d_tgt), nt, 10, 20, ICP_RULES_CLI) != ICP_HIP_OK)
    return bail("registration failed");
  print_metric(a);
  if (target_normals(a, ctx) != ICP_HIP_OK) return bail("cannot estimate the target normals");
  if (source_normals(a, ctx) != ICP_HIP_OK) return bail("cannot estimate the source normals");
  print_rejector(a);
  const icp_run_options opt = cli_options(a);
  const int rc = a.reject == ICP_REJECT_SIGMA ? icp_engine_run_metric(ctx, &p, a.metric, &res, hist.data(), cap, nullptr)
                                              : icp_engine_run_options(ctx, &p, &opt, &res, hist.data(), cap, nullptr);
  if (rc != ICP_HIP_OK) {
    std::cerr << "ICP failed (" << rc << ")";
    return bail("registration failed");
  }
  std::vector<double> transforms((size_t)cap * 16);
  int32_t n_tr = 0;
  collect_transforms(res, hist, cap, transforms.data(), &n_tr);
  print_transform(res.final_R, res.final_t);

  if (icp_hip_write_source_las(ctx, out_path(a, "registered_source.las").c_str(), ICP_LAS_CLI, hs.scale, hs.offset,
                               nullptr) != ICP_HIP_OK ||
      icp_hip_write_las_device(ctx, out_path(a, "registered_target.las").c_str(), static_cast<double*>(d_tgt), nt,
                               ICP_LAS_CLI, hs.scale, hs.offset, nullptr) != ICP_HIP_OK ||
      icp_write_transform_report(out_path(a, "icp_transformation.txt").c_str(), res.final_R, res.final_t, transforms.data(),
                                 n_tr < cap ? n_tr : cap) != 0)
    return bail("cannot write the results");
  (void)icp_hip_dev_free(ctx, d_tgt);
  icp_hip_destroy(ctx);
  std::cout << "\ndone: registered_source.las, registered_target.las, icp_transformation.txt" << std::endl;
  if (a.pause) std::cin.get();
  return 0;
}

// ICP() with another metric or a rejector on host clouds: icp_cli_icp_devices' steps on one context,
// with the metric's normals estimated once the clouds are set. src is moved in place.
int cli_icp_options(const Args& a, double* src, int64_t ns, const double* tgt, int64_t nt, double R[9], double t[3],
                  double* transforms, int32_t cap, int32_t* n_tr) {
  const icp_params p = cli_params(a);
  std::vector<icp_iteration_record> hist((size_t)cap);
  icp_result res;
  icp_hip_ctx* ctx = nullptr;
  int rc = icp_hip_create(&ctx, a.devices[0]);
  if (rc == ICP_HIP_OK) rc = icp_hip_set_target(ctx, tgt, nt, 10, 20, ICP_RULES_CLI);
  if (rc == ICP_HIP_OK) rc = target_normals(a, ctx);
  if (rc == ICP_HIP_OK) rc = icp_hip_set_source(ctx, src, ns);
  if (rc == ICP_HIP_OK) rc = source_normals(a, ctx);
  const icp_run_options opt = cli_options(a);
  if (rc == ICP_HIP_OK)
    rc = a.reject == ICP_REJECT_SIGMA ? icp_engine_run_metric(ctx, &p, a.metric, &res, hist.data(), cap, nullptr)
                                      : icp_engine_run_options(ctx, &p, &opt, &res, hist.data(), cap, nullptr);
  if (rc == ICP_HIP_OK) rc = icp_hip_get_source(ctx, src);
  icp_hip_destroy(ctx);
  if (rc != ICP_HIP_OK) return rc;
  std::memcpy(R, res.final_R, sizeof(res.final_R));
  std::memcpy(t, res.final_t, sizeof(res.final_t));
  collect_transforms(res, hist, cap, transforms, n_tr);
  return ICP_HIP_OK;
}

}  // namespace

int main(int argc, char** argv) {
  const Args a = parse(argc, argv);
  std::cout << "=== ICP point-cloud fine registration (MI355X) ===" << std::endl;
  if (a.device_io) return run_device_io(a);

  std::vector<double> src, tgt;
  icp_las_header hs{}, ht{};
  std::cout << "\nsource: " << a.source << std::endl;
  if (!read_cloud(a.source, src, hs)) return fail(a, "cannot read the source point cloud");
  std::cout << "\ntarget: " << a.target << std::endl;
  if (!read_cloud(a.target, tgt, ht)) return fail(a, "cannot read the target point cloud");

  // Stride down-sampling; both sampled clouds carry the SOURCE's scale/offset (:862-876).
  std::cout << "\ndown-sampling (1/" << a.sample_rate << ")..." << std::endl;
  std::vector<double> ss, ts;
  for (size_t i = 0; i < src.size() / 3; i += (size_t)a.sample_rate) ss.insert(ss.end(), &src[3 * i], &src[3 * i] + 3);
  for (size_t i = 0; i < tgt.size() / 3; i += (size_t)a.sample_rate) ts.insert(ts.end(), &tgt[3 * i], &tgt[3 * i] + 3);
  int64_t ns = (int64_t)ss.size() / 3, nt = (int64_t)ts.size() / 3;
  std::cout << "source: " << ns << " points\ntarget: " << nt << " points" << std::endl;
  src.clear();
  src.shrink_to_fit();
  tgt.clear();
  tgt.shrink_to_fit();
  if (a.voxel > 0.0) {
    const int64_t ns0 = ns, nt0 = nt;
    if (!voxel_reduce(a, ss) || !voxel_reduce(a, ts)) {
      std::cerr << "voxel grid: " << icp_hip_last_error() << std::endl;
      return fail(a, "cannot reduce the clouds to the voxel grid");
    }
    ns = (int64_t)ss.size() / 3, nt = (int64_t)ts.size() / 3;
    print_voxel(a, ns0, ns, nt0, nt);
  }
  if (a.filtered()) {
    print_outlier_head(a);
    icp_hip_ctx* fctx = nullptr;
    const bool ok = icp_hip_create(&fctx, a.devices[0]) == ICP_HIP_OK && outlier_reduce(a, fctx, "source", ss) &&
                    outlier_reduce(a, fctx, "target", ts);
    icp_hip_destroy(fctx);
    if (!ok) {
      std::cerr << "outlier removal: " << icp_hip_last_error() << std::endl;
      return fail(a, "cannot filter the clouds");
    }
    ns = (int64_t)ss.size() / 3, nt = (int64_t)ts.size() / 3;
  }

  if (icp_las_write_cli(out_path(a, "sampled_source.las").c_str(), ss.data(), ns, hs.scale, hs.offset) != 0 ||
      icp_las_write_cli(out_path(a, "sampled_target.las").c_str(), ts.data(), nt, hs.scale, hs.offset) != 0)
    return fail(a, "cannot write the sampled clouds");

  std::cout << "\nparameters: max iterations=" << a.max_iters << ", tolerance=" << a.tolerance << std::endl;
  double R[9], t[3];
  const int cap = a.max_iters > 0 ? a.max_iters : 1;
  std::vector<double> transforms((size_t)cap * 16);
  int32_t n_tr = 0;
  if (a.devices.size() > 1) std::cout << "devices: " << a.devices.size() << " GPUs" << std::endl;
  print_metric(a);
  print_rejector(a);
  const int rc = a.with_normals() || a.reject != ICP_REJECT_SIGMA
                     ? cli_icp_options(a, ss.data(), ns, ts.data(), nt, R, t, transforms.data(), cap, &n_tr)
                     : icp_cli_icp_devices(ss.data(), ns, ts.data(), nt, a.max_iters, a.tolerance, R, t, transforms.data(),
                                           cap, &n_tr, (int)a.devices.size(), a.devices.data());
  if (rc != 0) {
    std::cerr << "ICP failed (" << rc << "): " << icp_hip_last_error() << std::endl;
    return fail(a, "registration failed");
  }

  print_transform(R, t);

  // The source cloud was moved in place by ICP() (:598-605); the target is written unchanged.
  if (icp_las_write_cli(out_path(a, "registered_source.las").c_str(), ss.data(), ns, hs.scale, hs.offset) != 0 ||
      icp_las_write_cli(out_path(a, "registered_target.las").c_str(), ts.data(), nt, hs.scale, hs.offset) != 0 ||
      icp_write_transform_report(out_path(a, "icp_transformation.txt").c_str(), R, t, transforms.data(),
                                 n_tr < cap ? n_tr : cap) != 0)
    return fail(a, "cannot write the results");
  std::cout << "\ndone: registered_source.las, registered_target.las, icp_transformation.txt" << std::endl;
  if (a.pause) std::cin.get();
  return 0;
}
