// lk_epipolar_search.cpp - host side of the stereo initial guess along the epipolar curve (include/lk_engine.h:
// lk_search_epipolar, lk_get_epipolar_search_info, lk_get_epipolar_search_profile, lk_epipolar_curves).  The kernels are
// lk_epipolar_search.hip; the cameras are lk_stereo.hpp's functions, compiled for the host here as in lk_stereo.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_stereo.hpp"

namespace {

constexpr double kMaxDisplacement = 1073741824.0; // 2^30: a displacement of this size or above is no curve
constexpr int kRunCandidates = 1024;              // shape = 0: the candidates of a workgroup at most (four per lane)

// the table of a call as the host builds it
struct EpTable {
  std::vector<lk_epipolar_curve> curve; // [n]
  std::vector<int32_t> other, node;     // [stations]
  std::vector<double> inv_depth;        // [stations]
  std::vector<float> shape;             // [n][N][4] (shape = 1)
};

// what the pass keeps on its slot of the engine: the table on both sides, the per-node records, the results of the last call
struct LkEpipolarState : LkPassSlot {
  LkDevBytes curve, other, node, inv_depth, shape, run, rec, profile, match;
  EpTable table;
  std::vector<int2> h_run;
  std::vector<float> h_centres;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; // before the search kernel, between the two, after the reduce kernel
  int S = 0;                 // what `match` and `profile` hold (0: no search yet)
  double curves_ms = 0.0;    // the host's time for the table of the last call
  long long candidates = 0;  // stations times band over all sectors
  int win_bytes = 0, max_run = 0;
  hipError_t init() {
    hipError_t err = hipSuccess;
    for (int i = 0; i < 3 && err == hipSuccess; ++i)
      err = hipEventCreate(&ev[i]);
    return err;
  }
  ~LkEpipolarState() override {
    for (hipEvent_t x : ev)
      if (x)
        (void)hipEventDestroy(x);
  }
};

bool depths_ok(double z_near, double z_far) { return std::isfinite(z_near) && std::isfinite(z_far) && z_near > 0.0 && z_near <= z_far; }

// null: usable; else what is wrong with the configuration, the cameras or the depth ranges (level and slot are the engine's)
const char *refusal(const lk_epipolar_search *cfg, const lk_camera *cams, int n, const double *depth_range) {
  if (!cfg)
    return "no configuration";
  if (cfg->search.radius < 0 || cfg->search.radius > LK_EP_MAX_BAND)
    return "the band (search.radius) must be in 0 .. LK_EP_MAX_BAND";
  if (cfg->n_nodes < 2 || cfg->n_nodes > LK_EP_MAX_NODES)
    return "n_nodes must be in 2 .. LK_EP_MAX_NODES";
  if (cfg->shape != 0 && cfg->shape != 1)
    return "shape must be 0 or 1";
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return "reserved words must be 0";
  if (!depths_ok(cfg->z_near, cfg->z_far))
    return "depths must be 0 < z_near <= z_far, both finite";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(cfg->normal[i]))
      return "the normal must be finite";
  if (!cams)
    return "no cameras";
  const double origin[3] = {0.0, 0.0, 0.0};
  double px[2];
  for (int k = 0; k < 2; ++k)
    if (lk_stereo_project(cams + k, 1, origin, px, nullptr) != LK_ERROR_NONE)
      return k ? "camera 1 is one that lk_stereo_project refuses" : "camera 0 is one that lk_stereo_project refuses";
  if (depth_range)
    for (int s = 0; s < n; ++s)
      if (!depths_ok(depth_range[2 * (size_t)s], depth_range[2 * (size_t)s + 1]))
        return "every depth_range entry must be 0 < z_near <= z_far, both finite";
  return nullptr;
}

// camera-0 pixel p -> camera-1 pixel over the plane n . (X - P) = 0; false: the point fails
bool over_plane(const lk_camera *cams, double px, double py, const double *P, const double *nrm, double &qx, double &qy) {
  double mu, mv, o[3], d[3];
  if (lk_stereo_undistort(cams[0], px, py, mu, mv))
    return false;
  lk_stereo_ray(cams[0], mu, mv, o, d);
  const double dn = (d[0] * nrm[0] + d[1] * nrm[1]) + d[2] * nrm[2];
  if (dn == 0.0)
    return false;
  const double z = (((P[0] - o[0]) * nrm[0] + (P[1] - o[1]) * nrm[1]) + (P[2] - o[2]) * nrm[2]) / dn;
  if (!(z > 0.0))
    return false;
  if (lk_stereo_project_impl(cams[1], o[0] + z * d[0], o[1] + z * d[1], o[2] + z * d[2], qx, qy))
    return false;
  return std::isfinite(qx) && std::isfinite(qy);
}

// the curve of one centre, appended to the table (include/lk_engine.h, `curve`)
void one_curve(const lk_epipolar_search *cfg, const lk_camera *cams, double cx, double cy, double z_near, double z_far, int level,
               EpTable &t, float *shape4N) {
  const int N = cfg->n_nodes, B = cfg->search.radius;
  lk_epipolar_curve cv{};
  cv.first_index = (int32_t)t.other.size();
  cv.status = LK_GS_NO_CURVE;
  const double inv = 1.0 / (double)(1 << level);
  double mu, mv, o[3], d[3];
  double rho[LK_EP_MAX_NODES], wx[LK_EP_MAX_NODES], wy[LK_EP_MAX_NODES], P[LK_EP_MAX_NODES][3];
  bool ok = !lk_stereo_undistort(cams[0], cx, cy, mu, mv);
  if (ok) {
    lk_stereo_ray(cams[0], mu, mv, o, d);
    const double rho_near = 1.0 / z_near, rho_far = 1.0 / z_far, step = (rho_far - rho_near) / (double)(N - 1);
    for (int k = 0; k < N && ok; ++k) {
      rho[k] = rho_near + (double)k * step;
      const double z = 1.0 / rho[k];
      double qx, qy;
      for (int i = 0; i < 3; ++i)
        P[k][i] = o[i] + z * d[i];
      ok = !lk_stereo_project_impl(cams[1], P[k][0], P[k][1], P[k][2], qx, qy);
      wx[k] = (qx - cx) * inv;
      wy[k] = (qy - cy) * inv;
      ok = ok && std::fabs(wx[k]) < kMaxDisplacement && std::fabs(wy[k]) < kMaxDisplacement; // (false for a NaN)
    }
  }
  if (ok) {
    cv.axis = std::fabs(wx[N - 1] - wx[0]) >= std::fabs(wy[N - 1] - wy[0]) ? 0 : 1;
  }
  const double *a = cv.axis == 0 ? wx : wy, *b = cv.axis == 0 ? wy : wx;
  const bool up = ok && a[N - 1] >= a[0];
  for (int k = 0; k + 1 < N && ok; ++k)
    ok = up ? a[k + 1] >= a[k] : a[k + 1] <= a[k];
  if (ok && cfg->shape) {
    double nrm[3] = {cfg->normal[0], cfg->normal[1], cfg->normal[2]};
    if (nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0)
      nrm[0] = cams[0].R[6], nrm[1] = cams[0].R[7], nrm[2] = cams[0].R[8];
    for (int k = 0; k < N && ok; ++k) {
      double xp[2], xm[2], yp[2], ym[2];
      ok = over_plane(cams, cx + 1.0, cy, P[k], nrm, xp[0], xp[1]) && over_plane(cams, cx - 1.0, cy, P[k], nrm, xm[0], xm[1]) &&
           over_plane(cams, cx, cy + 1.0, P[k], nrm, yp[0], yp[1]) && over_plane(cams, cx, cy - 1.0, P[k], nrm, ym[0], ym[1]);
      if (!ok)
        break;
      shape4N[4 * k] = (float)((xp[0] - xm[0]) / 2.0);
      shape4N[4 * k + 1] = (float)((yp[0] - ym[0]) / 2.0);
      shape4N[4 * k + 2] = (float)((xp[1] - xm[1]) / 2.0);
      shape4N[4 * k + 3] = (float)((yp[1] - ym[1]) / 2.0);
    }
    if (!ok)
      for (int i = 0; i < 4 * N; ++i)
        shape4N[i] = 0.f;
  }
  if (!ok) {
    cv.axis = 0;
    t.curve.push_back(cv);
    return;
  }
  const double lo = std::min(a[0], a[N - 1]), hi = std::max(a[0], a[N - 1]);
  double t0 = std::ceil(lo), t1 = std::floor(hi);
  if (t0 > t1)
    t0 = t1 = std::floor((lo + hi) / 2.0 + 0.5);
  cv.status = LK_GS_TOO_LONG;
  if (t1 - t0 + 1.0 > (double)LK_EP_MAX_STATIONS) {
    t.curve.push_back(cv);
    return;
  }
  const int first = (int)t0, count = (int)(t1 - t0) + 1;
  int j = 0, run_node = -1, run_len = 0; // j: the segment in the order of increasing a
  for (int m = 0; m < count; ++m) {
    const double tt = (double)(first + m);
    int k = up ? j : N - 2 - j;
    while (j < N - 2 && !((up ? a[k + 1] : a[k]) >= tt)) {
      ++j;
      k = up ? j : N - 2 - j;
    }
    const double den = a[k + 1] - a[k];
    double lam = den == 0.0 ? 0.0 : (tt - a[k]) / den;
    lam = lam < 0.0 ? 0.0 : lam > 1.0 ? 1.0 : lam;
    const int nd = lam < 0.5 ? k : k + 1;
    t.other.push_back((int32_t)std::floor(b[k] + lam * (b[k + 1] - b[k]) + 0.5));
    t.node.push_back(nd);
    t.inv_depth.push_back(rho[k] + lam * (rho[k + 1] - rho[k]));
    run_len = nd == run_node ? run_len + 1 : 1;
    run_node = nd;
    if ((long long)run_len * (2 * B + 1) > LK_EP_MAX_GROUP) {
      t.other.resize((size_t)cv.first_index);
      t.node.resize((size_t)cv.first_index);
      t.inv_depth.resize((size_t)cv.first_index);
      t.curve.push_back(cv);
      return;
    }
  }
  cv.status = 0;
  cv.first_station = first;
  cv.n_stations = count;
  t.curve.push_back(cv);
}

// the table of n centres (the inputs have passed refusal())
void build_table(const lk_epipolar_search *cfg, const lk_camera *cams, int n, const float *centres, const double *depth_range, int level,
                 EpTable &t) {
  const int N = cfg->n_nodes;
  t.curve.clear();
  t.other.clear();
  t.node.clear();
  t.inv_depth.clear();
  t.curve.reserve((size_t)n);
  t.shape.assign(cfg->shape ? (size_t)n * (size_t)N * 4 : 0, 0.f);
  for (int s = 0; s < n; ++s) {
    const double zn = depth_range ? depth_range[2 * (size_t)s] : cfg->z_near, zf = depth_range ? depth_range[2 * (size_t)s + 1] : cfg->z_far;
    one_curve(cfg, cams, (double)centres[2 * (size_t)s], (double)centres[2 * (size_t)s + 1], zn, zf, level, t,
              cfg->shape ? t.shape.data() + (size_t)s * (size_t)N * 4 : nullptr);
  }
}

// the results of the last search, once it covers the committed sectors
int last_search(lk_engine *e, const char *who, LkEpipolarState **st) {
  *st = static_cast<LkEpipolarState *>(*lk_internal_pass_slot(e, LK_PASS_EPIPOLAR));
  if (!*st || (*st)->S <= 0 || (*st)->S != lk_internal_sector_count(e))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": no epipolar search of the committed sectors").c_str());
  return LK_ERROR_NONE;
}

template <class T> hipError_t upload(LkDevBytes &dst, const std::vector<T> &src, hipStream_t stream) {
  hipError_t err = dst.ensure(sizeof(T) * std::max<size_t>(src.size(), 1));
  if (err == hipSuccess && !src.empty()) // (pageable source: the copy has left it when the call returns)
    err = hipMemcpyAsync(dst.p, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice, stream);
  return err;
}

} // namespace

extern "C" {

int lk_epipolar_curves(const lk_epipolar_search *cfg, const lk_camera *cams, int n, const float *centres, const double *depth_range,
                       int level, lk_epipolar_curve *curves_out, int *n_stations_out, int capacity, int32_t *other_out,
                       int32_t *node_out, double *inv_depth_out, float *shape_out) {
  if (n < 1 || !centres || !curves_out || !n_stations_out || level < 0 || level > 30 || refusal(cfg, cams, n, depth_range))
    return LK_ERROR_BAD_DOMAIN;
  const bool arrays = other_out || node_out || inv_depth_out || shape_out;
  if (arrays && (!other_out || !node_out || !inv_depth_out || (cfg->shape && !shape_out)))
    return LK_ERROR_BAD_DOMAIN;
  EpTable t;
  build_table(cfg, cams, n, centres, depth_range, level, t);
  if (arrays && (size_t)std::max(capacity, 0) < t.other.size())
    return LK_ERROR_BAD_DOMAIN;
  std::copy(t.curve.begin(), t.curve.end(), curves_out);
  *n_stations_out = (int)t.other.size();
  if (arrays) {
    std::copy(t.other.begin(), t.other.end(), other_out);
    std::copy(t.node.begin(), t.node.end(), node_out);
    std::copy(t.inv_depth.begin(), t.inv_depth.end(), inv_depth_out);
    if (cfg->shape)
      std::copy(t.shape.begin(), t.shape.end(), shape_out);
  }
  return LK_ERROR_NONE;
}

int lk_search_epipolar(lk_engine *e, const lk_epipolar_search *cfg, const lk_camera *cams, const double *depth_range,
                       float *guesses_inout) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_epipolar: no configuration");
  const lk_guess_search &gs = cfg->search;
  if (gs.level < -1 || gs.def_slot < -1 || !(gs.min_score == gs.min_score))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_epipolar: bad level, ring slot or min_score");
  LkGuessSearchView v{};
  if (int rc = lk_internal_guess_search_view(e, gs.level, gs.def_slot, &v, "lk_search_epipolar")) // (level -1: py_stop)
    return rc;
  if (v.model == LK_FM_U)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_epipolar: LK_FM_U has no parameter for the second coordinate of a displacement");
  if (cfg->shape == 1 && v.model != LK_FM_UVUXUYVXVY)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_epipolar: shape = 1 needs LK_FM_UVUXUYVXVY, the model that carries a matrix");
  if (const char *why = refusal(cfg, cams, v.S, depth_range))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string("lk_search_epipolar: ") + why).c_str());
  LkEpipolarState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_EPIPOLAR, "lk_search_epipolar: state", &st))
    return rc;
  st->S = 0;
  const int S = v.S, N = cfg->n_nodes, B = gs.radius;

  // the table, from the host's centres, before anything is enqueued
  const auto t_begin = std::chrono::steady_clock::now();
  st->h_centres.resize(2 * (size_t)std::max(S, 1));
  for (int s = 0; s < S; ++s)
    if (int rc = lk_get_sector_info(e, s, nullptr, &st->h_centres[2 * (size_t)s], &st->h_centres[2 * (size_t)s + 1]))
      return rc;
  EpTable &t = st->table;
  build_table(cfg, cams, S, st->h_centres.data(), depth_range, v.level, t);
  // The runs of stations the workgroups take.  shape = 1: a node's stations, which share its matrix (run k of a sector is node
  // k's).  shape = 0: every station shares the identity, so a curve is cut into runs of at most kRunCandidates candidates and
  // a short curve is one workgroup's; the hook LK_EPIPOLAR_RUNS=1 (tests, scripts/epipolar_bench.py) cuts by node there too -
  // the same bytes, the decomposition DESIGN.md section 33 measures against.  Then the longest run, and the window the
  // largest workgroup reads: the template's box (an implicit rectangle's, under the node's matrix with the rounding's pixel on
  // either side) widened by the run's displacements.  Only a bound for the launch: the kernel decides per workgroup, from the
  // window it meets, whether the window is staged.
  // A cut by node rests on this: node(t) is monotone in m (the segments are taken in the order of increasing coordinate and
  // lambda grows within one), so the stations of a node are ONE contiguous run and every run has its own entry of h_run.  A
  // segment rule that let a node come back would overwrite an entry: the walk below refuses to write one twice.
  const bool by_node = cfg->shape != 0 || lk_pass_env_choice("LK_EPIPOLAR_RUNS", 0, 1, 0) == 1;
  const int chunk = std::max(1, kRunCandidates / (2 * B + 1));
  int n_runs = 1;
  if (by_node)
    n_runs = N;
  else
    for (int s = 0; s < S; ++s)
      n_runs = std::max(n_runs, (t.curve[(size_t)s].n_stations + chunk - 1) / chunk);
  st->h_run.assign((size_t)std::max(S, 1) * (size_t)n_runs, int2{0, 0});
  int max_run = 1;
  long long need = 0, stations = 0;
  bool lists = false;
  for (int s = 0; s < S; ++s) {
    const lk_epipolar_curve &cv = t.curve[(size_t)s];
    const int4 r = v.h_rect[s];
    if (r.z <= 0 && v.h_off[s + 1] > v.h_off[s])
      lists = true;
    stations += cv.n_stations;
    for (int m = 0; m < cv.n_stations;) {
      const size_t at = (size_t)cv.first_index + (size_t)m;
      const int nd = t.node[at];
      int len = 0, lo = t.other[at], hi = t.other[at];
      for (; m + len < cv.n_stations && (by_node ? t.node[at + (size_t)len] == nd : len < chunk); ++len) {
        lo = std::min(lo, t.other[at + (size_t)len]);
        hi = std::max(hi, t.other[at + (size_t)len]);
      }
      int2 &entry = st->h_run[(size_t)s * (size_t)n_runs + (size_t)(by_node ? nd : m / chunk)];
      if (entry.y != 0)
        return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_search_epipolar: internal: the stations of a node are not one run");
      entry = int2{m, len};
      max_run = std::max(max_run, len);
      if (r.z > 0) {
        long long bw = r.z, bh = r.w / r.z;
        if (cfg->shape) {
          const float *A = t.shape.data() + ((size_t)s * (size_t)N + (size_t)nd) * 4;
          const double w1 = (double)(r.z - 1), h1 = (double)(r.w / r.z - 1);
          bw = (long long)(std::fabs((double)A[0]) * w1 + std::fabs((double)A[1]) * h1) + 3;
          bh = (long long)(std::fabs((double)A[2]) * w1 + std::fabs((double)A[3]) * h1) + 3;
        }
        const long long along = len, across = (long long)hi - lo + 2 * B + 1;
        need = std::max(need, (bw - 1 + (cv.axis == 0 ? along : across)) * (bh - 1 + (cv.axis == 0 ? across : along)));
      }
      m += len;
    }
  }
  const int max_cand = max_run * (2 * B + 1);
  const int budget = lk_epipolar_search_window_budget(max_run, max_cand);
  if (lists)
    need = budget;
  st->curves_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  st->candidates = stations * (2 * B + 1);
  st->max_run = max_run;

  const size_t cells = (size_t)std::max(S, 1) * (size_t)n_runs;
  LK_HIPCHK(st->rec.ensure(sizeof(LkEpNodeRecord) * cells));
  LK_HIPCHK(st->profile.ensure(sizeof(double) * std::max<size_t>(t.other.size(), 1)));
  LK_HIPCHK(st->match.ensure(sizeof(lk_epipolar_match) * (size_t)std::max(S, 1)));
  LK_HIPCHK(upload(st->curve, t.curve, v.stream));
  LK_HIPCHK(upload(st->other, t.other, v.stream));
  LK_HIPCHK(upload(st->node, t.node, v.stream));
  LK_HIPCHK(upload(st->inv_depth, t.inv_depth, v.stream));
  LK_HIPCHK(upload(st->shape, t.shape, v.stream));
  LK_HIPCHK(upload(st->run, st->h_run, v.stream));

  LkEpipolarSearchArgs a{};
  a.gs.und = v.und;
  a.gs.def = v.def;
  a.gs.urows = v.urows;
  a.gs.ucols = v.ucols;
  a.gs.drows = v.drows;
  a.gs.dcols = v.dcols;
  a.gs.xy = v.xy;
  a.gs.off = v.off;
  a.gs.rect = v.rect;
  a.gs.guess = v.d_guess;
  a.gs.prev_p = v.d_prev_p;
  a.gs.match = nullptr;
  a.gs.n_sectors = S;
  a.gs.level = v.level;
  a.gs.radius = B;
  a.gs.has_v = 1;
  a.gs.min_samples = gs.min_samples > 0 ? gs.min_samples : 9;
  a.gs.min_score = gs.min_score;
  a.gs.win_bytes = (int)std::max<long long>(0, std::min<long long>(budget, (need + 3) / 4 * 4));
  a.center = v.center;
  a.curve = st->curve.as<lk_epipolar_curve>();
  a.other = st->other.as<int32_t>();
  a.node = st->node.as<int32_t>();
  a.inv_depth = st->inv_depth.as<double>();
  a.shape = st->shape.as<float4>();
  a.run = st->run.as<int2>();
  a.rec = st->rec.as<LkEpNodeRecord>();
  a.profile = st->profile.as<double>();
  a.match = st->match.as<lk_epipolar_match>();
  a.n_nodes = N;
  a.n_runs = n_runs;
  a.with_shape = cfg->shape;
  a.max_run = max_run;
  a.max_cand = max_cand;
  st->win_bytes = a.gs.win_bytes;

  if (guesses_inout)
    LK_HIPCHK(hipMemcpyAsync(v.d_guess, guesses_inout, 6 * sizeof(float) * (size_t)S, hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipEventRecord(st->ev[0], v.stream));
  LK_HIPCHK(lk_launch_epipolar_search(a, v.stream));
  LK_HIPCHK(hipEventRecord(st->ev[1], v.stream));
  LK_HIPCHK(lk_launch_epipolar_reduce(a, v.stream));
  LK_HIPCHK(hipEventRecord(st->ev[2], v.stream));
  st->S = S;
  if (guesses_inout) {
    LK_HIPCHK(hipMemcpyAsync(guesses_inout, v.d_guess, 6 * sizeof(float) * (size_t)S, hipMemcpyDeviceToHost, v.stream));
    LK_HIPCHK(hipStreamSynchronize(v.stream));
  }
  return LK_ERROR_NONE;
}

int lk_get_epipolar_search_info(lk_engine *e, lk_epipolar_match *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LkEpipolarState *st = nullptr;
  if (int rc = last_search(e, "lk_get_epipolar_search_info", &st))
    return rc;
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_get_epipolar_search_info: no output");
  hipStream_t stream = nullptr;
  if (int rc = lk_internal_engine_stream(e, &stream))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(out, st->match.p, sizeof(lk_epipolar_match) * (size_t)st->S, hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  return LK_ERROR_NONE;
}

int lk_get_epipolar_search_profile(lk_engine *e, lk_epipolar_curve *curves_out, double *profile_out, int *n_stations_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LkEpipolarState *st = nullptr;
  if (int rc = last_search(e, "lk_get_epipolar_search_profile", &st))
    return rc;
  const EpTable &t = st->table;
  if (curves_out)
    std::copy(t.curve.begin(), t.curve.end(), curves_out);
  if (n_stations_out)
    *n_stations_out = (int)t.other.size();
  if (!profile_out || t.other.empty())
    return LK_ERROR_NONE;
  hipStream_t stream = nullptr;
  if (int rc = lk_internal_engine_stream(e, &stream))
    return rc;
  LK_HIPCHK(hipMemcpyAsync(profile_out, st->profile.p, sizeof(double) * t.other.size(), hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  return LK_ERROR_NONE;
}

// Bench hook (scripts/epipolar_bench.py): the last lk_search_epipolar's two kernels by HIP events (waits for them), the
// host's time for the table, the candidates of all sectors, the LDS window bound and the longest run.  Any pointer may be null.
int lk_internal_epipolar_last(lk_engine *e, float *search_ms, float *reduce_ms, double *curves_ms, long long *candidates,
                              int *win_bytes, int *max_run) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LkEpipolarState *st = nullptr;
  if (int rc = last_search(e, "lk_internal_epipolar_last", &st))
    return rc;
  LK_HIPCHK(hipEventSynchronize(st->ev[2]));
  if (search_ms)
    LK_HIPCHK(hipEventElapsedTime(search_ms, st->ev[0], st->ev[1]));
  if (reduce_ms)
    LK_HIPCHK(hipEventElapsedTime(reduce_ms, st->ev[1], st->ev[2]));
  if (curves_ms)
    *curves_ms = st->curves_ms;
  if (candidates)
    *candidates = st->candidates;
  if (win_bytes)
    *win_bytes = st->win_bytes;
  if (max_run)
    *max_run = st->max_run;
  return LK_ERROR_NONE;
}

} // extern "C"
