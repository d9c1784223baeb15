// lk_stereo.cpp - host side of the two-camera rig (include/lk_engine.h: lk_stereo_points, lk_stereo_strain, lk_stereo_project,
// lk_stereo_triangulate, lk_stereo_fundamental, lk_stereo_surface_from_sums).  The kernels are lk_stereo.hip; the bounding box
// and the cell grid are the recovery pass's; the camera, the triangulation and the surface fit are lk_stereo.hpp's, here
// compiled for the host as well.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_pass.hpp"
#include "lk_stereo.hpp"

namespace {

// Lanes per (frame, sector): lk_strain.cpp's rule, a 16-lane row while the 3 x 3 cells around a sector hold at most this many
// members on average.  The walk is lk_strain_field's with a wider gather, and nothing measured says that the switch lies
// elsewhere (scripts/stereo_bench.py times both groups).
constexpr double kWideGroupFrom = 1024.0;
constexpr int kMaxFrames = 65534; // (a frame per blockIdx.y, the reference state included)
constexpr double kRotationTol = 1e-9;

struct StereoState : LkPassState {
  LkDevBytes ref1, rec0, rec1, held, ref_up, pts_up, out, bbox;
  LkCellGridBufs grid;
  int held_frames = -1, held_sectors = 0; // what `held` holds: [1 + held_frames][held_sectors] points; -1: nothing yet
  int group = 0, strain_frames = 0;       // of the last lk_stereo_strain (0: the last call was lk_stereo_points)
  double members = 0;
};

// null: the camera is usable; else what is wrong with it
const char *camera_refusal(const lk_camera *c) {
  if (!c)
    return "no camera";
  for (int i = 0; i < 7; ++i)
    if (c->reserved[i] != 0.0)
      return "a camera's reserved words must be 0";
  if (!std::isfinite(c->fx) || !std::isfinite(c->fy) || !std::isfinite(c->cx) || !std::isfinite(c->cy) || !std::isfinite(c->skew))
    return "a camera's intrinsics must be finite";
  if (!(c->fx > 0.0) || !(c->fy > 0.0))
    return "fx and fy must be > 0";
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(c->R[i]))
      return "R must be finite";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(c->t[i]))
      return "t must be finite";
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double dot = c->R[i] * c->R[j] + c->R[3 + i] * c->R[3 + j] + c->R[6 + i] * c->R[6 + j];
      if (!(std::fabs(dot - (i == j ? 1.0 : 0.0)) <= kRotationTol))
        return "R^T R must be the identity within 1e-9";
    }
  const lk_lens &L = c->lens;
  if (L.reserved != 0.0)
    return "the lens's reserved word must be 0";
  if (!std::isfinite(L.k1) || !std::isfinite(L.k2) || !std::isfinite(L.p1) || !std::isfinite(L.p2))
    return "the lens must be finite";
  if (lk_camera_has_lens(*c)) {
    if (!std::isfinite(L.rn) || !(L.rn > 0.0))
      return "the lens's rn must be finite and > 0";
    if (!std::isfinite(L.cx) || !std::isfinite(L.cy))
      return "the lens must be finite";
  }
  return nullptr;
}

// K^-1 of a camera, row-major
void inverse_intrinsics(const lk_camera &c, double *Ki) {
  const double m[9] = {1.0 / c.fx, (0.0 - c.skew) / (c.fx * c.fy), (c.skew * c.cy - c.cx * c.fy) / (c.fx * c.fy),
                       0.0, 1.0 / c.fy, (0.0 - c.cy) / c.fy,
                       0.0, 0.0, 1.0};
  std::memcpy(Ki, m, sizeof m);
}
void mul3(const double *A, const double *B, double *C) { // C = A B
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
void transpose3(const double *A, double *T) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      T[3 * i + j] = A[3 * j + i];
}

// F = K1^-T [t_r]x R_r K0^-1 with R_r = R1 R0^T, t_r = t1 - R_r t0
void fundamental(const lk_camera *cams, double *F) {
  double R0t[9], Rr[9], K0i[9], K1i[9], K1it[9], E[9], EK[9];
  transpose3(cams[0].R, R0t);
  mul3(cams[1].R, R0t, Rr);
  double tr[3];
  for (int i = 0; i < 3; ++i)
    tr[i] = cams[1].t[i] - ((Rr[3 * i] * cams[0].t[0] + Rr[3 * i + 1] * cams[0].t[1]) + Rr[3 * i + 2] * cams[0].t[2]);
  const double Tx[9] = {0.0, 0.0 - tr[2], tr[1], tr[2], 0.0, 0.0 - tr[0], 0.0 - tr[1], tr[0], 0.0};
  mul3(Tx, Rr, E);
  inverse_intrinsics(cams[0], K0i);
  inverse_intrinsics(cams[1], K1i);
  transpose3(K1i, K1it);
  mul3(E, K0i, EK);
  mul3(K1it, EK, F);
}

int rig_of(lk_engine *e, const char *who, const lk_camera *cams, LkStereoRig *rig) {
  if (!cams)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": no cameras").c_str());
  for (int k = 0; k < 2; ++k)
    if (const char *why = camera_refusal(cams + k))
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": camera " + (k ? "1: " : "0: ") + why).c_str());
  rig->cam[0] = cams[0], rig->cam[1] = cams[1];
  fundamental(cams, rig->F);
  return LK_ERROR_NONE;
}

} // namespace

extern "C" {

int lk_stereo_project(const lk_camera *cam, int n, const double *xyz, double *xy_out, uint8_t *status_out) {
  if (camera_refusal(cam) || !xyz || !xy_out || n < 1)
    return LK_ERROR_BAD_DOMAIN;
  for (int i = 0; i < n; ++i) {
    double x, y;
    const int behind = lk_stereo_project_impl(*cam, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], x, y);
    xy_out[2 * i] = x, xy_out[2 * i + 1] = y;
    if (status_out)
      status_out[i] = (uint8_t)behind;
  }
  return LK_ERROR_NONE;
}

int lk_stereo_fundamental(const lk_camera *cams, double *F_out) {
  if (!cams || !F_out || camera_refusal(cams) || camera_refusal(cams + 1))
    return LK_ERROR_BAD_DOMAIN;
  fundamental(cams, F_out);
  return LK_ERROR_NONE;
}

int lk_stereo_triangulate(const lk_camera *cams, int n, const double *x0, const double *x1, lk_stereo_point *out) {
  if (!cams || camera_refusal(cams) || camera_refusal(cams + 1) || !x0 || !x1 || !out || n < 1)
    return LK_ERROR_BAD_DOMAIN;
  LkStereoRig rig;
  rig.cam[0] = cams[0], rig.cam[1] = cams[1];
  fundamental(cams, rig.F);
  for (int i = 0; i < n; ++i)
    out[i] = lk_stereo_triangulate_impl(rig, 1, x0[2 * i], x0[2 * i + 1], x1[2 * i], x1[2 * i + 1]);
  return LK_ERROR_NONE;
}

int lk_stereo_surface_from_sums(int n, const double *sums23, int min_neighbours, int self_good, double residual_sum,
                                lk_stereo_surface *out, double *planes_out) {
  if (!sums23 || !out || n < 0 || min_neighbours < 3)
    return LK_ERROR_BAD_DOMAIN;
  const LkStereoPlanes p = lk_stereo_planes(n, sums23, min_neighbours, self_good ? 1 : 0);
  *out = lk_stereo_surface_impl(n, p, residual_sum);
  if (planes_out)
    for (int k = 0; k < 6; ++k)
      planes_out[3 * k] = p.f0[k], planes_out[3 * k + 1] = p.fx[k], planes_out[3 * k + 2] = p.fy[k];
  return LK_ERROR_NONE;
}

int lk_stereo_points(lk_engine *e, const lk_stereo_config *cfg, const lk_camera *cams, const lk_result *ref1, int n_frames,
                     const lk_result *rec0, const lk_result *rec1, lk_stereo_point *ref_out, lk_stereo_point *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: no configuration");
  if (!ref1)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: no ref1 records");
  if (!ref_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: no output for the reference points");
  if (n_frames < 0 || n_frames > kMaxFrames)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: n_frames must be 0 .. 65534");
  if (n_frames > 0 && (!rec0 || !rec1 || !out))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: rec0, rec1 and the output are needed with n_frames > 0");
  if (n_frames == 0 && (rec0 || rec1 || out))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: rec0, rec1 and the output must be NULL with n_frames = 0");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->reserved != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_points: the reserved word must be 0");
  LkStereoPointsArgs a{};
  if (int rc = rig_of(e, "lk_stereo_points", cams, &a.rig))
    return rc;
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_stereo_points", 0, -1, &v))
    return rc;
  StereoState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_STEREO, "hipHostMalloc / hipEventCreate (lk_stereo_points)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames;
  st->held_frames = -1; // (until this call has finished)
  LK_HIPCHK(st->held.ensure((F + 1) * S * sizeof(lk_stereo_point)));
  const lk_result *d_ref1 = nullptr, *d_rec0 = nullptr, *d_rec1 = nullptr;
  if (int rc = lk_pass_records(e, st->ref1, ref1, S, v.stream, &d_ref1))
    return rc;
  if (int rc = lk_pass_records(e, st->rec0, rec0, F * S, v.stream, &d_rec0))
    return rc;
  if (int rc = lk_pass_records(e, st->rec1, rec1, F * S, v.stream, &d_rec1))
    return rc;
  a.center = v.center;
  a.ref1 = d_ref1, a.rec0 = d_rec0, a.rec1 = d_rec1;
  a.out = st->held.as<lk_stereo_point>();
  a.n_frames = n_frames, a.n_sectors = v.S, a.model = v.model;
  a.chi_max = cfg->chi_max;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_launch_stereo_points(a, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(ref_out, st->held.p, S * sizeof(lk_stereo_point), hipMemcpyDeviceToHost, v.stream));
  if (n_frames > 0)
    LK_HIPCHK(hipMemcpyAsync(out, st->held.as<lk_stereo_point>() + S, F * S * sizeof(lk_stereo_point), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->held_frames = n_frames, st->held_sectors = v.S;
  st->group = 0, st->strain_frames = 0, st->members = 0;
  st->finished();
  return LK_ERROR_NONE;
}

int lk_stereo_strain(lk_engine *e, const lk_stereo_config *cfg, int n_frames, const lk_stereo_point *ref_points,
                     const lk_stereo_point *points, lk_stereo_surface *out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: no output");
  if (!std::isfinite(cfg->radius) || !(cfg->radius > 0.f))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: radius must be finite and positive");
  if (cfg->min_neighbours < 3)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: min_neighbours must be at least 3 (a plane has three unknowns)");
  if (cfg->reserved != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: the reserved word must be 0");
  if (n_frames < 1 || n_frames > kMaxFrames)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: n_frames must be 1 .. 65534");
  if ((ref_points == nullptr) != (points == nullptr))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: ref_points and points must both be given or both be NULL");
  LkPassView v{};
  if (int rc = lk_internal_pass_view(e, "lk_stereo_strain", 0, -1, &v))
    return rc;
  StereoState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_STEREO, "hipHostMalloc / hipEventCreate (lk_stereo_strain)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames;
  LkStereoStrainArgs a{};
  if (!points) {
    if (st->held_frames < 0)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: no points on the device: no lk_stereo_points yet");
    if (st->held_sectors != v.S)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: the points on the device are of another sector count");
    if (st->held_frames != n_frames)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_stereo_strain: n_frames differs from the lk_stereo_points call whose points are on the device");
    a.ref = st->held.as<lk_stereo_point>();
    a.pts = a.ref + S;
  } else {
    LK_HIPCHK(st->ref_up.ensure(S * sizeof(lk_stereo_point)));
    LK_HIPCHK(st->pts_up.ensure(F * S * sizeof(lk_stereo_point)));
    LK_HIPCHK(hipMemcpyAsync(st->ref_up.p, ref_points, S * sizeof(lk_stereo_point), hipMemcpyHostToDevice, v.stream));
    LK_HIPCHK(hipMemcpyAsync(st->pts_up.p, points, F * S * sizeof(lk_stereo_point), hipMemcpyHostToDevice, v.stream));
    a.ref = st->ref_up.as<lk_stereo_point>();
    a.pts = st->pts_up.as<lk_stereo_point>();
  }
  LK_HIPCHK(st->out.ensure(F * S * sizeof(lk_stereo_surface)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  LK_HIPCHK(st->begin(v.stream));
  if (int rc = lk_pass_grid(e, "lk_stereo_strain", st, st->bbox, st->grid, v.center, v.S, cfg->radius, v.stream, &a.grid))
    return rc;
  a.center = v.center;
  a.out = st->out.as<lk_stereo_surface>();
  a.n_frames = n_frames, a.n_sectors = v.S, a.min_neighbours = cfg->min_neighbours;
  a.radius = (double)cfg->radius;
  st->members = 9.0 * (double)v.S / ((double)a.grid.nx * (double)a.grid.ny);
  // test hook and tuning experiments (scripts/stereo_bench.py): LK_STEREO_GROUP = 16 / 64 overrides the choice
  st->group = lk_pass_env_choice("LK_STEREO_GROUP", 16, 64, st->members > kWideGroupFrom ? 64 : 16);
  st->strain_frames = n_frames;
  LK_HIPCHK(lk_launch_stereo_strain(a, st->group, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(out, st->out.p, F * S * sizeof(lk_stereo_surface), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_stereo_last(lk_engine *e, float *device_ms, int *group, double *members, int *held_frames) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  StereoState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_STEREO, "lk_internal_stereo_last: no lk_stereo_points or lk_stereo_strain yet", device_ms, &st))
    return rc;
  if (group)
    *group = st->group;
  if (members)
    *members = st->members;
  if (held_frames)
    *held_frames = st->held_frames;
  return LK_ERROR_NONE;
}

} // extern "C"
