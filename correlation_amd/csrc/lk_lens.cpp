// lk_lens.cpp - host side of the lens distortion (include/lk_engine.h: lk_lens_fit, lk_lens_correct, lk_lens_distort,
// lk_lens_undistort, lk_lens_correct_record, lk_lens_step_from_sums).  The kernels are lk_lens.hip; the bounding box is the
// recovery pass's (lk_reseed.hip); the model, the correction and the rows are lk_lens.hpp's, here compiled for the host as well.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_lens.hpp"
#include "lk_pass.hpp"

namespace {

// Sectors per chunk, one workgroup each: eight per lane.  LK_LENS_CHUNK = 64 (tests: a small domain then spans several
// chunks) / 2048 overrides it.
constexpr int kChunk = 2048, kChunkSmall = 64;
constexpr unsigned kAllFree = LK_LENS_FREE_K1 | LK_LENS_FREE_K2 | LK_LENS_FREE_P1 | LK_LENS_FREE_P2 | LK_LENS_FREE_CENTRE;
constexpr double kPivot = 1e-10;

struct LensState : LkPassState {
  LkDevBytes rec, pack, mask, nuisance, partial, sums, rec_out, centres, status, bbox;
  hipEvent_t ev2 = nullptr, ev3 = nullptr; // around the last evaluation of a fit
  int chunk = 0, chunks = 0, evaluations = 0;
  hipError_t init() {
    hipError_t err = LkPassState::init();
    if (err == hipSuccess)
      err = hipEventCreate(&ev2);
    if (err == hipSuccess)
      err = hipEventCreate(&ev3);
    return err;
  }
  ~LensState() override {
    if (ev2)
      (void)hipEventDestroy(ev2);
    if (ev3)
      (void)hipEventDestroy(ev3);
  }
};

bool known_nuisance(int k) { return k >= LK_LENS_TRANSLATION && k <= LK_LENS_AFFINE; }

// null: the lens is usable; else what is wrong with it
const char *lens_refusal(const lk_lens *L) {
  if (!L)
    return "no lens";
  if (!std::isfinite(L->rn) || !(L->rn > 0.0))
    return "rn must be finite and > 0";
  if (!std::isfinite(L->cx) || !std::isfinite(L->cy) || !std::isfinite(L->k1) || !std::isfinite(L->k2) || !std::isfinite(L->p1) ||
      !std::isfinite(L->p2))
    return "the lens must be finite";
  if (L->reserved != 0.0)
    return "the lens's reserved word must be 0";
  return nullptr;
}

// lk_track_points' rules for the three record sources; *n_frames becomes the window's count where it was 0
int check_source(lk_engine *e, const std::string &who, int source, const lk_result *records, int *n_frames, LkPassView *v) {
  if (source != LK_TRACK_RECORDS_CALLER && source != LK_TRACK_RECORDS_ENGINE && source != LK_TRACK_RECORDS_WINDOW)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": unknown source").c_str());
  if (source == LK_TRACK_RECORDS_CALLER) {
    if (!records)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": source CALLER needs records").c_str());
    if (*n_frames < 1)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": n_frames must be at least 1").c_str());
  } else if (records) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": records must be NULL unless the source is CALLER").c_str());
  } else if (source == LK_TRACK_RECORDS_ENGINE && *n_frames != 1) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": n_frames must be 1 for the engine-held records of a batch solve").c_str());
  } else if (source == LK_TRACK_RECORDS_WINDOW && *n_frames < 0) {
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": n_frames must be 0 or the window's frame count").c_str());
  }
  const unsigned need = source == LK_TRACK_RECORDS_ENGINE ? LK_VIEW_RECORDS : source == LK_TRACK_RECORDS_WINDOW ? LK_VIEW_WINDOW : 0u;
  if (int rc = lk_internal_pass_view(e, who.c_str(), need, -1, v))
    return rc;
  if (source == LK_TRACK_RECORDS_WINDOW) {
    if (*n_frames != 0 && *n_frames != v->window_frames)
      return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": n_frames must be 0 or the window's frame count").c_str());
    *n_frames = v->window_frames;
  }
  if (*n_frames > 65535)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (who + ": n_frames must be at most 65535 per call").c_str());
  return LK_ERROR_NONE;
}

// Cholesky of the Jacobi-scaled n x n matrix m (row-major, n <= 6): scale[i] = sqrt(m_ii), l = the lower factor of
// m_ij / (scale_i scale_j).  False for a diagonal <= 0 or a pivot <= kPivot.
bool scaled_cholesky(int n, const double *m, double *scale, double *l) {
  for (int i = 0; i < n; ++i) {
    if (!(m[i * n + i] > 0.0) || !std::isfinite(m[i * n + i]))
      return false;
    scale[i] = std::sqrt(m[i * n + i]);
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double t = m[i * n + j] / (scale[i] * scale[j]);
      for (int k = 0; k < j; ++k)
        t -= l[i * n + k] * l[j * n + k];
      if (i == j) {
        if (!(t > kPivot))
          return false;
        l[i * n + i] = std::sqrt(t);
      } else {
        l[i * n + j] = t / l[j * n + j];
      }
    }
  return true;
}
// x = m^-1 b with the factor above
void scaled_solve(int n, const double *scale, const double *l, const double *b, double *x) {
  double y[6];
  for (int i = 0; i < n; ++i) {
    double t = b[i] / scale[i];
    for (int k = 0; k < i; ++k)
      t -= l[i * n + k] * y[k];
    y[i] = t / l[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = y[i];
    for (int k = i + 1; k < n; ++k)
      t -= l[k * n + i] * x[k];
    x[i] = t / l[i * n + i];
  }
  for (int i = 0; i < n; ++i)
    x[i] = x[i] / scale[i];
}

int step_from_sums(int nuisance, unsigned free_mask, double rn, int min_sectors, int n_frames, const double *sums, lk_lens_step *out,
                   double *nuisance_delta) {
  const int Q = lk_lens_q(nuisance), W = lk_lens_width(Q), LEN = lk_lens_sums_len(Q);
  std::memset(out, 0, sizeof *out);
  if (nuisance_delta)
    std::memset(nuisance_delta, 0, (size_t)n_frames * 6 * sizeof(double));
  int idx[6], nf = 0;
  for (int j = 0; j < 6; ++j)
    if (free_mask & (j < 4 ? 1u << j : (unsigned)LK_LENS_FREE_CENTRE))
      idx[nf++] = j;
  auto at = [&](const double *s, int i, int j) { // entry (i, j) of a frame's symmetric W x W matrix
    if (i > j)
      std::swap(i, j);
    return s[1 + i * W - i * (i - 1) / 2 + (j - i)];
  };
  double S[36] = {0}, b[6] = {0};
  // of every used frame: Hnn^-1 [Hnl | gn], Q x (nf + 1)
  std::vector<double> Z((size_t)n_frames * 6 * 7, 0.0);
  std::vector<char> used((size_t)n_frames, 0);
  bool degenerate = false;
  for (int f = 0; f < n_frames; ++f) {
    const double *s = sums + (size_t)f * LEN;
    out->n_outside += (int)s[LEN - 1];
    const int n = (int)s[0];
    if (n < min_sectors)
      continue;
    used[f] = 1;
    out->n_records += n;
    out->n_frames_used += 1;
    const double rr = at(s, W - 1, W - 1);
    out->chi2 += rr;
    double Hnn[36], scale[6], l[36] = {0};
    for (int p = 0; p < Q; ++p)
      for (int q = 0; q < Q; ++q)
        Hnn[p * Q + q] = at(s, 6 + p, 6 + q);
    if (!scaled_cholesky(Q, Hnn, scale, l)) {
      degenerate = true;
      continue;
    }
    double *z = &Z[(size_t)f * 42];
    for (int c = 0; c <= nf; ++c) {
      double rhs[6], x[6];
      for (int q = 0; q < Q; ++q)
        rhs[q] = at(s, 6 + q, c < nf ? idx[c] : W - 1);
      scaled_solve(Q, scale, l, rhs, x);
      for (int q = 0; q < Q; ++q)
        z[q * 7 + c] = x[q];
    }
    double profiled = rr;
    for (int q = 0; q < Q; ++q)
      profiled -= at(s, 6 + q, W - 1) * z[q * 7 + nf];
    out->chi2_profiled += profiled;
    for (int i = 0; i < nf; ++i) {
      for (int j = 0; j < nf; ++j) {
        double t = at(s, idx[i], idx[j]);
        for (int q = 0; q < Q; ++q)
          t -= at(s, idx[i], 6 + q) * z[q * 7 + j];
        S[i * nf + j] += t;
      }
      double t = at(s, idx[i], W - 1);
      for (int q = 0; q < Q; ++q)
        t -= at(s, idx[i], 6 + q) * z[q * 7 + nf];
      b[i] += t;
    }
  }
  double scale[6], l[36] = {0};
  if (degenerate || out->n_frames_used == 0 || !scaled_cholesky(nf, S, scale, l)) {
    out->status = LK_LENS_DEGENERATE;
    return LK_ERROR_NONE;
  }
  double minus_b[6], d[6];
  for (int i = 0; i < nf; ++i)
    minus_b[i] = 0.0 - b[i];
  scaled_solve(nf, scale, l, minus_b, d);
  const double dof = 2.0 * out->n_records - nf - (double)Q * out->n_frames_used;
  for (int i = 0; i < nf; ++i) {
    out->delta[idx[i]] = d[i];
    const double step = std::fabs(d[i]) / (idx[i] < 4 ? 1.0 : rn);
    out->scaled_step = step > out->scaled_step ? step : out->scaled_step;
    double unit[6] = {0}, col[6];
    unit[i] = 1.0;
    scaled_solve(nf, scale, l, unit, col);
    out->sigma[idx[i]] = dof > 0.0 && col[i] > 0.0 ? std::sqrt(out->chi2 / dof * col[i]) : 0.0;
  }
  if (nuisance_delta)
    for (int f = 0; f < n_frames; ++f) {
      if (!used[f])
        continue;
      const double *z = &Z[(size_t)f * 42];
      for (int q = 0; q < Q; ++q) {
        double t = z[q * 7 + nf];
        for (int i = 0; i < nf; ++i)
          t += z[q * 7 + i] * d[i];
        nuisance_delta[(size_t)f * 6 + q] = 0.0 - t;
      }
    }
  out->status = LK_LENS_OK;
  return LK_ERROR_NONE;
}

bool zero_lens(const lk_lens &L) { return L.k1 == 0.0 && L.k2 == 0.0 && L.p1 == 0.0 && L.p2 == 0.0; }

} // namespace

extern "C" {

int lk_lens_distort(const lk_lens *lens, int n, const double *xy, double *xy_out) {
  if (lens_refusal(lens) || !xy || !xy_out || n < 1)
    return LK_ERROR_BAD_DOMAIN;
  for (int i = 0; i < n; ++i) {
    double x, y;
    lk_lens_distort_point(*lens, xy[2 * i], xy[2 * i + 1], x, y);
    xy_out[2 * i] = x, xy_out[2 * i + 1] = y;
  }
  return LK_ERROR_NONE;
}

int lk_lens_undistort(const lk_lens *lens, int n, const double *xy, double *xy_out, uint8_t *status_out) {
  if (lens_refusal(lens) || !xy || !xy_out || n < 1)
    return LK_ERROR_BAD_DOMAIN;
  for (int i = 0; i < n; ++i) {
    LkLensJac J;
    double x, y;
    const bool outside = lk_lens_undistort_point(*lens, xy[2 * i], xy[2 * i + 1], x, y, J) != 0;
    xy_out[2 * i] = outside ? xy[2 * i] : x, xy_out[2 * i + 1] = outside ? xy[2 * i + 1] : y;
    if (status_out)
      status_out[i] = outside ? 2 : 0;
  }
  return LK_ERROR_NONE;
}

int lk_lens_correct_record(int model, const lk_lens *lens, float cx, float cy, const lk_result *in, lk_result *out, int *status) {
  if (lens_refusal(lens) || !in || !out || model < LK_FM_U || model > LK_FM_UVUXUYVXVY)
    return LK_ERROR_BAD_DOMAIN;
  lk_result r = *in;
  float *p = r.resultingParameters;
  const int st = lk_lens_correct_params(model, *lens, cx, cy, p[0], p[1], p[2], p[3], p[4], p[5]);
  *out = r;
  if (status)
    *status = st;
  return LK_ERROR_NONE;
}

int lk_lens_step_from_sums(int nuisance, unsigned free_mask, double rn, int min_sectors, int n_frames, const double *sums,
                           lk_lens_step *out, double *nuisance_delta) {
  if (!sums || !out || !known_nuisance(nuisance) || free_mask == 0 || (free_mask & ~kAllFree) || !std::isfinite(rn) || !(rn > 0.0) ||
      n_frames < 1 || min_sectors < lk_lens_q(nuisance))
    return LK_ERROR_BAD_DOMAIN;
  return step_from_sums(nuisance, free_mask, rn, min_sectors, n_frames, sums, out, nuisance_delta);
}

int lk_lens_correct(lk_engine *e, const lk_lens_config *cfg, const lk_lens *lens, int n_frames, const lk_result *records,
                    lk_result *records_out, float *centres_out, uint8_t *status_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_correct: no configuration");
  if (!records_out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_correct: no output");
  if (const char *why = lens_refusal(lens))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string("lk_lens_correct: ") + why).c_str());
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_correct: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_correct: reserved words must be 0");
  LkPassView v{};
  if (int rc = check_source(e, "lk_lens_correct", cfg->source, records, &n_frames, &v))
    return rc;
  LensState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_LENS, "hipHostMalloc / hipEventCreate (lk_lens_correct)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames;
  LK_HIPCHK(st->pack.ensure(F * S * sizeof(float4)));
  LK_HIPCHK(st->rec_out.ensure(F * S * sizeof(lk_result)));
  LK_HIPCHK(st->centres.ensure(S * sizeof(float2)));
  LK_HIPCHK(st->status.ensure(F * S));
  const lk_result *d_rec = cfg->source == LK_TRACK_RECORDS_WINDOW ? v.window : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, F * S, v.stream, &d_rec))
    return rc;
  LkLensCorrectArgs a{};
  a.pack = st->pack.as<float4>();
  a.rec = d_rec;
  a.center = v.center;
  a.rec_out = st->rec_out.as<lk_result>();
  a.centres_out = centres_out ? st->centres.as<float2>() : nullptr;
  a.status = status_out ? st->status.as<uint8_t>() : nullptr;
  a.lens = *lens;
  a.n_frames = n_frames;
  a.n_sectors = v.S;
  a.model = v.model;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, n_frames, v.model, cfg->chi_max, 0, nullptr, st->pack.as<float4>(), v.stream));
  LK_HIPCHK(lk_launch_lens_correct(a, v.stream));
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipMemcpyAsync(records_out, st->rec_out.p, F * S * sizeof(lk_result), hipMemcpyDeviceToHost, v.stream));
  if (centres_out)
    LK_HIPCHK(hipMemcpyAsync(centres_out, st->centres.p, S * sizeof(float2), hipMemcpyDeviceToHost, v.stream));
  if (status_out)
    LK_HIPCHK(hipMemcpyAsync(status_out, st->status.p, F * S, hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->chunk = st->chunks = st->evaluations = 0;
  st->finished();
  return LK_ERROR_NONE;
}

int lk_lens_fit(lk_engine *e, const lk_lens_fit_config *cfg, const lk_lens *init, int n_frames, const lk_result *records,
                const uint8_t *fit_mask, lk_lens_result *out, lk_lens_frame *frames_out, double *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: no configuration");
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: no output");
  if (const char *why = lens_refusal(init))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string("lk_lens_fit: ") + why).c_str());
  if (!known_nuisance(cfg->nuisance))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: unknown nuisance");
  if (cfg->free == 0 || (cfg->free & ~kAllFree))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: free must name at least one of k1, k2, p1, p2 and the centre, and nothing else");
  if ((cfg->free & LK_LENS_FREE_CENTRE) && cfg->nuisance == LK_LENS_AFFINE)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN,
                            "lk_lens_fit: the centre cannot be free with LK_LENS_AFFINE (a shift of the centre is an affine field to first order)");
  if (!std::isfinite(cfg->chi_max))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: chi_max must be finite (<= 0: the error code alone decides)");
  if (cfg->max_iters < 1 || cfg->max_iters > 32)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: max_iters must be 1 .. 32");
  if (!std::isfinite(cfg->tol) || cfg->tol < 0.0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: tol must be finite and >= 0");
  const int Q = lk_lens_q(cfg->nuisance), LEN = lk_lens_sums_len(Q);
  if (cfg->min_sectors < Q)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: min_sectors is below the nuisance's unknowns (2, 4, 6)");
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: reserved words must be 0");
  LkPassView v{};
  if (int rc = check_source(e, "lk_lens_fit", cfg->source, records, &n_frames, &v))
    return rc;
  if (v.model == LK_FM_U)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: LK_FM_U has no v: a lens cannot be fitted to it");
  LensState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_LENS, "hipHostMalloc / hipEventCreate (lk_lens_fit)", &st))
    return rc;
  const size_t S = (size_t)v.S, F = (size_t)n_frames;
  st->chunk = lk_pass_env_choice("LK_LENS_CHUNK", kChunkSmall, kChunk, kChunk);
  st->chunks = (v.S + st->chunk - 1) / st->chunk;
  LK_HIPCHK(st->pack.ensure(F * S * sizeof(float4)));
  LK_HIPCHK(st->nuisance.ensure(F * 6 * sizeof(double)));
  LK_HIPCHK(st->partial.ensure(F * (size_t)st->chunks * LEN * sizeof(double)));
  LK_HIPCHK(st->sums.ensure(F * LEN * sizeof(double)));
  LK_HIPCHK(st->bbox.ensure(4 * sizeof(float)));
  const lk_result *d_rec = cfg->source == LK_TRACK_RECORDS_WINDOW ? v.window : v.result;
  if (int rc = lk_pass_records(e, st->rec, records, F * S, v.stream, &d_rec))
    return rc;
  if (fit_mask) {
    LK_HIPCHK(st->mask.ensure(S));
    LK_HIPCHK(hipMemcpyAsync(st->mask.p, fit_mask, S, hipMemcpyHostToDevice, v.stream)); // (pageable: staged before it returns)
  }
  // o of the nuisance: the centre of the centres' bounding box (the call's one round trip before its kernels)
  LK_HIPCHK(lk_launch_reseed_bbox(v.center, v.S, st->bbox.as<float>(), v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->h_bbox, st->bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_lens_fit: a sector centre is not finite");
  LkLensFitArgs a{};
  a.pack = st->pack.as<float4>();
  a.fit_mask = fit_mask ? st->mask.as<uint8_t>() : nullptr;
  a.nuisance = st->nuisance.as<double>();
  a.partial = st->partial.as<double>();
  a.sums = st->sums.as<double>();
  a.lens = *init;
  a.n_frames = n_frames;
  a.n_sectors = v.S;
  a.chunk = st->chunk;
  a.chunks = st->chunks;
  a.nuisance_kind = cfg->nuisance;
  a.ox = ((double)st->h_bbox[0] + (double)st->h_bbox[2]) / 2.0;
  a.oy = ((double)st->h_bbox[1] + (double)st->h_bbox[3]) / 2.0;

  std::vector<double> nu(F * 6, 0.0), dnu(F * 6, 0.0), sums(F * LEN, 0.0), first_sums;
  lk_lens_result fit;
  std::memset(&fit, 0, sizeof fit);
  fit.lens = *init;
  fit.status = LK_LENS_MAX_ITERS;
  lk_lens_step step;
  // one evaluation at the running lens and nuisance: upload, two kernels, download
  auto evaluate = [&](bool last) -> int {
    a.lens = fit.lens;
    LK_HIPCHK(hipMemcpyAsync(st->nuisance.p, nu.data(), F * 6 * sizeof(double), hipMemcpyHostToDevice, v.stream));
    if (last)
      LK_HIPCHK(hipEventRecord(st->ev2, v.stream));
    LK_HIPCHK(lk_launch_lens_sums(a, v.stream));
    if (last)
      LK_HIPCHK(hipEventRecord(st->ev3, v.stream));
    LK_HIPCHK(hipMemcpyAsync(sums.data(), st->sums.p, F * LEN * sizeof(double), hipMemcpyDeviceToHost, v.stream));
    LK_HIPCHK(hipStreamSynchronize(v.stream));
    st->evaluations += 1;
    return LK_ERROR_NONE;
  };
  // the centre has no effect on a lens without coefficients: it is held for such an iteration
  auto free_now = [&]() { return zero_lens(fit.lens) ? cfg->free & ~(unsigned)LK_LENS_FREE_CENTRE : cfg->free; };
  st->evaluations = 0;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_launch_pack_prep(d_rec, v.center, v.S, n_frames, v.model, cfg->chi_max, 0, nullptr, st->pack.as<float4>(), v.stream));
  for (int it = 0; it < cfg->max_iters; ++it) {
    if (int rc = evaluate(false))
      return rc;
    if (it == 0)
      first_sums = sums;
    const unsigned free_mask = free_now();
    if (free_mask == 0) {
      fit.status = LK_LENS_DEGENERATE;
      break;
    }
    (void)step_from_sums(cfg->nuisance, free_mask, fit.lens.rn, cfg->min_sectors, n_frames, sums.data(), &step, dnu.data());
    if (it == 0)
      fit.rms_before = step.n_records > 0 && step.chi2_profiled > 0.0 ? std::sqrt(step.chi2_profiled / step.n_records) : 0.0;
    if (step.status != LK_LENS_OK) {
      fit.status = step.status;
      break;
    }
    fit.lens.k1 += step.delta[0], fit.lens.k2 += step.delta[1], fit.lens.p1 += step.delta[2], fit.lens.p2 += step.delta[3];
    fit.lens.cx += step.delta[4], fit.lens.cy += step.delta[5];
    for (size_t i = 0; i < F * 6; ++i)
      nu[i] += dnu[i];
    fit.iterations = it + 1;
    fit.last_step = step.scaled_step;
    if (step.scaled_step <= cfg->tol) {
      fit.status = LK_LENS_OK;
      break;
    }
  }
  if (int rc = evaluate(true))
    return rc;
  LK_HIPCHK(st->end(v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  const unsigned free_mask = free_now();
  std::memset(&step, 0, sizeof step);
  if (free_mask != 0)
    (void)step_from_sums(cfg->nuisance, free_mask, fit.lens.rn, cfg->min_sectors, n_frames, sums.data(), &step, nullptr);
  else
    (void)step_from_sums(cfg->nuisance, cfg->free, fit.lens.rn, cfg->min_sectors, n_frames, sums.data(), &step, nullptr);
  for (int j = 0; j < 6; ++j)
    fit.sigma[j] = step.status == LK_LENS_OK ? step.sigma[j] : 0.0;
  fit.rms = step.n_records > 0 ? std::sqrt(step.chi2 / step.n_records) : 0.0;
  fit.n_records = step.n_records, fit.n_frames_used = step.n_frames_used, fit.n_outside = step.n_outside;
  *out = fit;
  if (frames_out)
    for (size_t f = 0; f < F; ++f) {
      const double *s = &sums[f * LEN];
      lk_lens_frame fr;
      std::memset(&fr, 0, sizeof fr);
      fr.n = (int)s[0];
      fr.status = fr.n < cfg->min_sectors ? LK_LENS_FRAME_TOO_FEW : LK_LENS_FRAME_OK;
      if (fr.status == LK_LENS_FRAME_OK) {
        for (int q = 0; q < Q; ++q)
          fr.nuisance[q] = nu[f * 6 + q];
        fr.rms = std::sqrt(s[LEN - 2] / (double)fr.n); // (the triangle's last entry: sum |r|^2)
      }
      frames_out[f] = fr;
    }
  if (sums_out) {
    std::memcpy(sums_out, first_sums.data(), F * LEN * sizeof(double));
    std::memcpy(sums_out + F * LEN, sums.data(), F * LEN * sizeof(double));
  }
  st->finished();
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_lens_last(lk_engine *e, float *device_ms, int *chunk, int *chunks, int *evaluations, float *eval_ms) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  LensState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_LENS, "lk_internal_lens_last: no lk_lens_fit or lk_lens_correct yet", device_ms, &st))
    return rc;
  if (chunk)
    *chunk = st->chunk;
  if (chunks)
    *chunks = st->chunks;
  if (evaluations)
    *evaluations = st->evaluations;
  if (eval_ms) {
    *eval_ms = 0.f;
    if (st->evaluations > 0)
      LK_HIPCHK(hipEventElapsedTime(eval_ms, st->ev2, st->ev3));
  }
  return LK_ERROR_NONE;
}

} // extern "C"
