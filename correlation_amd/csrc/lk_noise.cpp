// lk_noise.cpp - host side of the camera-noise pass (include/lk_engine.h: lk_camera_noise, lk_sector_noise,
// lk_noise_from_bins, lk_noise_from_sums).  The kernels are lk_noise.hip and give integers only; every floating-point number
// of a record comes from the two host functions below.  The frames come through lk_internal_frames_view.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_launch.hpp"
#include "lk_noise.hpp"
#include "lk_pass.hpp"

namespace {

struct NoiseState : LkPassState {
  LkDevBytes mask, tables, order, sums; // tables: bins [256][2], then frame_sums [LK_NOISE_MAX_FRAMES]
  std::vector<uint32_t> h_order;
  int workgroups = 0;
  hipError_t init() { return LkPassState::init(false); } // no bounding box
};

const char *const kWhere = "hipEventCreate (lk_camera_noise, lk_sector_noise)";
constexpr size_t kTableWords = 2 * kLkNoiseBins + LK_NOISE_MAX_FRAMES;

typedef __int128 i128; // the integer combinations of the record are formed exactly; each is converted and divided once

// the checks the two engine calls share; who: the function's name
int check_config(lk_engine *e, const char *who, const lk_noise_config *cfg, const void *out) {
  const std::string w(who);
  if (!cfg)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": no configuration").c_str());
  if (!out)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": no output").c_str());
  if (cfg->reserved[0] != 0 || cfg->reserved[1] != 0 || cfg->reserved[2] != 0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": reserved words must be 0").c_str());
  if (cfg->source != LK_NOISE_IMAGES && cfg->source != LK_NOISE_RING)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (w + ": unknown source (LK_NOISE_IMAGES or LK_NOISE_RING)").c_str());
  return LK_ERROR_NONE;
}

int frames_view(lk_engine *e, const char *who, const lk_noise_config *cfg, int need_sectors, LkFramesView *v) {
  return lk_internal_frames_view(e, who, cfg->source == LK_NOISE_RING, cfg->n_frames, cfg->slots, cfg->first, need_sectors, v);
}

bool frames_ok(int n_frames) { return n_frames >= 2 && n_frames <= LK_NOISE_MAX_FRAMES; }

} // namespace

extern "C" {

int lk_noise_from_bins(int n_frames, const int64_t *bins, const int64_t *frame_sums, int grey_low, int grey_high, int min_count,
                       struct lk_noise *out) {
  if (!bins || !frame_sums || !out || !frames_ok(n_frames) || grey_low < 0 || grey_low > 255 || grey_high < 0 || grey_high > 255 ||
      min_count < 2)
    return LK_ERROR_BAD_DOMAIN;
  for (int g = 0; g < 2 * kLkNoiseBins; ++g)
    if (bins[g] < 0)
      return LK_ERROR_BAD_DOMAIN;
  for (int f = 0; f < n_frames; ++f)
    if (frame_sums[f] < 0)
      return LK_ERROR_BAD_DOMAIN;
  const int64_t K = n_frames, KK1 = K * (K - 1);
  i128 N = 0, SQ = 0, F = 0; // pixels, sum q, sum of the frame sums
  for (int g = 0; g < kLkNoiseBins; ++g) {
    N += bins[2 * g];
    SQ += bins[2 * g + 1];
  }
  for (int f = 0; f < n_frames; ++f)
    F += frame_sums[f];
  std::memset(out, 0, sizeof *out);
  out->n_pixels = (int64_t)N;
  out->n_frames = n_frames;
  if (N < 2) {
    out->status = LK_NOISE_TOO_FEW;
    return LK_ERROR_NONE;
  }
  const double n = (double)N, k = (double)K;
  const double var = (double)SQ / (double)(N * KK1);
  const double mean = (double)F / (double)(N * K);
  // o_f = (K frame_sums[f] - F) / (K N): O2 = sum of the squared numerators
  i128 O2 = 0;
  for (int f = 0; f < n_frames; ++f) {
    const i128 d = (i128)K * frame_sums[f] - F;
    O2 += d * d;
  }
  const double flicker = std::sqrt((double)O2 / (k * k * k)) / n;
  // SQ / K - N sum o_f^2 = (SQ K N - O2) / (K^2 N)
  const i128 D = SQ * K * N - O2;
  const double var_detrended = D > 0 ? (double)D / ((double)(N * K * K) * (double)((N - 1) * (K - 1))) : 0.0;
  // the line over the usable bins, weights = counts: W, G = sum w g, G2 = sum w g^2, Q = sum (sum q_g), GQ = sum g (sum q_g)
  i128 W = 0, G = 0, G2 = 0, Q = 0, GQ = 0;
  int used = 0;
  for (int g = grey_low; g <= grey_high; ++g) {
    const int64_t c = bins[2 * g], q = bins[2 * g + 1];
    if (c < min_count)
      continue;
    ++used;
    W += c;
    G += (i128)c * g;
    G2 += (i128)c * g * g;
    Q += q;
    GQ += (i128)q * g;
  }
  const i128 det = W * G2 - G * G; // W^2 times the weighted variance of g: 0 without a spread
  double a = var, b = 0.0, rms = 0.0;
  int status = LK_NOISE_NO_MODEL;
  if (used >= 2 && det > 0) {
    status = LK_NOISE_OK;
    const double den = (double)det * (double)KK1;
    a = (double)(Q * G2 - G * GQ) / den;
    b = (double)(W * GQ - G * Q) / den;
    if (used > 2) { // (two bins: the line passes through both)
      double rr = 0.0;
      for (int g = grey_low; g <= grey_high; ++g) {
        const int64_t c = bins[2 * g];
        if (c < min_count)
          continue;
        const double r = (double)bins[2 * g + 1] / (double)(c * KK1) - (a + b * (double)g);
        rr += (double)c * (r * r);
      }
      rms = std::sqrt(rr / (double)W);
    }
  }
  const double at_mean = a + b * mean;
  out->var = var;
  out->var_detrended = var_detrended;
  out->a = a;
  out->b = b;
  out->status = status;
  out->bins_used = used;
  out->sigma = (float)std::sqrt(var);
  out->sigma_detrended = (float)std::sqrt(var_detrended);
  out->flicker = (float)flicker;
  out->mean = (float)mean;
  out->sigma_at_mean = (float)std::sqrt(at_mean > 0.0 ? at_mean : 0.0);
  out->fit_rms = (float)rms;
  return LK_ERROR_NONE;
}

int lk_noise_from_sums(int n_frames, const int64_t *sums3, struct lk_sector_noise *out) {
  if (!sums3 || !out || !frames_ok(n_frames) || sums3[0] < 0 || sums3[0] > INT32_MAX || sums3[1] < 0 || sums3[2] < 0)
    return LK_ERROR_BAD_DOMAIN;
  std::memset(out, 0, sizeof *out);
  out->n = (int32_t)sums3[0];
  if (sums3[0] < 2) {
    out->status = LK_NOISE_TOO_FEW;
    return LK_ERROR_NONE;
  }
  const int64_t K = n_frames;
  out->status = LK_NOISE_OK;
  out->var = (double)sums3[1] / (double)(sums3[0] * K * (K - 1));
  out->sigma = (float)std::sqrt(out->var);
  out->mean = (float)((double)sums3[2] / (double)(sums3[0] * K));
  return LK_ERROR_NONE;
}

int lk_camera_noise(lk_engine *e, const lk_noise_config *cfg, const uint8_t *mask, struct lk_noise *out, int64_t *bins_out,
                    int64_t *frame_sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (int rc = check_config(e, "lk_camera_noise", cfg, out))
    return rc;
  if (cfg->grey_low < 0 || cfg->grey_low > 255 || cfg->grey_high < 0 || cfg->grey_high > 255)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_camera_noise: grey_low and grey_high must lie in 0 .. 255");
  if (cfg->min_count < 2)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_camera_noise: min_count must be at least 2");
  LkFramesView v{};
  if (int rc = frames_view(e, "lk_camera_noise", cfg, 0, &v))
    return rc;
  int x0 = cfg->x0, y0 = cfg->y0, x1 = cfg->x1, y1 = cfg->y1;
  if (x0 == 0 && y0 == 0 && x1 == 0 && y1 == 0) { // the whole frame
    x1 = v.cols - 1;
    y1 = v.rows - 1;
  }
  if (x1 < x0 || y1 < y0)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_camera_noise: the region is empty (x0 <= x1 and y0 <= y1, inclusive)");
  if (x0 < 0 || y0 < 0 || x1 >= v.cols || y1 >= v.rows)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, "lk_camera_noise: the region leaves the level-py_start frame");
  NoiseState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_NOISE, kWhere, &st))
    return rc;
  const size_t pixels = (size_t)v.rows * (size_t)v.cols;
  LK_HIPCHK(st->tables.ensure(kTableWords * sizeof(unsigned long long)));
  if (mask) {
    LK_HIPCHK(st->mask.ensure(pixels));
    LK_HIPCHK(hipMemcpyAsync(st->mask.p, mask, pixels, hipMemcpyHostToDevice, v.stream));
  }
  LkNoiseFrameArgs a{};
  for (int f = 0; f < v.n_frames; ++f)
    a.frame[f] = v.frame[f];
  a.mask = mask ? st->mask.as<uint8_t>() : nullptr;
  a.n_frames = v.n_frames;
  a.rows = v.rows;
  a.cols = v.cols;
  a.x0 = x0;
  a.y0 = y0;
  a.w = x1 - x0 + 1;
  a.h = y1 - y0 + 1;
  a.bins = st->tables.as<unsigned long long>();
  a.frame_sums = a.bins + 2 * kLkNoiseBins;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(hipMemsetAsync(st->tables.p, 0, kTableWords * sizeof(unsigned long long), v.stream));
  LK_HIPCHK(lk_launch_noise_frames(a, &st->workgroups, v.stream));
  LK_HIPCHK(st->end(v.stream));
  int64_t tables[kTableWords];
  LK_HIPCHK(hipMemcpyAsync(tables, st->tables.p, sizeof tables, hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->finished();
  if (lk_noise_from_bins(v.n_frames, tables, tables + 2 * kLkNoiseBins, cfg->grey_low, cfg->grey_high, cfg->min_count, out) != LK_ERROR_NONE)
    return lk_internal_fail(e, LK_ERROR_DEVICE, "lk_camera_noise: the device's tables are not tables");
  if (bins_out)
    std::memcpy(bins_out, tables, 2 * kLkNoiseBins * sizeof(int64_t));
  if (frame_sums_out)
    std::memcpy(frame_sums_out, tables + 2 * kLkNoiseBins, (size_t)v.n_frames * sizeof(int64_t));
  return LK_ERROR_NONE;
}

int lk_sector_noise(lk_engine *e, const lk_noise_config *cfg, struct lk_sector_noise *out, int64_t *sums_out) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (int rc = check_config(e, "lk_sector_noise", cfg, out))
    return rc;
  LkFramesView v{};
  if (int rc = frames_view(e, "lk_sector_noise", cfg, 1, &v))
    return rc;
  NoiseState *st = nullptr;
  if (int rc = lk_pass_state(e, LK_PASS_NOISE, kWhere, &st))
    return rc;
  const size_t n = (size_t)v.S;
  int count[3];
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, count);
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->sums.ensure(n * kLkNoiseSums * sizeof(int64_t)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LkNoiseSectorArgs a{};
  a.ev.und = a.ev.def = v.frame[0];
  a.ev.urows = a.ev.drows = v.rows;
  a.ev.ucols = a.ev.dcols = v.cols;
  a.ev.xy = v.xy;
  a.ev.off = v.off;
  a.ev.rect = v.rect;
  a.ev.center = v.center;
  for (int f = 0; f < v.n_frames; ++f)
    a.frame[f] = v.frame[f];
  a.sums = st->sums.as<long long>();
  a.n_frames = v.n_frames;
  a.level = v.level;
  LK_HIPCHK(st->begin(v.stream));
  LK_HIPCHK(lk_pass_each_group(st->order.as<uint32_t>(), count, [&](int group, const uint32_t *order, int n_sectors) {
    a.ev.order = order;
    a.n_sectors = n_sectors;
    return lk_launch_noise_sectors(a, group, v.stream);
  }));
  LK_HIPCHK(st->end(v.stream));
  std::vector<int64_t> sums(n * kLkNoiseSums);
  LK_HIPCHK(hipMemcpyAsync(sums.data(), st->sums.p, sums.size() * sizeof(int64_t), hipMemcpyDeviceToHost, v.stream));
  LK_HIPCHK(hipStreamSynchronize(v.stream));
  st->workgroups = 0;
  st->finished();
  for (size_t s = 0; s < n; ++s)
    if (lk_noise_from_sums(v.n_frames, &sums[s * kLkNoiseSums], &out[s]) != LK_ERROR_NONE)
      return lk_internal_fail(e, LK_ERROR_DEVICE, "lk_sector_noise: the device's sums are not sums");
  if (sums_out)
    std::memcpy(sums_out, sums.data(), sums.size() * sizeof(int64_t));
  return LK_ERROR_NONE;
}

// bench hook (lk_internal.hpp)
int lk_internal_noise_last(lk_engine *e, float *device_ms, int *workgroups) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  NoiseState *st = nullptr;
  if (int rc = lk_pass_last(e, LK_PASS_NOISE, "lk_internal_noise_last: no lk_camera_noise or lk_sector_noise yet", device_ms, &st))
    return rc;
  if (workgroups)
    *workgroups = st->workgroups;
  return LK_ERROR_NONE;
}

} // extern "C"
