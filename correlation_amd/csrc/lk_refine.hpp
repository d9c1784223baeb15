// lk_refine.hpp - the host side the refinement passes share (lk_znssd.cpp, lk_quadratic.cpp, lk_spline.cpp, lk_weighted.cpp,
// lk_composed.cpp): the refusals, the state, the seeds and tables a call uploads, the fill of the two device argument
// blocks, the downloads and the tail of the *_step_from_sums exports.  A pass writes its own checks, and its own launches
// between lk_refine_prepare and lk_refine_finish ("adding a refinement variant").  Host only: no .hip
// file includes it.  Everything here has internal linkage: a copy per pass, no symbol of the library.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "lk_pass.hpp"
#include "lk_znssd.hpp"

namespace {

// What a pass keeps on its slot; a pass with buffers of its own derives from it.
struct LkRefineState : LkPassState {
  LkDevBytes rec, guess, second, order, count0, rec_out, out, sums, mask; // (every call uploads its mask: none can go stale)
  std::vector<uint32_t> h_order;
  std::vector<int32_t> h_count0;
  int count[3] = {0, 0, 0};
  hipError_t init() { return LkPassState::init(false); } // (no cell grid: no bounding box to land)
};

// the words every configuration begins with
struct LkRefineHead {
  int def_slot;
  float chi_max;
  int max_iters;
  float precision, lambda0;
};

// One call.  The pass fills the first block from its arguments; the steps below fill the others.
struct LkRefineCall {
  const char *who; // the pass's name, in front of every refusal
  const lk_result *records;
  const float *guesses, *second; // second, mask: null in a pass without them
  const uint8_t *mask;
  lk_result *records_out;
  void *info_out;
  double *sums_out;
  size_t info_bytes, n_sums; // of one sector: the pass's info record, the doubles of its kept sums
  LkRefineHead head{};       // lk_refine_check_head; lk_refine_check_view puts the defaults in
  // the weights' words of a configuration that has them, by the pass; zeros, which pass every check, in one that has not
  float sigma = 0.f, min_fraction = 0.f;
  int mask_rows = 0, mask_cols = 0;
  LkPassView v{}; // lk_refine_check_view
  // lk_refine_prepare: the seeds on the device, each null where the caller gave none; d_rec: also the engine-held records
  const lk_result *d_rec = nullptr;
  const float *d_guess = nullptr, *d_second = nullptr;
  const uint8_t *d_mask = nullptr;
  double *d_sums = nullptr;
};

inline int lk_refine_refuse(lk_engine *e, const LkRefineCall &c, const char *what) {
  return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(c.who) + ": " + what).c_str());
}

// the refusals every pass begins with; its own words come behind them
template <class Config> int lk_refine_check_head(lk_engine *e, LkRefineCall &c, const Config *cfg) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!cfg)
    return lk_refine_refuse(e, c, "no configuration");
  if (!c.records_out && !c.info_out)
    return lk_refine_refuse(e, c, "no output (records_out and info_out are both null)");
  for (int r : cfg->reserved)
    if (r != 0)
      return lk_refine_refuse(e, c, "reserved words must be 0");
  c.head = {cfg->def_slot, cfg->chi_max, cfg->max_iters, cfg->precision, cfg->lambda0};
  return LK_ERROR_NONE;
}

// The refusals behind the pass's own words - seeds, head, weights - then the view (the level images and lists, the engine-held
// records where the caller gave no seeds) and the mask against it; what the head left open takes lk_config's documented defaults.
inline int lk_refine_check_view(lk_engine *e, LkRefineCall &c) {
  constexpr int kDefaultIters = 50;
  constexpr float kDefaultPrecision = 1e-3f, kDefaultLambda = 1e-3f;
  LkRefineHead &h = c.head;
  if (c.records && c.guesses)
    return lk_refine_refuse(e, c, "records and guesses are both given (seeds are one or the other)");
  if (!std::isfinite(h.chi_max))
    return lk_refine_refuse(e, c, "chi_max must be finite (<= 0: the error code alone decides)");
  if (!std::isfinite(h.precision) || !std::isfinite(h.lambda0))
    return lk_refine_refuse(e, c, "precision and lambda0 must be finite (<= 0: the default)");
  if (!(c.sigma >= 0.f) || !std::isfinite(c.sigma))
    return lk_refine_refuse(e, c, "sigma must be finite and >= 0 (0: no window)");
  if (!(c.min_fraction >= 0.f && c.min_fraction <= 1.f))
    return lk_refine_refuse(e, c, "min_fraction must lie in [0, 1]");
  if (c.mask && (c.mask_rows <= 0 || c.mask_cols <= 0))
    return lk_refine_refuse(e, c, "a mask without dimensions (mask_rows, mask_cols)");
  if (!c.mask && (c.mask_rows != 0 || c.mask_cols != 0))
    return lk_refine_refuse(e, c, "mask dimensions without a mask (0, 0 with mask == NULL)");
  const bool held = !c.records && !c.guesses;
  if (int rc = lk_internal_pass_view(e, c.who, LK_VIEW_IMAGES | (held ? LK_VIEW_RECORDS : 0), h.def_slot, &c.v))
    return rc;
  if (c.mask && (c.mask_rows != c.v.urows || c.mask_cols != c.v.ucols))
    return lk_refine_refuse(e, c, "the mask dimensions are not those of the level-py_start undeformed image");
  h.max_iters = h.max_iters < 0 ? kDefaultIters : h.max_iters;
  h.precision = h.precision > 0.f ? h.precision : kDefaultPrecision;
  h.lambda0 = h.lambda0 > 0.f ? h.lambda0 : kDefaultLambda;
  return LK_ERROR_NONE;
}

// the window's constant at the view's level: *inv = log2(e) / (2 sigma_L^2), or 0 without a window
inline int lk_refine_window(lk_engine *e, const LkRefineCall &c, float *inv) {
  *inv = 0.f;
  if (c.sigma > 0.f) {
    const double sigma_l = std::ldexp((double)c.sigma, -c.v.level);
    *inv = (float)(1.4426950408889634 / (2.0 * sigma_l * sigma_l)); // log2(e)
    if (!(*inv > 0.f) || !std::isfinite(*inv))
      return lk_refine_refuse(e, c, "sigma is outside the range a float window can have");
  }
  return LK_ERROR_NONE;
}

// The state of pass `which` (State: an LkRefineState; `where` as lk_pass_state), the sectors by lane group and their
// level-0 counts, the buffers of the outputs, and what the caller passed on its way to the device: all of it on the view's
// stream, ahead of the timed part.
template <class State> int lk_refine_prepare(lk_engine *e, LkRefineCall &c, int which, const char *where, State **state) {
  if (int rc = lk_pass_state(e, which, where, state))
    return rc;
  LkRefineState *st = *state;
  const LkPassView &v = c.v;
  const size_t n = (size_t)v.S;
  lk_pass_order_by_group(v.h_rect0, v.h_off0, v.S, st->h_order, st->count);
  st->h_count0.resize(n);
  for (size_t s = 0; s < n; ++s)
    st->h_count0[s] = lk_pass_count0(v.h_rect0, v.h_off0, s);
  LK_HIPCHK(st->order.ensure(n * sizeof(uint32_t)));
  LK_HIPCHK(st->count0.ensure(n * sizeof(int32_t)));
  LK_HIPCHK(st->rec_out.ensure(n * sizeof(lk_result)));
  LK_HIPCHK(st->out.ensure(n * c.info_bytes));
  if (c.sums_out)
    LK_HIPCHK(st->sums.ensure(n * c.n_sums * sizeof(double)));
  LK_HIPCHK(hipMemcpyAsync(st->order.p, st->h_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, v.stream));
  LK_HIPCHK(hipMemcpyAsync(st->count0.p, st->h_count0.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, v.stream));
  if (c.mask) {
    const size_t bytes = (size_t)v.urows * (size_t)v.ucols;
    LK_HIPCHK(st->mask.ensure(bytes));
    LK_HIPCHK(hipMemcpyAsync(st->mask.p, c.mask, bytes, hipMemcpyHostToDevice, v.stream));
  }
  c.d_rec = c.guesses ? nullptr : v.result;
  if (int rc = lk_pass_records(e, st->rec, c.records, n, v.stream, &c.d_rec))
    return rc;
  if (c.guesses) {
    LK_HIPCHK(st->guess.ensure(n * 6 * sizeof(float)));
    LK_HIPCHK(hipMemcpyAsync(st->guess.p, c.guesses, n * 6 * sizeof(float), hipMemcpyHostToDevice, v.stream));
  }
  if (c.second) {
    LK_HIPCHK(st->second.ensure(n * 6 * sizeof(float)));
    LK_HIPCHK(hipMemcpyAsync(st->second.p, c.second, n * 6 * sizeof(float), hipMemcpyHostToDevice, v.stream));
  }
  c.d_guess = c.guesses ? st->guess.as<float>() : nullptr;
  c.d_second = c.second ? st->second.as<float>() : nullptr;
  c.d_mask = c.mask ? st->mask.as<uint8_t>() : nullptr;
  c.d_sums = c.sums_out ? st->sums.as<double>() : nullptr;
  return LK_ERROR_NONE;
}

// The device arguments of the first-order loop but for three: where the info goes is the pass's to say (a.out, or the block
// around `a`), and n_sectors and ev.order are set per launch.
template <class Args = LkZnssdArgs> void lk_refine_fill(Args &a, const LkRefineCall &c, LkRefineState *st) {
  a.ev = lk_pass_sector_eval(c.v, c.d_rec);
  a.guess = c.d_guess;
  a.count0 = st->count0.as<int32_t>();
  a.rec_out = st->rec_out.as<lk_result>();
  a.sums = c.d_sums;
  a.level = c.v.level;
  a.max_iters = c.head.max_iters;
  a.chi_max = c.head.chi_max;
  a.precision = c.head.precision;
  a.lambda0 = c.head.lambda0;
}
// and of the second-order loop: the same words, and its two own
inline void lk_refine_fill_second(LkQuadraticArgs &a, const LkRefineCall &c, LkRefineState *st) {
  lk_refine_fill(a, c, st);
  a.second = c.d_second;
  a.model = c.v.model;
}

// Behind the pass's last launch: the end of the timed part, the outputs to the caller, the one wait of the call.
inline int lk_refine_finish(lk_engine *e, const LkRefineCall &c, LkRefineState *st) {
  const size_t n = (size_t)c.v.S;
  LK_HIPCHK(st->end(c.v.stream));
  if (c.records_out)
    LK_HIPCHK(hipMemcpyAsync(c.records_out, st->rec_out.p, n * sizeof(lk_result), hipMemcpyDeviceToHost, c.v.stream));
  if (c.info_out)
    LK_HIPCHK(hipMemcpyAsync(c.info_out, st->out.p, n * c.info_bytes, hipMemcpyDeviceToHost, c.v.stream));
  if (c.sums_out)
    LK_HIPCHK(hipMemcpyAsync(c.sums_out, st->sums.p, n * c.n_sums * sizeof(double), hipMemcpyDeviceToHost, c.v.stream));
  LK_HIPCHK(hipStreamSynchronize(c.v.stream));
  st->finished();
  return LK_ERROR_NONE;
}

// the tail of a *_step_from_sums export: the step and the criterion into the outputs the caller gave
inline void lk_refine_step_out(const double *delta, int n_delta, const LkZnCriterion &cr, double *delta_out, double *crit,
                               double *gain_offset2) {
  if (delta_out)
    for (int k = 0; k < n_delta; ++k)
      delta_out[k] = delta[k];
  if (crit)
    *crit = cr.crit;
  if (gain_offset2) {
    gain_offset2[0] = cr.gain;
    gain_offset2[1] = cr.offset;
  }
}

} // namespace
