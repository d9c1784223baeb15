// lk_pass.hpp - the host plumbing the add-on passes share (lk_reseed.cpp, lk_strain.cpp, lk_uncertainty.cpp, lk_outlier.cpp,
// lk_track.cpp, lk_residual.cpp, lk_pattern.cpp, lk_field.cpp, lk_motion.cpp, lk_noise.cpp, lk_lens.cpp, lk_stereo.cpp and, through lk_refine.hpp, the five
// refinement passes; the error macro also lk_guess_search.cpp): device buffers that free themselves, the state a pass keeps on
// its slot of the engine, the upload of caller records, the bounding box and cell grid over the centres, the order of the
// sectors by lane group and the launch per group.  Host only: no .hip file includes it; the device half is lk_neighbours.hpp
// and lk_sector_eval.hpp.  A new pass starts here ("adding a pass").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/lk_engine.h"
#include "lk_device.hpp"
#include "lk_internal.hpp"

// in a function that has the engine as `e` and returns an lk error code
#define LK_HIPCHK(call)                                                                               \
  do {                                                                                                \
    hipError_t _e = (call);                                                                           \
    if (_e != hipSuccess)                                                                             \
      return lk_internal_hipfail(e, _e, #call);                                                       \
  } while (0)

struct LkDevBytes { // device memory grown on demand, never shrunk, freed with its owner
  void *p = nullptr;
  size_t bytes = 0;
  LkDevBytes() = default;
  LkDevBytes(const LkDevBytes &) = delete;
  LkDevBytes &operator=(const LkDevBytes &) = delete;
  ~LkDevBytes() {
    if (p)
      (void)hipFree(p);
  }
  hipError_t ensure(size_t want) {
    if (p && want <= bytes)
      return hipSuccess;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    bytes = 0;
    const hipError_t err = hipMalloc(&p, std::max<size_t>(want, 16));
    if (err == hipSuccess)
      bytes = want;
    return err;
  }
  template <class T> T *as() const { return (T *)p; }
};

#include "lk_cell_grid.hpp" // (LkCellGridBufs is made of LkDevBytes)

// What a pass with a timed device part keeps on its slot besides its own buffers: the two events that bracket that part
// (read by the pass's lk_internal_*_last bench hook) and the pinned landing place of the centres' bounding box.
struct LkPassState : LkPassSlot {
  float *h_bbox = nullptr; // pinned [4]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;      // ev0 / ev1 bracket the device part of a finished call
  hipError_t init(bool with_bbox = true) {
    hipError_t err = with_bbox ? hipHostMalloc((void **)&h_bbox, 4 * sizeof(float), hipHostMallocDefault) : hipSuccess;
    if (err == hipSuccess)
      err = hipEventCreate(&ev0);
    if (err == hipSuccess)
      err = hipEventCreate(&ev1);
    return err;
  }
  ~LkPassState() override {
    if (h_bbox)
      (void)hipHostFree(h_bbox);
    if (ev0)
      (void)hipEventDestroy(ev0);
    if (ev1)
      (void)hipEventDestroy(ev1);
  }
  hipError_t begin(hipStream_t stream) {
    timed = false;
    return hipEventRecord(ev0, stream);
  }
  hipError_t end(hipStream_t stream) { return hipEventRecord(ev1, stream); }
  void finished() { timed = true; }
  hipError_t elapsed(float *ms) const { return hipEventElapsedTime(ms, ev0, ev1); }
};

// The state of pass `which` (T: an LkPassSlot with a hipError_t init()), made on first use; `where` names the calls of init()
// in the message of a failure.
template <class T> int lk_pass_state(lk_engine *e, int which, const char *where, T **out) {
  LkPassSlot **slot = lk_internal_pass_slot(e, which);
  if (!*slot) {
    T *st = new T();
    const hipError_t err = st->init();
    if (err != hipSuccess) {
      delete st;
      return lk_internal_hipfail(e, err, where);
    }
    *slot = st;
  }
  *out = static_cast<T *>(*slot);
  return LK_ERROR_NONE;
}

// The first lines of a pass's bench hook: its state once a call has finished (else the refusal `none_yet`) and, where
// device_ms is given, the time between the two events.
template <class T> int lk_pass_last(lk_engine *e, int which, const char *none_yet, float *device_ms, T **out) {
  T *st = static_cast<T *>(*lk_internal_pass_slot(e, which));
  if (!st || !st->timed)
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, none_yet);
  if (device_ms)
    LK_HIPCHK(st->elapsed(device_ms));
  *out = st;
  return LK_ERROR_NONE;
}

// The whole hook of a pass that launches per lane group (T has count[3], lk_pass_order_by_group's): also the sectors each
// group took; `state`: for what the pass reports besides.
template <class T> int lk_pass_last_groups(lk_engine *e, int which, const char *none_yet, float *device_ms, int *count3, T **state = nullptr) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  T *st = nullptr;
  if (int rc = lk_pass_last(e, which, none_yet, device_ms, &st))
    return rc;
  if (count3)
    for (int g = 0; g < 3; ++g)
      count3[g] = st->count[g];
  if (state)
    *state = st;
  return LK_ERROR_NONE;
}

// Records the caller passed (`count` of them) go to the device through `rec` and replace *d_rec, the engine's; null: nothing
// happens.  R: lk_result or const lk_result.
template <class R>
int lk_pass_records(lk_engine *e, LkDevBytes &rec, const lk_result *records, size_t count, hipStream_t stream, R **d_rec) {
  if (!records)
    return LK_ERROR_NONE;
  LK_HIPCHK(rec.ensure(count * sizeof(lk_result)));
  LK_HIPCHK(hipMemcpyAsync(rec.p, records, count * sizeof(lk_result), hipMemcpyHostToDevice, stream));
  *d_rec = rec.as<lk_result>();
  return LK_ERROR_NONE;
}

// The cell grid over the centres for a pass that looks for neighbours within `radius`: the centres' bounding box sizes it,
// which is the call's one round trip before its kernels.  d_bbox: 4 floats on the device.
inline int lk_pass_grid(lk_engine *e, const char *who, LkPassState *st, const LkDevBytes &d_bbox, LkCellGridBufs &bufs,
                        const float2 *center, int n_sectors, float radius, hipStream_t stream, LkReseedGrid *g) {
  LK_HIPCHK(lk_launch_reseed_bbox(center, n_sectors, d_bbox.as<float>(), stream));
  LK_HIPCHK(hipMemcpyAsync(st->h_bbox, d_bbox.p, 4 * sizeof(float), hipMemcpyDeviceToHost, stream));
  LK_HIPCHK(hipStreamSynchronize(stream));
  if (!lk_cell_grid_bbox_finite(st->h_bbox))
    return lk_internal_fail(e, LK_ERROR_BAD_DOMAIN, (std::string(who) + ": a sector centre is not finite").c_str());
  LK_HIPCHK(lk_cell_grid_build(bufs, center, n_sectors, radius, st->h_bbox, stream, g));
  return LK_ERROR_NONE;
}

// a sector's level-0 sample count: the rectangle's, or the length of its explicit list (rectangle width 0)
inline int lk_pass_count0(const int4 *h_rect0, const uint32_t *h_off0, size_t s) {
  const int4 r = h_rect0[s];
  return r.z > 0 ? r.w : (int)(h_off0[s + 1] - h_off0[s]);
}

// The sectors by lane group, from the level-0 sample count alone, as the backward solve's tables: h_order holds the sectors
// of kLkPassGroups[0], then [1], then [2]; count[g] says how many each took.
constexpr int kLkPassGroups[3] = {16, 64, 512};
inline void lk_pass_order_by_group(const int4 *h_rect0, const uint32_t *h_off0, int S, std::vector<uint32_t> &h_order, int count[3]) {
  h_order.resize((size_t)S);
  size_t at = 0;
  for (int g = 0; g < 3; ++g) {
    const size_t begin = at;
    for (int s = 0; s < S; ++s)
      if (lk_bw_group(lk_pass_count0(h_rect0, h_off0, (size_t)s)) == kLkPassGroups[g])
        h_order[at++] = (uint32_t)s;
    count[g] = (int)(at - begin);
  }
}

// A launch per lane group: launch(group, order, n) for every group that took sectors, with the part of d_order
// (lk_pass_order_by_group's, on the device) that is its own; the first failure ends the walk.
template <class F> hipError_t lk_pass_each_group(const uint32_t *d_order, const int count[3], F &&launch) {
  hipError_t err = hipSuccess;
  for (int g = 0; g < 3 && err == hipSuccess; d_order += count[g++])
    if (count[g] > 0)
      err = launch(kLkPassGroups[g], d_order, count[g]);
  return err;
}

// What the kernels of lk_sector_eval.hpp read of the view (LK_VIEW_IMAGES), for the records d_rec; the caller sets `order`
// per launch.
inline LkSectorEvalArgs lk_pass_sector_eval(const LkPassView &v, const lk_result *d_rec) {
  LkSectorEvalArgs a{};
  a.und = v.und;
  a.def = v.def;
  a.urows = v.urows;
  a.ucols = v.ucols;
  a.drows = v.drows;
  a.dcols = v.dcols;
  a.xy = v.xy;
  a.off = v.off;
  a.rect = v.rect;
  a.center = v.center;
  a.rec = d_rec;
  return a;
}

// an environment variable that chooses between a and b (tuning experiments and test hooks); anything else: `otherwise`
inline int lk_pass_env_choice(const char *name, int a, int b, int otherwise) {
  const char *s = std::getenv(name);
  if (!s || !*s)
    return otherwise;
  const int v = std::atoi(s);
  return v == a || v == b ? v : otherwise;
}
