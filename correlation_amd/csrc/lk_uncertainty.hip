// lk_uncertainty.hip - per-sector uncertainty of the solved parameters (include/lk_engine.h: lk_parameter_uncertainty;
// DESIGN.md section 16).
//
// One lane group evaluates one sector once, at its record's parameters and at the finest level the solve reaches: a
// 16-lane DPP row, a wavefront or a 512-thread workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).
// A sample is the forward evaluation's - Warp<>::apply, sample_def<>, the residual against the undeformed node,
// Warp<>::jac, in float - and its products J_a J_b, J_a V, V^2 are formed and summed in double.  Lane j takes the samples
// j, j + G, j + 2G, ...; the reduction (lk_sector_eval.hpp: DPP inside rows, readlane across rows, LDS across wavefronts)
// has one fixed order, so a sector's sums and record are the same bytes in any launch.  Lane 0 of the group turns the
// sums into the record with the function the host exports (lk_uncertainty.hpp).
#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_sector_eval.hpp"
#include "lk_uncertainty.hpp"

namespace {

constexpr int kUncLdsStride = 32; // doubles per wavefront in the cross-wavefront reduction (29 used at most)

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_uncertainty_kernel(LkUncertaintyArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL), NA = P * (P + 1) / 2, N = NA + P + 1;
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kUncLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid], level = a.level;
  const lk_result rec = a.ev.rec[s];
  const bool good = reseed_good(rec, P, 0.f);
  const SectorLevel c = sector_level(a.ev, s, level, a.ev.center[s]);
  const int n = c.n;
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = i < P ? rec.resultingParameters[i] : 0.f;
  translate<P>(p, 0, level); // the record is in level-0 scale (pyramid_class.cpp:260-287, as the solve between levels)
  double v[N + 1]; // the sums, and the samples the sampler flagged
#pragma unroll
  for (int i = 0; i <= N; ++i)
    v[i] = 0.0;
  for (int k = lane; k < (good ? n : 0); k += GROUP) { // (a bad record is not evaluated)
    const f32x2 q = sector_sample(c, k);
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply(q.x, q.y, c.cx, c.cy, p, xd, yd, dx, dy);
    const float und_w = sector_und_node(c, q);
    float W, Wx, Wy;
    if (!sample_def<INTERP>(c.def, c.drows, c.dcols, xd, yd, W, Wx, Wy)) {
      v[N] += 1.0;
      continue; // the sums of an evaluation that hit the error are never used
    }
    const float V = und_w - W;
    float H[P];
    Warp<MODEL>::jac(Wx, Wy, dx, dy, H);
    double Hd[P];
#pragma unroll
    for (int i = 0; i < P; ++i)
      Hd[i] = (double)H[i];
    const double Vd = (double)V;
    int idx = 0;
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1)
#pragma unroll
      for (int p2 = p1; p2 < P; ++p2)
        v[idx] += Hd[p1] * Hd[p2], ++idx; // (no contraction: a rounded product, then a rounded sum)
#pragma unroll
    for (int p1 = 0; p1 < P; ++p1)
      v[NA + p1] += Hd[p1] * Vd;
    v[N - 1] += Vd * Vd;
  }
  reduce_f64<GROUP, N + 1, 0, kUncLdsStride>(v, lds);
  if (lane != 0)
    return;
  const bool evaluated = good && v[N] == 0.0;
  double sums[kLkUncSums];
#pragma unroll
  for (int i = 0; i < kLkUncSums; ++i)
    sums[i] = i < N && evaluated ? v[i] : 0.0;
  lk_uncertainty r;
  if (!good)
    lk_uncertainty_clear(&r, n, LK_UNC_BAD_RECORD);
  else if (!evaluated)
    lk_uncertainty_clear(&r, n, LK_UNC_OUT_OF_IMAGE);
  else
    lk_uncertainty_record<P>(n, sums, level, &r);
  a.out[s] = r;
  if (a.sums) {
#pragma unroll
    for (int i = 0; i < kLkUncSums; ++i)
      a.sums[(size_t)s * kLkUncSums + i] = sums[i];
  }
}

} // namespace

hipError_t lk_launch_uncertainty(const LkUncertaintyArgs &a, int model, int interp, int group, hipStream_t st) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    return launch_sector_groups<G>(lk_uncertainty_kernel<M, I, G>, a, a.n_sectors, st);
  });
}
