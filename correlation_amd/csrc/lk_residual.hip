// lk_residual.hip - device side of the photometry pass and the back-warped residual map (include/lk_engine.h: lk_photometry,
// lk_residual_map).
//
// photometry  lk_uncertainty.hip's evaluation with other sums.  One lane group evaluates one good sector once, at its
//             record's parameters and at the finest level the solve reaches: a 16-lane DPP row, a wavefront or a 512-thread
//             workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).  A sample is f = the undeformed
//             node, g = sample_def<> at Warp<>::apply, V = f - g, in float; f, g, f^2, g^2, f g, V^2 are formed and summed in
//             double, the flagged samples are counted and max |V| is kept.  Lane j takes the samples j, j + G, ...; the
//             reduction (lk_sector_eval.hpp: DPP inside rows, readlane across rows, LDS across wavefronts) has one fixed
//             order, so a sector's eight numbers and its record are the same bytes in any launch.  Lane 0 turns them into
//             the record with the function the host exports (lk_residual.hpp).
// map prep    a thread per sector: the good rule once per record; the level-0 centre (cx = NaN marks a sector that owns
//             nothing - it fails the distance test by itself), the level-L centre and the level-L parameters in 48 bytes.
// map         one workgroup per tile of 32 x 8 pixels, x fastest: a wavefront covers two image rows of 32 pixels, so the
//             byte loads of the undeformed pixel and the stores of the three maps are contiguous along image rows, and
//             neighbouring lanes read neighbouring 4 x 4 windows of the deformed image.  A pixel's candidates are the
//             members of the 3 x 3 cells around its cell (cell size = radius); the cells of all pixels of a tile form a
//             rectangle of cells, whose members' centres and indices are staged once in LDS (12 bytes each, up to
//             kLkMapCapacity) and searched by every pixel - all lanes read the same address at a time, a broadcast.  A
//             superset of a pixel's own candidates changes nothing: only centres within the radius compete, and those lie in
//             its 3 x 3 cells.  A tile whose rectangle holds more members than fit takes the fall-back: every pixel walks
//             its own 3 x 3 cells in global memory - the same rule, the same bits.  Then the owner's 48 bytes, the solve's
//             warp and sampler, three stores.
#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_residual.hpp"
#include "lk_sector_eval.hpp"

namespace {

constexpr int kPhotoLdsStride = 8; // doubles per wavefront in the cross-wavefront reduction
constexpr int kPhotoAdds = 7;      // the six sums and the flagged count; slot 7 is the maximum

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_photometry_kernel(LkPhotometryArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL);
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kPhotoLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid], level = a.level;
  const lk_result rec = a.ev.rec[s];
  const bool good = reseed_good(rec, P, a.chi_max);
  const SectorLevel c = sector_level(a.ev, s, level, a.ev.center[s]);
  const int n = c.n;
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = i < P ? rec.resultingParameters[i] : 0.f;
  translate<P>(p, 0, level);
  double v[kLkPhotoSums];
#pragma unroll
  for (int i = 0; i < kLkPhotoSums; ++i)
    v[i] = 0.0;
  for (int k = lane; k < (good ? n : 0); k += GROUP) { // (a record that is not good is not evaluated)
    const f32x2 q = sector_sample(c, k);
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply(q.x, q.y, c.cx, c.cy, p, xd, yd, dx, dy);
    const float f = sector_und_node(c, q);
    float g;
    if (!sample_def_value<INTERP>(c.def, c.drows, c.dcols, xd, yd, g)) {
      v[6] += 1.0;
      continue; // the sums of an evaluation that hit the error are never used
    }
    const float V = f - g;
    const double fd = (double)f, gd = (double)g, Vd = (double)V;
    v[0] += fd;
    v[1] += gd;
    v[2] += fd * fd; // (no contraction: a rounded product, then a rounded sum)
    v[3] += gd * gd;
    v[4] += fd * gd;
    v[5] += Vd * Vd;
    v[7] = max_f64(v[7], (double)fabsf(V));
  }
  reduce_f64<GROUP, kPhotoAdds, kLkPhotoSums - kPhotoAdds, kPhotoLdsStride>(v, lds);
  if (lane != 0)
    return;
  const bool evaluated = good && v[6] == 0.0;
  double sums[kLkPhotoSums];
#pragma unroll
  for (int i = 0; i < kLkPhotoSums; ++i)
    sums[i] = evaluated ? v[i] : 0.0;
  struct lk_photometry r;
  if (!good)
    lk_photometry_clear(&r, n, LK_PHOTO_BAD_RECORD);
  else if (!evaluated)
    lk_photometry_clear(&r, n, LK_PHOTO_OUT_OF_IMAGE);
  else
    lk_photometry_record(n, sums, &r);
  a.out[s] = r;
  if (a.sums) {
#pragma unroll
    for (int i = 0; i < kLkPhotoSums; ++i)
      a.sums[(size_t)s * kLkPhotoSums + i] = sums[i];
  }
}

// ---- residual map ------------------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ __launch_bounds__(kBlock) void lk_map_prep_kernel(const lk_result *rec, const float2 *center, int n, int level,
                                                             float chi_max, LkMapSector *pack) {
  constexpr int P = n_params(MODEL);
  const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (s >= n)
    return;
  const lk_result r = rec[s];
  const bool g = reseed_good(r, P, chi_max);
  const float2 c = center[s];
  const float inv = 1.f / (float)(1 << level); // as the solve kernels scale the centre
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = i < P ? r.resultingParameters[i] : 0.f;
  translate<P>(p, 0, level);
  LkMapSector o;
  o.cx0 = g ? c.x : __uint_as_float(0x7fc00000u);
  o.cy0 = c.y;
  o.cx = level == 0 ? c.x : c.x * inv;
  o.cy = level == 0 ? c.y : c.y * inv;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    o.p[i] = p[i];
  o.pad[0] = o.pad[1] = 0.f;
  pack[s] = o;
}

template <int MODEL, int INTERP> __global__ __launch_bounds__(kBlock) void lk_residual_map_kernel(LkResidualMapArgs a) {
  static_assert(kLkMapTileW * kLkMapTileH == kBlock, "a thread per pixel of the tile");
  __shared__ float s_cx[kLkMapCapacity], s_cy[kLkMapCapacity];
  __shared__ int s_idx[kLkMapCapacity];
  const LkReseedGrid &g = a.grid;
  const int tid = (int)threadIdx.x;
  const int tile_x = (int)blockIdx.x % a.tiles_x, tile_y = (int)blockIdx.x / a.tiles_x;
  // the tile's pixels, and the rectangle of cells their 3 x 3 neighbourhoods cover (uniform over the workgroup)
  const int px0 = a.x0 + tile_x * kLkMapTileW, py0 = a.y0 + tile_y * kLkMapTileH;
  const int px1 = min(px0 + kLkMapTileW, a.x0 + a.w) - 1, py1 = min(py0 + kLkMapTileH, a.y0 + a.h) - 1;
  const double up = (double)(1 << a.level);
  const uint32_t S = (uint32_t)a.n_sectors;
  const CellRange cells = cell_range(g, free_cell_coord((double)px0 * up, g.x0, g.cell, g.nx), free_cell_coord((double)px1 * up, g.x0, g.cell, g.nx),
                                     free_cell_coord((double)py0 * up, g.y0, g.cell, g.ny), free_cell_coord((double)py1 * up, g.y0, g.cell, g.ny));
  const long long total = cell_range_entries(g, cells, S);
  const bool staged = total <= (long long)kLkMapCapacity;
  if (staged) {
    walk_entries<kBlock>(g, cells, S, tid, [&](uint32_t at, uint32_t m) { // at < total <= kLkMapCapacity
      const bool known = m < S;
      s_idx[at] = known ? (int)m : 0;
      s_cx[at] = known ? a.pack[m].cx0 : __uint_as_float(0x7fc00000u);
      s_cy[at] = known ? a.pack[m].cy0 : 0.f;
    });
    __syncthreads();
  } else if (tid == 0) {
    atomicAdd(a.fallback, 1u);
  }
  const int x = px0 + tid % kLkMapTileW, y = py0 + tid / kLkMapTileW;
  if (x > px1 || y > py1) // (behind the only barrier)
    return;
  const double X = (double)x * up, Y = (double)y * up;
  int best = -1;
  double best_d2 = 0.0;
  if (staged) {
    for (int i = 0; i < (int)total; ++i) {
      const double d2 = lk_map_d2(s_cx[i], s_cy[i], X, Y);
      const int m = s_idx[i];
      if (d2 <= a.r2 && lk_map_better(d2, m, best_d2, best)) { // (a NaN centre - a sector that is not good - is outside)
        best = m;
        best_d2 = d2;
      }
    }
  } else {
    const CellRange around = cell_range(g, free_cell_coord(X, g.x0, g.cell, g.nx), free_cell_coord(Y, g.y0, g.cell, g.ny));
    walk_members<1>(g, around, S, 0, [&](uint32_t m) {
      const double d2 = lk_map_d2(a.pack[m].cx0, a.pack[m].cy0, X, Y);
      if (d2 <= a.r2 && lk_map_better(d2, (int)m, best_d2, best)) {
        best = (int)m;
        best_d2 = d2;
      }
    });
  }
  const float nan = __uint_as_float(0x7fc00000u);
  float W = nan, R = nan;
  int own = -1;
  if (best >= 0) {
    const float4 *q = (const float4 *)(a.pack + best); // (48-byte entries in hipMalloc'ed memory: 16-byte aligned)
    const float4 q0 = q[0], q1 = q[1], q2 = q[2];
    const float p[6] = {q1.x, q1.y, q1.z, q1.w, q2.x, q2.y};
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply((float)x, (float)y, q0.z, q0.w, p, xd, yd, dx, dy);
    float val;
    if (sample_def_value<INTERP>((gptr<uint8_t>)a.def, a.drows, a.dcols, xd, yd, val)) {
      const float f = (float)((gptr<uint8_t>)a.und)[(size_t)y * (size_t)a.ucols + (size_t)x]; // (the window is inside the image)
      W = val;
      R = f - val;
      own = best;
    } else {
      own = -2 - best;
    }
  }
  const size_t at = (size_t)(y - a.y0) * (size_t)a.w + (size_t)(x - a.x0);
  if (a.warped)
    a.warped[at] = W;
  if (a.residual)
    a.residual[at] = R;
  if (a.owner)
    a.owner[at] = own;
}

} // namespace

hipError_t lk_launch_photometry(const LkPhotometryArgs &a, int model, int interp, int group, hipStream_t st) {
  return dispatch_sector_kernel(model, interp, group, [&](auto m, auto i, auto g) {
    constexpr int M = decltype(m)::value, I = decltype(i)::value, G = decltype(g)::value;
    return launch_sector_groups<G>(lk_photometry_kernel<M, I, G>, a, a.n_sectors, st);
  });
}

hipError_t lk_launch_map_prep(const lk_result *rec, const float2 *center, int n_sectors, int model, int level, float chi_max,
                              LkMapSector *pack, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  return dispatch_model(model, [&](auto m) {
    hipLaunchKernelGGL(lk_map_prep_kernel<decltype(m)::value>, dim3(blocks_for(n_sectors, kBlock)), dim3(kBlock), 0, st, rec, center,
                       n_sectors, level, chi_max, pack);
    return hipGetLastError();
  });
}

hipError_t lk_launch_residual_map(const LkResidualMapArgs &a, int model, int interp, int *n_tiles, hipStream_t st) {
  if (a.n_sectors <= 0 || a.w <= 0 || a.h <= 0 || a.tiles_x != (a.w + kLkMapTileW - 1) / kLkMapTileW)
    return hipErrorInvalidValue;
  const long long tiles = (long long)a.tiles_x * (long long)((a.h + kLkMapTileH - 1) / kLkMapTileH);
  if (tiles > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (n_tiles)
    *n_tiles = (int)tiles;
  return dispatch_model(model, [&](auto m) {
    return dispatch_interp(interp, [&](auto i) {
      hipLaunchKernelGGL((lk_residual_map_kernel<decltype(m)::value, decltype(i)::value>), dim3((unsigned)tiles), dim3(kBlock), 0, st, a);
      return hipGetLastError();
    });
  });
}
