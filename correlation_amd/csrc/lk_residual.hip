// lk_residual.hip - device side of the photometry pass and the back-warped residual map (include/lk_engine.h: lk_photometry,
// lk_residual_map).
//
// photometry  lk_uncertainty.hip's evaluation with other sums.  One lane group evaluates one good sector once, at its
//             record's parameters and at the finest level the solve reaches: a 16-lane DPP row, a wavefront or a 512-thread
//             workgroup, chosen from the sector's level-0 sample count alone (lk_bw_group).  A sample is f = the undeformed
//             node, g = sample_def<> at Warp<>::apply, V = f - g, in float; f, g, f^2, g^2, f g, V^2 are formed and summed in
//             double, the flagged samples are counted and max |V| is kept.  Lane j takes the samples j, j + G, ...; the
//             reduction (DPP inside rows, readlane across rows, LDS across wavefronts) has the uncertainty kernel's fixed
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
#include "lk_good.hpp"
#include "lk_launch.hpp"
#include "lk_residual.hpp"
#include "lk_solver_common.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kPhotoLdsStride = 8; // doubles per wavefront in the cross-wavefront reduction
constexpr int kPhotoAdds = 7;      // the six sums and the flagged count; slot 7 is the maximum

template <int CTRL> __device__ __forceinline__ double dpp_get_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ double max_f64(double a, double b) { return a > b ? a : b; } // (never a NaN: |V| of finite floats)

template <int CTRL> __device__ __forceinline__ void photo_stage(double (&v)[kLkPhotoSums]) {
#pragma unroll
  for (int i = 0; i < kPhotoAdds; ++i)
    v[i] = v[i] + dpp_get_f64<CTRL>(v[i]);
  v[kPhotoAdds] = max_f64(v[kPhotoAdds], dpp_get_f64<CTRL>(v[kPhotoAdds]));
}

// The eight numbers over the group, in the order of unc_reduce (lk_uncertainty.hip); every lane ends with the same bits.
// GROUP <= 64 uses no barrier; GROUP == 512 is the whole (uniform) workgroup.
template <int GROUP> __device__ __forceinline__ void photo_reduce(double (&v)[kLkPhotoSums], double *lds) {
  photo_stage<0xB1>(v);  // quad_perm [1,0,3,2]
  photo_stage<0x4E>(v);  // quad_perm [2,3,0,1]
  photo_stage<0x141>(v); // row_half_mirror
  photo_stage<0x140>(v); // row_mirror
  if constexpr (GROUP >= 64) {
#pragma unroll
    for (int i = 0; i < kPhotoAdds; ++i)
      v[i] = (readlane_f64(v[i], 0) + readlane_f64(v[i], 16)) + (readlane_f64(v[i], 32) + readlane_f64(v[i], 48));
    v[kPhotoAdds] = max_f64(max_f64(readlane_f64(v[kPhotoAdds], 0), readlane_f64(v[kPhotoAdds], 16)),
                            max_f64(readlane_f64(v[kPhotoAdds], 32), readlane_f64(v[kPhotoAdds], 48)));
  }
  if constexpr (GROUP > 64) {
    constexpr int WAVES = GROUP / kWave;
    const int wave = (int)threadIdx.x / kWave;
    if ((int)threadIdx.x % kWave == 0) {
#pragma unroll
      for (int i = 0; i < kLkPhotoSums; ++i)
        lds[wave * kPhotoLdsStride + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kLkPhotoSums; ++i) {
      double t = lds[i];
      for (int w = 1; w < WAVES; ++w)
        t = i < kPhotoAdds ? t + lds[w * kPhotoLdsStride + i] : max_f64(t, lds[w * kPhotoLdsStride + i]);
      v[i] = t;
    }
  }
}

template <int MODEL, int INTERP, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_photometry_kernel(LkPhotometryArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  constexpr int P = n_params(MODEL);
  __shared__ double lds[(GROUP > 64 ? GROUP / kWave : 1) * kPhotoLdsStride];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.order[gid];
  const lk_result rec = a.rec[s];
  const bool good = reseed_good(rec, P, a.chi_max);
  // the sector at level L, as lk_uncertainty_kernel sees it
  const int4 rc = a.rect[s];
  const uint32_t off = a.off[s];
  const gptr<uint8_t> und = (gptr<uint8_t>)a.und, def = (gptr<uint8_t>)a.def;
  const gptr<f32x2> xy = (gptr<f32x2>)(a.xy + off);
  const int rw = rc.z;
  const int n = rw > 0 ? rc.w : (int)(a.off[s + 1] - off);
  const float inv_w = rw > 0 ? 1.f / (float)rw : 0.f;
  const float2 c0 = a.center[s];
  const float inv = 1.f / (float)(1 << a.level);
  const float cx = a.level == 0 ? c0.x : c0.x * inv, cy = a.level == 0 ? c0.y : c0.y * inv;
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
    p[i] = i < P ? rec.resultingParameters[i] : 0.f;
  translate<P>(p, 0, a.level);
  double v[kLkPhotoSums];
#pragma unroll
  for (int i = 0; i < kLkPhotoSums; ++i)
    v[i] = 0.0;
  const int umaxr = a.urows - 1, umaxc = a.ucols - 1;
  for (int k = lane; k < (good ? n : 0); k += GROUP) { // (a record that is not good is not evaluated)
    f32x2 q;
    if (rw > 0) { // implicit rectangle, row by row
      int row = (int)((float)k * inv_w);
      int col = k - row * rw;
      if (col < 0) {
        col += rw;
        --row;
      } else if (col >= rw) {
        col -= rw;
        ++row;
      }
      q.x = (float)(rc.x + col);
      q.y = (float)(rc.y + row);
    } else {
      q = xy[k];
    }
    float xd, yd, dx = 0.f, dy = 0.f;
    Warp<MODEL>::apply(q.x, q.y, cx, cy, p, xd, yd, dx, dy);
    int uix = (int)(q.x + 0.5f), uiy = (int)(q.y + 0.5f); // the node the forward residual reads
    uix = min(max(uix, 0), umaxc);                          // (memory safety only; valid lists never clamp)
    uiy = min(max(uiy, 0), umaxr);
    const float f = (float)und[(size_t)uiy * (size_t)a.ucols + (size_t)uix];
    float g;
    if (!sample_def_value<INTERP>(def, a.drows, a.dcols, xd, yd, g)) {
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
  photo_reduce<GROUP>(v, lds);
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

template <int MODEL, int INTERP> hipError_t launch_photo_mi(const LkPhotometryArgs &a, int group, hipStream_t st) {
  const int per_block = group <= 64 ? 256 / group : 1;
  const int blocks = (a.n_sectors + per_block - 1) / per_block;
  if (blocks <= 0)
    return hipSuccess;
  if (group == 16)
    hipLaunchKernelGGL((lk_photometry_kernel<MODEL, INTERP, 16>), dim3(blocks), dim3(256), 0, st, a);
  else if (group == 64)
    hipLaunchKernelGGL((lk_photometry_kernel<MODEL, INTERP, 64>), dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((lk_photometry_kernel<MODEL, INTERP, 512>), dim3(blocks), dim3(512), 0, st, a);
  return hipGetLastError();
}

template <int MODEL> hipError_t launch_photo_m(const LkPhotometryArgs &a, int interp, int group, hipStream_t st) {
  switch (interp) {
  case LK_IM_NEAREST: return launch_photo_mi<MODEL, LK_IM_NEAREST>(a, group, st);
  case LK_IM_BILINEAR: return launch_photo_mi<MODEL, LK_IM_BILINEAR>(a, group, st);
  case LK_IM_BICUBIC: return launch_photo_mi<MODEL, LK_IM_BICUBIC>(a, group, st);
  default: return launch_photo_mi<MODEL, LK_IM_BICUBIC_SEPARABLE>(a, group, st);
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

// the cell coordinate of a level-0 position, as lk_track.hip's: the grid kernel's expression for a centre, clamped to
// [-2, n + 1]; -2 and n + 1 stand for everything more than a cell (>= radius) from every centre
__device__ inline int map_cell_coord(double v, double origin, double cell, int n) {
  const double q = floor((v - origin) / cell);
  return q >= (double)(n + 1) ? n + 1 : (q > -2.0 ? (int)q : -2);
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
  const int S = a.n_sectors;
  const int cx_lo = map_cell_coord((double)px0 * up, g.x0, g.cell, g.nx), cx_hi = map_cell_coord((double)px1 * up, g.x0, g.cell, g.nx);
  const int cy_lo = map_cell_coord((double)py0 * up, g.y0, g.cell, g.ny), cy_hi = map_cell_coord((double)py1 * up, g.y0, g.cell, g.ny);
  const int x_lo = cx_lo > 0 ? cx_lo - 1 : 0, x_hi = cx_hi + 1 < g.nx ? cx_hi + 1 : g.nx - 1;
  const int y_lo = cy_lo > 0 ? cy_lo - 1 : 0, y_hi = cy_hi + 1 < g.ny ? cy_hi + 1 : g.ny - 1;
  long long total = 0;
  if (x_lo <= x_hi)
    for (int yy = y_lo; yy <= y_hi; ++yy) {
      const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_lo];
      uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_hi + 1];
      e = e < (uint32_t)S ? e : (uint32_t)S;
      total += e > b ? (long long)(e - b) : 0;
    }
  const bool staged = total <= (long long)kLkMapCapacity;
  if (staged) {
    int base = 0;
    if (x_lo <= x_hi)
      for (int yy = y_lo; yy <= y_hi; ++yy) {
        const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_lo];
        uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)x_hi + 1];
        e = e < (uint32_t)S ? e : (uint32_t)S;
        for (uint32_t k = b + (uint32_t)tid; k < e; k += kBlock) {
          const uint32_t m = g.members[k];
          const int at = base + (int)(k - b); // < total <= kLkMapCapacity
          const bool known = m < (uint32_t)S;
          s_idx[at] = known ? (int)m : 0;
          s_cx[at] = known ? a.pack[m].cx0 : __uint_as_float(0x7fc00000u);
          s_cy[at] = known ? a.pack[m].cy0 : 0.f;
        }
        base += e > b ? (int)(e - b) : 0;
      }
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
    const int ix = map_cell_coord(X, g.x0, g.cell, g.nx), iy = map_cell_coord(Y, g.y0, g.cell, g.ny);
    const int qx_lo = ix > 0 ? ix - 1 : 0, qx_hi = ix + 1 < g.nx ? ix + 1 : g.nx - 1;
    const int qy_lo = iy > 0 ? iy - 1 : 0, qy_hi = iy + 1 < g.ny ? iy + 1 : g.ny - 1;
    if (qx_lo <= qx_hi)
      for (int yy = qy_lo; yy <= qy_hi; ++yy) {
        const uint32_t b = g.start[(size_t)yy * (size_t)g.nx + (size_t)qx_lo];
        uint32_t e = g.start[(size_t)yy * (size_t)g.nx + (size_t)qx_hi + 1];
        e = e < (uint32_t)S ? e : (uint32_t)S;
        for (uint32_t k = b; k < e; ++k) {
          const uint32_t m = g.members[k];
          if (m >= (uint32_t)S)
            continue;
          const double d2 = lk_map_d2(a.pack[m].cx0, a.pack[m].cy0, X, Y);
          if (d2 <= a.r2 && lk_map_better(d2, (int)m, best_d2, best)) {
            best = (int)m;
            best_d2 = d2;
          }
        }
      }
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

template <int MODEL> hipError_t launch_map_m(const LkResidualMapArgs &a, int interp, unsigned tiles, hipStream_t st) {
  const dim3 grid(tiles), block(kBlock);
  switch (interp) {
  case LK_IM_NEAREST: hipLaunchKernelGGL((lk_residual_map_kernel<MODEL, LK_IM_NEAREST>), grid, block, 0, st, a); break;
  case LK_IM_BILINEAR: hipLaunchKernelGGL((lk_residual_map_kernel<MODEL, LK_IM_BILINEAR>), grid, block, 0, st, a); break;
  case LK_IM_BICUBIC: hipLaunchKernelGGL((lk_residual_map_kernel<MODEL, LK_IM_BICUBIC>), grid, block, 0, st, a); break;
  default: hipLaunchKernelGGL((lk_residual_map_kernel<MODEL, LK_IM_BICUBIC_SEPARABLE>), grid, block, 0, st, a); break;
  }
  return hipGetLastError();
}

} // namespace

hipError_t lk_launch_photometry(const LkPhotometryArgs &a, int model, int interp, int group, hipStream_t st) {
  switch (model) {
  case LK_FM_U: return launch_photo_m<LK_FM_U>(a, interp, group, st);
  case LK_FM_UV: return launch_photo_m<LK_FM_UV>(a, interp, group, st);
  case LK_FM_UVQ: return launch_photo_m<LK_FM_UVQ>(a, interp, group, st);
  default: return launch_photo_m<LK_FM_UVUXUYVXVY>(a, interp, group, st);
  }
}

hipError_t lk_launch_map_prep(const lk_result *rec, const float2 *center, int n_sectors, int model, int level, float chi_max,
                              LkMapSector *pack, hipStream_t st) {
  if (n_sectors <= 0)
    return hipSuccess;
  const dim3 grid((unsigned)((n_sectors + kBlock - 1) / kBlock)), block(kBlock);
  switch (model) {
  case LK_FM_U: hipLaunchKernelGGL(lk_map_prep_kernel<LK_FM_U>, grid, block, 0, st, rec, center, n_sectors, level, chi_max, pack); break;
  case LK_FM_UV: hipLaunchKernelGGL(lk_map_prep_kernel<LK_FM_UV>, grid, block, 0, st, rec, center, n_sectors, level, chi_max, pack); break;
  case LK_FM_UVQ: hipLaunchKernelGGL(lk_map_prep_kernel<LK_FM_UVQ>, grid, block, 0, st, rec, center, n_sectors, level, chi_max, pack); break;
  default:
    hipLaunchKernelGGL(lk_map_prep_kernel<LK_FM_UVUXUYVXVY>, grid, block, 0, st, rec, center, n_sectors, level, chi_max, pack);
    break;
  }
  return hipGetLastError();
}

hipError_t lk_launch_residual_map(const LkResidualMapArgs &a, int model, int interp, int *n_tiles, hipStream_t st) {
  if (a.n_sectors <= 0 || a.w <= 0 || a.h <= 0 || a.tiles_x != (a.w + kLkMapTileW - 1) / kLkMapTileW)
    return hipErrorInvalidValue;
  const long long tiles = (long long)a.tiles_x * (long long)((a.h + kLkMapTileH - 1) / kLkMapTileH);
  if (tiles > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (n_tiles)
    *n_tiles = (int)tiles;
  switch (model) {
  case LK_FM_U: return launch_map_m<LK_FM_U>(a, interp, (unsigned)tiles, st);
  case LK_FM_UV: return launch_map_m<LK_FM_UV>(a, interp, (unsigned)tiles, st);
  case LK_FM_UVQ: return launch_map_m<LK_FM_UVQ>(a, interp, (unsigned)tiles, st);
  default: return launch_map_m<LK_FM_UVUXUYVXVY>(a, interp, (unsigned)tiles, st);
  }
}
