// lk_spline.hip - the B-spline refinement pass (include/lk_engine.h: lk_refine_spline, lk_spline_coefficients,
// lk_spline_sample).
//
// Three parts.  The prefilter turns a level image into the float coefficients of its cubic or quintic B-spline: Unser's
// recursive filter with a mirror boundary along every row, then along every column.  A line is filtered by ONE lane from end
// to end in the order the header states, so its coefficients are the bytes of the sequential recursion whatever the launch
// shape; the lanes of a wavefront take neighbouring lines.  Along the columns that is coalesced by itself (lane = column).
// Along the rows a workgroup takes kSplTileRows rows and walks them in tiles of 64 columns through LDS: the wavefront loads
// a tile row by row (lane = column, 256 contiguous bytes), lane r then filters row r's 64 elements in LDS carrying its
// recursion state in registers from tile to tile - forward for the causal sweep, backward for the anticausal one - and the
// wavefront stores the tile as it loaded it.  The tile's row stride is 65 dwords, so the lanes of the filter step (bank
// (65 r + k) mod 32) and of the load step (consecutive dwords) meet no bank twice.
// The sampler (spline_sample and ZnSplineSampler, lk_sector_policies.hpp, where lk_composed.hip finds them too) evaluates
// the spline and its gradient separably, like LK_IM_BICUBIC_SEPARABLE.  The pass kernel is lk_znssd_loop.hpp with that sampler.
#include "lk_launch.hpp"
#include "lk_sector_policies.hpp" // spline_sample, ZnSplineSampler
#include "lk_spline.hpp"
#include "lk_znssd_loop.hpp"

namespace {

constexpr int kSplTileRows = 16, kSplTileCols = 64, kSplTileStride = kSplTileCols + 1;
constexpr int kSplChunk = 8; // elements a lane holds in registers at a time: their loads go out together, the recursion follows

// c[k] = s[k] + z c[k - 1] for n elements `stride` apart, c[-1] = last on entry; on return last = the final c and prev the
// one before it.  GAIN: s[k] = gain c[k], a rounded product (the first pole of the column step; the row step scales as it
// loads).
template <bool GAIN> __device__ __forceinline__ void spline_forward(float *c, size_t stride, int n, float z, float gain, float &prev, float &last) {
  int k = 0;
  for (; k + kSplChunk <= n; k += kSplChunk) {
    float v[kSplChunk];
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j)
      v[j] = c[(size_t)(k + j) * stride];
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j) {
      const float s = GAIN ? v[j] * gain : v[j];
      prev = last;
      last = s + z * last;
      v[j] = last;
    }
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j)
      c[(size_t)(k + j) * stride] = v[j];
  }
  for (; k < n; ++k) {
    const float s = GAIN ? c[(size_t)k * stride] * gain : c[(size_t)k * stride];
    prev = last;
    last = s + z * last;
    c[(size_t)k * stride] = last;
  }
}

// c[k] = z (c[k + 1] - c[k]) for k = n - 1 down to 0, c[n] = last on entry; on return last = c[0]
__device__ __forceinline__ void spline_backward(float *c, size_t stride, int n, float z, float &last) {
  int k = n;
  for (; k >= kSplChunk; k -= kSplChunk) {
    float v[kSplChunk];
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j)
      v[j] = c[(size_t)(k - 1 - j) * stride];
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j) {
      last = z * (last - v[j]);
      v[j] = last;
    }
#pragma unroll
    for (int j = 0; j < kSplChunk; ++j)
      c[(size_t)(k - 1 - j) * stride] = v[j];
  }
  for (; k > 0; --k) {
    last = z * (last - c[(size_t)(k - 1) * stride]);
    c[(size_t)(k - 1) * stride] = last;
  }
}

// the causal start of a line of n elements: s[0] + sum zp_k s[k], k = 1 .. min(n, 28) - 1 ascending, zp_1 = z, zp_(k + 1) = zp_k z
template <bool GAIN> __device__ __forceinline__ float spline_start(const float *c, size_t stride, int n, float z, float gain) {
  const int K = n < kLkSplineStart ? n : kLkSplineStart;
  float acc = GAIN ? c[0] * gain : c[0], zp = z;
  for (int k = 1; k < K; ++k) {
    const float s = GAIN ? c[(size_t)k * stride] * gain : c[(size_t)k * stride];
    acc = acc + zp * s;
    zp = zp * z;
  }
  return acc;
}

// the anticausal start from the last two elements of the causal sweep
__device__ __forceinline__ float spline_end(float z, float before_last, float last) { return (z / (z * z - 1.f)) * (z * before_last + last); }

// Rows [blockIdx.x * kSplTileRows, + kSplTileRows) of the image: gain and every pole along the row; coef = the result.
// 64 threads.  rows, cols >= 2.
template <int ORDER> __global__ void __launch_bounds__(64) lk_spline_rows_kernel(const uint8_t *img, int rows, int cols, float *coef) {
  using Z = LkSplinePoles<ORDER>;
  __shared__ float tile[kSplTileRows * kSplTileStride];
  const int lane = (int)threadIdx.x, row0 = (int)blockIdx.x * kSplTileRows;
  const int nr = rows - row0 < kSplTileRows ? rows - row0 : kSplTileRows; // (uniform over the workgroup, as every bound below)
  const int n_tiles = (cols + kSplTileCols - 1) / kSplTileCols;
  float *mine = tile + lane * kSplTileStride; // lane < nr: the row this lane filters
#pragma unroll
  for (int p = 0; p < Z::N; ++p) {
    const float z = Z::z(p);
    float prev = 0.f, last = 0.f;
    for (int t = 0; t < n_tiles; ++t) {
      const int c0 = t * kSplTileCols, w = cols - c0 < kSplTileCols ? cols - c0 : kSplTileCols;
      if (lane < w)
        for (int i = 0; i < nr; ++i) {
          const size_t at = (size_t)(row0 + i) * (size_t)cols + (size_t)(c0 + lane);
          tile[i * kSplTileStride + lane] = p == 0 ? (float)img[at] * Z::gain : coef[at];
        }
      __syncthreads();
      if (lane < nr) {
        int k = 0;
        if (t == 0) { // (28 <= 64: the start-up sum lies in the first tile)
          last = spline_start<false>(mine, 1, cols, z, 1.f);
          mine[0] = last;
          k = 1;
        }
        spline_forward<false>(mine + k, 1, w - k, z, 1.f, prev, last);
      }
      __syncthreads();
      if (lane < w) // (a lane reads here what it alone overwrites in the next load)
        for (int i = 0; i < nr; ++i)
          coef[(size_t)(row0 + i) * (size_t)cols + (size_t)(c0 + lane)] = tile[i * kSplTileStride + lane];
    }
    last = spline_end(z, prev, last);
    for (int t = n_tiles - 1; t >= 0; --t) {
      const int c0 = t * kSplTileCols, w = cols - c0 < kSplTileCols ? cols - c0 : kSplTileCols;
      if (lane < w) // (and reads back what it stored itself)
        for (int i = 0; i < nr; ++i)
          tile[i * kSplTileStride + lane] = coef[(size_t)(row0 + i) * (size_t)cols + (size_t)(c0 + lane)];
      __syncthreads();
      if (lane < nr) {
        int k = w;
        if (t == n_tiles - 1)
          mine[--k] = last;
        spline_backward(mine, 1, k, z, last);
      }
      __syncthreads();
      if (lane < w)
        for (int i = 0; i < nr; ++i)
          coef[(size_t)(row0 + i) * (size_t)cols + (size_t)(c0 + lane)] = tile[i * kSplTileStride + lane];
    }
  }
}

// Column blockIdx.x * 64 + lane of coef, in place: gain and every pole down the column.  rows >= 2.
template <int ORDER> __global__ void __launch_bounds__(64) lk_spline_cols_kernel(int rows, int cols, float *coef) {
  using Z = LkSplinePoles<ORDER>;
  const int x = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (x >= cols)
    return;
  float *c = coef + x;
  const size_t stride = (size_t)cols;
#pragma unroll
  for (int p = 0; p < Z::N; ++p) {
    const float z = Z::z(p);
    float prev = 0.f, last;
    if (p == 0) {
      last = spline_start<true>(c, stride, rows, z, Z::gain);
      c[0] = last;
      spline_forward<true>(c + stride, stride, rows - 1, z, Z::gain, prev, last);
    } else {
      last = spline_start<false>(c, stride, rows, z, 1.f);
      c[0] = last;
      spline_forward<false>(c + stride, stride, rows - 1, z, 1.f, prev, last);
    }
    last = spline_end(z, prev, last);
    c[(size_t)(rows - 1) * stride] = last;
    spline_backward(c, stride, rows - 1, z, last);
  }
}

template <int ORDER> __global__ void lk_spline_sample_kernel(const float *coef, int rows, int cols, const float2 *pts, int n, float4 *out) {
  const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (k >= n)
    return;
  float W = 0.f, Wx = 0.f, Wy = 0.f;
  const bool ok = spline_sample<ORDER>((gptr<float>)coef, rows, cols, pts[k].x, pts[k].y, W, Wx, Wy);
  out[k] = ok ? make_float4(W, Wx, Wy, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int MODEL, int ORDER, int GROUP>
__global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_spline_kernel(LkSplineArgs a) {
  lk_znssd_sector<MODEL, GROUP>(a.zn, ZnSplineSampler<ORDER>{(gptr<float>)a.coef}, LkZnUnitWeight{});
}

template <class F> hipError_t dispatch_order(int order, F &&f) {
  return order == 3 ? f(std::integral_constant<int, 3>{}) : f(std::integral_constant<int, 5>{});
}

} // namespace

hipError_t lk_launch_spline_build(int order, const uint8_t *img, int rows, int cols, float *coef, hipStream_t st) {
  if (rows < 2 || cols < 2)
    return hipErrorInvalidValue;
  return dispatch_order(order, [&](auto o) {
    constexpr int O = decltype(o)::value;
    hipLaunchKernelGGL(lk_spline_rows_kernel<O>, dim3((unsigned)((rows + kSplTileRows - 1) / kSplTileRows)), dim3(64), 0, st, img, rows, cols,
                       coef);
    hipLaunchKernelGGL(lk_spline_cols_kernel<O>, dim3((unsigned)((cols + 63) / 64)), dim3(64), 0, st, rows, cols, coef);
    return hipGetLastError();
  });
}

hipError_t lk_launch_spline_sample(int order, const float *coef, int rows, int cols, const float2 *pts, int n, float4 *out, hipStream_t st) {
  if (n <= 0)
    return hipSuccess;
  return dispatch_order(order, [&](auto o) {
    hipLaunchKernelGGL(lk_spline_sample_kernel<decltype(o)::value>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, coef, rows, cols, pts,
                       n, out);
    return hipGetLastError();
  });
}

hipError_t lk_launch_spline(const LkSplineArgs &a, int model, int order, int group, hipStream_t st) {
  return dispatch_model(model, [&](auto m) {
    return dispatch_order(order, [&](auto o) {
      return dispatch_group(group, [&](auto g) {
        constexpr int M = decltype(m)::value, O = decltype(o)::value, G = decltype(g)::value;
        return launch_sector_groups<G>(lk_spline_kernel<M, O, G>, a, a.zn.n_sectors, st);
      });
    });
  });
}
