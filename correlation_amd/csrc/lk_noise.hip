// lk_noise.hip - device side of the camera-noise pass (include/lk_engine.h: lk_camera_noise, lk_sector_noise; DESIGN.md
// section 30).  Both kernels read the u8 pixels of K static frames at level L = py_start and write integers only; the
// definitions of q and of the bin are in lk_noise.hpp, the records are formed on the host (lk_noise.cpp).
//
// frames      one launch over the region.  A row of the region is cut at the 16-byte boundaries of its address (the frames
//             share one geometry and every base is 16-byte aligned, so the cut is the same in all of them); a lane takes
//             one such unit: one aligned 16-byte load per frame for a unit inside the row, byte loads of the pixels inside
//             for the cut units at a row's head and tail.  s1 and s2 of the 16 pixels stay in registers over the frames.
//             Each workgroup keeps a 256-bin table in LDS, a 32-bit count (a workgroup sees far fewer than 2^32 pixels)
//             and a 64-bit sum of q.  A lane merges neighbouring pixels of one bin before it touches the table (16 q fit 32
//             bits), and a wavefront whose lanes all end in the same bin adds once: a flat frame, the worst case for the
//             table, costs two LDS atomics per wavefront and unit.  A frame's pixel sum is reduced over the wavefront per
//             unit, added to LDS by one lane, and leaves the workgroup in one atomic per frame.  The workgroup flushes its
//             non-empty bins with 64-bit integer atomics.  Every sum across lanes, wavefronts and workgroups is an integer
//             sum: the tables are the same bytes for any grid and any order.
// sectors     lk_pattern.hip's walk: one lane group per sector (16 / 64 / 512 lanes from the level-0 sample count), lane j
//             takes the samples j, j + G, ...; a sample whose node lies outside the frame is skipped.  n, sum q and sum s1
//             are reduced as integers over the group (reduce_i64, the order of reduce_f64).
#include "lk_device.hpp"
#include "lk_launch.hpp"
#include "lk_neighbours.hpp"
#include "lk_noise.hpp"
#include "lk_sector_eval.hpp"

namespace {

// ---- the group reduction on integers -----------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ long long dpp_get_i64(long long v) {
  const unsigned long long u = (unsigned long long)v;
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
}
__device__ __forceinline__ long long readlane_i64(long long v, int lane) {
  const unsigned long long u = (unsigned long long)v;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), lane);
  return (long long)(((unsigned long long)hi << 32) | (unsigned long long)lo);
}

// v[0 .. N) summed over the group by the stages of reduce_f64 (lk_sector_eval.hpp); every lane ends with the sums.  GROUP
// <= 64 uses no barrier; GROUP == 512 is the whole (uniform) workgroup, which calls this once.  lds: (GROUP / 64) * N words
// when GROUP > 64, else unused.
template <int GROUP, int N> __device__ __forceinline__ void reduce_i64(long long (&v)[N], long long *lds) {
  auto stage = [&](auto ctrl) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      v[i] += dpp_get_i64<decltype(ctrl)::value>(v[i]);
  };
  stage(std::integral_constant<int, 0xB1>{});  // quad_perm [1,0,3,2]
  stage(std::integral_constant<int, 0x4E>{});  // quad_perm [2,3,0,1]
  stage(std::integral_constant<int, 0x141>{}); // row_half_mirror
  stage(std::integral_constant<int, 0x140>{}); // row_mirror
  if constexpr (GROUP >= 64) {
#pragma unroll
    for (int i = 0; i < N; ++i)
      v[i] = (readlane_i64(v[i], 0) + readlane_i64(v[i], 16)) + (readlane_i64(v[i], 32) + readlane_i64(v[i], 48));
  }
  if constexpr (GROUP > 64) {
    constexpr int WAVES = GROUP / kWave;
    const int wave = (int)threadIdx.x / kWave;
    if ((int)threadIdx.x % kWave == 0) {
#pragma unroll
      for (int i = 0; i < N; ++i)
        lds[wave * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
      long long t = lds[i];
      for (int w = 1; w < WAVES; ++w)
        t += lds[w * N + i];
      v[i] = t;
    }
  }
}

// ---- frames ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void table_add(unsigned int *count, unsigned long long *sum_q, uint32_t g, uint32_t n, unsigned long long q) {
  atomicAdd(&count[g], n);
  if (q)
    atomicAdd(&sum_q[g], q);
}

// bytes lo .. hi - 1 of the aligned 16-byte piece at p, the others 0
__device__ __forceinline__ void load_unit(gptr<uint8_t> p, bool whole, uint32_t bits, uint32_t (&w)[4]) {
  if (whole) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = *(gptr<u32x4>)p;
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int i = 0; i < kLkNoiseRun; ++i)
      if (bits >> i & 1u)
        w[i / 4] |= (uint32_t)p[i] << (8 * (i % 4));
  }
}

__global__ void __launch_bounds__(kLkNoiseThreads) lk_noise_frames_kernel(LkNoiseFrameArgs a) {
  __shared__ unsigned int lds_count[kLkNoiseBins];
  __shared__ unsigned long long lds_q[kLkNoiseBins];
  __shared__ unsigned long long lds_frame[LK_NOISE_MAX_FRAMES];
  const int tid = (int)threadIdx.x, lane = tid % kWave;
  if (tid < kLkNoiseBins) {
    lds_count[tid] = 0;
    lds_q[tid] = 0;
  }
  if (tid < LK_NOISE_MAX_FRAMES)
    lds_frame[tid] = 0;
  __syncthreads();
  const uint32_t K = (uint32_t)a.n_frames, magic = lk_noise_magic(a.n_frames);
  const uint32_t per_row = (uint32_t)lk_noise_units_per_row(a.w);
  const uint32_t total = (uint32_t)a.h * per_row; // (below 2^32: the launcher checks)
  const uint32_t tiles = (total + kLkNoiseThreads - 1) / kLkNoiseThreads;
  for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) { // (uniform over the workgroup: no lane leaves early)
    const uint32_t u = tile * kLkNoiseThreads + (uint32_t)tid;
    uint32_t bits = 0; // the pixels of the unit that count: bit i = byte i of the piece at `at`
    size_t at = 0;
    if (u < total) {
      const uint32_t y = u / per_row, k = u - y * per_row;
      const size_t o = (size_t)(a.y0 + (int)y) * (size_t)a.cols + (size_t)a.x0;
      const int c0 = (int)k * kLkNoiseRun - (int)(o & (kLkNoiseRun - 1)); // the region column of the piece's byte 0
      const int lo = c0 < 0 ? -c0 : 0, hi = min(kLkNoiseRun, a.w - c0);
      if (hi > lo) {
        bits = (hi == kLkNoiseRun ? 0xFFFFu : (1u << hi) - 1u) & ~((1u << lo) - 1u);
        at = (size_t)((long long)o + (long long)c0);
      }
    }
    const bool whole = bits == 0xFFFFu;
    if (a.mask && bits) {
      uint32_t m[4];
      load_unit((gptr<uint8_t>)a.mask + at, whole, bits, m);
#pragma unroll
      for (int i = 0; i < kLkNoiseRun; ++i)
        if (((m[i / 4] >> (8 * (i % 4))) & 255u) == 0)
          bits &= ~(1u << i);
    }
    uint32_t keep[4]; // 0xFF in the bytes that count
#pragma unroll
    for (int j = 0; j < 4; ++j)
      keep[j] = ((bits >> (4 * j) & 1u) ? 0xFFu : 0u) | ((bits >> (4 * j + 1) & 1u) ? 0xFF00u : 0u) |
                ((bits >> (4 * j + 2) & 1u) ? 0xFF0000u : 0u) | ((bits >> (4 * j + 3) & 1u) ? 0xFF000000u : 0u);
    uint32_t s1[kLkNoiseRun], s2[kLkNoiseRun];
#pragma unroll
    for (int i = 0; i < kLkNoiseRun; ++i)
      s1[i] = s2[i] = 0;
    for (uint32_t f = 0; f < K; ++f) {
      uint32_t w[4] = {0, 0, 0, 0};
      if (bits)
        load_unit((gptr<uint8_t>)a.frame[f] + at, whole, bits, w);
      uint32_t sum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        w[j] &= keep[j];
        sum = __builtin_amdgcn_sad_u8(w[j], 0u, sum); // the four bytes added
      }
#pragma unroll
      for (int i = 0; i < kLkNoiseRun; ++i) {
        const uint32_t b = (w[i / 4] >> (8 * (i % 4))) & 255u;
        s1[i] += b;
        s2[i] += b * b;
      }
      long long fs[1] = {(long long)sum};
      reduce_i64<kWave, 1>(fs, nullptr);
      if (lane == 0 && fs[0])
        atomicAdd(&lds_frame[f], (unsigned long long)fs[0]);
    }
    // the table: neighbouring pixels of one bin are merged in the lane first
    uint32_t cur = 0, n = 0, q = 0;
#pragma unroll
    for (int i = 0; i < kLkNoiseRun; ++i) {
      if (bits >> i & 1u) {
        const uint32_t g = lk_noise_bin(s1[i], K, magic);
        if (n && g != cur) {
          table_add(lds_count, lds_q, cur, n, q);
          n = q = 0;
        }
        cur = g;
        ++n;
        q += lk_noise_q(s1[i], s2[i], K);
      }
    }
    const unsigned long long active = __ballot(n != 0);
    if (active) { // (uniform over the wavefront)
      const uint32_t ref = (uint32_t)__builtin_amdgcn_readlane((int)cur, __ffsll((long long)active) - 1);
      if (__ballot(n != 0 && cur != ref) == 0) { // every lane that holds pixels holds them for one bin: one add
        long long v[2] = {(long long)n, (long long)q};
        reduce_i64<kWave, 2>(v, nullptr);
        if (lane == 0)
          table_add(lds_count, lds_q, ref, (uint32_t)v[0], (unsigned long long)v[1]);
      } else if (n) {
        table_add(lds_count, lds_q, cur, n, q);
      }
    }
  }
  __syncthreads();
  const unsigned int count = tid < kLkNoiseBins ? lds_count[tid] : 0u;
  if (count) {
    atomicAdd(&a.bins[2 * tid], (unsigned long long)count);
    const unsigned long long sum_q = lds_q[tid];
    if (sum_q)
      atomicAdd(&a.bins[2 * tid + 1], sum_q);
  }
  if (tid < a.n_frames && lds_frame[tid])
    atomicAdd(&a.frame_sums[tid], lds_frame[tid]);
}

// ---- sectors -----------------------------------------------------------------------------------------------------------------
template <int GROUP> __global__ void __launch_bounds__(GROUP <= 64 ? 256 : GROUP) lk_noise_sectors_kernel(LkNoiseSectorArgs a) {
  constexpr int THREADS = GROUP <= 64 ? 256 : GROUP;
  __shared__ long long lds[(GROUP > 64 ? GROUP / kWave : 1) * kLkNoiseSums];
  const int gid = (int)blockIdx.x * (THREADS / GROUP) + (int)threadIdx.x / GROUP;
  const int lane = (int)threadIdx.x % GROUP;
  if (gid >= a.n_sectors) // (GROUP == 512: the whole workgroup; GROUP <= 64: whole rows / wavefronts, no barriers below)
    return;
  const int s = (int)a.ev.order[gid];
  const SectorLevel c = sector_level(a.ev, s, a.level, a.ev.center[s]);
  const uint32_t K = (uint32_t)a.n_frames;
  long long v[kLkNoiseSums] = {0, 0, 0};
  for (int k = lane; k < c.n; k += GROUP) {
    const f32x2 p = sector_sample(c, k);
    const int x = lk_noise_node(p.x, c.ucols), y = lk_noise_node(p.y, c.urows);
    if (x < 0 || y < 0) // outside the frame: not counted
      continue;
    const size_t at = (size_t)y * (size_t)c.ucols + (size_t)x;
    uint32_t s1 = 0, s2 = 0;
    for (uint32_t f = 0; f < K; ++f) {
      const uint32_t b = (uint32_t)((gptr<uint8_t>)a.frame[f])[at];
      s1 += b;
      s2 += b * b;
    }
    v[0] += 1;
    v[1] += (long long)lk_noise_q(s1, s2, K);
    v[2] += (long long)s1;
  }
  reduce_i64<GROUP, kLkNoiseSums>(v, lds);
  if (lane != 0)
    return;
#pragma unroll
  for (int i = 0; i < kLkNoiseSums; ++i)
    a.sums[(size_t)s * kLkNoiseSums + i] = v[i];
}

bool aligned16(const void *p) { return ((uintptr_t)p & (uintptr_t)(kLkNoiseRun - 1)) == 0; }

} // namespace

hipError_t lk_launch_noise_frames(const LkNoiseFrameArgs &a, int *n_blocks, hipStream_t st) {
  if (a.n_frames < 2 || a.n_frames > LK_NOISE_MAX_FRAMES || a.w < 1 || a.h < 1 || a.x0 < 0 || a.y0 < 0 ||
      (long long)a.x0 + a.w > a.cols || (long long)a.y0 + a.h > a.rows || !a.bins || !a.frame_sums || !aligned16(a.mask))
    return hipErrorInvalidValue;
  for (int f = 0; f < a.n_frames; ++f)
    if (!a.frame[f] || !aligned16(a.frame[f]))
      return hipErrorInvalidValue;
  const unsigned long long units = (unsigned long long)a.h * (unsigned long long)lk_noise_units_per_row(a.w);
  if (units > 0xFFFFFF00ull) // (the kernel counts units and tiles in 32 bits)
    return hipErrorInvalidValue;
  const unsigned blocks = min(blocks_for((long long)units, kLkNoiseThreads), (unsigned)kLkNoiseMaxBlocks);
  if (n_blocks)
    *n_blocks = (int)blocks;
  hipLaunchKernelGGL(lk_noise_frames_kernel, dim3(blocks), dim3(kLkNoiseThreads), 0, st, a);
  return hipGetLastError();
}

hipError_t lk_launch_noise_sectors(const LkNoiseSectorArgs &a, int group, hipStream_t st) {
  if (a.n_frames < 2 || a.n_frames > LK_NOISE_MAX_FRAMES || !a.sums)
    return hipErrorInvalidValue;
  return dispatch_group(group, [&](auto g) {
    constexpr int G = decltype(g)::value;
    return launch_sector_groups<G>(lk_noise_sectors_kernel<G>, a, a.n_sectors, st);
  });
}
