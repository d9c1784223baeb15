// lk_noise.hpp - the integer arithmetic that the kernels of the camera-noise pass (lk_noise.hip) share with the host
// (lk_noise.cpp; include/lk_engine.h: lk_camera_noise, lk_sector_noise).  Everything the GPU produces is an integer, so the
// definitions here are all there is to agree on: a pixel's q and bin from its K values, the node of a sector's sample, and
// the shape of the frame kernel's work.  The records are formed from the tables by the host alone (lk_noise.cpp).
//
// Per counted pixel with its K values x_f (u8): s1 = sum x_f <= 255 K, s2 = sum x_f^2, q = K s2 - s1^2 = K sum (x_f - mean)^2
// <= K^2 255^2 / 4 < 2^25 for K <= 16, and the bin g = (2 s1 + K) / (2 K), the rounded temporal mean.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lk_engine.h"

constexpr int kLkNoiseBins = 256;
constexpr int kLkNoiseSums = 3;     // per sector: n, sum q, sum s1
constexpr int kLkNoiseRun = 16;     // frame kernel: consecutive pixels of a row per lane, one aligned 16-byte load per frame
// frame kernel: a workgroup of 16 wavefronts and at most one workgroup per compute unit.  Every workgroup flushes up to 512
// atomics into the same 4 KiB, and atomics on so few lines run an order of magnitude below the spread rate: with 1024
// workgroups of 256 threads the flush alone took about 30 us on 2048 x 2048 speckle frames (profiles/noise_bench.txt has the
// run after the change).
constexpr int kLkNoiseThreads = 1024;
constexpr int kLkNoiseMaxBlocks = 256;
static_assert(kLkNoiseThreads >= kLkNoiseBins, "the flush is a bin per thread");
static_assert(LK_NOISE_MAX_FRAMES * LK_NOISE_MAX_FRAMES * 255ull * 255ull / 4 < (1ull << 25), "q fits 25 bits");
static_assert((LK_NOISE_MAX_FRAMES * LK_NOISE_MAX_FRAMES * 255ull * 255ull / 4) * kLkNoiseRun < (1ull << 32), "a lane's run of q fits 32 bits");

// The division by 2 K as a multiplication: for n = 2 s1 + K <= 511 K and d = 2 K <= 32, n / d = (n m) >> 19 with
// m = 2^19 / d + 1, because n (m d - 2^19) <= n d < 2^19 and n m < 2^32 (checked for every K and s1 below).
constexpr int kLkNoiseShift = 19;
__host__ __device__ constexpr uint32_t lk_noise_magic(int K) { return (1u << kLkNoiseShift) / (2u * (uint32_t)K) + 1u; }
__host__ __device__ constexpr uint32_t lk_noise_bin(uint32_t s1, uint32_t K, uint32_t magic) { return ((2u * s1 + K) * magic) >> kLkNoiseShift; }
__host__ __device__ constexpr uint32_t lk_noise_q(uint32_t s1, uint32_t s2, uint32_t K) { return K * s2 - s1 * s1; }
constexpr bool lk_noise_magic_holds(int K) {
  for (uint32_t s1 = 0; s1 <= 255u * (uint32_t)K; ++s1)
    if (lk_noise_bin(s1, (uint32_t)K, lk_noise_magic(K)) != (2u * s1 + (uint32_t)K) / (2u * (uint32_t)K))
      return false;
  return true;
}
static_assert(lk_noise_magic_holds(2) && lk_noise_magic_holds(3) && lk_noise_magic_holds(4) && lk_noise_magic_holds(5) &&
                  lk_noise_magic_holds(6) && lk_noise_magic_holds(7) && lk_noise_magic_holds(8) && lk_noise_magic_holds(9) &&
                  lk_noise_magic_holds(10) && lk_noise_magic_holds(11) && lk_noise_magic_holds(12) && lk_noise_magic_holds(13) &&
                  lk_noise_magic_holds(14) && lk_noise_magic_holds(15) && lk_noise_magic_holds(16),
              "the multiplication is the division for every K and every s1");

// the node of a sample along one axis of `size` pixels: (int)(q + 0.5f), the node sector_und_node reads, for 0 <= q + 0.5f <
// size, else -1: outside (a position that is not finite included; -1 + 0.5f would truncate to node 0, but the sample lies
// beyond the border); compared on the float, so that no conversion overflows
__host__ __device__ inline int lk_noise_node(float q, int size) {
  const float f = q + 0.5f;
  return f >= 0.f && f < (float)size ? (int)f : -1;
}

// The frame kernel's work: row y of the region begins at byte o = (y0 + y) cols + x0 of every frame (all bases are 16-byte
// aligned); its units are the aligned 16-byte pieces that overlap the row's w pixels, unit k = the region columns
// 16 k - (o & 15) .. + 15 cut to 0 .. w - 1.  At most (w + 30) / 16 of them overlap; a unit beyond the row is empty.
__host__ __device__ constexpr int lk_noise_units_per_row(int w) { return (w + 2 * (kLkNoiseRun - 1)) / kLkNoiseRun; }
