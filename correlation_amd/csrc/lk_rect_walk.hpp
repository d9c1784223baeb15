// lk_rect_walk.hpp - the samples of an implicit rectangle as one lane of a lane group meets them.  A lane visits the
// row-major sample indices k = lane0, lane0 + stride, lane0 + 2 stride, ...; (row, col) = (k / rw, k % rw) of those indices
// advance by the constant (stride / rw, stride % rw) with at most one carry, so the floor division is done once per
// evaluation (RectWalk::start) and a trip of the sample loop costs two adds, a compare, a select and an add-with-carry
// (RectWalk::step) - no division, no conversion, no divergent block.  The integers are the ones the division gives
// (tests/test_rect_walk_host.py compares them for every k), so every float operation downstream sees the same operands.
// Plain C++ on the host, __host__ __device__ under hipcc.
#pragma once

#if defined(__HIPCC__)
#define LK_WALK_HD __host__ __device__ __forceinline__
#else
#define LK_WALK_HD inline
#endif

struct RectWalk {
  int row, col;   // of the lane's current sample
  int drow, dcol; // what one trip adds: stride / rw, stride % rw (dcol < rw: one conditional subtraction is enough)

  // a / w and a % w for 0 <= a < 2^21, 1 <= w, inv within a few ulps of 1 / w: the truncated product is off by at most one
  // either way (|a * inv - a / w| <= a / w * 2^-21 < 1), which the two selects put right.  Exact whatever the reciprocal's
  // last bits are, so the host's divide and the device's v_rcp_f32 give the same integers.
  static LK_WALK_HD void divmod(int a, int w, float inv, int &quot, int &rem) {
    int q = (int)((float)a * inv);
    int r = a - q * w;
    const int low = r < 0 ? 1 : 0, high = r >= w ? 1 : 0;
    quot = q - low + high;
    rem = r + (low ? w : 0) - (high ? w : 0);
  }

  // rw: width of the rectangle (rw <= 0, an explicit list: a walk that is never read and never overflows);
  // 0 <= lane0, 0 < stride, both below 2^21 (the widest group, a team of 256 workgroups, has 2^17 lanes)
  static LK_WALK_HD RectWalk start(int rw, int lane0, int stride) {
    const int w = rw > 0 ? rw : 1;
#if defined(__HIP_DEVICE_COMPILE__)
    const float inv = __builtin_amdgcn_rcpf((float)w);
#else
    const float inv = 1.f / (float)w;
#endif
    RectWalk k;
    divmod(lane0, w, inv, k.row, k.col);
    divmod(stride, w, inv, k.drow, k.dcol);
    k.drow = rw > 0 ? k.drow : 0;
    return k;
  }

  // the next sample of the lane: k += stride
  LK_WALK_HD void step(int rw) {
    col += dcol;
    row += drow;
    const bool carry = col >= rw;
    col = carry ? col - rw : col;
    row += carry ? 1 : 0;
  }
};
