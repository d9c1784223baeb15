// The implicit-rectangle walk of the lane-group sample loop (csrc/lk_rect_walk.hpp) against the floor division it replaces:
// for every width, stride, first lane and sample count of the grid below, the loop of evaluate<> is run on the host and
// (row, col) of every visited k compared with (k / rw, k % rw).  Stand-alone (tests/test_rect_walk_host.py builds it plain
// and under ASan + UBSan).
#include <cstdio>
#include <initializer_list>

#include "lk_rect_walk.hpp"

int main() {
  const int strides[] = {16, 32, 64, 512, 4096};
  long long visited = 0, walks = 0;
  for (int rw = 1; rw <= 70; ++rw) {
    const int counts[] = {0, 1, rw, rw * rw, 361, 4999}; // 4999: a prime, so the last row is partial for every rw > 1
    for (int stride : strides) {
      // the lanes of a wavefront, and the last lane of a group wider than one (workgroups, teams)
      for (int lane0 = 0; lane0 < stride; lane0 = (lane0 == 63 && stride > 64) ? stride - 1 : lane0 + 1) {
        for (int n : counts) {
          RectWalk w = RectWalk::start(rw, lane0, stride);
          if (w.drow != stride / rw || w.dcol != stride % rw) {
            std::printf("step: rw %d stride %d: (%d, %d)\n", rw, stride, w.drow, w.dcol);
            return 1;
          }
          ++walks;
          for (int k = lane0; k < n; k += stride, w.step(rw)) {
            if (w.row != k / rw || w.col != k % rw) {
              std::printf("rw %d stride %d lane0 %d n %d k %d: (%d, %d), expected (%d, %d)\n", rw, stride, lane0, n, k, w.row,
                          w.col, k / rw, k % rw);
              return 1;
            }
            ++visited;
          }
        }
      }
    }
  }
  // the operands' bound: the division of start() is exact for every lane0, stride < 2^21
  for (int rw : {1, 2, 3, 7, 19, 33, 70, 4093, 2097151})
    for (int a : {0, 1, 18, 19, 20, 4095, 131071, 131072, 2097150, 2097151}) {
      const RectWalk w = RectWalk::start(rw, a, a > 0 ? a : 1);
      if (w.row != a / rw || w.col != a % rw || (a > 0 && (w.drow != a / rw || w.dcol != a % rw))) {
        std::printf("start: rw %d a %d: (%d, %d) (%d, %d)\n", rw, a, w.row, w.col, w.drow, w.dcol);
        return 1;
      }
    }
  // an explicit list (rw == 0) carries a walk that nothing reads: it must stay defined however long the list is
  RectWalk l = RectWalk::start(0, 63, 64);
  for (int trip = 0; trip < 40000000; ++trip)
    l.step(0);
  if (l.col != 0 || l.row != 63 + 40000000) {
    std::printf("list walk: (%d, %d)\n", l.row, l.col);
    return 1;
  }
  std::printf("rect_walk ok: %lld walks, %lld samples\n", walks, visited);
  return 0;
}
