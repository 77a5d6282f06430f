// resample_route.hpp — which resampler kernels are instantiated (iamf_resample.hip) and what rs_run's launchers ask of a
// call before they take it.  Plain C++, included inside the unit's namespace behind <type_traits>: the launchers
// dispatch over these lists and the instance listing (iamf_route.hip) walks them.
#pragma once

#include "instance_lists.hpp"

// resample_block_kernel<C, R>: mono, stereo / binaural, 5.1 / 3.1.2, 7.1 / 5.1.2, ... ; R outputs of one phase per thread
using RsBlockC = Ints<1, 2, 6, 8, 10, 12, 14, 24>;
using RsBlockR = Ints<4, 2, 1>;
// the largest R for a channel count: 4 R C accumulators per thread in interpolated mode
constexpr int rs_block_r(int c) { return c <= 2 ? 4 : (c <= 8 ? 2 : 1); }

// resample_direct_kernel<C, N, NUMP, R>: filter lengths of quality 4 — 64 (up-sampling), 96 (3:2), 128 (2:1), 192 (3:1) —
// with the planes of a whole-ratio down-sampling; R = rs_direct_r(C) outputs a thread works on at once
constexpr int rs_np(int n, int nump) { return n * 4 + nump; }
constexpr int rs_np_n(int v) { return v / 4; }
constexpr int rs_np_p(int v) { return v % 4; }
using RsDirectC = Ints<1, 2, 6, 8, 10, 12>;
using RsDirectNP = Ints<rs_np(64, 1), rs_np(96, 1), rs_np(128, 2), rs_np(192, 3)>;
constexpr int rs_direct_r(int c) { return c <= 2 ? 4 : (c <= 8 ? 2 : 1); }
// the launcher's rule on top of the lists.  192 taps + accumulators: two waves per SIMD; 1, 2 and 8 channels measured 0.8
// of the tiled kernel, which takes them instead (their instances exist but no call reaches them)
constexpr bool rs_direct_takes(int c, int n) { return n != 192 || c == 6 || c >= 10; }

// f(family, variant, m, c, k) as for_each_render_instance (render_route.hpp), for the resampler's kernels
template <class F>
void for_each_resample_instance(F &&f) {
  f(IAMF_HIP_ROUTE_RS_PLAIN, 0, 0, 0, 0);
  f(IAMF_HIP_ROUTE_RS_TILE, 0, 0, 0, 0);   // interpolated mode
  f(IAMF_HIP_ROUTE_RS_TILE, 1, 0, 0, 0);   // direct mode
  for_each_int(RsBlockC{}, [&](int c) {
    for_each_int(RsBlockR{}, [&](int r) {
      if (r <= rs_block_r(c)) f(IAMF_HIP_ROUTE_RS_BLOCK, 0, 0, c, r);
    });
  });
  for_each_int(RsDirectC{}, [&](int c) {
    for_each_int(RsDirectNP{}, [&](int v) { f(IAMF_HIP_ROUTE_RS_DIRECT, rs_np_p(v), rs_np_n(v), c, rs_direct_r(c)); });
  });
}
