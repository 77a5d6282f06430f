// iamf_render_fanout.hip — render_fanout_kernel<M, K, false> (render_fanout.hpp), the f32-fed form: one element rendered
// into K = 2..4 member batches of one or two output channels each with ONE pass over the input, in a translation unit of
// its own (compiled beside iamf_render.hip and iamf_render_fanout_lp.hip, which instantiates the packet-fed form;
// render_fast_kernel is not instantiated here and its code generation does not move).
// M: ambisonics of order 1..3 (4, 9, 16 channels) and 5.1 / 7.1 / 7.1.4 (6, 8, 12).  Entry: iamf_hip_batch_render_fanout
// (iamf_render.hip), which renders every member this kernel does not take exactly as iamf_hip_batch_render does.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <atomic>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/iamf_hip.h"
#include "render_entry.hpp"

namespace {

#include "render_common.hpp"
#include "render_downmix.hpp"
#include "render_fir.hpp"
#include "render_fir16.hpp"
#include "render_fir_fft.hpp"
#include "render_fast.hpp"
#include "render_fanout.hpp"

// LDS per workgroup: 55.9 / 81.7 / 107.6 KB for K = 2 / 3 / 4 at M = 16 — two, two, one workgroup per CU of 160 KiB
static_assert(2 * sizeof(float) * fan_lds_floats(3, 16) <= 160 * 1024, "K = 2 and 3: two workgroups per CU");
static_assert(sizeof(float) * fan_lds_floats(kFanMax, 16) <= 160 * 1024, "K = 4 fits a CU");

static_assert(FanK::has(2) && FanK::has(kFanMax) && !FanK::has(kFanMax + 1), "FanK is 2..kFanMax");

template <int M, int K>
void launch_fan_mk(const FanParams &p, hipStream_t st) {
  constexpr size_t lds = sizeof(float) * (size_t)fan_lds_floats(K, M);
  launch_big_lds<&render_fanout_kernel<M, K, false>, (int)lds>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

}  // namespace

int iamf_hip_fanout_launch(const void *params, int m, int k, hipStream_t st) {
  FanParams p;
  memcpy(&p, params, sizeof(p));
  for (int j = 0; j < k && j < kFanMax; ++j)
    if (p.mem[j].out_ch < 1 || p.mem[j].out_ch > 2) return 0;
  return dispatch(FanM{}, m, [&](auto M) {
    return dispatch(FanK{}, k, [&](auto K) { launch_fan_mk<M.value, K.value>(p, st); });
  });
}
