// iamf_render_fanout.hip — render_fanout_kernel<M, K> (render_fanout.hpp): one element rendered into K = 2..4 member
// batches of one or two output channels each with ONE pass over the input, in a translation unit of its own (compiled
// beside iamf_render.hip; render_fast_kernel is not instantiated here and its code generation does not move).
// M: ambisonics of order 1..3 (4, 9, 16 channels) and 5.1 / 7.1 / 7.1.4 (6, 8, 12).  Entry: iamf_hip_batch_render_fanout
// (iamf_render.hip), which renders every member this kernel does not take exactly as iamf_hip_batch_render does.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <atomic>
#include <stdlib.h>
#include <string.h>

#include "../../include/iamf_hip.h"

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

template <int M, int K>
void launch_fan_mk(const FanParams &p, hipStream_t st) {
  constexpr size_t lds = sizeof(float) * (size_t)fan_lds_floats(K, M);
  // more than 64 KiB of dynamic LDS has to be opted into per kernel and device
  static OptIn opted;
  if (opted.begin()) {
    opted.set(reinterpret_cast<const void *>(&render_fanout_kernel<M, K>), (int)lds);
    opted.end();
  }
  hipLaunchKernelGGL((render_fanout_kernel<M, K>), dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

template <int M>
int launch_fan_m(const FanParams &p, int k, hipStream_t st) {
  switch (k) {
    case 2: launch_fan_mk<M, 2>(p, st); return 1;
    case 3: launch_fan_mk<M, 3>(p, st); return 1;
    case 4: launch_fan_mk<M, 4>(p, st); return 1;
    default: return 0;
  }
}

}  // namespace

extern "C" __attribute__((visibility("hidden"))) int iamf_hip_fanout_has(int m, int k) {
  return (m == 4 || m == 9 || m == 16 || m == 6 || m == 8 || m == 12) && k >= 2 && k <= kFanMax;
}

// returns 1 if launched; params: a FanParams whose first k members are set
extern "C" __attribute__((visibility("hidden"))) int iamf_hip_fanout_launch(const void *params, int m, int k, hipStream_t st) {
  FanParams p;
  memcpy(&p, params, sizeof(p));
  if (!iamf_hip_fanout_has(m, k)) return 0;
  for (int j = 0; j < k; ++j)
    if (p.mem[j].out_ch < 1 || p.mem[j].out_ch > 2) return 0;
  switch (m) {
    case 4: return launch_fan_m<4>(p, k, st);
    case 6: return launch_fan_m<6>(p, k, st);
    case 8: return launch_fan_m<8>(p, k, st);
    case 9: return launch_fan_m<9>(p, k, st);
    case 12: return launch_fan_m<12>(p, k, st);
    case 16: return launch_fan_m<16>(p, k, st);
    default: return 0;
  }
}
