// iamf_render_fanout_lp.hip — render_fanout_kernel<M, K, true> (render_fanout.hpp), the packet-fed form: one mono-coded
// ambisonics element, held as 16-bit LPCM packets, rendered into K = 2..4 member batches of one or two output channels each
// with ONE pass over the packets, in a translation unit of its own (compiled beside iamf_render_fanout.hip, which
// instantiates the f32-fed form, and iamf_render_lpcm.hip; render_fast_kernel is not instantiated here and its code
// generation does not move).
// M: ambisonics of order 1..3 (4, 9, 16 channels), the element sizes both the packet-fed kernel and the fan-out take.
// Entry: iamf_hip_batch_render_fanout_lpcm (iamf_render.hip), which renders every member this kernel does not take
// exactly as iamf_hip_batch_render_lpcm does.
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

// LDS per workgroup is the f32-fed form's (fan_lds_floats): two, two, one workgroup per CU for K = 2 / 3 / 4
static_assert(FanLpK::has(2) && FanLpK::has(kFanMax) && !FanLpK::has(kFanMax + 1), "FanLpK is 2..kFanMax");
static_assert(!FanLpM::has(17), "one run offset per channel: at most sixteen");

template <int M, int K>
void launch_fan_lp_mk(const FanLpParams &p, hipStream_t st) {
  static_assert(LpcmM::has(M) && FanM::has(M) && FanK::has(K), "FanLpM x FanLpK lies inside LpcmM x FanM x FanK");
  constexpr size_t lds = sizeof(float) * (size_t)fan_lds_floats(K, M);
  launch_big_lds<&render_fanout_kernel<M, K, true>, (int)lds>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

}  // namespace

int iamf_hip_fanout_lp_launch(const void *params, int m, int k, hipStream_t st) {
  FanLpParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || p.n_launch <= 0) return 0;
  for (int j = 0; j < k && j < kFanMax; ++j)
    if (p.mem[j].out_ch < 1 || p.mem[j].out_ch > 2) return 0;
  return dispatch(FanLpM{}, m, [&](auto M) {
    return dispatch(FanLpK{}, k, [&](auto K) { launch_fan_lp_mk<M.value, K.value>(p, st); });
  });
}
