// iamf_render_fanout_pk16c.hip — render_fanout_kernel<M, K, true, 2, true> (render_fanout.hpp): one 5.1 / 7.1 / 5.1.4 / 7.1.4
// element whose pairs are coupled 16-bit sub-streams (lpcm_form.hpp, S16C), rendered into K = 2..4 member batches with ONE
// pass over the packets, in a translation unit of its own.  (M, K): FanPk16cMK (render_route.hpp).
// Entry: iamf_hip_batch_render_fanout_packets (iamf_render.hip).
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
#include "render_fanout_pk_unit.hpp"

}  // namespace

int iamf_hip_fanout_pk16c_launch(const void *params, int m, int k, hipStream_t st) {
  return fan_pk_launch<2, true>(FanPk16cMK{}, params, m, k, st);
}
