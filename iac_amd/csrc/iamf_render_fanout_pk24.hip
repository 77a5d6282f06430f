// iamf_render_fanout_pk24.hip — render_fanout_kernel<M, K, true, 3> (render_fanout.hpp): one mono-coded ambisonics element,
// held as 24-bit LPCM packets (lpcm_form.hpp, S24), rendered into K = 2..4 member batches with ONE pass over the packets, in
// a translation unit of its own.  (M, K): FanPk24MK (render_route.hpp).
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

int iamf_hip_fanout_pk24_launch(const void *params, int m, int k, hipStream_t st) {
  return fan_pk_launch<3, false>(FanPk24MK{}, params, m, k, st);
}
