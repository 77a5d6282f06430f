// iamf_render_fir_m2b.hip — the binaural FIR renderer for CHANNEL-BASED elements (the role of
// IAMF_element_renderer_render_M2B, reference m2b_rdr.c:103-121, call site IAMF_decoder.c:2562-2570):
// instantiations of render_fast_kernel<M, 2, FIR> for the channel counts of the IAMF loudspeaker
// layouts (stereo 2, 5.1 / 3.1.2 6, 5.1.2 / 7.1 8, 5.1.4 / 7.1.2 10, 7.1.4 12), in a translation unit of
// their own so that the build compiles them next to the ambisonics ones (iamf_render.hip: 1, 4, 9, 16).
//   y[ear][t] = sum_c sum_k h[ear][c][k] * x[c][t - k]        c = loudspeaker channel, playback order
// PARITY UNPINNED like the scene-based form: the reference hands this to BEAR (bear/iamf_bear_api.h),
// which is not in its tree; the formula above, with one HRIR pair per loudspeaker supplied by the
// caller, is this library's specification (render_fir.hpp).
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
#include "render_fir_launch.hpp"

}  // namespace

int iamf_hip_fir_m2b_launch_fft(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  return dispatch(FirM2bM{}, m, [&](auto M) { launch_fft_m<M.value>(p, st); });
}

int iamf_hip_fir_m2b_launch(const void *params, int m, int stage, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  return dispatch(FirM2bM{}, m, [&](auto M) { launch_fir_m<M.value>(p, stage, st); });
}
