// iamf_render_interleaved.hip — the headline kernel fed with ordinary interleaved f32 of any call length:
// render_fast_kernel<M, OC, 0, false, false, false, true, 2, false, 0, IL = true, RAG = true> (render_fast.hpp) for one or two
// channels into one or two, in a translation unit of its own.
//
// What it replaces: the limiter stage behind a rate converter — a frame_size == 1 batch over the resampler's output, 1114 or
// 1115 sample-frames for 1024 at 44.1 -> 48 kHz — ran on render_kernel<M> (render_generic.hpp: one sample per lane, 256-sample
// chunks, four barriers and 31 LDS reads per lane and chunk), because the fast kernel wanted planar rows and whole 64-sample
// blocks.  Here a lane's four sample-frames are 16 * M contiguous bytes, loaded as one or two 16-byte pieces and transposed in
// registers, and the last chunk of a call may end anywhere; everything behind the load is the planar form's body.  PCM, the
// sample-frames emitted and the persisted stream state are bit-identical to the general kernel's (tests/test_gpu_interleaved.py).
// Entry: iamf_hip_batch_render_interleaved (iamf_render.hip), which takes the path of iamf_hip_batch_render_range for every
// call this kernel does not take.
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

template <int M, int OC>
void launch_il_mc(const RenderParams &p, hipStream_t st) {
  constexpr size_t lds = sizeof(float) * (size_t)fast_lds_floats(OC, M);
  // built for the four workgroups per CU of the planar f32 form <M, OC> (render_fast_kernel's launch bounds)
  static_assert(lds * 4 <= 160 * 1024, "the workgroups the instance is built for fit a CU's LDS");
  launch_big_lds<&render_fast_kernel<M, OC, 0, false, false, false, true, 2, false, 0, true, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds,
                                                                                                                st, p);
}

}  // namespace

int iamf_hip_fast_interleaved_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.interleaved || !p.in || p.frame_size != 1 || p.in_frame_stride != m) return 0;
  return dispatch(InterleavedM{}, m, [&](auto M) {
    return dispatch(InterleavedOC{}, p.out_ch, [&](auto OC) { launch_il_mc<M.value, OC.value>(p, st); });
  });
}
