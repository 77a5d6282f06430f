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
#include "render_fast_unit.hpp"

int iamf_hip_fast_interleaved_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.interleaved || !p.in || p.frame_size != 1 || p.in_frame_stride != m) return 0;
  return launch_fast_rag<InterleavedM, InterleavedOC, true>(p, m, st);
}
