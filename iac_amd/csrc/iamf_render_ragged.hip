// iamf_render_ragged.hip — the headline kernel fed with planar f32 of any call length:
// render_fast_kernel<M, OC, 0, false, false, false, true, 2, false, 0, IL = false, RAG = true> (render_fast.hpp) for the element
// shapes LPCM streams take (RaggedM = LpcmM and LpcmCoupledM together) into one or two channels, in a translation unit of its own.
//
// What it replaces: a call that is no whole number of 64-sample blocks — one frame of 1000, 480 or 120 samples per call, or the
// trimmed first or last frame of a stream (n_frames == 1, n_samples set) — ran on render_kernel<M> (render_generic.hpp: one
// sample per lane, 256-sample chunks, four barriers and 31 LDS reads per lane and chunk), because the fast kernel wanted whole
// blocks.  Here the last chunk of a call may end anywhere, as in the interleaved form; the loads are the planar form's.  PCM,
// the sample-frames emitted and the persisted stream state are bit-identical to the general kernel's (tests/test_gpu_ragged.py).
//
// Memory bounds.  The kernel reads no float outside the rows [0, frame_size) of the call's frames — rows the caller owns in
// full, frame_size floats per channel from d_in on, also for a frame trimmed to n_samples (include/iamf_hip.h says so).  A call's `total` is
// n_frames * frame_size or an n_samples <= frame_size (range_args_check), and frame_size is a multiple of 4 (ragged_shape_ok).
// A lane loads the quad of samples k .. k + 3 of the call, k a multiple of 4, only if k < total: it lies at position
// i = k mod frame_size of frame k / frame_size, i a multiple of 4 below frame_size, so i + 3 < frame_size — a quad that starts
// below `total` ends inside its row, though it may end behind n_samples (those floats are replaced by zeros by a select before
// anything looks at them: render_fast.hpp, RAG).  A lane at or past `total` asks for the stream's first quad (frame 0, position
// 0: inside its row) while there is a next chunk, and through the zero-record resource — no memory access — when there is none.
// Entry: iamf_hip_batch_render_ragged (iamf_render.hip), which takes the path of iamf_hip_batch_render_range for every call
// this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_ragged_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.ragged || !p.in || p.total < 1 || p.frame_size < 4 || (p.frame_size & 3)) return 0;
  return launch_fast_rag<RaggedM, RaggedOC, false>(p, m, st);
}
