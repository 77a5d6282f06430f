// iamf_render_nolim_packets.hip — the limiter-less renderer fed with 16-bit LPCM packets: render_nolim_kernel<M, 2, LPC>
// (render_nolim.hpp) for LpcmM = 1, 4, 9, 16 mono-coded channels and LpcmCoupledM = 2, 6, 8, 10, 12 coupled ones, nine instances
// in a translation unit of their own.  Its sibling iamf_render_nolim_packets24.hip holds the nine 24-bit instances and refers to
// the argument below.
//
// What it replaces: the first stage of a rate-converting stream (render -> resampler -> limiter) and the whole render of a
// stream whose limiter is switched off ran iamf_hip_lpcm_unpack — an f32 copy of the element written to and read from HBM — and
// then render_nolim_kernel<M> or the general kernel.  For a 3rd-order 16-bit element into stereo f32 that is 32 + 64 + 64 + 8 =
// 168 bytes per sample-frame against 32 + 8 = 40 here.  The geometry, the body behind the loads and the tile store are
// render_nolim_kernel<M>'s (one template, render_nolim.hpp); PCM is bit-identical to the unfused pair's (tests/test_gpu_zz_nolim_packets.py).
//
// Memory bounds.  The kernel reads no byte outside the samples of the call.  A run is what iamf_hip_lpcm_layout describes and
// lpcm_form_check (iamf_render.hip) has checked to lie inside the frame's packet row: frame_size samples from src_offset[c] on,
// src_step[c] bytes apart, also for a frame trimmed to n_samples.  The kernel starts `first` = first_sample samples into every
// run (RenderParams::lpcm_off holds src_offset + src_step * first).  A call's `total` is n_frames * frame_size with first == 0,
// or an n_samples with first + n_samples <= frame_size; frame_size and total are multiples of 4 and at least 4
// (nolim_packets_shape_ok, render_route.hpp; this unit's entry checks the two again).
//   * A lane loads the quad of samples k .. k + 3 of the call, k a multiple of 4, only if k < total; a lane at or past `total`
//     loads nothing.  In a call of whole frames the quad lies at position i = k mod frame_size of frame k / frame_size, i a
//     multiple of 4 below frame_size, so i + 3 < frame_size: a quad never straddles a frame.  In a trimmed frame (one frame,
//     total <= frame_size, so k / frame_size == 0 and i == k) it covers samples first + k .. first + k + 3 of the run, and
//     k + 4 <= total, so first + k + 3 < first + total <= frame_size: it ends inside the samples of the call.
//   * The four load shapes.  A mono run of 16-bit samples: 8 bytes at lpcm_off[c] + 2 * i, samples i .. i + 3 of the run.  Of
//     24-bit samples: 12 bytes at lpcm_off[c] + 3 * i, the same four samples.  A coupled 16-bit pair (c, c + 1), one run of
//     interleaved samples: 16 bytes at lpcm_off[c] + 4 * i, samples i .. i + 3 of channel c (step 4) and, 2 bytes on, of
//     channel c + 1 — the last byte loaded is the last byte of sample i + 3 of channel c + 1.  A coupled 24-bit pair: 2 x 12
//     bytes at lpcm_off[c] + 6 * i and 12 bytes on, samples i .. i + 3 of both channels (step 6, the partner 3 bytes on), ending
//     with sample i + 3 of channel c + 1.  In each shape the bytes loaded are exactly those of samples i .. i + 3 of the
//     run(s), every one of which is a sample of the call.
//   * Addresses are 64-bit pointers (stream * raw_stream_stride + frame * raw_frame_stride + run offset, in int64_t), as in the
//     f32 form: no bound on the call's extent is needed.
//   * Stores: the tile holds kNlChunk sample-frames of out_ch * bytes <= kNlMaxFrameBytes each (60 KiB of LDS, the launch's
//     dynamic size); lane t writes sample-frames 4 t .. 4 t + 3 of it.  PCM: the chunk's n_here * out_ch * bytes bytes from
//     pcm + stream * pcm_stream_stride + c0 * out_ch * bytes on, whole 16-byte pieces, which range_args_check (iamf_render.hip)
//     has checked to fit the stream's row.
// Entry: iamf_hip_batch_render_packets_nolim (iamf_render.hip), which takes exactly the path of
// iamf_hip_batch_render_packets_ragged for every call this kernel does not take.
#include "render_nolim_unit.hpp"

int iamf_hip_nolim_packets_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!nolim_lp_params_ok(p, 2) || (p.lpcm_coupled != 0 && p.lpcm_coupled != 1)) return 0;
  return p.lpcm_coupled ? launch_nolim_lp<LpcmCoupledM, 2, true>(p, m, st) : launch_nolim_lp<LpcmM, 2, false>(p, m, st);
}
