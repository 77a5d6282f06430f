// iamf_render_packets_ragged.hip — the headline kernel fed with 16-bit mono-coded LPCM packets of any call length:
// render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY = true, LPB = 2, LPC = false, 0, IL = false, RAG = true>
// (render_fast.hpp) for LpcmM = 1, 4, 9, 16 channels into one or two, in a translation unit of its own.  Its three siblings
// hold the other single-element packet forms — iamf_render_packets_ragged_coupled.hip (LPB = 2, LPC), _packets_ragged24.hip
// (LPB = 3) and _packets_ragged24_coupled.hip (LPB = 3, LPC) — and refer to the argument below.
//
// What it replaces: a packet call that is no whole number of 64-sample blocks — an LPCM stream with frames of 1000, 480, 240
// or 120 samples rendered frame by frame, or the trimmed first or last frame of any stream (n_frames == 1, n_samples set) —
// ran iamf_hip_lpcm_unpack (an f32 copy of the element written to and read from HBM) and then render_kernel<M>
// (render_generic.hpp: one sample per lane, 256-sample chunks), because the packet-fed forms of the fast kernel wanted whole
// blocks.  Here the last chunk of a call may end anywhere, as in the planar f32 form (iamf_render_ragged.hip); the loads are
// the packet forms' own.  PCM, the sample-frames emitted and the persisted stream state are bit-identical to the unfused
// pair's (tests/test_gpu_zz_packets_ragged.py).
//
// Memory bounds.  The kernel reads no byte outside the channel runs of the call's frames.  A run is what
// iamf_hip_lpcm_layout describes and lpcm_form_check (iamf_render.hip) has checked to lie inside the frame's packet row:
// frame_size samples from src_offset[c] on, src_step[c] bytes apart, also for a frame trimmed to n_samples
// (include/iamf_hip.h says so).  The kernel starts `first` = first_sample samples into every run (RenderParams::lpcm_off holds
// src_offset + src_step * first).  A call's `total` is n_frames * frame_size with first == 0, or an n_samples with
// first + n_samples <= frame_size (lpcm_form_check, range_args_check); frame_size is a multiple of 4, and for a call shorter
// than a frame first + ((total + 3) & ~3) <= frame_size (packets_ragged_shape_ok, render_route.hpp).
//   * A lane loads the quad of samples k .. k + 3 of the call, k a multiple of 4, only if k < total.  In a call of whole frames it
//     lies at position i = k mod frame_size of frame k / frame_size, i a multiple of 4 below frame_size, so i + 3 < frame_size.
//     In a trimmed frame it covers samples first + k .. first + k + 3 of the run, and k + 4 <= (total + 3) & ~3, so
//     first + k + 3 < frame_size.  Either way a quad that starts below `total` ends inside its run, though it may end behind
//     n_samples: those packet samples are converted like any others (integers: finite numbers) and replaced by zeros by the
//     select in front of the maxima (render_fast.hpp, RAG).
//   * A lane at or past `total` asks for the call's first quad (frame 0, position 0: total >= 1, so it is inside its run by
//     the line above) while there is a next chunk, and through the zero-record resource — no memory access — when there
//     is none.
//   * The four load shapes.  A mono run of 16-bit samples: 8 bytes at lpcm_off[c] + 2 * i, samples i .. i + 3 of the run.  Of
//     24-bit samples: 12 bytes at lpcm_off[c] + 3 * i, the same four samples.  A coupled 16-bit pair (c, c + 1), one run of
//     interleaved samples: 16 bytes at lpcm_off[c] + 4 * i, which are samples i .. i + 3 of channel c (step 4) and, 2 bytes on, of
//     channel c + 1 — the last byte loaded is the last byte of sample i + 3 of channel c + 1.  A coupled 24-bit pair: 2 x 12
//     bytes at lpcm_off[c] + 6 * i and 12 bytes on, samples i .. i + 3 of both channels (step 6, the partner 3 bytes on), ending
//     with sample i + 3 of channel c + 1.  In each shape the bytes loaded are exactly those of samples i .. i + 3 of the
//     run(s), every one of which is below frame_size.
// Entry: iamf_hip_batch_render_packets_ragged (iamf_render.hip), which takes exactly the path of iamf_hip_batch_render_packets
// for every call this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_packets_ragged_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (p.ragged != kCallPacketsRagged || !p.lpcm || p.lpcm_coupled || p.lpcm_bytes == 3 || p.total < 1 || p.frame_size < 4 || (p.frame_size & 3)) return 0;
  return launch_fast_lp_rag<LpcmM, LpcmOC, 2, false>(p, m, st);
}
