// iamf_render_nolim_packets_mix.hip — the limiter-less renderer fed with BOTH elements of a mix as 16-bit LPCM packets:
// render_nolim_kernel<M, 2, LPC, LP2> (render_nolim.hpp) for element 0 in LpcmM = 1, 4, 9, 16 (mono-coded) or LpcmCoupledM = 2, 6, 8,
// 10, 12 (coupled) and LP2 in LpcmMixK (1: a mono-coded second element of 1 or 4 runs, 2: ONE coupled stereo pair), eighteen
// instances in a translation unit of their own.  Its sibling iamf_render_nolim_packets24_mix.hip holds the eighteen 24-bit
// instances and refers to the argument below.
//
// What it replaces: a bed plus dialogue or commentary on a batch without the limiter — the first stage of a rate-converting
// stream and the whole render of a stream whose limiter is switched off — ran two iamf_hip_lpcm_unpack passes and then the general
// kernel, one sample per lane.  For a 3rd-order 16-bit bed plus a coupled stereo element into stereo f32 that is 36 bytes of
// packets, 72 of f32 written, 72 of f32 read and 8 of PCM per sample-frame against 36 + 8 = 44 here.  The geometry, element 0's
// loads and the tile store are render_nolim_kernel<M, LPB, LPC>'s; the arithmetic per output slot is the general kernel's,
// operation for operation (render_generic.hpp), so PCM is bit-identical to the unfused path's (tests/test_gpu_zz_nolim_packets_mix.py).
//
// Memory bounds.  The kernel reads no byte outside the samples of the call.  Element 0: the argument of
// iamf_render_nolim_packets.hip, unchanged (the same loads under the same rule: nolim_packets_mix_shape_ok repeats
// nolim_packets_shape_ok's terms).  Element 1's runs are what its own iamf_hip_lpcm_layout describes and lpcm_form_check_ch
// (iamf_render.hip) has checked to lie inside its frame's packet row: frame_size samples from src_offset[c] on, src_step[c] bytes
// apart.  Both elements share `first` = first_sample (render_lpcm_mix_impl refuses a call whose two inputs differ in it), total and
// frame_size, all multiples of 4 with first + total <= frame_size for a trimmed frame.
//   * A lane loads element 1's quad of samples k .. k + 3 of the call under the condition it loads element 0's: k < total; the
//     quad lies at position i of frame f exactly as element 0's does, so i + 3 < frame_size in whole frames and
//     first + k + 3 < first + total <= frame_size in a trimmed one.
//   * LP2 == 1: 8 bytes at lpcm2_off[m] + 2 * i for m < m2 only (m2 = 1 or 4, lpcm_mix_m2_ok: a one-channel element's runs
//     1 .. 3 do not exist and are not read), samples i .. i + 3 of run m.  LP2 == 2: 16 bytes at lpcm2_off[0] + 4 * i, samples
//     i .. i + 3 of L and, 2 bytes on, of R — the last byte loaded is the last byte of sample i + 3 of R (the partner lies one
//     sample behind: nolim_packets_mix_shape_ok).  With 24-bit samples: 12 bytes at lpcm2_off[m] + 3 * i, and 2 x 12 bytes at
//     lpcm2_off[0] + 6 * i.  In each shape the bytes loaded are exactly those of samples i .. i + 3 of the run(s).
//   * Ramps, where the call gives them: one float4 at ramp + s * ramp_stream_stride + k, floats k .. k + 3 of the stream's row
//     with k + 4 <= total: no float behind the call's last sample is read (16-byte aligned: the row starts on the grid, the
//     stride and k are multiples of 4).
//   * matrix2 rows [fd2 * m2, fd2 * m2 + m2), src_feed2[c] for c < out_ch and gains2[s]: the batch's own tables, as the general
//     kernel reads them.
//   * Addresses are 64-bit pointers, as in the single-element form: no bound on the call's extent is needed.
//   * Stores: the single-element form's, unchanged — and the stream state.  The general kernel persists its LDS ring behind
//     every call, limiter or not, and the state exported behind a call of this kernel is that kernel's, bit for bit
//     (render_nolim.hpp): ring_y[s][c][e] for c < out_ch, e < kSave = 256 — a sample's own entry e = k + q - (total - 256) >= 0,
//     below 256 because k + q < total, and in a call shorter than 256 the entries below 256 - total moved up through the tile
//     (256 floats per channel: out_ch * 1024 bytes of the tile's out_ch * bytes * 1024) — and ring_pm[s][e], e = the lane.  Both
//     are the batch's [n_streams][out_ch][256] and [n_streams][256]; s is a stream of the batch.
// Entry: iamf_hip_batch_render_packets_mix_nolim (iamf_render.hip), which takes exactly the path of
// iamf_hip_batch_render_packets_mix_ragged for every call this kernel does not take.
#include "render_nolim_unit.hpp"

int iamf_hip_nolim_packets_mix_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (!nolim_lp_mix_params_ok(p, 2, lp2) || (p.lpcm_coupled != 0 && p.lpcm_coupled != 1)) return 0;
  return p.lpcm_coupled ? launch_nolim_lp_mix<LpcmCoupledM, 2, true>(p, m, lp2, st) : launch_nolim_lp_mix<LpcmM, 2, false>(p, m, lp2, st);
}
