// iamf_render_packets_mix_ragged.hip — the headline kernel fed with the 16-bit LPCM packets of BOTH elements of a two-element
// mix, the first one a mono-coded ambisonics element, in a call of any length: render_fast_kernel<M, OC, 0, false, IN2 = true,
// LP = true, EARLY = true, LPB = 2, LPC = false, LP2, IL = false, RAG = true> (render_fast.hpp) for LpcmM = 1, 4, 9, 16 channels into
// one or two, the second element mono-coded runs (LP2 = 1: mono or first-order ambisonics) or one coupled stereo pair
// (LP2 = 2), in a translation unit of its own.  Its three siblings hold the other two-element packet forms —
// iamf_render_packets_mix_ragged_coupled.hip (LPB = 2, LPC), _packets_mix_ragged24.hip (LPB = 3) and
// _packets_mix_ragged24_coupled.hip (LPB = 3, LPC) — and refer to the argument below.
//
// What it replaces: a two-element packet call that is no whole number of 64-sample blocks — frames of 1000, 480, 240 or 120
// samples rendered frame by frame, or the trimmed first or last frame of any stream (n_frames == 1, n_samples set) — ran
// iamf_hip_lpcm_unpack twice (an f32 copy of either element written to and read from HBM) and then render_kernel<M>
// (render_generic.hpp: one sample per lane, 256-sample chunks), because the whole-block mix forms (iamf_render_lpcm_mix.hip,
// iamf_render_lpcm24_mix.hip) wanted whole blocks.  Here the last chunk of a call may end anywhere, as in the single-element
// form (iamf_render_packets_ragged.hip); both elements' loads are the mix forms' own, and everything behind the two
// projections — constant or per-sample gains, the mix, the limiter, the pack — is the mixing variant's code, so ramps are
// fused as well.  PCM, the sample-frames emitted and the persisted stream state are bit-identical to the unfused sequence's
// (tests/test_gpu_zz_packets_mix_ragged.py).
//
// Memory bounds.  The kernel reads no byte outside the channel runs of the call's frames, in either element, and no ramp float
// at or behind index `total` of a stream's row.
//   * Packets.  iamf_render_packets_ragged.hip has the argument for one element: a run holds frame_size samples from
//     src_offset on (lpcm_form_check_ch, iamf_render.hip, has checked it to lie inside the frame's packet row, for each element
//     with its own layout and strides); the kernel starts `first` samples into every run (RenderParams::lpcm_off and
//     RenderMixParams::lpcm2_off hold src_offset + src_step * first — the entry refuses a call whose two inputs name different
//     first samples); frame_size is a multiple of 4, and for a call shorter than a frame first + ((total + 3) & ~3) <= frame_size
//     (packets_mix_ragged_shape_ok, render_route.hpp).  A lane loads the quad of samples k .. k + 3 of the call, k a multiple of
//     4, only if k < total — element 1 and the ramps under exactly that condition (`if (k < p.total)` for the first chunk,
//     `if (k + kFChunk < p.total)` for every next one), element 0 as in the single-element form (a lane at or past `total` asks
//     for the call's first quad while there is a next chunk, through the zero-record resource when there is none).  Either way
//     a quad that starts below `total` ends inside its run, though it may end behind n_samples: those packet samples are
//     converted like any others (integers: finite numbers) and replaced by zeros by the select behind the mixing stage
//     (render_fast.hpp, RAG).
//   * Element 1's load shapes are element 0's: a mono run of 16-bit samples, 8 bytes at lpcm2_off[c] + 2 * i; of 24-bit samples,
//     12 bytes at lpcm2_off[c] + 3 * i; the coupled 16-bit pair, 16 bytes at lpcm2_off[0] + 4 * i; the coupled 24-bit pair,
//     2 x 12 bytes at lpcm2_off[0] + 6 * i and 12 bytes on.  In each the bytes loaded are exactly those of samples i .. i + 3 of
//     the run(s).  Channels at or beyond m2 are not loaded.
//   * Ramps.  A row holds `total` floats per stream from the call's first sample on (iamf_hip_render_args), rows 16-byte
//     aligned and ramp_stream_stride a multiple of 4 (the rule), so the quad at sample k, k a multiple of 4, is 16-byte
//     aligned.  A lane that loads it has k < total: with total - k >= 4 it loads 16 bytes, floats k .. k + 3, all below `total`;
//     otherwise floats k .. total - 1 singly (render_fast.hpp, load_x2).
// Entry: iamf_hip_batch_render_packets_mix_ragged (iamf_render.hip), which takes exactly the path of
// iamf_hip_batch_render_packets_mix for every call this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_packets_mix_ragged_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (p.ragged != kCallPacketsMixRagged || !p.lpcm || !p.lpcm2 || p.lpcm_coupled || p.lpcm_bytes == 3 || p.lpcm_mix != lp2 || p.total < 1 || p.frame_size < 4 ||
      (p.frame_size & 3))
    return 0;
  return launch_fast_lp_mix_rag<LpcmM, LpcmOC, false, LpcmMixK, 2>(p, m, lp2, st);
}
