// iamf_render_lpcm24_mix.hip — the headline kernel fed with the 24-bit LPCM packets of BOTH elements of a two-element mix, the
// first one a mono-coded ambisonics element: render_fast_kernel<M, OC, 0, false, IN2 = true, LP = true, EARLY = true, 3,
// LPC = false, LP2> (render_fast.hpp) for 1 / 4 / 9 / 16 channels into one or two, the second element mono-coded runs
// (LP2 = 1: mono or first-order ambisonics) or one coupled stereo pair (LP2 = 2).  Its sibling for a coupled element 0 is
// iamf_render_lpcm24_mix_coupled.hip; each is a translation unit of its own, compiled beside the 16-bit ones
// (iamf_render_lpcm_mix.hip), whose body they share: the loads and cuts are those of the single-element 24-bit forms.
//
// What it replaces: two iamf_hip_lpcm_unpack passes (3 * (M + m2) bytes read, 4 * (M + m2) written per sample-frame) and
// the f32 mixing kernel (4 * (M + m2) read, 4 written into s16 stereo): 11 * (M + m2) + 4 bytes, 202 for a 3rd-order bed with
// a stereo second element.  Here the render kernel reads both elements' packets itself, 3 * (M + m2) + 4 = 58 bytes, and
// converts every channel where it is consumed, by the reference's expression (pcm/IAMF_pcm_decoder.c:71-76, 144-148:
// sample / 2^23, the power of two folded into the staged weights of both matrices).  Results are bit-identical to the
// unfused sequence (tests/test_gpu_zz_lpcm24_mix.py).
// Entry: iamf_hip_batch_render_packets_mix (iamf_render.hip), which takes exactly the path of
// iamf_hip_batch_render_lpcm_mix for every input this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm24_mix_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || !p.lpcm2 || p.lpcm_coupled || p.lpcm_bytes != 3 || p.lpcm_mix != (4 | lp2)) return 0;
  return launch_fast_lp_mix<LpcmM, LpcmOC, false, LpcmMixK, 3>(p, m, lp2, st);
}
