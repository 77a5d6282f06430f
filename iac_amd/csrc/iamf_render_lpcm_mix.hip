// iamf_render_lpcm_mix.hip — the headline kernel fed with the 16-bit LPCM packets of BOTH elements of a two-element mix, the
// first one a mono-coded ambisonics element: render_fast_kernel<M, OC, 0, false, IN2 = true, LP = true, EARLY = true, 2,
// LPC = false, LP2> (render_fast.hpp) for 1 / 4 / 9 / 16 channels into one or two, the second element mono-coded runs
// (LP2 = 1: mono or first-order ambisonics) or one coupled stereo pair (LP2 = 2).  Its sibling for a coupled element 0 is
// iamf_render_lpcm_mix_coupled.hip; each is a translation unit of its own, compiled beside the single-element ones.
//
// What it replaces: iamf_hip_lpcm_unpack of the second element (2 * m2 bytes read, 4 * m2 written per sample-frame), then
// iamf_hip_batch_render_lpcm with d_in2, which unpacks the first element (2 * M read, 4 * M written) and runs the f32 mixing
// kernel (4 * (M + m2) read, 4 written into s16 stereo): 10 * (M + m2) + 4 bytes, 184 for a 3rd-order bed with a stereo
// second element.  Here the render kernel reads both elements' packets itself, 2 * (M + m2) + 4 = 40 bytes, and converts
// every channel where it is consumed, by the reference's expression (pcm/IAMF_pcm_decoder.c:64-83: sample / 32768.f, the
// power of two folded into the staged weights of both matrices).  Everything behind the two projections — constant or
// per-sample gains, the mix, the limiter, the pack — is the f32 mixing variant's code, so ramps are fused as well.  Results
// are bit-identical to the unfused sequence (tests/test_gpu_lpcm_mix.py).
// Entry: iamf_hip_batch_render_lpcm_mix (iamf_render.hip), which falls back to exactly that sequence for every input this
// kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm_mix_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || !p.lpcm2 || p.lpcm_coupled || p.lpcm_bytes == 3 || p.lpcm_mix != lp2) return 0;
  return launch_fast_lp_mix<LpcmM, LpcmOC, false, LpcmMixK>(p, m, lp2, st);
}
