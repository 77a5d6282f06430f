// iamf_render_lpcm24_mix_coupled.hip — the headline kernel fed with the 24-bit LPCM packets of BOTH elements of a two-element
// mix, the first one a channel-based element whose pairs are coupled sub-streams: render_fast_kernel<M, OC, 0, false,
// IN2 = true, LP = true, EARLY = true, 3, LPC = true, LP2> (render_fast.hpp) for stereo, 5.1, 5.1.2 / 7.1, 5.1.4 / 7.1.2 and
// 7.1.4 into one or two channels, the second element mono-coded runs (LP2 = 1) or one coupled stereo pair (LP2 = 2).  See
// iamf_render_lpcm24_mix.hip, its sibling for a mono-coded element 0, for what the form replaces: 5.1 with a mono second
// element reads 25 bytes per sample-frame into s16 stereo instead of 81, 7.1.4 with a stereo one 46 instead of 158.
// Entry: iamf_hip_batch_render_packets_mix (iamf_render.hip).
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm24_mix_coupled_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || !p.lpcm2 || p.lpcm_coupled != 2 || p.lpcm_bytes != 3 || p.lpcm_mix != (4 | lp2)) return 0;
  return launch_fast_lp_mix<LpcmCoupledM, LpcmOC, true, LpcmMixK, 3>(p, m, lp2, st);
}
