// iamf_render_packets_mix_ragged24.hip — the headline kernel fed with the 24-bit LPCM packets of BOTH elements of a two-element
// mix, the first one a mono-coded ambisonics element, in a call of any length: render_fast_kernel<M, OC, 0, false, IN2 = true,
// LP = true, EARLY = true, LPB = 3, LPC = false, LP2, IL = false, RAG = true> (render_fast.hpp) for LpcmM = 1, 4, 9, 16 channels into
// one or two, the second element mono-coded runs (LP2 = 1) or one coupled stereo pair (LP2 = 2), in a translation unit of its
// own.  What it replaces, and why every byte it loads lies inside the channel runs of the call's frames and every ramp float
// below the call's end, iamf_render_packets_mix_ragged.hip says for all four units.
// Entry: iamf_hip_batch_render_packets_mix_ragged (iamf_render.hip).
#include "render_fast_unit.hpp"

int iamf_hip_fast_packets_mix_ragged24_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (p.ragged != kCallPacketsMixRagged || !p.lpcm || !p.lpcm2 || p.lpcm_coupled || p.lpcm_bytes != 3 || p.lpcm_mix != (4 | lp2) || p.total < 1 ||
      p.frame_size < 4 || (p.frame_size & 3))
    return 0;
  return launch_fast_lp_mix_rag<LpcmM, LpcmOC, false, LpcmMixK, 3>(p, m, lp2, st);
}
