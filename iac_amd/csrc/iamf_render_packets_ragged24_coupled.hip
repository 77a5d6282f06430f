// iamf_render_packets_ragged24_coupled.hip — the headline kernel fed with the coupled 24-bit LPCM packets of a channel-based
// element, any call length: render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY = true, LPB = 3, LPC = true, 0,
// IL = false, RAG = true> (render_fast.hpp) for LpcmCoupledM = 2, 6, 8, 10, 12 channels into one or two, in a translation unit
// of its own.  What it replaces, and why every byte it loads lies inside the channel runs of the call's frames — a pair's
// 2 x 12 bytes per lane and a mono run's 12 — iamf_render_packets_ragged.hip says for all four units.
// Entry: iamf_hip_batch_render_packets_ragged (iamf_render.hip).
#include "render_fast_unit.hpp"

int iamf_hip_fast_packets_ragged24_coupled_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (p.ragged != kCallPacketsRagged || !p.lpcm || p.lpcm_coupled != 2 || p.lpcm_bytes != 3 || p.total < 1 || p.frame_size < 4 || (p.frame_size & 3)) return 0;
  return launch_fast_lp_rag<LpcmCoupledM, LpcmOC, 3, true>(p, m, st);
}
