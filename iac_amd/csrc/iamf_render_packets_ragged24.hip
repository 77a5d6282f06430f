// iamf_render_packets_ragged24.hip — the headline kernel fed with 24-bit mono-coded LPCM packets of any call length:
// render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY = true, LPB = 3, LPC = false, 0, IL = false, RAG = true>
// (render_fast.hpp) for LpcmM = 1, 4, 9, 16 channels into one or two, in a translation unit of its own.  What it replaces, and
// why every byte it loads lies inside the channel runs of the call's frames — 12 bytes per lane and channel —
// iamf_render_packets_ragged.hip says for all four units.
// Entry: iamf_hip_batch_render_packets_ragged (iamf_render.hip).
#include "render_fast_unit.hpp"

int iamf_hip_fast_packets_ragged24_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (p.ragged != kCallPacketsRagged || !p.lpcm || p.lpcm_coupled || p.lpcm_bytes != 3 || p.total < 1 || p.frame_size < 4 || (p.frame_size & 3)) return 0;
  return launch_fast_lp_rag<LpcmM, LpcmOC, 3, false>(p, m, st);
}
