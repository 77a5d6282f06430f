// iamf_render_nolim_packets24_mix.hip — the limiter-less renderer fed with both elements of a mix as 24-bit LPCM packets:
// render_nolim_kernel<M, 3, LPC, LP2> (render_nolim.hpp) for element 0 in LpcmM or LpcmCoupledM and LP2 in LpcmMixK, eighteen
// instances.  What it replaces, the memory bounds of the 12-byte loads (dword-aligned: lpcm_form.hpp, S24 and S24C) and the
// entry: iamf_render_nolim_packets_mix.hip.
#include "render_nolim_unit.hpp"

int iamf_hip_nolim_packets24_mix_launch(const void *params, int m, int lp2, hipStream_t st) {
  RenderMixParams p;
  memcpy(&p, params, sizeof(p));
  if (!nolim_lp_mix_params_ok(p, 3, lp2) || (p.lpcm_coupled != 0 && p.lpcm_coupled != 2)) return 0;
  return p.lpcm_coupled ? launch_nolim_lp_mix<LpcmCoupledM, 3, true>(p, m, lp2, st) : launch_nolim_lp_mix<LpcmM, 3, false>(p, m, lp2, st);
}
