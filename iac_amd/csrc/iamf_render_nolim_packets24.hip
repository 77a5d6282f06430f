// iamf_render_nolim_packets24.hip — the limiter-less renderer fed with 24-bit LPCM packets: render_nolim_kernel<M, 3, LPC>
// (render_nolim.hpp) for LpcmM = 1, 4, 9, 16 mono-coded channels and LpcmCoupledM = 2, 6, 8, 10, 12 coupled ones, nine instances.
// What it replaces, the memory bounds of the 12-byte loads (dword-aligned: lpcm_form.hpp, S24 and S24C) and the entry:
// iamf_render_nolim_packets.hip.
#include "render_nolim_unit.hpp"

int iamf_hip_nolim_packets24_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!nolim_lp_params_ok(p, 3) || (p.lpcm_coupled != 0 && p.lpcm_coupled != 2)) return 0;
  return p.lpcm_coupled ? launch_nolim_lp<LpcmCoupledM, 3, true>(p, m, st) : launch_nolim_lp<LpcmM, 3, false>(p, m, st);
}
