// iamf_render_lpcm24_coupled.hip — the headline kernel fed with the 24-bit LPCM packets of a channel-based element whose
// channel pairs are coupled sub-streams: render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY, LPB = 3, LPC = true>
// (render_fast.hpp) for stereo, 5.1, 5.1.2 / 7.1, 5.1.4 / 7.1.2 and 7.1.4 into one or two channels, in a translation unit
// of its own (compiled beside iamf_render_lpcm24.hip and iamf_render_lpcm_coupled.hip, whose two forms it combines).
//
// What it replaces: iamf_hip_lpcm_unpack (3 * M bytes read, 4 * M written per sample-frame) followed by the f32 kernel
// (4 * M read, 4 written into s16 stereo) — 26 / 70 / 136 bytes per sample-frame of a stereo / 5.1 / 7.1.4 element.  Here
// the render kernel reads the packets themselves, 3 * M + 4 bytes: a pair's four sample-frames L0 R0 .. L3 R3 are 24 bytes
// on the dword grid, two 12-byte loads per lane, C and LFE one 12-byte load as in the mono-coded 24-bit form, and every
// channel is cut out and converted where it is consumed, by the reference's expression (pcm/IAMF_pcm_decoder.c:71-76,
// 144-148: sample / 2^23, the power of two folded into the staged weights).  Results are bit-identical to the unfused pair
// (tests/test_gpu_zz_lpcm24_coupled.py).
// Entry: iamf_hip_batch_render_packets (iamf_render.hip), which takes exactly the path of iamf_hip_batch_render_lpcm_range
// for every input this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm24_coupled_launch(const void *params, int m, int early, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || p.lpcm_coupled != 2 || p.lpcm_bytes != 3) return 0;
  return launch_fast_lp<LpcmCoupledM, LpcmOC, 3, true>(p, m, early != 0, st);
}
