// iamf_render_lpcm_coupled.hip — the headline kernel fed with the 16-bit LPCM packets of a channel-based element whose
// channel pairs are coupled sub-streams: render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY, LPB = 2, LPC = true>
// (render_fast.hpp) for stereo, 5.1, 5.1.2 / 7.1, 5.1.4 / 7.1.2 and 7.1.4 into one or two channels, in a translation unit
// of its own (compiled beside iamf_render_lpcm.hip and iamf_render_lpcm24.hip).
//
// What it replaces: iamf_hip_lpcm_unpack (2 * M bytes read, 4 * M written per sample-frame) followed by the f32 kernel
// (4 * M read, 4 written into s16 stereo) — 24 / 64 / 124 bytes per sample-frame of a stereo / 5.1 / 7.1.4 element.  Here
// the render kernel reads the packets themselves, 2 * M + 4 bytes: a pair's four sample-frames L0 R0 .. L3 R3 are one
// 16-byte load per lane, C and LFE 8-byte loads as in the mono-coded form, and every channel is cut out and converted
// where it is consumed, by the reference's expression (pcm/IAMF_pcm_decoder.c:64-83: sample / 32768.f, the power of two
// folded into the staged weights).  Results are bit-identical to the unfused pair (tests/test_gpu_lpcm_coupled.py).
// Entry: iamf_hip_batch_render_lpcm (iamf_render.hip), which falls back to exactly that pair for every input this kernel
// does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm_coupled_launch(const void *params, int m, int early, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || !p.lpcm_coupled || p.lpcm_bytes == 3) return 0;
  return launch_fast_lp<LpcmCoupledM, LpcmOC, 2, true>(p, m, early != 0, st);
}
