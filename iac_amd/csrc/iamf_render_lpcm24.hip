// iamf_render_lpcm24.hip — the headline kernel fed with 24-bit LPCM packets: render_fast_kernel<M, OC, 0, false, false,
// LP = true, EARLY, LPB = 3> (render_fast.hpp) for the elements and layouts of iamf_render_lpcm.hip, in a translation unit
// of its own (compiled beside it).
//
// What it replaces: iamf_hip_lpcm_unpack (48 bytes read, 64 written per sample-frame of a 3rd-order element) followed by the
// f32 kernel (64 read, 4 written).  Here the render kernel reads the 24-bit samples themselves — 12 bytes per lane and
// channel in one load, 48 + 4 bytes per sample-frame — and converts them where a channel is consumed, by the reference's
// expression (pcm/IAMF_pcm_decoder.c:71-76, 144-148: sample / 2^23, the power of two folded into the staged weights):
// results are bit-identical to the unfused pair (tests/test_gpu_lpcm24.py).  Entry: iamf_hip_batch_render_lpcm
// (iamf_render.hip), which falls back to exactly that pair for every input this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm24_launch(const void *params, int m, int early, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || p.lpcm_bytes != 3) return 0;
  return launch_fast_lp<LpcmM, LpcmOC, 3, false>(p, m, early != 0, st);
}
