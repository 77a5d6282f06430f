// iamf_render_lpcm.hip — the headline kernel fed with LPCM packets: render_fast_kernel<M, OC, 0, false, false, LP = true>
// (render_fast.hpp) for mono-coded ambisonics elements (M = 1, 4, 9, 16 sub-streams of one channel each) into one- and
// two-channel layouts, in a translation unit of its own (compiled beside iamf_render.hip).
//
// What it replaces: the reference decodes an LPCM sub-stream packet into its planar f32 decoder buffer
// (src/iamf_dec/pcm/IAMF_pcm_decoder.c:64-83, 133-149: sample / 2^15; channel order by IAMF_decoder.c:2230-2260) and the
// renderer reads that buffer (IAMF_decoder.c:2550-2640).  On the device the f32 copy is 64 of the path's 68 bytes per
// sample-frame; here the render kernel reads the 16-bit samples themselves (32 + 4 bytes per sample-frame) and converts
// them where it loads them, by the same expression — results are bit-identical to iamf_hip_lpcm_unpack followed by the
// f32 kernel (tests/test_gpu_lpcm.py).  Entry: iamf_hip_batch_render_lpcm (iamf_render.hip), which falls back to exactly
// that pair for every input this kernel does not take.
#include "render_fast_unit.hpp"

int iamf_hip_fast_lpcm_launch(const void *params, int m, int early, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm) return 0;
  return launch_fast_lp<LpcmM, LpcmOC, 2, false>(p, m, early != 0, st);
}
