// render_nolim_unit.hpp — what the translation units that feed the limiter-less renderer (render_nolim.hpp) LPCM packets share:
// iamf_render_nolim_packets.hip (16-bit samples) and iamf_render_nolim_packets24.hip (24-bit ones), and their two-element
// siblings iamf_render_nolim_packets_mix.hip and iamf_render_nolim_packets24_mix.hip.  Each includes this header
// at file scope and nothing else, and holds its head comment and its entry of render_entry.hpp: the parameter sanity test and
// the launcher below over the mono-coded and the coupled list, which are the lists the instance listing walks
// (render_route.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <atomic>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/iamf_hip.h"
#include "render_entry.hpp"

namespace {

#include "render_common.hpp"
#include "render_nolim.hpp"

// render_nolim_kernel<M, LPB, LPC> for M out of MList: (streams, chunks of kNlChunk sample-frames), the tile in the output
// format as for render_nolim_kernel (at most kNlChunk * kNlMaxFrameBytes = 60 KiB).  False if m names no instance.
template <class MList, int LPB, bool LPC>
bool launch_nolim_lp(const RenderParams &p, int m, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
    const dim3 grid((unsigned)p.n_launch, (unsigned)((p.total + kNlChunk - 1) / kNlChunk));
    hipLaunchKernelGGL((render_nolim_kernel<decltype(M)::value, LPB, LPC>), grid, dim3(256), (size_t)kNlChunk * p.out_ch * bytes, st, p);
  });
}

// what both units refuse before they launch: a block that does not carry the form's mark or would index outside the tile
inline bool nolim_lp_params_ok(const RenderParams &p, int lpb) {
  const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
  if (p.ragged != kCallPacketsNolim || !p.lpcm || p.limiter_on || (lpb == 3) != (p.lpcm_bytes == 3)) return false;
  if (p.total < 4 || (p.total & 3) || p.frame_size < 4 || (p.frame_size & 3)) return false;
  return p.out_ch >= 1 && !((p.out_ch * bytes) & 3) && p.out_ch * bytes <= kNlMaxFrameBytes;
}

// render_nolim_kernel<M, LPB, LPC, LP2> for M out of MList and LP2 out of LpcmMixK (iamf_render_nolim_packets*_mix.hip): the same
// grid and tile, the block with the second element's packets behind it.  False if (m, lp2) names no instance.
template <class MList, int LPB, bool LPC>
bool launch_nolim_lp_mix(const RenderMixParams &p, int m, int lp2, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(LpcmMixK{}, lp2, [&](auto K) {
      const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
      const dim3 grid((unsigned)p.n_launch, (unsigned)((p.total + kNlChunk - 1) / kNlChunk));
      hipLaunchKernelGGL((render_nolim_kernel<decltype(M)::value, LPB, LPC, decltype(K)::value>), grid, dim3(256),
                         (size_t)kNlChunk * p.out_ch * bytes, st, p);
    });
  });
}

// what the two mix units refuse before they launch: a block that does not carry the form's mark, names no second element the
// kernel reads, or would index outside the tile
inline bool nolim_lp_mix_params_ok(const RenderMixParams &p, int lpb, int lp2) {
  const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
  if (p.ragged != kCallPacketsMixNolim || !p.lpcm || !p.lpcm2 || p.limiter_on || (lpb == 3) != (p.lpcm_bytes == 3)) return false;
  if (p.lpcm_mix != ((lpb == 3 ? 4 : 0) | lp2) || !lpcm_mix_m2_ok(lp2, p.m2) || !p.matrix2 || !p.src_feed2 || !p.gains2) return false;
  if (p.total < 4 || (p.total & 3) || p.frame_size < 4 || (p.frame_size & 3)) return false;
  if ((p.elem_ramp || p.elem2_ramp || p.out_ramp) && (p.ramp_stream_stride & 3)) return false;
  return p.out_ch >= 1 && !((p.out_ch * bytes) & 3) && p.out_ch * bytes <= kNlMaxFrameBytes;
}

}  // namespace
