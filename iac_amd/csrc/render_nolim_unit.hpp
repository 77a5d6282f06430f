// render_nolim_unit.hpp — what the translation units that feed the limiter-less renderer (render_nolim.hpp) LPCM packets share:
// iamf_render_nolim_packets.hip (16-bit samples) and iamf_render_nolim_packets24.hip (24-bit ones).  Each includes this header
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
  if (p.ragged != 4 || !p.lpcm || p.limiter_on || (lpb == 3) != (p.lpcm_bytes == 3)) return false;
  if (p.total < 4 || (p.total & 3) || p.frame_size < 4 || (p.frame_size & 3)) return false;
  return p.out_ch >= 1 && !((p.out_ch * bytes) & 3) && p.out_ch * bytes <= kNlMaxFrameBytes;
}

}  // namespace
