// iamf_render_wide4_lfe.hip — instantiations of the LFE variant of render_wide4_kernel (render_wide4.hpp,
// LFE = true: ambisonics elements of order 1..3 rendered to a layout with LFE channels while the HOA LFE
// generator is on), in a translation unit of their own so that the build compiles them next to the others.
// Compiled with -ffp-contract=off like every kernel of the library.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <atomic>
#include <string.h>

#include <type_traits>

#include "../../include/iamf_hip.h"
#include "render_entry.hpp"

namespace {

#include "render_common.hpp"
#include "render_downmix.hpp"
#include "render_fir.hpp"
#include "render_fir16.hpp"
#include "render_fir_fft.hpp"
#include "render_fast.hpp"
#include "render_wide4.hpp"

template <int M, int C>
void launch_mc(const RenderParams &p, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)wide4_lds_floats(C, M, 0);
  const dim3 grid((unsigned)p.n_launch);
  if (p.use_mfma) launch_big_lds<&render_wide4_kernel<M, C, true, false, false, false, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
  else launch_big_lds<&render_wide4_kernel<M, C, false, false, false, false, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
}

}  // namespace

int iamf_hip_wide4_lfe_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lfe || p.dmx_on || p.demix_on) return 0;
  return dispatch(Wide4LfeM{}, m, [&](auto M) {
    return dispatch(Wide4C{}, p.out_ch, [&](auto C) { launch_mc<M.value, C.value>(p, st); });
  });
}
