// iamf_render_wide4_mix.hip — instantiations of the mixing variant of render_wide4_kernel
// (render_wide4.hpp, MIX = true: second element and / or per-sample gain ramps), in a translation
// unit of their own so that the build compiles them next to the other kernels.
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
  static_assert(wide4_lds_floats(C, M, kW4MixFloats) <= 20480, "two workgroups per CU");
  const size_t lds = sizeof(float) * (size_t)wide4_lds_floats(C, M, kW4MixFloats);
  const dim3 grid((unsigned)p.n_launch);
  if (p.use_mfma) launch_big_lds<&render_wide4_kernel<M, C, true, false, false, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
  else launch_big_lds<&render_wide4_kernel<M, C, false, false, false, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
}

}  // namespace

int iamf_hip_wide4_mix_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  return dispatch(Wide4M{}, m, [&](auto M) {
    return dispatch(Wide4MixC{}, p.out_ch, [&](auto C) { launch_mc<M.value, C.value>(p, st); });
  });
}
