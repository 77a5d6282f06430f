// iamf_render_wide4.hip — instantiations of render_wide4_kernel<M, C> (render_wide4.hpp), in a
// translation unit of their own so that the build compiles them next to iamf_render.hip.
// Compiled with -ffp-contract=off like every kernel of the library: the projection is bit-exact.
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
  if (p.use_mfma) launch_big_lds<&render_wide4_kernel<M, C, true, false>, 80 * 1024>(grid, dim3(256), lds, st, p);
  else launch_big_lds<&render_wide4_kernel<M, C, false, false>, 80 * 1024>(grid, dim3(256), lds, st, p);
}

// scalable channel audio: M decoded channels -> demixer -> the M channels of the target layout -> C
template <int M, int C>
void launch_mc_demixer(const RenderParams &p, hipStream_t st) {
  static_assert(wide4_lds_floats(C, M, kW4DmxFloats) <= 20480, "two workgroups per CU");
  const size_t lds = sizeof(float) * (size_t)wide4_lds_floats(C, M, kW4DmxFloats);
  launch_big_lds<&render_wide4_kernel<M, C, false, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

// parametric down-mixer: M channels of the element's layout -> the C channels of a smaller IAMF layout
template <int M, int C>
void launch_mc_downmixer(const RenderParams &p, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)wide4_lds_floats(C, M, 0);
  launch_big_lds<&render_wide4_kernel<M, C, false, false, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

}  // namespace

int iamf_hip_wide4_launch(const void *params, int m, hipStream_t st) {
  RenderParams p;
  memcpy(&p, params, sizeof(p));
  if (p.dmx_on)
    return dispatch(Wide4DownMC{}, mc(m, p.out_ch), [&](auto V) { launch_mc_downmixer<mc_m(V.value), mc_c(V.value)>(p, st); });
  if (p.demix_on)
    return dispatch(Wide4DemixM{}, m, [&](auto M) {
      return dispatch(Wide4DemixC{}, p.out_ch, [&](auto C) { launch_mc_demixer<M.value, C.value>(p, st); });
    });
  return dispatch(Wide4M{}, m, [&](auto M) {
    return dispatch(Wide4C{}, p.out_ch, [&](auto C) { launch_mc<M.value, C.value>(p, st); });
  });
}
