// render_fast_unit.hpp — what the translation units that feed render_fast_kernel (render_fast.hpp) another input form share:
// iamf_render_lpcm.hip, _lpcm24.hip, _lpcm_coupled.hip, _lpcm24_coupled.hip, _lpcm_mix.hip, _lpcm_mix_coupled.hip, _lpcm24_mix.hip,
// _lpcm24_mix_coupled.hip, iamf_render_interleaved.hip,
// iamf_render_ragged.hip, iamf_render_packets_ragged.hip, _packets_ragged_coupled.hip, _packets_ragged24.hip,
// _packets_ragged24_coupled.hip and iamf_render_packets_mix_ragged.hip, _packets_mix_ragged_coupled.hip, _packets_mix_ragged24.hip,
// _packets_mix_ragged24_coupled.hip.
// The units stay separate, so that they compile side by side; each includes this header at file scope and nothing else, and
// holds its head comment and its entry of render_entry.hpp: the parameter sanity test and one call of a launcher below, in
// which the form's template arguments are written once.  A launcher dispatches over the lists it is given, which are the
// lists the instance listing walks (render_route.hpp), and returns false if (m, p.out_ch[, lp2]) names no instance of them.
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
#include "render_downmix.hpp"
#include "render_fir.hpp"
#include "render_fir16.hpp"
#include "render_fir_fft.hpp"
#include "render_fast.hpp"

// One element as LPCM packets: render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY, LPB, LPC>.  LPB: bytes per sample
// (2 or 3), LPC: the coupled form; early: the per-channel (per-pair) prefetch (pick_route says when).
template <class MList, class OCList, int LPB, bool LPC>
bool launch_fast_lp(const RenderParams &p, int m, bool early, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(OCList{}, p.out_ch, [&](auto OC) {
      constexpr int m_ = decltype(M)::value, oc_ = decltype(OC)::value;
      const size_t lds = sizeof(float) * (size_t)fast_lds_floats(oc_, m_);
      const dim3 grid((unsigned)p.n_launch);
      if (early) launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, false, true, true, LPB, LPC>, 80 * 1024>(grid, dim3(256), lds, st, p);
      else launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, false, true, false, LPB, LPC>, 80 * 1024>(grid, dim3(256), lds, st, p);
    });
  });
}

// Both elements of a mix as packets of LPB bytes per sample: render_fast_kernel<M, OC, 0, false, IN2 = true, LP = true,
// EARLY = true, LPB, LPC, LP2> with LP2 = lp2 out of KList.  LPC: element 0 is coupled.
template <class MList, class OCList, bool LPC, class KList, int LPB = 2>
bool launch_fast_lp_mix(const RenderMixParams &p, int m, int lp2, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(OCList{}, p.out_ch, [&](auto OC) {
      return dispatch(KList{}, lp2, [&](auto K) {
        constexpr int m_ = decltype(M)::value, oc_ = decltype(OC)::value, lp2_ = decltype(K)::value;
        constexpr size_t lds = sizeof(float) * (size_t)fast_lds_floats(oc_, m_);   // (the second element's matrix rows are in it)
        static_assert(lds * (LPB == 3 ? lpcm24_mix_wgs(m_, oc_, lp2_) : lpcm_mix_wgs(m_, oc_, lp2_)) <= 160 * 1024,
                      "the workgroups the instance is built for fit a CU's LDS");
        launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, true, true, true, LPB, LPC, lp2_>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
      });
    });
  });
}

// f32 of any call length: render_fast_kernel<M, OC, 0, false, false, false, true, 2, false, 0, IL, RAG = true>.  IL: ordinary
// interleaved sample-frames (iamf_render_interleaved.hip); else planar rows (iamf_render_ragged.hip)
template <class MList, class OCList, bool IL>
bool launch_fast_rag(const RenderParams &p, int m, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(OCList{}, p.out_ch, [&](auto OC) {
      constexpr int m_ = decltype(M)::value, oc_ = decltype(OC)::value;
      constexpr size_t lds = sizeof(float) * (size_t)fast_lds_floats(oc_, m_);
      // built for the four workgroups per CU of the planar f32 form <M, OC> (render_fast_kernel's launch bounds)
      static_assert(lds * 4 <= 160 * 1024, "the workgroups the instance is built for fit a CU's LDS");
      launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, false, false, true, 2, false, 0, IL, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
    });
  });
}

// One element as LPCM packets of any call length: render_fast_kernel<M, OC, 0, false, false, LP = true, EARLY = true, LPB, LPC,
// 0, IL = false, RAG = true> (iamf_render_packets_ragged*.hip).  LPB, LPC as launch_fast_lp; the early prefetch only.
template <class MList, class OCList, int LPB, bool LPC>
bool launch_fast_lp_rag(const RenderParams &p, int m, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(OCList{}, p.out_ch, [&](auto OC) {
      constexpr int m_ = decltype(M)::value, oc_ = decltype(OC)::value;
      constexpr size_t lds = sizeof(float) * (size_t)fast_lds_floats(oc_, m_);
      static_assert(lds * packets_ragged_wgs(m_, oc_, LPB, LPC) <= 160 * 1024, "the workgroups the instance is built for fit a CU's LDS");
      launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, false, true, true, LPB, LPC, 0, false, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
    });
  });
}

// Both elements of a mix as packets of any call length: render_fast_kernel<M, OC, 0, false, IN2 = true, LP = true, EARLY = true,
// LPB, LPC, LP2, IL = false, RAG = true> with LP2 = lp2 out of KList (iamf_render_packets_mix_ragged*.hip).  LPB, LPC, KList as
// launch_fast_lp_mix.
template <class MList, class OCList, bool LPC, class KList, int LPB>
bool launch_fast_lp_mix_rag(const RenderMixParams &p, int m, int lp2, hipStream_t st) {
  return dispatch(MList{}, m, [&](auto M) {
    return dispatch(OCList{}, p.out_ch, [&](auto OC) {
      return dispatch(KList{}, lp2, [&](auto K) {
        constexpr int m_ = decltype(M)::value, oc_ = decltype(OC)::value, lp2_ = decltype(K)::value;
        constexpr size_t lds = sizeof(float) * (size_t)fast_lds_floats(oc_, m_);   // (the second element's matrix rows are in it)
        static_assert(lds * packets_mix_ragged_wgs(m_, oc_, LPB, lp2_) <= 160 * 1024, "the workgroups the instance is built for fit a CU's LDS");
        launch_big_lds<&render_fast_kernel<m_, oc_, 0, false, true, true, true, LPB, LPC, lp2_, false, true>, 80 * 1024>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
      });
    });
  });
}

}  // namespace
