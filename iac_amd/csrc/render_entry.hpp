// render_entry.hpp — the launch entry points between the render translation units, each declared exactly once: the caller
// (iamf_render.hip) and the defining file both include this header at file scope, so a definition that drifts from its
// declaration does not compile.  Kernel and parameter types live in each unit's anonymous namespace (the kernels' symbol
// names depend on it), hence `const void *params`: the caller's RenderParams / FanParams, the same definition on both
// sides (render_params.hpp, render_fanout.hpp).  Each returns 1 if it launched, 0 if (m, the block's channel counts) is
// not in the instance list the caller has already consulted (render_route.hpp).  The units that feed render_fast_kernel
// another input form (the eighteen iamf_hip_fast_*_launch entries) share their launchers: render_fast_unit.hpp.  Behind the
// launch entries: the unpacker's, and the one entry through which every launcher counts what it ran (iamf_route.hip).
#pragma once

#define IAMF_INTERNAL extern "C" __attribute__((visibility("hidden")))

// iamf_render_wide4.hip: render_wide4_kernel<M, C>, its demixer and its down-mixer variant (by params->demix_on / dmx_on)
IAMF_INTERNAL int iamf_hip_wide4_launch(const void *params, int m, hipStream_t st);
// iamf_render_wide4_mix.hip, iamf_render_wide4_lfe.hip
IAMF_INTERNAL int iamf_hip_wide4_mix_launch(const void *params, int m, hipStream_t st);
IAMF_INTERNAL int iamf_hip_wide4_lfe_launch(const void *params, int m, hipStream_t st);
// iamf_render_fanout.hip; params: a FanParams whose first k members are set
IAMF_INTERNAL int iamf_hip_fanout_launch(const void *params, int m, int k, hipStream_t st);
// iamf_render_fanout_lp.hip; params: a FanLpParams whose first k members are set
IAMF_INTERNAL int iamf_hip_fanout_lp_launch(const void *params, int m, int k, hipStream_t st);
// iamf_render_fanout_pk24.hip, _fanout_pk16c.hip, _fanout_pk24c.hip: render_fanout_kernel<M, K, true, LPB, LPC>, the fan-out fed
// with 24-bit mono-coded, coupled 16-bit and coupled 24-bit packets; params as above, (m, k) in the unit's list
// (FanPk24MK, FanPk16cMK, FanPk24cMK of render_route.hpp)
IAMF_INTERNAL int iamf_hip_fanout_pk24_launch(const void *params, int m, int k, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fanout_pk16c_launch(const void *params, int m, int k, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fanout_pk24c_launch(const void *params, int m, int k, hipStream_t st);
// iamf_render_lpcm.hip; early: Route::variant of Family::Lpcm
IAMF_INTERNAL int iamf_hip_fast_lpcm_launch(const void *params, int m, int early, hipStream_t st);
// iamf_render_lpcm24.hip: the same for 24-bit samples (params->lpcm_bytes == 3); early: Route::variant of Family::Lpcm24
IAMF_INTERNAL int iamf_hip_fast_lpcm24_launch(const void *params, int m, int early, hipStream_t st);
// iamf_render_lpcm_coupled.hip: the same for the coupled 16-bit form (params->lpcm_coupled); early: Route::variant of
// Family::LpcmCoupled
IAMF_INTERNAL int iamf_hip_fast_lpcm_coupled_launch(const void *params, int m, int early, hipStream_t st);
// iamf_render_lpcm24_coupled.hip: the same for the coupled 24-bit form (params->lpcm_coupled == 2, lpcm_bytes == 3); early:
// Route::variant of Family::Lpcm24Coupled
IAMF_INTERNAL int iamf_hip_fast_lpcm24_coupled_launch(const void *params, int m, int early, hipStream_t st);
// iamf_render_lpcm_mix.hip, iamf_render_lpcm_mix_coupled.hip: both elements as 16-bit packets, element 0 mono-coded / coupled
// (params->lpcm_coupled); params: a RenderMixParams; lp2: Route::variant of Family::LpcmMix
IAMF_INTERNAL int iamf_hip_fast_lpcm_mix_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_lpcm_mix_coupled_launch(const void *params, int m, int lp2, hipStream_t st);
// iamf_render_lpcm24_mix.hip, iamf_render_lpcm24_mix_coupled.hip: the same with 24-bit packets on both elements
// (params->lpcm_bytes == 3, lpcm_mix == (4 | lp2), lpcm_coupled 0 / 2); lp2: Route::variant of Family::Lpcm24Mix
IAMF_INTERNAL int iamf_hip_fast_lpcm24_mix_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_lpcm24_mix_coupled_launch(const void *params, int m, int lp2, hipStream_t st);
// iamf_render_interleaved.hip: render_fast_kernel<M, OC, .., IL, RAG>, interleaved f32 of any call length (params->interleaved)
IAMF_INTERNAL int iamf_hip_fast_interleaved_launch(const void *params, int m, hipStream_t st);
// iamf_render_ragged.hip: render_fast_kernel<M, OC, .., IL = false, RAG>, planar f32 of any call length (params->ragged)
IAMF_INTERNAL int iamf_hip_fast_ragged_launch(const void *params, int m, hipStream_t st);
// iamf_render_packets_ragged.hip, _packets_ragged_coupled.hip, _packets_ragged24.hip, _packets_ragged24_coupled.hip:
// render_fast_kernel<M, OC, .., LP, true, LPB, LPC, 0, IL = false, RAG>, one element as packets of any call length
// (params->ragged == 2); the four single-element packet forms by params->lpcm_bytes (0 or 2 / 3) and params->lpcm_coupled (0 /
// 1 with 16-bit samples, 2 with 24-bit ones)
IAMF_INTERNAL int iamf_hip_fast_packets_ragged_launch(const void *params, int m, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_ragged_coupled_launch(const void *params, int m, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_ragged24_launch(const void *params, int m, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_ragged24_coupled_launch(const void *params, int m, hipStream_t st);
// iamf_render_packets_mix_ragged.hip, _packets_mix_ragged_coupled.hip, _packets_mix_ragged24.hip, _packets_mix_ragged24_coupled.hip:
// render_fast_kernel<M, OC, .., IN2, LP, true, LPB, LPC, LP2, IL = false, RAG>, both elements of a mix as packets of any call length
// (params->ragged == 3, params: RenderMixParams); the four two-element packet forms by params->lpcm_bytes and params->lpcm_coupled
// as above, lp2 = LP2
IAMF_INTERNAL int iamf_hip_fast_packets_mix_ragged_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_mix_ragged_coupled_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_mix_ragged24_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fast_packets_mix_ragged24_coupled_launch(const void *params, int m, int lp2, hipStream_t st);
// iamf_render_nolim_packets.hip, _nolim_packets24.hip: render_nolim_kernel<M, LPB, LPC> (render_nolim.hpp), the limiter-less
// renderer over one element's packets (params->ragged == 4); 16- / 24-bit samples by unit, mono-coded or coupled by
// params->lpcm_coupled (0 / 1 with 16-bit samples, 2 with 24-bit ones).  Their launcher: render_nolim_unit.hpp
IAMF_INTERNAL int iamf_hip_nolim_packets_launch(const void *params, int m, hipStream_t st);
IAMF_INTERNAL int iamf_hip_nolim_packets24_launch(const void *params, int m, hipStream_t st);
// iamf_render_nolim_packets_mix.hip, _nolim_packets24_mix.hip: render_nolim_kernel<M, LPB, LPC, LP2>, the same renderer over both
// elements' packets (params->ragged == 5; params a RenderMixParams); lp2 = the second element's form (LpcmMixK)
IAMF_INTERNAL int iamf_hip_nolim_packets_mix_launch(const void *params, int m, int lp2, hipStream_t st);
IAMF_INTERNAL int iamf_hip_nolim_packets24_mix_launch(const void *params, int m, int lp2, hipStream_t st);
// iamf_render_fir_m2b.hip: render_fast_kernel<M, 2, stage> / the FFT stage alone (fir_fft_kernel)
IAMF_INTERNAL int iamf_hip_fir_m2b_launch(const void *params, int m, int stage, hipStream_t st);
IAMF_INTERNAL int iamf_hip_fir_m2b_launch_fft(const void *params, int m, hipStream_t st);
// iamf_unpack.hip
IAMF_INTERNAL int iamf_hip_lpcm_unpack_frames(const iamf_hip_lpcm_layout *lay, const void *d_raw, int64_t raw_stream_stride,
                                              int64_t raw_frame_stride, int32_t n_frames, const int32_t *d_first_count,
                                              int64_t first_count_stride, float *d_out, int64_t out_stream_stride,
                                              int64_t out_frame_stride, int32_t n_streams, void *stream, int32_t uniform_first,
                                              int32_t uniform_count);
// iamf_route.hip: one launch of the instance (family, variant, m, c, k) of iamf_hip_route_row succeeded; set: the row set
// that lists it (RouteKey::set of render_route.hpp; 0: the base table, 1: the extension table).  The one counting entry:
// launch() and the two fan-out entries of iamf_render.hip and the resampler call it
IAMF_INTERNAL void iamf_hip_route_count(int set, int family, int variant, int m, int c, int k);
