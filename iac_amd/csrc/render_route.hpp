// render_route.hpp — which render kernels are instantiated, and which of them a call takes.  Plain C++ like
// render_params.hpp (included behind it, inside the unit's namespace; the unit includes <stdlib.h> and <type_traits> in
// front): the launchers of every translation unit walk these lists, the host asks them whether an instance exists, and
// pick_route() holds the whole routing decision, so that tests/test_route_host.py can pin it without a GPU.
#pragma once

#ifdef __HIPCC__
#define IAMF_HD __host__ __device__
#else
#define IAMF_HD
#endif

// ------------------------------------------------------------------------------------------
// instance lists
// ------------------------------------------------------------------------------------------

#include "instance_lists.hpp"
#include "resample_route.hpp"   // the resampler's instances are rows of the base table (for_each_instance_of_set)

// inputs of render_kernel (render_generic.hpp) and render_nolim_kernel.  11 inputs: no element of the reference has them,
// but the stage behind the resampler takes the OUTPUT layout's channels through the identity, and Sound System E has 11
// (found by tests/test_gpu_fuzz_facade.py: resampling into layout E was refused).  The general kernels only.
using GenericM = Ints<1, 2, 4, 6, 8, 9, 10, 11, 12, 14, 16, 24>;
using NolimM = GenericM;
using FastM = Ints<1, 2, 4, 6, 8, 9, 10, 12, 14, 16, 24>;   // render_fast_kernel<M, 1 | 2> and its mixing variant
using FastOC = Ints<1, 2>;
using WideM = FastM;                                        // render_wide_kernel<M, MFMA>
// render_fast_kernel<M, OC, 0, DOWN>, the parametric down-mixer to mono / stereo: 7.1 -> {2, 1}, 5.1 -> {2, 1}, stereo -> mono
using FastDownMC = Ints<mc(8, 2), mc(8, 1), mc(6, 2), mc(6, 1), mc(2, 1)>;
// render_wide4_kernel<M, C>: plain and MFMA projection (C = 14: Sound System G, 4+9+0)
using Wide4M = Ints<4, 6, 8, 9, 10, 12, 16>;
using Wide4C = Ints<6, 8, 10, 12, 14, 24>;
// its demixer variant: M = channels of the scalable element's target layout (5.1 .. 7.1.4)
using Wide4DemixM = Ints<6, 8, 10, 12>;
using Wide4DemixC = Ints<6, 8, 10, 12, 24>;
// its down-mixer variant: 7.1.4 -> {10, 8, 6}, 5.1.4 / 7.1.2 -> {8, 6}, 5.1.2 / 7.1 -> 6 channels
using Wide4DownMC = Ints<mc(12, 10), mc(12, 8), mc(12, 6), mc(10, 8), mc(10, 6), mc(8, 6)>;
// its mixing variant: Wide4M inputs of the first element
using Wide4MixC = Ints<6, 8, 10, 12>;
// its LFE variant: ambisonics elements of order 1..3, Wide4C outputs
using Wide4LfeM = Ints<4, 9, 16>;
// render_fanout_kernel<M, K>: ambisonics of order 1..3 and 5.1 / 7.1 / 7.1.4 into K members
using FanM = Ints<4, 6, 8, 9, 12, 16>;
using FanK = Ints<2, 3, 4>;
// render_fast_kernel<M, OC, .., LP>: mono-coded ambisonics elements as LPCM packets
using LpcmM = Ints<1, 4, 9, 16>;
using LpcmOC = Ints<1, 2>;
// render_fast_kernel<.., LP, EARLY, 2, LPC>: channel-based elements whose pairs are coupled sub-streams (lpcm_form.hpp,
// S16C) — stereo, 5.1, 5.1.2 / 7.1, 5.1.4 / 7.1.2, 7.1.4 — into LpcmOC
// (and, with 24-bit samples, render_fast_kernel<.., LP, EARLY, 3, LPC>: lpcm_form.hpp, S24C — the same lists)
using LpcmCoupledM = Ints<2, 6, 8, 10, 12>;
// The coupled form's pairing, a function of the channel count alone.  In the renderer's (playback) order every loudspeaker
// layout of LpcmCoupledM reads L R [C LFE, then pairs]: channels (0,1) are a coupled pair, 2 and 3 mono sub-streams,
// (4,5) .. (M-2, M-1) pairs again.  The form rule (lpcm_form.hpp) and the kernel (render_fast.hpp, LPC) both build on it.
IAMF_HD constexpr bool lpcm_coupled_m(int m_total) { return LpcmCoupledM::has(m_total); }
IAMF_HD constexpr bool lpcm_coupled_paired(int m_total, int m) { return m_total == 2 || m < 2 || m >= 4; }
// render_fast_kernel<.., LP2>: BOTH elements of a mix as 16-bit packets (iamf_hip_batch_render_lpcm_mix).  Element 0: LpcmM
// (mono-coded) or LpcmCoupledM (coupled); outputs LpcmOC; element 1: LP2 = 1 mono-coded runs (m2 = 1 or 4 at run time), 2 one
// coupled stereo pair (m2 == 2).
using LpcmMixK = Ints<1, 2>;
IAMF_HD constexpr bool lpcm_mix_m2_ok(int lp2, int m2) { return lp2 == 1 ? (m2 == 1 || m2 == 4) : (lp2 == 2 && m2 == 2); }
// Workgroups per CU the instance <M, OC, LP2> is built for: the highest of 4 / 3 / 2 at which the compiler reports no scratch
// and no vector spill.  Every one of the 36 instances fits four (at most 127 vector registers: <16, 2, 1>; DESIGN.md 4.1e has
// the table), where the f32 mixing variant is built for two; an instance that stops fitting gets its own answer here.
IAMF_HD constexpr int lpcm_mix_wgs(int m, int oc, int lp2) {
  (void)m, (void)oc, (void)lp2;
  return 4;
}
// render_fast_kernel<.., LP, true, 3, LPC, LP2>: both elements as 24-bit packets (iamf_hip_batch_render_packets_mix) — the same
// lists, element 1 of element 0's sample size.  Workgroups per CU the instance <M, OC, LP2> is built for, under the rule of
// lpcm_mix_wgs(): the highest of 4 / 3 / 2 at which the compiler reports no scratch and no vector spill (M tells the
// mono-coded element 0, LpcmM, from the coupled one, LpcmCoupledM: the lists share no number).  DESIGN.md 4.1i has the table.
// Five instances keep 12 to 92 bytes of scratch per lane at four (the 24-bit form holds a dword more per channel than the 16-bit
// one, whose <16, 2, 1> already uses 127 registers) and are built for three: <16, 2, 1>, <16, 2, 2>, <16, 1, 1>, <12, 2, 1>,
// <10, 2, 1>.
IAMF_HD constexpr int lpcm24_mix_wgs(int m, int oc, int lp2) {
  if (m == 16 && (oc == 2 || lp2 == 1)) return 3;
  if ((m == 12 || m == 10) && oc == 2 && lp2 == 1) return 3;
  return 4;
}
// render_fast_kernel<.., LP, true, LPB, LPC, 0, IL = false, RAG = true>: one element as packets of any call length
// (iamf_hip_batch_render_packets_ragged) — LpcmM (mono-coded) or LpcmCoupledM (coupled) x LpcmOC x {16, 24 bit}, the early
// prefetch only.  Workgroups per CU the instance <M, OC, LPB, LPC> is built for, under the rule of lpcm_mix_wgs(): the highest of
// 4 / 3 / 2 at which the compiler reports no scratch and no vector spill.  Every one of the 36 instances fits four (at most
// 111 vector registers: <16, 2, LPB = 3>; DESIGN.md 4.1j has the table); an instance that stops fitting gets its own answer here.
IAMF_HD constexpr int packets_ragged_wgs(int m, int oc, int lpb, bool lpc) {
  (void)m, (void)oc, (void)lpb, (void)lpc;
  return 4;
}
// render_fast_kernel<.., IN2, LP, true, LPB, LPC, LP2, IL = false, RAG = true>: both elements of a mix as packets of any call length
// (iamf_hip_batch_render_packets_mix_ragged) — (LpcmM + LpcmCoupledM) x LpcmOC x LpcmMixK x {16, 24 bit}, 72 instances.
// Workgroups per CU the instance <M, OC, LPB, LP2> is built for, under the rule of lpcm_mix_wgs(): the highest of 4 / 3 / 2 at
// which the compiler reports no scratch and no vector spill (M tells the mono-coded element 0 from the coupled one).  DESIGN.md
// 4.1k has the table.  The 36 16-bit instances all fit four (at most 127 vector registers: <16, 2, 2, 1>).  Of the 24-bit ones,
// six keep 12 to 116 bytes of scratch per lane at four and are built for three, without scratch: the five that
// lpcm24_mix_wgs() builds for three — <16, 2, 3, 1>, <16, 2, 3, 2>, <16, 1, 3, 1>, <12, 2, 3, 1>, <10, 2, 3, 1> — and
// <16, 1, 3, 2>, which the ragged form's tail (the select, the ramps' single loads) pushes over by 32 bytes.
IAMF_HD constexpr int packets_mix_ragged_wgs(int m, int oc, int lpb, int lp2) {
  if (lpb == 3 && m == 16) return 3;
  if (lpb == 3 && (m == 12 || m == 10) && oc == 2 && lp2 == 1) return 3;
  return 4;
}
// render_fast_kernel<.., IL, RAG>: ordinary interleaved f32 of any call length (iamf_hip_batch_render_interleaved): the stage
// behind the resampler, mono or stereo in and out
using InterleavedM = Ints<1, 2>;
using InterleavedOC = Ints<1, 2>;
// render_fast_kernel<.., IL = false, RAG = true>: planar f32 of any call length (iamf_hip_batch_render_ragged) — the element
// shapes LPCM streams take, LpcmM and LpcmCoupledM together (a live service renders what it decodes, frame by frame)
using RaggedM = Ints<1, 2, 4, 6, 8, 9, 10, 12, 16>;
using RaggedOC = Ints<1, 2>;
// render_fanout_kernel<M, K, LP>: the fan-out fed with LPCM packets.  M: what LpcmM and FanM share (mono-coded ambisonics
// elements are the only ones whose channels are contiguous 16-bit runs), K within FanK
using FanLpM = Ints<4, 9, 16>;
using FanLpK = Ints<2, 3, 4>;
// render_fanout_kernel<M, K, LP, LPB, LPC>: the fan-out fed with the other three packet forms of lpcm_form.hpp
// (iamf_hip_batch_render_fanout_packets), one list of (M, K) pairs — mc(m, k) — per form and translation unit: 24-bit
// mono-coded ambisonics (S24: FanLpM), coupled 5.1 / 7.1 / 5.1.4 / 7.1.4 with 16-bit (S16C) and 24-bit samples (S24C), K within
// FanK.  Stereo is left out: its 4 or 6 bytes per sample-frame are less than what its members write.  Every instance listed
// runs without scratch and without a vector spill under the kernel's launch bounds (DESIGN.md 4.1n has the table); one that
// stops doing so is taken out of its list here, and the listing, the host rule and the tests follow.
using FanPk24MK = Ints<mc(4, 2), mc(4, 3), mc(4, 4), mc(9, 2), mc(9, 3), mc(9, 4), mc(16, 2), mc(16, 3), mc(16, 4)>;
using FanPk16cMK = Ints<mc(6, 2), mc(6, 3), mc(6, 4), mc(8, 2), mc(8, 3), mc(8, 4), mc(10, 2), mc(10, 3), mc(10, 4), mc(12, 2), mc(12, 3), mc(12, 4)>;
using FanPk24cMK = FanPk16cMK;
// variant of an IAMF_HIP_ROUTE_FANOUT_PACKETS row: bit 0 = 24-bit samples, bit 1 = coupled pairs (1 / 2 / 3 = S24 / S16C / S24C)
IAMF_HD constexpr int fan_pk_variant(int lpb, bool lpc) { return (lpb == 3 ? 1 : 0) | (lpc ? 2 : 0); }
// whether the form `variant` has an instance for an element of m channels into k members
IAMF_HD constexpr bool fan_pk_has(int variant, int m, int k) {
  return variant == 1 ? FanPk24MK::has(mc(m, k)) : (variant == 2 ? FanPk16cMK::has(mc(m, k)) : (variant == 3 && FanPk24cMK::has(mc(m, k))));
}
// the HRTF stage: ambisonics elements (iamf_render.hip) and channel-based ones, the loudspeaker layouts' channel counts
// (iamf_render_fir_m2b.hip)
using FirHomeM = Ints<1, 4, 9, 16>;
using FirM2bM = Ints<2, 6, 8, 10, 12>;

// ------------------------------------------------------------------------------------------
// what the routing decision needs of the kernels' geometry
// ------------------------------------------------------------------------------------------

constexpr int kFWin = 1088;    // render_fast.hpp: staged limiter-table window / head length (> chunk + 1), multiple of 64
constexpr int kFIn2 = 4;       // channels of a second element the mixing variants take (render_fast.hpp, IN2)

// render_wide.hpp
constexpr int kWChunk = 256;
constexpr int kWPos = 512;   // ring positions (power of two >= chunk + look-ahead + 15)
constexpr int kWWin = 320;   // staged table window / head length (> chunk + 1)

IAMF_HD constexpr int wide_lds_floats(int c, int m) {
  return kWPos * c + 2 * kWPos + kWPos / 16 + 3 * kWChunk + 2 * kWWin + ((c + 3) & ~3) * m + 16;
}

// render_nolim.hpp (both kernels)
constexpr int kNlChunk = 1024;                       // sample-frames per workgroup
constexpr int kNlMaxFrameBytes = 60;                 // out_ch * bytes per sample-frame the LDS tile takes (60 KiB)

// ------------------------------------------------------------------------------------------
// what the shape rules share: each check stated once.  A wrong answer here is a misaligned or stray load on the GPU, not a
// slower rate (tests/route_host pins every rule, tests/route_host/route_host_sweep_check.cpp the whole decision)
// ------------------------------------------------------------------------------------------

inline bool on_grid16(const void *ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }
// PCM rows on the 16-byte grid: every kernel but the general one stores a lane's sample-frames as whole 16-byte pieces
inline bool pcm_rows_ok(const RenderParams &p) { return on_grid16(p.pcm) && !(p.pcm_stream_stride & 15); }
// per-sample gains, where given: rows on the 16-byte grid with a stride that is a multiple of 4 (one float4 per lane)
inline bool ramp_quads_ok(const RenderParams &p) {
  if (!p.elem_ramp && !p.elem2_ramp && !p.out_ramp) return true;
  return !(p.ramp_stream_stride & 3) && on_grid16(p.elem_ramp) && on_grid16(p.elem2_ramp) && on_grid16(p.out_ramp);
}
// the stream position of a kernel that places its ring per call (render_fast.hpp `base`, render_wide4.hpp): a multiple of 16,
// or — a trimmed first frame — any position from 240 samples on
inline bool pos_ok(const RenderParams &p) { return !(p.pos0 & 15) || p.pos0 >= kDelay; }
// the fast kernel addresses a stream's packets of one call with 32-bit byte offsets (buffer loads, render_fast.hpp): the
// call's frames and two more at `frame_stride` bytes, and 2^24 bytes for what one frame's runs span, stay below 2^31
inline bool packet_offsets32_ok(const RenderParams &p, int64_t frame_stride) {
  return ((int64_t)p.total / p.frame_size + 2) * frame_stride + ((int64_t)1 << 24) < (int64_t)1 << 31;
}
// the same for planar f32 rows, the stride in floats
inline bool f32_offsets32_ok(const RenderParams &p) {
  return ((int64_t)p.total / p.frame_size + 2) * p.in_frame_stride * 4 + 100 * (int64_t)p.frame_size < (int64_t)1 << 31;
}
// the grid of a packet form as a mask (lpcm_form.hpp: 8 bytes for 16-bit samples, 4 for 24-bit ones) and its sample size
inline int lpcm_grid(const RenderParams &p) { return p.lpcm_bytes == 3 ? 3 : 7; }
inline int lpcm_sample_bytes(const RenderParams &p) { return p.lpcm_bytes == 3 ? 3 : 2; }
// one element's packets: the buffer on 16 bytes, both strides on the form's grid, frames one behind the other
inline bool packet_rows_ok(const void *raw, int64_t stream_stride, int64_t frame_stride, int grid) {
  return on_grid16(raw) && !(stream_stride & grid) && !(frame_stride & grid) && frame_stride > 0;
}
// Element 0's packets have one of the four forms the marked packet rules read: 16-bit mono-coded (LpcmM), 16-bit coupled
// (lpcm_coupled == 1), 24-bit mono-coded, 24-bit coupled (== 2), with an instance for m, on the form's grid — the rows and every
// run's start, first_sample included; a pair's second channel lies one sample behind its first, the pair's one run starts at the
// first.  zero_is_16: the rule reads lpcm_bytes == 0 as 16 bit (the ragged forms; the limiter-less ones require 2).
inline bool lpcm_elem0_form_ok(const RenderParams &p, int m, bool zero_is_16) {
  if (p.lpcm_bytes != 3 && p.lpcm_bytes != 2 && !(zero_is_16 && p.lpcm_bytes == 0)) return false;
  if (p.lpcm_coupled != 0 && p.lpcm_coupled != (p.lpcm_bytes == 3 ? 2 : 1)) return false;
  if (!(p.lpcm_coupled ? LpcmCoupledM::has(m) : LpcmM::has(m))) return false;
  const int grid = lpcm_grid(p);
  if (!packet_rows_ok(p.lpcm, p.lpcm_stream_stride, p.lpcm_frame_stride, grid)) return false;
  for (int c = 0; c < m; ++c) {
    if (p.lpcm_coupled && lpcm_coupled_paired(m, c) && (c & 1)) {
      if (p.lpcm_off[c] != p.lpcm_off[c - 1] + lpcm_sample_bytes(p)) return false;
    } else if (p.lpcm_off[c] < 0 || (p.lpcm_off[c] & grid)) return false;
  }
  return true;
}
// lpcm_mix names element 1's form (LP2, or 4 | LP2 with 24-bit samples) of element 0's sample size, and the second element given
// has a channel count that form takes
inline bool lpcm_mix_form_ok(const RenderParams &p) {
  const int lp2 = p.lpcm_mix & 3;
  return p.lpcm_mix == ((p.lpcm_bytes == 3 ? 4 : 0) | lp2) && LpcmMixK::has(lp2) && p.in2 && lpcm_mix_m2_ok(lp2, p.m2);
}
// A trimmed frame (`first`, iamf_hip_lpcm_input::first_sample, is call_first_sample(p): one for both elements of a mix): only a
// call shorter than a frame has one, and every quad that starts below `total` ends inside the run of frame_size samples.
// round_up: the kernel's last quad may be ragged, so the total counts rounded up to a quad (the ragged forms); else the rule has
// asked for whole quads, and no byte outside the samples of the call is read (the limiter-less forms).
inline bool trimmed_frame_ok(const RenderParams &p, bool round_up) {
  const int first = call_first_sample(p);
  if (first < 0 || (first > 0 && p.total >= p.frame_size)) return false;
  return p.total >= p.frame_size || (int64_t)first + (round_up ? (p.total + 3) & ~3 : p.total) <= p.frame_size;
}
// what the LDS tile of render_nolim.hpp takes: a lane's 4 sample-frames are whole 16-byte pieces, a sample-frame at most 60 bytes
inline bool nolim_frame_bytes_ok(const RenderParams &p) {
  const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
  return !((p.out_ch * bytes) & 3) && p.out_ch * bytes <= kNlMaxFrameBytes;
}
// the early per-channel prefetch of a whole-block packet form: as measured per size (the form's *_early), unless
// IAMF_HIP_LP_LATE=1 forces the late variant or IAMF_HIP_LP_EARLY=1 the early one
inline bool lp_early_variant(bool measured_early) { return !getenv("IAMF_HIP_LP_LATE") && (getenv("IAMF_HIP_LP_EARLY") || measured_early); }

// what render_nolim_kernel's addressing needs; the caller has checked that the call is of the plain kind
inline bool nolim_shape_ok(const RenderParams &p) {
  if ((p.frame_size & 3) || (p.total & 3) || p.total <= 0) return false;
  if (!on_grid16(p.in) || (p.in_stream_stride & 3) || (p.in_frame_stride & 3)) return false;
  return pcm_rows_ok(p) && nolim_frame_bytes_ok(p);
}

// What the packet-fed form of the limiter-less renderer (render_nolim.hpp, render_nolim_kernel) needs of a call that came
// through iamf_hip_batch_render_packets_nolim (kCallPacketsNolim, which that entry alone sets): the plain kind render_nolim_kernel
// takes (pick_route's Family::Nolim rule: limiter off, one matrix-rendered element, no second element, ramps, down-mixer, demixer,
// pre-matrix, HRTF stage or LFE generator, no reduced out_gain_channels); element 0's form (lpcm_elem0_form_ok, lpcm_bytes == 2 or
// 3); frame size and the call's samples per stream multiples of 4 and at least 4, so that a lane's quad never straddles a frame;
// a trimmed frame inside its run (trimmed_frame_ok, whole quads); PCM rows and a sample-frame the tile takes, as nolim_shape_ok
// has it.  The kernel addresses with 64-bit pointers: no bound on the call's extent, no n_end, no rule on the position.
// IAMF_HIP_NOLIM_PACKETS_UNFUSED=1, IAMF_HIP_LPCM_UNFUSED=1 and IAMF_HIP_FORCE_GENERIC=1 send every such call down the other rules.
inline bool nolim_packets_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (p.ragged != kCallPacketsNolim || !p.lpcm || force_generic || getenv("IAMF_HIP_NOLIM_PACKETS_UNFUSED") || getenv("IAMF_HIP_LPCM_UNFUSED")) return false;
  if (p.limiter_on || !p.in || p.og_ch < p.out_ch) return false;
  if (p.in2 || p.lpcm_mix || p.elem_ramp || p.elem2_ramp || p.out_ramp || p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe)
    return false;
  if (p.total < 4 || (p.total & 3) || p.frame_size < 4 || (p.frame_size & 3)) return false;
  if (!pcm_rows_ok(p) || p.out_ch < 1 || !nolim_frame_bytes_ok(p)) return false;
  return lpcm_elem0_form_ok(p, m, false) && trimmed_frame_ok(p, false);
}

// What the two-element packet form of the limiter-less renderer (render_nolim_kernel<M, LPB, LPC, LP2>) needs of a call that came
// through iamf_hip_batch_render_packets_mix_nolim (kCallPacketsMixNolim, which that entry alone sets, on a RenderMixParams):
// everything nolim_packets_shape_ok asks, with a second element given as packets in place of "no second element, no ramps" —
// lpcm_mix names its form (lpcm_mix_form_ok); pick_route's fields and the kernel's (the block behind RenderParams) agree; element 1
// on element 0's grid: its rows, every run's start with first_sample counted in, and a pair's partner one sample behind — and
// ramps, where given, as ramp_quads_ok has them.  The trimmed frame's rule holds for both elements (one first_sample).
// IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED=1, IAMF_HIP_LPCM_UNFUSED=1 and IAMF_HIP_FORCE_GENERIC=1 send every such call down the other rules.
inline bool nolim_packets_mix_shape_ok(const RenderMixParams &p, int m, bool force_generic) {
  if (p.ragged != kCallPacketsMixNolim || !p.lpcm || force_generic || getenv("IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED") || getenv("IAMF_HIP_LPCM_UNFUSED")) return false;
  if (p.limiter_on || !p.in || p.og_ch < p.out_ch) return false;
  if (p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe) return false;
  if (p.total < 4 || (p.total & 3) || p.frame_size < 4 || (p.frame_size & 3)) return false;
  if (!pcm_rows_ok(p) || p.out_ch < 1 || !nolim_frame_bytes_ok(p)) return false;
  if (!lpcm_elem0_form_ok(p, m, false) || !lpcm_mix_form_ok(p)) return false;
  // element 1: where pick_route's fields and the kernel's agree, on element 0's grid
  const int grid = lpcm_grid(p);
  if (!p.lpcm2 || reinterpret_cast<const uint8_t *>(p.in2) != p.lpcm2 || !p.matrix2 || !p.src_feed2 || !p.gains2) return false;
  if (p.in2_stream_stride != p.lpcm2_stream_stride || p.in2_frame_stride != p.lpcm2_frame_stride) return false;
  if (!packet_rows_ok(p.lpcm2, p.lpcm2_stream_stride, p.lpcm2_frame_stride, grid)) return false;
  if ((p.lpcm_mix & 3) == 2) {
    if (p.lpcm2_off[0] < 0 || (p.lpcm2_off[0] & grid) || p.lpcm2_off[1] != p.lpcm2_off[0] + lpcm_sample_bytes(p)) return false;
  } else {
    for (int c = 0; c < p.m2; ++c)
      if (p.lpcm2_off[c] < 0 || (p.lpcm2_off[c] & grid)) return false;
  }
  return ramp_quads_ok(p) && trimmed_frame_ok(p, false);
}

// which HRTF stage a FIR call runs (host): 3 = overlap-save FFT (default), 2 = split-f16 MFMA, 1 = f32 MFMA
// 4 = the FFT stage as a kernel of its own + the two-channel matrix kernel behind it (default); IAMF_HIP_FIR_FUSED=1 keeps
// the FFT stage inside render_fast_kernel<M, 2, 3> (one pass over HBM, but the hops of a stream run one pass after the other
// and the limiter stages at two workgroups per CU: 29 instead of the split's rate, NOTEBOOK.md 4.2c)
inline int fir_stage_choice(const RenderParams &p) {
  if (getenv("IAMF_HIP_FIR_F32")) return 1;
  if (getenv("IAMF_HIP_FIR_F16") && p.fir_h16) return 2;
  if (p.fir_pq && p.fir_tw && p.fir_zero && (p.frame_size & 63) == 0)   // its input runs of 64 must not straddle frames
    return (p.fir_y && p.fir_id_matrix && !getenv("IAMF_HIP_FIR_FUSED")) ? 4 : 3;
  return p.fir_h16 ? 2 : 1;
}

// ------------------------------------------------------------------------------------------
// the routing decision
// ------------------------------------------------------------------------------------------

// What the fast kernel's addressing needs: aligned, limiter-on calls into 1- or 2-channel layouts; everything else (odd
// sizes, flush, limiter off, wide layouts) goes to the generic kernel.  Both are exact.  (Not looked at here: the
// parametric down-mixer, which only the DOWN variant takes — pick_route.)
inline bool fast_shape_ok(const RenderParams &p, bool force_generic) {
  if (force_generic || p.og_ch < p.out_ch) return false;
  if (!p.limiter_on || !p.in || p.out_ch > 2 || p.n_end < kFWin) return false;
  if (p.pre_matrix || p.demix_on) return false;
  if (p.elem_ramp || p.elem2_ramp || p.out_ramp) {  // per-sample gains: the mixing variant reads them 4 at a time
    if (p.dmx_on || p.fir_taps > 0 || (p.elem2_ramp && !p.in2) || !ramp_quads_ok(p)) return false;
  }
  if (p.in2 && (p.dmx_on || p.fir_taps > 0 || p.m2 > kFIn2 || !on_grid16(p.in2) || (p.in2_stream_stride & 3) || (p.in2_frame_stride & 3)))
    return false;  // a second element of up to 4 channels rides along (render_fast_kernel<.., IN2>)
  if (!pos_ok(p) || (p.total & 63) || (p.frame_size & 3)) return false;
  if (!on_grid16(p.in) || (p.in_stream_stride & 3) || (p.in_frame_stride & 3)) return false;
  if (!pcm_rows_ok(p)) return false;
  // the kernel addresses a stream's input of one call with 32-bit byte offsets
  return f32_offsets32_ok(p) && (!p.lpcm || packet_offsets32_ok(p, p.lpcm_frame_stride));
}

// What the interleaved, ragged form of the fast kernel (render_fast.hpp, IL and RAG) needs of a call that came through
// iamf_hip_batch_render_interleaved: one matrix-rendered element of one or two channels with constant gains into one or two
// channels with the limiter on, dense sample-frames on the 16-byte grid, any length.  The position as fast_shape_ok wants
// it: a multiple of 16, or 240 samples on (the ring is placed per call).  IAMF_HIP_INTERLEAVED_UNFUSED=1 sends every such
// call down the rules below, as does a zero `interleaved`.
inline bool interleaved_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (!p.interleaved || force_generic || getenv("IAMF_HIP_INTERLEAVED_UNFUSED")) return false;
  if (!p.limiter_on || !p.in || !InterleavedOC::has(p.out_ch) || !InterleavedM::has(m) || p.og_ch < p.out_ch || p.n_end < kFWin) return false;
  if (p.in2 || p.elem_ramp || p.elem2_ramp || p.out_ramp || p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe || p.lpcm)
    return false;
  if (p.frame_size != 1 || p.in_frame_stride != m) return false;   // dense: sample-frame k of the call at float k * m
  if (!on_grid16(p.in) || (p.in_stream_stride & 3) || !pcm_rows_ok(p) || !pos_ok(p)) return false;
  // the kernel addresses a stream's input of one call with 32-bit byte offsets, and its buffer resource ends with the call
  if (p.total < 1 || (int64_t)p.total * m * 4 + ((int64_t)1 << 24) >= (int64_t)1 << 31) return false;
  return true;
}

// What the planar ragged form of the fast kernel (render_fast.hpp, RAG without IL) needs of a call that came through
// iamf_hip_batch_render_ragged: fast_shape_ok's rule for the plain matrix variant — one matrix-rendered element with constant
// gains into one or two channels, limiter on, planar rows on the 16-byte grid — with "whole 64-sample blocks" replaced by
// "any length >= 1 that is NOT a whole number of blocks".  A call of whole blocks is left to the rules below (Family::Fast
// and so on), as is every call with a zero `ragged`.  What keeps the kernel's loads inside the frames' rows: frame_size is a
// multiple of 4 and a call's total is n_frames * frame_size or an n_samples <= frame_size, so a lane's quad that starts
// below `total` ends inside its row (iamf_render_ragged.hip).  IAMF_HIP_RAGGED_UNFUSED=1 sends every such call down the
// rules below.
inline bool ragged_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (p.ragged != kCallRagged || force_generic || getenv("IAMF_HIP_RAGGED_UNFUSED")) return false;
  if (!p.limiter_on || !p.in || !RaggedOC::has(p.out_ch) || !RaggedM::has(m) || p.og_ch < p.out_ch || p.n_end < kFWin) return false;
  if (p.in2 || p.elem_ramp || p.elem2_ramp || p.out_ramp || p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe || p.lpcm)
    return false;
  if (p.total < 1 || !(p.total & 63) || (p.frame_size & 3) || !pos_ok(p)) return false;
  if (!on_grid16(p.in) || (p.in_stream_stride & 3) || (p.in_frame_stride & 3) || !pcm_rows_ok(p)) return false;
  return f32_offsets32_ok(p);   // 32-bit byte offsets: fast_shape_ok's bound
}

// What the ragged packet form of the fast kernel (render_fast.hpp, RAG with LP) needs of a call that came through
// iamf_hip_batch_render_packets_ragged (kCallPacketsRagged, which that entry alone sets): everything fast_shape_ok asks of a
// single packet-fed element, with "whole 64-sample blocks" replaced by "any length >= 1 that is NOT a whole number of blocks";
// element 0's form (lpcm_elem0_form_ok; lpcm_bytes == 0 reads as 16 bit, as the whole-block families read it); a trimmed frame
// inside its run with the total rounded up to a quad (trimmed_frame_ok); the packets inside the kernel's 32-bit offsets.  A call
// of whole blocks, and every call this rule does not take, is left to the rules below.  IAMF_HIP_PACKETS_RAGGED_UNFUSED=1 sends
// every such call down them.
inline bool packets_ragged_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (p.ragged != kCallPacketsRagged || !p.lpcm || force_generic || getenv("IAMF_HIP_PACKETS_RAGGED_UNFUSED")) return false;
  if (!p.limiter_on || !p.in || !LpcmOC::has(p.out_ch) || p.og_ch < p.out_ch || p.n_end < kFWin) return false;
  if (p.in2 || p.lpcm_mix || p.elem_ramp || p.elem2_ramp || p.out_ramp || p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe)
    return false;
  if (p.total < 1 || !(p.total & 63) || p.frame_size < 4 || (p.frame_size & 3) || !pos_ok(p)) return false;
  if (!on_grid16(p.in) || !pcm_rows_ok(p)) return false;
  return lpcm_elem0_form_ok(p, m, true) && trimmed_frame_ok(p, true) && packet_offsets32_ok(p, p.lpcm_frame_stride);
}

// What the ragged two-element packet form of the fast kernel (render_fast.hpp, RAG with LP and LP2) needs of a call that came
// through iamf_hip_batch_render_packets_mix_ragged (kCallPacketsMixRagged, which that entry alone sets): everything
// packets_ragged_shape_ok asks, with a second element given as packets in place of "no second element, no ramps" — lpcm_mix names
// its form (lpcm_mix_form_ok); its rows on element 0's grid (its run starts travel behind this block, RenderMixParams::lpcm2_off,
// and are held to the same grid by the form check that let the call come here, lpcm_form.hpp) and inside the same 32-bit bound —
// and ramps, where given, as ramp_quads_ok has them (the call's last quad is read float by float).  The trimmed frame's rule holds
// for both elements (one first_sample).  A call of whole blocks, and every call this rule does not take, is left to the rules
// below.  IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED=1 sends every such call down them.
inline bool packets_mix_ragged_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (p.ragged != kCallPacketsMixRagged || !p.lpcm || force_generic || getenv("IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED")) return false;
  if (!p.limiter_on || !p.in || !LpcmOC::has(p.out_ch) || p.og_ch < p.out_ch || p.n_end < kFWin) return false;
  if (p.dmx_on || p.demix_on || p.pre_matrix || p.fir_taps > 0 || p.lfe) return false;
  if (p.total < 1 || !(p.total & 63) || p.frame_size < 4 || (p.frame_size & 3) || !pos_ok(p)) return false;
  if (!on_grid16(p.in) || !pcm_rows_ok(p)) return false;
  if (!lpcm_elem0_form_ok(p, m, true) || !lpcm_mix_form_ok(p)) return false;
  if (!packet_rows_ok(p.in2, p.in2_stream_stride, p.in2_frame_stride, lpcm_grid(p))) return false;
  if (!ramp_quads_ok(p) || !trimmed_frame_ok(p, true)) return false;
  return packet_offsets32_ok(p, p.lpcm_frame_stride) && packet_offsets32_ok(p, p.in2_frame_stride);
}

// What the wide kernels (render_wide.hpp, render_wide4.hpp) share: 3..24 output channels, limiter on, aligned calls.
// (Not looked at here: the stream position and the stages in front — demixer, down-mixer, mixer — which differ
// between the two: pick_route.)
inline bool wide_shape_ok(const RenderParams &p, int m, bool force_generic) {
  if (force_generic || p.og_ch < p.out_ch) return false;
  if (!p.limiter_on || !p.in || p.out_ch <= 2 || p.out_ch > kMaxOut || p.n_end < kWWin) return false;
  if (p.pre_matrix) return false;
  if ((p.total & 63) || !pcm_rows_ok(p)) return false;
  return sizeof(float) * (size_t)wide_lds_floats(p.out_ch, m) <= 80 * 1024;
}

// What the 4-samples-per-lane wide kernel (render_wide4.hpp) needs on top: 16-bit PCM, whole 1024-sample chunks,
// 16-byte aligned planar input (and second element and ramps, for the mixing variant).
inline bool wide4_shape_ok(const RenderParams &p, bool mixing) {
  if (getenv("IAMF_HIP_NO_WIDE4")) return false;
  // whole 1024-sample chunks; the last one may be short if it still holds the 256 samples of stream state
  if (p.out_format != IAMF_HIP_FMT_S16 || ((p.total & 1023) && (p.total & 1023) < 256) ||
      (p.frame_size & 3) || p.n_end < 1088)
    return false;
  if ((reinterpret_cast<uintptr_t>(p.in) & 15) || (p.in_stream_stride & 3) || (p.in_frame_stride & 3)) return false;
  if (mixing) {  // the mixing variant (render_wide4.hpp, MIX)
    if (p.in2 && (p.m2 > kFIn2 || (reinterpret_cast<uintptr_t>(p.in2) & 15) || (p.in2_stream_stride & 3) ||
                  (p.in2_frame_stride & 3)))
      return false;
    if ((p.ramp_stream_stride & 3) || (p.elem2_ramp && !p.in2) ||
        ((reinterpret_cast<uintptr_t>(p.elem_ramp) | reinterpret_cast<uintptr_t>(p.elem2_ramp) |
          reinterpret_cast<uintptr_t>(p.out_ramp)) & 15))
      return false;
  }
  return true;
}

// Kernel families (all share the persisted per-stream state, so consecutive calls of one stream may take different
// ones) and, per family, what Route::variant says.
enum class Family {
  Refused,      // no kernel takes the call: Route::err
  Lpcm,         // render_fast_kernel<.., LP>; variant 1: the early per-channel prefetch, 0: the late one
  FirSplit,     // fir_fft_kernel, then render_fast_kernel<2, 2> with the identity over its output
  FirFused,     // render_fast_kernel<M, 2, FIR>; variant = FIR: 3 FFT, 2 split-f16 MFMA, 1 f32 MFMA
  FastDown,     // render_fast_kernel<M, OC, 0, DOWN>
  Wide4Lfe,     // render_wide4_kernel<.., LFE>; variant 1: MFMA projection          } iamf_render_wide4_lfe.hip
  Wide4,        // render_wide4_kernel<M, C>; variant 1: MFMA projection             } iamf_render_wide4.hip
  Wide4Demix,   // render_wide4_kernel<.., DMX>                                      }
  Wide4Down,    // render_wide4_kernel<.., DOWN>                                     }
  Wide4Mix,     // render_wide4_kernel<.., MIX>; variant 1: MFMA projection          } iamf_render_wide4_mix.hip
  Nolim,        // render_nolim_kernel<M>
  Fast,         // render_fast_kernel<M, OC>; variant 1: the mixing one (IN2)
  Wide,         // render_wide_kernel<M, MFMA>; variant 1: MFMA projection
  Generic,      // render_kernel<M>
  // The families below are listed in row sets of their own (for_each_instance_of_set, RouteKey::set): the base table's row
  // set is pinned, and so are those of the numbered tables, of which there stay three.
  Lpcm24,       // render_fast_kernel<.., LP, EARLY, LPB = 3> (iamf_render_lpcm24.hip); variant as Lpcm.  Set 2, which is table 2
                // of iamf_hip_route_table_instances
  LpcmCoupled,  // render_fast_kernel<.., LP, EARLY, 2, LPC> (iamf_render_lpcm_coupled.hip); variant as Lpcm.  Set 3: behind the
                // numbered tables, listed by iamf_hip_route_family_instances only
  LpcmMix,      // render_fast_kernel<.., LP, true, 2, LPC, LP2> (iamf_render_lpcm_mix.hip, iamf_render_lpcm_mix_coupled.hip): both
                // elements of a mix as 16-bit packets; variant = LP2 (1 mono-coded second element, 2 a coupled pair).  Set 4,
                // listed by family only
  FastInterleaved,  // render_fast_kernel<M, OC, .., IL, RAG> (iamf_render_interleaved.hip): interleaved f32 of any call length,
                // RenderParams::interleaved.  Set 5, listed by family only
  FastRagged,   // render_fast_kernel<M, OC, .., IL = false, RAG = true> (iamf_render_ragged.hip): planar f32 of any call length that
                // is no whole number of 64-sample blocks, RenderParams::ragged.  Set 6, listed by family only
  Lpcm24Coupled,  // render_fast_kernel<.., LP, EARLY, 3, LPC> (iamf_render_lpcm24_coupled.hip): RenderParams::lpcm_coupled == 2,
                // which only iamf_hip_batch_render_packets sets; variant as Lpcm.  Set 7, listed by family only
  Lpcm24Mix,    // render_fast_kernel<.., LP, true, 3, LPC, LP2> (iamf_render_lpcm24_mix.hip, iamf_render_lpcm24_mix_coupled.hip): both
                // elements of a mix as 24-bit packets, RenderParams::lpcm_mix == (4 | LP2), which only
                // iamf_hip_batch_render_packets_mix sets; variant = LP2.  Set 8, listed by family only
  PacketsRagged,  // render_fast_kernel<.., LP, true, LPB, LPC, 0, false, RAG = true> (iamf_render_packets_ragged*.hip): one element as
                // packets of any call length that is no whole number of 64-sample blocks, kCallPacketsRagged, which only
                // iamf_hip_batch_render_packets_ragged sets; variant 0.  Set 9, listed by family only
  PacketsMixRagged,  // render_fast_kernel<.., IN2, LP, true, LPB, LPC, LP2, false, RAG = true> (iamf_render_packets_mix_ragged*.hip):
                // both elements of a mix as packets of any call length that is no whole number of 64-sample blocks,
                // kCallPacketsMixRagged, which only iamf_hip_batch_render_packets_mix_ragged sets; variant = LP2.  Set 10, listed by
                // family only
  NolimPackets,  // render_nolim_kernel<M, LPB, LPC> (iamf_render_nolim_packets*.hip): the limiter-less renderer over one
                // element's packets, kCallPacketsNolim, which only iamf_hip_batch_render_packets_nolim sets; variant 0.  Set 11,
                // listed by family only
  NolimPacketsMix,  // render_nolim_kernel<M, LPB, LPC, LP2> (iamf_render_nolim_packets*_mix.hip): the limiter-less renderer over both
                // elements' packets, kCallPacketsMixNolim, which only iamf_hip_batch_render_packets_mix_nolim sets; variant = LP2.
                // Set 12, listed by family only
};
struct Route {
  Family family;
  int variant;
  int err;   // IAMF_HIP_OK unless family == Refused
};

// Which prefetch variant a launch of n_launch workgroups of the 24-bit LPCM form takes: the faster one per size as measured
// (tools/lpcm24_rate.py, MI355X, 3rd-order element into stereo s16, 64 frames x 1024, profiles/r09_lpcm24_rate.json): the
// early per-channel prefetch at every size — 512 / 2048 / 4096 streams: 0.370 / 1.346 / 2.688 ms against 0.417 / 1.400 /
// 2.753 ms for the late one.  (Unlike the 16-bit form, whose late variant wins beyond 1024 workgroups: here <16, 2> with the
// late prefetch is built for three workgroups per CU, render_fast.hpp.)  No cut, so the rule is the constant; the late
// instances stay reachable by IAMF_HIP_LP_LATE=1.
inline bool lpcm24_early(int n_launch) {
  (void)n_launch;
  return true;
}
// Whether a range of n_launch streams takes the 24-bit form at all: a size at which it does not beat the unfused pair
// (unpack, then the f32 kernel) by more than that pair's own run-to-run spread is not fused (render_prepare asks).  Same
// run, same file: the unfused pair takes 4.26 / 4.66 / 4.61 times the fused call's time at 512 / 2048 / 4096 streams, its
// spread against itself at most 0.0006 — every measured size wins, so every size is fused; this is where a size that stops
// winning would be cut.
inline bool lpcm24_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Which prefetch variant a launch of n_launch workgroups of the coupled 16-bit form (RenderParams::lpcm_coupled) takes: the
// faster one per size as measured (tools/lpcm_coupled_rate.py, MI355X, stereo / 5.1 / 7.1.4 element into stereo s16, 64
// frames x 1024, profiles/r10_lpcm_coupled_rate.json): the early per-pair prefetch at every size and for every element —
// 7.1.4, 512 / 2048 / 4096 streams: 0.694 / 1.477 / 2.838 ms against 0.750 / 1.573 / 3.066 ms for the late one; stereo:
// 0.296 / 0.632 / 1.225 against 0.322 / 0.674 / 1.311 — by 5 to 9 %, the baseline's run-to-run spread being at most 0.3 %.
// (Unlike the mono-coded 16-bit form, whose late variant wins beyond 1024 workgroups: a pair is ONE request for two
// channels, so the early form issues half as many per chunk.)  No cut, so the rule is the constant; the late instances stay
// reachable by IAMF_HIP_LP_LATE=1, and IAMF_HIP_LP_EARLY=1 forces the early one (pick_route).
inline bool lpcm_coupled_early(int n_launch) {
  (void)n_launch;
  return true;
}
// Whether a range of n_launch streams takes the coupled form at all (render_prepare asks): a size at which it does not
// beat what the call ran before — unpack, then the f32 kernel, timed from a build of the parent commit in the same process —
// by more than that pair's own run-to-run spread is not fused.  Same run, same file: the pair takes 1.45 / 1.89 / 1.93
// (stereo), 1.78 / 2.57 / 2.63 (5.1) and 2.18 / 3.34 / 3.46 (7.1.4) times the fused call's time at 512 / 2048 / 4096 streams,
// its spread against itself at most 0.0027 — every measured size wins, so every size is fused; this is where a size that
// stops winning would be cut.
inline bool lpcm_coupled_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Which prefetch variant a launch of n_launch workgroups of the coupled 24-bit form (RenderParams::lpcm_coupled == 2) takes,
// under the rule of lpcm_coupled_early(): the faster one per size as measured by tools/lpcm24_coupled_rate.py (stereo / 5.1 /
// 7.1.4 element into stereo s16, 64 frames x 1024, profiles/r15_lpcm24_coupled_rate.json).
// Measured on an MI355X: the early per-pair prefetch at every size and for every element — 7.1.4, 512 / 2048 / 4096 streams:
// 0.711 / 1.620 / 3.086 ms against 0.790 / 1.756 / 3.378 ms for the late one; 5.1: 0.516 / 1.124 / 2.159 against 0.567 / 1.195 /
// 2.316; stereo: 0.303 / 0.664 / 1.285 against 0.336 / 0.714 / 1.393 — by 6 to 11 %, the baseline's run-to-run spread being at
// most 0.6 %.  (All twenty instances are built for four workgroups per CU: DESIGN.md 4.1h.)  No cut, so the rule is the constant.
// The late instances stay reachable by IAMF_HIP_LP_LATE=1, and IAMF_HIP_LP_EARLY=1 forces the early one (pick_route).
inline bool lpcm24_coupled_early(int n_launch) {
  (void)n_launch;
  return true;
}
// Whether a range of n_launch streams takes the coupled 24-bit form at all (render_prepare asks), under the rule of
// lpcm_coupled_fused(): a size at which it does not beat what the call ran before — unpack, then the f32 kernel, timed from a
// build of the parent commit in the same process — by more than that pair's own run-to-run spread is not fused.
// Same run, same file: the pair takes 1.47 / 1.93 / 1.96 (stereo), 1.84 / 2.59 / 2.62 (5.1) and 2.31 / 3.23 / 3.38 (7.1.4) times
// the fused call's time at 512 / 2048 / 4096 streams, its spread against itself at most 0.0055 — every measured (shape, size)
// wins, so every size is fused; this is where a size that stops winning would be cut.
inline bool lpcm24_coupled_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams takes the two-element packet form at all (render_prepare asks), under the rule of
// lpcm_coupled_fused(): a (shape, size) at which it does not beat what a caller ran before — iamf_hip_lpcm_unpack of the
// second element, then iamf_hip_batch_render_lpcm with d_in2, timed from a build of the parent commit in the same process —
// by more than that baseline's own run-to-run spread is not fused.  Measured (tools/lpcm_mix_rate.py, MI355X, into stereo
// s16, 64 frames x 1024, profiles/r11_lpcm_mix_rate.json): the baseline takes 3.93 / 5.19 / 5.62 (3rd-order bed + coupled
// stereo), 1.85 / 2.59 / 2.67 (5.1 + mono) and 2.36 / 3.87 / 3.96 (7.1.4 + coupled stereo) times the fused call's time at
// 512 / 2048 / 4096 streams, its spread against itself at most 0.0026 — every measured (shape, size) wins, so every size
// is fused; this is where one that stops winning would be cut.
inline bool lpcm_mix_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams takes the two-element 24-bit packet form at all (render_prepare asks), under the rule of
// lpcm_mix_fused(): a (shape, size) at which it does not beat what the call ran before — two iamf_hip_lpcm_unpack passes and the
// f32 mixing kernel, timed from a build of the parent commit in the same process through iamf_hip_batch_render_lpcm_mix — by
// more than that baseline's own run-to-run spread is not fused (tools/lpcm24_mix_rate.py, profiles/r16_lpcm24_mix_rate.json).
// Measured on an MI355X, into stereo s16, 64 frames x 1024: the baseline takes 3.92 / 4.13 / 4.51 (3rd-order bed + coupled
// stereo), 1.96 / 2.67 / 2.74 (5.1 + mono) and 2.42 / 3.70 / 3.89 (7.1.4 + coupled stereo) times the fused call's time at 512 /
// 2048 / 4096 streams, its spread against itself at most 0.0052 — every measured (shape, size) wins, so every size is fused;
// this is where one that stops winning would be cut.  (<16, 2, 2> and the others of lpcm24_mix_wgs() run at three workgroups
// per CU: the 3rd-order bed is among the measured shapes.)
inline bool lpcm24_mix_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_interleaved takes the interleaved form at all
// (render_prepare asks), under the rule of lpcm_coupled_fused(): a size at which it does not beat what the call ran before —
// iamf_hip_batch_render_range on a twin batch in the same process, the general kernel — by more than that baseline's own
// run-to-run spread is not fused.  Measured (tools/interleaved_rate.py, MI355X, mono and stereo through the identity into
// s16, 64 x 1115 or 64 x 1024 sample-frames per stream and step, profiles/r12_interleaved_rate.json): the baseline takes
// 1.88 / 1.85 / 1.54 (mono) and 1.85 / 1.69 / 1.50 (stereo) times the new entry's time in calls of 1115 sample-frames at
// 512 / 2048 / 4096 streams, 1.66 / 1.70 / 1.46 and 1.66 / 1.65 / 1.36 in calls of 1024, 3.66 / 3.88 / 3.44 and 3.59 / 3.61 /
// 3.13 in one call of 64 x 1115; its spread against itself at most 0.0078 — every measured (shape, size) wins, so every
// size is fused; this is where one that stops winning would be cut.
inline bool interleaved_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_ragged takes the planar ragged form at all
// (render_prepare asks), under the rule of lpcm_coupled_fused(): a size at which it does not beat what the call ran before —
// iamf_hip_batch_render_range on a twin batch in the same process, the general kernel — by more than that baseline's own
// run-to-run spread is not fused.  Measured (tools/ragged_rate.py, MI355X, a 3rd-order and a stereo element into stereo s16,
// 64 calls of one frame per stream and step, profiles/r13_ragged_rate.json): the baseline takes 1.88 / 1.55 / 1.49 (3rd
// order) and 1.97 / 1.87 / 1.59 (stereo) times the new entry's time in calls of 1000 samples at 512 / 2048 / 4096 streams,
// 1.60 / 1.44 / 1.28 and 1.61 / 1.56 / 1.28 in calls of 480; its spread against itself at most 0.0027 — every measured
// (shape, size) wins, so every size is fused; this is where one that stops winning would be cut.  (One call of 64 frames
// of 1000 is 1000 whole blocks: both entries run Family::Fast there, 0.99 to 1.01 of each other.)
inline bool ragged_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_packets_ragged takes the ragged packet form at
// all (render_prepare asks), under the rule of lpcm_coupled_fused(): a (shape, size) at which it does not beat what the call
// ran before — iamf_hip_batch_render_packets on a twin batch in the same process: iamf_hip_lpcm_unpack, then the general
// kernel — by more than that baseline's own run-to-run spread is not fused (tools/packets_ragged_rate.py,
// profiles/r17_packets_ragged_rate.json).
// Measured on an MI355X, into stereo s16, 64 one-frame calls per stream and step: the baseline takes 2.83 / 2.83 / 3.65 (3rd order,
// 16-bit mono-coded), 2.87 / 2.87 / 3.65 (3rd order, 24 bit), 2.30 / 2.27 / 1.89 and 2.29 / 2.24 / 1.92 (5.1 coupled, 16 / 24 bit),
// 2.18 / 2.30 / 2.44 and 2.19 / 2.21 / 2.50 (7.1.4 coupled, 16 / 24 bit) times the new entry's time in calls of 1000 samples at
// 512 / 2048 / 4096 streams, and 2.37 / 2.24 / 2.09, 2.39 / 2.30 / 2.23, 1.85 / 1.93 / 1.53, 1.86 / 1.86 / 1.54, 2.22 / 2.26 / 2.00 and
// 2.17 / 2.18 / 2.00 in calls of 480; its spread against itself at most 0.0033 — every measured (shape, size) wins, so every size
// is fused; this is where one that stops winning would be cut.  (One call of 64 frames of 1000 is 1000 whole blocks: both
// entries run the form's whole-block family there, 0.996 to 1.014 of each other.)
inline bool packets_ragged_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_packets_mix_ragged takes the ragged two-element
// packet form at all (render_prepare asks), under the rule of lpcm_mix_fused(): a (shape, size) at which it does not beat what
// the call ran before — iamf_hip_batch_render_packets_mix on a twin batch in the same process: two iamf_hip_lpcm_unpack passes,
// then the general kernel — by more than that baseline's own run-to-run spread is not fused (tools/packets_mix_ragged_rate.py,
// profiles/r18_packets_mix_ragged_rate.json).
// Measured on an MI355X, into stereo s16, 64 one-frame calls per stream and step (5 steps per region, 3 regions): the baseline takes
// 3.05 / 3.11 / 3.89 (3rd-order bed + coupled stereo, 16 bit), 2.80 / 2.64 / 3.11 (24 bit), 2.28 / 2.26 / 1.90 and 2.29 / 2.27 / 1.96 (5.1 + mono, 16 / 24 bit),
// 2.51 / 2.65 / 2.85 and 2.41 / 2.45 / 2.75 (7.1.4 + coupled stereo, 16 / 24 bit) times the new entry's time in calls of 1000 samples at
// 512 / 2048 / 4096 streams, and 2.40 / 2.34 / 2.15, 2.14 / 1.79 / 1.76, 1.93 / 1.98 / 1.63, 1.97 / 1.94 / 1.66, 2.24 / 2.29 / 1.99 and
// 2.18 / 2.17 / 1.95 in calls of 480; its spread against itself at most 0.0035 — every measured (shape, size) wins, so every size
// is fused; this is where one that stops winning would be cut.  (One call of 64 frames of 1000 is 1000 whole blocks: both
// entries run the whole-block mix family there, 0.990 to 1.010 of each other.)
inline bool packets_mix_ragged_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_packets_nolim takes the packet-fed limiter-less
// renderer at all (render_prepare asks), under the rule of lpcm_coupled_fused(): a (shape, size) at which it does not beat what the
// call ran before — iamf_hip_batch_render_packets_ragged on a twin batch in the same process: iamf_hip_lpcm_unpack, then
// render_nolim_kernel — by more than that baseline's own run-to-run spread is not fused (tools/nolim_packets_rate.py,
// profiles/r19_nolim_packets_rate.json).
// Measured on an MI355X, limiter off, 64 frames of 1024 per stream and step (5 steps per region, 5 regions after a discarded one): the
// baseline takes 2.43 / 3.47 / 6.02 (3rd order, 16-bit mono-coded, into stereo f32: a rate-converting stream's first stage) and
// 2.31 / 3.49 / 4.86 (7.1.4, 24-bit coupled, into stereo s16) times the new entry's time in one-frame calls at 512 / 2048 / 4096
// streams, and 5.22 / 5.40 / 5.83 and 5.01 / 4.56 / 5.13 in one call of 64 frames; its spread against itself at most 0.0039 — every
// measured (shape, size) wins, so every size is fused; this is where one that stops winning would be cut.
inline bool nolim_packets_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Whether a range of n_launch streams that came through iamf_hip_batch_render_packets_mix_nolim takes the two-element packet form of
// the limiter-less renderer at all (render_prepare asks), under the rule of lpcm_coupled_fused(): a (shape, size) at which it does
// not beat what the call ran before — iamf_hip_batch_render_packets_mix_ragged on a twin batch in the same process: two
// iamf_hip_lpcm_unpack passes, then the general kernel — by more than that baseline's own run-to-run spread is not fused
// (tools/nolim_packets_mix_rate.py, profiles/r20_nolim_packets_mix_rate.json).
// Measured on an MI355X, limiter off, 64 frames of 1024 per stream and step (5 steps per region, 5 regions after a discarded one): the
// baseline takes 3.98 / 4.38 / 6.04 (3rd-order bed + coupled stereo, 16 bit, into stereo f32: a rate-converting stream's first stage)
// and 3.36 / 3.65 / 5.24 (7.1.4 coupled + mono, 24 bit, into stereo s16) times the new entry's time in one-frame calls at 512 / 2048 /
// 4096 streams, and 7.25 / 5.89 / 5.78 and 6.23 / 5.23 / 5.21 in one call of 64 frames; its spread against itself at most 0.0040 — every
// measured (shape, size) wins, so every size is fused and nothing is cut; this is where one that stops winning would be.
inline bool nolim_packets_mix_fused(int n_launch) {
  (void)n_launch;
  return true;
}

// Which kernel launch() runs for p with m inputs.  The rules in priority order: the first that holds decides.  Every
// kernel is exact, so a call that misses its rule still renders right, only slower: tests/test_route_host.py pins the
// rules.  The environment switches are read at every call (the tests set and unset them within one process).
inline Route pick_route(const RenderParams &p, int m) {
  const auto take = [](Family f, int variant = 0) { return Route{f, variant, IAMF_HIP_OK}; };
  const auto refuse = [](int err) { return Route{Family::Refused, 0, err}; };
  const bool force_generic = getenv("IAMF_HIP_FORCE_GENERIC") != nullptr;
  const bool mixing = p.in2 || p.elem_ramp || p.elem2_ramp || p.out_ramp;
  const bool staged = p.demix_on || p.dmx_on || mixing;   // a stage in front of or beside the projection
  const bool fast_shape = fast_shape_ok(p, force_generic);

  // interleaved f32 of any call length (RenderParams::interleaved, zero unless iamf_hip_batch_render_interleaved set it): the
  // form's own kernel where its rules hold, else whatever the rules below give the call
  if (interleaved_shape_ok(p, m, force_generic)) return take(Family::FastInterleaved);
  // planar f32 that is no whole number of 64-sample blocks (RenderParams::ragged, zero unless iamf_hip_batch_render_ragged set
  // it): the same way
  if (ragged_shape_ok(p, m, force_generic)) return take(Family::FastRagged);

  // one element as packets, no whole number of 64-sample blocks (kCallPacketsRagged, which only
  // iamf_hip_batch_render_packets_ragged sets): the same way, in front of the packet rules, which refuse such a length
  if (packets_ragged_shape_ok(p, m, force_generic)) return take(Family::PacketsRagged);
  // both elements of a mix as packets, no whole number of 64-sample blocks (kCallPacketsMixRagged, which only
  // iamf_hip_batch_render_packets_mix_ragged sets): the same way, in front of the packet-mix rules, which refuse such a length
  if (packets_mix_ragged_shape_ok(p, m, force_generic)) return take(Family::PacketsMixRagged, p.lpcm_mix & 3);
  // one element as packets on a limiter-less batch (kCallPacketsNolim, which only iamf_hip_batch_render_packets_nolim sets):
  // the same way, in front of the packet rules, which refuse a batch without the limiter
  if (nolim_packets_shape_ok(p, m, force_generic)) return take(Family::NolimPackets);
  // (both elements as packets on such a batch, kCallPacketsMixNolim: the rule reads the second element's run starts, which
  //  travel behind this block — pick_route(const RenderMixParams &) below asks it, here, in front of the packet rules)

  // element 0 as LPCM packets: only the fused kernel reads them (render_prepare asks here and unpacks to f32 otherwise)
  if (p.lpcm) {
    const bool elem0_listed = p.lpcm_coupled ? LpcmCoupledM::has(m) : LpcmM::has(m);
    const bool fast_call = LpcmOC::has(p.out_ch) && fast_shape && !p.dmx_on;   // what every whole-block packet form refuses otherwise
    // both elements as packets (RenderParams::lpcm_mix, zero unless an entry of the two-element forms set it): LP2 with 16-bit
    // samples (iamf_hip_batch_render_lpcm_mix), 4 | LP2 with 24-bit samples on both elements and lpcm_coupled == 2 for a coupled bed
    // (values of the form's own, set by iamf_hip_batch_render_packets_mix alone — 4 | LP2 with any other sample size or coupling
    // names no form).  The refusals of the single-element forms; element 1's packets on the sample size's grid (8 bytes / 4 bytes) and
    // inside the same 32-bit offset bound as element 0's (fast_shape_ok); ramps under fast_shape_ok's rules
    if (p.lpcm_mix) {
      const bool s24 = p.lpcm_mix >= 4;
      const int lp2 = s24 ? p.lpcm_mix - 4 : p.lpcm_mix;
      const bool sizes = s24 ? p.lpcm_bytes == 3 && (p.lpcm_coupled == 0 || p.lpcm_coupled == 2) : p.lpcm_bytes != 3;
      if (!sizes || !elem0_listed || !fast_call) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      if (!p.in2 || !LpcmMixK::has(lp2) || !lpcm_mix_m2_ok(lp2, p.m2)) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      if (!on_grid16(p.in2) || (p.in2_stream_stride & (s24 ? 3 : 7)) || (p.in2_frame_stride & (s24 ? 3 : 7))) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      if (!packet_offsets32_ok(p, p.in2_frame_stride)) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      return take(s24 ? Family::Lpcm24Mix : Family::LpcmMix, lp2);
    }
    // the coupled 24-bit form (lpcm_coupled == 2, set by iamf_hip_batch_render_packets alone, and 24-bit samples — 2 with any
    // other sample size names no form): the coupled instances' lists under exactly the refusals of Family::Lpcm24
    if (p.lpcm_coupled == 2) {
      if (p.lpcm_bytes != 3 || !elem0_listed || !fast_call) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      return take(Family::Lpcm24Coupled, lp_early_variant(lpcm24_coupled_early(p.n_launch)));
    }
    // the coupled 16-bit form: its own instances (the pairing is a function of m: lpcm_form.hpp), the same refusals
    if (p.lpcm_coupled) {
      if (!elem0_listed || !fast_call || p.lpcm_bytes == 3) return refuse(IAMF_HIP_ERR_INVALID_STATE);
      return take(Family::LpcmCoupled, lp_early_variant(lpcm_coupled_early(p.n_launch)));
    }
    if (!elem0_listed || !fast_call) return refuse(IAMF_HIP_ERR_INVALID_STATE);
    // 24-bit samples (lpcm_bytes: 0 or 2 = 16 bit): the same instances and refusals, the kernel's LPB = 3 form
    // (IAMF_HIP_LP_EARLY=1 forces the early variant as IAMF_HIP_LP_LATE=1 forces the late one: tools/lpcm24_rate.py times both
    //  at every size, and the tests run both whatever the cut)
    if (p.lpcm_bytes == 3) return take(Family::Lpcm24, lp_early_variant(lpcm24_early(p.n_launch)));
    // up to four workgroups a CU: the early per-channel prefetch (latency bound); beyond: the plain one (issue bound).
    // Measured on MI355X, 512 / 4096 streams: 117 against 109 / 136 against 145 Gsamples/s (profiles/r04_ab_fast.txt)
    return take(Family::Lpcm, p.n_launch <= 1024 && !getenv("IAMF_HIP_LP_LATE"));
  }
  // HRTF renderer: aligned calls only (the flush goes to the generic kernel)
  if (p.fir_taps > 0 && p.in) {
    // the FIR stage keeps input offsets of one stream as 32-bit integers.  (In front of the fast kernel's own, tighter
    // bound on byte offsets, which would shadow it: a frame stride no stage can address is a bad argument.)
    if (((int64_t)(p.total / p.frame_size) + 1) * p.in_frame_stride >= (int64_t)1 << 31) return refuse(IAMF_HIP_ERR_BAD_ARG);
    if (!fast_shape || p.dmx_on) return refuse(IAMF_HIP_ERR_UNIMPLEMENTED);
    if (!FirHomeM::has(m) && !FirM2bM::has(m)) return refuse(IAMF_HIP_ERR_UNIMPLEMENTED);
    // Three stages with one specification (render_fir.hpp): overlap-save FFT on the VALU (default, render_fir_fft.hpp),
    // split-f16 MFMA (IAMF_HIP_FIR_F16=1, render_fir16.hpp), f32 MFMA (IAMF_HIP_FIR_F32=1); they differ in the last bits
    const int stage = fir_stage_choice(p);
    return stage == 4 ? take(Family::FirSplit) : take(Family::FirFused, stage);
  }
  // the parametric down-mixer to mono / stereo, with the frames' parameters at hand
  if (p.dmx_on && p.dmx_frames && fast_shape && FastDownMC::has(mc(m, p.out_ch))) return take(Family::FastDown);

  const bool fast = !p.lfe && fast_shape && !p.dmx_on;
  const bool wide_shape = wide_shape_ok(p, m, force_generic);
  const bool wide4_shape = wide_shape && wide4_shape_ok(p, mixing);
  // render_wide4_kernel (like render_fast_kernel) places its ring per call and takes a position that is not a multiple
  // of 16 from 240 samples on; the 256-sample kernel of render_wide.hpp keeps absolute ring positions and needs the
  // stream at a multiple of 16
  const bool pos16 = !(p.pos0 & 15);
  const bool pos_any = pos_ok(p);

  // an LFE slot is filled by render_wide4_kernel<.., LFE> where that exists, else by the generic kernel
  if (p.lfe) {
    if (!p.lfe_k0 && !staged && wide4_shape && pos16 && Wide4LfeM::has(m) && Wide4C::has(p.out_ch))
      return take(Family::Wide4Lfe, p.use_mfma != 0);
  } else if (wide4_shape && pos_any) {
    // demixer / down-mixer / mixer: wide4 variants only, and one of them at a time
    if (mixing) {
      if (!p.demix_on && !p.dmx_on && Wide4M::has(m) && Wide4MixC::has(p.out_ch)) return take(Family::Wide4Mix, p.use_mfma != 0);
    } else if (p.dmx_on) {  // (demixer AND down-mixer: generic kernel)
      if (p.dmx_frames && !p.demix_on && Wide4DownMC::has(mc(m, p.out_ch))) return take(Family::Wide4Down);
    } else if (p.demix_on) {  // scalable channel audio: the variant with the demixer in front of the projection
      if (p.demix_w4 && !p.use_mfma && (p.demix_i0 & 3) == 0 && Wide4DemixM::has(m) && Wide4DemixC::has(p.out_ch))
        return take(Family::Wide4Demix);
    } else if (Wide4M::has(m) && Wide4C::has(p.out_ch)) {
      return take(Family::Wide4, p.use_mfma != 0);
    }
  }
  // limiter off, one matrix-rendered element, constant gains (render_nolim.hpp)
  if (!p.limiter_on && p.in && !p.lfe && !p.pre_matrix && !staged && p.fir_taps == 0 && p.og_ch >= p.out_ch && !force_generic &&
      nolim_shape_ok(p))
    return NolimM::has(m) ? take(Family::Nolim) : refuse(IAMF_HIP_ERR_UNIMPLEMENTED);
  // aligned calls of one matrix-rendered element (the fast kernel: with a small second element or ramps, too)
  if (fast && FastM::has(m)) return take(Family::Fast, mixing);
  if (!p.lfe && wide_shape && !staged && pos16 && WideM::has(m)) return take(Family::Wide, p.use_mfma != 0);
  // everything else: ragged calls, flush, wide second elements, exact two-stage projection, demixer + down-mixer
  // together, other PCM formats of the stages above
  return GenericM::has(m) ? take(Family::Generic) : refuse(IAMF_HIP_ERR_UNIMPLEMENTED);
}

// The same for the block launch() holds: both elements as packets on a limiter-less batch (kCallPacketsMixNolim, which only
// iamf_hip_batch_render_packets_mix_nolim sets) take the two-element form of the limiter-less renderer where
// nolim_packets_mix_shape_ok holds — the marks exclude one another, so its place among the marked rules above does not matter —
// and every other block is routed by the rules above, the mark meaning nothing to them.
inline Route pick_route(const RenderMixParams &p, int m) {
  if (nolim_packets_mix_shape_ok(p, m, getenv("IAMF_HIP_FORCE_GENERIC") != nullptr)) return Route{Family::NolimPacketsMix, p.lpcm_mix & 3, IAMF_HIP_OK};
  return pick_route(static_cast<const RenderParams &>(p), m);
}

// ------------------------------------------------------------------------------------------
// the instance table: every render kernel instance of the build, as rows of include/iamf_hip.h
// ------------------------------------------------------------------------------------------

// f(family, variant, m, c, k) — family: IAMF_HIP_ROUTE_*, the other fields as iamf_hip.h says per family — for every
// instance the launchers can name, walking the lists they dispatch over.  iamf_route.hip numbers the rows in this order.
template <class F>
void for_each_render_instance(F &&f) {
  for_each_int(GenericM{}, [&](int m) { f(IAMF_HIP_ROUTE_GENERIC, 0, m, 0, 0); });
  for_each_int(NolimM{}, [&](int m) { f(IAMF_HIP_ROUTE_NOLIM, 0, m, 0, 0); });
  for (int mixing = 0; mixing < 2; ++mixing)
    for_each_int(FastM{}, [&](int m) { for_each_int(FastOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_FAST, mixing, m, oc, 0); }); });
  for_each_int(FastDownMC{}, [&](int v) { f(IAMF_HIP_ROUTE_FAST_DOWN, 0, mc_m(v), mc_c(v), 0); });
  for (int mfma = 0; mfma < 2; ++mfma) for_each_int(WideM{}, [&](int m) { f(IAMF_HIP_ROUTE_WIDE, mfma, m, 0, 0); });
  for (int mfma = 0; mfma < 2; ++mfma)
    for_each_int(Wide4M{}, [&](int m) { for_each_int(Wide4C{}, [&](int c) { f(IAMF_HIP_ROUTE_WIDE4, mfma, m, c, 0); }); });
  for_each_int(Wide4DemixM{}, [&](int m) { for_each_int(Wide4DemixC{}, [&](int c) { f(IAMF_HIP_ROUTE_WIDE4_DEMIX, 0, m, c, 0); }); });
  for_each_int(Wide4DownMC{}, [&](int v) { f(IAMF_HIP_ROUTE_WIDE4_DOWN, 0, mc_m(v), mc_c(v), 0); });
  for (int mfma = 0; mfma < 2; ++mfma)
    for_each_int(Wide4M{}, [&](int m) { for_each_int(Wide4MixC{}, [&](int c) { f(IAMF_HIP_ROUTE_WIDE4_MIX, mfma, m, c, 0); }); });
  for (int mfma = 0; mfma < 2; ++mfma)
    for_each_int(Wide4LfeM{}, [&](int m) { for_each_int(Wide4C{}, [&](int c) { f(IAMF_HIP_ROUTE_WIDE4_LFE, mfma, m, c, 0); }); });
  for (int early = 0; early < 2; ++early)
    for_each_int(LpcmM{}, [&](int m) { for_each_int(LpcmOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_LPCM, early, m, oc, 0); }); });
  for_each_int(FanM{}, [&](int m) { for_each_int(FanK{}, [&](int k) { f(IAMF_HIP_ROUTE_FANOUT, 0, m, 0, k); }); });
  for (int home = 1; home >= 0; --home) {
    const auto firs = [&](int m) {
      f(IAMF_HIP_ROUTE_FIR_SPLIT, 0, m, 0, 0);
      for (int stage = 1; stage <= 3; ++stage) f(IAMF_HIP_ROUTE_FIR_FUSED, stage, m, 0, 0);
    };
    if (home) for_each_int(FirHomeM{}, firs);
    else for_each_int(FirM2bM{}, firs);
  }
}

// The extension table (iamf_hip_route_instances_ext): instances added behind the table above, whose row set is pinned.
template <class F>
void for_each_render_instance_ext(F &&f) {
  for_each_int(FanLpM{}, [&](int m) { for_each_int(FanLpK{}, [&](int k) { f(IAMF_HIP_ROUTE_FANOUT_LPCM, 0, m, 0, k); }); });
}

// The rows of a packet form over element 0's shapes: f(m) for LpcmM (mono-coded), then LpcmCoupledM (coupled) — the two lists
// share no number, so m tells the one from the other — as the form's launchers walk them.
template <class F>
void for_each_packet_m(F &&rows) {
  for_each_int(LpcmM{}, rows);
  for_each_int(LpcmCoupledM{}, rows);
}

// Table 2 (iamf_hip_route_table_instances): the 24-bit LPCM form, walking LpcmM x LpcmOC as its launcher does.
template <class F>
void for_each_render_instance_lpcm24(F &&f) {
  for (int early = 0; early < 2; ++early)
    for_each_int(LpcmM{}, [&](int m) { for_each_int(LpcmOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_LPCM24, early, m, oc, 0); }); });
}

// The forms below are listed by family only (iamf_hip_route_family_instances), each walking its lists as its launchers do.
// The coupled 16-bit LPCM form: LpcmCoupledM x LpcmOC.
template <class F>
void for_each_render_instance_lpcm_coupled(F &&f) {
  for (int early = 0; early < 2; ++early)
    for_each_int(LpcmCoupledM{}, [&](int m) { for_each_int(LpcmOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_LPCM_COUPLED, early, m, oc, 0); }); });
}

// The two-element packet form: element 0's shapes x LpcmOC x LpcmMixK; k = LP2.
template <class F>
void for_each_render_instance_lpcm_mix(F &&f) {
  for_each_packet_m([&](int m) {
    for_each_int(LpcmOC{}, [&](int oc) { for_each_int(LpcmMixK{}, [&](int k) { f(IAMF_HIP_ROUTE_LPCM_MIX, 0, m, oc, k); }); });
  });
}

// The interleaved form: InterleavedM x InterleavedOC.
template <class F>
void for_each_render_instance_interleaved(F &&f) {
  for_each_int(InterleavedM{}, [&](int m) { for_each_int(InterleavedOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_FAST_INTERLEAVED, 0, m, oc, 0); }); });
}

// The planar ragged form: RaggedM x RaggedOC.
template <class F>
void for_each_render_instance_ragged(F &&f) {
  for_each_int(RaggedM{}, [&](int m) { for_each_int(RaggedOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_FAST_RAGGED, 0, m, oc, 0); }); });
}

// The coupled 24-bit LPCM form: LpcmCoupledM x LpcmOC.
template <class F>
void for_each_render_instance_lpcm24_coupled(F &&f) {
  for (int early = 0; early < 2; ++early)
    for_each_int(LpcmCoupledM{}, [&](int m) { for_each_int(LpcmOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_LPCM24_COUPLED, early, m, oc, 0); }); });
}

// The two-element 24-bit packet form: element 0's shapes x LpcmOC x LpcmMixK; k = LP2.
template <class F>
void for_each_render_instance_lpcm24_mix(F &&f) {
  for_each_packet_m([&](int m) {
    for_each_int(LpcmOC{}, [&](int oc) { for_each_int(LpcmMixK{}, [&](int k) { f(IAMF_HIP_ROUTE_LPCM24_MIX, 0, m, oc, k); }); });
  });
}

// The ragged packet form: element 0's shapes x LpcmOC, the 16-bit units first; k = bytes per packet sample.
template <class F>
void for_each_render_instance_packets_ragged(F &&f) {
  for (int k = 2; k <= 3; ++k)
    for_each_packet_m([&](int m) { for_each_int(LpcmOC{}, [&](int oc) { f(IAMF_HIP_ROUTE_PACKETS_RAGGED, 0, m, oc, k); }); });
}

// The ragged two-element packet form: element 0's shapes x LpcmOC x LpcmMixK, the 16-bit units first; variant = bytes per packet
// sample, k = LP2.
template <class F>
void for_each_render_instance_packets_mix_ragged(F &&f) {
  for (int v = 2; v <= 3; ++v)
    for_each_packet_m([&](int m) {
      for_each_int(LpcmOC{}, [&](int oc) { for_each_int(LpcmMixK{}, [&](int k) { f(IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED, v, m, oc, k); }); });
    });
}

// The packet-fed limiter-less renderer: element 0's shapes, the 16-bit unit first; k = bytes per packet sample.  The output
// channel count and format are run-time values of the kernel: c = 0, as for the f32 form's rows.
template <class F>
void for_each_render_instance_nolim_packets(F &&f) {
  for (int k = 2; k <= 3; ++k) for_each_packet_m([&](int m) { f(IAMF_HIP_ROUTE_NOLIM_PACKETS, 0, m, 0, k); });
}

// The two-element packet form of the limiter-less renderer: element 0's shapes x LpcmMixK, the 16-bit unit first; variant = bytes
// per packet sample, k = LP2, c = 0 (the output channel count and format are run-time values of the kernel).
template <class F>
void for_each_render_instance_nolim_packets_mix(F &&f) {
  for (int v = 2; v <= 3; ++v)
    for_each_packet_m([&](int m) { for_each_int(LpcmMixK{}, [&](int k) { f(IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX, v, m, 0, k); }); });
}

// The fan-out fed with 24-bit and coupled packets: the three forms' (M, K) lists, variant = fan_pk_variant, k = members.
template <class F>
void for_each_render_instance_fanout_packets(F &&f) {
  for_each_int(FanPk24MK{}, [&](int v) { f(IAMF_HIP_ROUTE_FANOUT_PACKETS, fan_pk_variant(3, false), mc_m(v), 0, mc_c(v)); });
  for_each_int(FanPk16cMK{}, [&](int v) { f(IAMF_HIP_ROUTE_FANOUT_PACKETS, fan_pk_variant(2, true), mc_m(v), 0, mc_c(v)); });
  for_each_int(FanPk24cMK{}, [&](int v) { f(IAMF_HIP_ROUTE_FANOUT_PACKETS, fan_pk_variant(3, true), mc_m(v), 0, mc_c(v)); });
}

// The row sets behind the listing, by number: f as above for every instance of set `set`, no row for any other number.  Sets
// 0 .. kRouteTables - 1 are the numbered tables of iamf_hip_route_table_instances — their count and the rows of each are pinned —
// and the sets behind them are listed by family only (iamf_hip_route_family_instances), in this order.  The only place that maps
// a set number to a walker: iamf_route.hip builds and counts by it, and every key is in exactly one set (tests/route_host).  A
// form added later is one more case and one more set; the numbers in front of it stay.
constexpr int kRouteTables = 3;
constexpr int kRouteSets = 13;
template <class F>
void for_each_instance_of_set(int set, F &&f) {
  switch (set) {
    case 0: for_each_render_instance(f); for_each_resample_instance(f); break;   // the base table: the resampler's kernels too
    case 1: for_each_render_instance_ext(f); break;
    case 2: for_each_render_instance_lpcm24(f); break;
    case 3: for_each_render_instance_lpcm_coupled(f); break;
    case 4: for_each_render_instance_lpcm_mix(f); break;
    case 5: for_each_render_instance_interleaved(f); break;
    case 6: for_each_render_instance_ragged(f); break;
    case 7: for_each_render_instance_lpcm24_coupled(f); break;
    case 8: for_each_render_instance_lpcm24_mix(f); break;
    case 9: for_each_render_instance_packets_ragged(f); break;
    case 10: for_each_render_instance_packets_mix_ragged(f); break;
    case 11: for_each_render_instance_nolim_packets(f); break;
    case 12: for_each_render_instance_nolim_packets_mix(f); break;
  }
}
// Row sets behind those: kernels that no call of pick_route names (the fan-out entry decides for itself) and that were added
// after the rows of the sets above had been counted by their callers (tests/golden/route_sweep.txt counts the rows of sets
// 0 .. kRouteSets - 1 that pick_route does not name).  Set kRouteSets + i is walked by for_each_instance_of_later_set(i, f);
// iamf_route.hip builds, lists (by family only) and counts these exactly as the sets above.
constexpr int kRouteLaterSets = 1;
constexpr int kRouteSetFanoutPackets = kRouteSets + 0;   // what the fan-out entry counts its packet launch in (it has no Route to ask)
template <class F>
void for_each_instance_of_later_set(int i, F &&f) {
  switch (i) {
    case 0: for_each_render_instance_fanout_packets(f); break;
  }
}

// the row of the kernel launch() runs for a route, and the set that lists it: what iamf_hip_route_count takes (a FirSplit
// call launches render_fast_kernel<2, 2> behind it as well: launch() counts that row too)
struct RouteKey {
  int family, variant, m, c, k;
  int set = 0;   // the base table, unless route_key says otherwise
};
inline RouteKey route_key(const Route &r, const RenderParams &p, int m) {
  switch (r.family) {
    case Family::Refused: break;
    case Family::Lpcm: return {IAMF_HIP_ROUTE_LPCM, r.variant, m, p.out_ch, 0};
    case Family::FirSplit: return {IAMF_HIP_ROUTE_FIR_SPLIT, 0, m, 0, 0};
    case Family::FirFused: return {IAMF_HIP_ROUTE_FIR_FUSED, r.variant, m, 0, 0};
    case Family::FastDown: return {IAMF_HIP_ROUTE_FAST_DOWN, 0, m, p.out_ch, 0};
    case Family::Wide4Lfe: return {IAMF_HIP_ROUTE_WIDE4_LFE, r.variant, m, p.out_ch, 0};
    case Family::Wide4: return {IAMF_HIP_ROUTE_WIDE4, r.variant, m, p.out_ch, 0};
    case Family::Wide4Demix: return {IAMF_HIP_ROUTE_WIDE4_DEMIX, 0, m, p.out_ch, 0};
    case Family::Wide4Down: return {IAMF_HIP_ROUTE_WIDE4_DOWN, 0, m, p.out_ch, 0};
    case Family::Wide4Mix: return {IAMF_HIP_ROUTE_WIDE4_MIX, r.variant, m, p.out_ch, 0};
    case Family::Nolim: return {IAMF_HIP_ROUTE_NOLIM, 0, m, 0, 0};
    case Family::Fast: return {IAMF_HIP_ROUTE_FAST, r.variant, m, p.out_ch, 0};
    case Family::Wide: return {IAMF_HIP_ROUTE_WIDE, r.variant, m, 0, 0};
    case Family::Generic: return {IAMF_HIP_ROUTE_GENERIC, 0, m, 0, 0};
    case Family::Lpcm24: return {IAMF_HIP_ROUTE_LPCM24, r.variant, m, p.out_ch, 0, 2};   // a row of table 2
    case Family::LpcmCoupled: return {IAMF_HIP_ROUTE_LPCM_COUPLED, r.variant, m, p.out_ch, 0, 3};   // a family listing's row
    case Family::LpcmMix: return {IAMF_HIP_ROUTE_LPCM_MIX, 0, m, p.out_ch, r.variant, 4};   // a family listing's row, k = LP2
    case Family::FastInterleaved: return {IAMF_HIP_ROUTE_FAST_INTERLEAVED, 0, m, p.out_ch, 0, 5};   // a family listing's row
    case Family::FastRagged: return {IAMF_HIP_ROUTE_FAST_RAGGED, 0, m, p.out_ch, 0, 6};   // a family listing's row
    case Family::Lpcm24Coupled: return {IAMF_HIP_ROUTE_LPCM24_COUPLED, r.variant, m, p.out_ch, 0, 7};   // a family listing's row
    case Family::Lpcm24Mix: return {IAMF_HIP_ROUTE_LPCM24_MIX, 0, m, p.out_ch, r.variant, 8};   // a family listing's row, k = LP2
    case Family::PacketsRagged: return {IAMF_HIP_ROUTE_PACKETS_RAGGED, 0, m, p.out_ch, p.lpcm_bytes == 3 ? 3 : 2, 9};   // a family listing's row, k = sample bytes
    case Family::PacketsMixRagged:   // a family listing's row, variant = sample bytes, k = LP2
      return {IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED, p.lpcm_bytes == 3 ? 3 : 2, m, p.out_ch, r.variant, 10};
    case Family::NolimPackets: return {IAMF_HIP_ROUTE_NOLIM_PACKETS, 0, m, 0, p.lpcm_bytes == 3 ? 3 : 2, 11};   // a family listing's row, k = sample bytes
    case Family::NolimPacketsMix:   // a family listing's row, variant = sample bytes, k = LP2
      return {IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX, p.lpcm_bytes == 3 ? 3 : 2, m, 0, r.variant, 12};
  }
  return {IAMF_HIP_ROUTE_NONE, 0, 0, 0, 0};
}
