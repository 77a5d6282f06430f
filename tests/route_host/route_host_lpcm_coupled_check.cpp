// Host-only check of the coupled 16-bit LPCM form: the packet-form rule (iac_amd/csrc/lpcm_form.hpp, LpcmForm::S16C) and its
// routing (pick_route() in iac_amd/csrc/render_route.hpp, Family::LpcmCoupled).  One row per rule, each a well-formed call
// with exactly one thing changed.  The 16-byte loads of render_fast_kernel<.., LPC> read a PAIR of channels from one run,
// and the form rule is all that stands between a legal call and a kernel that reads the wrong bytes as the partner: a
// wrong row here is wrong PCM (or a misaligned load) on the GPU, not a slower rate.
// Driven by tests/test_route_host_coupled.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/iamf_hip.h"

namespace {
#include "../../iac_amd/csrc/render_params.hpp"
#include "../../iac_amd/csrc/render_route.hpp"
#include "../../iac_amd/csrc/lpcm_form.hpp"

int g_failed = 0, g_cases = 0;

void row(const char *what, bool ok) {
  printf("%-92s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
constexpr uintptr_t kRaw = 0x50000;
constexpr int kFs = 1024;

// the aligned call of route_host_lpcm24_check.cpp with element 0 as 16-bit packets, coupled or not
RenderParams call(int m, int out_ch, int coupled) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = kFs;
  p.total = 4096;
  p.in = kIn;
  p.pcm = kPcm;
  p.out_ch = p.og_ch = out_ch;
  p.out_format = IAMF_HIP_FMT_S16;
  p.pcm_stream_stride = (int64_t)(p.total + 1024) * out_ch * 4;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 241;
  p.n_end = 9651;
  p.lpcm = reinterpret_cast<const uint8_t *>(kRaw);
  p.lpcm_frame_stride = 16 * kFs * 2;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
  p.lpcm_bytes = 2;
  p.lpcm_coupled = coupled;
  return p;
}
template <class F>
RenderParams with(RenderParams p, F f) {
  f(p);
  return p;
}
bool same_key(const RouteKey &k, int f, int v, int m, int c, int kk) {
  return f == k.family && v == k.variant && m == k.m && c == k.c && kk == k.k;
}
void expect(const char *what, const RenderParams &p, int m, const char *env, Family family, int variant, int err = IAMF_HIP_OK) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  if (env) unsetenv(env);
  bool listed = true;   // a coupled route names a row of the family's listing and no row of the three tables
  if (r.family == Family::LpcmCoupled) {
    const RouteKey k = route_key(r, p, m);
    listed = false;
    for_each_render_instance_lpcm_coupled([&](int f, int v, int km, int kc, int kk) { listed = listed || same_key(k, f, v, km, kc, kk); });
    for_each_render_instance([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_ext([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm24([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
  }
  row(what, r.family == family && r.variant == variant && r.err == err && listed);
}

// The packets of a loudspeaker layout of ch channels in playback order, `bytes`-byte samples: pair (0,1) first, then (from
// six channels on) C and LFE as mono runs, then the pairs (4,5) ..; run after run from `head`.  coupled = false: every
// channel a mono run of its own (the mono-coded element).
iamf_hip_lpcm_layout layout(int ch, bool coupled = true, int bytes = 2, int head = 0) {
  iamf_hip_lpcm_layout L;
  memset(&L, 0, sizeof(L));
  L.sample_bytes = bytes;
  L.little_endian = 1;
  L.channels = ch;
  L.frame_size = kFs;
  int off = head;
  for (int c = 0; c < ch; ++c) {
    const bool pair = coupled && (ch == 2 || c < 2 || c >= 4);
    if (pair && (c & 1)) {
      L.src_offset[c] = L.src_offset[c - 1] + bytes;
      L.src_step[c] = 2 * bytes;
      continue;
    }
    L.src_offset[c] = off;
    L.src_step[c] = pair ? 2 * bytes : bytes;
    off += kFs * L.src_step[c];
  }
  return L;
}
constexpr int64_t kRow = 17 * kFs * 4;   // a packet row that holds every layout below; a multiple of 8
LpcmForm form(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw) {
  return lpcm_form(L, ch, ss, fst, raw, first);
}
template <class F>
iamf_hip_lpcm_layout with_l(iamf_hip_lpcm_layout L, F f) {
  f(L);
  return L;
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  const int STATE = IAMF_HIP_ERR_INVALID_STATE;
  char what[160];

  // ---- the pairing the kernel is built on ----
  static_assert(IAMF_HIP_ROUTE_LPCM_COUPLED == 17, "stable number");
  static_assert(lpcm_coupled_paired(2, 0) && lpcm_coupled_paired(2, 1), "stereo: one pair");
  static_assert(lpcm_coupled_paired(6, 0) && lpcm_coupled_paired(6, 1) && !lpcm_coupled_paired(6, 2) && !lpcm_coupled_paired(6, 3) &&
                    lpcm_coupled_paired(6, 4) && lpcm_coupled_paired(12, 11),
                "L R, C and LFE mono, pairs behind");
  static_assert(lpcm_coupled_m(2) && lpcm_coupled_m(6) && lpcm_coupled_m(12) && !lpcm_coupled_m(4) && !lpcm_coupled_m(16) && !lpcm_coupled_m(1),
                "LpcmCoupledM");

  // ---- the form rule: each M ----
  for_each_int(LpcmCoupledM{}, [&](int m) {
    snprintf(what, sizeof(what), "16-bit LE, %d channels, every pair coupled: the coupled form", m);
    row(what, form(layout(m), m) == LpcmForm::S16C);
    snprintf(what, sizeof(what), "  %d channels, head 8: pair runs only 8-byte aligned", m);
    row(what, form(layout(m, true, 2, 8), m) == LpcmForm::S16C);
  });
  row("  bytes of the forms: 0 / 2 / 3 / 2", lpcm_form_bytes(LpcmForm::None) == 0 && lpcm_form_bytes(LpcmForm::S16) == 2 &&
                                                 lpcm_form_bytes(LpcmForm::S24) == 3 && lpcm_form_bytes(LpcmForm::S16C) == 2);
  const int not_coupled[] = {4, 14, 16};
  for (int m : not_coupled) {
    snprintf(what, sizeof(what), "  %d channels with (0,1) coupled: no layout of the form", m);
    row(what, form(with_l(layout(m, false), [](iamf_hip_lpcm_layout &L) { L.src_step[0] = L.src_step[1] = 4; L.src_offset[1] = L.src_offset[0] + 2; }), m) ==
                  LpcmForm::None);
  }

  // ---- one thing changed at a time, on 5.1 and on stereo ----
  const iamf_hip_lpcm_layout L6 = layout(6), L2 = layout(2), L12 = layout(12);
  row("5.1: pair (0,1) at offset 4 mod 8", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[0] += 4; L.src_offset[1] += 4; }), 6) == LpcmForm::None);
  row("5.1: pair (4,5) at offset 4 mod 8", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[4] += 4; L.src_offset[5] += 4; }), 6) == LpcmForm::None);
  row("stereo: the pair at offset 4 mod 8", form(layout(2, true, 2, 4), 2) == LpcmForm::None);
  row("  ... with first_sample = 1: 4 + 4 on the grid", form(layout(2, true, 2, 4), 2, 1) == LpcmForm::S16C);
  row("stereo: first_sample = 2 (8 bytes of a pair)", form(L2, 2, 2) == LpcmForm::S16C);
  row("stereo: first_sample = 6", form(L2, 2, 6) == LpcmForm::S16C);
  row("stereo: first_sample = 1 (4 bytes: off the grid)", form(L2, 2, 1) == LpcmForm::None);
  row("stereo: first_sample = 3", form(L2, 2, 3) == LpcmForm::None);
  row("5.1: first_sample = 2: the pairs on the grid, C and LFE 4 bytes off it", form(L6, 6, 2) == LpcmForm::None);
  row("5.1: first_sample = 4", form(L6, 6, 4) == LpcmForm::S16C);
  row("5.1: first_sample = 1", form(L6, 6, 1) == LpcmForm::None);
  row("stereo: the partner at +4 instead of +2", form(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_offset[1] = L.src_offset[0] + 4; }), 2) == LpcmForm::None);
  row("stereo: the partner in front (R L)", form(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_offset[0] = 2; L.src_offset[1] = 0; }), 2) == LpcmForm::None);
  row("7.1.4: the last pair's partner at +4", form(with_l(L12, [](iamf_hip_lpcm_layout &L) { L.src_offset[11] += 2; }), 12) == LpcmForm::None);
  row("5.1: a pair on (1,2), 0 mono", form(with_l(layout(6, false), [](iamf_hip_lpcm_layout &L) {
        L.src_step[1] = L.src_step[2] = 4;
        L.src_offset[2] = L.src_offset[1] + 2;
      }), 6) == LpcmForm::None);
  row("5.1: a pair on (2,3) as well (C and LFE coupled)", form(with_l(L6, [](iamf_hip_lpcm_layout &L) {
        L.src_step[2] = L.src_step[3] = 4;
        L.src_offset[3] = L.src_offset[2] + 2;
      }), 6) == LpcmForm::None);
  row("5.1: C with step 4", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_step[2] = 4; }), 6) == LpcmForm::None);
  row("5.1: LFE at offset 4 mod 8", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[3] += 4; }), 6) == LpcmForm::None);
  row("5.1: one half of a pair with step 2", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_step[5] = 2; }), 6) == LpcmForm::None);
  row("5.1 as six mono sub-streams", form(layout(6, false), 6) == LpcmForm::None);
  row("5.1: (0,1) coupled, (4,5) two mono sub-streams", form(with_l(L6, [](iamf_hip_lpcm_layout &L) {
        L.src_step[4] = L.src_step[5] = 2;
        L.src_offset[5] = L.src_offset[4] + 2 * kFs;
      }), 6) == LpcmForm::None);
  row("stereo as two mono sub-streams (and no list of the 16-bit family has M = 2)", form(layout(2, false), 2) == LpcmForm::None && !LpcmM::has(2));
  row("24-bit coupled stereo", form(layout(2, true, 3), 2) == LpcmForm::None);
  row("24-bit coupled 5.1", form(layout(6, true, 3), 6) == LpcmForm::None);
  row("32-bit coupled stereo", form(layout(2, true, 4), 2) == LpcmForm::None);
  row("big-endian", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.little_endian = 0; }), 6) == LpcmForm::None);
  row("a missing channel: the first of a pair", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[4] = -1; }), 6) == LpcmForm::None);
  row("a missing channel: the second of a pair", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[1] = -1; }), 6) == LpcmForm::None);
  row("a missing channel: LFE", form(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[3] = -1; }), 6) == LpcmForm::None);
  row("raw_frame_stride 4 mod 8", form(L6, 6, 0, 4 * kRow, kRow + 4) == LpcmForm::None);
  row("raw_stream_stride 4 mod 8", form(L6, 6, 0, 4 * kRow + 4, kRow) == LpcmForm::None);
  row("d_raw + 8 B (16-byte alignment)", form(L6, 6, 0, 4 * kRow, kRow, kRaw + 8) == LpcmForm::None);

  // ---- the rows of the other forms that look at the same fields keep their answers ----
  const iamf_hip_lpcm_layout M16 = layout(16, false);
  row("16 mono runs: the 16-bit form", form(M16, 16) == LpcmForm::S16);
  row("  src_step == 4 on one channel of 16", form(with_l(M16, [](iamf_hip_lpcm_layout &L) { L.src_step[0] = 4; }), 16) == LpcmForm::None);
  row("  24 bit, src_step == 6 on (0,1) of 16", form(with_l(layout(16, false, 3), [](iamf_hip_lpcm_layout &L) {
        L.src_step[0] = L.src_step[1] = 6;
        L.src_offset[1] = 3;
      }), 16) == LpcmForm::None);
  row("  one mono run: the 16-bit form (a mono channel-based element)", form(layout(1, false), 1) == LpcmForm::S16);

  // ---- routing ----
  for_each_int(LpcmCoupledM{}, [&](int m) {
    for_each_int(LpcmOC{}, [&](int oc) {
      snprintf(what, sizeof(what), "coupled packets, m = %d into %d channel(s): LpcmCoupled, early", m, oc);
      expect(what, call(m, oc, 1), m, nullptr, Family::LpcmCoupled, 1);
    });
  });
  int rows = 0;
  for_each_render_instance_lpcm_coupled([&](int f, int v, int m, int oc, int) {
    rows += (f == IAMF_HIP_ROUTE_LPCM_COUPLED && (v == 0 || v == 1) && LpcmCoupledM::has(m) && LpcmOC::has(oc)) ? 1 : 1000;
  });
  row("the family's listing: LpcmCoupledM x LpcmOC x {late, early} = 20 rows of family 17", rows == 20);
  expect("  lpcm_coupled with m = 4: refused", call(4, 2, 1), 4, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled with m = 16: refused", call(16, 2, 1), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled with m = 1: refused", call(1, 2, 1), 1, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 0 with m = 6: refused as before", call(6, 2, 0), 6, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 0 with m = 2: refused as before", call(2, 2, 0), 2, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 0 with m = 4: the 16-bit family as before", call(4, 2, 0), 4, nullptr, Family::Lpcm, 1);
  expect("  lpcm_coupled with 24-bit samples: refused", with(call(6, 2, 1), [](RenderParams &p) { p.lpcm_bytes = 3; }), 6, nullptr,
         Family::Refused, 0, STATE);
  expect("  lpcm_bytes = 0 (16 bit): LpcmCoupled", with(call(6, 2, 1), [](RenderParams &p) { p.lpcm_bytes = 0; }), 6, nullptr,
         Family::LpcmCoupled, 1);

  // ---- the prefetch variant by the launch's size, and the switches ----
  const RenderParams pc = call(12, 2, 1);
  int cut = 0;   // the largest launch lpcm_coupled_early() still gives the early variant; one cut or one variant
  for (int n = 1; n <= 65536; ++n)
    if (lpcm_coupled_early(n)) cut = n;
  row("lpcm_coupled_early: one cut (early up to it, late beyond) or one variant for every size", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (lpcm_coupled_early(n) != (n <= cut)) return false;
    return true;
  }());
  row("lpcm_coupled_fused: every size up to 65536 (no size has been measured to lose)", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (!lpcm_coupled_fused(n)) return false;
    return true;
  }());
  expect("  n_launch = 1: what lpcm_coupled_early(1) says", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 1; }), 12, nullptr,
         Family::LpcmCoupled, lpcm_coupled_early(1));
  expect("  n_launch = 65536: what lpcm_coupled_early(65536) says", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 12,
         nullptr, Family::LpcmCoupled, lpcm_coupled_early(65536));
  if (cut > 0 && cut < 65536) {
    expect("  n_launch at the cut: early", with(pc, [&](RenderParams &p) { p.n_launch = p.n_streams = cut; }), 12, nullptr, Family::LpcmCoupled, 1);
    expect("  n_launch one beyond the cut: late", with(pc, [&](RenderParams &p) { p.n_launch = p.n_streams = cut + 1; }), 12, nullptr,
           Family::LpcmCoupled, 0);
  }
  expect("  IAMF_HIP_LP_LATE", pc, 12, "IAMF_HIP_LP_LATE", Family::LpcmCoupled, 0);
  expect("  IAMF_HIP_LP_EARLY at 65536 workgroups", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 12,
         "IAMF_HIP_LP_EARLY", Family::LpcmCoupled, 1);
  setenv("IAMF_HIP_LP_EARLY", "1", 1);
  expect("  both switches: late", pc, 12, "IAMF_HIP_LP_LATE", Family::LpcmCoupled, 0);
  unsetenv("IAMF_HIP_LP_EARLY");

  // ---- each refusal of Family::Lpcm holds for Family::LpcmCoupled ----
  expect("  3 output channels: no instance", call(6, 3, 1), 6, nullptr, Family::Refused, 0, STATE);
  expect("  6 output channels: no instance", call(12, 6, 1), 12, nullptr, Family::Refused, 0, STATE);
  expect("  limiter off", with(pc, [](RenderParams &p) { p.limiter_on = 0; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(pc, [](RenderParams &p) { p.pos0 = 8; }), 12, nullptr, Family::Refused, 0, STATE);
  // the staged limiter-table window (kFWin, render_fast.hpp): (n_atk, n_end) = (6, 1087) at 5407 Hz and (6, 1088) at 5408 Hz
  expect("  n_end = kFWin - 1: a table that ends inside the staged window", with(pc, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; }), 12,
         nullptr, Family::Refused, 0, STATE);
  expect("  n_end = kFWin", with(pc, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; }), 12, nullptr, Family::LpcmCoupled, 1);
  expect("  pos0 = 250: off the 16-sample grid, past the look-ahead", with(pc, [](RenderParams &p) { p.pos0 = 250; }), 12, nullptr,
         Family::LpcmCoupled, 1);
  expect("  total % 64 != 0", with(pc, [](RenderParams &p) { p.total = 4096 + 32; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  down-mixer", with(call(6, 2, 1), [](RenderParams &p) { p.dmx_on = 1; }), 6, nullptr, Family::Refused, 0, STATE);
  expect("  an output ramp off the 16-byte grid", with(pc, [](RenderParams &p) { p.out_ramp = kIn + 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  IAMF_HIP_FORCE_GENERIC", pc, 12, "IAMF_HIP_FORCE_GENERIC", Family::Refused, 0, STATE);
  expect("  pcm + 2 B", with(pc, [](RenderParams &p) { p.pcm += 2; }), 12, nullptr, Family::Refused, 0, STATE);
  constexpr int64_t kLpMax = 355117736;     // the 32-bit bound of the packet offsets, as for the other forms
  expect("  lpcm_frame_stride at the 32-bit bound", with(pc, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 12, nullptr,
         Family::LpcmCoupled, 1);
  expect("  lpcm_frame_stride 8 bytes beyond", with(pc, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 8; }), 12, nullptr,
         Family::Refused, 0, STATE);

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
