// Host-only check of the two-element 24-bit packet form: the second element's forms as lpcm_form_packets() answers them
// (iac_amd/csrc/lpcm_form.hpp) and the routing (pick_route() in iac_amd/csrc/render_route.hpp, Family::Lpcm24Mix: lpcm_mix ==
// (4 | LP2) with lpcm_bytes == 3, lpcm_coupled == 2 for a coupled bed).  One row per rule, each a well-formed call with exactly
// one pointer, stride, bound, form or flag changed.  render_fast_kernel<.., LP, true, 3, LPC, LP2> reads element 1 through
// a buffer resource without a bound of its own, 12 bytes per load on the dword grid: a wrong row here is wrong PCM or a
// stray load on the GPU, not a slower rate.  The pinned refusals of lpcm_mix 1 / 2 / 3 are asked again.
// Driven by tests/test_route_host_lpcm24_mix.py.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../../include/iamf_hip.h"

namespace {
#include "../../iac_amd/csrc/render_params.hpp"
#include "../../iac_amd/csrc/render_route.hpp"
#include "route_sets.hpp"
#include "../../iac_amd/csrc/lpcm_form.hpp"

int g_failed = 0, g_cases = 0;

void row(const char *what, bool ok) {
  printf("%-110s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kRamp = reinterpret_cast<float *>(0x20000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
constexpr uintptr_t kRaw = 0x50000, kRaw2 = 0x90000;
constexpr int kFs = 1024;

// the aligned call of route_host_lpcm_mix_check.cpp with 24-bit packets on both elements: lpcm_mix = 4 | lp2
RenderParams call(int m, int out_ch, int coupled, int lp2, int m2) {
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
  p.lpcm_frame_stride = 16 * kFs * 3;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
  p.lpcm_bytes = 3;
  p.lpcm_coupled = coupled;
  p.lpcm_mix = 4 | lp2;
  p.in2 = reinterpret_cast<const float *>(kRaw2);   // the second element's packets: address, strides in bytes
  p.in2_frame_stride = 4 * kFs * 3 + 4;             // (on the dword grid only)
  p.in2_stream_stride = 4 * p.in2_frame_stride;
  p.m2 = m2;
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
  bool listed = true;   // a route of the family names a row of the family's listing, set 8, and no row of sets 0 .. 7
  if (r.family == Family::Lpcm24Mix) {
    const RouteKey k = route_key(r, p, m);
    listed = false;
    for_each_render_instance_lpcm24_mix([&](int f, int v, int km, int kc, int kk) { listed = listed || same_key(k, f, v, km, kc, kk); });
    listed = listed && k.set == 8 && k.set >= kRouteTables && sets_of_key(k.family, k.variant, k.m, k.c, k.k) == 1 << 8;
    listed = listed && k.family == IAMF_HIP_ROUTE_LPCM24_MIX && k.variant == 0 && k.k == p.lpcm_mix - 4;
  }
  row(what, r.family == family && r.variant == variant && r.err == err && listed);
}

// a second element of ch channels: mono runs, or (coupled) one interleaved pair
iamf_hip_lpcm_layout layout2(int ch, bool coupled, int bytes = 3, int head = 0) {
  iamf_hip_lpcm_layout L;
  memset(&L, 0, sizeof(L));
  L.sample_bytes = bytes;
  L.little_endian = 1;
  L.channels = ch;
  L.frame_size = kFs;
  for (int c = 0; c < ch; ++c) {
    L.src_offset[c] = coupled ? head + bytes * c : head + c * kFs * bytes;
    L.src_step[c] = coupled ? ch * bytes : bytes;
  }
  return L;
}
constexpr int64_t kRow = 5 * kFs * 4;
LpcmForm packets(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw2) {
  return lpcm_form_packets(L, ch, ss, fst, raw, first);
}
LpcmForm form(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw2) {
  return lpcm_form(L, ch, ss, fst, raw, first);
}
// the mix form's rule for element 1 as iamf_render.hip states it: the sample size of element 0 (24 bit), mono runs of 1 or 4
// channels under the S24 rule or one pair under lpcm_form_coupled24()
int lp2_of(LpcmForm f, int m2) {
  if (f != LpcmForm::S24 && f != LpcmForm::S24C) return 0;
  const int lp2 = f == LpcmForm::S24C ? 2 : 1;
  return lpcm_mix_m2_ok(lp2, m2) ? lp2 : 0;
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  const int STATE = IAMF_HIP_ERR_INVALID_STATE;
  const LpcmForm None = LpcmForm::None, S24 = LpcmForm::S24, S24C = LpcmForm::S24C;
  char what[200];

  // ---- the numbers and the pinned sizes ----
  static_assert(IAMF_HIP_ROUTE_LPCM24_MIX == 33, "stable number (32 stays unused)");
  static_assert((int)Family::Lpcm24Mix == (int)Family::Lpcm24Coupled + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 8 + 1 && kRouteTables == 3, "set 8 behind the three tables; sets added later leave it alone");
  static_assert(sizeof(RenderParams) == 616 && sizeof(RenderMixParams) == 656, "the blocks keep their sizes");
  static_assert(offsetof(RenderParams, interleaved) == 380 && offsetof(RenderParams, dump) == 384 && offsetof(RenderParams, ragged) == 412 &&
                    offsetof(RenderParams, lfe_div) == 416 && offsetof(RenderParams, lpcm) == 528 && offsetof(RenderParams, lpcm_off) == 552,
                "no field moved");
  static_assert(sizeof(RenderMixParams) - sizeof(RenderParams) == 8 + 2 * 8 + 4 * 4, "nor was one added behind the block");
  row("every instance is built for 4, 3 or 2 workgroups per CU, the 16-bit ones as they were", [&] {
    bool ok = true;
    for_each_render_instance_lpcm24_mix([&](int, int, int m, int oc, int k) {
      ok = ok && lpcm24_mix_wgs(m, oc, k) >= 2 && lpcm24_mix_wgs(m, oc, k) <= 4 && lpcm_mix_wgs(m, oc, k) == 4;
    });
    return ok;
  }());

  // ---- the form of the second element: lpcm_form_packets() on its own layout ----
  row("second element, mono: S24, LP2 = 1", packets(layout2(1, false), 1) == S24 && lp2_of(S24, 1) == 1);
  row("second element, four mono runs: S24, LP2 = 1", packets(layout2(4, false), 4) == S24 && lp2_of(S24, 4) == 1);
  row("second element, a coupled pair: S24C through the wrapper, None from lpcm_form(); LP2 = 2",
      packets(layout2(2, true), 2) == S24C && form(layout2(2, true), 2) == None && lp2_of(S24C, 2) == 2);
  row("  ... dword-aligned only (head 4)", packets(layout2(2, true, 3, 4), 2) == S24C && packets(layout2(4, false, 3, 4), 4) == S24);
  row("  ... first_sample 64", packets(layout2(2, true), 2, 64) == S24C && packets(layout2(4, false), 4, 64) == S24);
  row("  ... first_sample 2: a pair's 12 bytes on the grid, a mono run's 6 off it", packets(layout2(2, true), 2, 2) == S24C && packets(layout2(4, false), 4, 2) == None);
  row("  ... first_sample 1: off the grid for both", packets(layout2(2, true), 2, 1) == None && packets(layout2(1, false), 1, 1) == None);
  row("second element, stereo as two mono runs: S24 from both, and no form of the mix", packets(layout2(2, false), 2) == S24 &&
                                                                                               form(layout2(2, false), 2) == S24 && lp2_of(S24, 2) == 0);
  row("second element, three mono runs: no form of the mix", packets(layout2(3, false), 3) == S24 && lp2_of(S24, 3) == 0);
  row("second element, 16-bit mono / pair: the 16-bit forms, no form of the 24-bit mix",
      packets(layout2(1, false, 2), 1) == LpcmForm::S16 && packets(layout2(2, true, 2), 2) == LpcmForm::S16C && lp2_of(LpcmForm::S16, 1) == 0 &&
          lp2_of(LpcmForm::S16C, 2) == 0);
  row("second element, 32-bit mono / pair: unpacked", packets(layout2(1, false, 4), 1) == None && packets(layout2(2, true, 4), 2) == None);
  row("second element, big-endian mono / pair: unpacked", [&] {
    iamf_hip_lpcm_layout L = layout2(1, false), P = layout2(2, true);
    L.little_endian = P.little_endian = 0;
    return packets(L, 1) == None && packets(P, 2) == None;
  }());
  row("second element: d_raw + 8 B: unpacked", packets(layout2(1, false), 1, 0, 4 * kRow, kRow, kRaw2 + 8) == None &&
                                                   packets(layout2(2, true), 2, 0, 4 * kRow, kRow, kRaw2 + 8) == None);
  row("second element: a stride 2 mod 4: unpacked", packets(layout2(1, false), 1, 0, 4 * kRow + 2, kRow) == None && packets(layout2(1, false), 1, 0, 4 * kRow, kRow + 2) == None &&
                                                        packets(layout2(2, true), 2, 0, 4 * kRow + 2, kRow) == None && packets(layout2(2, true), 2, 0, 4 * kRow, kRow + 2) == None);
  row("second element: a stride 4 mod 8: the dword grid is enough", packets(layout2(1, false), 1, 0, 4 * kRow + 4, kRow + 4) == S24 &&
                                                                        packets(layout2(2, true), 2, 0, 4 * kRow + 4, kRow + 4) == S24C);
  row("second element, a pair whose partner lies 6 bytes on: unpacked", [&] {
    iamf_hip_lpcm_layout P = layout2(2, true);
    P.src_offset[1] = 6;
    return packets(P, 2) == None;
  }());

  // ---- routing: every instance ----
  int rows = 0;
  for_each_render_instance_lpcm24_mix([&](int f, int v, int m, int oc, int k) {
    rows += (f == IAMF_HIP_ROUTE_LPCM24_MIX && v == 0 && (LpcmM::has(m) || LpcmCoupledM::has(m)) && LpcmOC::has(oc) && LpcmMixK::has(k)) ? 1 : 1000;
    snprintf(what, sizeof(what), "element 0 m = %d (%s) into %d channel(s), second element form %d: Lpcm24Mix", m,
             LpcmCoupledM::has(m) ? "coupled" : "mono-coded", oc, k);
    expect(what, call(m, oc, LpcmCoupledM::has(m) ? 2 : 0, k, k == 2 ? 2 : (m & 1 ? 1 : 4)), m, nullptr, Family::Lpcm24Mix, k);
  });
  row("the family's listing: (LpcmM + LpcmCoupledM) x LpcmOC x {1, 2} = 36 rows of family 33", rows == 36);
  row("set 8 of for_each_instance_of_set is the listing: 36 rows, family 33 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_LPCM24_MIX, 8, 36));
  row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
  row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  row("lpcm24_mix_fused: one answer per size, whatever it is, and the route does not depend on it", [&] {
    bool ok = true;
    for (int n = 1; n <= 65536; n += 97) ok = ok && (lpcm24_mix_fused(n) == true || lpcm24_mix_fused(n) == false);
    return ok;
  }());

  // ---- the pinned refusals hold ----
  const RenderParams pm = call(16, 2, 0, 2, 2), pc = call(12, 2, 2, 1, 4);
  expect("lpcm_mix = 1 with 24-bit samples: refused as before", with(call(16, 2, 0, 1, 1), [](RenderParams &p) { p.lpcm_mix = 1; }), 16, nullptr,
         Family::Refused, 0, STATE);
  expect("lpcm_mix = 2 with 24-bit samples: refused as before", with(pm, [](RenderParams &p) { p.lpcm_mix = 2; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("lpcm_mix = 2 with 24-bit samples and lpcm_coupled = 2: refused as before", with(call(12, 2, 2, 2, 2), [](RenderParams &p) { p.lpcm_mix = 2; }), 12,
         nullptr, Family::Refused, 0, STATE);
  expect("lpcm_mix = 3: no such form", with(pm, [](RenderParams &p) { p.lpcm_mix = 3; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("lpcm_mix = 3 with 16-bit samples: no such form", with(pm, [](RenderParams &p) { p.lpcm_mix = 3; p.lpcm_bytes = 2; }), 16, nullptr,
         Family::Refused, 0, STATE);
  expect("lpcm_mix = 2 with 16-bit samples: LpcmMix as before", with(pm, [](RenderParams &p) { p.lpcm_mix = 2; p.lpcm_bytes = 2; p.in2_frame_stride = 4 * kFs * 2; p.in2_stream_stride = 16 * kFs * 2; }),
         16, nullptr, Family::LpcmMix, 2);
  expect("lpcm_mix = 0, lpcm_coupled = 2: Lpcm24Coupled as before", with(call(12, 2, 2, 1, 4), [](RenderParams &p) { p.lpcm_mix = 0; p.in2 = nullptr; }), 12, nullptr,
         Family::Lpcm24Coupled, lpcm24_coupled_early(64));
  expect("lpcm_mix = 0, mono-coded 24-bit: Lpcm24 as before", with(call(16, 2, 0, 1, 1), [](RenderParams &p) { p.lpcm_mix = 0; p.in2 = nullptr; }), 16, nullptr,
         Family::Lpcm24, 1);

  // ---- the form's own values ----
  expect("  lpcm_mix = 4: no form", with(pm, [](RenderParams &p) { p.lpcm_mix = 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 7: no form", with(pm, [](RenderParams &p) { p.lpcm_mix = 7; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 9: no form", with(pm, [](RenderParams &p) { p.lpcm_mix = 9; p.m2 = 1; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 6 with 16-bit samples: refused", with(pm, [](RenderParams &p) { p.lpcm_bytes = 2; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 6 with lpcm_bytes = 0 (16 bit): refused", with(pm, [](RenderParams &p) { p.lpcm_bytes = 0; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 6 with 32-bit samples: refused", with(pm, [](RenderParams &p) { p.lpcm_bytes = 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 5 with lpcm_coupled = 1 (the 16-bit coupling): refused", with(pc, [](RenderParams &p) { p.lpcm_coupled = 1; }), 12, nullptr,
         Family::Refused, 0, STATE);
  expect("  the switches of the prefetch variant do not matter: IAMF_HIP_LP_LATE", pm, 16, "IAMF_HIP_LP_LATE", Family::Lpcm24Mix, 2);
  expect("  n_launch = 65536", with(pm, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16, nullptr, Family::Lpcm24Mix, 2);

  // ---- the refusals of Family::LpcmMix, one field changed at a time ----
  expect("  mono-coded packets with m = 6: refused", call(6, 2, 0, 1, 1), 6, nullptr, Family::Refused, 0, STATE);
  expect("  coupled packets with m = 16: refused", call(16, 2, 2, 1, 1), 16, nullptr, Family::Refused, 0, STATE);
  expect("  m = 14: refused", call(14, 2, 0, 1, 1), 14, nullptr, Family::Refused, 0, STATE);
  expect("  3 output channels: no instance", call(16, 3, 0, 1, 1), 16, nullptr, Family::Refused, 0, STATE);
  expect("  6 output channels: no instance", call(12, 6, 2, 2, 2), 12, nullptr, Family::Refused, 0, STATE);
  expect("  limiter off", with(pm, [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(pm, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 16", with(pm, [](RenderParams &p) { p.pos0 = 16; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  n_end = kFWin - 1: a table that ends inside the staged window", with(pm, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; }), 16,
         nullptr, Family::Refused, 0, STATE);
  expect("  n_end = kFWin", with(pm, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  pos0 = 250: off the 16-sample grid, past the look-ahead", with(pm, [](RenderParams &p) { p.pos0 = 250; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  pos0 = 239", with(pm, [](RenderParams &p) { p.pos0 = 239; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  total % 64 != 0", with(pm, [](RenderParams &p) { p.total = 4096 + 32; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  down-mixer", with(pc, [](RenderParams &p) { p.dmx_on = 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  demixer", with(pc, [](RenderParams &p) { p.demix_on = 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  de-mapping matrix", with(pm, [](RenderParams &p) { p.pre_matrix = kIn; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  HRTF stage", with(pm, [](RenderParams &p) { p.fir_taps = 256; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  output gain on fewer channels than rendered", with(pm, [](RenderParams &p) { p.og_ch = 1; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  IAMF_HIP_FORCE_GENERIC", pm, 16, "IAMF_HIP_FORCE_GENERIC", Family::Refused, 0, STATE);
  expect("  pcm + 2 B", with(pm, [](RenderParams &p) { p.pcm += 2; }), 16, nullptr, Family::Refused, 0, STATE);
  // the 32-bit bound of the packet offsets (fast_shape_ok): (total / fs + 2) * stride + 2^24 < 2^31
  constexpr int64_t kLpMax = 355117736;
  static_assert((4096 / kFs + 2) * kLpMax + ((int64_t)1 << 24) < ((int64_t)1 << 31) && (4096 / kFs + 2) * (kLpMax + 4) + ((int64_t)1 << 24) >= ((int64_t)1 << 31),
                "the last stride on the dword grid inside the bound");
  expect("  lpcm_frame_stride at the 32-bit bound", with(pm, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  lpcm_frame_stride 4 bytes beyond", with(pm, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 4; }), 16, nullptr, Family::Refused, 0, STATE);
  // the second element's packets
  expect("  no second element", with(pm, [](RenderParams &p) { p.in2 = nullptr; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a coupled second element of 4 channels", with(pm, [](RenderParams &p) { p.m2 = 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a coupled second element of 1 channel", with(pm, [](RenderParams &p) { p.m2 = 1; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 2 channels", with(pc, [](RenderParams &p) { p.m2 = 2; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 3 channels", with(pc, [](RenderParams &p) { p.m2 = 3; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 1 channel", with(pc, [](RenderParams &p) { p.m2 = 1; }), 12, nullptr, Family::Lpcm24Mix, 1);
  expect("  a second element of 6 channels", with(pc, [](RenderParams &p) { p.m2 = 6; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  second element's packets + 8 B (16-byte alignment)",
         with(pm, [](RenderParams &p) { p.in2 = reinterpret_cast<const float *>(kRaw2 + 8); }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's packets + 4 B", with(pm, [](RenderParams &p) { p.in2 = reinterpret_cast<const float *>(kRaw2 + 4); }), 16, nullptr,
         Family::Refused, 0, STATE);
  expect("  second element's frame stride 2 mod 4", with(pm, [](RenderParams &p) { p.in2_frame_stride += 2; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's stream stride 2 mod 4", with(pm, [](RenderParams &p) { p.in2_stream_stride += 2; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's frame stride + 4: on the grid", with(pm, [](RenderParams &p) { p.in2_frame_stride += 4; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  second element's stream stride + 4: on the grid", with(pm, [](RenderParams &p) { p.in2_stream_stride += 4; }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  second element's frame stride at the 32-bit bound", with(pm, [](RenderParams &p) { p.in2_frame_stride = kLpMax; }), 16, nullptr,
         Family::Lpcm24Mix, 2);
  expect("  second element's frame stride 4 bytes beyond", with(pm, [](RenderParams &p) { p.in2_frame_stride = kLpMax + 4; }), 16, nullptr,
         Family::Refused, 0, STATE);
  // ramps: fast_shape_ok's rules
  expect("  three aligned ramps: fused", with(pm, [](RenderParams &p) {
           p.elem_ramp = kRamp, p.elem2_ramp = kRamp + 8192, p.out_ramp = kRamp + 16384;
           p.ramp_stream_stride = 4096;
         }), 16, nullptr, Family::Lpcm24Mix, 2);
  expect("  an output ramp off the 16-byte grid", with(pm, [](RenderParams &p) { p.out_ramp = kRamp + 1, p.ramp_stream_stride = 4096; }), 16, nullptr,
         Family::Refused, 0, STATE);
  expect("  an element-2 ramp off the 16-byte grid", with(pm, [](RenderParams &p) { p.elem2_ramp = kRamp + 2, p.ramp_stream_stride = 4096; }), 16,
         nullptr, Family::Refused, 0, STATE);
  expect("  ramp_stream_stride 2 mod 4", with(pm, [](RenderParams &p) { p.elem_ramp = kRamp, p.ramp_stream_stride = 4098; }), 16, nullptr,
         Family::Refused, 0, STATE);

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
