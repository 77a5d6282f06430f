// Host-only check of the two-element packet form: its routing (pick_route() in iac_amd/csrc/render_route.hpp,
// Family::LpcmMix, reached through the host-only field RenderParams::lpcm_mix) and the form of each element, which is
// lpcm_form() (iac_amd/csrc/lpcm_form.hpp) applied to that element's own layout, unchanged.  One row per rule, each an
// aligned call with exactly one field changed.  render_fast_kernel<.., LP2> reads the second element's packets through a
// buffer resource with 32-bit offsets, 8 or 16 bytes per lane: a wrong row here is a misaligned or out-of-range load on the
// GPU, not a slower rate.
// Driven by tests/test_route_host_lpcm_mix.py.
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
  printf("%-100s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kRamp = reinterpret_cast<float *>(0x20000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
constexpr uintptr_t kRaw = 0x50000, kRaw2 = 0x90000;
constexpr int kFs = 1024;

// the aligned call of route_host_lpcm_coupled_check.cpp with a second element of m2 channels as 16-bit packets of form lp2
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
  p.lpcm_frame_stride = 16 * kFs * 2;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
  p.lpcm_bytes = 2;
  p.lpcm_coupled = coupled;
  p.lpcm_mix = lp2;
  p.in2 = reinterpret_cast<const float *>(kRaw2);   // the second element's packets: address, strides in bytes
  p.in2_frame_stride = 4 * kFs * 2;
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
  bool listed = true;   // a route of the family names a row of the family's listing and no row of any other set
  if (r.family == Family::LpcmMix) {
    const RouteKey k = route_key(r, p, m);
    listed = false;
    for_each_render_instance_lpcm_mix([&](int f, int v, int km, int kc, int kk) { listed = listed || same_key(k, f, v, km, kc, kk); });
    for_each_render_instance([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_ext([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm24([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm_coupled([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    listed = listed && k.family == IAMF_HIP_ROUTE_LPCM_MIX && k.variant == 0 && k.k == p.lpcm_mix;
  }
  row(what, r.family == family && r.variant == variant && r.err == err && listed);
}

// a second element of ch channels: mono runs, or (coupled) one interleaved pair
iamf_hip_lpcm_layout layout2(int ch, bool coupled, int bytes = 2, int head = 0) {
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
LpcmForm form(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw2) {
  return lpcm_form(L, ch, ss, fst, raw, first);
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  const int STATE = IAMF_HIP_ERR_INVALID_STATE;
  char what[200];

  // ---- the number, and the second element's forms the kernel is built for ----
  // (20 .. 23 are the resampler's families; 18, 19 and 24 are held free by tests/test_lpcm_coupled_cpu.py)
  static_assert(IAMF_HIP_ROUTE_LPCM_MIX == 25, "stable number");
  static_assert(IAMF_HIP_ROUTE_LPCM_MIX != IAMF_HIP_ROUTE_RS_PLAIN && IAMF_HIP_ROUTE_LPCM_MIX != IAMF_HIP_ROUTE_RS_DIRECT, "a number of its own");
  static_assert(lpcm_mix_m2_ok(1, 1) && lpcm_mix_m2_ok(1, 4) && !lpcm_mix_m2_ok(1, 2) && !lpcm_mix_m2_ok(1, 3) && !lpcm_mix_m2_ok(1, 5),
                "mono-coded second element: mono or first-order ambisonics");
  static_assert(lpcm_mix_m2_ok(2, 2) && !lpcm_mix_m2_ok(2, 1) && !lpcm_mix_m2_ok(2, 4) && !lpcm_mix_m2_ok(0, 1) && !lpcm_mix_m2_ok(3, 2),
                "coupled second element: one stereo pair");
  static_assert(kFIn2 == 4, "the mixing variants take a second element of up to four channels");
  row("every instance is built for 4, 3 or 2 workgroups per CU", [&] {
    bool ok = true;
    for_each_render_instance_lpcm_mix([&](int, int, int m, int oc, int k) { ok = ok && lpcm_mix_wgs(m, oc, k) >= 2 && lpcm_mix_wgs(m, oc, k) <= 4; });
    return ok;
  }());

  // ---- the form of the second element: lpcm_form() on its own layout, no new rule ----
  row("second element, mono: the 16-bit form", form(layout2(1, false), 1) == LpcmForm::S16);
  row("second element, four mono runs: the 16-bit form", form(layout2(4, false), 4) == LpcmForm::S16);
  row("second element, a coupled pair: the coupled form", form(layout2(2, true), 2) == LpcmForm::S16C);
  row("  ... 8-byte aligned only (head 8)", form(layout2(2, true, 2, 8), 2) == LpcmForm::S16C);
  row("  ... first_sample 64", form(layout2(2, true), 2, 64) == LpcmForm::S16C && form(layout2(4, false), 4, 64) == LpcmForm::S16);
  row("  ... first_sample 1 (mono runs) / 1 (pair): off the grid", form(layout2(4, false), 4, 1) == LpcmForm::None && form(layout2(2, true), 2, 1) == LpcmForm::None);
  row("second element, stereo as two mono runs: unpacked", form(layout2(2, false), 2) == LpcmForm::None);
  row("second element, 24-bit mono: not a form the mix takes", form(layout2(1, false, 3), 1) == LpcmForm::S24);
  row("second element, 24-bit pair: unpacked", form(layout2(2, true, 3), 2) == LpcmForm::None);
  row("second element, big-endian: unpacked", [&] {
    iamf_hip_lpcm_layout L = layout2(1, false);
    L.little_endian = 0;
    return form(L, 1) == LpcmForm::None;
  }());
  row("second element: d_raw + 8 B / a stride 4 mod 8: unpacked",
      form(layout2(1, false), 1, 0, 4 * kRow, kRow, kRaw2 + 8) == LpcmForm::None && form(layout2(1, false), 1, 0, 4 * kRow + 4, kRow) == LpcmForm::None &&
          form(layout2(1, false), 1, 0, 4 * kRow, kRow + 4) == LpcmForm::None);

  // ---- routing: every instance ----
  int rows = 0;
  for_each_render_instance_lpcm_mix([&](int f, int v, int m, int oc, int k) {
    rows += (f == IAMF_HIP_ROUTE_LPCM_MIX && v == 0 && (LpcmM::has(m) || LpcmCoupledM::has(m)) && LpcmOC::has(oc) && LpcmMixK::has(k)) ? 1 : 1000;
    snprintf(what, sizeof(what), "element 0 m = %d (%s) into %d channel(s), second element form %d: LpcmMix", m,
             LpcmCoupledM::has(m) ? "coupled" : "mono-coded", oc, k);
    expect(what, call(m, oc, LpcmCoupledM::has(m) ? 1 : 0, k, k == 2 ? 2 : (m & 1 ? 1 : 4)), m, nullptr, Family::LpcmMix, k);
  });
  row("the family's listing: (LpcmM + LpcmCoupledM) x LpcmOC x {1, 2} = 36 rows of family 25", rows == 36);
  row("lpcm_mix_fused: every size up to 65536 (no measured size loses)", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (!lpcm_mix_fused(n)) return false;
    return true;
  }());

  // ---- lpcm_mix == 0: every rule as it stood ----
  expect("lpcm_mix = 0, mono-coded m = 16 with a second f32 element: the 16-bit family as before (render_prepare keeps such calls away)",
         with(call(16, 2, 0, 0, 1), [](RenderParams &p) { p.in2_stream_stride = p.in2_frame_stride = 4096; }), 16, nullptr, Family::Lpcm, 1);
  expect("lpcm_mix = 0, coupled m = 6: LpcmCoupled as before", with(call(6, 2, 1, 0, 1), [](RenderParams &p) { p.in2 = nullptr; }), 6, nullptr,
         Family::LpcmCoupled, 1);

  // ---- one field changed at a time ----
  const RenderParams pm = call(16, 2, 0, 2, 2), pc = call(12, 2, 1, 1, 4);
  expect("  the switches of the prefetch variant do not matter: IAMF_HIP_LP_LATE", pm, 16, "IAMF_HIP_LP_LATE", Family::LpcmMix, 2);
  expect("  n_launch = 65536", with(pm, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16, nullptr, Family::LpcmMix, 2);
  // the refusals of Family::Lpcm / LpcmCoupled
  expect("  mono-coded packets with m = 6: refused", call(6, 2, 0, 1, 1), 6, nullptr, Family::Refused, 0, STATE);
  expect("  coupled packets with m = 16: refused", call(16, 2, 1, 1, 1), 16, nullptr, Family::Refused, 0, STATE);
  expect("  m = 14: refused", call(14, 2, 0, 1, 1), 14, nullptr, Family::Refused, 0, STATE);
  expect("  24-bit element 0: refused", with(pm, [](RenderParams &p) { p.lpcm_bytes = 3; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_bytes = 0 (16 bit): LpcmMix", with(pm, [](RenderParams &p) { p.lpcm_bytes = 0; }), 16, nullptr, Family::LpcmMix, 2);
  expect("  3 output channels: no instance", call(16, 3, 0, 1, 1), 16, nullptr, Family::Refused, 0, STATE);
  expect("  6 output channels: no instance", call(12, 6, 1, 2, 2), 12, nullptr, Family::Refused, 0, STATE);
  expect("  limiter off", with(pm, [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(pm, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Refused, 0, STATE);
  // the staged limiter-table window (kFWin, render_fast.hpp): (n_atk, n_end) = (6, 1087) at 5407 Hz and (6, 1088) at 5408 Hz
  expect("  n_end = kFWin - 1: a table that ends inside the staged window", with(pm, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; }), 16,
         nullptr, Family::Refused, 0, STATE);
  expect("  n_end = kFWin", with(pm, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; }), 16, nullptr, Family::LpcmMix, 2);
  expect("  pos0 = 250: off the 16-sample grid, past the look-ahead", with(pm, [](RenderParams &p) { p.pos0 = 250; }), 16, nullptr, Family::LpcmMix, 2);
  expect("  total % 64 != 0", with(pm, [](RenderParams &p) { p.total = 4096 + 32; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  down-mixer", with(pc, [](RenderParams &p) { p.dmx_on = 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  demixer", with(pc, [](RenderParams &p) { p.demix_on = 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  de-mapping matrix", with(pm, [](RenderParams &p) { p.pre_matrix = kIn; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  HRTF stage", with(pm, [](RenderParams &p) { p.fir_taps = 256; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  output gain on fewer channels than rendered", with(pm, [](RenderParams &p) { p.og_ch = 1; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  IAMF_HIP_FORCE_GENERIC", pm, 16, "IAMF_HIP_FORCE_GENERIC", Family::Refused, 0, STATE);
  expect("  pcm + 2 B", with(pm, [](RenderParams &p) { p.pcm += 2; }), 16, nullptr, Family::Refused, 0, STATE);
  constexpr int64_t kLpMax = 355117736;     // the 32-bit bound of the packet offsets, as for the other forms
  expect("  lpcm_frame_stride at the 32-bit bound", with(pm, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 16, nullptr, Family::LpcmMix, 2);
  expect("  lpcm_frame_stride 8 bytes beyond", with(pm, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 8; }), 16, nullptr, Family::Refused, 0, STATE);
  // the second element's packets
  expect("  no second element", with(pm, [](RenderParams &p) { p.in2 = nullptr; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix = 3: no such form", with(pm, [](RenderParams &p) { p.lpcm_mix = 3; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a coupled second element of 4 channels", with(pm, [](RenderParams &p) { p.m2 = 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a coupled second element of 1 channel", with(pm, [](RenderParams &p) { p.m2 = 1; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 2 channels", with(pc, [](RenderParams &p) { p.m2 = 2; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 3 channels", with(pc, [](RenderParams &p) { p.m2 = 3; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  a mono-coded second element of 1 channel", with(pc, [](RenderParams &p) { p.m2 = 1; }), 12, nullptr, Family::LpcmMix, 1);
  expect("  a second element of 6 channels", with(pc, [](RenderParams &p) { p.m2 = 6; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  second element's packets + 8 B (16-byte alignment)",
         with(pm, [](RenderParams &p) { p.in2 = reinterpret_cast<const float *>(kRaw2 + 8); }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's frame stride 4 mod 8", with(pm, [](RenderParams &p) { p.in2_frame_stride += 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's stream stride 4 mod 8", with(pm, [](RenderParams &p) { p.in2_stream_stride += 4; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  second element's frame stride + 8: on the grid", with(pm, [](RenderParams &p) { p.in2_frame_stride += 8; }), 16, nullptr, Family::LpcmMix, 2);
  expect("  second element's frame stride at the 32-bit bound", with(pm, [](RenderParams &p) { p.in2_frame_stride = kLpMax; }), 16, nullptr,
         Family::LpcmMix, 2);
  expect("  second element's frame stride 8 bytes beyond", with(pm, [](RenderParams &p) { p.in2_frame_stride = kLpMax + 8; }), 16, nullptr,
         Family::Refused, 0, STATE);
  // ramps: fast_shape_ok's rules
  expect("  three aligned ramps: fused", with(pm, [](RenderParams &p) {
           p.elem_ramp = kRamp, p.elem2_ramp = kRamp + 8192, p.out_ramp = kRamp + 16384;
           p.ramp_stream_stride = 4096;
         }), 16, nullptr, Family::LpcmMix, 2);
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
