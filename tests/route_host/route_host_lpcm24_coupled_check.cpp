// Host-only check of the coupled 24-bit LPCM form: the packet-form rule (iac_amd/csrc/lpcm_form.hpp, LpcmForm::S24C,
// lpcm_form_coupled24() and the wrapper lpcm_form_packets() that iamf_hip_batch_render_packets asks) and its routing
// (pick_route() in iac_amd/csrc/render_route.hpp, Family::Lpcm24Coupled).  One row per rule, each a well-formed call with
// exactly one thing changed.  The two 12-byte loads of render_fast_kernel<.., LP, EARLY, 3, LPC> read a PAIR of channels from
// one run on the dword grid, and the form rule is all that stands between a legal call and a kernel that reads the wrong
// bytes as the partner or a misaligned dword: a wrong row here is wrong PCM on the GPU, not a slower rate.  lpcm_form()
// itself keeps every answer: each canonical layout is asked of it as well.
// Driven by tests/test_route_host_lpcm24_coupled.py.
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
  printf("%-96s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
constexpr uintptr_t kRaw = 0x50000;
constexpr int kFs = 1024;

// the aligned call of route_host_lpcm_coupled_check.cpp with element 0 as packets of `bytes`-byte samples
RenderParams call(int m, int out_ch, int coupled, int bytes = 3) {
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
  p.lpcm_frame_stride = 16 * kFs * 4;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
  p.lpcm_bytes = bytes;
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
  bool listed = true;   // a route of the form names a row of the family's listing, its set, and no row of any other set
  if (r.family == Family::Lpcm24Coupled) {
    const RouteKey k = route_key(r, p, m);
    listed = false;
    for_each_render_instance_lpcm24_coupled([&](int f, int v, int km, int kc, int kk) { listed = listed || same_key(k, f, v, km, kc, kk); });
    listed = listed && k.set == 7 && k.set >= kRouteTables && sets_of_key(k.family, k.variant, k.m, k.c, k.k) == 1 << 7;
  }
  row(what, r.family == family && r.variant == variant && r.err == err && listed);
}

// The packets of a loudspeaker layout of ch channels in playback order, `bytes`-byte samples: pair (0,1) first, then (from
// six channels on) C and LFE as mono runs, then the pairs (4,5) ..; run after run from `head`.  coupled = false: every
// channel a mono run of its own (the mono-coded element).
iamf_hip_lpcm_layout layout(int ch, bool coupled = true, int bytes = 3, int head = 0) {
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
LpcmForm packets(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw) {
  return lpcm_form_packets(L, ch, ss, fst, raw, first);
}
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
  const LpcmForm None = LpcmForm::None, S24C = LpcmForm::S24C;
  char what[160];

  static_assert(IAMF_HIP_ROUTE_LPCM24_COUPLED == 31, "stable number");
  static_assert((int)Family::Lpcm24Coupled == (int)Family::FastRagged + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 7 + 1 && kRouteTables == 3, "set 7 behind the three tables; sets added later leave it alone");
  static_assert((int)LpcmForm::S24C == (int)LpcmForm::S16C + 1, "appended to the enum");
  static_assert(sizeof(RenderParams) == 616, "the block keeps its size");

  // ---- the form rule: each M ----
  for_each_int(LpcmCoupledM{}, [&](int m) {
    snprintf(what, sizeof(what), "24-bit LE, %d channels, every pair coupled: S24C through the wrapper, None from lpcm_form()", m);
    row(what, packets(layout(m), m) == S24C && form(layout(m), m) == None && lpcm_form_coupled24(layout(m), m, 0));
    snprintf(what, sizeof(what), "  %d channels, head 4: runs only dword-aligned", m);
    row(what, packets(layout(m, true, 3, 4), m) == S24C && form(layout(m, true, 3, 4), m) == None);
  });
  row("  bytes of the forms: 0 / 2 / 3 / 2 / 3", lpcm_form_bytes(LpcmForm::None) == 0 && lpcm_form_bytes(LpcmForm::S16) == 2 &&
                                                     lpcm_form_bytes(LpcmForm::S24) == 3 && lpcm_form_bytes(LpcmForm::S16C) == 2 &&
                                                     lpcm_form_bytes(LpcmForm::S24C) == 3);
  const int not_coupled[] = {4, 14, 16};
  for (int m : not_coupled) {
    snprintf(what, sizeof(what), "  %d channels with (0,1) coupled: no layout of the form", m);
    const iamf_hip_lpcm_layout L = with_l(layout(m, false), [](iamf_hip_lpcm_layout &l) { l.src_step[0] = l.src_step[1] = 6; l.src_offset[1] = l.src_offset[0] + 3; });
    row(what, packets(L, m) == None && !lpcm_form_coupled24(L, m, 0));
  }

  // ---- one thing changed at a time ----
  const iamf_hip_lpcm_layout L6 = layout(6), L2 = layout(2), L12 = layout(12);
  row("stereo: first_sample = 2 (12 bytes of a pair)", packets(L2, 2, 2) == S24C);
  row("stereo: first_sample = 6", packets(L2, 2, 6) == S24C);
  row("stereo: first_sample = 1 (6 bytes: off the dword grid)", packets(L2, 2, 1) == None);
  row("stereo: first_sample = 3", packets(L2, 2, 3) == None);
  row("stereo: the pair at offset 2 mod 4", packets(layout(2, true, 3, 2), 2) == None);
  row("  ... with first_sample = 1: 2 + 6 on the grid", packets(layout(2, true, 3, 2), 2, 1) == S24C);
  row("5.1: first_sample = 2: the pairs on the grid, C and LFE 2 bytes off it", packets(L6, 6, 2) == None);
  row("5.1: first_sample = 4", packets(L6, 6, 4) == S24C);
  row("5.1: first_sample = 1", packets(L6, 6, 1) == None);
  row("5.1: first_sample = 6", packets(L6, 6, 6) == None);
  row("7.1.4: first_sample = 8", packets(L12, 12, 8) == S24C);
  row("5.1: pair (4,5) with step 12", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_step[4] = L.src_step[5] = 12; }), 6) == None);
  row("5.1: one half of a pair with step 3", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_step[5] = 3; }), 6) == None);
  row("stereo: step 4 (16-bit pairs' step)", packets(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_step[0] = L.src_step[1] = 4; }), 2) == None);
  row("stereo: the partner at +6 instead of +3", packets(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_offset[1] = L.src_offset[0] + 6; }), 2) == None);
  row("stereo: the partner at +2", packets(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_offset[1] = L.src_offset[0] + 2; }), 2) == None);
  row("stereo: the partner in front (R L)", packets(with_l(L2, [](iamf_hip_lpcm_layout &L) { L.src_offset[0] = 3; L.src_offset[1] = 0; }), 2) == None);
  row("7.1.4: the last pair's partner at +6", packets(with_l(L12, [](iamf_hip_lpcm_layout &L) { L.src_offset[11] += 3; }), 12) == None);
  row("5.1: step 6 with the partner elsewhere (another run)", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[5] = L.src_offset[0] + 3; }), 6) == None);
  row("5.1: pair (4,5) at offset 2 mod 4", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[4] += 2; L.src_offset[5] += 2; }), 6) == None);
  row("5.1: C at step 6", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_step[2] = 6; }), 6) == None);
  row("5.1: LFE at offset 2 mod 4", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[3] += 2; }), 6) == None);
  row("5.1: a pair on (2,3) as well (C and LFE coupled)", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) {
        L.src_step[2] = L.src_step[3] = 6;
        L.src_offset[3] = L.src_offset[2] + 3;
      }), 6) == None);
  {
    const iamf_hip_lpcm_layout L = with_l(layout(6, false), [](iamf_hip_lpcm_layout &l) {
      l.src_step[1] = l.src_step[2] = 6;
      l.src_offset[2] = l.src_offset[1] + 3;
    });
    row("5.1: a pair on (1,2), 0 mono", packets(L, 6) == None && !lpcm_form_coupled24(L, 6, 0));
  }
  row("5.1 as six mono runs: not the coupled form (lpcm_form()'s answer, which no kernel of six inputs takes)",
      !lpcm_form_coupled24(layout(6, false), 6, 0) && packets(layout(6, false), 6) == form(layout(6, false), 6) &&
          packets(layout(6, false), 6) != S24C && !LpcmM::has(6));
  row("5.1: (0,1) coupled, (4,5) two mono runs", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) {
        L.src_step[4] = L.src_step[5] = 3;
        L.src_offset[5] = L.src_offset[4] + 3 * kFs;
      }), 6) == None);
  row("raw_frame_stride 2 mod 4", packets(L6, 6, 0, 4 * kRow, kRow + 2) == None);
  row("raw_stream_stride 2 mod 4", packets(L6, 6, 0, 4 * kRow + 2, kRow) == None);
  row("raw_frame_stride 4 mod 8: the dword grid is enough", packets(L6, 6, 0, 4 * kRow, kRow + 4) == S24C);
  row("d_raw + 8 B (16-byte alignment)", packets(L6, 6, 0, 4 * kRow, kRow, kRaw + 8) == None);
  row("d_raw + 4 B", packets(L2, 2, 0, 4 * kRow, kRow, kRaw + 4) == None);
  row("big-endian", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.little_endian = 0; }), 6) == None);
  row("a missing channel: the first of a pair", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[4] = -1; }), 6) == None);
  row("a missing channel: the second of a pair", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[1] = -1; }), 6) == None);
  row("a missing channel: LFE", packets(with_l(L6, [](iamf_hip_lpcm_layout &L) { L.src_offset[3] = -1; }), 6) == None);
  row("32-bit coupled stereo", packets(layout(2, true, 4), 2) == None);
  row("32-bit coupled 5.1", packets(layout(6, true, 4), 6) == None);

  // ---- the 16-bit and the mono-coded 24-bit rows keep their answers through the wrapper ----
  for_each_int(LpcmCoupledM{}, [&](int m) {
    snprintf(what, sizeof(what), "16-bit coupled, %d channels: S16C from both", m);
    row(what, packets(layout(m, true, 2), m) == LpcmForm::S16C && form(layout(m, true, 2), m) == LpcmForm::S16C);
  });
  row("16-bit coupled stereo, first_sample = 1: None from both", packets(layout(2, true, 2), 2, 1) == None && form(layout(2, true, 2), 2, 1) == None);
  row("16 mono 16-bit runs: S16 from both", packets(layout(16, false, 2), 16) == LpcmForm::S16 && form(layout(16, false, 2), 16) == LpcmForm::S16);
  row("16 mono 24-bit runs: S24 from both", packets(layout(16, false, 3), 16) == LpcmForm::S24 && form(layout(16, false, 3), 16) == LpcmForm::S24);
  row("4 mono 24-bit runs, first_sample = 1: None from both", packets(layout(4, false, 3), 4, 1) == None && form(layout(4, false, 3), 4, 1) == None);
  row("one mono 24-bit run: S24 from both", packets(layout(1, false, 3), 1) == LpcmForm::S24 && form(layout(1, false, 3), 1) == LpcmForm::S24);
  row("24 bit, src_step == 6 on (0,1) of 16: None from both", [&] {
    const iamf_hip_lpcm_layout L = with_l(layout(16, false, 3), [](iamf_hip_lpcm_layout &l) {
      l.src_step[0] = l.src_step[1] = 6;
      l.src_offset[1] = 3;
    });
    return packets(L, 16) == None && form(L, 16) == None;
  }());

  // ---- routing ----
  for_each_int(LpcmCoupledM{}, [&](int m) {
    for_each_int(LpcmOC{}, [&](int oc) {
      snprintf(what, sizeof(what), "coupled 24-bit packets, m = %d into %d channel(s): Lpcm24Coupled, what lpcm24_coupled_early says", m, oc);
      expect(what, call(m, oc, 2), m, nullptr, Family::Lpcm24Coupled, lpcm24_coupled_early(64));
      snprintf(what, sizeof(what), "  m = %d into %d: IAMF_HIP_LP_LATE", m, oc);
      expect(what, call(m, oc, 2), m, "IAMF_HIP_LP_LATE", Family::Lpcm24Coupled, 0);
      snprintf(what, sizeof(what), "  m = %d into %d: IAMF_HIP_LP_EARLY", m, oc);
      expect(what, call(m, oc, 2), m, "IAMF_HIP_LP_EARLY", Family::Lpcm24Coupled, 1);
    });
  });
  int rows = 0;
  for_each_render_instance_lpcm24_coupled([&](int f, int v, int m, int oc, int k) {
    rows += (f == IAMF_HIP_ROUTE_LPCM24_COUPLED && (v == 0 || v == 1) && LpcmCoupledM::has(m) && LpcmOC::has(oc) && k == 0) ? 1 : 1000;
  });
  row("the family's listing: LpcmCoupledM x LpcmOC x {late, early} = 20 rows of family 31", rows == 20);
  row("set 7 of for_each_instance_of_set is the listing: 20 rows, family 31 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_LPCM24_COUPLED, 7, 20));
  row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
  row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  expect("  lpcm_coupled = 2 with 16-bit samples: refused", call(6, 2, 2, 2), 6, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 2 with lpcm_bytes = 0 (16 bit): refused", call(6, 2, 2, 0), 6, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 2 with 32-bit samples: refused", call(2, 2, 2, 4), 2, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 1 with 24-bit samples: still refused", call(6, 2, 1, 3), 6, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 1 with 16-bit samples: LpcmCoupled as before", call(6, 2, 1, 2), 6, nullptr, Family::LpcmCoupled, 1);
  expect("  lpcm_coupled = 0 with 24-bit samples, m = 6: refused as before", call(6, 2, 0, 3), 6, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_coupled = 0 with 24-bit samples, m = 4: Lpcm24 as before", call(4, 2, 0, 3), 4, nullptr, Family::Lpcm24, 1);
  expect("  m = 4: refused", call(4, 2, 2), 4, nullptr, Family::Refused, 0, STATE);
  expect("  m = 16: refused", call(16, 2, 2), 16, nullptr, Family::Refused, 0, STATE);
  expect("  m = 1: refused", call(1, 2, 2), 1, nullptr, Family::Refused, 0, STATE);
  expect("  lpcm_mix set: the two-element form has no 24-bit instance", with(call(6, 2, 2), [](RenderParams &p) { p.lpcm_mix = 1; p.in2 = kIn; p.m2 = 1; }), 6,
         nullptr, Family::Refused, 0, STATE);

  // ---- the prefetch variant by the launch's size, and the switches ----
  const RenderParams pc = call(12, 2, 2);
  int cut = 0;   // the largest launch lpcm24_coupled_early() still gives the early variant; one cut or one variant
  for (int n = 1; n <= 65536; ++n)
    if (lpcm24_coupled_early(n)) cut = n;
  row("lpcm24_coupled_early: one cut (early up to it, late beyond) or one variant for every size", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (lpcm24_coupled_early(n) != (n <= cut)) return false;
    return true;
  }());
  expect("  n_launch = 1: what lpcm24_coupled_early(1) says", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 1; }), 12, nullptr,
         Family::Lpcm24Coupled, lpcm24_coupled_early(1));
  expect("  n_launch = 65536: what lpcm24_coupled_early(65536) says", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 12,
         nullptr, Family::Lpcm24Coupled, lpcm24_coupled_early(65536));
  if (cut > 0 && cut < 65536) {
    expect("  n_launch at the cut: early", with(pc, [&](RenderParams &p) { p.n_launch = p.n_streams = cut; }), 12, nullptr, Family::Lpcm24Coupled, 1);
    expect("  n_launch one beyond the cut: late", with(pc, [&](RenderParams &p) { p.n_launch = p.n_streams = cut + 1; }), 12, nullptr,
           Family::Lpcm24Coupled, 0);
  }
  expect("  IAMF_HIP_LP_EARLY at 65536 workgroups", with(pc, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 12,
         "IAMF_HIP_LP_EARLY", Family::Lpcm24Coupled, 1);
  setenv("IAMF_HIP_LP_EARLY", "1", 1);
  expect("  both switches: late", pc, 12, "IAMF_HIP_LP_LATE", Family::Lpcm24Coupled, 0);
  unsetenv("IAMF_HIP_LP_EARLY");

  // ---- each refusal of Family::Lpcm24 holds for Family::Lpcm24Coupled ----
  expect("  3 output channels: no instance", call(6, 3, 2), 6, nullptr, Family::Refused, 0, STATE);
  expect("  6 output channels: no instance", call(12, 6, 2), 12, nullptr, Family::Refused, 0, STATE);
  expect("  limiter off", with(pc, [](RenderParams &p) { p.limiter_on = 0; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(pc, [](RenderParams &p) { p.pos0 = 8; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 16", with(pc, [](RenderParams &p) { p.pos0 = 16; }), 12, nullptr, Family::Lpcm24Coupled, lpcm24_coupled_early(64));
  expect("  n_end = kFWin - 1: a table that ends inside the staged window", with(pc, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; }), 12,
         nullptr, Family::Refused, 0, STATE);
  expect("  n_end = kFWin", with(pc, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; }), 12, nullptr, Family::Lpcm24Coupled, lpcm24_coupled_early(64));
  expect("  pos0 = 250: off the 16-sample grid, past the look-ahead", with(pc, [](RenderParams &p) { p.pos0 = 250; }), 12, nullptr,
         Family::Lpcm24Coupled, lpcm24_coupled_early(64));
  expect("  pos0 = 239", with(pc, [](RenderParams &p) { p.pos0 = 239; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  total % 64 != 0", with(pc, [](RenderParams &p) { p.total = 4096 + 32; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  down-mixer", with(call(6, 2, 2), [](RenderParams &p) { p.dmx_on = 1; }), 6, nullptr, Family::Refused, 0, STATE);
  expect("  an output ramp off the 16-byte grid", with(pc, [](RenderParams &p) { p.out_ramp = kIn + 1; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  IAMF_HIP_FORCE_GENERIC", pc, 12, "IAMF_HIP_FORCE_GENERIC", Family::Refused, 0, STATE);
  expect("  pcm + 2 B", with(pc, [](RenderParams &p) { p.pcm += 2; }), 12, nullptr, Family::Refused, 0, STATE);
  expect("  out_gain_channels below the output's", with(pc, [](RenderParams &p) { p.og_ch = 1; }), 12, nullptr, Family::Refused, 0, STATE);
  // the 32-bit bound of the packet offsets, as for Family::Lpcm24 (fast_shape_ok): (total / fs + 2) * stride + 2^24 < 2^31
  constexpr int64_t kLpMax = 355117736;
  static_assert((4096 / kFs + 2) * kLpMax + ((int64_t)1 << 24) < ((int64_t)1 << 31) && (4096 / kFs + 2) * (kLpMax + 4) + ((int64_t)1 << 24) >= ((int64_t)1 << 31),
                "the last stride on the dword grid inside the bound");
  expect("  lpcm_frame_stride at the 32-bit bound", with(pc, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 12, nullptr,
         Family::Lpcm24Coupled, lpcm24_coupled_early(64));
  expect("  lpcm_frame_stride 4 bytes beyond", with(pc, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 4; }), 12, nullptr,
         Family::Refused, 0, STATE);
  expect("  the same two strides for Family::Lpcm24: taken", with(call(16, 2, 0, 3), [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 16, nullptr,
         Family::Lpcm24, 1);
  expect("  ... and refused", with(call(16, 2, 0, 3), [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 4; }), 16, nullptr, Family::Refused, 0, STATE);

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
