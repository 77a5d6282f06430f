// Host-only check of the 24-bit LPCM form: the packet-form rule (iac_amd/csrc/lpcm_form.hpp) and its routing
// (pick_route() in iac_amd/csrc/render_route.hpp, Family::Lpcm24).  One row per rule, each a well-formed call with exactly
// one thing changed.  The 12-byte loads of render_fast_kernel<.., LPB = 3> need dword alignment, and the form rule is all
// that stands between a legal call and a misaligned load: a wrong row here is a fault on the GPU, not a slower rate.
// Driven by tests/test_route_host_lpcm24.py.
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
  printf("%-84s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
constexpr uintptr_t kRaw = 0x50000;

// the aligned stereo call of route_host_check.cpp with element 0 as packets of `bytes`-byte samples
RenderParams call(int m, int out_ch, int bytes) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = 1024;
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
  p.lpcm_frame_stride = 16 * 1024 * 3;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
  p.lpcm_bytes = bytes;
  return p;
}
template <class F>
RenderParams with(RenderParams p, F f) {
  f(p);
  return p;
}
void expect(const char *what, const RenderParams &p, int m, const char *env, Family family, int variant, int err = IAMF_HIP_OK) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  if (env) unsetenv(env);
  bool listed = r.family != Family::Lpcm24;   // an Lpcm24 route names a row of table 2 and no row of the other tables
  const RouteKey k = route_key(r, p, m);
  if (r.family == Family::Lpcm24) {
    const auto same = [&](int f, int v, int km, int kc, int kk) {
      return f == k.family && v == k.variant && km == k.m && kc == k.c && kk == k.k;
    };
    for_each_render_instance_lpcm24([&](int f, int v, int km, int kc, int kk) { listed = listed || same(f, v, km, kc, kk); });
    for_each_render_instance([&](int f, int v, int km, int kc, int kk) { listed = listed && !same(f, v, km, kc, kk); });
    for_each_render_instance_ext([&](int f, int v, int km, int kc, int kk) { listed = listed && !same(f, v, km, kc, kk); });
  }
  row(what, r.family == family && r.variant == variant && r.err == err && listed);
}

// 24-bit little-endian packets of ch mono sub-streams, run after run from `head`, `pad` bytes between runs
iamf_hip_lpcm_layout layout(int ch, int bytes, int head = 0, int pad = 0) {
  iamf_hip_lpcm_layout L;
  memset(&L, 0, sizeof(L));
  L.sample_bytes = bytes;
  L.little_endian = 1;
  L.channels = ch;
  L.frame_size = 1024;
  for (int c = 0; c < ch; ++c) {
    L.src_offset[c] = head + c * (1024 * bytes + pad);
    L.src_step[c] = bytes;
  }
  return L;
}
constexpr int64_t kRow = 17 * 1024 * 4;   // a packet row that holds every layout below; a multiple of 8
LpcmForm form(const iamf_hip_lpcm_layout &L, int ch, int first = 0, int64_t ss = 4 * kRow, int64_t fst = kRow, uintptr_t raw = kRaw) {
  return lpcm_form(L, ch, ss, fst, raw, first);
}
template <class F>
iamf_hip_lpcm_layout with_l(iamf_hip_lpcm_layout L, F f) {
  f(L);
  return L;
}

// ---- the packet layouts of tests/gpu_util.py (the PK_ table there), 24-bit packets ----
// As packet_layout_rows() of route_host_check.cpp: one row per layout and call of tests/test_gpu_packet_layouts.py (3 streams,
// four 1024-sample frames, a call of 1 frame from frame 0 and one of 3 frames from frame 1), lpcm_form()'s answer and
// pick_route()'s family; a call that is not fused is unpacked into dense f32 rows for the f32 kernel.
void packet_layout_rows() {
  constexpr int kCh = 16, kF = 4, kG = 4;
  constexpr int64_t kPkRow = 49232;   // lpcm_util.rows: 16 runs of 3072 bytes, head 4, pad 4, rounded up to 16
  constexpr int64_t k31 = (int64_t)1 << 31;
  constexpr int64_t kB3 = ((k31 - (1 << 24) - 1) / 5) & ~(int64_t)15;   // B(3): (3 + 2) * B + 2^24 < 2^31
  static_assert(kB3 == 426141280 && 5 * kB3 + (1 << 24) < k31 && 5 * (kB3 + 16) + (1 << 24) >= k31 && 3 * (kB3 + 16) + (1 << 24) < k31,
                "B(3)");
  iamf_hip_lpcm_layout L = layout(kCh, 3, 4, 4);
  for (int c = 0; c < kCh / 2; ++c) {   // reversed channel order: no offset ascends
    const int32_t o = L.src_offset[c];
    L.src_offset[c] = L.src_offset[kCh - 1 - c];
    L.src_offset[kCh - 1 - c] = o;
  }
  struct Pk {
    const char *name;
    int64_t off, fst, sst;
    bool fused[2];
  };
  const Pk rows[] = {
      {"PK_DENSE", 0, kPkRow, kF * kPkRow, {true, true}},
      {"PK_PAD16", 16, kPkRow + 16, kF * (kPkRow + 16) + 48, {true, true}},
      {"PK_GRID", 16, kPkRow + kG, kF * (kPkRow + kG) + kG, {true, false}},
      {"PK_OFF_BASE", 8, kPkRow + 16, kF * (kPkRow + 16), {false, false}},
      {"PK_OFF_STRIDE", 0, kPkRow + kG / 2, kF * (kPkRow + kG / 2), {false, false}},
      {"PK_FAR_STREAMS", 16, kPkRow, k31 + 16, {true, true}},
      {"PK_BOUND", 0, kB3, kF * kB3, {true, true}},
      {"PK_BEYOND", 0, kB3 + 16, kF * (kB3 + 16), {true, false}},
  };
  const int f0s[2] = {0, 1}, nfs[2] = {1, 3};
  for (const Pk &r : rows) {
    for (int c = 0; c < 2; ++c) {
      const uintptr_t raw = kRaw + (uintptr_t)((r.off + f0s[c] * r.fst) & 15);
      const LpcmForm form = lpcm_form(L, kCh, r.sst, r.fst, raw, 0);
      RenderParams p = call(kCh, 2, lpcm_form_bytes(form));
      p.n_streams = p.n_launch = 3;
      p.pos0 = (int64_t)f0s[c] * 1024;
      p.total = nfs[c] * 1024;
      p.lpcm = reinterpret_cast<const uint8_t *>(raw);
      p.lpcm_frame_stride = r.fst;
      p.lpcm_stream_stride = r.sst;
      RenderParams q = p;   // the unpacked call: dense f32 rows of the batch's own buffer
      q.lpcm = nullptr;
      q.lpcm_frame_stride = q.lpcm_stream_stride = 0;
      q.lpcm_bytes = 0;
      q.in_frame_stride = (int64_t)kCh * 1024;
      q.in_stream_stride = nfs[c] * q.in_frame_stride;
      const Route f32 = pick_route(q, kCh);
      bool ok = f32.family == Family::Fast && f32.variant == 0 && form != LpcmForm::S16;
      ok = ok && (form == LpcmForm::S24) == (r.fused[c] || !strcmp(r.name, "PK_BEYOND"));
      for (int early = 0; early < 2; ++early) {   // under either switch, as the GPU test forces the variant
        setenv(early ? "IAMF_HIP_LP_EARLY" : "IAMF_HIP_LP_LATE", "1", 1);
        const Route rt = form == LpcmForm::None ? Route{Family::Refused, 0, IAMF_HIP_ERR_INVALID_STATE} : pick_route(p, kCh);
        unsetenv(early ? "IAMF_HIP_LP_EARLY" : "IAMF_HIP_LP_LATE");
        const bool fused = rt.family == Family::Lpcm24 && rt.variant == early;
        ok = ok && fused == r.fused[c] && (fused || rt.family == Family::Refused);
      }
      char what[128];
      snprintf(what, sizeof(what), "%s, %d frame(s) from frame %d: %s", r.name, nfs[c], f0s[c],
               r.fused[c] ? "Lpcm24, the variant asked for" : "unpack + Fast");
      row(what, ok);
    }
  }
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  const int STATE = IAMF_HIP_ERR_INVALID_STATE;
  char what[128];

  // ---- routing: every (m, oc) of the lists takes Lpcm24 ----
  static_assert(IAMF_HIP_ROUTE_LPCM24 == 16, "stable number");
  for_each_int(LpcmM{}, [&](int m) {
    for_each_int(LpcmOC{}, [&](int oc) {
      snprintf(what, sizeof(what), "24-bit packets, m = %d into %d channel(s)", m, oc);
      expect(what, call(m, oc, 3), m, nullptr, Family::Lpcm24, 1);
    });
  });
  int rows = 0;
  for_each_render_instance_lpcm24([&](int f, int v, int, int, int) { rows += (f == IAMF_HIP_ROUTE_LPCM24 && (v == 0 || v == 1)) ? 1 : 1000; });
  row("table 2: LpcmM x LpcmOC x {late, early} rows of family 16", rows == 16);

  // ---- the prefetch variant by the launch's size, and the switch ----
  const RenderParams p24 = call(16, 2, 3);
  int cut = 0;   // the largest launch lpcm24_early() still gives the early variant; the rule is monotonic or constant
  for (int n = 1; n <= 65536; ++n)
    if (lpcm24_early(n)) cut = n;
  row("lpcm24_early: one cut (early up to it, late beyond) or one variant for every size",
      [&] {
        for (int n = 1; n <= 65536; ++n)
          if (lpcm24_early(n) != (n <= cut)) return false;
        return true;
      }());
  expect("  n_launch = 1: what lpcm24_early(1) says", with(p24, [](RenderParams &p) { p.n_launch = p.n_streams = 1; }), 16, nullptr,
         Family::Lpcm24, lpcm24_early(1));
  expect("  n_launch = 65536: what lpcm24_early(65536) says", with(p24, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16,
         nullptr, Family::Lpcm24, lpcm24_early(65536));
  if (cut > 0 && cut < 65536) {
    expect("  n_launch at the cut: early", with(p24, [&](RenderParams &p) { p.n_launch = p.n_streams = cut; }), 16, nullptr, Family::Lpcm24, 1);
    expect("  n_launch one beyond the cut: late", with(p24, [&](RenderParams &p) { p.n_launch = p.n_streams = cut + 1; }), 16, nullptr,
           Family::Lpcm24, 0);
  }
  expect("  IAMF_HIP_LP_LATE", p24, 16, "IAMF_HIP_LP_LATE", Family::Lpcm24, 0);
  expect("  IAMF_HIP_LP_EARLY at 65536 workgroups", with(p24, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16,
         "IAMF_HIP_LP_EARLY", Family::Lpcm24, 1);
  setenv("IAMF_HIP_LP_EARLY", "1", 1);
  expect("  both switches: late", p24, 16, "IAMF_HIP_LP_LATE", Family::Lpcm24, 0);
  expect("  IAMF_HIP_LP_EARLY does not reach the 16-bit family", with(call(16, 2, 2), [](RenderParams &p) { p.n_launch = p.n_streams = 1025; }),
         16, nullptr, Family::Lpcm, 0);
  unsetenv("IAMF_HIP_LP_EARLY");

  // ---- each refusal of Family::Lpcm holds for Family::Lpcm24 ----
  expect("  m = 6: no instance", call(6, 2, 3), 6, nullptr, Family::Refused, 0, STATE);
  expect("  6 output channels: no instance", call(16, 6, 3), 16, nullptr, Family::Refused, 0, STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(p24, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Refused, 0, STATE);
  // the staged limiter-table window (kFWin, render_fast.hpp): (n_atk, n_end) = (6, 1087) at 5407 Hz and (6, 1088) at 5408 Hz
  expect("  n_end = kFWin - 1: a table that ends inside the staged window", with(p24, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; }), 16,
         nullptr, Family::Refused, 0, STATE);
  expect("  n_end = kFWin", with(p24, [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; }), 16, nullptr, Family::Lpcm24, 1);
  expect("  total % 64 != 0", with(p24, [](RenderParams &p) { p.total = 4096 + 32; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  limiter off", with(p24, [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, Family::Refused, 0, STATE);
  expect("  down-mixer", with(call(4, 2, 3), [](RenderParams &p) { p.dmx_on = 1; }), 4, nullptr, Family::Refused, 0, STATE);
  expect("  IAMF_HIP_FORCE_GENERIC", p24, 16, "IAMF_HIP_FORCE_GENERIC", Family::Refused, 0, STATE);
  expect("  pcm + 2 B", with(p24, [](RenderParams &p) { p.pcm += 2; }), 16, nullptr, Family::Refused, 0, STATE);
  constexpr int64_t kLpMax = 355117736;     // the 32-bit bound of the packet offsets, as for 16 bit
  expect("  lpcm_frame_stride at the 32-bit bound", with(p24, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; }), 16, nullptr,
         Family::Lpcm24, 1);
  expect("  lpcm_frame_stride 8 bytes beyond", with(p24, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 8; }), 16, nullptr,
         Family::Refused, 0, STATE);

  // ---- the 16-bit rows still decide as before: lpcm_bytes 0 (a block that never heard of the field) and 2 ----
  for (int bytes = 0; bytes <= 2; bytes += 2) {
    const RenderParams p16 = call(16, 2, bytes);
    snprintf(what, sizeof(what), "lpcm_bytes = %d: the 16-bit family, early up to 1024 workgroups", bytes);
    expect(what, with(p16, [](RenderParams &p) { p.n_launch = p.n_streams = 1024; }), 16, nullptr, Family::Lpcm, 1);
    expect("  n_launch = 1025", with(p16, [](RenderParams &p) { p.n_launch = p.n_streams = 1025; }), 16, nullptr, Family::Lpcm, 0);
    expect("  IAMF_HIP_LP_LATE", p16, 16, "IAMF_HIP_LP_LATE", Family::Lpcm, 0);
    expect("  pos0 = 8", with(p16, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Refused, 0, STATE);
  }

  // ---- the form rule, 24 bit ----
  const iamf_hip_lpcm_layout L24 = layout(16, 3);
  row("24-bit LE, 16 runs at multiples of 3072: the 24-bit form", form(L24, 16) == LpcmForm::S24);
  row("  bytes of the forms: 0 / 2 / 3", lpcm_form_bytes(LpcmForm::None) == 0 && lpcm_form_bytes(LpcmForm::S16) == 2 &&
                                            lpcm_form_bytes(LpcmForm::S24) == 3);
  row("  head 4, pad 4 (runs only 4-byte aligned)", form(layout(16, 3, 4, 4), 16) == LpcmForm::S24);
  row("  one run at offset 2 mod 4", form(with_l(L24, [](iamf_hip_lpcm_layout &L) { L.src_offset[5] += 2; }), 16) == LpcmForm::None);
  row("  every run at offset 2 mod 4", form(layout(16, 3, 2, 0), 16) == LpcmForm::None);
  row("  raw_frame_stride 2 mod 4", form(L24, 16, 0, 4 * kRow, kRow + 2) == LpcmForm::None);
  row("  raw_stream_stride 2 mod 4", form(L24, 16, 0, 4 * kRow + 2, kRow) == LpcmForm::None);
  row("  d_raw + 4 B (16-byte alignment, as for 16 bit)", form(L24, 16, 0, 4 * kRow, kRow, kRaw + 4) == LpcmForm::None);
  row("  first_sample = 64: 3 * 64 on the grid", form(L24, 16, 64) == LpcmForm::S24);
  row("  first_sample = 4: 12 bytes, on the grid", form(L24, 16, 4) == LpcmForm::S24);
  row("  first_sample = 2: 3 * first off the grid", form(L24, 16, 2) == LpcmForm::None);
  row("  first_sample = 2 with offsets 2 mod 4: the sum is on the grid", form(layout(16, 3, 2, 0), 16, 2) == LpcmForm::S24);
  row("  src_step == 6 (a coupled sub-stream)",
      form(with_l(L24, [](iamf_hip_lpcm_layout &L) { L.src_step[0] = L.src_step[1] = 6; L.src_offset[1] = 3; }), 16) == LpcmForm::None);
  row("  src_step == 6, one channel", form(with_l(L24, [](iamf_hip_lpcm_layout &L) { L.src_step[3] = 6; }), 16) == LpcmForm::None);
  row("  a missing channel", form(with_l(L24, [](iamf_hip_lpcm_layout &L) { L.src_offset[7] = -1; }), 16) == LpcmForm::None);
  row("  big-endian", form(with_l(L24, [](iamf_hip_lpcm_layout &L) { L.little_endian = 0; }), 16) == LpcmForm::None);
  row("  17 channels", form(layout(17, 3), 17) == LpcmForm::None);
  row("  32-bit samples", form(layout(16, 4), 16) == LpcmForm::None);

  // ---- the form rule, 16 bit: as it stood ----
  const iamf_hip_lpcm_layout L16 = layout(16, 2, 16, 0);
  row("16-bit LE, head 16: the 16-bit form", form(L16, 16) == LpcmForm::S16);
  row("  one run at offset 4 mod 8", form(with_l(L16, [](iamf_hip_lpcm_layout &L) { L.src_offset[2] += 4; }), 16) == LpcmForm::None);
  row("  raw_frame_stride 4 mod 8", form(L16, 16, 0, 4 * kRow, kRow + 4) == LpcmForm::None);
  row("  raw_stream_stride 4 mod 8", form(L16, 16, 0, 4 * kRow + 4, kRow) == LpcmForm::None);
  row("  d_raw + 8 B", form(L16, 16, 0, 4 * kRow, kRow, kRaw + 8) == LpcmForm::None);
  row("  first_sample = 4 (8 bytes)", form(L16, 16, 4) == LpcmForm::S16);
  row("  first_sample = 6 (12 bytes)", form(L16, 16, 6) == LpcmForm::None);
  row("  src_step == 4", form(with_l(L16, [](iamf_hip_lpcm_layout &L) { L.src_step[0] = 4; }), 16) == LpcmForm::None);
  row("  a missing channel", form(with_l(L16, [](iamf_hip_lpcm_layout &L) { L.src_offset[0] = -1; }), 16) == LpcmForm::None);
  row("  big-endian", form(with_l(L16, [](iamf_hip_lpcm_layout &L) { L.little_endian = 0; }), 16) == LpcmForm::None);

  packet_layout_rows();

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
