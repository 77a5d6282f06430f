// Host-only check of the planar ragged form: its routing (pick_route() in iac_amd/csrc/render_route.hpp, Family::FastRagged,
// reached through the host-only field RenderParams::ragged).  One row per rule of ragged_shape_ok, with one field changed
// and nothing else: the form's kernel on the near side, the family iamf_hip_batch_render_range gets (the same RenderParams
// with ragged == 0) on the far side.  render_fast_kernel<.., IL = false, RAG = true> reads a lane's four samples as one
// 16-byte load per channel at 32-bit offsets and trusts the host that a quad which starts inside a call ends inside its row:
// a wrong row here is a misaligned or stray load on the GPU, not a slower rate.
// Driven by tests/test_route_host_ragged.py.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/iamf_hip.h"

namespace {
#include "../../iac_amd/csrc/render_params.hpp"
#include "../../iac_amd/csrc/render_route.hpp"
#include "route_sets.hpp"

int g_failed = 0, g_cases = 0;

void row(const char *what, bool ok) {
  printf("%-110s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kRamp = reinterpret_cast<float *>(0x20000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);

// a live service: one frame of `total` samples per call (frame size = total rounded up to 4), m planar channels, the stream
// at position pos0
RenderParams call(int m, int out_ch, int total = 1000, int64_t pos0 = 1000, int frame_size = 0) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = frame_size ? frame_size : (total + 3) & ~3;
  p.total = total;
  p.pos0 = pos0;
  p.in = kIn;
  p.in_frame_stride = (int64_t)m * p.frame_size;
  p.in_stream_stride = p.in_frame_stride * (total / p.frame_size + 1);
  p.pcm = kPcm;
  p.out_ch = p.og_ch = out_ch;
  p.out_format = IAMF_HIP_FMT_S16;
  p.pcm_stream_stride = (((int64_t)total * out_ch * 4) + 15) & ~(int64_t)15;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 48;
  p.n_end = 9649;
  p.ragged = 1;
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
bool same_route(const Route &a, const Route &b) { return a.family == b.family && a.variant == b.variant && a.err == b.err; }

// the sets that list a key, as a bit mask
int sets_of(const RouteKey &k) {
  int mask = 0;
  for (int s = 0; s < kRouteSets; ++s)
    for_each_instance_of_set(s, [&](int f, int v, int km, int kc, int kk) { mask |= same_key(k, f, v, km, kc, kk) ? 1 << s : 0; });
  return mask;
}

// fused: the form's family, a row of set 6 and of no other set.  Else: exactly what the same call gets with the flag at 0 —
// the family of iamf_hip_batch_render_range —, which must be `fallback` (what the parent commit gives the call).
void expect(const char *what, const RenderParams &p, int m, const char *env, bool fused, Family fallback = Family::Generic) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  RenderParams q = p;
  q.ragged = 0;
  const Route r0 = pick_route(q, m);
  if (env) unsetenv(env);
  bool ok = r0.family == fallback;
  if (fused) {
    const RouteKey k = route_key(r, p, m);
    ok = ok && r.family == Family::FastRagged && r.variant == 0 && r.err == IAMF_HIP_OK && k.set == 6 && sets_of(k) == 1 << 6 &&
         k.family == IAMF_HIP_ROUTE_FAST_RAGGED && k.variant == 0 && k.m == m && k.c == p.out_ch && k.k == 0;
  } else {
    ok = ok && same_route(r, r0);
  }
  row(what, ok);
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED"};
  for (const char *e : switches) unsetenv(e);
  char what[200];

  // ---- the number, the block ----
  static_assert(IAMF_HIP_ROUTE_FAST_RAGGED == 29, "stable number");
  static_assert(IAMF_HIP_ROUTE_FAST_INTERLEAVED == 27 && IAMF_HIP_ROUTE_LPCM_MIX == 25 && IAMF_HIP_ROUTE_RS_DIRECT == 23,
                "the numbers in use keep their values");
  static_assert(sizeof(RenderParams) == 616, "the block keeps its size");
  static_assert(offsetof(RenderParams, lfe_k0) == 408 && offsetof(RenderParams, ragged) == 412 && offsetof(RenderParams, lfe_div) == 416,
                "the flag lies in what was padding in front of the double");
  static_assert(offsetof(RenderParams, interleaved) == 380 && offsetof(RenderParams, dump) == 384 && offsetof(RenderParams, lfe_mask) == 424 &&
                    offsetof(RenderParams, lpcm) == 528 && offsetof(RenderParams, lpcm_off) == 552,
                "every other field keeps its offset");
  static_assert(sizeof(RenderMixParams) == 616 + 8 + 16 + 16, "the mixing block behind it too");
  static_assert((int)Family::FastRagged == (int)Family::FastInterleaved + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 6 + 1 && kRouteTables == 3, "set 6 behind the three tables; sets added later leave it alone");

  // ---- every instance ----
  int rows = 0;
  for_each_render_instance_ragged([&](int f, int v, int m, int oc, int k) {
    rows += (f == IAMF_HIP_ROUTE_FAST_RAGGED && v == 0 && RaggedM::has(m) && RaggedOC::has(oc) && k == 0) ? 1 : 1000;
    snprintf(what, sizeof(what), "%d channel(s) into %d, one frame of 1000: FastRagged", m, oc);
    expect(what, call(m, oc), m, nullptr, true);
  });
  row("the family's listing: {1, 2, 4, 6, 8, 9, 10, 12, 16} x {1, 2} = 18 rows of family 29", rows == 18);
  row("RaggedM is LpcmM and LpcmCoupledM together", [] {
    for (int m = 0; m <= 32; ++m)
      if (RaggedM::has(m) != (LpcmM::has(m) || LpcmCoupledM::has(m))) return false;
    return true;
  }());
  {
    // every key of set 6 is in that set only, and route_key names it
    bool only6 = true;
    int n6 = 0;
    for_each_instance_of_set(6, [&](int f, int v, int m, int c, int k) {
      ++n6;
      only6 = only6 && sets_of(RouteKey{f, v, m, c, k}) == 1 << 6;
      const RenderParams p = call(m, c);
      const RouteKey rk = route_key(pick_route(p, m), p, m);
      only6 = only6 && rk.set == 6 && same_key(rk, f, v, m, c, k);
    });
    row("every key of set 6 is in that set only, and route_key() names set 6 for it", only6 && n6 == 18);
    row("set 6 is the listing: 18 rows, family 29 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_FAST_RAGGED, 6, 18));
    row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
    row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  }
  row("ragged_fused: every size up to 65536", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (!ragged_fused(n)) return false;
    return true;
  }());

  // ---- lengths ----
  const int ragged[] = {1, 3, 63, 65, 100, 120, 480, 1000, 1023, 1025, 5000};
  for (int total : ragged) {
    snprintf(what, sizeof(what), "  %d samples in one frame: fused", total);
    expect(what, call(16, 2, total, 1000, total > 1024 ? (total + 3) & ~3 : 2048), 16, nullptr, true);
  }
  expect("  3 frames of 100 (a chunk spans frames): fused", call(9, 2, 300, 300, 100), 9, nullptr, true);
  expect("  5 frames of 1000: fused", call(6, 2, 5000, 5000, 1000), 6, nullptr, true);
  const int whole[] = {64, 128, 1024, 4096};
  for (int total : whole) {
    snprintf(what, sizeof(what), "  %d samples, whole blocks, the flag set: Fast, as with the flag at 0", total);
    expect(what, call(16, 2, total, 1024), 16, nullptr, false, Family::Fast);
  }
  expect("  8 frames of 1000 = 125 blocks: Fast", call(4, 2, 8000, 8000, 1000), 4, nullptr, false, Family::Fast);
  expect("  0 samples", call(2, 2, 0, 1000, 1024), 2, nullptr, false, Family::Fast);

  // ---- positions ----
  const struct {
    int64_t pos;
    bool fused;
  } positions[] = {{0, true}, {16, true}, {100, false}, {239, false}, {240, true}, {241, true}, {1100, true}, {((int64_t)1 << 31) + 1, true}};
  for (const auto &c : positions) {
    snprintf(what, sizeof(what), "  position %lld: %s", (long long)c.pos, c.fused ? "fused" : "the general kernel");
    expect(what, call(2, 2, 1000, c.pos), 2, nullptr, c.fused);
  }

  // ---- one field changed at a time ----
  const RenderParams ps = call(16, 2);
  expect("  ragged = 0: as iamf_hip_batch_render_range", with(ps, [](RenderParams &p) { p.ragged = 0; }), 16, nullptr, false);
  expect("  limiter off (1000 = 4 * 250: the kernel without limiter)", with(ps, [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, false,
         Family::Nolim);
  expect("  limiter off, 1001 samples", with(call(16, 2, 1001), [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, false);
  expect("  3 output channels", call(16, 3), 16, nullptr, false);
  expect("  6 output channels", call(16, 6), 16, nullptr, false);
  expect("  M = 14", call(14, 2), 14, nullptr, false);
  expect("  M = 24", call(24, 2), 24, nullptr, false);
  expect("  M = 11", call(11, 2), 11, nullptr, false);
  expect("  output gain on fewer channels than rendered", with(ps, [](RenderParams &p) { p.og_ch = 1; }), 16, nullptr, false);
  expect("  a limiter table shorter than the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin - 1; }), 16, nullptr, false);
  expect("  a limiter table of exactly the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin; }), 16, nullptr, true);
  expect("  a second element", with(ps, [](RenderParams &p) { p.in2 = kIn + 65536, p.m2 = 2, p.in2_frame_stride = 2000, p.in2_stream_stride = 4000; }),
         16, nullptr, false);
  expect("  an element ramp", with(ps, [](RenderParams &p) { p.elem_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16, nullptr, false);
  expect("  a ramp for a second element (no second element given)", with(ps, [](RenderParams &p) { p.elem2_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16,
         nullptr, false);
  expect("  an output ramp", with(ps, [](RenderParams &p) { p.out_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16, nullptr, false);
  expect("  down-mixer", with(call(8, 2), [](RenderParams &p) { p.dmx_on = 1; }), 8, nullptr, false);
  expect("  demixer", with(ps, [](RenderParams &p) { p.demix_on = 1; }), 16, nullptr, false);
  expect("  de-mapping matrix", with(ps, [](RenderParams &p) { p.pre_matrix = kIn; }), 16, nullptr, false);
  expect("  HRTF stage: refused as before", with(ps, [](RenderParams &p) { p.fir_taps = 256; }), 16, nullptr, false, Family::Refused);
  expect("  LFE generator", with(ps, [](RenderParams &p) { p.lfe = kIn; }), 16, nullptr, false);
  expect("  LPCM packets: refused as before", with(ps, [](RenderParams &p) { p.lpcm = reinterpret_cast<const uint8_t *>(kIn); }), 16, nullptr, false,
         Family::Refused);
  expect("  flush (no input)", with(ps, [](RenderParams &p) { p.in = nullptr; }), 16, nullptr, false);
  expect("  frame size 1002 (1001 samples)", call(16, 2, 1001, 1000, 1002), 16, nullptr, false);
  expect("  frame size 1001 (1001 samples)", call(16, 2, 1001, 1000, 1001), 16, nullptr, false);
  expect("  frame size 1004 (1001 samples)", call(16, 2, 1001, 1000, 1004), 16, nullptr, true);
  expect("  input base + 4 B", with(ps, [](RenderParams &p) { p.in += 1; }), 16, nullptr, false);
  expect("  input base + 8 B", with(ps, [](RenderParams &p) { p.in += 2; }), 16, nullptr, false);
  expect("  input base + 16 B", with(ps, [](RenderParams &p) { p.in += 4; }), 16, nullptr, true);
  expect("  stream stride 2 floats off the 16-byte grid", with(ps, [](RenderParams &p) { p.in_stream_stride += 2; }), 16, nullptr, false);
  expect("  stream stride + 4 floats", with(ps, [](RenderParams &p) { p.in_stream_stride += 4; }), 16, nullptr, true);
  expect("  frame stride 1 float off the 16-byte grid", with(ps, [](RenderParams &p) { p.in_frame_stride += 1; }), 16, nullptr, false);
  expect("  frame stride + 4 floats", with(ps, [](RenderParams &p) { p.in_frame_stride += 4; }), 16, nullptr, true);
  expect("  pcm + 2 B", with(ps, [](RenderParams &p) { p.pcm += 2; }), 16, nullptr, false);
  expect("  pcm + 16 B", with(ps, [](RenderParams &p) { p.pcm += 16; }), 16, nullptr, true);
  expect("  pcm stream stride + 4 B", with(ps, [](RenderParams &p) { p.pcm_stream_stride += 4; }), 16, nullptr, false);
  expect("  pcm stream stride + 16 B", with(ps, [](RenderParams &p) { p.pcm_stream_stride += 16; }), 16, nullptr, true);
  for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_S32, IAMF_HIP_FMT_F32}) {
    snprintf(what, sizeof(what), "  PCM format %d: fused", fmt);
    expect(what, with(ps, [&](RenderParams &p) { p.out_format = fmt; }), 16, nullptr, true);
  }
  {
    // fast_shape_ok's 32-bit bound: (total / frame_size + 2) * in_frame_stride * 4 + 100 * frame_size < 2^31, here 3 frames'
    // worth for one frame of 1000
    const int64_t lim = (((int64_t)1 << 31) - 100 * 1000) / 12;
    const int64_t at = (lim - 1) & ~(int64_t)3;
    const int64_t beyond = (lim + 4) & ~(int64_t)3;
    const auto ok = [](int64_t fst) { return 3 * fst * 4 + 100 * 1000 < ((int64_t)1 << 31); };
    row("  the 32-bit bound's two test strides lie either side of it", ok(at) && !ok(beyond) && beyond - at <= 8);
    expect("  frame stride at the 32-bit bound", with(ps, [&](RenderParams &p) { p.in_frame_stride = at; }), 16, nullptr, true);
    expect("  frame stride beyond the 32-bit bound", with(ps, [&](RenderParams &p) { p.in_frame_stride = beyond; }), 16, nullptr, false);
  }
  expect("  n_launch = 65536", with(ps, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16, nullptr, true);
  expect("  IAMF_HIP_FORCE_GENERIC", ps, 16, "IAMF_HIP_FORCE_GENERIC", false);
  expect("  IAMF_HIP_RAGGED_UNFUSED", ps, 16, "IAMF_HIP_RAGGED_UNFUSED", false);
  expect("  IAMF_HIP_INTERLEAVED_UNFUSED does not reach the form", ps, 16, "IAMF_HIP_INTERLEAVED_UNFUSED", true);
  expect("  both flags set on a frame_size == 1 batch: the interleaved rule is asked first, and refuses a planar call",
         with(ps, [](RenderParams &p) { p.interleaved = 1; }), 16, nullptr, true);

  // ---- the flag at 0 changes nothing: aligned and ragged planar calls, with and without the switch ----
  for (int total : {4096, 1000}) {
    RenderParams p = call(2, 2, total, 0, total == 4096 ? 1024 : 1000);
    p.ragged = 0;
    const Route a = pick_route(p, 2);
    setenv("IAMF_HIP_RAGGED_UNFUSED", "1", 1);
    const Route b = pick_route(p, 2);
    unsetenv("IAMF_HIP_RAGGED_UNFUSED");
    snprintf(what, sizeof(what), "ragged = 0, planar stereo, %d samples: %s, whatever the switch says", total, total == 4096 ? "Fast" : "Generic");
    row(what, a.family == (total == 4096 ? Family::Fast : Family::Generic) && same_route(a, b));
  }

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
