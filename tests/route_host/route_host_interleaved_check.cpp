// Host-only check of the interleaved f32 form: its routing (pick_route() in iac_amd/csrc/render_route.hpp,
// Family::FastInterleaved, reached through the host-only field RenderParams::interleaved).  One row per rule: the form's
// kernel on the near side, the family iamf_hip_batch_render_range gets (the same RenderParams with interleaved == 0) on the
// far side.  render_fast_kernel<.., IL, RAG> reads a lane's four sample-frames as 16-byte pieces through a buffer resource
// that ends with the call, at 32-bit offsets: a wrong row here is a misaligned load on the GPU, not a slower rate.
// Driven by tests/test_route_host_interleaved.py.
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

int g_failed = 0, g_cases = 0;

void row(const char *what, bool ok) {
  printf("%-100s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kRamp = reinterpret_cast<float *>(0x20000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);

// the stage behind the resampler: a frame_size == 1 batch, m channels dense, 1115 sample-frames at position 1115
RenderParams call(int m, int out_ch, int total = 1115, int64_t pos0 = 1115) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = 1;
  p.total = total;
  p.pos0 = pos0;
  p.in = kIn;
  p.in_frame_stride = m;
  p.in_stream_stride = ((int64_t)total * m + 3) & ~(int64_t)3;
  p.pcm = kPcm;
  p.out_ch = p.og_ch = out_ch;
  p.out_format = IAMF_HIP_FMT_S16;
  p.pcm_stream_stride = (((int64_t)total * out_ch * 4) + 15) & ~(int64_t)15;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 48;
  p.n_end = 9649;
  p.interleaved = 1;
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

// fused: the form's family, a row of its listing and of no other set.  Else: exactly what the same call gets with the flag at
// 0 — the family of iamf_hip_batch_render_range —, which must be `fallback`.
void expect(const char *what, const RenderParams &p, int m, const char *env, bool fused, Family fallback = Family::Generic) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  RenderParams q = p;
  q.interleaved = 0;
  const Route r0 = pick_route(q, m);
  if (env) unsetenv(env);
  bool ok = r0.family == fallback;
  if (fused) {
    const RouteKey k = route_key(r, p, m);
    bool listed = false;
    for_each_render_instance_interleaved([&](int f, int v, int km, int kc, int kk) { listed = listed || same_key(k, f, v, km, kc, kk); });
    for_each_render_instance([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_ext([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm24([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm_coupled([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    for_each_render_instance_lpcm_mix([&](int f, int v, int km, int kc, int kk) { listed = listed && !same_key(k, f, v, km, kc, kk); });
    ok = ok && r.family == Family::FastInterleaved && r.variant == 0 && r.err == IAMF_HIP_OK && listed &&
         k.family == IAMF_HIP_ROUTE_FAST_INTERLEAVED && k.m == m && k.c == p.out_ch && k.k == 0;
  } else {
    ok = ok && same_route(r, r0);
  }
  row(what, ok);
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_INTERLEAVED_UNFUSED"};
  for (const char *e : switches) unsetenv(e);
  char what[200];

  // ---- the number, the block ----
  static_assert(IAMF_HIP_ROUTE_FAST_INTERLEAVED == 27, "stable number");
  static_assert(IAMF_HIP_ROUTE_LPCM_MIX == 25 && IAMF_HIP_ROUTE_RS_DIRECT == 23, "the numbers in use keep their values");
  static_assert(sizeof(RenderParams) == 616, "the block keeps its size");
  static_assert(offsetof(RenderParams, demix_w4) == 376 && offsetof(RenderParams, interleaved) == 380 && offsetof(RenderParams, dump) == 384,
                "the flag lies in what was padding");
  static_assert(offsetof(RenderParams, lfe_div) == 416 && offsetof(RenderParams, lpcm) == 528 && offsetof(RenderParams, lpcm_off) == 552,
                "every field behind it keeps its offset");
  static_assert((int)Family::FastInterleaved == (int)Family::LpcmMix + 1, "added at the end of the enum");

  // ---- every instance ----
  int rows = 0;
  for_each_render_instance_interleaved([&](int f, int v, int m, int oc, int k) {
    rows += (f == IAMF_HIP_ROUTE_FAST_INTERLEAVED && v == 0 && InterleavedM::has(m) && InterleavedOC::has(oc) && k == 0) ? 1 : 1000;
    snprintf(what, sizeof(what), "%d channel(s) into %d: FastInterleaved", m, oc);
    expect(what, call(m, oc), m, nullptr, true);
  });
  row("the family's listing: {1, 2} x {1, 2} = 4 rows of family 27", rows == 4);
  row("interleaved_fused: every size up to 65536 (no measured size loses)", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (!interleaved_fused(n)) return false;
    return true;
  }());

  // ---- lengths and positions ----
  const int lengths[] = {1, 3, 63, 64, 65, 1023, 1025, 1115};
  for (int total : lengths) {
    snprintf(what, sizeof(what), "  %d sample-frames: fused", total);
    expect(what, call(2, 2, total), 2, nullptr, true);
  }
  expect("  64 sample-frames at position 1024, planar-compatible: fused (the flag at 0: the fast kernel takes frame size 1 nowhere)",
         call(1, 1, 64, 1024), 1, nullptr, true);
  expect("  0 sample-frames", call(2, 2, 0), 2, nullptr, false);
  const struct {
    int64_t pos;
    bool fused;
  } positions[] = {{0, true}, {16, true}, {239, false}, {240, true}, {241, true}, {1115, true}, {((int64_t)1 << 31) + 1, true}};
  for (const auto &c : positions) {
    snprintf(what, sizeof(what), "  position %lld: %s", (long long)c.pos, c.fused ? "fused" : "the general kernel");
    expect(what, call(2, 2, 1115, c.pos), 2, nullptr, c.fused);
  }
  expect("  position 8: the general kernel", call(2, 2, 1115, 8), 2, nullptr, false);

  // ---- one field changed at a time ----
  const RenderParams ps = call(2, 2), pm = call(1, 1);
  expect("  interleaved = 0: as iamf_hip_batch_render_range", with(ps, [](RenderParams &p) { p.interleaved = 0; }), 2, nullptr, false);
  expect("  limiter off (dense sample-frames are no planar rows: the general kernel)", with(ps, [](RenderParams &p) { p.limiter_on = 0; }), 2, nullptr,
         false);
  expect("  3 output channels", call(2, 3), 2, nullptr, false);
  expect("  6 output channels", call(2, 6), 2, nullptr, false);
  expect("  4 input channels", call(4, 2), 4, nullptr, false);
  expect("  output gain on fewer channels than rendered", with(ps, [](RenderParams &p) { p.og_ch = 1; }), 2, nullptr, false);
  expect("  a limiter table shorter than the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin - 1; }), 2, nullptr, false);
  expect("  a limiter table of exactly the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin; }), 2, nullptr, true);
  expect("  a second element", with(ps, [](RenderParams &p) { p.in2 = kIn + 65536, p.m2 = 2, p.in2_frame_stride = 2, p.in2_stream_stride = 4096; }), 2,
         nullptr, false);
  expect("  an element ramp", with(ps, [](RenderParams &p) { p.elem_ramp = kRamp, p.ramp_stream_stride = 4096; }), 2, nullptr, false);
  expect("  an output ramp", with(ps, [](RenderParams &p) { p.out_ramp = kRamp, p.ramp_stream_stride = 4096; }), 2, nullptr, false);
  expect("  down-mixer", with(ps, [](RenderParams &p) { p.dmx_on = 1; }), 2, nullptr, false);
  expect("  demixer", with(ps, [](RenderParams &p) { p.demix_on = 1; }), 2, nullptr, false);
  expect("  de-mapping matrix", with(ps, [](RenderParams &p) { p.pre_matrix = kIn; }), 2, nullptr, false);
  expect("  HRTF stage: refused as before", with(ps, [](RenderParams &p) { p.fir_taps = 256; }), 2, nullptr, false, Family::Refused);
  expect("  LFE generator", with(ps, [](RenderParams &p) { p.lfe = kIn; }), 2, nullptr, false);
  expect("  flush (no input)", with(ps, [](RenderParams &p) { p.in = nullptr; }), 2, nullptr, false);
  expect("  in_frame_stride == M + 1 (strided)", with(ps, [](RenderParams &p) { p.in_frame_stride = 3; }), 2, nullptr, false);
  expect("  mono, in_frame_stride == 2 (strided)", with(pm, [](RenderParams &p) { p.in_frame_stride = 2; }), 1, nullptr, false);
  expect("  input base + 4 B", with(ps, [](RenderParams &p) { p.in += 1; }), 2, nullptr, false);
  expect("  input base + 8 B", with(ps, [](RenderParams &p) { p.in += 2; }), 2, nullptr, false);
  expect("  input base + 16 B", with(ps, [](RenderParams &p) { p.in += 4; }), 2, nullptr, true);
  expect("  stream stride 2 floats off the 16-byte grid", with(ps, [](RenderParams &p) { p.in_stream_stride += 2; }), 2, nullptr, false);
  expect("  stream stride + 4 floats", with(ps, [](RenderParams &p) { p.in_stream_stride += 4; }), 2, nullptr, true);
  expect("  pcm + 2 B", with(ps, [](RenderParams &p) { p.pcm += 2; }), 2, nullptr, false);
  expect("  pcm stream stride + 4 B", with(ps, [](RenderParams &p) { p.pcm_stream_stride += 4; }), 2, nullptr, false);
  expect("  frame size 1024 (the entry refuses such a batch; the route would not fuse it either)",
         with(ps, [](RenderParams &p) { p.frame_size = 1024, p.total = 1024, p.in_frame_stride = 2048; }), 2, nullptr, false, Family::Fast);
  // total * M * 4 + 2^24 < 2^31
  constexpr int kMax2 = ((1u << 31) - (1u << 24) - 1) / 8, kMax1 = ((1u << 31) - (1u << 24) - 1) / 4;
  static_assert((int64_t)kMax2 * 8 + (1 << 24) < ((int64_t)1 << 31) && (int64_t)(kMax2 + 1) * 8 + (1 << 24) >= ((int64_t)1 << 31), "the bound");
  expect("  stereo, total at the 32-bit bound", call(2, 2, kMax2), 2, nullptr, true);
  expect("  stereo, one sample-frame beyond", call(2, 2, kMax2 + 1), 2, nullptr, false);
  expect("  mono, total at the 32-bit bound", call(1, 1, kMax1), 1, nullptr, true);
  expect("  mono, one sample-frame beyond", call(1, 1, kMax1 + 1), 1, nullptr, false);
  expect("  n_launch = 65536", with(ps, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 2, nullptr, true);
  expect("  IAMF_HIP_FORCE_GENERIC", ps, 2, "IAMF_HIP_FORCE_GENERIC", false);
  expect("  IAMF_HIP_INTERLEAVED_UNFUSED", ps, 2, "IAMF_HIP_INTERLEAVED_UNFUSED", false);

  // ---- the flag at 0 changes nothing: an aligned planar call of the fast kernel, with and without the switch ----
  {
    RenderParams p = call(2, 2, 4096, 0);
    p.interleaved = 0;
    p.frame_size = 1024;
    p.in_frame_stride = 2048;
    p.in_stream_stride = 8192;
    const Route a = pick_route(p, 2);
    setenv("IAMF_HIP_INTERLEAVED_UNFUSED", "1", 1);
    const Route b = pick_route(p, 2);
    unsetenv("IAMF_HIP_INTERLEAVED_UNFUSED");
    row("interleaved = 0, planar stereo 4 x 1024: Fast, whatever the switch says", a.family == Family::Fast && same_route(a, b));
  }

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
