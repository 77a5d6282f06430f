// Host-only check of the routing of the limiter-less renderer's two-element packet form: nolim_packets_mix_shape_ok() and
// pick_route(const RenderMixParams &) in iac_amd/csrc/render_route.hpp (Family::NolimPacketsMix, reached through the value 5 of the
// host-only field RenderParams::ragged, which iamf_hip_batch_render_packets_mix_nolim alone sets) behind lpcm_form_packets() of
// lpcm_form.hpp on each element, put together as render_lpcm_mix_impl and render_prepare (iamf_render.hip) put them together.  One
// row per rule, with that rule flipped and nothing else: the form's kernel on the near side, on the far side exactly the route the
// same block gets without the mark.  The kernel loads a lane's four samples of either element as 8, 12, 16 or 2 x 12 bytes and a
// ramp's four floats as one float4, and trusts the host that they are aligned and end inside the samples of the call: a wrong row
// here is a misaligned or stray load on the GPU, not a slower rate.
// Driven by tests/test_route_host_nolim_packets_mix.py.
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
#include "../../iac_amd/csrc/lpcm_form.hpp"

int g_failed = 0, g_cases = 0;

void row(const char *what, bool ok) {
  printf("%-118s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

// one element's packets of a call (addresses are never dereferenced: routing looks at alignment only)
struct Elem {
  iamf_hip_lpcm_layout L;
  int ch;
  int64_t raw_stream_stride, raw_frame_stride;
  uintptr_t raw;
};

// ch channels of `bytes`-byte samples: mono-coded runs, or (coupled) the loudspeaker layouts' pairs and mono runs, one behind
// the other behind a head of 16 bytes, every run's start on the 8-byte grid
Elem elem(int ch, int bytes, bool coupled, int frame_size, int frames, uintptr_t raw) {
  Elem e;
  memset(&e, 0, sizeof(e));
  e.ch = ch;
  e.L.sample_bytes = bytes;
  e.L.little_endian = 1;
  e.L.channels = ch;
  e.L.frame_size = frame_size;
  int off = 16;
  for (int k = 0; k < ch; ++k) {
    const bool paired = coupled && lpcm_coupled_paired(ch, k);
    if (paired && (k & 1)) {
      e.L.src_offset[k] = e.L.src_offset[k - 1] + bytes;
      e.L.src_step[k] = 2 * bytes;
      off = (off + 2 * bytes * frame_size + 7) & ~7;
    } else {
      e.L.src_offset[k] = off;
      e.L.src_step[k] = paired ? 2 * bytes : bytes;
      if (!paired) off = (off + bytes * frame_size + 7) & ~7;
    }
  }
  e.raw_frame_stride = (off + 15) & ~15;
  e.raw_stream_stride = e.raw_frame_stride * (frames + 1);
  e.raw = raw;
  return e;
}

// a two-element packet call on a batch, as the entry sees it
struct Call {
  Elem e0, e1;
  int first, total, frame_size;
  int limiter_on, out_ch, og_ch, out_format;
  uintptr_t pcm, ramp[3];   // element 0's, element 1's, the output's (0: none)
  int64_t pcm_stream_stride, ramp_stream_stride;
};

// the bed: m channels (coupled where m is a loudspeaker layout's count); element 1: lp2 == 2 one coupled stereo pair, lp2 == 1 m2
// mono runs (0: one for odd m, four for even); both of `bytes`-byte samples unless bytes1 says otherwise
Call call(int m, int bytes, int lp2, int frame_size = 1000, int total = 1000, int first = 0, int out_ch = 2, int fmt = IAMF_HIP_FMT_F32, int m2 = 0,
          int bytes1 = 0) {
  Call c;
  memset(&c, 0, sizeof(c));
  const int frames = total / frame_size;
  c.e0 = elem(m, bytes, LpcmCoupledM::has(m), frame_size, frames, 0x10000);
  c.e1 = elem(lp2 == 2 ? 2 : (m2 ? m2 : ((m & 1) ? 1 : 4)), bytes1 ? bytes1 : bytes, lp2 == 2, frame_size, frames, 0x8000000);
  c.first = first;
  c.total = total;
  c.frame_size = frame_size;
  c.out_ch = c.og_ch = out_ch;
  c.out_format = fmt;
  c.pcm = 0x40000;
  c.pcm_stream_stride = (((int64_t)total * out_ch * 4) + 15) & ~(int64_t)15;
  c.ramp_stream_stride = (total + 3) & ~3;
  return c;
}

// the block render_prepare builds for the fused attempt of iamf_hip_batch_render_packets_mix_nolim; false: render_lpcm_mix_impl finds
// no pair of forms the mix kernels read (or render_prepare sample sizes that differ), and makes no attempt
bool block_of(const Call &c, RenderMixParams &p) {
  const LpcmForm f0 = lpcm_form_packets(c.e0.L, c.e0.ch, c.e0.raw_stream_stride, c.e0.raw_frame_stride, c.e0.raw, c.first);
  const LpcmForm f1 = lpcm_form_packets(c.e1.L, c.e1.ch, c.e1.raw_stream_stride, c.e1.raw_frame_stride, c.e1.raw, c.first);
  const int m = c.e0.ch, m2 = c.e1.ch;
  bool ok0 = (f0 == LpcmForm::S16 && LpcmM::has(m)) || f0 == LpcmForm::S16C;
  bool ok1 = (f1 == LpcmForm::S16 || f1 == LpcmForm::S16C) && lpcm_mix_m2_ok(f1 == LpcmForm::S16C ? 2 : 1, m2);
  if (!(ok0 && ok1)) {
    ok0 = (f0 == LpcmForm::S24 && LpcmM::has(m)) || f0 == LpcmForm::S24C;
    ok1 = (f1 == LpcmForm::S24 || f1 == LpcmForm::S24C) && lpcm_mix_m2_ok(f1 == LpcmForm::S24C ? 2 : 1, m2);
  }
  if (!(ok0 && ok1) || c.e0.L.sample_bytes != c.e1.L.sample_bytes) return false;
  memset(&p, 0, sizeof(p));
  p.frame_size = c.frame_size;
  p.total = c.total;
  p.lpcm = reinterpret_cast<const uint8_t *>(c.e0.raw);
  p.in = reinterpret_cast<const float *>(c.e0.raw);   // the placeholder render_lpcm_mix_impl sets: "not a flush"
  p.lpcm_stream_stride = c.e0.raw_stream_stride;
  p.lpcm_frame_stride = c.e0.raw_frame_stride;
  p.lpcm_bytes = c.e0.L.sample_bytes;
  p.lpcm_coupled = f0 == LpcmForm::S16C ? 1 : (f0 == LpcmForm::S24C ? 2 : 0);
  for (int k = 0; k < m; ++k) p.lpcm_off[k] = c.e0.L.src_offset[k] + c.e0.L.src_step[k] * c.first;
  const bool pair = f1 == LpcmForm::S16C || f1 == LpcmForm::S24C;
  p.lpcm_mix = (p.lpcm_bytes == 3 ? 4 : 0) | (pair ? 2 : 1);
  p.in2 = reinterpret_cast<const float *>(c.e1.raw);
  p.in2_stream_stride = c.e1.raw_stream_stride;
  p.in2_frame_stride = c.e1.raw_frame_stride;
  p.lpcm2 = reinterpret_cast<const uint8_t *>(c.e1.raw);
  p.lpcm2_stream_stride = c.e1.raw_stream_stride;
  p.lpcm2_frame_stride = c.e1.raw_frame_stride;
  for (int k = 0; k < m2 && k < 4; ++k) p.lpcm2_off[k] = c.e1.L.src_offset[k] + c.e1.L.src_step[k] * c.first;
  p.m2 = m2;
  p.matrix2 = reinterpret_cast<const float *>(0x30000);
  p.src_feed2 = reinterpret_cast<const int32_t *>(0x31000);
  p.gains2 = reinterpret_cast<const float *>(0x32000);
  p.elem_ramp = reinterpret_cast<const float *>(c.ramp[0]);
  p.elem2_ramp = reinterpret_cast<const float *>(c.ramp[1]);
  p.out_ramp = reinterpret_cast<const float *>(c.ramp[2]);
  p.ramp_stream_stride = c.ramp_stream_stride;
  p.pcm = reinterpret_cast<uint8_t *>(c.pcm);
  p.pcm_stream_stride = c.pcm_stream_stride;
  p.out_ch = c.out_ch;
  p.og_ch = c.og_ch;
  p.out_format = c.out_format;
  p.limiter_on = c.limiter_on;
  p.n_streams = p.n_launch = 64;
  p.n_atk = 48;
  p.n_end = 9649;
  p.ragged = 5;
  p.demix_i0 = c.first;
  return true;
}

bool same_key(const RouteKey &k, int f, int v, int m, int c, int kk) {
  return f == k.family && v == k.variant && m == k.m && c == k.c && kk == k.k;
}
int sets_of(const RouteKey &k) {
  int mask = 0;
  for (int s = 0; s < kRouteSets; ++s)
    for_each_instance_of_set(s, [&](int f, int v, int km, int kc, int kk) { mask |= same_key(k, f, v, km, kc, kk) ? 1 << s : 0; });
  return mask;
}
bool same_route(const Route &a, const Route &b) { return a.family == b.family && a.variant == b.variant && a.err == b.err; }

// fused: the rule holds, the family is NolimPacketsMix, its key the row (47, sample bytes, m, 0, LP2) of set 12 and of no other
// set.  Else: no pair of forms, or the rule does not hold and the block routes exactly as without the mark — through either
// pick_route.  `tweak` changes the block behind the form check (a batch property no layout shows).
template <class F>
void expect(const char *what, const Call &c, bool fused, F tweak, const char *env = nullptr) {
  if (env) setenv(env, "1", 1);
  RenderMixParams p;
  bool ok;
  if (!block_of(c, p)) {
    ok = !fused;
  } else {
    tweak(p);
    const int m = c.e0.ch;
    const bool rule = nolim_packets_mix_shape_ok(p, m, getenv("IAMF_HIP_FORCE_GENERIC") != nullptr);
    const Route r = pick_route(p, m);
    if (fused) {
      const RouteKey k = route_key(r, p, m);
      const int lp2 = p.lpcm_mix & 3;
      ok = rule && r.family == Family::NolimPacketsMix && r.variant == lp2 && r.err == IAMF_HIP_OK && k.set == 12 && sets_of(k) == 1 << 12 &&
           same_key(k, IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX, c.e0.L.sample_bytes, m, 0, lp2);
    } else {
      RenderMixParams q = p;
      q.ragged = 0;
      ok = !rule && r.family != Family::NolimPacketsMix && same_route(r, pick_route(q, m)) &&
           same_route(r, pick_route(static_cast<const RenderParams &>(q), m));
    }
  }
  if (env) unsetenv(env);
  row(what, ok);
}
void expect(const char *what, const Call &c, bool fused, const char *env = nullptr) {
  expect(what, c, fused, [](RenderMixParams &) {}, env);
}
template <class F>
Call with(Call c, F f) {
  f(c);
  return c;
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED", "IAMF_HIP_NOLIM_PACKETS_UNFUSED", "IAMF_HIP_LPCM_UNFUSED",
                                  "IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE",
                                  "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  char what[240];

  // ---- the number, the block, the sets ----
  static_assert(IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX == 47 && IAMF_HIP_ROUTE_NOLIM_PACKETS == 43 && IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED == 39, "stable numbers");
  static_assert(sizeof(RenderParams) == 616 && offsetof(RenderParams, ragged) == 412, "the block keeps its size: the mark is a new VALUE of `ragged`");
  static_assert(sizeof(RenderMixParams) == 616 + 8 + 16 + 16, "and so does the block behind it");
  static_assert((int)Family::NolimPacketsMix == (int)Family::NolimPackets + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 12 + 1 && kRouteTables == 3, "set 12 behind the three tables; sets added later leave it alone");
  static_assert(kNlChunk == 1024 && kNlMaxFrameBytes == 60, "the tile");

  // ---- every instance: 36 rows, each fused into every PCM format ----
  int rows = 0;
  for_each_render_instance_nolim_packets_mix([&](int f, int v, int m, int c, int k) {
    const bool mono = LpcmM::has(m), cpl = LpcmCoupledM::has(m);
    rows += (f == IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX && (v == 2 || v == 3) && c == 0 && (mono != cpl) && LpcmMixK::has(k)) ? 1 : 1000;
    for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_S32, IAMF_HIP_FMT_F32}) {
      snprintf(what, sizeof(what), "instance m = %d, %d bit, LP2 = %d, stereo format %d: fused", m, 8 * v, k, fmt);
      // (stereo s24 is 6 bytes per sample-frame: no whole dwords, so that one is the twin's)
      expect(what, call(m, v, k, 1000, 1000, 0, 2, fmt), fmt != IAMF_HIP_FMT_S24);
    }
  });
  row("the family lists 36 rows", rows == 36);
  {
    row("set 12 of for_each_instance_of_set is the listing: 36 rows, family 47 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX, 12, 36));
    row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
    row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  }

  const Call toa = call(16, 2, 2), b714 = call(12, 3, 1), b51 = call(6, 2, 1), foa4 = call(4, 2, 1);
  const uintptr_t R0 = 0x50000, R1 = 0x60000, R2 = 0x70000;

  // ---- one case per rule, flipped alone ----
  expect("3rd order + coupled stereo, 16 bit -> stereo f32, one frame of 1000: fused", toa, true);
  expect("7.1.4 coupled + mono, 24 bit -> stereo f32: fused", b714, true);
  expect("5.1 coupled + first order, 16 bit: fused", b51, true);
  expect("first order + first order (m2 = 4), 16 bit: fused", foa4, true);
  expect("limiter on", with(toa, [](Call &c) { c.limiter_on = 1; }), false);
  expect("total = 6 (a trimmed frame of 6 samples)", with(toa, [](Call &c) { c.total = 6; }), false);
  expect("total = 8: fused", with(toa, [](Call &c) { c.total = 8; }), true);
  expect("total = 4, one quad: fused", with(toa, [](Call &c) { c.total = 4; }), true);
  expect("total = 0", toa, false, [](RenderMixParams &p) { p.total = 0; });
  expect("total = 1002", call(16, 2, 2, 1004, 1002), false);
  expect("frame size = 6 (lpcm_form_check refuses it; the rule does too)", toa, false, [](RenderMixParams &p) { p.frame_size = 6, p.total = 12; });
  expect("frame size = 2", toa, false, [](RenderMixParams &p) { p.frame_size = 2, p.total = 4; });
  expect("first 100, n = fs - first: fused", call(16, 2, 1, 1000, 900, 100), true);
  expect("first 4 and fs - 4: fused", call(16, 2, 1, 1000, 996, 4), true);
  expect("                         ", call(16, 2, 1, 1000, 4, 996), true);
  expect("first + n > fs", call(16, 2, 1, 1000, 900, 100), false, [](RenderMixParams &p) { p.total = 904; });
  expect("first < 0", call(16, 2, 1, 1000, 900, 100), false, [](RenderMixParams &p) { p.demix_i0 = -4; });
  expect("first > 0 with whole frames", toa, false, [](RenderMixParams &p) { p.demix_i0 = 4; });
  expect("first 2: the mono runs of either element 4 bytes off the 8-byte grid", call(16, 2, 1, 1000, 996, 2), false);
  expect("first 2, a coupled stereo bed and a coupled stereo second: 8 bytes on, fused", call(2, 2, 2, 1000, 996, 2), true);
  expect("first 2, a coupled stereo bed, a mono second: element 1 off its grid", call(2, 2, 1, 1000, 996, 2, 2, IAMF_HIP_FMT_F32, 1), false);
  // element 1 off its grid, 16 and 24 bit; the pair's partner
  expect("element 1: a 16-bit run off the 8-byte grid", with(foa4, [](Call &c) { c.e1.L.src_offset[2] += 4; }), false);
  expect("element 1: a 16-bit run off the grid behind the form check", foa4, false, [](RenderMixParams &p) { p.lpcm2_off[3] += 4; });
  expect("element 1: a 24-bit run off the dword grid", with(call(4, 3, 1), [](Call &c) { c.e1.L.src_offset[1] += 2; }), false);
  expect("element 1: a 24-bit run off the grid behind the form check", call(4, 3, 1), false, [](RenderMixParams &p) { p.lpcm2_off[0] += 2; });
  expect("element 1: a negative run start", foa4, false, [](RenderMixParams &p) { p.lpcm2_off[1] = -8; });
  expect("element 1: raw_frame_stride off the grid", with(toa, [](Call &c) { c.e1.raw_frame_stride += 4; }), false);
  expect("element 1: raw_stream_stride off the grid", with(toa, [](Call &c) { c.e1.raw_stream_stride += 4; }), false);
  expect("element 1: d_raw off the 16-byte grid", with(toa, [](Call &c) { c.e1.raw += 8; }), false);
  expect("element 1: the kernel's block and pick_route's fields disagree", toa, false, [](RenderMixParams &p) { p.lpcm2 += 16; });
  expect("element 1: no packets behind the block", toa, false, [](RenderMixParams &p) { p.lpcm2 = nullptr; });
  expect("element 1: the pair's partner misplaced", with(toa, [](Call &c) { c.e1.L.src_offset[1] += 4; }), false);
  expect("element 1: the pair's partner misplaced behind the form check", toa, false, [](RenderMixParams &p) { p.lpcm2_off[1] += 2; });
  expect("element 1: the 24-bit pair's partner misplaced behind the form check", call(16, 3, 2), false, [](RenderMixParams &p) { p.lpcm2_off[1] -= 1; });
  expect("m2 = 2 as two mono runs", call(16, 2, 1, 1000, 1000, 0, 2, IAMF_HIP_FMT_F32, 2), false);
  expect("m2 = 3", call(16, 2, 1, 1000, 1000, 0, 2, IAMF_HIP_FMT_F32, 3), false);
  expect("m2 = 2 behind the form check, LP2 = 1", foa4, false, [](RenderMixParams &p) { p.m2 = 2; });
  expect("m2 = 4 with LP2 = 2", toa, false, [](RenderMixParams &p) { p.m2 = 4; });
  expect("sample sizes that differ: 16-bit bed, 24-bit second", call(16, 2, 2, 1000, 1000, 0, 2, IAMF_HIP_FMT_F32, 0, 3), false);
  expect("sample sizes that differ: 24-bit bed, 16-bit second", call(16, 3, 1, 1000, 1000, 0, 2, IAMF_HIP_FMT_F32, 0, 2), false);
  expect("lpcm_mix names the other sample size's form", toa, false, [](RenderMixParams &p) { p.lpcm_mix = 4 | 2; });
  expect("lpcm_mix 0", toa, false, [](RenderMixParams &p) { p.lpcm_mix = 0; });
  expect("lpcm_mix 3", toa, false, [](RenderMixParams &p) { p.lpcm_mix = 3; });
  expect("no second element on the block", toa, false, [](RenderMixParams &p) { p.in2 = nullptr; });
  expect("big-endian bed", with(toa, [](Call &c) { c.e0.L.little_endian = 0; }), false);
  expect("big-endian second", with(toa, [](Call &c) { c.e1.L.little_endian = 0; }), false);
  // element 0's form, as nolim_packets_shape_ok checks it
  expect("element 0: a 16-bit run off the 8-byte grid", with(toa, [](Call &c) { c.e0.L.src_offset[5] += 4; }), false);
  expect("element 0: a run off the grid behind the form check", toa, false, [](RenderMixParams &p) { p.lpcm_off[7] += 4; });
  expect("element 0: raw_frame_stride off the grid", with(toa, [](Call &c) { c.e0.raw_frame_stride += 4; }), false);
  expect("element 0: d_raw off the 16-byte grid", with(toa, [](Call &c) { c.e0.raw += 8; }), false);
  expect("element 0: a pair's partner elsewhere", with(b51, [](Call &c) { c.e0.L.src_offset[1] += 4; }), false);
  expect("element 0: mono-coded 5.1", with(b51, [](Call &c) { c.e0 = elem(6, 2, false, 1000, 1, 0x10000); }), false);
  expect("element 0: m = 3", call(3, 2, 1), false);
  expect("element 0: lpcm_coupled names the other sample size's form", b51, false, [](RenderMixParams &p) { p.lpcm_coupled = 2; });
  expect("element 0: lpcm_bytes 0", toa, false, [](RenderMixParams &p) { p.lpcm_bytes = 0; });
  // ramps
  expect("element ramp: fused", with(toa, [=](Call &c) { c.ramp[0] = R0; }), true);
  expect("element-2 ramp: fused", with(toa, [=](Call &c) { c.ramp[1] = R1; }), true);
  expect("output ramp: fused", with(toa, [=](Call &c) { c.ramp[2] = R2; }), true);
  expect("all three ramps: fused", with(toa, [=](Call &c) { c.ramp[0] = R0, c.ramp[1] = R1, c.ramp[2] = R2; }), true);
  expect("element ramp off 16 bytes", with(toa, [=](Call &c) { c.ramp[0] = R0 + 4; }), false);
  expect("element-2 ramp off 16 bytes", with(toa, [=](Call &c) { c.ramp[1] = R1 + 4; }), false);
  expect("output ramp off 16 bytes", with(toa, [=](Call &c) { c.ramp[0] = R0, c.ramp[2] = R2 + 8; }), false);
  expect("a ramp stride of 4k + 1", with(toa, [=](Call &c) { c.ramp[1] = R1, c.ramp_stream_stride = 1001; }), false);
  expect("a ramp stride of 4k + 2", with(toa, [=](Call &c) { c.ramp[2] = R2, c.ramp_stream_stride = 1002; }), false);
  expect("a ramp stride of 4k + 1 without a ramp says nothing: fused", with(toa, [](Call &c) { c.ramp_stream_stride = 1001; }), true);
  // PCM
  expect("d_pcm off the 16-byte grid", with(toa, [](Call &c) { c.pcm += 8; }), false);
  expect("pcm_stream_stride off the 16-byte grid", with(toa, [](Call &c) { c.pcm_stream_stride += 8; }), false);
  expect("out_ch * bytes = 2 (mono s16)", call(16, 2, 2, 1000, 1000, 0, 1, IAMF_HIP_FMT_S16), false);
  expect("out_ch * bytes = 4 (mono f32): fused", call(16, 2, 2, 1000, 1000, 0, 1, IAMF_HIP_FMT_F32), true);
  expect("out_ch * bytes = 60 (15 x f32): fused", call(16, 2, 2, 1000, 1000, 0, 15, IAMF_HIP_FMT_F32), true);
  expect("out_ch * bytes = 64 (16 x f32)", call(16, 2, 2, 1000, 1000, 0, 16, IAMF_HIP_FMT_F32), false);
  expect("5.1 s16, 14 channels s16: fused", call(16, 2, 2, 1000, 1000, 0, 6, IAMF_HIP_FMT_S16), true);
  expect("                               ", call(16, 2, 2, 1000, 1000, 0, 14, IAMF_HIP_FMT_S16), true);
  expect("6 channels s24 (18 bytes)", call(16, 2, 2, 1000, 1000, 0, 6, IAMF_HIP_FMT_S24), false);
  // every stage that keeps the form away
  expect("down-mixer", toa, false, [](RenderMixParams &p) { p.dmx_on = 1; });
  expect("demixer", toa, false, [](RenderMixParams &p) { p.demix_on = 1; });
  expect("pre-matrix", toa, false, [](RenderMixParams &p) { p.pre_matrix = reinterpret_cast<const float *>(0x20000); });
  expect("HRTF stage", toa, false, [](RenderMixParams &p) { p.fir_taps = 256; });
  expect("LFE generator", toa, false, [](RenderMixParams &p) { p.lfe = reinterpret_cast<const float *>(0x20000); });
  expect("reduced out_gain_channels", with(toa, [](Call &c) { c.og_ch = 1; }), false);
  expect("a flush (no input)", toa, false, [](RenderMixParams &p) { p.in = nullptr; });
  // the marks and the switches
  expect("the mark of the limiter-on entry (3)", toa, false, [](RenderMixParams &p) { p.ragged = 3; });
  expect("the mark of the single-element entry (4)", toa, false, [](RenderMixParams &p) { p.ragged = 4; });
  expect("no mark", toa, false, [](RenderMixParams &p) { p.ragged = 0; });
  expect("IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED", toa, false, "IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED");
  expect("IAMF_HIP_LPCM_UNFUSED", toa, false, "IAMF_HIP_LPCM_UNFUSED");
  expect("IAMF_HIP_FORCE_GENERIC", toa, false, "IAMF_HIP_FORCE_GENERIC");
  expect("IAMF_HIP_NOLIM_PACKETS_UNFUSED says nothing here: fused", toa, true, "IAMF_HIP_NOLIM_PACKETS_UNFUSED");
  expect("IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED says nothing here: fused", toa, true, "IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED");
  // lengths: whole frames, chunk boundaries
  for (int n : {4, 1020, 1024, 1028, 2044})
    expect("frame size 2048, a trimmed call of 4 .. 2044: fused", call(9, 3, 1, 2048, n), true);
  for (int n : {4, 1020, 1024, 1028, 2052})
    expect("frames of 4, 4 .. 2052 samples: fused", call(4, 2, 1, 4, n), true);
  for (int fs : {8, 240, 1000, 1024})
    expect("frame sizes 8, 240, 1000, 1024, five frames: fused", call(6, 3, 2, fs, 5 * fs), true);
  // a far call: 64-bit addressing, no bound on the extent
  expect("element 1: a frame stride of 2^30 bytes, 64 frames: fused",
         with(toa, [](Call &c) { c.e1.raw_frame_stride = (int64_t)1 << 30, c.e1.raw_stream_stride = (int64_t)1 << 37, c.total = 64000; }), true);

  // ---- the mark changes no other call's route: a block with mark 4 or none, and a limiter-on one with mark 5, route as in the parent
  // (the rules of pick_route(const RenderParams &), which this change leaves as they are) ----
  int same = 0, all = 0;
  for_each_render_instance_nolim_packets_mix([&](int, int v, int m, int, int k) {
    for (int total : {1000, 1024, 64}) {
      RenderMixParams p;
      if (!block_of(with(call(m, v, k, total, total, 0, 2, IAMF_HIP_FMT_S16), [](Call &c) { c.limiter_on = 1; }), p)) continue;
      p.pos0 = 1024;
      for (int mark : {0, 3, 4, 5}) {
        RenderMixParams q = p;
        q.ragged = mark;
        ++all;
        same += same_route(pick_route(q, m), pick_route(static_cast<const RenderParams &>(q), m)) ? 1 : 0;
      }
      RenderMixParams q = p, q0 = p;
      q0.ragged = 0;
      ++all;
      same += same_route(pick_route(q, m), pick_route(q0, m)) ? 1 : 0;
    }
  });
  row("limiter-on blocks route through the older rules, and with mark 5 as without a mark", all == 36 * 3 * 5 && same == all);

  printf("%d cases, %d wrong\n%s\n", g_cases, g_failed, g_failed ? "FAILED" : "OK");
  return g_failed ? 1 : 0;
}
