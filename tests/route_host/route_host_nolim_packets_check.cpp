// Host-only check of the packet-fed limiter-less renderer's routing: nolim_packets_shape_ok() and pick_route() in
// iac_amd/csrc/render_route.hpp (Family::NolimPackets, reached through the value 4 of the host-only field RenderParams::ragged,
// which iamf_hip_batch_render_packets_nolim alone sets) behind lpcm_form_packets() of lpcm_form.hpp, put together as
// render_prepare (iamf_render.hip) puts them together.  One row per rule, with that rule flipped and nothing else: the form's
// kernel on the near side, on the far side exactly the route the same block gets without the mark.  The kernel loads a lane's
// four samples as 8, 12, 16 or 2 x 12 bytes and trusts the host that the quad is aligned and ends inside the samples of the
// call: a wrong row here is a misaligned or stray load on the GPU, not a slower rate.
// Driven by tests/test_route_host_nolim_packets.py.
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

// a packet call on a batch, as the entry sees it (addresses are never dereferenced: routing looks at alignment only)
struct Call {
  iamf_hip_lpcm_layout L;
  int ch;
  int64_t raw_stream_stride, raw_frame_stride;
  uintptr_t raw, pcm;
  int first, total, frame_size;
  int limiter_on, out_ch, og_ch, out_format;
  int64_t pcm_stream_stride;
};

// ch channels of `bytes`-byte samples: mono-coded runs, or (coupled) the loudspeaker layouts' pairs and mono runs, one behind
// the other behind a head of 16 bytes, every run's start on the 8-byte grid
Call call(int ch, int bytes, bool coupled, int frame_size = 1000, int total = 1000, int first = 0, int out_ch = 2, int fmt = IAMF_HIP_FMT_F32) {
  Call c;
  memset(&c, 0, sizeof(c));
  c.ch = ch;
  c.L.sample_bytes = bytes;
  c.L.little_endian = 1;
  c.L.channels = ch;
  c.L.frame_size = frame_size;
  int off = 16;
  for (int k = 0; k < ch; ++k) {
    const bool paired = coupled && lpcm_coupled_paired(ch, k);
    if (paired && (k & 1)) {
      c.L.src_offset[k] = c.L.src_offset[k - 1] + bytes;
      c.L.src_step[k] = 2 * bytes;
      off = (off + 2 * bytes * frame_size + 7) & ~7;
    } else {
      c.L.src_offset[k] = off;
      c.L.src_step[k] = paired ? 2 * bytes : bytes;
      if (!paired) off = (off + bytes * frame_size + 7) & ~7;
    }
  }
  c.raw_frame_stride = (off + 15) & ~15;
  c.raw_stream_stride = c.raw_frame_stride * (total / frame_size + 1);
  c.raw = 0x10000;
  c.pcm = 0x40000;
  c.first = first;
  c.total = total;
  c.frame_size = frame_size;
  c.limiter_on = 0;
  c.out_ch = c.og_ch = out_ch;
  c.out_format = fmt;
  c.pcm_stream_stride = (((int64_t)total * out_ch * 4) + 15) & ~(int64_t)15;
  return c;
}

// the block render_prepare builds for the fused attempt of iamf_hip_batch_render_packets_nolim; false: no form, no attempt
bool block_of(const Call &c, RenderParams &p) {
  const LpcmForm form = lpcm_form_packets(c.L, c.ch, c.raw_stream_stride, c.raw_frame_stride, c.raw, c.first);
  if (form == LpcmForm::None) return false;
  memset(&p, 0, sizeof(p));
  p.frame_size = c.frame_size;
  p.total = c.total;
  p.lpcm = reinterpret_cast<const uint8_t *>(c.raw);
  p.in = reinterpret_cast<const float *>(c.raw);   // the placeholder render_lpcm_range_impl sets: "not a flush"
  p.lpcm_stream_stride = c.raw_stream_stride;
  p.lpcm_frame_stride = c.raw_frame_stride;
  p.lpcm_bytes = c.L.sample_bytes;
  p.lpcm_coupled = form == LpcmForm::S16C ? 1 : (form == LpcmForm::S24C ? 2 : 0);
  for (int k = 0; k < c.ch; ++k) p.lpcm_off[k] = c.L.src_offset[k] + c.L.src_step[k] * c.first;
  p.pcm = reinterpret_cast<uint8_t *>(c.pcm);
  p.pcm_stream_stride = c.pcm_stream_stride;
  p.out_ch = c.out_ch;
  p.og_ch = c.og_ch;
  p.out_format = c.out_format;
  p.limiter_on = c.limiter_on;
  p.n_streams = p.n_launch = 64;
  p.n_atk = 48;
  p.n_end = 9649;
  p.ragged = 4;
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

// fused: the rule holds, the family is NolimPackets, its key the row (43, 0, m, 0, sample bytes) of set 11 and of no other set.
// Else: no form, or the rule does not hold and the block routes exactly as without the mark.  `tweak` changes the block behind
// the form check (a batch property no layout shows).
template <class F>
void expect(const char *what, const Call &c, bool fused, F tweak, const char *env = nullptr) {
  if (env) setenv(env, "1", 1);
  RenderParams p;
  bool ok;
  if (!block_of(c, p)) {
    ok = !fused;
  } else {
    tweak(p);
    const bool rule = nolim_packets_shape_ok(p, c.ch, getenv("IAMF_HIP_FORCE_GENERIC") != nullptr);
    const Route r = pick_route(p, c.ch);
    if (fused) {
      const RouteKey k = route_key(r, p, c.ch);
      ok = rule && r.family == Family::NolimPackets && r.variant == 0 && r.err == IAMF_HIP_OK && k.set == 11 && sets_of(k) == 1 << 11 &&
           same_key(k, IAMF_HIP_ROUTE_NOLIM_PACKETS, 0, c.ch, 0, c.L.sample_bytes);
    } else {
      RenderParams q = p;
      q.ragged = 0;
      ok = !rule && r.family != Family::NolimPackets && same_route(r, pick_route(q, c.ch));
    }
  }
  if (env) unsetenv(env);
  row(what, ok);
}
void expect(const char *what, const Call &c, bool fused, const char *env = nullptr) {
  expect(what, c, fused, [](RenderParams &) {}, env);
}
template <class F>
Call with(Call c, F f) {
  f(c);
  return c;
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NOLIM_PACKETS_UNFUSED", "IAMF_HIP_LPCM_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED",
                                  "IAMF_HIP_NO_WIDE4", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY"};
  for (const char *e : switches) unsetenv(e);
  char what[240];

  // ---- the number, the block, the sets ----
  static_assert(IAMF_HIP_ROUTE_NOLIM_PACKETS == 43 && IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED == 39 && IAMF_HIP_ROUTE_PACKETS_RAGGED == 37, "stable numbers");
  static_assert(sizeof(RenderParams) == 616 && offsetof(RenderParams, ragged) == 412, "the block keeps its size: the mark is a new VALUE of `ragged`");
  static_assert((int)Family::NolimPackets == (int)Family::PacketsMixRagged + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 11 + 1 && kRouteTables == 3, "set 11 behind the three tables; sets added later leave it alone");
  static_assert(kNlChunk == 1024 && kNlMaxFrameBytes == 60, "the tile");

  // ---- every instance: 18 rows, each fused into every PCM format ----
  int rows = 0;
  for_each_render_instance_nolim_packets([&](int f, int v, int m, int c, int k) {
    const bool mono = LpcmM::has(m), cpl = LpcmCoupledM::has(m);
    rows += (f == IAMF_HIP_ROUTE_NOLIM_PACKETS && v == 0 && c == 0 && (mono != cpl) && (k == 2 || k == 3)) ? 1 : 1000;
    for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_S32, IAMF_HIP_FMT_F32}) {
      snprintf(what, sizeof(what), "instance m = %d, %d-bit %s, stereo format %d: fused", m, 8 * k, cpl ? "coupled" : "mono-coded", fmt);
      // (stereo s24 is 6 bytes per sample-frame: no whole dwords, so that one is the f32 path's)
      expect(what, call(m, k, cpl, 1000, 1000, 0, 2, fmt), fmt != IAMF_HIP_FMT_S24);
    }
  });
  row("the family lists 18 rows", rows == 18);
  {
    row("set 11 of for_each_instance_of_set is the listing: 18 rows, family 43 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_NOLIM_PACKETS, 11, 18));
    row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
    row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  }

  const Call toa = call(16, 2, false), b714 = call(12, 3, true), b51 = call(6, 2, true), st = call(2, 2, true);

  // ---- one case per rule, flipped alone ----
  expect("3rd order 16 bit -> stereo f32, one frame of 1000: fused", toa, true);
  expect("7.1.4 coupled 24 bit -> stereo f32: fused", b714, true);
  expect("limiter on", with(toa, [](Call &c) { c.limiter_on = 1; }), false);
  expect("total = 6 (a trimmed frame of 6 samples)", with(toa, [](Call &c) { c.total = 6; }), false);
  expect("total = 8: fused", with(toa, [](Call &c) { c.total = 8; }), true);
  expect("total = 4, one quad: fused", with(toa, [](Call &c) { c.total = 4; }), true);
  expect("total = 0", toa, false, [](RenderParams &p) { p.total = 0; });
  expect("total = 1001 / 1002 / 1003", with(call(16, 2, false, 1004, 1001), [](Call &) {}), false);
  expect("                           ", call(16, 2, false, 1004, 1002), false);
  expect("                           ", call(16, 2, false, 1004, 1003), false);
  expect("frame size = 6 (lpcm_form_check refuses it; the rule does too)", toa, false, [](RenderParams &p) { p.frame_size = 6, p.total = 12; });
  expect("frame size = 2", toa, false, [](RenderParams &p) { p.frame_size = 2, p.total = 4; });
  expect("d_pcm off the 16-byte grid", with(toa, [](Call &c) { c.pcm += 8; }), false);
  expect("pcm_stream_stride off the 16-byte grid", with(toa, [](Call &c) { c.pcm_stream_stride += 8; }), false);
  expect("out_ch * bytes = 2 (mono s16)", call(16, 2, false, 1000, 1000, 0, 1, IAMF_HIP_FMT_S16), false);
  expect("out_ch * bytes = 4 (mono f32): fused", call(16, 2, false, 1000, 1000, 0, 1, IAMF_HIP_FMT_F32), true);
  expect("out_ch * bytes = 60 (15 x f32): fused", call(16, 2, false, 1000, 1000, 0, 15, IAMF_HIP_FMT_F32), true);
  expect("out_ch * bytes = 64 (16 x f32)", call(16, 2, false, 1000, 1000, 0, 16, IAMF_HIP_FMT_F32), false);
  expect("12 channels s16, 6 s32: fused", call(16, 2, false, 1000, 1000, 0, 12, IAMF_HIP_FMT_S16), true);
  expect("                            ", call(16, 2, false, 1000, 1000, 0, 6, IAMF_HIP_FMT_S32), true);
  expect("first 100, n = fs - first: fused", call(16, 2, false, 1000, 900, 100), true);
  expect("first 4 and 240: fused", call(16, 2, false, 1000, 996, 4), true);
  expect("                      ", call(16, 2, false, 1000, 760, 240), true);
  expect("first + n > fs", call(16, 2, false, 1000, 900, 100), false, [](RenderParams &p) { p.total = 904; });
  expect("first < 0", call(16, 2, false, 1000, 900, 100), false, [](RenderParams &p) { p.demix_i0 = -4; });
  expect("first > 0 with whole frames", toa, false, [](RenderParams &p) { p.demix_i0 = 4; });
  expect("first 2 on a 16-bit mono run: 4 bytes off the 8-byte grid", call(16, 2, false, 1000, 996, 2), false);
  expect("first 2 on a coupled 16-bit stereo pair: 8 bytes on, fused", call(2, 2, true, 1000, 996, 2), true);
  expect("first 1 on a coupled 16-bit stereo pair: off the grid", call(2, 2, true, 1000, 996, 1), false);
  expect("first 2 on a coupled 24-bit stereo pair: 12 bytes on, fused", call(2, 3, true, 1000, 996, 2), true);
  expect("first 2 on 5.1 coupled 16 bit: C and LFE off the grid", call(6, 2, true, 1000, 996, 2), false);
  expect("a 16-bit run off the 8-byte grid", with(toa, [](Call &c) { c.L.src_offset[5] += 4; }), false);
  expect("a 24-bit run off the dword grid", with(call(16, 3, false), [](Call &c) { c.L.src_offset[5] += 2; }), false);
  expect("raw_frame_stride off the grid", with(toa, [](Call &c) { c.raw_frame_stride += 4; }), false);
  expect("raw_stream_stride off the grid", with(toa, [](Call &c) { c.raw_stream_stride += 4; }), false);
  expect("d_raw off the 16-byte grid", with(toa, [](Call &c) { c.raw += 8; }), false);
  expect("big-endian", with(toa, [](Call &c) { c.L.little_endian = 0; }), false);
  expect("32 bit", call(16, 4, false), false);
  expect("mono-coded 5.1, 16 bit (six runs of step 2)", call(6, 2, false), false);
  expect("mono-coded 5.1, 24 bit (the form S24, no instance for six runs)", call(6, 3, false), false);
  expect("5.1 coupled 16 / 24 bit: fused", b51, true);
  expect("                        ", call(6, 3, true), true);
  expect("coupled stereo 16 bit: fused", st, true);
  expect("a channel no sub-stream carries", with(toa, [](Call &c) { c.L.src_offset[3] = -1; }), false);
  expect("a pair's partner elsewhere", with(b51, [](Call &c) { c.L.src_offset[1] += 4; }), false);
  expect("m = 3: no form's list", call(3, 2, false), false);
  expect("the mark of another entry (2)", toa, false, [](RenderParams &p) { p.ragged = 2; });
  expect("no mark", toa, false, [](RenderParams &p) { p.ragged = 0; });
  expect("lpcm_coupled names the other sample size's form", b51, false, [](RenderParams &p) { p.lpcm_coupled = 2; });
  expect("lpcm_bytes 0", toa, false, [](RenderParams &p) { p.lpcm_bytes = 0; });
  // the plain kind: every stage and flag that keeps the f32 limiter-less kernel away
  expect("a second element", toa, false, [](RenderParams &p) { p.in2 = p.in, p.m2 = 2; });
  expect("both elements as packets", toa, false, [](RenderParams &p) { p.lpcm_mix = 1; });
  expect("element ramp", toa, false, [](RenderParams &p) { p.elem_ramp = reinterpret_cast<const float *>(0x20000); });
  expect("output ramp", toa, false, [](RenderParams &p) { p.out_ramp = reinterpret_cast<const float *>(0x20000); });
  expect("down-mixer", toa, false, [](RenderParams &p) { p.dmx_on = 1; });
  expect("demixer", toa, false, [](RenderParams &p) { p.demix_on = 1; });
  expect("pre-matrix", toa, false, [](RenderParams &p) { p.pre_matrix = reinterpret_cast<const float *>(0x20000); });
  expect("HRTF stage", toa, false, [](RenderParams &p) { p.fir_taps = 256; });
  expect("LFE generator", toa, false, [](RenderParams &p) { p.lfe = reinterpret_cast<const float *>(0x20000); });
  expect("reduced out_gain_channels", with(toa, [](Call &c) { c.og_ch = 1; }), false);
  expect("a flush (no input)", toa, false, [](RenderParams &p) { p.in = nullptr; });
  // the switches
  expect("IAMF_HIP_NOLIM_PACKETS_UNFUSED", toa, false, "IAMF_HIP_NOLIM_PACKETS_UNFUSED");
  expect("IAMF_HIP_LPCM_UNFUSED", toa, false, "IAMF_HIP_LPCM_UNFUSED");
  expect("IAMF_HIP_FORCE_GENERIC", toa, false, "IAMF_HIP_FORCE_GENERIC");
  expect("IAMF_HIP_PACKETS_RAGGED_UNFUSED says nothing here: fused", toa, true, "IAMF_HIP_PACKETS_RAGGED_UNFUSED");
  // lengths: whole frames, chunk boundaries
  for (int n : {4, 8, 1020, 1024, 1028, 2044})
    expect("frame size 2048, a trimmed call of 4 .. 2044: fused", call(9, 3, false, 2048, n), true);
  expect("three / eleven frames of 100: fused", call(4, 2, false, 100, 300), true);
  expect("                                   ", call(4, 2, false, 100, 1100), true);
  // a far call: 64-bit addressing, no bound on the extent
  expect("a frame stride of 2^30 bytes, 64 frames: fused", with(toa, [](Call &c) { c.raw_frame_stride = (int64_t)1 << 30, c.raw_stream_stride = (int64_t)1 << 37, c.total = 64000; }), true);

  // ---- the mark changes no other call's route: a limiter-on block routes the same with ragged 4 and 0, whatever the shape ----
  int same = 0, all = 0;
  for_each_render_instance_nolim_packets([&](int, int, int m, int, int k) {
    for (int total : {1000, 1024, 64}) {
      RenderParams p;
      if (!block_of(with(call(m, k, LpcmCoupledM::has(m), total, total, 0, 2, IAMF_HIP_FMT_S16), [](Call &c) { c.limiter_on = 1; }), p)) continue;
      p.pos0 = 1024;
      RenderParams q = p;
      q.ragged = 0;
      ++all;
      same += same_route(pick_route(p, m), pick_route(q, m)) ? 1 : 0;
    }
  });
  row("limiter-on blocks route as without the mark", all == 54 && same == all);

  printf("%d cases, %d wrong\n%s\n", g_cases, g_failed, g_failed ? "FAILED" : "OK");
  return g_failed ? 1 : 0;
}
