// Host-only check of the ragged packet form: its routing (pick_route() in iac_amd/csrc/render_route.hpp, Family::PacketsRagged,
// reached through the value 2 of the host-only field RenderParams::ragged, which iamf_hip_batch_render_packets_ragged alone sets).
// One row per clause of packets_ragged_shape_ok, with one field changed and nothing else: the form's kernel on the near side,
// on the far side exactly what the same RenderParams get with ragged == 0 — what iamf_hip_batch_render_packets is given, and
// what render_prepare answers with the unpacker.  render_fast_kernel<.., LP, .., RAG = true> loads a lane's four samples as 8,
// 12, 16 or 2 x 12 bytes at 32-bit offsets and trusts the host that a quad which starts inside a call ends inside its run: a
// wrong row here is a misaligned or stray load on the GPU, not a slower rate.
// Driven by tests/test_packets_ragged_cpu.py.
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
  printf("%-118s %s\n", what, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

uint8_t *const kRaw = reinterpret_cast<uint8_t *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kRamp = reinterpret_cast<float *>(0x20000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);

// the four forms: bytes per sample, coupled
struct Form {
  const char *name;
  int bytes, coupled;   // coupled: RenderParams::lpcm_coupled (0, 1 with 16-bit samples, 2 with 24-bit ones)
};
const Form kForms[4] = {{"16-bit mono-coded", 2, 0}, {"16-bit coupled", 2, 1}, {"24-bit mono-coded", 3, 0}, {"24-bit coupled", 3, 2}};

// a live service: one frame of `total` samples per call (frame size = total rounded up to 4 unless given), m channels as
// packets of form f laid out as lpcm_util.rows does (a head of 16 bytes, the runs one behind the other), first_sample `first`
RenderParams call(const Form &f, int m, int out_ch, int total = 1000, int64_t pos0 = 1000, int frame_size = 0, int first = 0) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = frame_size ? frame_size : (total + 3) & ~3;
  p.total = total;
  p.pos0 = pos0;
  p.lpcm = kRaw;
  p.in = reinterpret_cast<const float *>(kRaw);   // the placeholder render_lpcm_range_impl sets: "not a flush"
  p.lpcm_bytes = f.bytes;
  p.lpcm_coupled = f.coupled;
  int off = 16;
  for (int c = 0; c < m; ++c) {
    const bool paired = f.coupled && lpcm_coupled_paired(m, c);
    const int step = paired ? 2 * f.bytes : f.bytes;
    if (paired && (c & 1)) {
      p.lpcm_off[c] = p.lpcm_off[c - 1] + f.bytes;
      off += 2 * f.bytes * p.frame_size;
    } else {
      p.lpcm_off[c] = off + step * first;
      if (!paired) off += f.bytes * p.frame_size;
    }
    off = paired && !(c & 1) ? off : (off + 7) & ~7;
  }
  p.lpcm_frame_stride = (off + 15) & ~15;
  p.lpcm_stream_stride = p.lpcm_frame_stride * (total / p.frame_size + 1);
  p.demix_i0 = first;
  p.pcm = kPcm;
  p.out_ch = p.og_ch = out_ch;
  p.out_format = IAMF_HIP_FMT_S16;
  p.pcm_stream_stride = (((int64_t)total * out_ch * 4) + 15) & ~(int64_t)15;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 48;
  p.n_end = 9649;
  p.ragged = 2;
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

// fused: the form's family, a row of set 9 and of no other set.  Else: exactly what the same call gets with the mark at 0 —
// what iamf_hip_batch_render_packets is given —, which must be `fallback` (what the parent commit gives the call: a ragged
// packet call is refused, and render_prepare unpacks it).
void expect(const char *what, const RenderParams &p, int m, const char *env, bool fused, Family fallback = Family::Refused) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  RenderParams q = p;
  q.ragged = 0;
  const Route r0 = pick_route(q, m);
  if (env) unsetenv(env);
  bool ok = r0.family == fallback;
  if (fused) {
    const RouteKey k = route_key(r, p, m);
    ok = ok && r.family == Family::PacketsRagged && r.variant == 0 && r.err == IAMF_HIP_OK && k.set == 9 && sets_of(k) == 1 << 9 &&
         k.family == IAMF_HIP_ROUTE_PACKETS_RAGGED && k.variant == 0 && k.m == m && k.c == p.out_ch && k.k == (p.lpcm_bytes == 3 ? 3 : 2);
  } else {
    ok = ok && same_route(r, r0);
  }
  row(what, ok);
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_RAGGED_UNFUSED", "IAMF_HIP_INTERLEAVED_UNFUSED",
                                  "IAMF_HIP_PACKETS_RAGGED_UNFUSED", "IAMF_HIP_LP_LATE", "IAMF_HIP_LP_EARLY", "IAMF_HIP_LPCM_UNFUSED"};
  for (const char *e : switches) unsetenv(e);
  char what[240];
  const Form &S16 = kForms[0], &S16C = kForms[1], &S24 = kForms[2], &S24C = kForms[3];

  // ---- the number, the block, the sets ----
  static_assert(IAMF_HIP_ROUTE_PACKETS_RAGGED == 37, "stable number");
  static_assert(IAMF_HIP_ROUTE_LPCM24_MIX == 33 && IAMF_HIP_ROUTE_LPCM24_COUPLED == 31 && IAMF_HIP_ROUTE_FAST_RAGGED == 29 &&
                    IAMF_HIP_ROUTE_FAST_INTERLEAVED == 27 && IAMF_HIP_ROUTE_LPCM_MIX == 25,
                "the numbers in use keep their values");
  static_assert(sizeof(RenderParams) == 616, "the block keeps its size");
  static_assert(offsetof(RenderParams, ragged) == 412 && offsetof(RenderParams, lfe_div) == 416 && offsetof(RenderParams, lpcm) == 528 &&
                    offsetof(RenderParams, lpcm_off) == 552 && offsetof(RenderParams, interleaved) == 380,
                "every field keeps its offset: the mark is a new VALUE of `ragged`, the first sample travels in demix_i0");
  static_assert(sizeof(RenderMixParams) == 616 + 8 + 16 + 16, "the mixing block behind it too");
  static_assert((int)Family::PacketsRagged == (int)Family::Lpcm24Mix + 1, "added at the end of the enum");
  static_assert(kRouteSets >= 9 + 1 && kRouteTables == 3, "set 9 behind the three tables; sets added later leave it alone");
  static_assert(packets_ragged_wgs(16, 2, 3, false) >= 2 && packets_ragged_wgs(16, 2, 3, false) <= 4, "workgroups per CU");

  // ---- every instance ----
  int rows = 0;
  for_each_render_instance_packets_ragged([&](int f, int v, int m, int oc, int k) {
    const bool mono = LpcmM::has(m), cpl = LpcmCoupledM::has(m);
    rows += (f == IAMF_HIP_ROUTE_PACKETS_RAGGED && v == 0 && (mono != cpl) && LpcmOC::has(oc) && (k == 2 || k == 3)) ? 1 : 1000;
    const Form &form = kForms[(k == 3 ? 2 : 0) + (cpl ? 1 : 0)];
    snprintf(what, sizeof(what), "%s, %d channel(s) into %d, one frame of 1000: PacketsRagged", form.name, m, oc);
    expect(what, call(form, m, oc), m, nullptr, true);
  });
  row("the family's listing: ({1, 4, 9, 16} + {2, 6, 8, 10, 12}) x {1, 2} x {2, 3 bytes} = 36 rows of family 37", rows == 36);
  {
    bool only9 = true;
    int n9 = 0;
    for_each_instance_of_set(9, [&](int f, int v, int m, int c, int k) {
      ++n9;
      only9 = only9 && sets_of(RouteKey{f, v, m, c, k}) == 1 << 9;
    });
    row("every key of set 9 is in that set only", only9 && n9 == 36);
    row("set 9 of for_each_instance_of_set is the listing: 36 rows, family 37 alone, which no other set lists", family_in_one_set(IAMF_HIP_ROUTE_PACKETS_RAGGED, 9, 36));
    row("no row for a set number outside the listing (-1, kRouteSets)", no_rows_outside());
    row("every set keeps its row count and its family (sets 0 .. 12)", pinned_sets_ok());
  }
  row("packets_ragged_fused: every size up to 65536", [&] {
    for (int n = 1; n <= 65536; ++n)
      if (!packets_ragged_fused(n)) return false;
    return true;
  }());

  // ---- lengths ----
  for (const Form &f : kForms) {
    const int m = f.coupled ? 6 : 16;
    for (int total : {1, 3, 63, 65, 100, 120, 240, 480, 1000, 1001, 1002, 1003, 1023, 1025}) {
      snprintf(what, sizeof(what), "  %s: %d samples in one frame of 2048: fused", f.name, total);
      expect(what, call(f, m, 2, total, 1000, 2048), m, nullptr, true);
    }
    snprintf(what, sizeof(what), "  %s: 3 frames of 100 (a chunk spans frames): fused", f.name);
    expect(what, call(f, m, 2, 300, 300, 100), m, nullptr, true);
    snprintf(what, sizeof(what), "  %s: 5 frames of 1000: fused", f.name);
    expect(what, call(f, m, 2, 5000, 5000, 1000), m, nullptr, true);
  }
  const Family wholes[4] = {Family::Lpcm, Family::LpcmCoupled, Family::Lpcm24, Family::Lpcm24Coupled};
  for (int i = 0; i < 4; ++i) {
    const int m = kForms[i].coupled ? 6 : 16;
    for (int total : {64, 1024, 4096}) {
      snprintf(what, sizeof(what), "  %s: %d samples, whole blocks, the mark set: the whole-block family, as without the mark", kForms[i].name, total);
      expect(what, call(kForms[i], m, 2, total, 1024), m, nullptr, false, wholes[i]);
    }
    snprintf(what, sizeof(what), "  %s: 8 frames of 1000 = 125 blocks: the whole-block family", kForms[i].name);
    expect(what, call(kForms[i], m, 2, 8000, 8000, 1000), m, nullptr, false, wholes[i]);
  }
  expect("  0 samples", call(S16, 4, 2, 0, 1000, 1024), 4, nullptr, false, Family::Lpcm);

  // ---- positions ----
  const struct {
    int64_t pos;
    bool fused;
  } positions[] = {{0, true}, {16, true}, {100, false}, {239, false}, {240, true}, {241, true}, {1100, true}, {((int64_t)1 << 31) + 1, true}};
  for (const auto &c : positions) {
    snprintf(what, sizeof(what), "  position %lld: %s", (long long)c.pos, c.fused ? "fused" : "refused (unpacked, the general kernel)");
    expect(what, call(S16C, 2, 2, 1000, c.pos), 2, nullptr, c.fused);
  }

  // ---- each form's grid ----
  for (const Form &f : kForms) {
    const int m = f.coupled ? 6 : 4, g = f.bytes == 2 ? 8 : 4;
    const RenderParams pf = call(f, m, 2);
    snprintf(what, sizeof(what), "  %s: frame stride + %d B (on the form's grid)", f.name, g);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_frame_stride += g; }), m, nullptr, true);
    snprintf(what, sizeof(what), "  %s: frame stride + %d B (off it)", f.name, g / 2);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_frame_stride += g / 2; }), m, nullptr, false);
    snprintf(what, sizeof(what), "  %s: stream stride + %d B (on the grid)", f.name, g);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_stream_stride += g; }), m, nullptr, true);
    snprintf(what, sizeof(what), "  %s: stream stride + %d B (off it)", f.name, g / 2);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_stream_stride += g / 2; }), m, nullptr, false);
    snprintf(what, sizeof(what), "  %s: the mono run of channel 2 + %d B (on the grid)", f.name, g);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_off[2] += g; }), m, nullptr, true);
    snprintf(what, sizeof(what), "  %s: the mono run of channel 2 + %d B (off it)", f.name, g / 2);
    expect(what, with(pf, [&](RenderParams &p) { p.lpcm_off[2] += g / 2; }), m, nullptr, false);
    if (f.coupled) {
      snprintf(what, sizeof(what), "  %s: the pair (4, 5) + %d B (on the grid)", f.name, g);
      expect(what, with(pf, [&](RenderParams &p) { p.lpcm_off[4] += g, p.lpcm_off[5] += g; }), m, nullptr, true);
      snprintf(what, sizeof(what), "  %s: the pair (4, 5) + %d B (off it)", f.name, g / 2);
      expect(what, with(pf, [&](RenderParams &p) { p.lpcm_off[4] += g / 2, p.lpcm_off[5] += g / 2; }), m, nullptr, false);
      snprintf(what, sizeof(what), "  %s: the partner of channel 0 not %d bytes behind it", f.name, f.bytes);
      expect(what, with(pf, [&](RenderParams &p) { p.lpcm_off[1] += g; }), m, nullptr, false);
    }
    snprintf(what, sizeof(what), "  %s: packets + 8 B (d_raw off the 16-byte rule)", f.name);
    expect(what, with(pf, [](RenderParams &p) { p.lpcm += 8, p.in += 2; }), m, nullptr, false);
    snprintf(what, sizeof(what), "  %s: packets + 16 B", f.name);
    expect(what, with(pf, [](RenderParams &p) { p.lpcm += 16, p.in += 4; }), m, nullptr, true);
    // a channel count of the other coding
    snprintf(what, sizeof(what), "  %s: a channel count of the other coding", f.name);
    expect(what, call(f, f.coupled ? 4 : 6, 2), f.coupled ? 4 : 6, nullptr, false);
  }
  expect("  sample bytes 3 with the 16-bit coupling (lpcm_coupled == 1): no form", with(call(S24C, 6, 2), [](RenderParams &p) { p.lpcm_coupled = 1; }), 6, nullptr,
         false);
  expect("  sample bytes 2 with the 24-bit coupling (lpcm_coupled == 2): no form", with(call(S16C, 6, 2), [](RenderParams &p) { p.lpcm_coupled = 2; }), 6, nullptr,
         false);
  expect("  sample bytes 4: no form", with(call(S16, 4, 2), [](RenderParams &p) { p.lpcm_bytes = 4; }), 4, nullptr, false);
  expect("  sample bytes 0 (16 bit, as the older entries leave it): fused", with(call(S16, 4, 2), [](RenderParams &p) { p.lpcm_bytes = 0; }), 4, nullptr, true);
  expect("  M = 14", call(S16, 14, 2), 14, nullptr, false);
  expect("  M = 24", call(S24, 24, 2), 24, nullptr, false);

  // ---- the first_sample rule, both sides of its bound: first + ((n + 3) & ~3) <= frame_size ----
  for (const Form &f : kForms) {
    const int m = f.coupled ? 6 : 4;
    for (int first : {4, 100, 240}) {
      snprintf(what, sizeof(what), "  %s: first_sample %d, the rest of a frame of 1000: fused", f.name, first);
      expect(what, call(f, m, 2, 1000 - first, 0, 1000, first), m, nullptr, true);
    }
    // n = 997 .. 999 from first 4 of a frame of 1004: the last quad ends at 4 + 1000 = 1004 — on the bound
    snprintf(what, sizeof(what), "  %s: first 4, 997 samples of 1004: the last quad ends with the run: fused", f.name);
    expect(what, call(f, m, 2, 997, 0, 1004, 4), m, nullptr, true);
    snprintf(what, sizeof(what), "  %s: first 8, 997 samples of 1004: the last quad would end 4 samples behind the run", f.name);
    expect(what, call(f, m, 2, 997, 0, 1004, 8), m, nullptr, false);
  }
  // a coupled pair's run is on its grid from every even first sample (16 bit: lpcm_form_coupled, 4 * first on 8; 24 bit: 6 *
  // first on 4); the mono runs C and LFE only from every fourth — stereo has none
  for (const Form *f : {&S16C, &S24C}) {
    snprintf(what, sizeof(what), "  %s, stereo: first 2, 996 samples of 1000 (2 + 996 <= 1000): fused", f->name);
    expect(what, call(*f, 2, 2, 996, 0, 1000, 2), 2, nullptr, true);
    snprintf(what, sizeof(what), "  %s, stereo: first 2, 997 samples of 1000 (2 + 1000 > 1000): unpacked", f->name);
    expect(what, call(*f, 2, 2, 997, 0, 1000, 2), 2, nullptr, false);
    snprintf(what, sizeof(what), "  %s, stereo: first 2, 998 samples of 1000, the whole rest of the frame (2 + 1000 > 1000): unpacked", f->name);
    expect(what, call(*f, 2, 2, 998, 0, 1000, 2), 2, nullptr, false);
    snprintf(what, sizeof(what), "  %s, stereo: first 2, 999 samples of 1001 rounded to 1004: fused", f->name);
    expect(what, call(*f, 2, 2, 999, 0, 1004, 2), 2, nullptr, true);
  }
  expect("  16-bit coupled stereo: first 2, 995 samples of 1000 (2 + 996 <= 1000): fused", call(S16C, 2, 2, 995, 0, 1000, 2), 2, nullptr, true);
  expect("  16-bit coupled stereo: first 6, 995 samples of 1000 (6 + 996 > 1000): unpacked", call(S16C, 2, 2, 995, 0, 1000, 6), 2, nullptr, false);
  expect("  24-bit coupled stereo: first 6, 994 samples of 1000 (6 + 996 > 1000): unpacked", call(S24C, 2, 2, 994, 0, 1000, 6), 2, nullptr, false);
  expect("  24-bit coupled stereo: first 6, 993 samples of 1000 (6 + 996 > 1000): unpacked", call(S24C, 2, 2, 993, 0, 1000, 6), 2, nullptr, false);
  expect("  24-bit coupled stereo: first 6, 992 samples of 1000: whole blocks? no, 992 = 15.5 blocks; 6 + 992 <= 1000: fused",
         call(S24C, 2, 2, 992, 0, 1000, 6), 2, nullptr, true);
  expect("  a first sample with whole frames (no trimmed frame has it): not taken", with(call(S16, 4, 2), [](RenderParams &p) { p.demix_i0 = 4; }), 4,
         nullptr, false);
  expect("  a negative first sample", with(call(S16, 4, 2, 500, 0, 1000), [](RenderParams &p) { p.demix_i0 = -4; }), 4, nullptr, false);

  // ---- one field changed at a time ----
  const RenderParams ps = call(S24, 16, 2);
  expect("  ragged = 0: as iamf_hip_batch_render_packets", with(ps, [](RenderParams &p) { p.ragged = 0; }), 16, nullptr, false);
  expect("  ragged = 1 (the f32 entry's mark) with packets: refused as before", with(ps, [](RenderParams &p) { p.ragged = 1; }), 16, nullptr, false);
  expect("  limiter off", with(ps, [](RenderParams &p) { p.limiter_on = 0; }), 16, nullptr, false);
  expect("  3 output channels", call(S24, 16, 3), 16, nullptr, false);
  expect("  6 output channels", call(S24, 16, 6), 16, nullptr, false);
  expect("  output gain on fewer channels than rendered", with(ps, [](RenderParams &p) { p.og_ch = 1; }), 16, nullptr, false);
  expect("  a limiter table shorter than the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin - 1; }), 16, nullptr, false);
  expect("  a limiter table of exactly the staged window", with(ps, [](RenderParams &p) { p.n_end = kFWin; }), 16, nullptr, true);
  expect("  a second element (f32)", with(ps, [](RenderParams &p) { p.in2 = kRamp, p.m2 = 2, p.in2_frame_stride = 2000, p.in2_stream_stride = 4000; }), 16,
         nullptr, false);
  expect("  a second element as packets (lpcm_mix)", with(ps, [](RenderParams &p) { p.lpcm_mix = 5, p.in2 = kRamp, p.m2 = 1; }), 16, nullptr, false);
  expect("  an element ramp", with(ps, [](RenderParams &p) { p.elem_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16, nullptr, false);
  expect("  a ramp for a second element", with(ps, [](RenderParams &p) { p.elem2_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16, nullptr, false);
  expect("  an output ramp", with(ps, [](RenderParams &p) { p.out_ramp = kRamp, p.ramp_stream_stride = 4096; }), 16, nullptr, false);
  expect("  down-mixer", with(call(S24C, 8, 2), [](RenderParams &p) { p.dmx_on = 1; }), 8, nullptr, false);
  expect("  demixer", with(ps, [](RenderParams &p) { p.demix_on = 1; }), 16, nullptr, false);
  expect("  de-mapping matrix", with(ps, [](RenderParams &p) { p.pre_matrix = kRamp; }), 16, nullptr, false);
  expect("  HRTF stage", with(ps, [](RenderParams &p) { p.fir_taps = 256; }), 16, nullptr, false);
  expect("  LFE generator", with(ps, [](RenderParams &p) { p.lfe = kRamp; }), 16, nullptr, false);
  expect("  no packets (planar f32 with the mark): the general kernel", with(ps, [](RenderParams &p) { p.lpcm = nullptr; }), 16, nullptr, false, Family::Generic);
  expect("  flush (no input)", with(ps, [](RenderParams &p) { p.in = nullptr; }), 16, nullptr, false);
  expect("  frame size 1002 (1001 samples)", call(S24, 16, 2, 1001, 1000, 1002), 16, nullptr, false);
  expect("  frame size 1001 (1001 samples)", call(S24, 16, 2, 1001, 1000, 1001), 16, nullptr, false);
  expect("  frame size 1004 (1001 samples)", call(S24, 16, 2, 1001, 1000, 1004), 16, nullptr, true);
  expect("  pcm + 2 B", with(ps, [](RenderParams &p) { p.pcm += 2; }), 16, nullptr, false);
  expect("  pcm + 16 B", with(ps, [](RenderParams &p) { p.pcm += 16; }), 16, nullptr, true);
  expect("  pcm stream stride + 4 B", with(ps, [](RenderParams &p) { p.pcm_stream_stride += 4; }), 16, nullptr, false);
  expect("  pcm stream stride + 16 B", with(ps, [](RenderParams &p) { p.pcm_stream_stride += 16; }), 16, nullptr, true);
  for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_S32, IAMF_HIP_FMT_F32}) {
    snprintf(what, sizeof(what), "  PCM format %d: fused", fmt);
    expect(what, with(ps, [&](RenderParams &p) { p.out_format = fmt; }), 16, nullptr, true);
  }
  {
    // fast_shape_ok's 32-bit bound on the packets: (total / frame_size + 2) * lpcm_frame_stride + 2^24 < 2^31, here 3 frames'
    // worth for one frame of 1000
    const int64_t lim = (((int64_t)1 << 31) - ((int64_t)1 << 24)) / 3;
    const int64_t at = (lim - 1) & ~(int64_t)15;
    const int64_t beyond = (lim + 16) & ~(int64_t)15;
    const auto ok = [](int64_t fst) { return 3 * fst + ((int64_t)1 << 24) < ((int64_t)1 << 31); };
    row("  the 32-bit bound's two test strides lie either side of it", ok(at) && !ok(beyond) && beyond - at <= 32);
    for (const Form &f : kForms) {
      const int m = f.coupled ? 6 : 4;
      snprintf(what, sizeof(what), "  %s: frame stride at the 32-bit bound", f.name);
      expect(what, with(call(f, m, 2), [&](RenderParams &p) { p.lpcm_frame_stride = at; }), m, nullptr, true);
      snprintf(what, sizeof(what), "  %s: frame stride beyond the 32-bit bound", f.name);
      expect(what, with(call(f, m, 2), [&](RenderParams &p) { p.lpcm_frame_stride = beyond; }), m, nullptr, false);
    }
  }
  expect("  n_launch = 65536", with(ps, [](RenderParams &p) { p.n_launch = p.n_streams = 65536; }), 16, nullptr, true);

  // ---- the switches ----
  expect("  IAMF_HIP_FORCE_GENERIC", ps, 16, "IAMF_HIP_FORCE_GENERIC", false);
  expect("  IAMF_HIP_PACKETS_RAGGED_UNFUSED", ps, 16, "IAMF_HIP_PACKETS_RAGGED_UNFUSED", false);
  expect("  IAMF_HIP_RAGGED_UNFUSED does not reach the form", ps, 16, "IAMF_HIP_RAGGED_UNFUSED", true);
  expect("  IAMF_HIP_LP_LATE does nothing to this family", ps, 16, "IAMF_HIP_LP_LATE", true);
  expect("  IAMF_HIP_LP_EARLY does nothing to this family", ps, 16, "IAMF_HIP_LP_EARLY", true);
  expect("  IAMF_HIP_LP_LATE, 16-bit mono-coded, 4096 streams", with(call(S16, 16, 2), [](RenderParams &p) { p.n_launch = p.n_streams = 4096; }), 16,
         "IAMF_HIP_LP_LATE", true);

  // ---- an unmarked call routes exactly as before: whole blocks and ragged, every form, with and without the new switch ----
  for (int i = 0; i < 4; ++i) {
    const int m = kForms[i].coupled ? 6 : 4;
    for (int total : {4096, 1000}) {
      RenderParams p = call(kForms[i], m, 2, total, 0, total == 4096 ? 1024 : 1000);
      p.ragged = 0;
      const Route a = pick_route(p, m);
      setenv("IAMF_HIP_PACKETS_RAGGED_UNFUSED", "1", 1);
      const Route b = pick_route(p, m);
      unsetenv("IAMF_HIP_PACKETS_RAGGED_UNFUSED");
      snprintf(what, sizeof(what), "ragged = 0, %s, %d samples: %s, whatever the switch says", kForms[i].name, total,
               total == 4096 ? "the whole-block family" : "refused");
      row(what, a.family == (total == 4096 ? wholes[i] : Family::Refused) && same_route(a, b) &&
                    (total == 4096 || a.err == IAMF_HIP_ERR_INVALID_STATE));
    }
  }
  {
    // planar f32 through the f32 entries: the mark's value 2 names no planar form
    RenderParams p;
    memset(&p, 0, sizeof(p));
    p.frame_size = p.total = 1000, p.pos0 = 1000, p.in = kRamp, p.in_frame_stride = 4000, p.in_stream_stride = 8000, p.pcm = kPcm, p.out_ch = p.og_ch = 2;
    p.pcm_stream_stride = 4000, p.n_streams = p.n_launch = 64, p.limiter_on = 1, p.n_atk = 48, p.n_end = 9649, p.ragged = 1;
    row("planar f32, ragged = 1: FastRagged as before", pick_route(p, 4).family == Family::FastRagged);
  }

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
