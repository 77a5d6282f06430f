// Host-only check of the render dispatch (iac_amd/csrc/render_route.hpp): a table of parameter blocks against the kernel
// family, variant and return code pick_route() must give, and the instance-list helper.  Every kernel is exact, so a
// wrong route shows in no parity test, only as a slower rate: this table is what pins it.  The expectations were read
// from launch() as it stood before the decision was gathered in pick_route().  Driven by tests/test_route_host.py.
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

const char *family_name(Family f) {
  static const char *const names[] = {"Refused", "Lpcm",      "FirSplit", "FirFused", "FastDown", "Wide4Lfe", "Wide4",
                                      "Wide4Demix", "Wide4Down", "Wide4Mix", "Nolim",    "Fast",     "Wide",     "Generic"};
  return names[(int)f];
}

float *const kIn = reinterpret_cast<float *>(0x10000);       // never dereferenced: routing looks at alignment only
float *const kIn2 = reinterpret_cast<float *>(0x20000);
float *const kTab = reinterpret_cast<float *>(0x30000);
uint8_t *const kPcm = reinterpret_cast<uint8_t *>(0x40000);
const iamf_hip_dmx_frame *const kDmxFrames = reinterpret_cast<const iamf_hip_dmx_frame *>(0x50000);

// "aligned": limiter on, 16-byte-aligned pointers, strides that are multiples of 4 floats / 16 bytes, total % 64 == 0,
// pos0 % 16 == 0, n_end large enough (the 48 kHz table: 9651); four whole 1024-sample frames of 64 streams
RenderParams aligned(int m, int out_ch, int fmt = IAMF_HIP_FMT_S16) {
  RenderParams p;
  memset(&p, 0, sizeof(p));
  p.frame_size = 1024;
  p.total = 4096;
  p.in = kIn;
  p.in_frame_stride = (int64_t)m * p.frame_size;
  p.in_stream_stride = 4 * p.in_frame_stride;
  p.pcm = kPcm;
  p.out_ch = p.og_ch = out_ch;
  p.out_format = fmt;
  p.pcm_stream_stride = (int64_t)(p.total + 1024) * out_ch * 4;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 241;
  p.n_end = 9651;
  return p;
}
void set_total(RenderParams &p, int total) { p.total = total; }
void second_element(RenderParams &p) {
  p.in2 = kIn2;
  p.m2 = 2;
  p.in2_frame_stride = 2 * p.frame_size;
  p.in2_stream_stride = 4 * p.in2_frame_stride;
}
void down_mixer(RenderParams &p) {
  p.dmx_on = 1;
  p.dmx_frames = kDmxFrames;
}
void demixer(RenderParams &p) {
  p.demix_on = 1;
  p.demix_w4 = 1;
}
void lfe(RenderParams &p) { p.lfe = kTab; }
void fir(RenderParams &p) {   // with the FFT stage's tables and the split form's scratch
  p.fir_taps = 256;
  p.fir_pq = p.fir_tw = p.fir_zero = p.fir_id_matrix = kTab;
  p.fir_y = kTab;
}
void lpcm(RenderParams &p) {
  p.lpcm = kPcm;
  p.lpcm_frame_stride = 16 * 2048;
  p.lpcm_stream_stride = 4 * p.lpcm_frame_stride;
}

int g_failed = 0, g_cases = 0;

// ---- the row sets behind the tally (for_each_instance_of_set; iamf_route.hip builds its tables from them) ----
// iamf_hip_route_count(set, ..) goes straight to the set it is given and searches no other, so every key (family, variant,
// m, c, k) must be in exactly one set and once within it, and route_key() must name that set (expect() asks for every route
// of the table below).  The per-form checks beside this file assert it for their own form against the others only.
struct ListedRow {
  int set, family, variant, m, c, k;
};
constexpr int kListedCap = 4096;
ListedRow g_listed[kListedCap];
int g_n_listed = -1;
int listed_rows() {
  if (g_n_listed >= 0) return g_n_listed;
  g_n_listed = 0;
  for (int s = 0; s < kRouteSets; ++s)
    for_each_instance_of_set(s, [&](int f, int v, int m, int c, int k) {
      if (g_n_listed < kListedCap) g_listed[g_n_listed] = ListedRow{s, f, v, m, c, k};
      ++g_n_listed;
    });
  return g_n_listed;
}
bool same_key(const ListedRow &a, int f, int v, int m, int c, int k) {
  return a.family == f && a.variant == v && a.m == m && a.c == c && a.k == k;
}
// the set that lists the key; -1: none, -2: more than one row
int set_listing(int f, int v, int m, int c, int k) {
  int set = -1;
  for (int i = 0; i < listed_rows() && i < kListedCap; ++i)
    if (same_key(g_listed[i], f, v, m, c, k)) set = set == -1 ? g_listed[i].set : -2;
  return set;
}
void set_checks() {
  const int n = listed_rows();
  int per_set[kRouteSets] = {0}, repeated = 0, outside = 0;
  for (int i = 0; i < n && i < kListedCap; ++i) {
    const ListedRow &r = g_listed[i];
    ++per_set[r.set];
    if (set_listing(r.family, r.variant, r.m, r.c, r.k) != r.set) ++repeated;
  }
  bool none_empty = true;
  for (int s = 0; s < kRouteSets; ++s) none_empty = none_empty && per_set[s] > 0;
  const int no_set[2] = {-1, kRouteSets};
  for (int s : no_set) for_each_instance_of_set(s, [&](int, int, int, int, int) { ++outside; });
  static_assert(kRouteTables == 3 && kRouteSets >= kRouteTables, "iamf_hip_route_tables() is pinned at three");
  const bool ok = n > 0 && n <= kListedCap && none_empty && repeated == 0 && outside == 0;
  printf("%-72s %d rows, %d repeated %s\n", "row sets: every key in exactly one set, once", n, repeated, ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

// env: one switch set to "1" for this case, or null
void expect(const char *what, RenderParams p, int m, const char *env, Family family, int variant, int err = IAMF_HIP_OK) {
  if (env) setenv(env, "1", 1);
  const Route r = pick_route(p, m);
  if (env) unsetenv(env);
  // a route that launches names an instance of the listing (iamf_hip_route_instances walks the same lists)
  bool listed = r.family == Family::Refused;
  const RouteKey k = route_key(r, p, m);
  for_each_render_instance([&](int f, int v, int km, int kc, int kk) {
    listed = listed || (f == k.family && v == k.variant && km == k.m && kc == k.c && kk == k.k);
  });
  // ... and counts in the set that lists it (iamf_hip_route_count goes by RouteKey::set alone)
  const bool own_set = r.family == Family::Refused || set_listing(k.family, k.variant, k.m, k.c, k.k) == k.set;
  const bool ok = r.family == family && r.variant == variant && r.err == err && listed && own_set;
  printf("%-72s %s/%d/%d %s\n", what, family_name(r.family), r.variant, r.err, ok ? "ok" : "WRONG");
  if (!ok) printf("    expected %s/%d/%d\n", family_name(family), variant, err);
  ++g_cases;
  g_failed += ok ? 0 : 1;
}
template <class F>
RenderParams with(RenderParams p, F f) {
  f(p);
  return p;
}

void list_checks() {
  static_assert(GenericM::has(11) && NolimM::has(11) && !FastM::has(11) && !WideM::has(11), "11 inputs: generic and nolim only");
  static_assert(Wide4DownMC::has(mc(12, 10)) && Wide4DownMC::has(mc(10, 8)) && Wide4DownMC::has(mc(8, 6)) &&
                    !Wide4DownMC::has(mc(10, 10)) && !Wide4DownMC::has(mc(8, 8)) && !Wide4DownMC::has(mc(6, 6)),
                "the down-mixer's pairs");
  static_assert(mc_m(mc(24, 24)) == 24 && mc_c(mc(24, 24)) == 24 && mc(1, 0) > mc(0, 24), "pairs of up to 24 channels do not collide");
  static_assert(!Wide4MixC::has(14) && Wide4C::has(14) && !Wide4DemixC::has(14), "14 channels: plain and LFE only");
  int got = 0, calls = 0;
  const bool hit = dispatch(FirHomeM{}, 9, [&](auto M) { got = M.value; ++calls; });
  const bool miss = dispatch(FirHomeM{}, 3, [&](auto) { ++calls; });
  int gm = 0, gc = 0;
  const bool nested = dispatch(Wide4M{}, 12, [&](auto M) { return dispatch(Wide4MixC{}, 10, [&](auto C) { gm = M.value; gc = C.value; }); });
  const bool nested_miss = dispatch(Wide4M{}, 12, [&](auto) { return dispatch(Wide4MixC{}, 14, [&](auto) { ++calls; }); });
  const bool ok = hit && got == 9 && !miss && calls == 1 && nested && gm == 12 && gc == 10 && !nested_miss;
  printf("%-72s %s\n", "dispatch: the matching constant once, false outside the list", ok ? "ok" : "WRONG");
  ++g_cases;
  g_failed += ok ? 0 : 1;
}

// ---- the packet layouts of tests/gpu_util.py (the PK_ table there), 16-bit packets ----
// tests/test_gpu_packet_layouts.py renders 3 streams of four 1024-sample frames in calls of 1 and 3 frames and expects, per
// layout, the packet-fed kernel or the unpacker in front of the f32 kernel.  Each row is the geometry of one of those calls:
// d_raw's residue, both strides, the frames; it asserts lpcm_form()'s answer and, where the form is admitted, pick_route()'s
// family.  A call that is not fused is unpacked into dense f32 rows, which the aligned stereo block's route renders.
void packet_layout_rows(const RenderParams &st) {
  constexpr int kCh = 16, kF = 4, kG = 8;
  constexpr int64_t kPkRow = 32912;   // lpcm_util.rows: 16 runs of 2048 bytes, head 8, pad 8, rounded up to 16
  constexpr int64_t k31 = (int64_t)1 << 31;
  constexpr int64_t kB3 = ((k31 - (1 << 24) - 1) / 5) & ~(int64_t)15;   // B(3): (3 + 2) * B + 2^24 < 2^31
  static_assert(kB3 == 426141280 && 5 * kB3 + (1 << 24) < k31 && 5 * (kB3 + 16) + (1 << 24) >= k31 && 3 * (kB3 + 16) + (1 << 24) < k31,
                "B(3)");
  iamf_hip_lpcm_layout L;
  memset(&L, 0, sizeof(L));
  L.sample_bytes = 2;
  L.little_endian = 1;
  L.channels = kCh;
  L.frame_size = 1024;
  for (int c = 0; c < kCh; ++c) {   // reversed channel order: no offset ascends
    L.src_offset[c] = 8 + (kCh - 1 - c) * (2048 + 8);
    L.src_step[c] = 2;
  }
  struct Pk {
    const char *name;
    int64_t off, fst, sst;
    bool fused[2];   // the call of 1 frame from frame 0, the call of 3 frames from frame 1
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
    for (int call = 0; call < 2; ++call) {
      const uintptr_t raw = 0x50000 + (uintptr_t)((r.off + f0s[call] * r.fst) & 15);
      const LpcmForm form = lpcm_form(L, kCh, r.sst, r.fst, raw, 0);
      RenderParams p = st;
      p.n_streams = p.n_launch = 3;
      p.pos0 = (int64_t)f0s[call] * 1024;
      p.total = nfs[call] * 1024;
      const Route f32 = pick_route(p, kCh);   // the unpacked call: dense f32 rows of the batch's own buffer
      p.lpcm = reinterpret_cast<const uint8_t *>(raw);
      p.lpcm_frame_stride = r.fst;
      p.lpcm_stream_stride = r.sst;
      p.lpcm_bytes = lpcm_form_bytes(form);
      const Route rt = form == LpcmForm::None ? Route{Family::Refused, 0, IAMF_HIP_ERR_INVALID_STATE} : pick_route(p, kCh);
      const bool fused = form == LpcmForm::S16 && rt.family == Family::Lpcm && rt.variant == 1;
      const bool form_ok = (form == LpcmForm::S16) == (r.fused[call] || !strcmp(r.name, "PK_BEYOND"));
      const bool ok = form_ok && form != LpcmForm::S24 && fused == r.fused[call] &&
                      (fused || rt.family == Family::Refused) && f32.family == Family::Fast && f32.variant == 0;
      char what[96];
      snprintf(what, sizeof(what), "%s, %d frame(s) from frame %d: %s", r.name, nfs[call], f0s[call],
               r.fused[call] ? "Lpcm, early" : "unpack + Fast");
      printf("%-72s form %d %s/%d/%d %s\n", what, (int)form, family_name(rt.family), rt.variant, rt.err, ok ? "ok" : "WRONG");
      ++g_cases;
      g_failed += ok ? 0 : 1;
    }
  }
}

// ---- the address rules: pointers, strides and the 32-bit bounds ----
// Each row is a block of the table above with exactly one field changed.  The vector kernels load 16 bytes at a time and
// keep 32-bit byte offsets, so these rules are all that stands between a legal call and a misaligned or wrapped access:
// the expectation of every row is the family as pick_route() gives it today.
template <class T>
T *bytes_on(T *ptr, int n) {
  return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(ptr) + n);
}
template <class F>
void one_change(const char *block, const char *change, const RenderParams &base, int m, F f, Family family, int variant,
                int err = IAMF_HIP_OK) {
  char what[96];
  snprintf(what, sizeof(what), "%s: %s", block, change);
  expect(what, with(base, f), m, nullptr, family, variant, err);
}
// the three rules of the first element's input
void input_rules(const char *block, const RenderParams &base, int m, Family family, int variant, int err = IAMF_HIP_OK) {
  one_change(block, "in + 4 B", base, m, [](RenderParams &p) { p.in = bytes_on(p.in, 4); }, family, variant, err);
  one_change(block, "in_stream_stride + 1", base, m, [](RenderParams &p) { p.in_stream_stride += 1; }, family, variant, err);
  one_change(block, "in_frame_stride + 2", base, m, [](RenderParams &p) { p.in_frame_stride += 2; }, family, variant, err);
}
void pcm_rules(const char *block, const RenderParams &base, int m, Family family, int variant) {
  one_change(block, "pcm + 2 B", base, m, [](RenderParams &p) { p.pcm = bytes_on(p.pcm, 2); }, family, variant);
  one_change(block, "pcm_stream_stride + 2", base, m, [](RenderParams &p) { p.pcm_stream_stride += 2; }, family, variant);
}
void second_rules(const char *block, const RenderParams &base, int m, Family family, int variant) {
  one_change(block, "in2 + 4 B", base, m, [](RenderParams &p) { p.in2 = bytes_on(p.in2, 4); }, family, variant);
  one_change(block, "in2_stream_stride + 1", base, m, [](RenderParams &p) { p.in2_stream_stride += 1; }, family, variant);
  one_change(block, "in2_frame_stride + 1", base, m, [](RenderParams &p) { p.in2_frame_stride += 1; }, family, variant);
}
void ramp_rules(const char *block, const RenderParams &base, int m, Family family, int variant) {
  one_change(block, "elem_ramp + 4 B", base, m, [](RenderParams &p) { p.elem_ramp = bytes_on(p.elem_ramp, 4); }, family, variant);
  one_change(block, "out_ramp + 4 B", base, m, [](RenderParams &p) { p.out_ramp = bytes_on(p.out_ramp, 4); }, family, variant);
  one_change(block, "ramp_stream_stride + 1", base, m, [](RenderParams &p) { p.ramp_stream_stride += 1; }, family, variant);
}

void address_rules(const RenderParams &st, const RenderParams &w, const RenderParams &nl, const RenderParams &f16,
                   const RenderParams &lp) {
  const int UNIMPL = IAMF_HIP_ERR_UNIMPLEMENTED;
  const RenderParams st_mix = with(st, second_element), w_mix = with(w, second_element);
  const RenderParams w24 = aligned(16, 12, IAMF_HIP_FMT_S24);
  // 11 channels (Sound System E): no wide4 layout.  render_wide_kernel loads its input as scalars, so wide_shape_ok looks
  // at the PCM only and an unaligned input keeps the kernel
  const RenderParams e11 = aligned(12, 11);
  expect("aligned, 11 channels, m = 12", e11, 12, nullptr, Family::Wide, 0);

  // ---- the first element's pointer and strides ----
  input_rules("stereo", st, 16, Family::Generic, 0);
  input_rules("limiter off", nl, 16, Family::Generic, 0);
  // (the fused LPCM kernel does not read `in`, but it is a call of the fast kernel's shape or none)
  input_rules("LPCM", lp, 16, Family::Refused, 0, IAMF_HIP_ERR_INVALID_STATE);
  input_rules("12 channels", w, 16, Family::Wide, 0);             // the scalar loads of render_wide_kernel take it
  input_rules("12 channels + second element", w_mix, 16, Family::Generic, 0);
  input_rules("FIR", f16, 16, Family::Refused, 0, UNIMPL);
  input_rules("11 channels", e11, 12, Family::Wide, 0);

  // ---- the PCM pointer and stride ----
  pcm_rules("stereo", st, 16, Family::Generic, 0);
  pcm_rules("12 channels, s24 (Wide)", w24, 16, Family::Generic, 0);
  pcm_rules("12 channels (Wide4)", w, 16, Family::Generic, 0);
  pcm_rules("limiter off", nl, 16, Family::Generic, 0);
  pcm_rules("11 channels", e11, 12, Family::Generic, 0);

  // ---- the second element ----
  expect("12 channels + second element, aligned", w_mix, 16, nullptr, Family::Wide4Mix, 0);
  second_rules("stereo + second element", st_mix, 16, Family::Generic, 0);
  second_rules("12 channels + second element", w_mix, 16, Family::Generic, 0);

  // ---- the ramps ----
  const auto ramps = [](RenderParams &p) {
    p.elem_ramp = kTab;
    p.out_ramp = kTab + 4096;
    p.ramp_stream_stride = 4096;
  };
  expect("stereo + ramps, aligned", with(st, ramps), 16, nullptr, Family::Fast, 1);
  expect("12 channels + ramps, aligned", with(w, ramps), 16, nullptr, Family::Wide4Mix, 0);
  ramp_rules("stereo + ramps", with(st, ramps), 16, Family::Generic, 0);
  ramp_rules("12 channels + ramps", with(w, ramps), 16, Family::Generic, 0);

  // ---- the 32-bit rules, one step to either side of each bound ----
  // render_fast_kernel: (total / frame_size + 2) * in_frame_stride * 4 + 100 * frame_size < 2^31, here 6 frames of 1024
  constexpr int64_t k31 = (int64_t)1 << 31;
  constexpr int64_t kFastMax = 89474216;    // the largest multiple of 4 within the bound
  static_assert(6 * kFastMax * 4 + 100 * 1024 < k31 && 6 * (kFastMax + 4) * 4 + 100 * 1024 >= k31, "in_frame_stride bound");
  one_change("stereo", "in_frame_stride at the 32-bit bound", st, 16, [](RenderParams &p) { p.in_frame_stride = kFastMax; },
             Family::Fast, 0);
  one_change("stereo", "in_frame_stride 4 floats beyond", st, 16, [](RenderParams &p) { p.in_frame_stride = kFastMax + 4; },
             Family::Generic, 0);
  // the packets of its LPCM variant: (total / frame_size + 2) * lpcm_frame_stride + 2^24 < 2^31
  constexpr int64_t kLpMax = 355117736;     // the largest multiple of 8 within the bound
  static_assert(6 * kLpMax + (1 << 24) < k31 && 6 * (kLpMax + 8) + (1 << 24) >= k31, "lpcm_frame_stride bound");
  one_change("LPCM", "lpcm_frame_stride at the 32-bit bound", lp, 16, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax; },
             Family::Lpcm, 1);
  one_change("LPCM", "lpcm_frame_stride 8 bytes beyond", lp, 16, [](RenderParams &p) { p.lpcm_frame_stride = kLpMax + 8; },
             Family::Refused, 0, IAMF_HIP_ERR_INVALID_STATE);
  // the FIR stage: (total / frame_size + 1) * in_frame_stride < 2^31 floats, else BAD_ARG.  Below the bound the call is
  // still beyond the fast kernel's byte offsets, which is the UNIMPLEMENTED of any call that kernel does not take
  constexpr int64_t kFirMax = 429496728;    // the largest multiple of 4 within the bound
  static_assert(5 * kFirMax < k31 && 5 * (kFirMax + 4) >= k31, "FIR in_frame_stride bound");
  one_change("FIR", "in_frame_stride at the fast kernel's bound", f16, 16, [](RenderParams &p) { p.in_frame_stride = kFastMax; },
             Family::FirSplit, 0);
  one_change("FIR", "in_frame_stride at the stage's 32-bit bound", f16, 16, [](RenderParams &p) { p.in_frame_stride = kFirMax; },
             Family::Refused, 0, UNIMPL);
  one_change("FIR", "in_frame_stride 4 floats beyond", f16, 16, [](RenderParams &p) { p.in_frame_stride = kFirMax + 4; },
             Family::Refused, 0, IAMF_HIP_ERR_BAD_ARG);
}

// ---- long-lived streams: the rules that read the position (fast_shape_ok, pos16, pos_any) ----
// A 48 kHz stream passes 2^31 samples after 12.4 hours and 2^32 after 24.9.  The rules look at pos0 & 15 and at
// pos0 < kDelay only, so a call at a large position takes the route the same call takes at a small position of the same
// residue: 2^31 as 4096, 2^31 + 16 as 4112, 2^32 + 8 as 4104, 2^40 + 237 as 4333.  A rule that narrowed pos0 to 32 bits
// would see 0, 16, 8 and 237: below kDelay, where the off-grid positions go to the generic kernel.
void long_positions(const RenderParams &st, const RenderParams &w, const RenderParams &nl, const RenderParams &lp) {
  constexpr int64_t k31 = (int64_t)1 << 31, k32 = (int64_t)1 << 32, k40 = (int64_t)1 << 40;
  const int64_t pairs[4][2] = {{k31, 4096}, {k31 + 16, 4112}, {k32 + 8, 4104}, {k40 + 237, 4333}};
  struct Block {
    const char *name;
    RenderParams p;
    int m;
    Family grid, off;   // the family on the 16-sample grid and off it
    int variant;
  };
  const Block blocks[] = {
      {"stereo", st, 16, Family::Fast, Family::Fast, 0},
      {"stereo + second element", with(st, second_element), 16, Family::Fast, Family::Fast, 1},
      {"down-mixer 8 -> 2", with(aligned(8, 2), down_mixer), 8, Family::FastDown, Family::FastDown, 0},
      {"LPCM", lp, 16, Family::Lpcm, Family::Lpcm, 1},
      {"12 channels", w, 16, Family::Wide4, Family::Wide4, 0},
      {"12 channels + second element", with(w, second_element), 16, Family::Wide4Mix, Family::Wide4Mix, 0},
      {"down-mixer 12 -> 6", with(aligned(12, 6), down_mixer), 12, Family::Wide4Down, Family::Wide4Down, 0},
      {"demixer 12 -> 12", with(aligned(12, 12), demixer), 12, Family::Wide4Demix, Family::Wide4Demix, 0},
      {"LFE, 12 channels", with(w, lfe), 16, Family::Wide4Lfe, Family::Generic, 0},
      {"12 channels, s24", aligned(16, 12, IAMF_HIP_FMT_S24), 16, Family::Wide, Family::Generic, 0},
      {"11 channels", aligned(12, 11), 12, Family::Wide, Family::Generic, 0},
      {"limiter off", nl, 16, Family::Nolim, Family::Nolim, 0},
  };
  for (const Block &b : blocks) {
    for (const auto &pr : pairs) {
      RenderParams big = b.p, small = b.p;
      big.pos0 = pr[0];
      small.pos0 = pr[1];
      const Route rs = pick_route(small, b.m);
      const Family want = (pr[1] & 15) ? b.off : b.grid;
      // a family that differs between the grid and off it keeps its variant only on the grid
      const int variant = want == Family::Generic ? 0 : b.variant;
      char what[96];
      snprintf(what, sizeof(what), "%s: pos0 = %lld as at %lld", b.name, (long long)pr[0], (long long)pr[1]);
      expect(what, big, b.m, nullptr, rs.family, rs.variant, rs.err);
      snprintf(what, sizeof(what), "%s: pos0 = %lld", b.name, (long long)pr[0]);
      expect(what, big, b.m, nullptr, want, variant);
    }
  }
}

// ---- the staged limiter-table windows: n_end against kFWin (render_fast.hpp, render_wide4.hpp, render_fanout.hpp) and
// kWWin (render_wide.hpp) ----
// iamf_hip_batch_create derives (n_atk, n_end) from the sample rate: (6, 1087) at 5407 Hz, (6, 1088) at 5408 Hz, (2, 319) at
// 1587 Hz and (2, 320) at 1588 Hz (tests/test_programmes_cpu.py asserts these from the same accumulation).  A vector kernel
// stages a window of its table as long as the constant and must not get a table that ends inside it; one step on it must.
// A member of a fan-out is fused where its own call routes to Fast/0 (iamf_hip_render_fanout), so the stereo rows are its
// rows too.  tests/test_gpu_rates.py runs both sides of each bound on the GPU.
void window_rules(const RenderParams &st, const RenderParams &w, const RenderParams &lp, const RenderParams &f16) {
  static_assert(kFWin == 1088 && kWWin == 320, "the rates of tests/programmes.py (WINDOW_RATES) sit on these two");
  const int UNIMPL = IAMF_HIP_ERR_UNIMPLEMENTED;
  const auto below = [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin - 1; };
  const auto at = [](RenderParams &p) { p.n_atk = 6; p.n_end = kFWin; };
  const auto wbelow = [](RenderParams &p) { p.n_atk = 2; p.n_end = kWWin - 1; };
  const auto wat = [](RenderParams &p) { p.n_atk = 2; p.n_end = kWWin; };
  struct Row {
    const char *name;
    RenderParams p;
    int m;
    Family taken;       // n_end == kFWin
    int variant;
    Family refused;     // n_end == kFWin - 1: what the call falls to
    int err;
  };
  const Row rows[] = {
      {"stereo (and a fan-out's member)", st, 16, Family::Fast, 0, Family::Generic, IAMF_HIP_OK},
      {"mono", aligned(16, 1), 16, Family::Fast, 0, Family::Generic, IAMF_HIP_OK},
      {"stereo + second element", with(st, second_element), 16, Family::Fast, 1, Family::Generic, IAMF_HIP_OK},
      {"down-mixer 6 -> 2", with(aligned(6, 2), down_mixer), 6, Family::FastDown, 0, Family::Generic, IAMF_HIP_OK},
      {"LPCM", lp, 16, Family::Lpcm, 1, Family::Refused, IAMF_HIP_ERR_INVALID_STATE},
      {"FIR", f16, 16, Family::FirSplit, 0, Family::Refused, UNIMPL},
      // the wide4 family: at 1087 the plain call lands on the 256-sample kernel, whose window is 320; the staged variants,
      // which that kernel does not have, on the general one
      {"12 channels", w, 16, Family::Wide4, 0, Family::Wide, IAMF_HIP_OK},
      {"6 -> 6", aligned(6, 6), 6, Family::Wide4, 0, Family::Wide, IAMF_HIP_OK},
      {"12 channels, MFMA", with(w, [](RenderParams &p) { p.use_mfma = 1; }), 16, Family::Wide4, 1, Family::Wide, IAMF_HIP_OK},
      {"12 channels + second element", with(w, second_element), 16, Family::Wide4Mix, 0, Family::Generic, IAMF_HIP_OK},
      {"down-mixer 12 -> 6", with(aligned(12, 6), down_mixer), 12, Family::Wide4Down, 0, Family::Generic, IAMF_HIP_OK},
      {"demixer 12 -> 12", with(aligned(12, 12), demixer), 12, Family::Wide4Demix, 0, Family::Generic, IAMF_HIP_OK},
      {"LFE, 12 channels", with(w, lfe), 16, Family::Wide4Lfe, 0, Family::Generic, IAMF_HIP_OK},
  };
  for (const Row &r : rows) {
    char what[96];
    snprintf(what, sizeof(what), "%s: n_end = kFWin", r.name);
    expect(what, with(r.p, at), r.m, nullptr, r.taken, r.variant);
    snprintf(what, sizeof(what), "%s: n_end = kFWin - 1", r.name);
    // (the MFMA row keeps its variant on the 256-sample kernel, every other refused side is variant 0)
    expect(what, with(r.p, below), r.m, nullptr, r.refused, r.refused == Family::Wide ? r.variant : 0, r.err);
  }
  // where wide4 refuses for another reason as well, 1087 or 1088 makes no difference
  expect("12 channels, IAMF_HIP_NO_WIDE4: n_end = kFWin - 1", with(w, below), 16, "IAMF_HIP_NO_WIDE4", Family::Wide, 0);
  // render_wide.hpp's own window
  const RenderParams e11 = aligned(12, 11), w24 = aligned(16, 12, IAMF_HIP_FMT_S24);
  expect("12 -> 11: n_end = kWWin", with(e11, wat), 12, nullptr, Family::Wide, 0);
  expect("12 -> 11: n_end = kWWin - 1", with(e11, wbelow), 12, nullptr, Family::Generic, 0);
  expect("12 -> 11, MFMA: n_end = kWWin", with(e11, [&](RenderParams &p) { wat(p); p.use_mfma = 1; }), 12, nullptr, Family::Wide, 1);
  expect("12 -> 11, MFMA: n_end = kWWin - 1", with(e11, [&](RenderParams &p) { wbelow(p); p.use_mfma = 1; }), 12, nullptr, Family::Generic, 0);
  expect("12 channels, s24: n_end = kWWin", with(w24, wat), 16, nullptr, Family::Wide, 0);
  expect("12 channels, s24: n_end = kWWin - 1", with(w24, wbelow), 16, nullptr, Family::Generic, 0);
  expect("12 channels, s16: n_end = kWWin (wide4 refuses, the 256-sample kernel takes it)", with(w, wat), 16, nullptr, Family::Wide, 0);
  expect("12 channels, s16: n_end = kWWin - 1", with(w, wbelow), 16, nullptr, Family::Generic, 0);
  expect("stereo: n_end = kWWin", with(st, wat), 16, nullptr, Family::Generic, 0);
}

}  // namespace

int main() {
  const char *const switches[] = {"IAMF_HIP_FORCE_GENERIC", "IAMF_HIP_NO_WIDE4", "IAMF_HIP_FIR_F16", "IAMF_HIP_FIR_F32",
                                  "IAMF_HIP_FIR_FUSED", "IAMF_HIP_LP_LATE"};
  for (const char *e : switches) unsetenv(e);
  list_checks();
  set_checks();
  const int UNIMPL = IAMF_HIP_ERR_UNIMPLEMENTED;

  // ---- stereo ----
  const RenderParams st = aligned(16, 2);
  expect("aligned stereo, m = 16", st, 16, nullptr, Family::Fast, 0);
  expect("  pos0 = 8", with(st, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Generic, 0);
  expect("  pos0 = 248 (>= 240, not a multiple of 16)", with(st, [](RenderParams &p) { p.pos0 = 248; }), 16, nullptr, Family::Fast, 0);
  expect("  total % 64 != 0", with(st, [](RenderParams &p) { set_total(p, 4096 + 32); }), 16, nullptr, Family::Generic, 0);
  expect("  in == nullptr (flush)", with(st, [](RenderParams &p) { p.in = nullptr; p.total = 240; }), 16, nullptr, Family::Generic, 0);
  expect("  IAMF_HIP_FORCE_GENERIC", st, 16, "IAMF_HIP_FORCE_GENERIC", Family::Generic, 0);
  expect("  m = 11", aligned(11, 2), 11, nullptr, Family::Generic, 0);
  expect("  m = 7", aligned(7, 2), 7, nullptr, Family::Refused, 0, UNIMPL);

  // ---- 12 channels ----
  const RenderParams w = aligned(16, 12);
  expect("aligned, 12 channels, s16, whole chunks, m = 16", w, 16, nullptr, Family::Wide4, 0);
  expect("  use_mfma", with(w, [](RenderParams &p) { p.use_mfma = 1; }), 16, nullptr, Family::Wide4, 1);
  expect("  s24", aligned(16, 12, IAMF_HIP_FMT_S24), 16, nullptr, Family::Wide, 0);
  expect("  s24, use_mfma", with(aligned(16, 12, IAMF_HIP_FMT_S24), [](RenderParams &p) { p.use_mfma = 1; }), 16, nullptr, Family::Wide, 1);
  expect("  a last chunk of 128", with(w, [](RenderParams &p) { set_total(p, 4096 + 128); }), 16, nullptr, Family::Wide, 0);
  expect("  a last chunk of 256", with(w, [](RenderParams &p) { set_total(p, 4096 + 256); }), 16, nullptr, Family::Wide4, 0);
  expect("  pos0 = 248: wide4 places its ring per call", with(w, [](RenderParams &p) { p.pos0 = 248; }), 16, nullptr, Family::Wide4, 0);
  expect("  pos0 = 248, s24: the 256-sample kernel needs a multiple of 16",
         with(aligned(16, 12, IAMF_HIP_FMT_S24), [](RenderParams &p) { p.pos0 = 248; }), 16, nullptr, Family::Generic, 0);
  expect("  IAMF_HIP_NO_WIDE4", w, 16, "IAMF_HIP_NO_WIDE4", Family::Wide, 0);
  expect("  IAMF_HIP_FORCE_GENERIC", w, 16, "IAMF_HIP_FORCE_GENERIC", Family::Generic, 0);
  expect("  m = 24: no wide4 instance", aligned(24, 12), 24, nullptr, Family::Wide, 0);
  expect("  m = 11", aligned(11, 12), 11, nullptr, Family::Generic, 0);

  // ---- second element or ramps ----
  expect("second element into stereo", with(st, second_element), 16, nullptr, Family::Fast, 1);
  expect("output ramp into stereo", with(st, [](RenderParams &p) { p.out_ramp = kTab; }), 16, nullptr, Family::Fast, 1);
  expect("second element into 12 channels", with(w, second_element), 16, nullptr, Family::Wide4Mix, 0);
  expect("  use_mfma", with(w, [](RenderParams &p) { second_element(p); p.use_mfma = 1; }), 16, nullptr, Family::Wide4Mix, 1);
  expect("second element into 14 channels: no mix instance", with(aligned(16, 14), second_element), 16, nullptr, Family::Generic, 0);
  expect("second element of 6 channels into stereo", with(st, [](RenderParams &p) { second_element(p); p.m2 = 6; }), 16, nullptr,
         Family::Generic, 0);

  // ---- down-mixer with per-frame parameters ----
  expect("down-mixer 8 -> 2", with(aligned(8, 2), down_mixer), 8, nullptr, Family::FastDown, 0);
  expect("down-mixer 12 -> 6", with(aligned(12, 6), down_mixer), 12, nullptr, Family::Wide4Down, 0);
  expect("down-mixer 10 -> 10: no pair", with(aligned(10, 10), down_mixer), 10, nullptr, Family::Generic, 0);
  expect("down-mixer without frames 8 -> 2", with(aligned(8, 2), [](RenderParams &p) { p.dmx_on = 1; }), 8, nullptr, Family::Generic, 0);
  expect("demixer and down-mixer together 12 -> 6", with(aligned(12, 6), [](RenderParams &p) { down_mixer(p); demixer(p); }), 12, nullptr,
         Family::Generic, 0);

  // ---- demixer of scalable channel audio ----
  const RenderParams dx = with(aligned(12, 12), demixer);
  expect("demixer with demix_w4, 12 -> 12", dx, 12, nullptr, Family::Wide4Demix, 0);
  expect("  use_mfma", with(dx, [](RenderParams &p) { p.use_mfma = 1; }), 12, nullptr, Family::Generic, 0);
  expect("  demix_i0 % 4 != 0", with(dx, [](RenderParams &p) { p.demix_i0 = 2; }), 12, nullptr, Family::Generic, 0);
  expect("  without demix_w4", with(dx, [](RenderParams &p) { p.demix_w4 = 0; }), 12, nullptr, Family::Generic, 0);

  // ---- HOA LFE generator ----
  expect("LFE buffer, m = 16, 12 channels", with(w, lfe), 16, nullptr, Family::Wide4Lfe, 0);
  expect("  use_mfma", with(w, [](RenderParams &p) { lfe(p); p.use_mfma = 1; }), 16, nullptr, Family::Wide4Lfe, 1);
  expect("  lfe_k0 > 0", with(w, [](RenderParams &p) { lfe(p); p.lfe_k0 = 3; }), 16, nullptr, Family::Generic, 0);
  expect("  stereo output", with(st, lfe), 16, nullptr, Family::Generic, 0);
  expect("  m = 6: no LFE instance", with(aligned(6, 12), lfe), 6, nullptr, Family::Generic, 0);

  // ---- limiter off ----
  const RenderParams nl = with(st, [](RenderParams &p) { p.limiter_on = 0; });
  expect("limiter off, a shape nolim_shape_ok accepts", nl, 16, nullptr, Family::Nolim, 0);
  expect("  IAMF_HIP_FORCE_GENERIC", nl, 16, "IAMF_HIP_FORCE_GENERIC", Family::Generic, 0);
  expect("  m = 11", with(aligned(11, 2), [](RenderParams &p) { p.limiter_on = 0; }), 11, nullptr, Family::Nolim, 0);
  expect("  total % 4 != 0", with(nl, [](RenderParams &p) { set_total(p, 4098); }), 16, nullptr, Family::Generic, 0);

  // ---- HRTF stage ----
  const RenderParams f16 = with(st, fir);
  expect("FIR, m = 16, spectra tables and scratch", f16, 16, nullptr, Family::FirSplit, 0);
  expect("  IAMF_HIP_FIR_FUSED", f16, 16, "IAMF_HIP_FIR_FUSED", Family::FirFused, 3);
  expect("  IAMF_HIP_FIR_F32", f16, 16, "IAMF_HIP_FIR_F32", Family::FirFused, 1);
  expect("  IAMF_HIP_FIR_F16 with its tables", with(f16, [](RenderParams &p) { p.fir_h16 = kTab; }), 16, "IAMF_HIP_FIR_F16", Family::FirFused, 2);
  expect("  without scratch", with(f16, [](RenderParams &p) { p.fir_y = nullptr; }), 16, nullptr, Family::FirFused, 3);
  expect("  m = 6 (channel-based set)", with(aligned(6, 2), fir), 6, nullptr, Family::FirSplit, 0);
  expect("  m = 6, IAMF_HIP_FIR_FUSED", with(aligned(6, 2), fir), 6, "IAMF_HIP_FIR_FUSED", Family::FirFused, 3);
  expect("  m = 3", with(aligned(3, 2), fir), 3, nullptr, Family::Refused, 0, UNIMPL);
  expect("  misaligned (total % 64 != 0)", with(f16, [](RenderParams &p) { set_total(p, 4096 + 32); }), 16, nullptr, Family::Refused, 0, UNIMPL);
  expect("  flush (in == nullptr)", with(f16, [](RenderParams &p) { p.in = nullptr; p.total = 240; }), 16, nullptr, Family::Generic, 0);

  // ---- element 0 as LPCM packets ----
  const RenderParams lp = with(st, lpcm);
  expect("LPCM input, n_launch = 1024", with(lp, [](RenderParams &p) { p.n_launch = p.n_streams = 1024; }), 16, nullptr, Family::Lpcm, 1);
  expect("  n_launch = 1025", with(lp, [](RenderParams &p) { p.n_launch = p.n_streams = 1025; }), 16, nullptr, Family::Lpcm, 0);
  expect("  IAMF_HIP_LP_LATE", lp, 16, "IAMF_HIP_LP_LATE", Family::Lpcm, 0);
  expect("  m = 6: no instance", with(aligned(6, 2), lpcm), 6, nullptr, Family::Refused, 0, IAMF_HIP_ERR_INVALID_STATE);
  expect("  pos0 = 8: not a call of the fast kernel", with(lp, [](RenderParams &p) { p.pos0 = 8; }), 16, nullptr, Family::Refused, 0,
         IAMF_HIP_ERR_INVALID_STATE);

  address_rules(st, w, nl, f16, lp);
  packet_layout_rows(st);
  long_positions(st, w, nl, lp);
  window_rules(st, w, lp, f16);

  printf("%d cases, %d wrong\n", g_cases, g_failed);
  if (!g_failed) printf("OK\n");
  return g_failed ? 1 : 0;
}
