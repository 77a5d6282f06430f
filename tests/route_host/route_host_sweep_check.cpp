// Host-only sweep of the whole routing decision (iac_amd/csrc/render_route.hpp): both pick_route overloads and route_key over a
// deterministic family of parameter blocks, printed as one digest line per 1024 cases.  The per-form checks beside this file pin
// one row per rule; this one pins that a change of the rules' wording moved NO route: tests/golden/route_sweep.txt holds the lines
// the same program printed against the tree in front of the change that gathered the packet rules into shared predicates, and
// tests/test_route_host_sweep.py compares line by line.
//
// The blocks: for every row of every set that pick_route can name (the fan-out's and the resampler's rows are launched by entries
// of their own), the smallest block that routes to it — the program checks that it does; from each, every single mutation of
// the fixed list in mutations() (each field the rules read: zero, a step off its grid, a step past each bound, each mark, each
// off-switch alone), and a seeded selection of pairs of them.
//
// The program checks its own coverage, so the sweep cannot hide a gap: every Family, Refused included, is reached by at least
// 100 cases, and each of the six marked rules answers true on at least 5 % and false on at least 5 % of the cases that carry
// its mark.
//
// Two names differ between the trees the golden file was made from and compared against: -DSWEEP_WALKER / -DSWEEP_SETS name the
// walker over every set and the number of sets.  For the same reason the marks are the bare values of RenderParams::ragged here.
// `--dump` prints every case instead of the digests (to find the case behind a line that differs).
// Driven by tests/test_route_host_sweep.py.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/iamf_hip.h"

#ifndef SWEEP_WALKER
#define SWEEP_WALKER for_each_instance_of_set
#endif
#ifndef SWEEP_SETS
#define SWEEP_SETS kRouteSets
#endif

namespace {
#include "../../iac_amd/csrc/render_params.hpp"
#include "../../iac_amd/csrc/render_route.hpp"

// a block and the channel count it is routed with; env: a switch the row needs (the late prefetch variants), or null
struct Blk {
  RenderMixParams p;
  int m;
  const char *env;
};

template <class T>
T *at(uintptr_t a) {
  return reinterpret_cast<T *>(a);   // never dereferenced: routing looks at alignment only
}
template <class T>
void bump(T *&ptr, int bytes) {
  ptr = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(ptr) + bytes);
}

// ---- the smallest valid block per row ----

// one frame of 1024 samples, 64 streams, limiter on, everything on its grid: route_host_check.cpp's "aligned"
Blk aligned(int m, int out_ch, int fmt = IAMF_HIP_FMT_S16) {
  Blk b;
  memset(&b.p, 0, sizeof(b.p));
  b.m = m;
  b.env = nullptr;
  RenderMixParams &p = b.p;
  p.frame_size = 1024;
  p.total = 1024;
  p.in = at<const float>(0x10000);
  p.in_frame_stride = (int64_t)m * p.frame_size;
  p.in_stream_stride = 2 * p.in_frame_stride;
  p.pcm = at<uint8_t>(0x40000);
  p.out_ch = p.og_ch = out_ch;
  p.out_format = fmt;
  p.pcm_stream_stride = (int64_t)2048 * out_ch * 4;
  p.n_streams = p.n_launch = 64;
  p.limiter_on = 1;
  p.n_atk = 241;
  p.n_end = 9651;
  p.ramp_stream_stride = 1024;
  return b;
}
void second_element(Blk &b) {
  b.p.in2 = at<const float>(0x20000);
  b.p.m2 = 2;
  b.p.in2_frame_stride = 2 * b.p.frame_size;
  b.p.in2_stream_stride = 2 * b.p.in2_frame_stride;
}
void down_mixer(Blk &b) {
  b.p.dmx_on = 1;
  b.p.dmx_frames = at<const iamf_hip_dmx_frame>(0x50000);
}
void fir(Blk &b, int stage) {   // 4: the split form; 3: the FFT stage fused; 2: split-f16 MFMA; 1: f32 MFMA
  const float *tab = at<const float>(0x30000);
  b.p.fir_taps = 256;
  if (stage >= 3) b.p.fir_pq = b.p.fir_tw = b.p.fir_zero = b.p.fir_id_matrix = tab;
  if (stage == 4) b.p.fir_y = at<float>(0x38000);
  if (stage == 2) b.p.fir_h16 = tab;
}
// element 0 as packets of `bytes`-byte samples, coupled where m is a loudspeaker layout's count: a head of 16 bytes, then the
// runs one behind the other, each start on the 8-byte grid, a pair's partner one sample behind its first (lpcm_form.hpp)
void packets(Blk &b, int bytes, int total, int frame_size) {
  RenderMixParams &p = b.p;
  const bool coupled = LpcmCoupledM::has(b.m);
  p.total = total;
  p.frame_size = frame_size;
  p.lpcm = at<const uint8_t>(0x100000);
  p.lpcm_bytes = bytes;
  p.lpcm_coupled = coupled ? (bytes == 3 ? 2 : 1) : 0;
  int off = 16;
  for (int c = 0; c < b.m && c < 16; ++c) {
    if (coupled && lpcm_coupled_paired(b.m, c)) {
      if (c & 1) {
        p.lpcm_off[c] = p.lpcm_off[c - 1] + bytes;
        off = (off + 2 * bytes * frame_size + 7) & ~7;
      } else {
        p.lpcm_off[c] = off;
      }
    } else {
      p.lpcm_off[c] = off;
      off = (off + bytes * frame_size + 7) & ~7;
    }
  }
  p.lpcm_frame_stride = (off + 15) & ~15;
  p.lpcm_stream_stride = 2 * p.lpcm_frame_stride;
  p.ramp_stream_stride = (total + 3) & ~3;
}
// element 1 as packets of element 0's sample size: lp2 == 2 one coupled stereo pair, lp2 == 1 one mono run
void packets2(Blk &b, int lp2) {
  RenderMixParams &p = b.p;
  const int bytes = p.lpcm_bytes;
  p.lpcm_mix = (bytes == 3 ? 4 : 0) | lp2;
  p.m2 = lp2 == 2 ? 2 : 1;
  p.lpcm2 = at<const uint8_t>(0x8000000);
  p.in2 = at<const float>(0x8000000);
  p.lpcm2_off[0] = 16;
  if (lp2 == 2) p.lpcm2_off[1] = 16 + bytes;
  p.lpcm2_frame_stride = (16 + 2 * bytes * p.frame_size + 15) & ~15;
  p.lpcm2_stream_stride = 2 * p.lpcm2_frame_stride;
  p.in2_frame_stride = p.lpcm2_frame_stride;
  p.in2_stream_stride = p.lpcm2_stream_stride;
  p.matrix2 = at<const float>(0x60000);
  p.src_feed2 = at<const int32_t>(0x61000);
  p.gains2 = at<const float>(0x62000);
}

// false: no call of pick_route names the row (the fan-out's and the resampler's kernels)
bool block_of_row(int f, int v, int m, int c, int k, Blk &b) {
  switch (f) {
    case IAMF_HIP_ROUTE_GENERIC: b = aligned(m, 2), b.p.pos0 = 8; return true;
    case IAMF_HIP_ROUTE_NOLIM: b = aligned(m, 2), b.p.limiter_on = 0; return true;
    case IAMF_HIP_ROUTE_FAST:
      b = aligned(m, c);
      if (v) second_element(b);
      return true;
    case IAMF_HIP_ROUTE_FAST_DOWN: b = aligned(m, c), down_mixer(b); return true;
    case IAMF_HIP_ROUTE_WIDE: b = aligned(m, 11), b.p.use_mfma = v; return true;
    case IAMF_HIP_ROUTE_WIDE4: b = aligned(m, c), b.p.use_mfma = v; return true;
    case IAMF_HIP_ROUTE_WIDE4_DEMIX: b = aligned(m, c), b.p.demix_on = 1, b.p.demix_w4 = 1; return true;
    case IAMF_HIP_ROUTE_WIDE4_DOWN: b = aligned(m, c), down_mixer(b); return true;
    case IAMF_HIP_ROUTE_WIDE4_MIX: b = aligned(m, c), second_element(b), b.p.use_mfma = v; return true;
    case IAMF_HIP_ROUTE_WIDE4_LFE: b = aligned(m, c), b.p.lfe = at<const float>(0x70000), b.p.use_mfma = v; return true;
    case IAMF_HIP_ROUTE_LPCM:
      b = aligned(m, c), packets(b, 2, 1024, 1024);
      if (!v) b.p.n_launch = b.p.n_streams = 1025;
      return true;
    case IAMF_HIP_ROUTE_FIR_SPLIT: b = aligned(m, 2), fir(b, 4); return true;
    case IAMF_HIP_ROUTE_FIR_FUSED: b = aligned(m, 2), fir(b, v); return true;
    case IAMF_HIP_ROUTE_LPCM24:
    case IAMF_HIP_ROUTE_LPCM24_COUPLED:
      b = aligned(m, c), packets(b, 3, 1024, 1024), b.env = v ? nullptr : "IAMF_HIP_LP_LATE";
      return true;
    case IAMF_HIP_ROUTE_LPCM_COUPLED:
      b = aligned(m, c), packets(b, 2, 1024, 1024), b.env = v ? nullptr : "IAMF_HIP_LP_LATE";
      return true;
    case IAMF_HIP_ROUTE_LPCM_MIX: b = aligned(m, c), packets(b, 2, 1024, 1024), packets2(b, k); return true;
    case IAMF_HIP_ROUTE_LPCM24_MIX: b = aligned(m, c), packets(b, 3, 1024, 1024), packets2(b, k); return true;
    case IAMF_HIP_ROUTE_FAST_INTERLEAVED:
      b = aligned(m, c);
      b.p.interleaved = 1, b.p.frame_size = 1, b.p.total = 1000, b.p.in_frame_stride = m, b.p.in_stream_stride = 1000 * m;
      return true;
    case IAMF_HIP_ROUTE_FAST_RAGGED:
      b = aligned(m, c);
      b.p.ragged = 1, b.p.frame_size = 1000, b.p.total = 1000, b.p.in_frame_stride = 1000 * m, b.p.in_stream_stride = 2000 * m;
      return true;
    case IAMF_HIP_ROUTE_PACKETS_RAGGED: b = aligned(m, c), packets(b, k, 1000, 1000), b.p.ragged = 2; return true;
    case IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED: b = aligned(m, c), packets(b, v, 1000, 1000), packets2(b, k), b.p.ragged = 3; return true;
    case IAMF_HIP_ROUTE_NOLIM_PACKETS:
      b = aligned(m, 2, IAMF_HIP_FMT_F32), packets(b, k, 1000, 1000), b.p.ragged = 4, b.p.limiter_on = 0;
      return true;
    case IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX:
      b = aligned(m, 2, IAMF_HIP_FMT_F32), packets(b, v, 1000, 1000), packets2(b, k), b.p.ragged = 5, b.p.limiter_on = 0;
      return true;
  }
  return false;
}

// ---- the mutations ----

struct Mut {
  std::string name;
  std::function<void(Blk &)> fn;   // null: only the switch
  const char *env;                 // a switch set to "1" for the case, or null
};

const char *const kSwitches[] = {"IAMF_HIP_FORCE_GENERIC",         "IAMF_HIP_LPCM_UNFUSED",           "IAMF_HIP_NOLIM_PACKETS_UNFUSED",
                                 "IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED", "IAMF_HIP_PACKETS_RAGGED_UNFUSED", "IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED",
                                 "IAMF_HIP_RAGGED_UNFUSED",        "IAMF_HIP_INTERLEAVED_UNFUSED",    "IAMF_HIP_NO_WIDE4",
                                 "IAMF_HIP_LP_LATE",               "IAMF_HIP_LP_EARLY",               "IAMF_HIP_FIR_F16",
                                 "IAMF_HIP_FIR_F32",               "IAMF_HIP_FIR_FUSED"};

// the largest stride on `grid` for which frames * stride * scale + slack stays below 2^31 (the kernels' 32-bit offsets)
int64_t bound32(const RenderMixParams &p, int64_t scale, int64_t slack, int64_t grid) {
  const int64_t frames = (int64_t)p.total / p.frame_size + 2;
  return (((((int64_t)1 << 31) - slack - 1) / (frames * scale)) / grid) * grid;
}

std::vector<Mut> mutations() {
  std::vector<Mut> v;
  const auto add = [&](std::string name, std::function<void(Blk &)> fn) { v.push_back(Mut{name, fn, nullptr}); };
  // a 32-bit field: zero, one step up and down, the values named
  const auto ints = [&](const char *name, int32_t RenderParams::*f, std::initializer_list<int> steps, std::initializer_list<int> values) {
    add(std::string(name) + " = 0", [=](Blk &b) { b.p.*f = 0; });
    for (int s : steps) add(std::string(name) + " += " + std::to_string(s), [=](Blk &b) { b.p.*f += s; });
    for (int x : values) add(std::string(name) + " = " + std::to_string(x), [=](Blk &b) { b.p.*f = x; });
  };
  // a stride: zero, steps off its grid
  const auto stride = [&](const char *name, auto f) {
    add(std::string(name) + " = 0", [=](Blk &b) { b.p.*f = 0; });
    for (int s : {-8, -4, -2, -1, 1, 2, 4, 8, 16}) add(std::string(name) + " += " + std::to_string(s), [=](Blk &b) { b.p.*f += s; });
    add(std::string(name) + " negated", [=](Blk &b) { b.p.*f = -(b.p.*f); });
  };
  // a pointer: null, steps off its grid; or, where the block has none, one on the 16-byte grid and one off it
  const auto ptr = [&](const char *name, auto f, uintptr_t fresh) {
    add(std::string(name) + " = null", [=](Blk &b) { b.p.*f = nullptr; });
    for (int s : {1, 2, 4, 8, 16}) add(std::string(name) + " += " + std::to_string(s) + " B", [=](Blk &b) { bump(b.p.*f, s); });
    add(std::string(name) + " set", [=](Blk &b) { b.p.*f = at<typename std::remove_pointer<typename std::remove_reference<decltype(b.p.*f)>::type>::type>(fresh); });
    add(std::string(name) + " set, + 4 B", [=](Blk &b) { b.p.*f = at<typename std::remove_pointer<typename std::remove_reference<decltype(b.p.*f)>::type>::type>(fresh + 4); });
  };

  // lengths.  (frame_size stays above zero: the rules divide by it, and no batch has such a frame)
  ints("total", &RenderParams::total, {-64, -4, -3, -2, -1, 1, 2, 3, 4, 24, 32, 64, 128, 256}, {1, 3, 4, 6, 8, 63, 64, 65, 240, 1024, 4096, 64000});
  for (int s : {-4, -2, -1, 1, 2, 4, 24})
    add("frame_size += " + std::to_string(s), [=](Blk &b) { if (b.p.frame_size + s > 0) b.p.frame_size += s; });
  for (int x : {1, 2, 3, 4, 6, 8, 64, 240, 1000, 1024, 2048})
    add("frame_size = " + std::to_string(x), [=](Blk &b) { b.p.frame_size = x; });
  add("five frames", [](Blk &b) { b.p.total = 5 * b.p.frame_size; });
  add("half a frame", [](Blk &b) { b.p.total = b.p.frame_size / 2; });
  // a trimmed frame: first + total against frame_size, one sample to either side of both variants of the rule
  for (int first : {-4, 2, 4, 100}) add("first = " + std::to_string(first), [=](Blk &b) { b.p.demix_i0 = first; });
  for (int first : {4, 100})
    for (int over : {-8, -4, -3, -2, -1, 0, 1, 2, 3, 4})
      add("first = " + std::to_string(first) + ", first + total = frame_size + " + std::to_string(over),
          [=](Blk &b) { b.p.demix_i0 = first, b.p.total = b.p.frame_size - first + over; });
  // the position and the limiter table's window
  for (int64_t pos : {(int64_t)8, (int64_t)16, (int64_t)239, (int64_t)240, (int64_t)248, (int64_t)1024, ((int64_t)1 << 32) + 8})
    add("pos0 = " + std::to_string(pos), [=](Blk &b) { b.p.pos0 = pos; });
  ints("n_end", &RenderParams::n_end, {}, {kWWin - 1, kWWin, kFWin - 1, kFWin});
  ints("n_launch", &RenderParams::n_launch, {}, {1, 1024, 1025, 4096});
  // the output
  ints("out_ch", &RenderParams::out_ch, {-1, 1}, {1, 2, 3, 6, 11, 12, 14, 15, 16, 24, 25});
  ints("og_ch", &RenderParams::og_ch, {-1, 1}, {});
  for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_S32, IAMF_HIP_FMT_F32})
    add("out_format = " + std::to_string(fmt), [=](Blk &b) { b.p.out_format = fmt; });
  for (int oc : {1, 6, 15, 16})
    for (int fmt : {IAMF_HIP_FMT_S16, IAMF_HIP_FMT_S24, IAMF_HIP_FMT_F32})
      add("out_ch = og_ch = " + std::to_string(oc) + ", out_format = " + std::to_string(fmt),
          [=](Blk &b) { b.p.out_ch = b.p.og_ch = oc, b.p.out_format = fmt; });
  ptr("pcm", &RenderParams::pcm, 0x48000);
  stride("pcm_stream_stride", &RenderParams::pcm_stream_stride);
  ints("limiter_on", &RenderParams::limiter_on, {}, {1});
  ints("use_mfma", &RenderParams::use_mfma, {}, {1});
  // the channel count the call is routed with
  for (int s : {-1, 1}) add("m += " + std::to_string(s), [=](Blk &b) { b.m += s; });
  for (int m : {1, 2, 3, 4, 6, 9, 11, 12, 16, 24}) add("m = " + std::to_string(m), [=](Blk &b) { b.m = m; });
  // element 0 as f32
  ptr("in", &RenderParams::in, 0x18000);
  stride("in_stream_stride", &RenderParams::in_stream_stride);
  stride("in_frame_stride", &RenderParams::in_frame_stride);
  for (int over : {0, 4}) {
    add("in_frame_stride at the 32-bit bound + " + std::to_string(over), [=](Blk &b) {
      b.p.in_frame_stride = (((((int64_t)1 << 31) - 100 * (int64_t)b.p.frame_size - 1) / (((int64_t)b.p.total / b.p.frame_size + 2) * 4)) & ~(int64_t)3) + over;
    });
    add("in_frame_stride at the FIR stage's bound + " + std::to_string(over),
        [=](Blk &b) { b.p.in_frame_stride = ((((int64_t)1 << 31) - 1) / ((int64_t)(b.p.total / b.p.frame_size) + 1) & ~(int64_t)3) + over; });
    add("interleaved: total at the 32-bit bound + " + std::to_string(over),
        [=](Blk &b) { b.p.total = (int32_t)(((((int64_t)1 << 31) - ((int64_t)1 << 24) - 1) / (4 * (int64_t)(b.m > 0 ? b.m : 1))) + over / 4); });
  }
  // element 0 as packets
  ptr("lpcm", &RenderParams::lpcm, 0x108000);
  stride("lpcm_stream_stride", &RenderParams::lpcm_stream_stride);
  stride("lpcm_frame_stride", &RenderParams::lpcm_frame_stride);
  for (int over : {0, 4, 8})
    add("lpcm_frame_stride at the 32-bit bound + " + std::to_string(over),
        [=](Blk &b) { b.p.lpcm_frame_stride = bound32(b.p, 1, (int64_t)1 << 24, 8) + over; });
  add("lpcm_frame_stride = 2^30, 64 frames", [](Blk &b) { b.p.lpcm_frame_stride = (int64_t)1 << 30, b.p.lpcm_stream_stride = (int64_t)1 << 37, b.p.total = 64 * b.p.frame_size; });
  ints("lpcm_bytes", &RenderParams::lpcm_bytes, {}, {1, 2, 3, 4});
  ints("lpcm_coupled", &RenderParams::lpcm_coupled, {}, {1, 2, 3});
  for (int c : {0, 1, 2, 3, 4, 5, 8, 11, 15}) {
    for (int s : {-4, -2, -1, 1, 2, 3, 4, 8}) add("lpcm_off[" + std::to_string(c) + "] += " + std::to_string(s), [=](Blk &b) { b.p.lpcm_off[c] += s; });
    add("lpcm_off[" + std::to_string(c) + "] = -8", [=](Blk &b) { b.p.lpcm_off[c] = -8; });
  }
  for (int first : {1, 2, 4})   // first_sample counted into every run's start, as lpcm_in_of does
    add("every run " + std::to_string(first) + " samples on", [=](Blk &b) {
      const int bytes = b.p.lpcm_bytes == 3 ? 3 : 2;
      for (int c = 0; c < 16; ++c) b.p.lpcm_off[c] += first * bytes * ((b.p.lpcm_coupled && lpcm_coupled_paired(b.m, c)) ? 2 : 1);
      for (int c = 0; c < 4; ++c) b.p.lpcm2_off[c] += first * bytes * ((b.p.lpcm_mix & 3) == 2 ? 2 : 1);
      b.p.demix_i0 = first, b.p.total = b.p.frame_size - 4;
    });
  // the second element: f32 or packets
  ptr("in2", &RenderParams::in2, 0x28000);
  stride("in2_stream_stride", &RenderParams::in2_stream_stride);
  stride("in2_frame_stride", &RenderParams::in2_frame_stride);
  for (int over : {0, 4, 8})
    add("in2_frame_stride at the 32-bit bound + " + std::to_string(over), [=](Blk &b) { b.p.in2_frame_stride = bound32(b.p, 1, (int64_t)1 << 24, 8) + over; });
  add("a second f32 element", [](Blk &b) { second_element(b); });
  ints("m2", &RenderParams::m2, {-1, 1}, {1, 2, 3, 4, 5, 6});
  ints("lpcm_mix", &RenderParams::lpcm_mix, {-1, 1}, {1, 2, 3, 4, 5, 6, 7, 8});
  add("lpcm_mix of the other sample size", [](Blk &b) { b.p.lpcm_mix ^= 4; });
  add("lpcm2 = null", [](Blk &b) { b.p.lpcm2 = nullptr; });
  for (int s : {4, 8, 16}) add("lpcm2 += " + std::to_string(s) + " B", [=](Blk &b) { bump(b.p.lpcm2, s); });
  for (int s : {4, 8, 16}) add("lpcm2 and in2 += " + std::to_string(s) + " B", [=](Blk &b) { bump(b.p.lpcm2, s), bump(b.p.in2, s); });
  for (int s : {-8, -4, -2, 2, 4, 8}) {
    add("lpcm2_stream_stride += " + std::to_string(s), [=](Blk &b) { b.p.lpcm2_stream_stride += s; });
    add("lpcm2_frame_stride += " + std::to_string(s), [=](Blk &b) { b.p.lpcm2_frame_stride += s; });
    add("lpcm2 and in2 stream strides += " + std::to_string(s), [=](Blk &b) { b.p.lpcm2_stream_stride += s, b.p.in2_stream_stride += s; });
    add("lpcm2 and in2 frame strides += " + std::to_string(s), [=](Blk &b) { b.p.lpcm2_frame_stride += s, b.p.in2_frame_stride += s; });
  }
  add("lpcm2_frame_stride = 0", [](Blk &b) { b.p.lpcm2_frame_stride = 0; });
  add("lpcm2 and in2 frame strides = 0", [](Blk &b) { b.p.lpcm2_frame_stride = b.p.in2_frame_stride = 0; });
  add("lpcm2 and in2 frame strides = 2^30, 64 frames", [](Blk &b) {
    b.p.lpcm2_frame_stride = b.p.in2_frame_stride = (int64_t)1 << 30, b.p.lpcm2_stream_stride = b.p.in2_stream_stride = (int64_t)1 << 37;
    b.p.total = 64 * b.p.frame_size;
  });
  for (int c : {0, 1, 2, 3}) {
    for (int s : {-4, -2, -1, 1, 2, 3, 4, 8}) add("lpcm2_off[" + std::to_string(c) + "] += " + std::to_string(s), [=](Blk &b) { b.p.lpcm2_off[c] += s; });
    add("lpcm2_off[" + std::to_string(c) + "] = -8", [=](Blk &b) { b.p.lpcm2_off[c] = -8; });
  }
  add("four mono runs of element 1", [](Blk &b) {
    b.p.m2 = 4, b.p.lpcm_mix = (b.p.lpcm_mix & 4) | 1;
    for (int c = 0; c < 4; ++c) b.p.lpcm2_off[c] = 16 + c * 4096;
  });
  add("matrix2 = null", [](Blk &b) { b.p.matrix2 = nullptr; });
  add("src_feed2 = null", [](Blk &b) { b.p.src_feed2 = nullptr; });
  add("gains2 = null", [](Blk &b) { b.p.gains2 = nullptr; });
  // ramps
  ptr("elem_ramp", &RenderParams::elem_ramp, 0x80000);
  ptr("elem2_ramp", &RenderParams::elem2_ramp, 0x88000);
  ptr("out_ramp", &RenderParams::out_ramp, 0x90000);
  stride("ramp_stream_stride", &RenderParams::ramp_stream_stride);
  for (int s : {1, 2, 4})
    add("all three ramps, ramp_stream_stride += " + std::to_string(s), [=](Blk &b) {
      b.p.elem_ramp = at<const float>(0x80000), b.p.elem2_ramp = at<const float>(0x88000), b.p.out_ramp = at<const float>(0x90000);
      b.p.ramp_stream_stride += s;
    });
  // the stages in front and behind
  ints("dmx_on", &RenderParams::dmx_on, {}, {1});
  add("down-mixer with frames", [](Blk &b) { down_mixer(b); });
  add("dmx_frames = null", [](Blk &b) { b.p.dmx_frames = nullptr; });
  ints("demix_on", &RenderParams::demix_on, {}, {1});
  ints("demix_w4", &RenderParams::demix_w4, {}, {1});
  add("demixer", [](Blk &b) { b.p.demix_on = 1, b.p.demix_w4 = 1; });
  add("pre_matrix set", [](Blk &b) { b.p.pre_matrix = at<const float>(0x98000); });
  add("lfe set", [](Blk &b) { b.p.lfe = at<const float>(0x70000); });
  add("lfe = null", [](Blk &b) { b.p.lfe = nullptr; });
  ints("lfe_k0", &RenderParams::lfe_k0, {}, {3});
  ints("fir_taps", &RenderParams::fir_taps, {}, {256});
  for (int stage : {1, 2, 3, 4}) add("HRTF stage " + std::to_string(stage), [=](Blk &b) { fir(b, stage); });
  add("fir_h16 set", [](Blk &b) { b.p.fir_h16 = at<const float>(0x30000); });
  add("fir_y = null", [](Blk &b) { b.p.fir_y = nullptr; });
  add("fir_pq = null", [](Blk &b) { b.p.fir_pq = nullptr; });
  add("fir_id_matrix = null", [](Blk &b) { b.p.fir_id_matrix = nullptr; });
  // the marks
  for (int mark = 0; mark <= 5; ++mark) add("ragged = " + std::to_string(mark), [=](Blk &b) { b.p.ragged = mark; });
  ints("interleaved", &RenderParams::interleaved, {}, {1});
  for (int mark : {4, 5}) add("ragged = " + std::to_string(mark) + ", limiter off", [=](Blk &b) { b.p.ragged = mark, b.p.limiter_on = 0; });
  for (int mark : {2, 3}) add("ragged = " + std::to_string(mark) + ", limiter on", [=](Blk &b) { b.p.ragged = mark, b.p.limiter_on = 1; });
  // the off-switches, each alone
  for (const char *e : kSwitches) v.push_back(Mut{e, nullptr, e});
  return v;
}

// ---- the sweep ----

constexpr int kFamilies = (int)Family::NolimPacketsMix + 1;
long g_family_cases[kFamilies];
long g_rule[6][2];   // interleaved, ragged == 1 .. 5: answers false / true among the cases that carry the mark
long g_cases = 0, g_failed = 0;
uint64_t g_hash = 1469598103934665603ull;
bool g_dump = false;

void mix(int64_t x) {
  for (int i = 0; i < 8; ++i) g_hash = (g_hash ^ (uint64_t)((x >> (8 * i)) & 255)) * 1099511628211ull;
}

void one_case(const Blk &b, const char *env, int base, int mut, int mut2) {
  if (b.env) setenv(b.env, "1", 1);
  if (env) setenv(env, "1", 1);
  const bool fg = getenv("IAMF_HIP_FORCE_GENERIC") != nullptr;
  const Route r[2] = {pick_route(static_cast<const RenderParams &>(b.p), b.m), pick_route(b.p, b.m)};
  if (b.p.interleaved) ++g_rule[0][interleaved_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (b.p.ragged == 1) ++g_rule[1][ragged_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (b.p.ragged == 2) ++g_rule[2][packets_ragged_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (b.p.ragged == 3) ++g_rule[3][packets_mix_ragged_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (b.p.ragged == 4) ++g_rule[4][nolim_packets_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (b.p.ragged == 5) ++g_rule[5][nolim_packets_mix_shape_ok(b.p, b.m, fg) ? 1 : 0];
  if (env) unsetenv(env);
  if (b.env) unsetenv(b.env);
  if (g_dump) printf("base %d mut %d %d:", base, mut, mut2);
  for (const Route &rt : r) {
    const RouteKey k = route_key(rt, b.p, b.m);
    ++g_family_cases[(int)rt.family];
    for (int x : {(int)rt.family, rt.variant, rt.err, k.family, k.variant, k.m, k.c, k.k, k.set}) {
      mix(x);
      if (g_dump) printf(" %d", x);
    }
    if (g_dump) printf(" |");
  }
  if (g_dump) printf("\n");
  if (++g_cases % 1024 == 0 && !g_dump) printf("cases %8ld .. %8ld  %016llx\n", g_cases - 1024, g_cases - 1, (unsigned long long)g_hash);
}

void check(const char *what, bool ok) {
  printf("%-110s %s\n", what, ok ? "ok" : "WRONG");
  g_failed += ok ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
  g_dump = argc > 1 && !strcmp(argv[1], "--dump");
  for (const char *e : kSwitches) unsetenv(e);
  const std::vector<Mut> muts = mutations();
  const int n_muts = (int)muts.size();
  uint64_t seed = 0x9e3779b97f4a7c15ull;   // the pairs: xorshift64*, the same on every host
  const auto next = [&]() {
    seed ^= seed >> 12, seed ^= seed << 25, seed ^= seed >> 27;
    return (uint32_t)((seed * 0x2545f4914f6cdd1dull) >> 33);
  };
  int bases = 0, rows_without = 0, rows_astray = 0;
  for (int set = 0; set < SWEEP_SETS; ++set) {
    SWEEP_WALKER(set, [&](int f, int v, int m, int c, int k) {
      Blk base;
      if (!block_of_row(f, v, m, c, k, base)) {
        ++rows_without;
        return;
      }
      // the block routes to its row, through either overload
      if (base.env) setenv(base.env, "1", 1);
      for (int mixp = 0; mixp < 2; ++mixp) {
        const Route r = mixp ? pick_route(base.p, base.m) : pick_route(static_cast<const RenderParams &>(base.p), base.m);
        const RouteKey key = route_key(r, base.p, base.m);
        const bool mix_only = f == IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX && !mixp;   // (the rule reads the block behind RenderParams)
        if (!mix_only && !(key.family == f && key.variant == v && key.m == m && key.c == c && key.k == k && key.set == set)) {
          ++rows_astray;
          printf("astray: set %d row (%d, %d, %d, %d, %d) routes to (%d, %d, %d, %d, %d) of set %d\n", set, f, v, m, c, k, key.family, key.variant,
                 key.m, key.c, key.k, key.set);
        }
      }
      if (base.env) unsetenv(base.env);
      one_case(base, nullptr, bases, -1, -1);
      for (int i = 0; i < n_muts; ++i) {
        Blk b = base;
        if (muts[i].fn) muts[i].fn(b);
        one_case(b, muts[i].env, bases, i, -1);
      }
      for (int pair = 0; pair < 96; ++pair) {   // (one switch at most: the second of two is dropped)
        const int i = (int)(next() % (uint32_t)n_muts), j = (int)(next() % (uint32_t)n_muts);
        Blk b = base;
        if (muts[i].fn) muts[i].fn(b);
        if (muts[j].fn) muts[j].fn(b);
        one_case(b, muts[i].env ? muts[i].env : muts[j].env, bases, i, j);
      }
      ++bases;
    });
  }
  if (!g_dump) printf("cases %8ld .. %8ld  %016llx\n", g_cases - g_cases % 1024, g_cases - 1, (unsigned long long)g_hash);
  printf("%d blocks (%d rows that no call of pick_route names), %d mutations, %ld cases\n", bases, rows_without, n_muts, g_cases);
  check("every block routes to the row it was built for", rows_astray == 0 && bases > 0);
  char what[160];
  for (int f = 0; f < kFamilies; ++f) {
    snprintf(what, sizeof(what), "Family %2d: %8ld routes (at least 100)", f, g_family_cases[f]);
    check(what, g_family_cases[f] >= 100);
  }
  const char *const rules[6] = {"interleaved_shape_ok", "ragged_shape_ok", "packets_ragged_shape_ok", "packets_mix_ragged_shape_ok",
                                "nolim_packets_shape_ok", "nolim_packets_mix_shape_ok"};
  for (int i = 0; i < 6; ++i) {
    const long all = g_rule[i][0] + g_rule[i][1];
    snprintf(what, sizeof(what), "%-28s true on %7ld, false on %7ld of the cases with its mark (each at least 5 %%)", rules[i], g_rule[i][1], g_rule[i][0]);
    check(what, all > 0 && 20 * g_rule[i][0] >= all && 20 * g_rule[i][1] >= all);
  }
  printf("%s\n", g_failed ? "FAILED" : "OK");
  return g_failed ? 1 : 0;
}
