// iamf_render.hip — MI355X (gfx950) kernels + the C ABI of include/iamf_hip.h.
//
// One workgroup owns one IAMF stream for the whole call and walks its samples in chunks.  Per
// chunk, fused in one pass over HBM:
//   [demixer of scalable channel audio, demixer.c] [projection de-mapping, IAMF_core_decoder.c:116-130]
//   -> element renderer (gain matrix h2m_rdr.c:1103-1150 / m2m_rdr.c:1826-1837, parametric
//      down-mixer downmix_renderer.c, or the HRTF FIR of render_fir.hpp)
//   -> element gain -> mix -> output gain -> loudness (IAMF_decoder.c:1392-1397, 2719-2730,
//   3206-3221) -> look-ahead peak limiter (audio_effect_peak_limiter.c:94-271)
//   -> float->PCM interleave (IAMF_decoder.c:100-167).
// Rendered samples never touch HBM (LDS ring or registers hold the limiter's 240-sample delay
// line); HBM sees the planar f32 input once and the packed PCM once.
//
// Kernel families (pick_route() of render_route.hpp picks one per call; all share the persisted per-stream state, so
// consecutive calls of one stream may take different ones):
//   render_fast.hpp     1- and 2-channel layouts, 1024-sample chunks, 4 samples per lane (headline);
//                       variants: FIR (HRTF stage on the f32 MFMA in front, render_fir.hpp), DOWN
//                       (parametric down-mixer, render_downmix.hpp), IN2 (second element of <= 4
//                       channels and / or per-sample gain ramps)
//   render_wide4.hpp    even 6..24-channel layouts, s16, rendered samples kept in registers; VALU or
//                       MFMA projection; variants: DMX (demixer of scalable channel audio in front),
//                       DOWN, MIX (as IN2) (own translation units: iamf_render_wide4.hip, _mix.hip)
//   render_wide.hpp     any other multi-channel aligned call, 256-sample chunks
//   render_generic.hpp  everything else: ragged calls, flush, limiter off, wide second elements,
//                       exact two-stage projection, demixer + down-mixer together, other PCM
//                       formats of the stages above
//
// Arithmetic is IEEE f32 in the reference's operation order (compiled with -ffp-contract=off,
// correctly rounded division), so the VALU paths are bit-exact against the CPU reference, not
// merely within +-1 LSB; the MFMA projection variants are the documented exception.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>
#include <vector>

#include "../../include/iamf_hip.h"

#define IAMF_FFT_HOST_TABLES   // render_fir_fft.hpp: the host-side table builder is compiled in this unit

#include "render_entry.hpp"

namespace {

#include "render_common.hpp"
#include "render_downmix.hpp"
#include "render_fir.hpp"
#include "render_fir16.hpp"
#include "render_fir_fft.hpp"
#include "render_fast.hpp"
#include "render_fir_launch.hpp"
#include "render_fanout.hpp"
#include "render_generic.hpp"
#include "render_nolim.hpp"
#include "render_wide.hpp"
#include "render_lfe.hpp"
#include "stream_state.hpp"
#include "lpcm_form.hpp"

// PCM with a fixed channel stride (the -DSAMSUNG_TV build: iamf_decoder_plane2stride_out with
// stride = SAMSUNG_SPECIFIC_CHANNELS = 12, IAMF_decoder.c:121-167,3492-3495).  The reference zeroes
// n * stride elements and then writes, channel by channel, element i * stride + c for every sample i:
// with more channels than the stride those land in the NEXT sample-frames' slots and the last writer
// wins (the highest channel), the last sample's surplus channels past the zeroed area.  One thread per
// output element reproduces exactly that.  src: natural interleaving [n][ch].
__global__ __launch_bounds__(256) void restride_kernel(const uint8_t *src, int64_t src_stream_stride, uint8_t *dst,
                                                       int64_t dst_stream_stride, int n, int ch, int sc, int bps, int stream0) {
  const int s = blockIdx.y + stream0;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_out = (int64_t)n * sc + (ch > sc ? ch - sc : 0);
  if (p >= n_out) return;
  const int c0 = (int)(p % sc);
  const int64_t i = p / sc;
  const uint8_t *from = nullptr;
  for (int k = (ch - 1 - c0) / sc; k >= 0 && ch > c0; --k) {   // the highest channel that maps here
    const int64_t ii = i - k;
    if (ii >= 0 && ii < n) {
      from = src + (int64_t)s * src_stream_stride + (ii * ch + c0 + (int64_t)sc * k) * bps;
      break;
    }
  }
  if (!from && p >= (int64_t)n * sc) return;   // past the zeroed area and nobody writes it
  uint8_t *to = dst + (int64_t)s * dst_stream_stride + p * bps;
  for (int b = 0; b < bps; ++b) to[b] = from ? from[b] : 0;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess) {                                                            \
      fprintf(stderr, "iamf_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(_e), \
              __FILE__, __LINE__);                                                     \
      return IAMF_HIP_ERR_DEVICE;                                                      \
    }                                                                                  \
  } while (0)

struct TableEntry {
  uint32_t kind, in_id, out_id;
  int32_t channels, lfe1, lfe2, m, n;
  uint32_t offset;
};

extern "C" const uint8_t _binary_rdr_tables_bin_start[];
extern "C" const uint8_t _binary_rdr_tables_bin_end[];
extern "C" const uint8_t _binary_rdr_tables_tv_bin_start[];   // the -DSAMSUNG_TV build's tables (m2m_rdr.c:36-830)
extern "C" const uint8_t _binary_rdr_tables_tv_bin_end[];

struct Tables {
  int n = 0;
  const TableEntry *ents = nullptr;
  const float *data = nullptr;
  bool ok = false;
  explicit Tables(bool tv) {
    const uint8_t *b = tv ? _binary_rdr_tables_tv_bin_start : _binary_rdr_tables_bin_start;
    const size_t sz = tv ? (size_t)(_binary_rdr_tables_tv_bin_end - _binary_rdr_tables_tv_bin_start)
                         : (size_t)(_binary_rdr_tables_bin_end - _binary_rdr_tables_bin_start);
    if (sz < 12 || memcmp(b, "IARDRTB1", 8) != 0) return;
    uint32_t cnt;
    memcpy(&cnt, b + 8, 4);
    n = (int)cnt;
    ents = reinterpret_cast<const TableEntry *>(b + 12);
    data = reinterpret_cast<const float *>(b + 12 + sizeof(TableEntry) * cnt);
    ok = true;
  }
};

const Tables &tables(bool tv) {
  static Tables t(false), t_tv(true);
  return tv ? t_tv : t;
}

int find_matrix(int kind, int in_id, int out_id, iamf_hip_matrix *out, bool tv = false) {
  const Tables &t = tables(tv);
  if (!t.ok || !out) return -1;
  for (int i = 0; i < t.n; ++i) {  // first match in table order, as the reference searches
    const TableEntry &e = t.ents[i];
    if ((int)e.kind == kind && (int)e.in_id == in_id && (int)e.out_id == out_id) {
      out->kind = kind;
      out->in_id = in_id;
      out->out_id = out_id;
      out->channels = e.channels;
      out->lfe1 = e.lfe1;
      out->lfe2 = e.lfe2;
      out->m = e.m;
      out->n = e.n;
      out->mat = t.data + e.offset;
      return 0;
    }
  }
  return -1;
}

// audio_effect_peak_limiter.c:267-271
float ease(float x) {
  if (1.0 < x) return 1.0f;
  if (x < 0) return 0.0f;
  return 1.0f - powf(x - 1, 2.0);
}

}  // namespace

struct iamf_hip_batch {
  iamf_hip_batch_config cfg;
  int device = 0;                    // the HIP device the batch was created on; every later call must run on it
  hipEvent_t done = nullptr;         // recorded behind every render / flush on the caller's stream: the synchronous
                                     // setters and destroy wait for IT, so the caller's stream may be gone by then
  bool rendered = false;
  int m = 0, n_feeds = 0;
  int32_t src_feed[kMaxOut];
  uint32_t nz_mask[6] = {0, 0, 0, 0, 0, 0};
  int sparse = 0;
  int32_t *d_src_feed = nullptr;
  float thr = 0.f;
  int n_atk = 0, n_end = 0;
  std::vector<int64_t> spos;        // samples consumed, per stream (streams advance together unless the range calls are used)
  std::vector<uint8_t> sflushed;    // per stream: the limiter's tail has been emitted
  bool any_rendered = false;        // the setters that must precede the first render check this
  bool lp_scale_ok = false;         // every non-zero weight w has w * 2^-15 exact and w * 2^-15 * sample normal (fused LPCM form)
  bool lp2_scale_ok = false;        // the same for the second element's matrix (iamf_hip_batch_set_second_element)
  float *d_matrix = nullptr, *d_gains = nullptr, *d_ctab = nullptr, *d_ring_y = nullptr,
        *d_ring_pm = nullptr;
  LimState *d_lim = nullptr;
  std::vector<float> h_gains;
  // second element / down-mixer
  bool has2 = false;
  int m2 = 0;
  float *d_matrix2 = nullptr, *d_gains2 = nullptr;
  int32_t *d_src_feed2 = nullptr, *d_dmx_tab = nullptr;
  bool dmx = false;
  int dmx_n_in = 0, dmx_n_out = 0;
  float *d_pre = nullptr;
  int pre_l = 0;
  std::vector<float> h_fm;          // host copy of d_matrix ([n_feeds][m])
  float *d_matrix_pre = nullptr;    // [n_feeds][pre_l]: renderer matrix x de-mapping matrix (tolerance mode)
  uint32_t nz_mask_pre[6] = {0, 0, 0, 0, 0, 0};
  int sparse_pre = 0;
  bool demix = false;
  int demix_steps = 0, demix_skip = 0, demix_layout = 0, demix_gmask = 0, demix_w4 = 0;
  int32_t *d_demix_tab = nullptr;
  float *d_demix_ftab = nullptr;
  bool fir = false;
  int fir_taps = 0;
  float *d_fir_hist[2] = {nullptr, nullptr};
  void *d_fir_h16 = nullptr;    // split-f16 filter tables (render_fir16.hpp)
  float *d_fir_pq = nullptr, *d_fir_tw = nullptr;   // spectra and twiddles of the FFT stage (render_fir_fft.hpp)
  float *d_fir_zero = nullptr;                      // m * frame size zero floats for that stage
  float *d_fir_pre[2] = {nullptr, nullptr};         // the history at the input's channel stride (RenderParams::fir_pre), or null
  size_t fir_pre_bytes = 0;
  float *d_fir_y = nullptr;                         // [n_streams][2][total] f32: its output when it runs as its own kernel
  size_t fir_y_bytes = 0;
  // iamf_hip_batch_render_lpcm, calls the fused kernel does not take: the unpacked element and the unpacker's {first, count}
  float *d_lp_in = nullptr;
  size_t lp_in_bytes = 0;
  // iamf_hip_batch_render_lpcm_mix, unfused: the unpacked second element
  float *d_lp_in2 = nullptr;
  size_t lp_in2_bytes = 0;
  float *d_fir_id = nullptr;                        // 2 x 2 identity + slot map for the limiter / pack kernel behind it
  int32_t *d_fir_id_feed = nullptr;
  float fir_inv_scale = 1.f;
  int fir_cur = 0;
  // HOA LFE generator (render_lfe.hpp)
  bool lfe = false;
  float lfe_a1 = 0.f, lfe_a2 = 0.f, lfe_a3 = 0.f, lfe_b1 = 0.f, lfe_b2 = 0.f;
  double lfe_div = 0.0;
  float *d_lfe_state = nullptr, *d_lfe_next = nullptr, *d_lfe_u = nullptr;
  bool lfe_shared = false;   // d_lfe_state / d_lfe_next belong to another batch (iamf_hip_batch_share_lfe_state)
  size_t lfe_u_bytes = 0;
  // fixed PCM channel stride (cfg.pcm_stride_channels): the kernels pack into d_nat, restride_kernel re-lays
  uint8_t *d_nat = nullptr;
  size_t nat_bytes = 0;
  uint8_t *d_dump = nullptr;   // RenderParams::dump
};

namespace {

// every entry point that touches device state: the caller's current device must be the batch's
bool on_batch_device(const iamf_hip_batch *b) {
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess && dev == b->device;
}

// the setters copy into buffers a queued render may still be reading (renders are asynchronous on the
// caller's stream, which may be non-blocking with respect to the null stream): wait for the batch's own
// event behind the last render (not for the stream handle, which the caller may have destroyed since)
int quiesce(iamf_hip_batch *b) {
  if (b->rendered) HIPCHK(hipEventSynchronize(b->done));
  return IAMF_HIP_OK;
}

// the channels of element 0 as the caller hands them over: in front of the projection's de-mapping where there is one
int element_channels(const iamf_hip_batch *b) { return b->d_pre ? b->pre_l : b->m; }

// streams [s0, s0 + cnt) lie in the batch
bool range_ok(const iamf_hip_batch *b, int32_t s0, int32_t cnt) {
  return s0 >= 0 && cnt > 0 && (int64_t)s0 + cnt <= b->cfg.n_streams;
}

// A scratch buffer of the batch that grows with the largest call seen: *ptr with *have bytes, of which the call on `st` needs
// need_bytes.  The old buffer may still be read by a render queued earlier, on another stream perhaps: wait for the batch's
// event and for the call's stream, then free it.  *ptr and *have are valid after every failure (null and 0 once the old
// buffer is gone).  zero: a new buffer is cleared on the call's stream (a null-stream memset is not ordered with a
// non-blocking stream).
template <class T>
int grow_scratch(iamf_hip_batch *b, hipStream_t st, T **ptr, size_t *have, size_t need_bytes, bool zero = false) {
  if (need_bytes <= *have) return IAMF_HIP_OK;
  const int q = quiesce(b);
  if (q != IAMF_HIP_OK) return q;
  HIPCHK(hipStreamSynchronize(st));
  (void)hipFree(*ptr);
  *ptr = nullptr;
  *have = 0;
  HIPCHK(hipMalloc(ptr, need_bytes));
  if (zero) HIPCHK(hipMemsetAsync(*ptr, 0, need_bytes, st));
  *have = need_bytes;
  return IAMF_HIP_OK;
}

int reset_state(iamf_hip_batch *b) {
  const int ns = b->cfg.n_streams;
  std::vector<LimState> init((size_t)ns);
  for (auto &l : init) {
    // audio_effect_peak_limiter.c:211-235: gain 1, targets -1, currentTC -1 (idle)
    l.g = 1.0f;
    l.gs = -1.0f;
    l.ge = -1.0f;
    l.n = b->n_end;
  }
  HIPCHK(hipMemcpy(b->d_lim, init.data(), sizeof(LimState) * ns, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(b->d_ring_y, 0, sizeof(float) * (size_t)ns * b->cfg.out_channels * kSave));
  HIPCHK(hipMemset(b->d_ring_pm, 0, sizeof(float) * (size_t)ns * kSave));
  if (b->fir) {
    const size_t hb = sizeof(float) * (size_t)ns * b->m * 256;
    HIPCHK(hipMemset(b->d_fir_hist[0], 0, hb));
    HIPCHK(hipMemset(b->d_fir_hist[1], 0, hb));
    for (float *q : b->d_fir_pre)
      if (q) HIPCHK(hipMemset(q, 0, b->fir_pre_bytes));
  }
  if (b->lfe && !b->lfe_shared) {  // lfefilter_init zeroes both histories (h2m_rdr.c:1210-1211)
    HIPCHK(hipMemset(b->d_lfe_state, 0, sizeof(float) * 4 * (size_t)ns));
    HIPCHK(hipMemset(b->d_lfe_next, 0, sizeof(float) * 2 * (size_t)ns));
  }
  // the copy and the memsets above went to the null stream: the caller's next render may run on a stream that does not
  // wait for it, so the fresh state is in place before create / reset return
  HIPCHK(hipStreamSynchronize(nullptr));
  b->spos.assign((size_t)ns, 0);
  b->sflushed.assign((size_t)ns, 0);
  b->any_rendered = false;
  return IAMF_HIP_OK;
}

template <int M>
void launch_m(const RenderParams &p, dim3 grid, size_t lds_bytes, hipStream_t st) {
  hipLaunchKernelGGL(render_kernel<M>, grid, dim3(kChunk), lds_bytes, st, p);
}

// limiter off, one matrix-rendered element, constant gains (render_nolim.hpp): (streams, chunks of 1024 sample-frames)
template <int M>
void launch_nolim_m(const RenderParams &p, hipStream_t st) {
  const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
  dim3 grid((unsigned)p.n_launch, (unsigned)((p.total + kNlChunk - 1) / kNlChunk));
  hipLaunchKernelGGL(render_nolim_kernel<M>, grid, dim3(256), (size_t)kNlChunk * p.out_ch * bytes, st, p);
}

template <int M, int OC>
void launch_fast_mc(const RenderParams &p, bool mixing, dim3 grid, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)fast_lds_floats(OC, M);
  if (mixing) launch_big_lds<&render_fast_kernel<M, OC, 0, false, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
  else launch_big_lds<&render_fast_kernel<M, OC>, 80 * 1024>(grid, dim3(256), lds, st, p);
}
template <int M>
void launch_fast_m(const RenderParams &p, bool mixing, dim3 grid, hipStream_t st) {
  if (p.out_ch == 1) launch_fast_mc<M, 1>(p, mixing, grid, st);
  else launch_fast_mc<M, 2>(p, mixing, grid, st);
}

template <int M, int OC>
void launch_fast_down_mc(const RenderParams &p, dim3 grid, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)fast_lds_floats(OC, M);
  launch_big_lds<&render_fast_kernel<M, OC, 0, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
}

template <int M>
void launch_wide_m(const RenderParams &p, dim3 grid, hipStream_t st) {
  const size_t lds = sizeof(float) * (size_t)wide_lds_floats(p.out_ch, M);
  if (p.use_mfma) launch_big_lds<&render_wide_kernel<M, true>, 80 * 1024>(grid, dim3(256), lds, st, p);
  else launch_big_lds<&render_wide_kernel<M, false>, 80 * 1024>(grid, dim3(256), lds, st, p);
}

// Family::FirSplit: (1) the FFT stage for every hop of every stream -> y in HBM (overlap-save blocks are independent: one
// grid); (2) gains, limiter, pack = the two-channel matrix kernel with the identity over y (one "frame" of `total` samples
// per stream).  1024 streams x 64 frames: 1.5 ms (vector ALU) + 0.6 ms (the limiter's chain, four workgroups a CU).
// Tried and dropped, both bit-exact: slices of STREAMS with the limiter kernel of one slice beside the stage of the next on
// a second stream (23.8 against 33.2 Gsamples/s: the limiter kernel takes 0.6 ms for 256 streams as for 1024), and slices of
// TIME the same way (31.1: four resident limiter workgroups and two stage workgroups each want all 512 VGPRs of a SIMD
// lane, so the two kernels take turns instead of overlapping).
int launch_fir_split(const RenderParams &p, int m, dim3 grid, hipStream_t st) {
  if (!dispatch(FirHomeM{}, m, [&](auto M) { launch_fft_m<M.value>(p, st); }) && !iamf_hip_fir_m2b_launch_fft(&p, m, st))
    return IAMF_HIP_ERR_INTERNAL;
  HIPCHK(hipGetLastError());
  RenderParams q = p;
  q.in = p.fir_y;                               // planar [2][total]: channel stride = "frame size" = total
  q.in_stream_stride = 2 * (int64_t)p.total;
  q.in_frame_stride = 2 * (int64_t)p.total;
  q.frame_size = p.total;
  q.matrix = p.fir_id_matrix;
  q.src_feed = p.fir_id_feed;
  q.n_feeds = 2;
  q.fir_taps = 0;
  q.fir_hist = q.fir_hist_next = nullptr;
  launch_fast_m<2>(q, false, grid, st);
  return IAMF_HIP_OK;
}

// Runs the kernel pick_route (render_route.hpp) names.  `launched` is false only if a launcher's instance list and the
// one the route was picked by disagree, which sharing the lists rules out.
// (p: the block every kernel takes and, behind it, what Family::LpcmMix alone reads)
int launch(const RenderMixParams &p, int m, size_t lds_bytes, hipStream_t st) {
  const Route r = pick_route(p, m);
  const dim3 grid((unsigned)p.n_launch);
  bool launched = false;
  switch (r.family) {
    case Family::Refused: return r.err;
    case Family::Lpcm: launched = iamf_hip_fast_lpcm_launch(&p, m, r.variant, st); break;
    case Family::Lpcm24: launched = iamf_hip_fast_lpcm24_launch(&p, m, r.variant, st); break;
    case Family::LpcmCoupled: launched = iamf_hip_fast_lpcm_coupled_launch(&p, m, r.variant, st); break;
    case Family::Lpcm24Coupled: launched = iamf_hip_fast_lpcm24_coupled_launch(&p, m, r.variant, st); break;
    case Family::LpcmMix:
      launched = p.lpcm_coupled ? iamf_hip_fast_lpcm_mix_coupled_launch(&p, m, r.variant, st) : iamf_hip_fast_lpcm_mix_launch(&p, m, r.variant, st);
      break;
    case Family::Lpcm24Mix:
      launched = p.lpcm_coupled ? iamf_hip_fast_lpcm24_mix_coupled_launch(&p, m, r.variant, st) : iamf_hip_fast_lpcm24_mix_launch(&p, m, r.variant, st);
      break;
    case Family::FastInterleaved: launched = iamf_hip_fast_interleaved_launch(&p, m, st); break;
    case Family::FastRagged: launched = iamf_hip_fast_ragged_launch(&p, m, st); break;
    case Family::PacketsRagged:   // the four single-element packet forms, a unit each
      if (p.lpcm_bytes == 3) launched = p.lpcm_coupled ? iamf_hip_fast_packets_ragged24_coupled_launch(&p, m, st) : iamf_hip_fast_packets_ragged24_launch(&p, m, st);
      else launched = p.lpcm_coupled ? iamf_hip_fast_packets_ragged_coupled_launch(&p, m, st) : iamf_hip_fast_packets_ragged_launch(&p, m, st);
      break;
    case Family::PacketsMixRagged:   // the four two-element packet forms, a unit each
      if (p.lpcm_bytes == 3)
        launched = p.lpcm_coupled ? iamf_hip_fast_packets_mix_ragged24_coupled_launch(&p, m, r.variant, st) : iamf_hip_fast_packets_mix_ragged24_launch(&p, m, r.variant, st);
      else
        launched = p.lpcm_coupled ? iamf_hip_fast_packets_mix_ragged_coupled_launch(&p, m, r.variant, st) : iamf_hip_fast_packets_mix_ragged_launch(&p, m, r.variant, st);
      break;
    case Family::NolimPackets:   // the limiter-less renderer over packets: a unit per sample size
      launched = p.lpcm_bytes == 3 ? iamf_hip_nolim_packets24_launch(&p, m, st) : iamf_hip_nolim_packets_launch(&p, m, st);
      break;
    case Family::NolimPacketsMix:   // the same over both elements' packets
      launched = p.lpcm_bytes == 3 ? iamf_hip_nolim_packets24_mix_launch(&p, m, r.variant, st) : iamf_hip_nolim_packets_mix_launch(&p, m, r.variant, st);
      break;
    case Family::FirSplit: {
      const int e = launch_fir_split(p, m, grid, st);
      if (e != IAMF_HIP_OK) return e;
      launched = true;
      break;
    }
    case Family::FirFused:  // channel-based elements (M2B), the loudspeaker layouts' channel counts: a unit of their own
      launched = dispatch(FirHomeM{}, m, [&](auto M) { launch_fir_m<M.value>(p, r.variant, st); }) ||
                 iamf_hip_fir_m2b_launch(&p, m, r.variant, st);
      break;
    case Family::FastDown:
      launched = dispatch(FastDownMC{}, mc(m, p.out_ch), [&](auto V) { launch_fast_down_mc<mc_m(V.value), mc_c(V.value)>(p, grid, st); });
      break;
    case Family::Wide4Lfe: launched = iamf_hip_wide4_lfe_launch(&p, m, st); break;
    case Family::Wide4Mix: launched = iamf_hip_wide4_mix_launch(&p, m, st); break;
    case Family::Wide4:
    case Family::Wide4Demix:
    case Family::Wide4Down: launched = iamf_hip_wide4_launch(&p, m, st); break;
    case Family::Nolim: launched = dispatch(NolimM{}, m, [&](auto M) { launch_nolim_m<M.value>(p, st); }); break;
    case Family::Fast: launched = dispatch(FastM{}, m, [&](auto M) { launch_fast_m<M.value>(p, r.variant != 0, grid, st); }); break;
    case Family::Wide: launched = dispatch(WideM{}, m, [&](auto M) { launch_wide_m<M.value>(p, grid, st); }); break;
    case Family::Generic: launched = dispatch(GenericM{}, m, [&](auto M) { launch_m<M.value>(p, grid, lds_bytes, st); }); break;
  }
  if (!launched) return IAMF_HIP_ERR_INTERNAL;
  HIPCHK(hipGetLastError());
  const RouteKey k = route_key(r, p, m);   // the tally of iamf_hip_route_tally
  iamf_hip_route_count(k.set, k.family, k.variant, k.m, k.c, k.k);
  if (r.family == Family::FirSplit) iamf_hip_route_count(0, IAMF_HIP_ROUTE_FAST, 0, 2, 2, 0);
  return IAMF_HIP_OK;
}

// layout tables of the down-mixer: playback channel order per IAChannelLayoutType (reference
// IAMF_utils.c:117-133) and surround / top counts (:157-161)
const int kLayoutCount[9] = {1, 2, 6, 8, 10, 8, 10, 12, 6};
const int kLayoutCh[9][12] = {
    {kChMono},
    {kChL2, kChR2},
    {kChL7, kChR7, kChC, kChLFE, kChSL5, kChSR5},
    {kChL7, kChR7, kChC, kChLFE, kChSL5, kChSR5, kChHL, kChHR},
    {kChL7, kChR7, kChC, kChLFE, kChSL5, kChSR5, kChHFL, kChHFR, kChHBL, kChHBR},
    {kChL7, kChR7, kChC, kChLFE, kChSL7, kChSR7, kChBL7, kChBR7},
    {kChL7, kChR7, kChC, kChLFE, kChSL7, kChSR7, kChBL7, kChBR7, kChHL, kChHR},
    {kChL7, kChR7, kChC, kChLFE, kChSL7, kChSR7, kChBL7, kChBR7, kChHFL, kChHFR, kChHBL, kChHBR},
    {kChL3, kChR3, kChC, kChLFE, kChTL, kChTR},
};
const int kLayoutSurround[9] = {1, 2, 5, 5, 5, 7, 7, 7, 3};
const int kLayoutTop[9] = {0, 0, 0, 2, 4, 0, 2, 4, 2};

// streams [s0, s0 + cnt) of the batch; they must stand at the same position (samples consumed so far)
// Element 0 as LPCM packets for the fused kernel (render_fast_kernel<.., LP>, iamf_render_lpcm.hip).  render_call
// returns kNotFused — before it has changed or launched anything — when the call is not one that kernel takes; the caller
// (iamf_hip_batch_render_lpcm) then unpacks to f32 and renders as usual.
struct LpcmIn {
  const uint8_t *raw;
  int64_t stream_stride, frame_stride;
  int32_t off[16];
  int32_t bytes;   // per sample: 2 or 3 (lpcm_form.hpp)
  int32_t coupled; // 1: LpcmForm::S16C, off[] of a pair's two channels 2 bytes apart; 2: LpcmForm::S24C, 3 bytes apart
};
constexpr int kNotFused = INT32_MIN;
// Which entry a call came through: what that entry's own kernel form may take, everything else as without.  Ordered — each
// packet form may take what the one in front of it takes: a limiter-less packet call is a ragged packet call is a packet call.
// Whether the call is a mix is a matter of a second element's packets being there (lp2), not of the form.
enum class CallForm {
  Plain,           // iamf_hip_batch_render_range and every entry on top of it
  Interleaved,     // iamf_hip_batch_render_interleaved: the interleaved form of the fast kernel
  Ragged,          // iamf_hip_batch_render_ragged: the planar ragged form
  Lpcm,            // iamf_hip_batch_render_lpcm_range, _lpcm_mix: the forms lpcm_form() names
  Packets,         // iamf_hip_batch_render_packets, _packets_mix: the forms lpcm_form_packets() names (24-bit coupled, 24-bit mix)
  PacketsRagged,   // iamf_hip_batch_render_packets_ragged, _packets_mix_ragged: and the ragged packet forms (kCallPacketsRagged,
                   // kCallPacketsMixRagged)
  PacketsNolim,    // iamf_hip_batch_render_packets_nolim, _packets_mix_nolim: and, first, the packet-fed limiter-less renderer
                   // (kCallPacketsNolim, kCallPacketsMixNolim)
};
// the family a packet call must route to for a fused kernel to read its packets (lp2: the second element's, or null;
// ragged: the call carries the mark of a ragged packet form and is no whole number of 64-sample blocks, which only that form takes)
Family lpcm_family(const LpcmIn *lp, const LpcmIn *lp2, bool ragged) {
  if (ragged) return lp2 ? Family::PacketsMixRagged : Family::PacketsRagged;
  if (lp2) return lp->bytes == 3 ? Family::Lpcm24Mix : Family::LpcmMix;   // (24-bit: iamf_hip_batch_render_packets_mix only)
  if (lp->coupled == 2) return Family::Lpcm24Coupled;
  if (lp->coupled) return Family::LpcmCoupled;
  return lp->bytes == 3 ? Family::Lpcm24 : Family::Lpcm;
}

// HOA LFE generator over `ltotal` samples of the element rows at d_in: feed-forward part in parallel, the recurrence one lane
// per stream, both on the caller's stream (render_lfe.hpp); the output lies in b->d_lfe_u (t4 quads per stream), the filter
// state of streams [s0, s0 + cnt) has moved on.
int lfe_prepass(iamf_hip_batch *b, const float *d_in, int64_t in_stream_stride, int64_t in_frame_stride, int ltotal,
                hipStream_t st, int s0, int cnt, int *t4_out) {
  const int ns = b->cfg.n_streams, nb = (ns + 63) / 64, t4 = (ltotal + 3) / 4;
  const int gr = grow_scratch(b, st, &b->d_lfe_u, &b->lfe_u_bytes, sizeof(float) * (size_t)nb * t4 * 64 * 4);
  if (gr != IAMF_HIP_OK) return gr;
  LfeParams lp;
  memset(&lp, 0, sizeof(lp));
  lp.in = d_in;
  lp.in_stream_stride = in_stream_stride;
  lp.in_frame_stride = in_frame_stride;
  lp.pre_matrix = b->d_pre;   // projection mode: W is channel 0 AFTER the de-mapping, in every mode
  lp.pre_l = b->pre_l;
  lp.pre_m = b->m;
  lp.frame_size = b->cfg.frame_size;
  lp.n_streams = ns;
  lp.total = ltotal;
  lp.t4 = t4;
  lp.a1 = b->lfe_a1; lp.a2 = b->lfe_a2; lp.a3 = b->lfe_a3; lp.b1 = b->lfe_b1; lp.b2 = b->lfe_b2;
  lp.state = b->d_lfe_state;
  lp.state_next = b->d_lfe_next;
  lp.u_t = reinterpret_cast<float4 *>(b->d_lfe_u);
  lp.s_first = s0;
  lp.s_count = cnt;
  hipLaunchKernelGGL(lfe_ff_kernel, dim3((unsigned)((t4 + kLfeTileQ - 1) / kLfeTileQ), (unsigned)nb), dim3(256), 0, st, lp);
  hipLaunchKernelGGL(lfe_chain_kernel, dim3((unsigned)nb), dim3(64), 0, st, lp);
  HIPCHK(hipGetLastError());
  *t4_out = t4;
  return IAMF_HIP_OK;
}

// A render call in three steps — prepare (checks, the kernel's parameter block, scratch that grows with the call; the LFE
// generator's pre-pass is queued here), launch, commit (positions, the FIR history flip, the re-lay of a fixed channel
// stride, the `done` event, the emitted count) — so that iamf_hip_batch_render_fanout can prepare every member, launch
// once, and commit each, and restates none of it.
struct PreparedCall {
  RenderMixParams p;   // (the part behind RenderParams: set for Family::LpcmMix and Family::Lpcm24Mix only)
  iamf_hip_render_args a;
  int m_eff;
  size_t lds;
  bool restride;
  int sc, bps;
  int64_t pos;
  int total, s0, cnt;
};

// lp: element 0 as packets of a fusable form, or null; lp2 (with lp): the second element as packets too, a.d_in2 then being a
// non-null placeholder.  form: the entry the call came through (CallForm); first: iamf_hip_lpcm_input::first_sample of a packet call.
// kNotFused comes back before anything is changed or launched.
int render_prepare(iamf_hip_batch *b, const iamf_hip_render_args &a, int total, int s0, int cnt, const LpcmIn *lp, const LpcmIn *lp2,
                   CallForm form, int first, PreparedCall &pc) {
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  const bool nolim = form == CallForm::PacketsNolim;
  // a fixed PCM channel stride: the call packs into scratch and is re-laid behind the kernel
  const int sc = b->cfg.pcm_stride_channels;
  const bool restride = sc > 0 && sc != b->cfg.out_channels;
  // (the weights' range: the limiter-less packet forms convert the samples first and need no rule, so they ask further down)
  if (lp && (b->fir || b->lfe || b->d_pre || b->demix || b->dmx || (!b->lp_scale_ok && !nolim) || getenv("IAMF_HIP_LPCM_UNFUSED")))
    return kNotFused;
  // a second element or ramps: the two-element packet form only, which also keeps away from a fixed PCM channel stride
  if (lp && !lp2 && (b->has2 || a.d_element_ramp || a.d_element2_ramp || a.d_output_ramp)) return kNotFused;
  if (lp2 && (!lp || !b->has2 || (!b->lp2_scale_ok && !nolim) || restride)) return kNotFused;
  // the coupled 24-bit form (iamf_hip_batch_render_packets) keeps away from a fixed PCM channel stride as well
  if (lp && lp->coupled == 2 && restride) return kNotFused;
  if (!range_ok(b, s0, cnt)) return IAMF_HIP_ERR_BAD_ARG;
  if (a.lfe_pre_samples < 0 || a.lfe_post_samples < 0 ||
      ((a.lfe_pre_samples || a.lfe_post_samples) &&
       (a.n_frames != 1 || (int64_t)a.lfe_pre_samples + total + a.lfe_post_samples > b->cfg.frame_size)))
    return IAMF_HIP_ERR_BAD_ARG;
  const int64_t pos = b->spos[(size_t)s0];
  for (int i = s0; i < s0 + cnt; ++i)
    if (b->spos[(size_t)i] != pos || b->sflushed[(size_t)i]) return IAMF_HIP_ERR_INVALID_STATE;
  const bool whole = s0 == 0 && cnt == b->cfg.n_streams;
  // per-batch (not per-stream) state: the FIR history ping-pong.  (The LFE generator's pre-pass takes the range: streams
  // outside it keep their filter state, round 4.)
  if (!whole && b->fir) return IAMF_HIP_ERR_UNIMPLEMENTED;
  memset(&pc.p, 0, sizeof(pc.p));
  RenderParams &p = pc.p;
  p.stream0 = s0;
  p.n_launch = cnt;
  p.in = a.d_in;
  p.in_stream_stride = a.in_stream_stride;
  p.in_frame_stride = a.in_frame_stride;
  p.pcm = static_cast<uint8_t *>(a.d_pcm);
  p.pcm_stream_stride = a.pcm_stream_stride_bytes;
  p.matrix = b->d_matrix;
  p.gains = b->d_gains;
  p.ctab = b->d_ctab;
  p.lim = b->d_lim;
  p.ring_y = b->d_ring_y;
  p.ring_pm = b->d_ring_pm;
  p.pos0 = pos;
  p.total = total;
  p.frame_size = b->cfg.frame_size;
  p.n_streams = b->cfg.n_streams;
  p.n_feeds = b->n_feeds;
  p.out_ch = b->cfg.out_channels;
  p.og_ch = (b->cfg.out_gain_channels > 0 && b->cfg.out_gain_channels < b->cfg.out_channels) ? b->cfg.out_gain_channels : b->cfg.out_channels;
  p.out_format = b->cfg.out_format;
  p.limiter_on = b->cfg.limiter_enable ? 1 : 0;
  p.loudness_on = b->cfg.loudness_enable ? 1 : 0;
  bool tolerance = false;
  {
    const int proj = b->cfg.projection;
    const char *env = getenv("IAMF_HIP_PROJECTION");  // "exact" / "mfma" override for experiments
    bool mf = proj == IAMF_HIP_PROJ_MFMA || (proj == IAMF_HIP_PROJ_AUTO && b->cfg.matrix.kind == IAMF_HIP_KIND_H2M);
    if (env && !strcmp(env, "exact")) mf = false;
    if (env && !strcmp(env, "mfma")) mf = true;
    p.use_mfma = (mf && b->n_feeds <= 32) ? 1 : 0;
    tolerance = mf;
  }
  p.n_atk = b->n_atk;
  p.n_end = b->n_end;
  p.thr = b->thr;
  p.src_feed = b->d_src_feed;
  p.dump = b->d_dump;
  for (int g = 0; g < 6; ++g) p.nz_mask[g] = b->nz_mask[g];
  p.sparse = getenv("IAMF_HIP_DENSE") ? 0 : b->sparse;
  if (b->has2 && a.d_in2) {
    p.in2 = a.d_in2;
    p.in2_stream_stride = a.in2_stream_stride;
    p.in2_frame_stride = a.in2_frame_stride;
    p.matrix2 = b->d_matrix2;
    p.src_feed2 = b->d_src_feed2;
    p.gains2 = b->d_gains2;
    p.m2 = b->m2;
  }
  p.elem_ramp = a.d_element_ramp;
  p.elem2_ramp = a.d_element2_ramp;
  p.out_ramp = a.d_output_ramp;
  p.ramp_stream_stride = a.ramp_stream_stride;
  if (b->dmx) {
    p.dmx_on = 1;
    p.dmx_frames = a.d_in ? a.d_dmx_frames : nullptr;
    p.dmx_n_in = b->dmx_n_in;
    p.dmx_n_out = b->dmx_n_out;
    p.dmx_tab = b->d_dmx_tab;
    p.dmx_in_layout = b->cfg.matrix.in_id;
    p.dmx_out_layout = b->cfg.matrix.out_id;
  }
  int m_eff = b->m;
  if (b->d_pre && a.d_in) {
    const int l = b->pre_l;
    if (tolerance && b->d_matrix_pre && FastM::has(l) && !p.in2) {  // one composed matrix, see iamf_hip_batch_set_projection
      p.matrix = b->d_matrix_pre;
      for (int g = 0; g < 6; ++g) p.nz_mask[g] = b->nz_mask_pre[g];
      p.sparse = getenv("IAMF_HIP_DENSE") ? 0 : b->sparse_pre;
      m_eff = l;
    } else {
      p.pre_matrix = b->d_pre;
      p.pre_l = b->pre_l;
    }
  }
  if (b->demix && a.d_in) {
    p.demix_on = 1;
    p.demix_steps = b->demix_steps;
    p.demix_skip = b->demix_skip;
    p.demix_tab = b->d_demix_tab;
    p.demix_ftab = b->d_demix_ftab;
    p.demix_frames = a.d_demix_frames;
    p.demix_i0 = a.n_frames == 1 ? a.demix_sample0 : 0;
    p.demix_layout = b->demix_layout;
    p.demix_gmask = b->demix_gmask;
    p.demix_w4 = b->demix_w4;
  }
  if (lp) {
    p.lpcm = lp->raw;
    p.lpcm_stream_stride = lp->stream_stride;
    p.lpcm_frame_stride = lp->frame_stride;
    for (int m = 0; m < 16; ++m) p.lpcm_off[m] = lp->off[m];
    p.lpcm_bytes = lp->bytes;
    p.lpcm_coupled = lp->coupled;
    if (lp2) {   // the kernel reads RenderMixParams; pick_route the packets' place in the in2 fields (strides in bytes)
      // 24-bit packets on both elements (iamf_hip_batch_render_packets_mix alone hands them over): the form's own values
      if (lp->bytes != lp2->bytes) return kNotFused;
      p.lpcm_mix = (lp->bytes == 3 ? 4 : 0) | (lp2->coupled ? 2 : 1);
      p.in2 = reinterpret_cast<const float *>(lp2->raw);
      p.in2_stream_stride = lp2->stream_stride;
      p.in2_frame_stride = lp2->frame_stride;
      pc.p.lpcm2 = lp2->raw;
      pc.p.lpcm2_stream_stride = lp2->stream_stride;
      pc.p.lpcm2_frame_stride = lp2->frame_stride;
      for (int m = 0; m < 4; ++m) pc.p.lpcm2_off[m] = lp2->off[m];
    }
    // The call's mark (render_params.hpp, CallMark), decided once: the limiter-less form's where the entry asks for it and its rule
    // holds (nolim_packets_shape_ok, nolim_packets_mix_shape_ok: asked of a copy that carries the mark), else the ragged form's
    // where the entry asks for it, else none.  These forms pack into the caller's buffer themselves: a fixed PCM channel stride
    // stays unfused.  Each has its own measurement and its own size cut.
    int32_t mark = kCallPlain;
    if (nolim && !restride && (lp2 ? nolim_packets_mix_fused(cnt) : nolim_packets_fused(cnt))) {
      RenderMixParams q = pc.p;
      q.ragged = lp2 ? kCallPacketsMixNolim : kCallPacketsNolim;
      q.demix_i0 = first;
      if (pick_route(q, m_eff).family == (lp2 ? Family::NolimPacketsMix : Family::NolimPackets)) mark = q.ragged;
    }
    const bool nolim_taken = mark != kCallPlain;
    if (!nolim_taken && (!b->lp_scale_ok || (lp2 && !b->lp2_scale_ok))) return kNotFused;
    // (the size cuts of the whole-block forms say nothing about a ragged call of a ragged packet entry, which no whole-block form
    //  takes, nor about a call the limiter-less renderer takes)
    if (!nolim_taken && !(form >= CallForm::PacketsRagged && (total & 63))) {   // a size at which the fused form measured no faster
      if (!lp2 && lp->bytes == 3 && !lp->coupled && !lpcm24_fused(cnt)) return kNotFused;
      if (!lp2 && lp->coupled == 1 && !lpcm_coupled_fused(cnt)) return kNotFused;
      if (!lp2 && lp->coupled == 2 && !lpcm24_coupled_fused(cnt)) return kNotFused;
      if (lp2 && !(lp->bytes == 3 ? lpcm24_mix_fused(cnt) : lpcm_mix_fused(cnt))) return kNotFused;
    }
    if (!nolim_taken && form >= CallForm::PacketsRagged && !restride && (lp2 ? packets_mix_ragged_fused(cnt) : packets_ragged_fused(cnt)))
      mark = lp2 ? kCallPacketsMixRagged : kCallPacketsRagged;
    if (mark != kCallPlain) {   // with the trimmed frame's first sample where the marked rules look for it (call_first_sample)
      p.ragged = mark;
      p.demix_i0 = first;
    }
    if (!nolim_taken && pick_route(p, m_eff).family != lpcm_family(lp, lp2, mark != kCallPlain && (total & 63))) return kNotFused;
  }
  if (b->fir) {
    p.fir_taps = b->fir_taps;
    p.fir_hist = b->d_fir_hist[b->fir_cur];
    p.fir_hist_next = b->d_fir_hist[b->fir_cur ^ 1];
    p.fir_h16 = b->d_fir_h16;
    p.fir_inv_scale = b->fir_inv_scale;
    p.fir_pq = b->d_fir_pq;
    p.fir_tw = b->d_fir_tw;
    p.fir_zero = b->d_fir_zero;
    p.fir_pre = b->d_fir_pre[b->fir_cur];
    p.fir_pre_next = b->d_fir_pre[b->fir_cur ^ 1];
    if (a.d_in && b->d_fir_pq && (b->cfg.frame_size & 63) == 0 && !getenv("IAMF_HIP_FIR_FUSED") && !getenv("IAMF_HIP_FIR_F16") &&
        !getenv("IAMF_HIP_FIR_F32")) {
      // the FFT stage's output of this call, [n_streams][2][total]
      const int gr = grow_scratch(b, static_cast<hipStream_t>(a.stream), &b->d_fir_y, &b->fir_y_bytes,
                                  sizeof(float) * (size_t)b->cfg.n_streams * 2 * (size_t)total);
      if (gr != IAMF_HIP_OK) return gr;
      p.fir_y = b->d_fir_y;
      p.fir_id_matrix = b->d_fir_id;
      p.fir_id_feed = b->d_fir_id_feed;
    }
  }
  if (b->lfe && a.d_in && total > 0) {
    // a trimmed frame: the filter also runs over what is cut off (iamf_hip_render_args::lfe_pre_samples; checked above)
    const int lpre = a.lfe_pre_samples, lpost = a.lfe_post_samples;
    int t4 = 0;
    const int rc = lfe_prepass(b, a.d_in - lpre, a.in_stream_stride, a.in_frame_stride, lpre + total + lpost,
                               static_cast<hipStream_t>(a.stream), s0, cnt, &t4);
    if (rc) return rc;
    p.lfe = b->d_lfe_u;
    p.lfe_t4 = t4;
    p.lfe_k0 = lpre;
    p.lfe_div = b->lfe_div;
    for (int c = 0; c < b->cfg.out_channels && c < 32; ++c)
      if (b->src_feed[c] == -2) p.lfe_mask |= 1 << c;
  }
  const size_t lds = sizeof(float) * ((size_t)(p.out_ch + 2) * kRing + 3 * kChunk + kHead + 4 +
                                      ((b->dmx || b->demix) ? (size_t)kChCount * kChunk : 0));
  const int bps = iamf_hip_format_bytes(p.out_format);
  if (restride) {  // pack naturally into scratch, then re-lay with the fixed channel stride
    const size_t per_stream = (size_t)(total > kDelay ? total : kDelay) * p.out_ch * bps;
    const int gr = grow_scratch(b, static_cast<hipStream_t>(a.stream), &b->d_nat, &b->nat_bytes, per_stream * (size_t)p.n_streams);
    if (gr != IAMF_HIP_OK) return gr;
    p.pcm = b->d_nat;
    p.pcm_stream_stride = (int64_t)per_stream;
  }
  // the interleaved form packs into the caller's buffer itself and knows no LFE slot; pick_route has the call's other rules
  p.interleaved = (form == CallForm::Interleaved && !restride && !b->lfe && interleaved_fused(cnt)) ? 1 : 0;
  // so does the planar ragged form (an LFE slot: pick_route sees p.lfe)
  if (form == CallForm::Ragged && !restride && ragged_fused(cnt)) p.ragged = kCallRagged;
  pc.a = a;
  pc.m_eff = m_eff;
  pc.lds = lds;
  pc.restride = restride;
  pc.sc = sc;
  pc.bps = bps;
  pc.pos = pos;
  pc.total = total;
  pc.s0 = s0;
  pc.cnt = cnt;
  return IAMF_HIP_OK;
}

int render_launch(const PreparedCall &pc) {
  return launch(pc.p, pc.m_eff, pc.lds, static_cast<hipStream_t>(pc.a.stream));
}

// behind a launch that succeeded: returns the sample-frames the call emitted per stream
int render_commit(iamf_hip_batch *b, const PreparedCall &pc) {
  const RenderParams &p = pc.p;
  const iamf_hip_render_args &a = pc.a;
  const bool restride = pc.restride;
  const int sc = pc.sc, bps = pc.bps, total = pc.total, s0 = pc.s0, cnt = pc.cnt;
  const int64_t pos = pc.pos;
  if (b->fir && p.in) b->fir_cur ^= 1;
  const int64_t before = p.limiter_on ? (pos > kDelay ? pos - kDelay : 0) : pos;
  for (int i = s0; i < s0 + cnt; ++i) b->spos[(size_t)i] = pos + total;
  b->any_rendered = true;
  const int64_t after = p.limiter_on ? (pos + total > kDelay ? pos + total - kDelay : 0) : pos + total;
  const int n_emit = (int)(after - before);
  if (restride && n_emit > 0) {
    const int64_t n_out = (int64_t)n_emit * sc + (p.out_ch > sc ? p.out_ch - sc : 0);
    hipLaunchKernelGGL(restride_kernel, dim3((unsigned)((n_out + 255) / 256), (unsigned)cnt), dim3(256), 0,
                       static_cast<hipStream_t>(a.stream), b->d_nat, p.pcm_stream_stride,
                       static_cast<uint8_t *>(a.d_pcm), a.pcm_stream_stride_bytes, n_emit, p.out_ch, sc, bps, s0);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipEventRecord(b->done, static_cast<hipStream_t>(a.stream)));
  b->rendered = true;
  return n_emit;
}

// a prepared call: launch, then commit.  The sample-frames emitted per stream, or the launch's error
int render_finish(iamf_hip_batch *b, const PreparedCall &pc) {
  const int r = render_launch(pc);
  return r != IAMF_HIP_OK ? r : render_commit(b, pc);
}

// the whole call (lp, lp2, form, first: as render_prepare, whose kNotFused comes back before anything is changed or launched)
int render_call(iamf_hip_batch *b, const iamf_hip_render_args &a, int total, int s0, int cnt, const LpcmIn *lp, const LpcmIn *lp2,
                CallForm form, int first) {
  PreparedCall pc;
  const int r = render_prepare(b, a, total, s0, cnt, lp, lp2, form, first, pc);
  return r != IAMF_HIP_OK ? r : render_finish(b, pc);
}

// What the six packet entries (iamf_hip_packet_call, iamf_hip_packet_mix_call) ask of their call block in front of everything else:
// the reserved words zero, and no f32 input beside the packets
template <class Call>
bool packet_call_ok(const iamf_hip_batch *b, const Call *call) {
  if (!b || !call || call->reserved[0] || call->reserved[1] || call->reserved[2] || call->reserved[3]) return false;
  return !call->args.d_in && !call->args.d_in2;
}

// feed-major copy of a renderer matrix and its output-slot map (h2m_rdr.c:1114-1150 keeps the
// slots lfe1/lfe2 free - the comparison is against the SOURCE index - and zeroes them; every
// other slot no feed reaches stays silent; m2m feeds map 1:1)
void build_feed_map(const iamf_hip_matrix &mx, int out_channels, std::vector<float> &fm, int32_t *src_feed) {
  for (int i = 0; i < kMaxOut; ++i) src_feed[i] = -1;
  for (int i = 0; i < mx.n; ++i) {
    int d = i;
    if (mx.kind == IAMF_HIP_KIND_H2M && (mx.lfe1 >= 0 || mx.lfe2 >= 0)) {
      if (mx.lfe1 >= 0 && mx.lfe1 <= i) ++d;
      if (mx.lfe2 >= 0 && mx.lfe2 <= i) ++d;
    }
    if (d < out_channels) src_feed[d] = i;
  }
  if (mx.kind == IAMF_HIP_KIND_H2M) {
    if (mx.lfe1 >= 0 && mx.lfe1 < out_channels) src_feed[mx.lfe1] = -1;
    if (mx.lfe2 >= 0 && mx.lfe2 < out_channels) src_feed[mx.lfe2] = -1;
  }
  fm.assign((size_t)mx.m * mx.n, 0.f);
  for (int f = 0; f < mx.n; ++f)
    for (int k = 0; k < mx.m; ++k)
      fm[(size_t)f * mx.m + k] = mx.kind == IAMF_HIP_KIND_H2M ? mx.mat[f * mx.m + k] : mx.mat[k * mx.n + f];
}

}  // namespace

extern "C" {

int iamf_hip_get_h2m_matrix(int order, int out_id, iamf_hip_matrix *out) {
  return find_matrix(IAMF_HIP_KIND_H2M, order, out_id, out);
}

int iamf_hip_get_m2m_matrix(int in_id, int out_id, iamf_hip_matrix *out) {
  return find_matrix(IAMF_HIP_KIND_M2M, in_id, out_id, out);
}

int iamf_hip_get_m2m_matrix_variant(int variant, int in_id, int out_id, iamf_hip_matrix *out) {
  if (variant != IAMF_HIP_VARIANT_DEFAULT && variant != IAMF_HIP_VARIANT_SAMSUNG_TV) return -1;
  return find_matrix(IAMF_HIP_KIND_M2M, in_id, out_id, out, variant == IAMF_HIP_VARIANT_SAMSUNG_TV);
}

int iamf_hip_layout_channels(int out_id) {
  switch (out_id) {
    case IAMF_HIP_SS_A: return 2;
    case IAMF_HIP_SS_B: return 6;
    case IAMF_HIP_SS_C: return 8;
    case IAMF_HIP_SS_D: return 10;
    case IAMF_HIP_SS_E: return 11;
    case IAMF_HIP_SS_F: return 12;
    case IAMF_HIP_SS_G: return 14;
    case IAMF_HIP_SS_H: return 24;
    case IAMF_HIP_SS_I: return 8;
    case IAMF_HIP_SS_J: return 12;
    case IAMF_HIP_L_712: return 10;
    case IAMF_HIP_L_312: return 6;
    case IAMF_HIP_L_MONO: return 1;
    case IAMF_HIP_L_BINAURAL: return 2;
    default: return 0;
  }
}

int iamf_hip_format_bytes(int f) {
  switch (f) {
    case IAMF_HIP_FMT_S16: return 2;
    case IAMF_HIP_FMT_S24: return 3;
    case IAMF_HIP_FMT_S32: return 4;
    case IAMF_HIP_FMT_F32: return 4;
    default: return 0;
  }
}

const char *iamf_hip_version(void) { return "iamf_hip 0.1 (gfx950, HIP)"; }

int iamf_hip_batch_create(const iamf_hip_batch_config *cfg, iamf_hip_batch **out) {
  if (!cfg || !out) return IAMF_HIP_ERR_BAD_ARG;
  *out = nullptr;
  iamf_hip_matrix mx = cfg->matrix;
  const bool dmx = mx.kind == IAMF_HIP_KIND_DMX;
  const bool fir = mx.kind == IAMF_HIP_KIND_FIR;
  if (fir && (cfg->fir_taps < 1 || cfg->fir_taps > 256 || mx.n != 2 || cfg->out_channels != 2 ||
              !cfg->limiter_enable ||
              (!FirHomeM::has(mx.m) && !FirM2bM::has(mx.m))))
    return IAMF_HIP_ERR_BAD_ARG;
  if (dmx) {
    if (!iamf_hip_dmx_valid(mx.in_id, mx.out_id)) return IAMF_HIP_ERR_BAD_ARG;
    mx.m = kLayoutCount[mx.in_id];
    mx.n = kLayoutCount[mx.out_id];
  }
  if (cfg->n_streams <= 0 || cfg->frame_size <= 0 || cfg->sample_rate <= 0 || (!dmx && !mx.mat) ||
      mx.m <= 0 || mx.m > kMaxIn || mx.n <= 0 || mx.n > kMaxOut || cfg->out_channels <= 0 ||
      cfg->out_channels > kMaxOut || !iamf_hip_format_bytes(cfg->out_format) || cfg->projection < 0 ||
      cfg->projection > IAMF_HIP_PROJ_MFMA || (dmx && cfg->out_channels != mx.n) || cfg->pcm_stride_channels < 0 || cfg->out_gain_channels < 0 ||
      cfg->pcm_stride_channels > 64)
    return IAMF_HIP_ERR_BAD_ARG;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return IAMF_HIP_ERR_DEVICE;

  iamf_hip_batch *b = new (std::nothrow) iamf_hip_batch();
  if (!b) return IAMF_HIP_ERR_ALLOC_FAIL;
  b->cfg = *cfg;
  if (hipGetDevice(&b->device) != hipSuccess) {
    delete b;
    return IAMF_HIP_ERR_DEVICE;
  }
  b->m = mx.m;
  b->n_feeds = mx.n;
  b->dmx = dmx;

  b->fir = fir;
  b->fir_taps = fir ? cfg->fir_taps : 0;
  std::vector<float> fm(1, 0.f);
  int32_t dmx_tab[24];
  memset(dmx_tab, 0, sizeof(dmx_tab));
  if (dmx) {
    for (int i = 0; i < kMaxOut; ++i) b->src_feed[i] = -1;
    b->dmx_n_in = mx.m;
    b->dmx_n_out = mx.n;
    for (int i = 0; i < mx.m; ++i) dmx_tab[i] = kLayoutCh[mx.in_id][i];
    for (int i = 0; i < mx.n; ++i) dmx_tab[12 + i] = kLayoutCh[mx.out_id][i];
  } else if (fir) {
    for (int i = 0; i < kMaxOut; ++i) b->src_feed[i] = -1;  // the flush renders silence
    fm.assign(mx.mat, mx.mat + (size_t)2 * mx.m * cfg->fir_taps);
  } else {
    build_feed_map(mx, cfg->out_channels, fm, b->src_feed);
    // The fused LPCM kernel folds the LPCM decoder's "/ 32768" into the weights: (w * 2^-15) * (float)s has the bits of
    // w * (s * 2^-15) as long as neither the scaled weight nor a product leaves the normal range — scaling by a power of two
    // commutes with rounding there.  True of every table of the reference (|w| in 1e-4 .. 2); a caller's own matrix with
    // weights below 2^-100 takes the unfused path.
    // The 24-bit form (render_fast_kernel<.., LPB = 3>) folds "/ 2^23" (pcm/IAMF_pcm_decoder.c:71-76, 144-148) the same way,
    // and the same check suffices: a 24-bit integer is exact in f32 and s * 2^-23 is exact; for a non-zero |w| in
    // [2^-100, 2^100] the staged weight w * 2^-23 >= 2^-123 is normal (no bit of w is lost), and with |s| >= 1 the product
    // (w * 2^-23) * s is at least 2^-123 and at most 2^100: normal, so it has the bits of w * (s * 2^-23).  s == 0 gives a
    // zero of the same sign either way.  (Not so for 32-bit samples: w * 2^-31 may be subnormal, and (float)s rounds.)
    b->lp_scale_ok = true;
    for (float w : fm)
      if (w != 0.f && !(fabsf(w) >= 0x1p-100f && fabsf(w) <= 0x1p100f)) b->lp_scale_ok = false;
    if (cfg->lfe_hoa && mx.kind == IAMF_HIP_KIND_H2M && (mx.lfe1 >= 0 || mx.lfe2 >= 0)) {
      // HOA LFE generator on (the reference built -DDISABLE_LFE_HOA=0): lfefilter_init(plfe, 120, rate),
      // h2m_rdr.c:1192-1212, in the reference's own expression types
      const float sample_rate = (float)cfg->sample_rate, cutoff_freq = 120;
      const float delta_time = 1 / sample_rate + 1.0e-10;
      const float c = 1.0f / (float)tanf(M_PI * cutoff_freq * delta_time);
      b->lfe = true;
      b->lfe_a1 = 1.0f / (1.0f + c + c * c);
      b->lfe_a2 = 2.0f * b->lfe_a1;
      b->lfe_a3 = b->lfe_a1;
      b->lfe_b1 = 2.0f * (1.0f - c * c) * b->lfe_a1;
      b->lfe_b2 = (1.0f - c + c * c) * b->lfe_a1;
      b->lfe_div = mx.n <= 2 ? 0.0 : sqrt((double)mx.n);
      if (mx.lfe1 >= 0 && mx.lfe1 < cfg->out_channels) b->src_feed[mx.lfe1] = -2;
      if (mx.lfe2 >= 0 && mx.lfe2 < cfg->out_channels) b->src_feed[mx.lfe2] = -2;
    }
    // sparsity of the matrix as the output slots see it (render_wide4.hpp skips all-zero weight batches)
    int set = 0, all = 0;
    for (int g = 0; g < 6 && 4 * g < cfg->out_channels; ++g)
      for (int k = 0; k < mx.m && k < 32; ++k) {
        bool nz = false;
        for (int c = 4 * g; c < 4 * g + 4 && c < cfg->out_channels; ++c)
          if (b->src_feed[c] >= 0 && fm[(size_t)b->src_feed[c] * mx.m + k] != 0.f) nz = true;
        ++all;
        if (nz) {
          ++set;
          b->nz_mask[g] |= 1u << k;
        }
      }
    b->sparse = 2 * set < all ? 1 : 0;
    b->h_fm = fm;
  }

  // limiter constants and the coefficient table.  currentTC only ever takes the values
  // T[n] = n-fold f32 accumulation of incTC from 0 (audio_effect_peak_limiter.c:82,242,248,263),
  // so the attack / release curve values are a function of n alone.
  const float atk = 0.001f, rel = 0.200f;  // common/audio_defines.h:39-40
  b->thr = (float)pow(10, cfg->limiter_threshold_db / 20);
  const float inc = (float)1 / (float)cfg->sample_rate;
  std::vector<float> T;
  T.push_back(0.0f);
  while (T.back() < rel + atk && T.size() < (1u << 22)) T.push_back(T.back() + inc);
  b->n_end = (int)T.size() - 1;
  b->n_atk = 0;
  while (b->n_atk < b->n_end && T[b->n_atk] < atk) ++b->n_atk;
  std::vector<float> ctab((size_t)b->n_end + 1, 1.0f);
  for (int k = 1; k <= b->n_end; ++k)
    ctab[k] = (k - 1) < b->n_atk ? ease(T[k] / atk) : ease((T[k] - atk) / rel);

  const int ns = cfg->n_streams;
  b->h_gains.assign((size_t)3 * ns, 1.0f);
#define CREATE_CHK(expr)                       \
  do {                                         \
    if ((expr) != hipSuccess) {                \
      iamf_hip_batch_destroy(b);               \
      return IAMF_HIP_ERR_DEVICE;              \
    }                                          \
  } while (0)
  CREATE_CHK(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
  CREATE_CHK(hipMalloc(&b->d_matrix, sizeof(float) * fm.size()));
  CREATE_CHK(hipMalloc(&b->d_gains, sizeof(float) * 3 * ns));
  CREATE_CHK(hipMalloc(&b->d_ctab, sizeof(float) * ctab.size()));
  CREATE_CHK(hipMalloc(&b->d_lim, sizeof(LimState) * ns));
  CREATE_CHK(hipMalloc(&b->d_ring_y, sizeof(float) * (size_t)ns * cfg->out_channels * kSave));
  CREATE_CHK(hipMalloc(&b->d_ring_pm, sizeof(float) * (size_t)ns * kSave));
  if (b->lfe) {
    CREATE_CHK(hipMalloc(&b->d_lfe_state, sizeof(float) * 4 * (size_t)ns));
    CREATE_CHK(hipMalloc(&b->d_lfe_next, sizeof(float) * 2 * (size_t)ns));
  }
  CREATE_CHK(hipMalloc(&b->d_dump, (size_t)ns * 256 * 16));
  CREATE_CHK(hipMalloc(&b->d_src_feed, sizeof(int32_t) * kMaxOut));
  CREATE_CHK(hipMemcpy(b->d_src_feed, b->src_feed, sizeof(int32_t) * kMaxOut, hipMemcpyHostToDevice));
  if (fir) {
    const size_t hb = sizeof(float) * (size_t)ns * mx.m * 256;
    CREATE_CHK(hipMalloc(&b->d_fir_hist[0], hb));
    CREATE_CHK(hipMalloc(&b->d_fir_hist[1], hb));
    CREATE_CHK(hipMemset(b->d_fir_hist[0], 0, hb));
    CREATE_CHK(hipMemset(b->d_fir_hist[1], 0, hb));
    // Tables of render_fir16.hpp: per channel [ear][hi/lo][shift r][304] halves with
    // table_r[n] = hp[n + r], hp[j] = h[j - 15] * scale split as hi + lo * 2^-11.  The scale is the
    // power of two that puts the largest tap in [2^13, 2^14).
    const int taps = cfg->fir_taps;
    float hmax = 0.f;
    for (size_t i = 0; i < (size_t)2 * mx.m * taps; ++i) hmax = fmaxf(hmax, fabsf(mx.mat[i]));
    if (hmax > 0.f && hmax < 1e30f) {
      int e = 0;
      (void)frexpf(hmax, &e);  // hmax = f * 2^e, f in [0.5, 1)
      const float scale = ldexpf(1.f, 14 - e);
      std::vector<_Float16> tab((size_t)mx.m * 2 * 2 * 8 * kF16Taps, (_Float16)0.f);
      for (int ch = 0; ch < mx.m; ++ch)
        for (int ear = 0; ear < 2; ++ear)
          for (int r = 0; r < 8; ++r)
            for (int n = 0; n < kF16Taps; ++n) {
              const int k = n + r - 15;  // tap index of hp[n + r]
              if (k < 0 || k >= taps) continue;
              const float v = mx.mat[((size_t)ear * mx.m + ch) * taps + k] * scale;
              const _Float16 hi = (_Float16)v;
              const _Float16 lo = (_Float16)((v - (float)hi) * 2048.f);
              const size_t at = ((((size_t)ch * 2 + ear) * 2 + 0) * 8 + r) * kF16Taps + n;
              tab[at] = hi;
              tab[at + (size_t)8 * kF16Taps] = lo;
            }
      CREATE_CHK(hipMalloc(&b->d_fir_h16, tab.size() * sizeof(_Float16)));
      CREATE_CHK(hipMemcpy(b->d_fir_h16, tab.data(), tab.size() * sizeof(_Float16), hipMemcpyHostToDevice));
      b->fir_inv_scale = 1.f / (scale * kF16InScale);
    }
    {  // the FFT stage's tables (render_fir_fft.hpp): pair spectra in the transform's own bin order, twiddles
      std::vector<float> pq, tw;
      fft_build_tables(mx.mat, mx.m, taps, pq, tw);
      CREATE_CHK(hipMalloc(&b->d_fir_pq, pq.size() * sizeof(float)));
      CREATE_CHK(hipMemcpy(b->d_fir_pq, pq.data(), pq.size() * sizeof(float), hipMemcpyHostToDevice));
      CREATE_CHK(hipMalloc(&b->d_fir_tw, tw.size() * sizeof(float)));
      CREATE_CHK(hipMemcpy(b->d_fir_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice));
      const size_t zf = (size_t)(mx.m > 0 ? mx.m : 1) * (size_t)(cfg->frame_size > 64 ? cfg->frame_size : 64);
      CREATE_CHK(hipMalloc(&b->d_fir_zero, zf * sizeof(float)));
      CREATE_CHK(hipMemset(b->d_fir_zero, 0, zf * sizeof(float)));
      if (cfg->frame_size >= 1024 && cfg->frame_size % 256 == 0 && mx.m % 2 == 0) {   // fir_fft_kernel<M, true>
        const int g = cfg->frame_size / 256;
        b->fir_pre_bytes = sizeof(float) * (size_t)((ns + g - 1) / g) * mx.m * cfg->frame_size;
        for (float *&q : b->d_fir_pre) {
          CREATE_CHK(hipMalloc(&q, b->fir_pre_bytes));
          CREATE_CHK(hipMemset(q, 0, b->fir_pre_bytes));
        }
      }
      const float id[4] = {1.f, 0.f, 0.f, 1.f};
      int32_t idf[kMaxOut];
      for (int i = 0; i < kMaxOut; ++i) idf[i] = i < 2 ? i : -1;
      CREATE_CHK(hipMalloc(&b->d_fir_id, sizeof(id)));
      CREATE_CHK(hipMemcpy(b->d_fir_id, id, sizeof(id), hipMemcpyHostToDevice));
      CREATE_CHK(hipMalloc(&b->d_fir_id_feed, sizeof(idf)));
      CREATE_CHK(hipMemcpy(b->d_fir_id_feed, idf, sizeof(idf), hipMemcpyHostToDevice));
    }
  }
  CREATE_CHK(hipMalloc(&b->d_dmx_tab, sizeof(dmx_tab)));
  CREATE_CHK(hipMemcpy(b->d_dmx_tab, dmx_tab, sizeof(dmx_tab), hipMemcpyHostToDevice));
  CREATE_CHK(hipMemcpy(b->d_matrix, fm.data(), sizeof(float) * fm.size(), hipMemcpyHostToDevice));
  CREATE_CHK(hipMemcpy(b->d_gains, b->h_gains.data(), sizeof(float) * 3 * ns, hipMemcpyHostToDevice));
  CREATE_CHK(hipMemcpy(b->d_ctab, ctab.data(), sizeof(float) * ctab.size(), hipMemcpyHostToDevice));
#undef CREATE_CHK
  const int r = reset_state(b);
  if (r != IAMF_HIP_OK) {
    iamf_hip_batch_destroy(b);
    return r;
  }
  *out = b;
  return IAMF_HIP_OK;
}

void iamf_hip_batch_destroy(iamf_hip_batch *b) {
  if (!b) return;
  int cur = -1;   // free on the batch's own device whatever is current, and restore
  const bool sw = hipGetDevice(&cur) == hipSuccess && cur != b->device && hipSetDevice(b->device) == hipSuccess;
  struct Restore {
    bool on;
    int dev;
    ~Restore() {
      if (on) (void)hipSetDevice(dev);
    }
  } restore{sw, cur};
  if (b->rendered) (void)hipEventSynchronize(b->done);
  if (b->done) (void)hipEventDestroy(b->done);
  (void)hipFree(b->d_matrix_pre);
  (void)hipFree(b->d_matrix);
  (void)hipFree(b->d_gains);
  (void)hipFree(b->d_ctab);
  (void)hipFree(b->d_lim);
  (void)hipFree(b->d_ring_y);
  (void)hipFree(b->d_ring_pm);
  (void)hipFree(b->d_src_feed);
  (void)hipFree(b->d_dmx_tab);
  (void)hipFree(b->d_pre);
  (void)hipFree(b->d_demix_tab);
  (void)hipFree(b->d_demix_ftab);
  (void)hipFree(b->d_fir_hist[0]);
  (void)hipFree(b->d_fir_hist[1]);
  (void)hipFree(b->d_fir_h16);
  (void)hipFree(b->d_fir_pq);
  (void)hipFree(b->d_fir_tw);
  (void)hipFree(b->d_fir_zero);
  (void)hipFree(b->d_fir_pre[0]);
  (void)hipFree(b->d_fir_pre[1]);
  (void)hipFree(b->d_fir_y);
  (void)hipFree(b->d_lp_in);
  (void)hipFree(b->d_lp_in2);
  (void)hipFree(b->d_fir_id);
  (void)hipFree(b->d_fir_id_feed);
  if (!b->lfe_shared) {
    (void)hipFree(b->d_lfe_state);
    (void)hipFree(b->d_lfe_next);
  }
  (void)hipFree(b->d_lfe_u);
  (void)hipFree(b->d_nat);
  (void)hipFree(b->d_dump);
  (void)hipFree(b->d_matrix2);
  (void)hipFree(b->d_gains2);
  (void)hipFree(b->d_src_feed2);
  delete b;
}

int iamf_hip_batch_set_gains(iamf_hip_batch *b, const float *eg, const float *og, const float *lg) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  {  // a render queued earlier may still be reading d_gains
    const int q = quiesce(b);
    if (q != IAMF_HIP_OK) return q;
  }
  const int ns = b->cfg.n_streams;
  // Only the rows given are uploaded: a row left NULL keeps what the device holds, which since iamf_hip_batch_import_range
  // may be newer than the host mirror (an imported stream's gains arrive in its blob, on the device).
  const float *rows[3] = {eg, og, lg};
  for (int k = 0; k < 3; ++k) {
    if (!rows[k]) continue;
    memcpy(&b->h_gains[(size_t)k * ns], rows[k], sizeof(float) * ns);
    HIPCHK(hipMemcpy(b->d_gains + (size_t)k * ns, rows[k], sizeof(float) * ns, hipMemcpyHostToDevice));
  }
  return IAMF_HIP_OK;
}

// the argument checks of a range call: IAMF_HIP_OK and the call's samples per stream in *total_out (0: nothing to do), or the error
static int range_args_check(const iamf_hip_batch *b, const iamf_hip_render_args *a, int32_t stream0, int32_t n_streams, int64_t *total_out) {
  *total_out = 0;
  if (!b || !a || !a->d_in || !a->d_pcm || a->n_frames < 0) return IAMF_HIP_ERR_BAD_ARG;
  if (!range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  if (a->n_frames == 0) return IAMF_HIP_OK;
  if (b->has2 && !a->d_in2) return IAMF_HIP_ERR_BAD_ARG;
  if (b->dmx && !a->d_dmx_frames) return IAMF_HIP_ERR_BAD_ARG;
  if (b->demix && a->d_in && (!a->d_demix_frames || a->demix_sample0 < 0 ||
                              a->demix_sample0 + (a->n_samples ? a->n_samples : 1) > b->cfg.frame_size))
    return IAMF_HIP_ERR_BAD_ARG;
  if ((a->d_element_ramp || a->d_element2_ramp || a->d_output_ramp) &&
      a->ramp_stream_stride < (int64_t)a->n_frames * b->cfg.frame_size && b->cfg.n_streams > 1)
    return IAMF_HIP_ERR_BAD_ARG;
  int64_t total = (int64_t)a->n_frames * b->cfg.frame_size;
  if (a->n_samples > 0) {
    if (a->n_frames != 1 || a->n_samples > b->cfg.frame_size) return IAMF_HIP_ERR_BAD_ARG;
    total = a->n_samples;
  }
  if (total > INT32_MAX) return IAMF_HIP_ERR_BAD_ARG;
  const int sc = b->cfg.pcm_stride_channels > 0 ? b->cfg.pcm_stride_channels : b->cfg.out_channels;
  const int64_t need = (total * sc + (b->cfg.out_channels > sc ? b->cfg.out_channels - sc : 0)) *
                       iamf_hip_format_bytes(b->cfg.out_format);
  if (b->cfg.n_streams > 1 && a->pcm_stream_stride_bytes < need) return IAMF_HIP_ERR_BUFFER_TOO_SMALL;
  *total_out = total;
  return IAMF_HIP_OK;
}

// a range call of one element: the argument checks, then the call (lp, form, first: as render_prepare)
static int render_range_impl(iamf_hip_batch *b, const iamf_hip_render_args *a, int32_t stream0, int32_t n_streams, const LpcmIn *lp,
                             CallForm form, int first) {
  int64_t total = 0;
  const int rc = range_args_check(b, a, stream0, n_streams, &total);
  if (rc != IAMF_HIP_OK || total == 0) return rc;
  return render_call(b, *a, (int)total, stream0, n_streams, lp, nullptr, form, first);
}

int iamf_hip_batch_render_range(iamf_hip_batch *b, const iamf_hip_render_args *a, int32_t stream0, int32_t n_streams) {
  return render_range_impl(b, a, stream0, n_streams, nullptr, CallForm::Plain, 0);
}

// Element 0 as LPCM packets.  Fused (render_fast_kernel<.., LP>: the packets' samples are converted where the render
// kernel loads them) when the call is one of the headline kernel's and every channel is a contiguous run of little-endian
// 16-bit or 24-bit samples on the form's grid (lpcm_form.hpp: 8 bytes / 4 bytes), or the channels are the 16-bit coupled
// pairs and mono runs of a loudspeaker layout (LpcmForm::S16C); in every other case exactly what the
// caller would do itself: iamf_hip_lpcm_unpack into a buffer of the batch, then the f32 path.  Both give the same PCM
// and leave the same stream state, bit for bit.
int iamf_hip_batch_render_lpcm(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *args) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  return iamf_hip_batch_render_lpcm_range(b, in, args, 0, b->cfg.n_streams);
}

// the same for the streams [stream0, stream0 + n_streams) only (as iamf_hip_batch_render_range: buffers and strides are
// still indexed by the stream's number in the batch)
// The packet-form checks of an LPCM call of nf frames (n_samples as iamf_hip_render_args::n_samples): an error, or
// IAMF_HIP_OK with the trim {first, count} and whether the packets have the form the fused kernels read
// (ch: the channels of the element the packets hold — element 0's, or the second element's for iamf_hip_batch_render_lpcm_mix;
//  packets: the call came through iamf_hip_batch_render_packets or _packets_mix, which also take LpcmForm::S24C)
static int lpcm_form_check_ch(const iamf_hip_batch *b, const iamf_hip_lpcm_input *in, int ch, int nf, int n_samples, LpcmForm *form_out,
                              int *first_out, int *count_out, bool packets) {
  const iamf_hip_lpcm_layout &L = in->layout;
  const int fs = b->cfg.frame_size;
  if (L.sample_bytes < 2 || L.sample_bytes > 4 || L.channels != ch || ch > IAMF_HIP_LPCM_MAX_CHANNELS || L.frame_size != fs ||
      (fs & 3) || in->raw_frame_stride <= 0 || in->raw_stream_stride < (int64_t)nf * in->raw_frame_stride)
    return IAMF_HIP_ERR_BAD_ARG;
  const int first = in->first_sample, count = n_samples > 0 ? n_samples : fs;
  if (first < 0 || (first > 0 && (nf != 1 || n_samples <= 0)) || first + count > fs) return IAMF_HIP_ERR_BAD_ARG;
  for (int c = 0; c < ch; ++c) {   // every byte a kernel may read lies inside the frame's packet row (as iamf_hip_lpcm_unpack)
    if (L.src_offset[c] < 0) continue;
    if (L.src_step[c] < L.sample_bytes ||
        (int64_t)L.src_offset[c] + (int64_t)(fs - 1) * L.src_step[c] + L.sample_bytes > in->raw_frame_stride)
      return IAMF_HIP_ERR_BAD_ARG;
  }
  // which form, if any, the fused kernels can load as it lies (lpcm_form.hpp; pinned by tests/route_host)
  *form_out = (packets ? lpcm_form_packets : lpcm_form)(L, ch, in->raw_stream_stride, in->raw_frame_stride,
                                                        reinterpret_cast<uintptr_t>(in->d_raw), first);
  *first_out = first;
  *count_out = count;
  return IAMF_HIP_OK;
}

static int lpcm_form_check(const iamf_hip_batch *b, const iamf_hip_lpcm_input *in, int nf, int n_samples, LpcmForm *form_out,
                           int *first_out, int *count_out, bool packets) {
  return lpcm_form_check_ch(b, in, element_channels(b), nf, n_samples, form_out, first_out, count_out, packets);
}

// packets of the fusable form as the fused kernels take them
static void lpcm_in_of(const iamf_hip_lpcm_input *in, int ch, int first, LpcmForm form, LpcmIn &lp) {
  memset(&lp, 0, sizeof(lp));
  lp.raw = static_cast<const uint8_t *>(in->d_raw);
  lp.stream_stride = in->raw_stream_stride;
  lp.frame_stride = in->raw_frame_stride;
  lp.bytes = in->layout.sample_bytes;
  lp.coupled = form == LpcmForm::S16C ? 1 : (form == LpcmForm::S24C ? 2 : 0);
  // (src_step: the sample bytes of a contiguous run, twice that for the halves of a coupled pair)
  for (int c = 0; c < ch; ++c) lp.off[c] = in->layout.src_offset[c] + in->layout.src_step[c] * first;
}

// The RANGE's packets -> planar f32 in a buffer of the batch (rows indexed by the stream's number in the batch, as every
// buffer of a range call); a's input fields then name that buffer.  {first, count} travel in the unpacker's kernel arguments
// (a device word updated by a blocking copy cost K host synchronisations per round of a group with K divergent runs).
// (second: the SECOND element's packets, into the batch's second buffer and a's in2 fields — iamf_hip_batch_render_lpcm_mix)
static int lpcm_unpack_range(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, int nf, int first, int count, int32_t stream0,
                             int32_t n_streams, hipStream_t st, iamf_hip_render_args &a, bool second = false) {
  const iamf_hip_lpcm_layout &L = in->layout;
  const int fs = b->cfg.frame_size, ch = second ? b->m2 : element_channels(b), ns = b->cfg.n_streams;
  float *&d_buf = second ? b->d_lp_in2 : b->d_lp_in;
  // as many frames per launch as the grid's third dimension takes; a range too wide for one frame is refused before
  // anything is allocated or queued
  const int fmax = 65535 / n_streams;
  if (fmax == 0) return IAMF_HIP_ERR_UNIMPLEMENTED;
  // zeroed when it grows: rows of channels no sub-stream carries (src_offset < 0) are never written by the unpacker
  const int gr = grow_scratch(b, st, &d_buf, second ? &b->lp_in2_bytes : &b->lp_in_bytes, sizeof(float) * (size_t)ns * nf * ch * fs, true);
  if (gr != IAMF_HIP_OK) return gr;
  const int64_t lp_stream_stride = (int64_t)nf * ch * fs;
  for (int f = 0; f < nf; f += fmax) {
    const int r = iamf_hip_lpcm_unpack_frames(
        &L, static_cast<const uint8_t *>(in->d_raw) + (int64_t)stream0 * in->raw_stream_stride + (int64_t)f * in->raw_frame_stride,
        in->raw_stream_stride, in->raw_frame_stride, nf - f < fmax ? nf - f : fmax, nullptr, 0,
        d_buf + (int64_t)stream0 * lp_stream_stride + (size_t)f * ch * fs, lp_stream_stride, (int64_t)ch * fs, n_streams, st, first,
        count);
    if (r != IAMF_HIP_OK) return r;
  }
  if (second) {
    a.d_in2 = d_buf;
    a.in2_stream_stride = lp_stream_stride;
    a.in2_frame_stride = (int64_t)ch * fs;
  } else {
    a.d_in = d_buf;
    a.in_stream_stride = lp_stream_stride;
    a.in_frame_stride = (int64_t)ch * fs;
  }
  return IAMF_HIP_OK;
}

// (form, CallForm::Lpcm and on: from Packets on the form is asked of lpcm_form_packets(), and the fused attempt carries what the
//  entry may take; everything else is the one path)
static int render_lpcm_range_impl(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *args,
                                  int32_t stream0, int32_t n_streams, CallForm call_form) {
  if (!b || !in || !args || !in->d_raw || args->d_in || !args->d_pcm || args->n_frames < 0) return IAMF_HIP_ERR_BAD_ARG;
  if (!range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (args->n_frames == 0) return 0;
  const int ch = element_channels(b), nf = args->n_frames;
  LpcmForm form = LpcmForm::None;
  int first = 0, count = 0;
  const int fc = lpcm_form_check(b, in, nf, args->n_samples, &form, &first, &count, call_form >= CallForm::Packets);
  if (fc != IAMF_HIP_OK) return fc;
  iamf_hip_render_args a = *args;
  if (form != LpcmForm::None) {
    LpcmIn lp;
    lpcm_in_of(in, ch, first, form, lp);
    a.d_in = reinterpret_cast<const float *>(in->d_raw);   // not read by the fused kernel; non-null = "not a flush"
    a.in_stream_stride = a.in_frame_stride = 0;
    const int r = render_range_impl(b, &a, stream0, n_streams, &lp, call_form, first);
    if (r != kNotFused) return r;
  }
  // Unfused: unpack, then the f32 path.  Everything the render call would refuse is refused here first, so that no unpack
  // launch precedes an error.
  {
    a.d_in = reinterpret_cast<const float *>(in->d_raw);   // placeholder for the checks: set below
    int64_t total = 0;
    const int rc = range_args_check(b, &a, stream0, n_streams, &total);
    if (rc != IAMF_HIP_OK || total == 0) return rc;
  }
  const int ur = lpcm_unpack_range(b, in, nf, first, count, stream0, n_streams, static_cast<hipStream_t>(args->stream), a);
  if (ur != IAMF_HIP_OK) return ur;
  return render_range_impl(b, &a, stream0, n_streams, nullptr, CallForm::Plain, 0);
}

int iamf_hip_batch_render_lpcm_range(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *args,
                                     int32_t stream0, int32_t n_streams) {
  return render_lpcm_range_impl(b, in, args, stream0, n_streams, CallForm::Lpcm);
}

// Element 0 as LPCM packets of every form a fused kernel reads (include/iamf_hip.h): iamf_hip_batch_render_lpcm_range with
// leave to take render_fast_kernel<.., LP, EARLY, 3, LPC> (Family::Lpcm24Coupled) where the packets have the coupled 24-bit
// form (lpcm_form_packets) and render_prepare and pick_route let the call through.  The same checks in the same order, the
// same path for everything else.
int iamf_hip_batch_render_packets(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_range_impl(b, &call->in, &call->args, stream0, n_streams, CallForm::Packets);
}

// Element 0 as LPCM packets of any call length (include/iamf_hip.h): iamf_hip_batch_render_packets with leave to take
// render_fast_kernel<.., LP, true, LPB, LPC, 0, false, RAG> (Family::PacketsRagged) where the call is no whole number of 64-sample
// blocks, the packets have one of the four fused forms and render_prepare and pick_route let the call through.  The same
// checks in the same order, the same path for everything else.
int iamf_hip_batch_render_packets_ragged(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_range_impl(b, &call->in, &call->args, stream0, n_streams, CallForm::PacketsRagged);
}

// Element 0 as LPCM packets on a limiter-less batch (include/iamf_hip.h): iamf_hip_batch_render_packets_ragged with leave to take
// render_nolim_kernel<M, LPB, LPC> (Family::NolimPackets) where the batch is of the plain limiter-less kind, the packets
// have one of the four fused forms and render_prepare and pick_route let the call through.  The same checks in the same order,
// the same path for everything else.
int iamf_hip_batch_render_packets_nolim(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_range_impl(b, &call->in, &call->args, stream0, n_streams, CallForm::PacketsNolim);
}

// Both elements of a mix as LPCM packets (include/iamf_hip.h).  Fused (render_fast_kernel<.., LP2>: Family::LpcmMix) when
// each element's packets have a form its side of the kernel reads — element 0: S16 with LpcmM channels or S16C; element 1:
// S16 with 1 or 4 channels or S16C with 2 (lpcm_form() on each element's own layout) — and pick_route takes the call; in
// every other case both elements are unpacked, each into a buffer of the batch, and the f32 path renders them.  Both ways
// give the same PCM and leave the same stream state, bit for bit.  Every refusal comes before the first launch.
// (call_form, CallForm::Lpcm and on: from Packets on the forms are asked of lpcm_form_packets(), 24-bit packets on both elements
//  are a fused form as well, and the fused attempt carries what the entry may take; everything else is the one path)
static int render_lpcm_mix_impl(iamf_hip_batch *b, const iamf_hip_lpcm_input *in0, const iamf_hip_lpcm_input *in1,
                                const iamf_hip_render_args *args, int32_t stream0, int32_t n_streams, CallForm call_form) {
  const bool packets = call_form >= CallForm::Packets;
  if (!b->has2 || args->d_in || args->d_in2 || !in0->d_raw || !in1->d_raw || in0->first_sample != in1->first_sample ||
      !args->d_pcm || args->n_frames < 0)
    return IAMF_HIP_ERR_BAD_ARG;
  if (!range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (args->n_frames == 0) return 0;
  const int ch = element_channels(b), nf = args->n_frames;
  LpcmForm form0 = LpcmForm::None, form1 = LpcmForm::None;
  int first = 0, count = 0, first1 = 0, count1 = 0;
  int fc = lpcm_form_check_ch(b, in0, ch, nf, args->n_samples, &form0, &first, &count, packets);
  if (fc != IAMF_HIP_OK) return fc;
  fc = lpcm_form_check_ch(b, in1, b->m2, nf, args->n_samples, &form1, &first1, &count1, packets);
  if (fc != IAMF_HIP_OK) return fc;
  // Everything the render call would refuse is refused here, in front of the fused attempt and of the first unpack launch
  // (the two packet buffers stand in for d_in / d_in2: "not a flush", "a second element is given")
  iamf_hip_render_args a = *args;
  a.d_in = reinterpret_cast<const float *>(in0->d_raw);
  a.d_in2 = reinterpret_cast<const float *>(in1->d_raw);
  a.in_stream_stride = a.in_frame_stride = a.in2_stream_stride = a.in2_frame_stride = 0;
  int64_t total = 0;
  const int rc = range_args_check(b, &a, stream0, n_streams, &total);
  if (rc != IAMF_HIP_OK || total == 0) return rc;
  bool form0_ok = (form0 == LpcmForm::S16 && LpcmM::has(ch)) || form0 == LpcmForm::S16C;
  bool form1_ok = (form1 == LpcmForm::S16 || form1 == LpcmForm::S16C) &&
                  lpcm_mix_m2_ok(form1 == LpcmForm::S16C ? 2 : 1, b->m2);
  if (packets && !(form0_ok && form1_ok)) {   // the 24-bit mix form: both elements 24-bit, each in a form its side reads
    form0_ok = (form0 == LpcmForm::S24 && LpcmM::has(ch)) || form0 == LpcmForm::S24C;
    form1_ok = (form1 == LpcmForm::S24 || form1 == LpcmForm::S24C) && lpcm_mix_m2_ok(form1 == LpcmForm::S24C ? 2 : 1, b->m2);
  }
  if (form0_ok && form1_ok) {
    LpcmIn lp0, lp1;
    lpcm_in_of(in0, ch, first, form0, lp0);
    lpcm_in_of(in1, b->m2, first, form1, lp1);
    const int r = render_call(b, a, (int)total, stream0, n_streams, &lp0, &lp1, call_form, first);
    if (r != kNotFused) return r;
  }
  const hipStream_t st = static_cast<hipStream_t>(args->stream);
  int ur = lpcm_unpack_range(b, in0, nf, first, count, stream0, n_streams, st, a);
  if (ur != IAMF_HIP_OK) return ur;
  ur = lpcm_unpack_range(b, in1, nf, first, count, stream0, n_streams, st, a, true);
  if (ur != IAMF_HIP_OK) return ur;
  return render_range_impl(b, &a, stream0, n_streams, nullptr, CallForm::Plain, 0);
}

int iamf_hip_batch_render_lpcm_mix(iamf_hip_batch *b, const iamf_hip_lpcm_mix_call *call, int32_t stream0, int32_t n_streams) {
  if (!b || !call) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_mix_impl(b, &call->in[0], &call->in[1], &call->args, stream0, n_streams, CallForm::Lpcm);
}

// Both elements of a mix as LPCM packets of every form a fused kernel reads (include/iamf_hip.h): iamf_hip_batch_render_lpcm_mix
// with leave to take render_fast_kernel<.., LP, true, 3, LPC, LP2> (Family::Lpcm24Mix) where both elements hold 24-bit packets
// — element 0: S24 with LpcmM channels or S24C; element 1: S24 with 1 or 4 channels or S24C with 2 (lpcm_form_packets() on
// each element's own layout) — and render_prepare and pick_route let the call through.  The same checks in the same order,
// the same path for everything else.
int iamf_hip_batch_render_packets_mix(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_mix_impl(b, &call->in[0], &call->in[1], &call->args, stream0, n_streams, CallForm::Packets);
}

// Both elements of a mix as LPCM packets of any call length (include/iamf_hip.h): iamf_hip_batch_render_packets_mix with leave to
// take render_fast_kernel<.., IN2, LP, true, LPB, LPC, LP2, false, RAG> (Family::PacketsMixRagged) where the call is no whole number of
// 64-sample blocks, both elements' packets have a form the whole-block mix kernels read and render_prepare and pick_route let the
// call through.  The same checks in the same order, the same path for everything else.
int iamf_hip_batch_render_packets_mix_ragged(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_mix_impl(b, &call->in[0], &call->in[1], &call->args, stream0, n_streams, CallForm::PacketsRagged);
}

// Both elements of a mix as LPCM packets on a limiter-less batch (include/iamf_hip.h): iamf_hip_batch_render_packets_mix_ragged with
// leave to take render_nolim_kernel<M, LPB, LPC, LP2> (Family::NolimPacketsMix) where the batch is of the limiter-less kind without
// stages in front, both elements' packets have a form the mix kernels read and render_prepare and pick_route let the call through.
// The same checks in the same order, the same path for everything else.
int iamf_hip_batch_render_packets_mix_nolim(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams) {
  if (!packet_call_ok(b, call)) return IAMF_HIP_ERR_BAD_ARG;
  return render_lpcm_mix_impl(b, &call->in[0], &call->in[1], &call->args, stream0, n_streams, CallForm::PacketsNolim);
}

// Interleaved f32 of any call length (include/iamf_hip.h): iamf_hip_batch_render_range with leave to take
// render_fast_kernel<.., IL, RAG> (Family::FastInterleaved) where pick_route's rules hold.  The same checks in the same
// order, the same internal route (render_call) for everything else.
int iamf_hip_batch_render_interleaved(iamf_hip_batch *b, const iamf_hip_interleaved_call *call, int32_t stream0, int32_t n_streams) {
  if (!b || !call || call->reserved[0] || call->reserved[1] || call->reserved[2] || call->reserved[3]) return IAMF_HIP_ERR_BAD_ARG;
  if (b->cfg.frame_size != 1) return IAMF_HIP_ERR_BAD_ARG;
  int64_t total = 0;
  const int rc = range_args_check(b, &call->args, stream0, n_streams, &total);
  if (rc != IAMF_HIP_OK || total == 0) return rc;
  return render_call(b, call->args, (int)total, stream0, n_streams, nullptr, nullptr, CallForm::Interleaved, 0);
}

// Planar f32 of any call length (include/iamf_hip.h): iamf_hip_batch_render_range with leave to take
// render_fast_kernel<.., IL = false, RAG> (Family::FastRagged) where pick_route's rules hold.  The same checks in the same
// order, the same internal route (render_call) for everything else.
int iamf_hip_batch_render_ragged(iamf_hip_batch *b, const iamf_hip_ragged_call *call, int32_t stream0, int32_t n_streams) {
  if (!b || !call || call->reserved[0] || call->reserved[1] || call->reserved[2] || call->reserved[3]) return IAMF_HIP_ERR_BAD_ARG;
  int64_t total = 0;
  const int rc = range_args_check(b, &call->args, stream0, n_streams, &total);
  if (rc != IAMF_HIP_OK || total == 0) return rc;
  return render_call(b, call->args, (int)total, stream0, n_streams, nullptr, nullptr, CallForm::Ragged, 0);
}

int iamf_hip_batch_render_ex(iamf_hip_batch *b, const iamf_hip_render_args *a) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  return iamf_hip_batch_render_range(b, a, 0, b->cfg.n_streams);
}

int iamf_hip_batch_render(iamf_hip_batch *b, const float *d_in, int64_t in_stream_stride,
                          int64_t in_frame_stride, int32_t n_frames, void *d_pcm,
                          int64_t pcm_stream_stride_bytes, void *stream) {
  iamf_hip_render_args a;
  memset(&a, 0, sizeof(a));
  a.d_in = d_in;
  a.in_stream_stride = in_stream_stride;
  a.in_frame_stride = in_frame_stride;
  a.n_frames = n_frames;
  a.d_pcm = d_pcm;
  a.pcm_stream_stride_bytes = pcm_stream_stride_bytes;
  a.stream = stream;
  if (b && (b->has2 || b->dmx || b->demix)) return IAMF_HIP_ERR_BAD_ARG;  // those need iamf_hip_batch_render_ex
  return iamf_hip_batch_render_ex(b, &a);
}

// How many members one launch of render_fanout_kernel takes.  The kernel exists for 2 .. IAMF_HIP_FANOUT_MAX; a count that
// measures slower than as many single launches at the bench geometry is not fused (tools/fanout_rate.py).  Measured on
// MI355X, 3rd-order element, 512 / 2048 streams x 64 frames x 1024 (profiles/r06_fanout_rate.json): K = 2 is 1.49 / 1.81
// times as fast as its single launches, K = 3 1.91 / 2.08, K = 4 1.29 / 1.28, the spread between two series of the
// single launches at most 0.009 — every count wins, so all are fused: at this value the `k >= kFanFuseMax` test below
// never holds (a call has at most IAMF_HIP_FANOUT_MAX members); it is where a count that stops winning would be cut.
static const int kFanFuseMax = IAMF_HIP_FANOUT_MAX;

// ---- what iamf_hip_batch_render_fanout* and iamf_hip_batch_render_fanout_lpcm check alike.  Each entry calls these in its
//      own order (which check answers a bad call first is part of the ABI); none of them needs a device. ----

// every member and every member's buffer given, no member given twice (pointers are compared, no member is looked at)
static bool fan_members_distinct(iamf_hip_batch *const *batches, void *const *d_pcm, int n_batches) {
  for (int j = 0; j < n_batches; ++j) {
    if (!batches[j] || !d_pcm[j]) return false;
    for (int i = 0; i < j; ++i)
      if (batches[i] == batches[j]) return false;
  }
  return true;
}

// member b against the first one: the same streams, frame size, element and input channels, and nothing that needs
// iamf_hip_batch_render_ex
static bool fan_member_like(const iamf_hip_batch *b, const iamf_hip_batch *b0) {
  return b->cfg.n_streams == b0->cfg.n_streams && b->cfg.frame_size == b0->cfg.frame_size && b->m == b0->m &&
         element_channels(b) == element_channels(b0) && !(b->has2 || b->dmx || b->demix);
}

// state: the range at one position in every member, unflushed; the HRTF stage's history is per batch, not per stream, so
// a proper sub-range of an HRTF batch is not built (as the single call)
static int fan_state_check(iamf_hip_batch *const *batches, int n_batches, int stream0, int n_streams) {
  const iamf_hip_batch *b0 = batches[0];
  for (int j = 0; j < n_batches; ++j) {
    const iamf_hip_batch *b = batches[j];
    for (int i = stream0; i < stream0 + n_streams; ++i)
      if (b->spos[(size_t)i] != b0->spos[(size_t)stream0] || b->sflushed[(size_t)i]) return IAMF_HIP_ERR_INVALID_STATE;
  }
  if (stream0 != 0 || n_streams != b0->cfg.n_streams)
    for (int j = 0; j < n_batches; ++j)
      if (batches[j]->fir) return IAMF_HIP_ERR_UNIMPLEMENTED;
  return IAMF_HIP_OK;
}

// what differs between the renditions of one fused launch, from a member's prepared call
static FanMember fan_member_of(const RenderParams &p) {
  FanMember mb;
  mb.pcm = p.pcm;
  mb.pcm_stream_stride = p.pcm_stream_stride;
  mb.matrix = p.matrix;
  mb.gains = p.gains;
  mb.ctab = p.ctab;
  mb.lim = p.lim;
  mb.ring_y = p.ring_y;
  mb.ring_pm = p.ring_pm;
  mb.src_feed = p.src_feed;
  mb.out_ch = p.out_ch;
  mb.out_format = p.out_format;
  mb.loudness_on = p.loudness_on;
  mb.n_atk = p.n_atk;
  mb.n_end = p.n_end;
  mb.thr = p.thr;
  return mb;
}

// iamf_hip_batch_render_fanout over the streams [stream0, stream0 + n_streams) of every member; whole: every stream of the
// members, whatever their count (the range arguments are not looked at).  n_samples: iamf_hip_render_args::n_samples of
// every member's call (0 for the public f32 entries).
static int fanout_range_impl(iamf_hip_batch *const *batches, int32_t n_batches, const float *d_in, int64_t in_stream_stride,
                             int64_t in_frame_stride, int32_t n_frames, int32_t n_samples, void *const *d_pcm,
                             const int64_t *pcm_stream_stride_bytes, void *stream, int32_t *n_emitted, int32_t *n_fused,
                             bool whole, int32_t stream0, int32_t n_streams) {
  // ---- checks that need no device ----
  if (n_batches < 1 || n_batches > IAMF_HIP_FANOUT_MAX) return IAMF_HIP_ERR_BAD_ARG;
  if (!batches || !d_in || !d_pcm || !pcm_stream_stride_bytes || !n_emitted) return IAMF_HIP_ERR_BAD_ARG;
  if (!whole && (stream0 < 0 || n_streams <= 0)) return IAMF_HIP_ERR_BAD_ARG;
  if (!fan_members_distinct(batches, d_pcm, n_batches)) return IAMF_HIP_ERR_BAD_ARG;
  // ---- every member's own checks, before anything is queued: what iamf_hip_batch_render would refuse ----
  iamf_hip_render_args args[IAMF_HIP_FANOUT_MAX];
  int64_t total = 0;
  const iamf_hip_batch *b0 = batches[0];
  if (whole) stream0 = 0, n_streams = b0->cfg.n_streams;
  for (int j = 0; j < n_batches; ++j) {
    const iamf_hip_batch *b = batches[j];
    if (!fan_member_like(b, b0)) return IAMF_HIP_ERR_BAD_ARG;
    iamf_hip_render_args &a = args[j];
    memset(&a, 0, sizeof(a));
    a.d_in = d_in;
    a.in_stream_stride = in_stream_stride;
    a.in_frame_stride = in_frame_stride;
    a.n_frames = n_frames;
    a.n_samples = n_samples;
    a.d_pcm = d_pcm[j];
    a.pcm_stream_stride_bytes = pcm_stream_stride_bytes[j];
    a.stream = stream;
    int64_t tj = 0;
    const int rc = range_args_check(b, &a, stream0, n_streams, &tj);
    if (rc != IAMF_HIP_OK) return rc;
    total = tj;   // the call's samples per stream: the same for every member
  }
  if (total == 0) {   // n_frames == 0: nothing to do and no state looked at, as the single call
    if (n_fused) *n_fused = 0;
    for (int j = 0; j < n_batches; ++j) n_emitted[j] = 0;
    return IAMF_HIP_OK;
  }
  for (int j = 0; j < n_batches; ++j)
    if (!on_batch_device(batches[j])) return IAMF_HIP_ERR_INVALID_STATE;   // (the same answer as a member out of position)
  const int state = fan_state_check(batches, n_batches, stream0, n_streams);
  if (state != IAMF_HIP_OK) return state;
  if (n_fused) *n_fused = 0;
  for (int j = 0; j < n_batches; ++j) n_emitted[j] = 0;

  // ---- which members share the input: those the single call would launch as the plain render_fast_kernel<M, OC> (pick_route) ----
  PreparedCall pcs[IAMF_HIP_FANOUT_MAX];
  bool fuse[IAMF_HIP_FANOUT_MAX];
  int k = 0;
  for (int j = 0; j < n_batches; ++j) {
    iamf_hip_batch *b = batches[j];
    fuse[j] = false;
    const int sc = b->cfg.pcm_stride_channels;
    // (nothing that prepare would queue or allocate for: no HRTF stage, LFE generator, de-mapping, fixed channel stride)
    if (k >= kFanFuseMax || b->fir || b->lfe || b->d_pre || (sc > 0 && sc != b->cfg.out_channels) || !b->cfg.limiter_enable ||
        b->cfg.out_channels > 2)
      continue;
    const int rc = render_prepare(b, args[j], (int)total, stream0, n_streams, nullptr, nullptr, CallForm::Plain, 0, pcs[j]);
    if (rc != IAMF_HIP_OK) return rc;
    const Route r = pick_route(pcs[j].p, pcs[j].m_eff);
    fuse[j] = r.family == Family::Fast && r.variant == 0 && pcs[j].m_eff == b0->m && FanM::has(pcs[j].m_eff);
    if (fuse[j]) ++k;
  }
  if (k < 2) k = 0;
  if (k) {
    FanParams fp;
    memset(&fp, 0, sizeof(fp));
    int n = 0;
    for (int j = 0; j < n_batches; ++j) {
      if (!fuse[j]) continue;
      const RenderParams &p = pcs[j].p;
      if (n == 0) {
        fp.in = p.in;
        fp.in_stream_stride = p.in_stream_stride;
        fp.in_frame_stride = p.in_frame_stride;
        fp.pos0 = p.pos0;
        fp.total = p.total;
        fp.frame_size = p.frame_size;
        fp.n_streams = p.n_streams;
        fp.stream0 = stream0;
        fp.n_launch = n_streams;
      }
      fp.mem[n++] = fan_member_of(p);
    }
    if (!iamf_hip_fanout_launch(&fp, b0->m, k, static_cast<hipStream_t>(stream))) return IAMF_HIP_ERR_INTERNAL;
    HIPCHK(hipGetLastError());
    iamf_hip_route_count(0, IAMF_HIP_ROUTE_FANOUT, 0, b0->m, 0, k);
    for (int j = 0; j < n_batches; ++j) {
      if (!fuse[j]) continue;
      const int r = render_commit(batches[j], pcs[j]);
      if (r < 0) return r;
      n_emitted[j] = r;
    }
    if (n_fused) *n_fused = k;
  }
  // ---- every other member: the single call, in member order, on the same stream ----
  for (int j = 0; j < n_batches; ++j) {
    if (k && fuse[j]) continue;
    const int r = render_call(batches[j], args[j], (int)total, stream0, n_streams, nullptr, nullptr, CallForm::Plain, 0);
    if (r < 0) return r;
    n_emitted[j] = r;
  }
  return IAMF_HIP_OK;
}

int iamf_hip_batch_render_fanout(iamf_hip_batch *const *batches, int32_t n_batches, const float *d_in, int64_t in_stream_stride,
                                 int64_t in_frame_stride, int32_t n_frames, void *const *d_pcm,
                                 const int64_t *pcm_stream_stride_bytes, void *stream, int32_t *n_emitted, int32_t *n_fused) {
  return fanout_range_impl(batches, n_batches, d_in, in_stream_stride, in_frame_stride, n_frames, 0, d_pcm, pcm_stream_stride_bytes,
                           stream, n_emitted, n_fused, true, 0, 0);
}

int iamf_hip_batch_render_fanout_range(iamf_hip_batch *const *batches, int32_t n_batches, const float *d_in,
                                       int64_t in_stream_stride, int64_t in_frame_stride, int32_t n_frames, void *const *d_pcm,
                                       const int64_t *pcm_stream_stride_bytes, void *stream, int32_t *n_emitted, int32_t *n_fused,
                                       int32_t stream0, int32_t n_streams) {
  return fanout_range_impl(batches, n_batches, d_in, in_stream_stride, in_frame_stride, n_frames, 0, d_pcm, pcm_stream_stride_bytes,
                           stream, n_emitted, n_fused, false, stream0, n_streams);
}

// How many members one launch of render_fanout_kernel<.., LP> takes for a range of `workgroups` streams: a (K, size) that
// does not beat K single packet-fed calls by more than the spread of two series of those calls is not fused
// (tools/fanout_lpcm_rate.py).  The rule may look at K and at the number of workgroups only.
static int fan_lp_fuse_max(int workgroups) {
  (void)workgroups;
  return IAMF_HIP_FANOUT_MAX;
}

// How many of k packet-fusable members one launch of render_fanout_kernel<.., LP, LPB, LPC> takes for a range of `workgroups`
// streams, under the rule of fan_lp_fuse_max(): a (form, K, size) that does not beat the better of its two baselines — K single
// iamf_hip_batch_render_packets calls, and iamf_hip_batch_render_fanout_lpcm (one unpack pass and the f32 fan-out) — by more
// than that baseline's spread against itself is not fused (tools/fanout_packets_rate.py, profiles/r21_fanout_packets_rate.json).
// The rule may look at the form, at K and at the number of workgroups only.
// Measured on an MI355X, 64 frames x 1024 samples per stream, the hot programme, members {A, A with gains, mono} s16 and mono
// s24, at 512 / 2048 / 4096 streams; in every row the better baseline is the K single calls (the old entry takes 1.13 to 3.85
// times the new launch's time everywhere), whose spread against itself is at most 0.0062:
//   3rd order, 24 bit      K = 2: 1.52 / 1.51 / 1.54 times as fast as its single calls, K = 3: 1.68 / 1.70 / 1.73,
//                          K = 4: 1.017 / 0.979 / 1.009 — fused up to 512 workgroups; above, three members share the launch (the
//                          2048 triple has to stay unfused, and the 0.9 % of the 4096 one are not worth a fourth member there);
//   5.1 coupled, 16 bit    K = 2: 1.025 / 0.547 / 0.542, K = 3: 1.014 / 0.537 / 0.533, K = 4: 0.549 / 0.293 / 0.290;
//   7.1.4 coupled, 24 bit  K = 2: 1.073 / 0.631 / 0.609, K = 3: 1.073 / 0.620 / 0.600, K = 4: 0.584 / 0.345 / 0.335
//                          — the coupled forms: two or three members up to 512 workgroups, nothing above.  (A loudspeaker
//                          layout's down-mix of the hot programme triggers the limiter in nearly every block; the members' limiter
//                          rounds run one after the other in a workgroup, at two workgroups per CU — one for K = 4 — where the
//                          single calls run four.  512 workgroups are the one round of two per CU: the cut lies there.)
// Not measured: fewer than 512 workgroups (the rule keeps its starting value there, IAMF_HIP_FANOUT_MAX, except that a coupled
// K = 4 at exactly the measured 512 is capped) and the sizes between the measured ones, which take the side of the larger.
static int fan_pk_fuse_max(LpcmForm form, int k, int workgroups) {
  if (k > IAMF_HIP_FANOUT_MAX) k = IAMF_HIP_FANOUT_MAX;
  if (workgroups < 512) return k;
  if (form == LpcmForm::S24) return (k == 4 && workgroups > 512) ? 3 : k;
  if (workgroups > 512) return 0;
  return k == 4 ? 3 : k;
}

// iamf_hip_batch_render_fanout_lpcm and, with `packets`, iamf_hip_batch_render_fanout_packets: the same checks in the same order,
// the same routes and report for every call whose packets the latter's kernel does not read.
static int fanout_lpcm_impl(iamf_hip_batch *const *batches, int32_t n_batches, const iamf_hip_lpcm_input *in, int32_t n_frames,
                            int32_t n_samples, void *const *d_pcm, const int64_t *pcm_stream_stride_bytes, void *stream,
                            int32_t stream0, int32_t n_streams, int32_t *n_emitted, iamf_hip_fanout_report *report, bool packets) {
  // ---- checks that need no device ----
  if (n_batches < 1 || n_batches > IAMF_HIP_FANOUT_MAX) return IAMF_HIP_ERR_BAD_ARG;
  if (!batches || !in || !in->d_raw || !d_pcm || !pcm_stream_stride_bytes || !n_emitted || n_frames < 0) return IAMF_HIP_ERR_BAD_ARG;
  if (stream0 < 0 || n_streams <= 0) return IAMF_HIP_ERR_BAD_ARG;
  if (!fan_members_distinct(batches, d_pcm, n_batches)) return IAMF_HIP_ERR_BAD_ARG;
  // ---- the members against each other and the range (as the f32 entry), the device (as the single LPCM call) ----
  iamf_hip_batch *b0 = batches[0];
  const int ch = element_channels(b0);
  for (int j = 0; j < n_batches; ++j)
    if (!fan_member_like(batches[j], b0)) return IAMF_HIP_ERR_BAD_ARG;
  if (stream0 + n_streams > b0->cfg.n_streams) return IAMF_HIP_ERR_BAD_ARG;
  for (int j = 0; j < n_batches; ++j)
    if (!on_batch_device(batches[j])) return IAMF_HIP_ERR_INVALID_STATE;
  iamf_hip_fanout_report rep;
  memset(&rep, 0, sizeof(rep));
  if (n_frames == 0) {   // nothing to do and no state looked at, as the single call
    for (int j = 0; j < n_batches; ++j) n_emitted[j] = 0;
    if (report) *report = rep;
    return IAMF_HIP_OK;
  }
  // ---- the packets (channels and frame size are the same for every member), then every member's own argument checks ----
  LpcmForm form = LpcmForm::None;
  int first = 0, count = 0;
  // (packets: the form is asked of lpcm_form_packets(), which also names S24C; IAMF_HIP_FANOUT_PACKETS_UNFUSED=1 makes the
  //  call iamf_hip_batch_render_fanout_lpcm's)
  if (packets && getenv("IAMF_HIP_FANOUT_PACKETS_UNFUSED")) packets = false;
  const int fc = lpcm_form_check(b0, in, n_frames, n_samples, &form, &first, &count, packets);
  if (fc != IAMF_HIP_OK) return fc;
  // "the form the single call fuses" is the 16-bit one for iamf_hip_batch_render_fanout_lpcm: render_fanout_kernel<.., LP>
  // reads no other there, and 24-bit packets and coupled 16-bit ones (LpcmForm::S16C) keep sharing one unpack pass and the f32
  // fan-out (include/iamf_hip.h).  iamf_hip_batch_render_fanout_packets adds the three forms render_fanout_kernel<.., LP, LPB,
  // LPC> reads (pk_more); a call of any other form (S16, None) takes the same path through either entry.
  const bool pk_more = packets && (form == LpcmForm::S24 || form == LpcmForm::S16C || form == LpcmForm::S24C);
  const int pk_variant = pk_more ? fan_pk_variant(lpcm_form_bytes(form), form != LpcmForm::S24) : 0;
  const bool pk_form = form == LpcmForm::S16 || pk_more;
  iamf_hip_render_args args[IAMF_HIP_FANOUT_MAX];
  int64_t total = 0;
  for (int j = 0; j < n_batches; ++j) {
    iamf_hip_render_args &a = args[j];
    memset(&a, 0, sizeof(a));
    a.d_in = reinterpret_cast<const float *>(in->d_raw);   // not read by the fused kernels; non-null = "not a flush"
    a.n_frames = n_frames;
    a.n_samples = n_samples;
    a.d_pcm = d_pcm[j];
    a.pcm_stream_stride_bytes = pcm_stream_stride_bytes[j];
    a.stream = stream;
    int64_t tj = 0;
    const int rc = range_args_check(batches[j], &a, stream0, n_streams, &tj);
    if (rc != IAMF_HIP_OK) return rc;
    total = tj;
  }
  // ---- state: the range at one position in every member, unflushed; no proper sub-range of an HRTF batch ----
  const int state = fan_state_check(batches, n_batches, stream0, n_streams);
  if (state != IAMF_HIP_OK) return state;

  // ---- what each member runs: 2 = the shared packet-fed launch, 1 = its single packet-fed call, 0 = f32 ----
  PreparedCall pcs[IAMF_HIP_FANOUT_MAX];
  int cls[IAMF_HIP_FANOUT_MAX];
  int k = 0, n_f32 = 0;
  const int k_max = fan_lp_fuse_max(n_streams);
  for (int j = 0; j < n_batches; ++j) {
    iamf_hip_batch *b = batches[j];
    cls[j] = 0;
    if (pk_form) {
      LpcmIn lp;
      lpcm_in_of(in, ch, first, form, lp);
      const int rc = pk_more ? render_prepare(b, args[j], (int)total, stream0, n_streams, &lp, nullptr, CallForm::Packets, first, pcs[j])
                             : render_prepare(b, args[j], (int)total, stream0, n_streams, &lp, nullptr, CallForm::Lpcm, 0, pcs[j]);
      if (rc != kNotFused && rc != IAMF_HIP_OK) return rc;
      if (rc == IAMF_HIP_OK && pk_more) {
        // the member's single call takes the form's family (Lpcm24, LpcmCoupled, Lpcm24Coupled: render_prepare has asked
        // pick_route); on top, nothing re-laid behind the kernel.  How many of these share the launch is decided below
        cls[j] = (!pcs[j].restride && pcs[j].m_eff == b0->m) ? 2 : 1;
        if (cls[j] == 2) ++k;
      } else if (rc == IAMF_HIP_OK) {   // the member's single call takes Family::Lpcm (render_prepare has asked pick_route)
        // what the f32 fan-out asks on top: nothing re-laid behind the kernel; then an instance of this kernel
        cls[j] = (!pcs[j].restride && k < k_max && pcs[j].m_eff == b0->m && FanLpM::has(pcs[j].m_eff)) ? 2 : 1;
        if (cls[j] == 2) ++k;
      }
    }
    if (cls[j] == 0) ++n_f32;
  }
  if (pk_more) {
    // the first k' candidates share the launch, k' the largest count within the measured cap that the form's list holds for M
    int kk = fan_pk_fuse_max(form, k, n_streams);
    while (kk >= 2 && !fan_pk_has(pk_variant, b0->m, kk)) --kk;
    if (kk < 2) kk = 0;
    k = 0;
    for (int j = 0; j < n_batches; ++j)
      if (cls[j] == 2 && k++ >= kk) cls[j] = 1;
    k = kk;
  } else if (k < 2 || !FanLpK::has(k)) {
    for (int j = 0; j < n_batches; ++j)
      if (cls[j] == 2) cls[j] = 1;
    k = 0;
  }
  if (n_f32 && 65535 / n_streams == 0) return IAMF_HIP_ERR_UNIMPLEMENTED;   // the unpacker's grid (lpcm_unpack_range)
  int32_t emitted[IAMF_HIP_FANOUT_MAX] = {0, 0, 0, 0};

  // ---- 1. the members that share the packets ----
  if (k) {
    FanLpParams fp;
    memset(&fp, 0, sizeof(fp));
    int n = 0;
    for (int j = 0; j < n_batches; ++j) {
      if (cls[j] != 2) continue;
      const RenderParams &p = pcs[j].p;
      if (n == 0) {
        fp.lpcm = p.lpcm;
        fp.lpcm_stream_stride = p.lpcm_stream_stride;
        fp.lpcm_frame_stride = p.lpcm_frame_stride;
        for (int m = 0; m < 16; ++m) fp.lpcm_off[m] = p.lpcm_off[m];
        fp.pos0 = p.pos0;
        fp.total = p.total;
        fp.frame_size = p.frame_size;
        fp.n_streams = p.n_streams;
        fp.stream0 = p.stream0;
        fp.n_launch = p.n_launch;
      }
      fp.mem[n++] = fan_member_of(p);
    }
    const auto fan_launch = !pk_more ? iamf_hip_fanout_lp_launch
                            : (form == LpcmForm::S24 ? iamf_hip_fanout_pk24_launch
                                                     : (form == LpcmForm::S16C ? iamf_hip_fanout_pk16c_launch : iamf_hip_fanout_pk24c_launch));
    if (!fan_launch(&fp, b0->m, k, static_cast<hipStream_t>(stream))) return IAMF_HIP_ERR_INTERNAL;
    HIPCHK(hipGetLastError());
    if (pk_more) iamf_hip_route_count(kRouteSetFanoutPackets, IAMF_HIP_ROUTE_FANOUT_PACKETS, pk_variant, b0->m, 0, k);   // by family only
    else iamf_hip_route_count(1, IAMF_HIP_ROUTE_FANOUT_LPCM, 0, b0->m, 0, k);   // the extension table
    for (int j = 0; j < n_batches; ++j) {
      if (cls[j] != 2) continue;
      const int r = render_commit(batches[j], pcs[j]);
      if (r < 0) return r;
      emitted[j] = r;
    }
    rep.n_fused = k;
    rep.input_fused = 1;
  }
  // ---- 2. the members whose single call reads the packets itself, in member order ----
  for (int j = 0; j < n_batches; ++j) {
    if (cls[j] != 1) continue;
    const int r = render_finish(batches[j], pcs[j]);
    if (r < 0) return r;
    emitted[j] = r;
  }
  // ---- 3. the members that need f32: one unpack pass into the first one's buffer, then the f32 fan-out over it ----
  if (n_f32) {
    iamf_hip_batch *sub_b[IAMF_HIP_FANOUT_MAX];
    void *sub_pcm[IAMF_HIP_FANOUT_MAX];
    int64_t sub_stride[IAMF_HIP_FANOUT_MAX];
    int32_t sub_emitted[IAMF_HIP_FANOUT_MAX] = {0, 0, 0, 0};
    int n = 0;
    for (int j = 0; j < n_batches; ++j) {
      if (cls[j] != 0) continue;
      sub_b[n] = batches[j];
      sub_pcm[n] = d_pcm[j];
      sub_stride[n] = pcm_stream_stride_bytes[j];
      ++n;
    }
    iamf_hip_render_args a = args[0];
    const int ur = lpcm_unpack_range(sub_b[0], in, n_frames, first, count, stream0, n_streams, static_cast<hipStream_t>(stream), a);
    if (ur != IAMF_HIP_OK) return ur;
    rep.n_unpacks = 1;
    int32_t f32_fused = 0;
    const int r = fanout_range_impl(sub_b, n, a.d_in, a.in_stream_stride, a.in_frame_stride, n_frames, n_samples, sub_pcm, sub_stride,
                                    stream, sub_emitted, &f32_fused, false, stream0, n_streams);
    if (r != IAMF_HIP_OK) return r;
    // the other members read the first one's buffer: it must not be re-used by that batch before they are done
    if (n > 1) HIPCHK(hipEventRecord(sub_b[0]->done, static_cast<hipStream_t>(stream)));
    if (!k) rep.n_fused = f32_fused;
    n = 0;
    for (int j = 0; j < n_batches; ++j)
      if (cls[j] == 0) emitted[j] = sub_emitted[n++];
  }
  for (int j = 0; j < n_batches; ++j) n_emitted[j] = emitted[j];
  if (report) *report = rep;
  return IAMF_HIP_OK;
}

int iamf_hip_batch_render_fanout_lpcm(iamf_hip_batch *const *batches, int32_t n_batches, const iamf_hip_lpcm_input *in,
                                      int32_t n_frames, int32_t n_samples, void *const *d_pcm,
                                      const int64_t *pcm_stream_stride_bytes, void *stream, int32_t stream0, int32_t n_streams,
                                      int32_t *n_emitted, iamf_hip_fanout_report *report) {
  return fanout_lpcm_impl(batches, n_batches, in, n_frames, n_samples, d_pcm, pcm_stream_stride_bytes, stream, stream0, n_streams,
                          n_emitted, report, false);
}

// The same with leave to read 24-bit and coupled packets in the shared launch (include/iamf_hip.h): render_fanout_kernel<..,
// LP, LPB, LPC>, IAMF_HIP_ROUTE_FANOUT_PACKETS.
// The call block is iamf_hip_batch_render_packets': the packets, and of its args the frames, the samples and the stream — the
// members' PCM buffers travel beside it, and a fan-out takes no ramps, frame records or f32 input, so every other field is 0.
int iamf_hip_batch_render_fanout_packets(iamf_hip_batch *const *batches, int32_t n_batches, const iamf_hip_packet_call *call,
                                         void *const *d_pcm, const int64_t *pcm_stream_stride_bytes, int32_t stream0, int32_t n_streams,
                                         int32_t *n_emitted, iamf_hip_fanout_report *report) {
  if (n_batches < 1 || n_batches > IAMF_HIP_FANOUT_MAX) return IAMF_HIP_ERR_BAD_ARG;   // (the first answer of the shared checks)
  if (!call || call->reserved[0] || call->reserved[1] || call->reserved[2] || call->reserved[3]) return IAMF_HIP_ERR_BAD_ARG;
  const iamf_hip_render_args &a = call->args;   // every field but n_frames, n_samples and stream: NULL / 0
  if (a.d_in || a.in_stream_stride || a.in_frame_stride || a.d_in2 || a.in2_stream_stride || a.in2_frame_stride || a.d_element_ramp ||
      a.d_element2_ramp || a.d_output_ramp || a.ramp_stream_stride || a.d_dmx_frames || a.d_pcm || a.pcm_stream_stride_bytes ||
      a.d_demix_frames || a.demix_sample0 || a.lfe_pre_samples || a.lfe_post_samples || a.reserved0)
    return IAMF_HIP_ERR_BAD_ARG;
  return fanout_lpcm_impl(batches, n_batches, &call->in, call->args.n_frames, call->args.n_samples, d_pcm, pcm_stream_stride_bytes,
                          call->args.stream, stream0, n_streams, n_emitted, report, true);
}

int iamf_hip_batch_flush_range(iamf_hip_batch *b, void *d_pcm, int64_t pcm_stream_stride_bytes, void *stream,
                               int32_t stream0, int32_t n_streams) {
  if (!b || !d_pcm) return IAMF_HIP_ERR_BAD_ARG;
  if (!range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  for (int i = stream0; i < stream0 + n_streams; ++i)
    if (b->sflushed[(size_t)i]) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b->cfg.limiter_enable) return 0;
  iamf_hip_render_args a;
  memset(&a, 0, sizeof(a));  // no inputs: 240 zero samples go through the limiter
  a.d_pcm = d_pcm;
  a.pcm_stream_stride_bytes = pcm_stream_stride_bytes;
  a.stream = stream;
  const int r = render_call(b, a, kDelay, stream0, n_streams, nullptr, nullptr, CallForm::Plain, 0);
  if (r >= 0)
    for (int i = stream0; i < stream0 + n_streams; ++i) b->sflushed[(size_t)i] = 1;
  return r;
}

int iamf_hip_batch_flush(iamf_hip_batch *b, void *d_pcm, int64_t pcm_stream_stride_bytes, void *stream) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  return iamf_hip_batch_flush_range(b, d_pcm, pcm_stream_stride_bytes, stream, 0, b->cfg.n_streams);
}

int iamf_hip_batch_set_second_element(iamf_hip_batch *b, const iamf_hip_matrix *mx, const float *g2) {
  if (b && !on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b || !mx || !mx->mat || mx->m <= 0 || mx->m > kMaxIn || mx->n <= 0 || mx->n > kMaxOut ||
      mx->kind == IAMF_HIP_KIND_DMX || b->any_rendered)
    return IAMF_HIP_ERR_BAD_ARG;
  std::vector<float> fm;
  int32_t feed[kMaxOut];
  build_feed_map(*mx, b->cfg.out_channels, fm, feed);
  const int ns = b->cfg.n_streams;
  std::vector<float> gains((size_t)ns, 1.0f);
  if (g2) memcpy(gains.data(), g2, sizeof(float) * ns);
  (void)hipFree(b->d_matrix2);
  (void)hipFree(b->d_gains2);
  (void)hipFree(b->d_src_feed2);
  b->d_matrix2 = nullptr;
  b->d_gains2 = nullptr;
  b->d_src_feed2 = nullptr;
  HIPCHK(hipMalloc(&b->d_matrix2, sizeof(float) * fm.size()));
  HIPCHK(hipMalloc(&b->d_gains2, sizeof(float) * ns));
  HIPCHK(hipMalloc(&b->d_src_feed2, sizeof(feed)));
  HIPCHK(hipMemcpy(b->d_matrix2, fm.data(), sizeof(float) * fm.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_gains2, gains.data(), sizeof(float) * ns, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_src_feed2, feed, sizeof(feed), hipMemcpyHostToDevice));
  b->m2 = mx->m;
  b->has2 = true;
  // the two-element packet form folds the decoder's 2^-15 into these weights as well (see lp_scale_ok)
  b->lp2_scale_ok = true;
  for (float w : fm)
    if (w != 0.f && !(fabsf(w) >= 0x1p-100f && fabsf(w) <= 0x1p100f)) b->lp2_scale_ok = false;
  return IAMF_HIP_OK;
}

// A frame of an element that feeds the HOA LFE generator is rendered and then trimmed away COMPLETELY (start + end trim =
// its length, neither of them the whole frame): the reference's filter has run over it (iamf_stream_render precedes
// iamf_frame_trim, IAMF_decoder.c:3372-3406), nothing is emitted.  Streams [first, first + count) only.
int iamf_hip_batch_lfe_advance(iamf_hip_batch *b, const float *d_in, int64_t in_stream_stride, int32_t n_samples, void *stream,
                               int32_t first, int32_t count) {
  if (!b || !d_in || n_samples <= 0 || n_samples > b->cfg.frame_size || first < 0 || count <= 0 || first + count > b->cfg.n_streams)
    return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b->lfe) return IAMF_HIP_OK;   // a layout without an LFE slot: no generator, nothing to advance
  int t4 = 0;
  return lfe_prepass(b, d_in, in_stream_stride, in_stream_stride, n_samples, static_cast<hipStream_t>(stream), first, count, &t4);
}

// The reference keeps the LFE generator's filter in the OUTPUT LAYOUT (IAMF_decoder.c:2629-2632: plfe =
// &stream->final_layout->sp.lfe_f), not in the stream: two scene-based elements of one presentation push their W channels
// through the same two histories in turn.  Two batches that render such a pair share the state: `b` adopts `owner`'s; the
// caller issues the calls of a frame in presentation order on one HIP stream.
int iamf_hip_batch_share_lfe_state(iamf_hip_batch *b, iamf_hip_batch *owner) {
  if (!b || !owner || b == owner) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b) || !on_batch_device(owner)) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b->lfe || !owner->lfe || owner->lfe_shared || b->lfe_shared || b->any_rendered || owner->any_rendered ||
      b->cfg.n_streams != owner->cfg.n_streams || b->cfg.sample_rate != owner->cfg.sample_rate)
    return IAMF_HIP_ERR_BAD_ARG;
  (void)hipFree(b->d_lfe_state);
  (void)hipFree(b->d_lfe_next);
  b->d_lfe_state = owner->d_lfe_state;
  b->d_lfe_next = owner->d_lfe_next;
  b->lfe_shared = true;
  return IAMF_HIP_OK;
}

int iamf_hip_batch_set_projection(iamf_hip_batch *b, const float *matrix, int l_in) {
  if (b && !on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b || !matrix || l_in <= 0 || l_in > kMaxIn || b->any_rendered || b->dmx || b->fir) return IAMF_HIP_ERR_BAD_ARG;
  (void)hipFree(b->d_pre);
  b->d_pre = nullptr;
  HIPCHK(hipMalloc(&b->d_pre, sizeof(float) * (size_t)l_in * b->m));
  HIPCHK(hipMemcpy(b->d_pre, matrix, sizeof(float) * (size_t)l_in * b->m, hipMemcpyHostToDevice));
  b->pre_l = l_in;
  // Tolerance mode (IAMF_HIP_PROJ_MFMA, or AUTO with an H2M matrix: results within +-1 LSB of the
  // reference): de-mapping and rendering are both linear, so one matrix W' = W * P^T (products and
  // sums in double, rounded once) takes the decoded channels straight to the output slots and the
  // call runs on the same kernels as a mono-mode element with l_in channels.  IAMF_HIP_PROJ_EXACT
  // keeps the reference's two stages and their f32 roundings (generic kernel).
  (void)hipFree(b->d_matrix_pre);
  b->d_matrix_pre = nullptr;
  if (!b->h_fm.empty()) {
    std::vector<float> w((size_t)b->n_feeds * l_in);
    for (int f = 0; f < b->n_feeds; ++f)
      for (int l = 0; l < l_in; ++l) {
        double acc = 0;
        for (int r = 0; r < b->m; ++r) acc += (double)b->h_fm[(size_t)f * b->m + r] * (double)matrix[(size_t)l * b->m + r];
        w[(size_t)f * l_in + l] = (float)acc;
      }
    int set = 0, all = 0;
    for (int g = 0; g < 6; ++g) b->nz_mask_pre[g] = 0;
    for (int g = 0; g < 6 && 4 * g < b->cfg.out_channels; ++g)
      for (int k = 0; k < l_in && k < 32; ++k) {
        bool nz = false;
        for (int c = 4 * g; c < 4 * g + 4 && c < b->cfg.out_channels; ++c)
          if (b->src_feed[c] >= 0 && w[(size_t)b->src_feed[c] * l_in + k] != 0.f) nz = true;
        ++all;
        if (nz) {
          ++set;
          b->nz_mask_pre[g] |= 1u << k;
        }
      }
    b->sparse_pre = 2 * set < all ? 1 : 0;
    HIPCHK(hipMalloc(&b->d_matrix_pre, sizeof(float) * w.size()));
    HIPCHK(hipMemcpy(b->d_matrix_pre, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
  }
  return IAMF_HIP_OK;
}

/* ---- demixer of scalable channel audio (reference src/iamf_dec/demixer.c) ---- */

int iamf_hip_batch_set_demixer(iamf_hip_batch *b, const iamf_hip_demix_config *c) {
  if (b && !on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  if (!b || !c || b->any_rendered || b->fir || b->d_pre) return IAMF_HIP_ERR_BAD_ARG;
  if (c->layout < 0 || c->layout > 8 || c->n_in != kLayoutCount[c->layout] || c->n_in != b->m ||
      c->n_gain < 0 || c->n_gain > 12)
    return IAMF_HIP_ERR_BAD_ARG;
  // which de-mix steps run: the reference reconstructs on demand (dmx_channel, demixer.c:379-424);
  // a step is skipped when its right-hand output is already there
  bool have[kChCount];
  for (int i = 0; i < kChCount; ++i) have[i] = false;
  for (int i = 0; i < c->n_in; ++i) {
    if (c->chs_in[i] <= 0 || c->chs_in[i] >= kChCount || have[c->chs_in[i]]) return IAMF_HIP_ERR_BAD_ARG;
    have[c->chs_in[i]] = true;
  }
  int steps = 0;
  bool ok = true;
  auto s2 = [&]() { if (!have[kChL2]) { ok = false; return; } if (have[kChR2]) return;
                    if (!have[kChMono]) { ok = false; return; } steps |= 1; have[kChR2] = true; };
  auto s3 = [&]() { if (have[kChR3]) return; s2(); if (!ok) return; if (!have[kChC]) { ok = false; return; }
                    steps |= 2; have[kChL3] = have[kChR3] = true; };
  auto s5 = [&]() { if (have[kChSR5]) return; s3(); if (!ok) return;
                    if (!have[kChL7] || !have[kChR7]) { ok = false; return; }
                    steps |= 4; have[kChSL5] = have[kChSR5] = true; };
  auto s7 = [&]() { if (have[kChBR7]) return; s5(); if (!ok) return;
                    if (!have[kChSL7] || !have[kChSR7]) { ok = false; return; }
                    steps |= 8; have[kChBL7] = have[kChBR7] = true; };
  auto h2 = [&]() { if (have[kChHR]) return; if (!have[kChTL] || !have[kChTR]) { ok = false; return; }
                    s5(); if (!ok) return; steps |= 16; have[kChHL] = have[kChHR] = true; };
  auto h4 = [&]() { if (have[kChHBR]) return; h2(); if (!ok) return;
                    if (!have[kChHFR] || !have[kChHFL]) { ok = false; return; }
                    steps |= 32; have[kChHBL] = have[kChHBR] = true; };
  int32_t tab[64];
  memset(tab, 0, sizeof(tab));
  for (int i = 0; i < c->n_in; ++i) {
    const int ch = kLayoutCh[c->layout][i];
    tab[i] = c->chs_in[i];
    tab[40 + c->chs_in[i]] = i;  // IAChannel -> decoded position (render_wide4.hpp)
    tab[12 + i] = ch;
    if (have[ch]) continue;
    switch (ch) {
      case kChR2: s2(); break;
      case kChL3: case kChR3: s3(); break;
      case kChSL5: case kChSR5: s5(); break;
      case kChBL7: case kChBR7: s7(); break;
      case kChHL: case kChHR: h2(); break;
      case kChHBL: case kChHBR: h4(); break;
      default: ok = false; break;
    }
    if (!ok || !have[ch]) return IAMF_HIP_ERR_BAD_ARG;
  }
  const int fs = b->cfg.frame_size;
  std::vector<float> ft(12 + 2 * (size_t)fs + 12, 0.f);
  float *gin = ft.data() + 12 + 2 * (size_t)fs;  // the same gains by decoded channel, for render_wide4.hpp
  for (int k = 0; k < 12; ++k) gin[k] = 1.f;
  int ng = 0, gmask = 0;
  bool gain_twice = false;
  for (int i = 0; i < c->n_gain; ++i) {  // dmx_gainup touches only channels that were decoded
    const int ch = c->gain_ch[i];
    int at = -1;
    for (int k = 0; k < c->n_in; ++k)
      if (c->chs_in[k] == ch) at = k;
    if (ch <= 0 || ch >= kChCount) return IAMF_HIP_ERR_BAD_ARG;
    if (at < 0) continue;
    tab[25 + ng] = ch;
    ft[ng] = c->gain[i];
    ++ng;
    gain_twice = gain_twice || ((gmask >> at) & 1);
    gmask |= 1 << at;
    gin[at] = c->gain[i];
  }
  tab[24] = ng;
  // demixer_open + demixer_set_frame_offset (demixer.c:476-567): Hann cross-fade of fs/16 samples
  // behind the first `skip` samples of every frame
  float *start = ft.data() + 12, *stop = start + fs;
  for (int i = 0; i < fs; ++i) {
    start[i] = 1;
    stop[i] = 0;
  }
  const int wl = fs / 8, ov = wl / 2, pre = (int)(c->frame_offset % (uint32_t)fs);
  if (pre + ov <= fs) {
    std::vector<float> hann((size_t)(wl > 0 ? wl : 1));
    for (int i = 0; i < wl; ++i) hann[i] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * (double)i / (double)(wl - 1))));
    for (int i = 0; i < pre; ++i) {
      start[i] = 0;
      stop[i] = 1;
    }
    for (int i = pre, j = 0; j < ov; ++i, ++j) {
      start[i] = hann[j];
      stop[i] = hann[j + ov];
    }
  }
  (void)hipFree(b->d_demix_tab);
  (void)hipFree(b->d_demix_ftab);
  b->d_demix_tab = nullptr;
  b->d_demix_ftab = nullptr;
  HIPCHK(hipMalloc(&b->d_demix_tab, sizeof(tab)));
  HIPCHK(hipMemcpy(b->d_demix_tab, tab, sizeof(tab), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&b->d_demix_ftab, sizeof(float) * ft.size()));
  HIPCHK(hipMemcpy(b->d_demix_ftab, ft.data(), sizeof(float) * ft.size(), hipMemcpyHostToDevice));
  b->demix = true;
  b->demix_steps = steps;
  b->demix_skip = pre;
  b->demix_layout = c->layout;
  b->demix_gmask = gmask;
  // the in-register demixer keeps the first 192 entries of the cross-fade windows and reads them 4 at a time
  b->demix_w4 = (!gain_twice && fs >= 256 && pre + ov <= 192 && (pre & 3) == 0) ? 1 : 0;
  return IAMF_HIP_OK;
}

namespace {
// demixer.c:66-78 (double literals narrowed to float) and fixedp11_5.c:81-82
const struct { float alpha, beta, gamma, delta; int woff; } kDemixMat[7] = {
    {1.0, 1.0, (float)0.707, (float)0.707, -1}, {(float)0.707, (float)0.707, (float)0.707, (float)0.707, -1},
    {1.0, (float)0.866, (float)0.866, (float)0.866, -1}, {0, 0, 0, 0, 0},
    {1.0, 1.0, (float)0.707, (float)0.707, 1}, {(float)0.707, (float)0.707, (float)0.707, (float)0.707, 1},
    {1.0, (float)0.866, (float)0.866, (float)0.866, 1}};
const float kDemixW[11] = {0.0, (float)0.0179, (float)0.0391, (float)0.0658, (float)0.1038, 0.25,
                           (float)0.3962, (float)0.4342, (float)0.4609, (float)0.4821, 0.5};
static void demix_factors(int mode, int w_idx, float out[5]) {
  out[0] = kDemixMat[mode].alpha;
  out[1] = kDemixMat[mode].beta;
  out[2] = kDemixMat[mode].gamma;
  out[3] = kDemixMat[mode].delta;
  out[4] = kDemixW[w_idx < 0 ? 0 : (w_idx > 10 ? 10 : w_idx)];
}
}  // namespace

void iamf_hip_demix_state_init(iamf_hip_demix_state *st) {
  memset(st, 0, sizeof(*st));
  for (int i = 0; i < 24; ++i) st->last_sfavg[i] = 1.0f;
}

int iamf_hip_demix_set_info(iamf_hip_demix_state *st, int mode, int w_idx) {
  if (!st || mode < 0 || mode == 3 || mode > 6) return IAMF_HIP_ERR_BAD_ARG;
  if (w_idx < 0 || w_idx > 10) {
    st->last_mode = st->mode;
    st->mode = mode;
    st->last_w_idx = st->w_idx;
    if (kDemixMat[mode].woff > 0)
      st->w_idx = st->last_w_idx + 1 < 10 ? st->last_w_idx + 1 : 10;
    else
      st->w_idx = st->last_w_idx - 1 > 0 ? st->last_w_idx - 1 : 0;
  } else {
    if (mode != st->mode) st->last_mode = st->mode = mode;
    if (st->w_idx != w_idx) st->last_w_idx = st->w_idx = w_idx;
  }
  return IAMF_HIP_OK;
}

void iamf_hip_demix_frame_fill(iamf_hip_demix_state *st, int n_recon, const int32_t *recon_ch,
                               const float *recon_gain, iamf_hip_demix_frame *out) {
  memset(out, 0, sizeof(*out));
  demix_factors(st->last_mode, st->last_w_idx, out->prev);
  demix_factors(st->mode, st->w_idx, out->cur);
  const float N = 7;
  out->n_recon = n_recon < 0 ? 0 : (n_recon > 12 ? 12 : n_recon);
  for (int i = 0; i < out->n_recon; ++i) {  // dmx_rms, demixer.c:447-478
    const int ch = recon_ch[i] > 0 && recon_ch[i] < 24 ? recon_ch[i] : 0;
    out->recon_ch[i] = ch;
    const float sf = recon_gain ? recon_gain[i] : 1.0f;
    const float sfavg = (2 / (N + 1)) * sf + (1 - 2 / (N + 1)) * st->last_sfavg[ch];
    out->recon_prev[i] = st->last_sfavg[ch];
    out->recon_cur[i] = sfavg;
    st->last_sfavg[ch] = sfavg;
  }
}

/* ---- down-mixer control plane (downmix_renderer.c:77-91,131-216; IAMF_utils.c:234-245;
 *      fixedp11_5.c:81-99) ---- */
int iamf_hip_dmx_layout_channels(int layout) { return layout >= 0 && layout < 9 ? kLayoutCount[layout] : 0; }

int iamf_hip_dmx_valid(int in, int out) {
  if (in == out || in < 0 || in >= 9 || out < 0 || out >= 9) return 0;  // binaural (9) is refused
  if (kLayoutTop[in] && !kLayoutTop[out]) return 0;
  return !(kLayoutSurround[in] < kLayoutSurround[out] || kLayoutTop[in] < kLayoutTop[out]);
}

void iamf_hip_dmx_state_init(iamf_hip_dmx_state *st) {
  memset(st, 0, sizeof(*st));
  st->mode = -1;
  st->w_idx = -1;
}

int iamf_hip_dmx_set_mode_weight(iamf_hip_dmx_state *st, int mode, int w_idx) {
  static const struct { float a, b, g, d; int woff; } mixf[7] = {
      {1.0, 1.0, (float)0.707, (float)0.707, -1}, {(float)0.707, (float)0.707, (float)0.707, (float)0.707, -1},
      {1.0, (float)0.866, (float)0.866, (float)0.866, -1}, {0, 0, 0, 0, 0},
      {1.0, 1.0, (float)0.707, (float)0.707, 1}, {(float)0.707, (float)0.707, (float)0.707, (float)0.707, 1},
      {1.0, (float)0.866, (float)0.866, (float)0.866, 1}};
  static const float wtab[11] = {0.0, (float)0.0179, (float)0.0391, (float)0.0658, (float)0.1038, 0.25,
                                 (float)0.3962, (float)0.4342, (float)0.4609, (float)0.4821, 0.5};
  if (!st || mode < 0 || mode == 3 || mode >= 7) return IAMF_HIP_ERR_BAD_ARG;
  if (st->mode != mode) {
    st->mode = mode;
    st->alpha = mixf[mode].a;
    st->beta = mixf[mode].b;
    st->gamma = mixf[mode].g;
    st->delta = mixf[mode].d;
    st->w_idx_offset = mixf[mode].woff;
  }
  if (w_idx < 0 || w_idx > 10) {  // no explicit index: step the weight state one way
    int nw = st->w_idx_offset > 0 ? (st->w_idx + 1 < 10 ? st->w_idx + 1 : 10) : (st->w_idx - 1 > 0 ? st->w_idx - 1 : 0);
    st->w_idx = nw;
    st->gamma_w = st->gamma * wtab[nw];
  } else if (st->w_idx != w_idx) {
    st->w_idx = w_idx;
    st->gamma_w = st->gamma * wtab[w_idx];
  }
  return IAMF_HIP_OK;
}

void iamf_hip_dmx_coefficients(const iamf_hip_dmx_state *st, float out[5]) {
  out[0] = st->alpha;
  out[1] = st->beta;
  out[2] = st->gamma;
  out[3] = st->delta;
  out[4] = st->gamma_w;
}

/* ---- per-stream lifecycle: restart, range gains, export, import (stream_state.hpp) ---- */

namespace {

// Field numbers of a batch's list: the bits of the kernels' field mask
enum { kFldLim = 0, kFldRingY, kFldRingPm, kFldLfeState, kFldLfeNext, kFldFirHist0, kFldFirHist1, kFldFirPre0, kFldFirPre1,
       kFldGain0, kFldGain1, kFldGain2, kFldGainE2, kFldCount };
constexpr uint32_t kFldGainMask = (1u << kFldGain0) | (1u << kFldGain1) | (1u << kFldGain2) | (1u << kFldGainE2);

// THE list: what reset_state touches, plus the gains.  *bytes (may be NULL) = bytes of one stream's blob.
StateFields batch_fields(const iamf_hip_batch *b, int64_t *bytes) {
  StateFields fl;
  memset(&fl, 0, sizeof(fl));
  const int ns = b->cfg.n_streams;
  fl.lim_n = b->n_end;
  static_assert(sizeof(LimState) == 4 * sizeof(float), "LimState travels as one 16-byte row");
  static_assert(kFldCount <= kStateMaxFields, "field list too long");
  state_add(fl, reinterpret_cast<float *>(b->d_lim), 4, kFreshLim, 0, true);
  state_add(fl, b->d_ring_y, b->cfg.out_channels * kSave, kFreshZero, 0, true);
  state_add(fl, b->d_ring_pm, kSave, kFreshZero, 0, true);
  const bool own_lfe = b->lfe && !b->lfe_shared;   // a borrowed filter state is its owner's to restart and to move
  state_add(fl, own_lfe ? b->d_lfe_state : nullptr, 4, kFreshZero, 0, true);
  state_add(fl, own_lfe ? b->d_lfe_next : nullptr, 2, kFreshZero, 0, true);
  // FIR: restart only (the history is a batch-wide ping-pong, fir_cur: both buffers are cleared)
  const int fm = b->m * 256;
  state_add(fl, b->fir ? b->d_fir_hist[0] : nullptr, fm, kFreshZero, 0, false);
  state_add(fl, b->fir ? b->d_fir_hist[1] : nullptr, fm, kFreshZero, 0, false);
  {  // the same history at the input's channel stride (RenderParams::fir_pre): G streams share the rows of a slab
    const int fs = b->cfg.frame_size, g = fs >= 256 ? fs / 256 : 1;
    for (int k = 0; k < 2; ++k)
      state_add_rows(fl, b->fir ? b->d_fir_pre[k] : nullptr, g, (int64_t)b->m * fs, 256, b->m, 256, fs, kFreshZero, 0, false);
  }
  for (int k = 0; k < 3; ++k) state_add(fl, b->d_gains + (size_t)k * ns, 1, kFreshValue, k, true);
  state_add(fl, b->has2 ? b->d_gains2 : nullptr, 1, kFreshValue, 3, true);
  const int64_t n = state_layout(fl);
  if (bytes) *bytes = n;
  return fl;
}

// everything the blob's layout and meaning depend on; not the matrices
uint32_t batch_signature(const iamf_hip_batch *b) {
  uint32_t thr_bits;
  memcpy(&thr_bits, &b->thr, 4);
  const uint32_t w[] = {kStateVersion, 1u /* kind */, (uint32_t)kSave, (uint32_t)sizeof(LimState), (uint32_t)b->cfg.out_channels,
                        b->cfg.limiter_enable ? 1u : 0u, thr_bits, (uint32_t)b->n_end, (uint32_t)b->n_atk,
                        (uint32_t)b->cfg.sample_rate, (b->lfe && !b->lfe_shared) ? 1u : 0u, b->has2 ? 1u : 0u};
  return state_hash(w, (int)(sizeof(w) / sizeof(w[0])));
}

// `st` behind everything queued on the batch so far, whatever stream that used
int lifecycle_enter(iamf_hip_batch *b, hipStream_t st) {
  if (b->rendered) HIPCHK(hipStreamWaitEvent(st, b->done, 0));
  return IAMF_HIP_OK;
}
// ... and the synchronous setters and destroy behind this call
int lifecycle_leave(iamf_hip_batch *b, hipStream_t st) {
  HIPCHK(hipEventRecord(b->done, st));
  b->rendered = true;
  return IAMF_HIP_OK;
}

// Restart job over [s0, s0 + cnt) with the field mask `mask`; the gains of `g` (rows NULL or not part of the mask are not
// read) travel in the kernel arguments, kStateChunk streams a launch.  Without gain fields: one launch.
int restart_launches(const StateFields &fl, uint32_t mask, int s0, int cnt, const iamf_hip_stream_gains *g, hipStream_t st) {
  StateValues vals;
  memset(&vals, 0, sizeof(vals));
  if (!(mask & kFldGainMask)) {
    stream_state_launch<StateJob::Restart>(fl, mask, s0, cnt, nullptr, 0, vals, st);
    HIPCHK(hipGetLastError());
    return IAMF_HIP_OK;
  }
  const float *rows[4] = {g->element_gain, g->output_gain, g->loudness_gain, g->element2_gain};
  for (int c0 = 0; c0 < cnt; c0 += kStateChunk) {
    const int c = cnt - c0 < kStateChunk ? cnt - c0 : kStateChunk;
    for (int k = 0; k < 4; ++k)
      if (rows[k]) memcpy(vals.v[k], rows[k] + c0, sizeof(float) * c);
    stream_state_launch<StateJob::Restart>(fl, mask, s0 + c0, c, nullptr, 0, vals, st);
    HIPCHK(hipGetLastError());
  }
  return IAMF_HIP_OK;
}

uint32_t gain_mask(const iamf_hip_stream_gains *g) {
  if (!g) return 0;
  return (g->element_gain ? 1u << kFldGain0 : 0u) | (g->output_gain ? 1u << kFldGain1 : 0u) |
         (g->loudness_gain ? 1u << kFldGain2 : 0u) | (g->element2_gain ? 1u << kFldGainE2 : 0u);
}

void gains_to_mirror(iamf_hip_batch *b, const iamf_hip_stream_gains *g, int s0, int cnt) {
  if (!g) return;
  const size_t ns = (size_t)b->cfg.n_streams;
  const float *rows[3] = {g->element_gain, g->output_gain, g->loudness_gain};
  for (int k = 0; k < 3; ++k)   // (the second element's gains have no host mirror: no setter re-uploads them)
    if (rows[k]) memcpy(&b->h_gains[k * ns + (size_t)s0], rows[k], sizeof(float) * cnt);
}

// the checks export and import share; *bytes = one stream's blob
int blob_args_check(const iamf_hip_batch *b, int32_t s0, int32_t cnt, const void *d_state, int64_t stride, const void *tickets,
                    int64_t *bytes) {
  if (!b || !d_state || !tickets) return IAMF_HIP_ERR_BAD_ARG;
  if (b->fir) return IAMF_HIP_ERR_UNIMPLEMENTED;
  if (!range_ok(b, s0, cnt)) return IAMF_HIP_ERR_BAD_ARG;
  (void)batch_fields(b, bytes);
  if (stride < *bytes || (stride & 15) || (reinterpret_cast<uintptr_t>(d_state) & 15)) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  return IAMF_HIP_OK;
}

}  // namespace

int iamf_hip_batch_set_gains_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, const iamf_hip_stream_gains *gains,
                                   void *stream) {
  if (!b || !gains || !range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  if (gains->element2_gain && !b->has2) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  const uint32_t mask = gain_mask(gains);
  if (!mask) return IAMF_HIP_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int r = lifecycle_enter(b, st);
  if (r != IAMF_HIP_OK) return r;
  r = restart_launches(batch_fields(b, nullptr), mask, stream0, n_streams, gains, st);
  if (r != IAMF_HIP_OK) return r;
  gains_to_mirror(b, gains, stream0, n_streams);
  return lifecycle_leave(b, st);
}

int iamf_hip_batch_restart_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, const iamf_hip_stream_gains *gains,
                                 void *stream) {
  if (!b || !range_ok(b, stream0, n_streams)) return IAMF_HIP_ERR_BAD_ARG;
  if (gains && gains->element2_gain && !b->has2) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int r = lifecycle_enter(b, st);
  if (r != IAMF_HIP_OK) return r;
  const uint32_t mask = (((1u << kFldCount) - 1u) & ~kFldGainMask) | gain_mask(gains);
  r = restart_launches(batch_fields(b, nullptr), mask, stream0, n_streams, gains, st);
  if (r != IAMF_HIP_OK) return r;
  gains_to_mirror(b, gains, stream0, n_streams);
  for (int i = stream0; i < stream0 + n_streams; ++i) {
    b->spos[(size_t)i] = 0;
    b->sflushed[(size_t)i] = 0;
  }
  return lifecycle_leave(b, st);
}

int64_t iamf_hip_batch_stream_state_bytes(const iamf_hip_batch *b) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  if (b->fir) return IAMF_HIP_ERR_UNIMPLEMENTED;
  int64_t bytes = 0;
  (void)batch_fields(b, &bytes);
  return bytes;
}

int iamf_hip_batch_export_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, void *d_state,
                                int64_t state_stream_stride_bytes, iamf_hip_stream_state *tickets, void *stream) {
  int64_t bytes = 0;
  int r = blob_args_check(b, stream0, n_streams, d_state, state_stream_stride_bytes, tickets, &bytes);
  if (r != IAMF_HIP_OK) return r;
  hipStream_t st = static_cast<hipStream_t>(stream);
  r = lifecycle_enter(b, st);
  if (r != IAMF_HIP_OK) return r;
  StateValues vals;
  memset(&vals, 0, sizeof(vals));
  const StateFields fl = batch_fields(b, nullptr);
  stream_state_launch<StateJob::Export>(fl, (1u << kFldCount) - 1u, stream0, n_streams, static_cast<float *>(d_state),
                                        state_stream_stride_bytes / 4, vals, st);
  HIPCHK(hipGetLastError());
  const uint32_t sig = batch_signature(b);
  for (int i = 0; i < n_streams; ++i) {   // the batch tracks the positions on the host, at enqueue
    iamf_hip_stream_state &t = tickets[i];
    memset(&t, 0, sizeof(t));
    t.magic = kStateMagic;
    t.version = kStateVersion;
    t.kind = 1;
    t.signature = sig;
    t.bytes = bytes;
    t.cursor[0] = b->spos[(size_t)(stream0 + i)];
    t.cursor[1] = b->sflushed[(size_t)(stream0 + i)];
  }
  return lifecycle_leave(b, st);
}

int iamf_hip_batch_import_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, const void *d_state,
                                int64_t state_stream_stride_bytes, const iamf_hip_stream_state *tickets, void *stream) {
  int64_t bytes = 0;
  int r = blob_args_check(b, stream0, n_streams, d_state, state_stream_stride_bytes, tickets, &bytes);
  if (r != IAMF_HIP_OK) return r;
  const uint32_t sig = batch_signature(b);
  for (int i = 0; i < n_streams; ++i) {
    const iamf_hip_stream_state &t = tickets[i];
    if (t.magic != kStateMagic || t.version != kStateVersion || t.kind != 1 || t.signature != sig || t.bytes != bytes ||
        t.cursor[0] < 0 || (t.cursor[1] != 0 && t.cursor[1] != 1))
      return IAMF_HIP_ERR_BAD_ARG;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  r = lifecycle_enter(b, st);
  if (r != IAMF_HIP_OK) return r;
  StateValues vals;
  memset(&vals, 0, sizeof(vals));
  const StateFields fl = batch_fields(b, nullptr);
  stream_state_launch<StateJob::Import>(fl, (1u << kFldCount) - 1u, stream0, n_streams,
                                        const_cast<float *>(static_cast<const float *>(d_state)), state_stream_stride_bytes / 4,
                                        vals, st);
  HIPCHK(hipGetLastError());
  for (int i = 0; i < n_streams; ++i) {
    b->spos[(size_t)(stream0 + i)] = tickets[i].cursor[0];
    b->sflushed[(size_t)(stream0 + i)] = (uint8_t)tickets[i].cursor[1];
  }
  b->any_rendered = true;
  return lifecycle_leave(b, st);
}

int iamf_hip_batch_reset(iamf_hip_batch *b) {
  if (!b) return IAMF_HIP_ERR_BAD_ARG;
  if (!on_batch_device(b)) return IAMF_HIP_ERR_INVALID_STATE;
  HIPCHK(hipDeviceSynchronize());
  return reset_state(b);
}

}  // extern "C"
