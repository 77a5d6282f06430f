// render_params.hpp — constants, per-stream state and the parameter block shared by the render kernels and the host
// code that routes a call to one of them (render_route.hpp).  Plain C++: no HIP, so that host-only code (the routing
// test, tests/route_host) can include it.  Like every render_*.hpp it is included INSIDE the including unit's namespace
// (the kernels' types stay in their translation unit's anonymous namespace) and therefore includes nothing itself: the
// unit includes <stdint.h> and include/iamf_hip.h in front.
#pragma once

constexpr int kChunk = 256;      // samples per workgroup step = threads per workgroup
constexpr int kDelay = 240;      // limiter look-ahead (reference common/audio_defines.h:41)
constexpr int kRing = 512;       // LDS ring length (power of two >= kChunk + kDelay + 15)
constexpr int kSave = 256;       // samples of ring persisted per stream between calls
constexpr int kHead = 256;       // coefficient-table head kept in LDS
constexpr int kMaxOut = 24;      // reference MAX_OUTPUT_CHANNELS
constexpr int kMaxIn = 24;

struct LimState {  // per stream, persisted in HBM between calls
  float g;   // currentGain
  float gs;  // targetStartGain
  float ge;  // targetEndGain
  int n;     // increments of currentTC since the last trigger; >= n_end means idle
};

struct RenderParams {
  const float *in;          // planar f32 element PCM (device) or nullptr = zeros (flush)
  int64_t in_stream_stride; // floats
  int64_t in_frame_stride;  // floats
  uint8_t *pcm;             // packed output (device)
  int64_t pcm_stream_stride;  // bytes
  const float *matrix;      // device, feed-major [n_feeds][M]
  const float *gains;       // device [3][n_streams]: element, output, loudness
  const float *ctab;        // device limiter coefficient table [n_end + 1]
  LimState *lim;            // device [n_streams]
  float *ring_y;            // device [n_streams][out_ch][kSave]
  float *ring_pm;           // device [n_streams][kSave]
  int64_t pos0;             // samples of each stream consumed before this call
  int32_t total;            // samples to process in this call
  int32_t frame_size;
  int32_t n_streams;        // streams of the batch (the per-stream arrays' extent)
  int32_t stream0, n_launch;  // the streams this launch renders: workgroup i takes stream stream0 + i
  int32_t n_feeds;
  int32_t out_ch;
  int32_t out_format;
  int32_t limiter_on;
  int32_t loudness_on;
  int32_t use_mfma;         // wide kernel: projection on v_mfma_f32_32x32x2_f32 instead of VALU
  int32_t n_atk, n_end;     // limiter table split points
  float thr;
  const int32_t *src_feed;  // device [out_ch]: output slot -> feed index, -1 = silent slot, -2 = LFE slot
                            // fed by the HOA LFE generator (render_lfe.hpp; generic and wide4 kernels)
  // wide4 VALU projection: bit m of nz_mask[g] = some output slot 4g..4g+3 has a non-zero weight for
  // input m; sparse = less than half of those bits are set (then all-zero weight batches are skipped)
  uint32_t nz_mask[6];
  int32_t sparse;
  int32_t lpcm_coupled;     // (LPCM block below) 1: the packets have the coupled 16-bit form (lpcm_form.hpp, S16C); 2: the coupled
                            // 24-bit form (S24C, with lpcm_bytes == 3: iamf_hip_batch_render_packets); 0: as before.
                            // Host only — the kernels know it at compile time — and kept HERE, in what was padding in front
                            // of the next pointer, like lpcm_bytes: no kernel's arguments move
  // ---- optional extras (generic kernel only) ----
  const float *in2;         // second element (planar f32) or nullptr
  int64_t in2_stream_stride, in2_frame_stride;
  const float *matrix2;     // device, feed-major [n_feeds2][m2]
  const int32_t *src_feed2; // device [out_ch]
  const float *gains2;      // device [n_streams] element-2 constant gain
  int32_t m2;
  int32_t dmx_on;           // element 0 is rendered by the parametric down-mixer
  const float *elem_ramp, *elem2_ramp, *out_ramp;  // per-sample gains of this call or nullptr
  int64_t ramp_stream_stride;
  const iamf_hip_dmx_frame *dmx_frames;  // device [n_streams][frames of this call]
  int32_t dmx_n_in, dmx_n_out;
  int32_t dmx_in_layout, dmx_out_layout;  // IAChannelLayoutType ids (render_downmix.hpp)
  const int32_t *dmx_tab;   // device [24]: IAChannel ids of the inputs, then (from [12]) of the outputs
  // ---- ambisonics projection de-mapping in front of element 0 (generic kernel) ----
  const float *pre_matrix;  // device [pre_l][M] or nullptr
  int32_t pre_l;            // decoded channels per frame when pre_matrix is set
  // ---- demixer of scalable channel audio in front of element 0 (generic kernel) ----
  int32_t demix_on;
  int32_t demix_steps;      // bit 0 S1to2, 1 S2to3, 2 S3to5, 3 S5to7, 4 TF2toT2, 5 T2toT4
  int32_t demix_skip;       // samples at the start of every frame that use the previous mode
  int32_t demix_i0;         // frame position of the call's first sample (trimmed single-frame calls)
  int32_t lpcm_mix;         // (RenderMixParams below) 0, or the form of a second element handed over as LPCM packets: 1 mono-coded
                            // runs, 2 one coupled pair (render_fast_kernel's LP2).  `in2` then holds the packets' address and
                            // in2_stream_stride / in2_frame_stride their strides in BYTES, for pick_route; the kernel reads
                            // RenderMixParams.  Host only, and kept HERE, in what was padding in front of the next pointer,
                            // like lpcm_bytes: no kernel's arguments move
  const int32_t *demix_tab; // device: [0..12) chs_in, [12..24) chs_out, [24] n_gain, [25..37) gain_ch,
                            //         [40..64) decoded position of an IAChannel (0 if it is not decoded)
  const float *demix_ftab;  // device: [0..12) gains, start_window[frame_size], stop_window[frame_size],
                            //         then [0..12) the gain of every decoded channel (1 where none)
  const iamf_hip_demix_frame *demix_frames;  // device [n_streams][frames of this call]
  int32_t demix_layout;     // IAChannelLayoutType of the target layout (render_wide4_kernel<.., DMX>)
  int32_t demix_gmask;      // bit m: decoded channel m takes the output gain demix_ftab[12 + 2*frame_size + m]
  int32_t demix_w4;         // 1 if the in-register demixer of render_wide4.hpp covers this configuration
  int32_t interleaved;      // 1: the call came through iamf_hip_batch_render_interleaved (frame size 1: `in` is ordinary interleaved
                            // f32) and may take render_fast_kernel<.., IL, RAG> (pick_route: Family::FastInterleaved); 0: every
                            // rule as it stood.  Host only, and kept HERE, in what was padding in front of the next pointer,
                            // like lpcm_bytes: the block keeps its size and every other field its offset
  // ---- render_wide4.hpp: where lanes that have nothing to emit send their 16-byte store, so that every
  //      chunk issues the same vector-memory instructions and the compiler can COUNT them (s_waitcnt vmcnt(N)
  //      instead of vmcnt(0) at the top of the chunk loop); device [n_streams][256 lanes][16 B] ----
  uint8_t *dump;
  // ---- HOA LFE generator (render_lfe.hpp): raw low-pass output of this call or nullptr ----
  const float *lfe;         // device, transposed by blocks of 64 streams: element lfe_index(s, k, lfe_t4) (render_lfe.hpp)
  int32_t lfe_t4;           // quads per stream in that buffer
  int32_t og_ch;            // output channels the OUTPUT gain multiplies (iamf_hip_batch_config::out_gain_channels; = out_ch: all)
  int32_t lfe_k0;           // the generator's output of the call's first sample sits at index lfe_k0 (trimmed frames: the
                            // filter also ran over the lfe_k0 samples cut off in front, iamf_hip_render_args)
  int32_t ragged;           // the call's mark, a CallMark (below): which entry the call came through, where that entry's own kernel
                            // form may take it; kCallPlain: every rule as it stood.  Host only, and kept HERE, in the 4 bytes of
                            // padding in front of the double, like lpcm_bytes: the block keeps its size and every other field
                            // its offset
  double lfe_div;           // sqrt(n) of h2m_rdr.c:1162; 0 = the `* 0.5` form (n <= 2)
  int32_t lfe_mask;         // bit c: output slot c is an LFE slot (src_feed[c] == -2), for render_wide4.hpp
  // ---- HRTF FIR renderer (render_fast_kernel<M, 2, true>): matrix = h[2][M][fir_taps] ----
  int32_t fir_taps;
  const float *fir_hist;    // device [n_streams][M][256] input history before this call
  float *fir_hist_next;     // device, same shape: history after this call
  const void *fir_h16;      // device: split-f16 filter tables [M][ear][hi/lo][shift 8][304] (render_fir16.hpp) or nullptr
  float fir_inv_scale;      // 1 / (filter scale * input scale) of those tables
  int32_t lpcm_bytes;       // (LPCM block below) bytes per packet sample: 0 or 2 = 16 bit, 3 = 24 bit.  Host only — the kernels
                            // know it at compile time — and kept HERE, in what was padding in front of the next pointer:
                            // the block keeps its size and every other field its offset, so no kernel's arguments move
  const float *fir_pq;      // device: spectra tables of the FFT stage [pairs][16][64] x 4 floats (render_fir_fft.hpp) or nullptr
  const float *fir_tw;      // device: its twiddles [16][64] + [16][4] complex
  const float *fir_zero;    // device: zero floats, M * frame size of them (what that stage loads for runs past the end of a
                            // call, at the input's channel stride)
  // the same history as fir_hist at the INPUT's channel stride, for fir_fft_kernel's two-base fetch (frame size a multiple
  // of 256 and >= 1024, M even): stream s, channel c, sample j of the last 256 at
  //   ((s / G) * M + c) * frame_size + (s % G) * 256 + j,   G = frame_size / 256   (G streams share the rows of a slab)
  const float *fir_pre;
  float *fir_pre_next;
  float *fir_y;             // device scratch [n_streams][2][total]: the FFT stage's output when it runs as a kernel of its own
  const float *fir_id_matrix;   // device: the 2 x 2 identity (feed-major) and its slot map, for the limiter / pack kernel behind it
  const int32_t *fir_id_feed;
  // ---- element 0 handed over as LPCM packets (render_fast_kernel<.., LP>, iamf_hip_batch_render_lpcm): 16-bit
  //      little-endian samples, one contiguous run per channel and frame.  Sample i of channel m, frame f, stream s:
  //      lpcm + s * lpcm_stream_stride + f * lpcm_frame_stride + lpcm_off[m] + 2 * i (bytes; every term a multiple of 8
  //      for i a multiple of 4).  `in` is not read then.  lpcm_bytes == 3 (above): 24-bit samples, 3 * i, every term a
  //      multiple of 4 (lpcm_form.hpp).  lpcm_coupled (above): channels m, m + 1 of a pair are interleaved, sample i of
  //      the pair's first channel at lpcm_off[m] + 4 * i and its partner's 2 bytes on (S24C: 6 * i, 3 bytes on) ----
  const uint8_t *lpcm;
  int64_t lpcm_stream_stride, lpcm_frame_stride;
  int32_t lpcm_off[16];
};

// The values of RenderParams::ragged.  Each is set by one entry alone (render_prepare, iamf_render.hip) and read by one rule of
// pick_route (render_route.hpp); a call whose rule does not hold routes as the entry named behind "else".
enum CallMark : int32_t {
  kCallPlain = 0,
  kCallRagged = 1,            // iamf_hip_batch_render_ragged: planar f32 that is no whole number of 64-sample blocks may take
                              // render_fast_kernel<.., IL = false, RAG = true> (Family::FastRagged)
  kCallPacketsRagged = 2,     // iamf_hip_batch_render_packets_ragged: element 0 as packets (`lpcm`), no whole number of blocks, may
                              // take render_fast_kernel<.., LP, .., RAG = true> (Family::PacketsRagged)
  kCallPacketsMixRagged = 3,  // iamf_hip_batch_render_packets_mix_ragged: both elements as packets (`lpcm`, `lpcm_mix`), no whole
                              // number of blocks, may take render_fast_kernel<.., IN2, LP, .., LP2, false, RAG = true>
                              // (Family::PacketsMixRagged)
  kCallPacketsNolim = 4,      // iamf_hip_batch_render_packets_nolim: element 0 as packets takes render_nolim_kernel<M, LPB, LPC>
                              // (Family::NolimPackets) — render_prepare sets the mark only where that rule holds, else
                              // kCallPacketsRagged
  kCallPacketsMixNolim = 5,   // iamf_hip_batch_render_packets_mix_nolim: both elements as packets (RenderMixParams) take
                              // render_nolim_kernel<M, LPB, LPC, LP2> (Family::NolimPacketsMix) — set only where that rule holds,
                              // else kCallPacketsMixRagged
};
// The frame position of a packet call's first sample (iamf_hip_lpcm_input::first_sample; the two inputs of a mix share it).  It
// travels in demix_i0, which no packet-fed kernel reads: no demixer runs beside packets.  Set with every mark from
// kCallPacketsRagged on.
inline int32_t call_first_sample(const RenderParams &p) { return p.demix_i0; }

// render_fast_kernel<.., LP2> (iamf_hip_batch_render_lpcm_mix): the block above and, behind it, the SECOND element as 16-bit
// little-endian LPCM packets.  Sample i of its channel m, frame f, stream s: lpcm2 + s * lpcm2_stream_stride + f *
// lpcm2_frame_stride + lpcm2_off[m] + 2 * i (mono-coded runs), or lpcm2_off[0] + 4 * i and 2 bytes on for the L and R of one
// coupled pair; every term a multiple of 8.  A type of its own: the block above keeps its size for every other kernel.
struct RenderMixParams : RenderParams {
  const uint8_t *lpcm2;
  int64_t lpcm2_stream_stride, lpcm2_frame_stride;
  int32_t lpcm2_off[4];
};

// IAChannel ids (reference IAMF_types.h:61-90; L5/R5 alias L7/R7)
enum {
  kChNone = 0, kChL7, kChR7, kChC, kChLFE, kChSL7, kChSR7, kChBL7, kChBR7, kChHFL, kChHFR, kChHBL,
  kChHBR, kChMono, kChL2, kChR2, kChTL, kChTR, kChL3, kChR3, kChSL5, kChSR5, kChHL, kChHR, kChCount
};
