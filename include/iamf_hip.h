/*
 * iamf_hip.h — C ABI of the MI355X-native IAMF post-decode renderer (libiamf_hip.so).
 *
 * Plain C: pointers, sizes and PODs only.  Every entry point names the reference interface
 * (Samsung/iac, paths relative to the reference tree) it stands in for.  The reference renders
 * one decoder handle, one frame at a time on the CPU; this ABI renders a BATCH of independent
 * streams x frames per call on one GPU, with the same per-stream arithmetic and stage order
 * (render -> element gain -> mix -> output gain -> loudness -> limiter -> PCM pack,
 * src/iamf_dec/IAMF_decoder.c:3335-3500).  There is no CPU fallback: every call fails with
 * IAMF_HIP_ERR_DEVICE if HIP is unusable.
 *
 * Pointers named d_* are DEVICE pointers owned by the caller (any allocator: hipMalloc, a
 * torch tensor's data_ptr ...).  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Calls are asynchronous on that stream unless stated otherwise.  The stream may be one
 * created with hipStreamNonBlocking: a call leaves no work on the null stream that its own stream
 * could overtake (tests/test_gpu_streams.py).
 * One exception holds for every render entry: scratch of the batch grows with the largest call seen
 * (the LFE generator's pre-pass, the HRTF stage's output, the natural-layout rows of a fixed PCM
 * channel stride, the f32 copy of unfused packets).  The call in which it grows waits, on the host,
 * for the batch's last call (whatever stream that used) and for `stream`, then replaces the buffer.
 * A call no larger than an earlier one on the same batch never waits.
 */
#ifndef IAMF_HIP_H
#define IAMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes: same numeric values as IAMF_defines.h:181-190, plus one for the device */
enum {
  IAMF_HIP_OK = 0,
  IAMF_HIP_ERR_BAD_ARG = -1,
  IAMF_HIP_ERR_BUFFER_TOO_SMALL = -2,
  IAMF_HIP_ERR_INTERNAL = -3,
  IAMF_HIP_ERR_INVALID_STATE = -5,
  IAMF_HIP_ERR_UNIMPLEMENTED = -6,
  IAMF_HIP_ERR_ALLOC_FAIL = -7,
  IAMF_HIP_ERR_DEVICE = -100
};

/* rendering ids of loudspeaker layouts, same values as src/iamf_dec/ae_rdr.h:40-61 */
enum {
  IAMF_HIP_SS_A = 0x020, IAMF_HIP_SS_B = 0x050, IAMF_HIP_SS_C = 0x250, IAMF_HIP_SS_D = 0x450,
  IAMF_HIP_SS_E = 0x451, IAMF_HIP_SS_F = 0x370, IAMF_HIP_SS_G = 0x490, IAMF_HIP_SS_H = 0x9A3,
  IAMF_HIP_SS_I = 0x070, IAMF_HIP_SS_J = 0x470,
  IAMF_HIP_L_STEREO = 0x200, IAMF_HIP_L_51 = 0x510, IAMF_HIP_L_512 = 0x512,
  IAMF_HIP_L_514 = 0x514, IAMF_HIP_L_71 = 0x710, IAMF_HIP_L_714 = 0x714,
  IAMF_HIP_L_MONO = 0x100, IAMF_HIP_L_712 = 0x712, IAMF_HIP_L_312 = 0x312,
  IAMF_HIP_L_BINAURAL = 0x1020
};

/* element renderer kinds.  DMX = the parametric down-mixer (downmix_renderer.c): matrix.in_id /
 * out_id are IAChannelLayoutType values (IAMF_defines.h:196-209), matrix.mat is unused. */
enum { IAMF_HIP_KIND_H2M = 0, IAMF_HIP_KIND_M2M = 1, IAMF_HIP_KIND_DMX = 2, IAMF_HIP_KIND_FIR = 3 };
/* FIR = binaural HRTF convolution: of a scene-based element (the role of
 * IAMF_element_renderer_render_H2B, h2b_rdr.c:109-130; matrix.m = ambisonics channels 1 / 4 / 9 / 16) or of
 * a channel-based element (the role of IAMF_element_renderer_render_M2B, m2b_rdr.c:103-121, taken by the
 * reference when headphones_rendering_mode == 1, IAMF_decoder.c:2562-2570; matrix.m = channels of the
 * element's loudspeaker layout 2 / 6 / 8 / 10 / 12, playback order, one HRIR pair per loudspeaker — a
 * zero pair mutes a channel, e.g. the LFE).  matrix.n = 2, matrix.mat = HRIRs h[ear][channel][fir_taps]
 * (host), out_channels = 2, limiter on.
 *   y[ear][t] = sum_c sum_k h[ear][c][k] * x[c][t-k]     (MFMA; fir_taps <= 256)
 * PARITY UNPINNED: the reference's binauraliser arithmetic lives in Resonance Audio / BEAR, which
 * are not in the reference tree; this formula is this library's specification. */

/* Projection arithmetic for output layouts wider than stereo.
 *   EXACT: VALU, separate f32 multiply and add in the reference's order -> bit-identical PCM.
 *   MFMA : v_mfma_f32_16x16x4_f32 (render_wide4.hpp; v_mfma_f32_32x32x2_f32 in the fallback render_wide.hpp):
 *          exact f32 products, fused k-ordered accumulation -> PCM within
 *          +-1 LSB of the reference (rounding ties only).
 *   AUTO : MFMA for the HOA projection (h2m_rdr.c:1103-1112, a dense contraction), EXACT for
 *          channel-layout matrices (m2m_rdr.c:1826-1837) and always for mono/stereo/binaural. */
enum { IAMF_HIP_PROJ_AUTO = 0, IAMF_HIP_PROJ_EXACT = 1, IAMF_HIP_PROJ_MFMA = 2 };

/* output sample formats.  16/24/32 = interleaved little-endian integer PCM exactly as
 * iamf_decoder_plane2stride_out writes it (IAMF_decoder.c:121-167).  F32 = the limiter output
 * as interleaved float, unscaled: a stage tap for parity tests, not a reference format. */
enum { IAMF_HIP_FMT_S16 = 16, IAMF_HIP_FMT_S24 = 24, IAMF_HIP_FMT_S32 = 32, IAMF_HIP_FMT_F32 = -32 };

/* A static rendering matrix: what IAMF_element_renderer_get_H2M_matrix (h2m_rdr.c:1070-1081,
 * struct h2m_rdr_t ae_rdr.h:142-151) or _get_M2M_matrix (m2m_rdr.c:1786-1804, struct m2m_rdr_t
 * ae_rdr.h:134-140) return.  `mat` points into the library's table (host memory, m*n floats,
 * H2M: mat[n*m_size+m], M2M: mat[m*n_size+n]) and stays valid for the process lifetime. */
typedef struct {
  int32_t kind;     /* IAMF_HIP_KIND_* */
  int32_t in_id;    /* H2M: ambisonics order 0..3 ; M2M: rendering id of the input layout */
  int32_t out_id;   /* rendering id of the output layout */
  int32_t channels; /* H2M: table `channels` field ; M2M: n */
  int32_t lfe1, lfe2;
  int32_t m, n;
  const float *mat;
} iamf_hip_matrix;

/* replaces IAMF_element_renderer_get_H2M_matrix, src/iamf_dec/h2m_rdr.c:1070 (0 or -1) */
int iamf_hip_get_h2m_matrix(int order, int out_id, iamf_hip_matrix *out);
/* replaces IAMF_element_renderer_get_M2M_matrix, src/iamf_dec/m2m_rdr.c:1786 (0 or -1) */
int iamf_hip_get_m2m_matrix(int in_id, int out_id, iamf_hip_matrix *out);
/* The reference has two sets of layout->layout tables, chosen at build time: m2m_rdr.c:36-830 under
 * -DSAMSUNG_TV (the upstream default, CMakeLists.txt:14-19) and :831-1628 otherwise; 47 of the 140
 * matrices differ.  This library carries both; iamf_hip_get_m2m_matrix is VARIANT_DEFAULT (= the
 * -DSAMSUNG_TV=OFF build).  The HOA tables are the same in both builds. */
enum { IAMF_HIP_VARIANT_DEFAULT = 0, IAMF_HIP_VARIANT_SAMSUNG_TV = 1 };
int iamf_hip_get_m2m_matrix_variant(int variant, int in_id, int out_id, iamf_hip_matrix *out);
/* channels of an output layout by rendering id (IAMF_decoder.c:3998-4008); 0 if unknown */
int iamf_hip_layout_channels(int out_id);

/* ------------------------------------------------------------------------------------------
 * Batched renderer: N independent streams that share one topology (same element layout, same
 * output layout, same frame size, bit depth and limiter settings) and keep separate state.
 * ---------------------------------------------------------------------------------------- */
typedef struct iamf_hip_batch iamf_hip_batch;

typedef struct {
  int32_t n_streams;
  int32_t frame_size;     /* samples per frame of element PCM (e.g. 1024) */
  int32_t sample_rate;    /* Hz; limiter time constants depend on it */
  int32_t out_channels;   /* channels of the output layout = PCM stride (IAMF_decoder.c:3497-3499) */
  int32_t out_format;     /* IAMF_HIP_FMT_* (IAMF_decoder_set_bit_depth, IAMF_decoder.h:161) */
  iamf_hip_matrix matrix; /* element renderer; `mat` may also be a caller-owned host array */
  int32_t limiter_enable; /* IAMF_decoder_peak_limiter_enable, IAMF_decoder.h:170 */
  float limiter_threshold_db; /* IAMF_decoder_peak_limiter_set_threshold, IAMF_decoder.h:179;
                                 attack 1 ms, release 200 ms, look-ahead 240 are the reference's
                                 constants (common/audio_defines.h:38-41) */
  int32_t loudness_enable; /* normalization_loudness != 0 (IAMF_decoder.c:3480) */
  int32_t projection;      /* IAMF_HIP_PROJ_*: how layouts with more than 2 channels are projected */
  int32_t fir_taps;        /* kind FIR: taps per HRIR (1..256) */
  int32_t lfe_hoa;         /* kind H2M into a layout with an LFE slot: 1 = the HOA LFE generator of
                              h2m_rdr.c:1151-1239 fills it (2nd-order Butterworth low-pass at 120 Hz over
                              ambisonics channel 0, scaled by 1/sqrt(n)), as a reference built with its
                              switch -DDISABLE_LFE_HOA=0 does (call site IAMF_decoder.c:2625-2636);
                              0 = the default build's silence (ae_rdr.h:63-65) */
  int32_t pcm_stride_channels; /* 0 = out_channels.  Otherwise the PCM is laid out as
                              iamf_decoder_plane2stride_out does with that `stride` (IAMF_decoder.c:121-167): the
                              -DSAMSUNG_TV build always passes SAMSUNG_SPECIFIC_CHANNELS = 12 (:3492-3495,
                              IAMF_defines.h:211-213) — sample-frame i starts at element 12 i, slots beyond
                              out_channels are zero, and for layouts of more than 12 channels the surplus
                              channels overwrite the following sample-frame exactly as the reference's loop
                              does.  A stream then needs (n * stride + max(0, out_channels - stride)) samples
                              of room per call. */
  /* 0, or K < out_channels: the OUTPUT mix gain (constant or ramp) multiplies output channels 0 .. K-1 only.  What the
   * reference's -DSAMSUNG_TV build does after a run-time switch to a layout of more channels: its mixed frame keeps the
   * channel count of the layout the presentation was enabled with, and iamf_frame_gain loops over that
   * (IAMF_decoder.c:1383-1408,3462-3469).  Such a batch renders through the general kernel. */
  int32_t out_gain_channels;
  int32_t reserved[2];
} iamf_hip_batch_config;

/* Creates device state for cfg->n_streams streams on the CURRENT HIP device.  Synchronous: it waits
 * for the null stream, and the state is in place on return, for a first render on any stream.
 * The batch remembers that device: every later call on it (setters, render, flush, reset) returns
 * IAMF_HIP_ERR_INVALID_STATE unless the same device is current; destroy switches to it and back.
 * Replaces, per stream: iamf_stream_renderer_open (IAMF_decoder.c:2480),
 * audio_effect_peak_limiter_create/_init (audio_effect_peak_limiter.c:50,73). */
int iamf_hip_batch_create(const iamf_hip_batch_config *cfg, iamf_hip_batch **out);
/* Synchronous: waits for the last call queued on the batch (the batch's own event, whatever stream
 * that call used), then frees; the PCM of a render queued before it is complete when it returns. */
void iamf_hip_batch_destroy(iamf_hip_batch *b);

/* Per-stream linear gains (host arrays of n_streams floats, NULL = leave unchanged):
 * element mix gain and output mix gain as iamf_frame_gain applies a constant gain
 * (IAMF_decoder.c:1392-1397: only if != 1 and > 0), and the loudness gain
 * db2lin(target - loudness) of iamf_loudness_process (IAMF_decoder.c:3206-3221).  Synchronous, and ordered after the renders already queued: it
 * first waits for the batch's last render / flush call (an event the batch itself records behind every call, so the
 * caller's stream need not outlive the call).  Only the rows given are uploaded: a NULL row keeps what the device holds,
 * the values of iamf_hip_batch_set_gains_range, _restart_range and _import_range included. */
int iamf_hip_batch_set_gains(iamf_hip_batch *b, const float *element_gain,
                             const float *output_gain, const float *loudness_gain);

/* Renders n_frames frames of every stream.
 *   d_in : planar f32 element PCM, sample i of channel c of frame f of stream s at
 *          d_in[s*in_stream_stride + f*in_frame_stride + c*frame_size + i]   (strides in floats)
 *   d_pcm: packed output; the k-th sample-frame this call emits for stream s starts at byte
 *          s*pcm_stream_stride_bytes + k*out_channels*bytes_per_sample
 * Returns the number of sample-frames emitted PER STREAM (>= 0; the limiter withholds the
 * first 240 of a stream's life exactly like audio_effect_peak_limiter_process_block :185-201)
 * or a negative IAMF_HIP_ERR_*.  This is the batched form of the render..pack section of
 * iamf_decoder_internal_decode (IAMF_decoder.c:3374-3500) i.e. of iamf_stream_render,
 * iamf_frame_gain, iamf_mixer_mix, iamf_loudness_process,
 * audio_effect_peak_limiter_process_block and iamf_decoder_plane2stride_out. */
int iamf_hip_batch_render(iamf_hip_batch *b, const float *d_in, int64_t in_stream_stride,
                          int64_t in_frame_stride, int32_t n_frames, void *d_pcm,
                          int64_t pcm_stream_stride_bytes, void *stream);

/* ---- parametric down-mixer control (host side of src/iamf_dec/downmix_renderer.c) ---- */
typedef struct {
  int32_t mode, w_idx;     /* -1 until set (DMRenderer_open, downmix_renderer.c:151-152) */
  int32_t w_idx_offset;
  int32_t reserved;
  float alpha, beta, gamma, delta; /* MixFactors of the mode (IAMF_utils.c:236-240) */
  float gamma_w;                   /* gamma * w(w_idx): the TL/TR weight (downmix_renderer.c:199-211) */
} iamf_hip_dmx_state;

/* one frame of one stream: samples [0, offset) use `prev`, the rest `cur`
 * ({alpha, beta, gamma, delta, gamma_w}); this is how iamf_stream_render applies a demixing mode
 * change (IAMF_decoder.c:2574-2583) */
typedef struct {
  int32_t offset;
  float prev[5];
  float cur[5];
} iamf_hip_dmx_frame;

/* 1 if DMRenderer_open(in, out) would succeed (downmix_renderer.c:77-91,131-139), else 0 */
int iamf_hip_dmx_valid(int in_layout, int out_layout);
/* channel count of an IAChannelLayoutType (IAMF_utils.c:111), 0 if invalid */
int iamf_hip_dmx_layout_channels(int layout);
void iamf_hip_dmx_state_init(iamf_hip_dmx_state *st);
/* replaces DMRenderer_set_mode_weight (downmix_renderer.c:180-216): 0 or IAMF_HIP_ERR_BAD_ARG */
int iamf_hip_dmx_set_mode_weight(iamf_hip_dmx_state *st, int mode, int w_idx);
/* copies the state's five coefficients into out[5] */
void iamf_hip_dmx_coefficients(const iamf_hip_dmx_state *st, float out[5]);

/* A second audio element for the mix (a sub-mix carries 1 or 2, IAMF_OBU.c:742-752): its renderer
 * matrix (H2M or M2M) and, per stream, its constant element mix gain.  Call before the first
 * render.  The mix is  0 + element0 + element1  in that order (iamf_mixer_mix,
 * IAMF_decoder.c:2719-2730). */
int iamf_hip_batch_set_second_element(iamf_hip_batch *b, const iamf_hip_matrix *mx,
                                      const float *element2_gain);

/* HOA LFE generator with TWO scene-based elements: the reference keeps the filter in the output layout
 * (IAMF_decoder.c:2629-2632, h2m_rdr.c:1151-1239), so both elements' W channels run through the same two histories in
 * turn, frame by frame, in presentation order.  Two batches created with lfe_hoa (same n_streams and sample rate, nothing
 * rendered yet) that render such a pair: `b` adopts `owner`'s filter state; the caller issues each frame's calls in
 * presentation order on ONE HIP stream, and destroys `b` before `owner`.  IAMF_HIP_OK / _BAD_ARG / _INVALID_STATE. */
int iamf_hip_batch_share_lfe_state(iamf_hip_batch *b, iamf_hip_batch *owner);
/* HOA LFE generator: a frame that is rendered and then trimmed away completely (start + end trim = its length, neither of
 * them the whole frame: iamf_stream_render precedes iamf_frame_trim, IAMF_decoder.c:3372-3406).  The generator's filter
 * runs over the frame's n_samples (d_in: the element's planar rows of the frame, as for a render call) for streams
 * [first, first + count); nothing is emitted.  IAMF_HIP_OK (also for a batch without a generator) / _BAD_ARG / _DEVICE. */
int iamf_hip_batch_lfe_advance(iamf_hip_batch *b, const float *d_in, int64_t in_stream_stride, int32_t n_samples, void *stream,
                               int32_t first, int32_t count);
/* Ambisonics projection de-mapping in front of element 0's renderer (projection-mode scene-based
 * elements): x[r] = sum over the l_in decoded channels l, ascending, of in[l] * matrix[l*m + r]
 * (iamf_core_decoder_convert_projection, src/iamf_dec/IAMF_core_decoder.c:116-130).  `matrix` is a
 * host array of l_in * m floats (the Q15 demixing matrix of the bitstream as floats); afterwards
 * element 0's input carries l_in channels per frame instead of m.  Call before the first render.
 * With IAMF_HIP_PROJ_EXACT the two stages run as the reference runs them (bit-exact); in tolerance
 * mode (IAMF_HIP_PROJ_MFMA, or _AUTO with an H2M matrix: +-1 LSB of the PCM) they are composed into
 * one matrix on the host and the call costs what a mono-mode element of l_in channels costs. */
int iamf_hip_batch_set_projection(iamf_hip_batch *b, const float *matrix, int l_in);

/* ------------------------------------------------------------------------------------------
 * Demixer of scalable channel audio in front of element 0's renderer (reference
 * src/iamf_dec/demixer.c, driven per frame by iamf_stream_scale_decoder_demix,
 * IAMF_decoder.c:2324-2349).  Element 0's input then carries the decoded channels of all layers up
 * to the chosen one in their bitstream order; the demixer applies the layers' output gains,
 * reconstructs the channels the target layout lacks (S1to2 ... S5to7, TF2toT2, T2toT4 with the
 * frame's demixing mode), smooths the recon gains and hands the renderer the target layout in
 * playback order.  Channel ids are IAChannel values (IAMF_types.h:61-90).
 * ------------------------------------------------------------------------------------------ */
typedef struct iamf_hip_demix_config {
  int32_t layout;         /* target IAChannelLayoutType 0..8 (demixer_set_channel_layout) */
  int32_t n_in;           /* decoded channels = channels of `layout` (demixer_set_channels_order) */
  int32_t chs_in[12];
  int32_t n_gain;         /* demixer_set_output_gain */
  int32_t gain_ch[12];
  float gain[12];
  uint32_t frame_offset;  /* demixer_set_frame_offset: the codec's delay (0 for LPCM) */
} iamf_hip_demix_config;

/* Call before the first render; the batch's matrix must take the target layout's channels. */
int iamf_hip_batch_set_demixer(iamf_hip_batch *b, const iamf_hip_demix_config *cfg);

/* Host-side state of one stream's demixer (demixer_set_demixing_info, demixer.c:592-618, and the
 * recon-gain smoothing of dmx_rms, :447-478). */
typedef struct iamf_hip_demix_state {
  int32_t mode, last_mode, w_idx, last_w_idx;
  float last_sfavg[24];
} iamf_hip_demix_state;

/* What the kernel needs for one frame of one stream (device array [n_streams][n_frames]). */
typedef struct iamf_hip_demix_frame {
  float prev[5], cur[5];            /* alpha, beta, gamma, delta, w of the previous / current mode:
                                       the first frame_offset % frame_size samples use prev */
  int32_t n_recon;                  /* channels of demixer_set_recon_gain valid for this frame: decoded or */
  int32_t recon_ch[12];             /* reconstructed channels of the target layout; distinct IAChannel ids */
  float recon_prev[12], recon_cur[12]; /* per recon channel: smoothed gain of the last frame / of this one */
} iamf_hip_demix_frame;

void iamf_hip_demix_state_init(iamf_hip_demix_state *st);
/* replaces demixer_set_demixing_info: 0 or IAMF_HIP_ERR_BAD_ARG (then nothing changes) */
int iamf_hip_demix_set_info(iamf_hip_demix_state *st, int mode, int w_idx);
/* fills one frame record from the state and the recon channels / gains valid for this frame
 * (recon_gain[i] belongs to recon_ch[i]), and advances the smoothing */
void iamf_hip_demix_frame_fill(iamf_hip_demix_state *st, int n_recon, const int32_t *recon_ch,
                               const float *recon_gain, iamf_hip_demix_frame *out);

/* Everything one render call can take.  Unused pointers are NULL. */
typedef struct {
  const float *d_in;            /* element 0 planar f32, layout as iamf_hip_batch_render */
  int64_t in_stream_stride, in_frame_stride;
  const float *d_in2;           /* element 1 (needs iamf_hip_batch_set_second_element) */
  int64_t in2_stream_stride, in2_frame_stride;
  /* per-sample mix gains for this call, [n_streams][n_frames*frame_size] f32 on the device,
   * built by the host like iamf_database_parameter_get_mix_gain_unit (IAMF_decoder.c:857-982);
   * when given they are multiplied in unconditionally (iamf_frame_gain, :1401-1405) and the
   * constant gain of that stage is not used */
  const float *d_element_ramp, *d_element2_ramp, *d_output_ramp;
  int64_t ramp_stream_stride;   /* floats */
  const iamf_hip_dmx_frame *d_dmx_frames; /* kind DMX: [n_streams][n_frames] on the device */
  int32_t n_frames;
  int32_t n_samples;            /* 0, or with n_frames == 1: render only the first n_samples of the frame
                                   (a frame shortened by iamf_frame_trim, IAMF_decoder.c:1361-1381) */
  void *d_pcm;
  int64_t pcm_stream_stride_bytes;
  void *stream;
  const iamf_hip_demix_frame *d_demix_frames; /* with a demixer: [n_streams][n_frames] on the device */
  int32_t demix_sample0;        /* with a demixer and n_frames == 1: position inside its frame of the call's
                                   first sample (a frame whose start was trimmed before the call) */
  /* HOA LFE generator and a TRIMMED frame (n_frames == 1): the reference renders the whole frame and trims the result
   * (iamf_stream_render then iamf_frame_trim, IAMF_decoder.c:3424-3430), so its low-pass filter also runs over the samples
   * that are cut.  d_in points at the first KEPT sample of every channel row; the generator additionally takes the
   * lfe_pre_samples in front of it and the lfe_post_samples behind the call's last sample from the same rows (W, or every
   * decoded channel in projection mode).  lfe_pre_samples + samples + lfe_post_samples <= frame_size.  0 otherwise. */
  int32_t lfe_pre_samples, lfe_post_samples, reserved0;
} iamf_hip_render_args;

/* Extended form of iamf_hip_batch_render; same return value. */
int iamf_hip_batch_render_ex(iamf_hip_batch *b, const iamf_hip_render_args *args);

/* The same for the streams [stream0, stream0 + n_streams) of the batch only; the others neither advance nor emit.
 * Buffers, strides and the per-stream arrays of `args` are still indexed by the stream's number in the batch.  The
 * streams of the range must stand at the same position (they have consumed the same number of samples) and must not
 * have been flushed, else IAMF_HIP_ERR_INVALID_STATE; after ranges have diverged, the whole-batch calls return that too
 * until the positions meet again.  IAMF_HIP_ERR_UNIMPLEMENTED for a proper sub-range of a batch of kind FIR or with
 * lfe_hoa (state that is kept per batch).  This is what lets a set of decoder handles that do NOT advance in step —
 * a frame trimmed in one stream, a temporal unit still incomplete in another, one stream ending before the rest — share
 * one batch (iamf_hip_decoder_group below); each reference handle is its own state machine, IAMF_decoder.c:3303-3525. */
int iamf_hip_batch_render_range(iamf_hip_batch *b, const iamf_hip_render_args *args, int32_t stream0, int32_t n_streams);
int iamf_hip_batch_flush_range(iamf_hip_batch *b, void *d_pcm, int64_t pcm_stream_stride_bytes, void *stream,
                               int32_t stream0, int32_t n_streams);

/* End of stream: pushes 240 zero samples through each stream's limiter and emits the withheld
 * tail (iamf_delay_buffer_handle, IAMF_decoder.c:3250-3301).  Returns sample-frames per stream. */
int iamf_hip_batch_flush(iamf_hip_batch *b, void *d_pcm, int64_t pcm_stream_stride_bytes,
                         void *stream);

/* One element rendered into several batches (the layouts of a mix presentation; several mix presentations over one
 * element, each with its own gains and bit depth) with ONE pass over the input where that is possible.
 *
 * Meaning: for every j the call leaves batches[j] (device state, position, the event the setters wait for) and d_pcm[j]
 * exactly as
 *   n_emitted[j] = iamf_hip_batch_render(batches[j], d_in, in_stream_stride, in_frame_stride, n_frames, d_pcm[j],
 *                                        pcm_stream_stride_bytes[j], stream)
 * would, called for j = 0 .. n_batches - 1 in turn: bit for bit, for every output format, gains, threshold, limiter on
 * or off.  The members keep the persisted state they have, so this call and the single-batch calls may be mixed freely
 * on the same batches.  The flush stays per batch (iamf_hip_batch_flush reads no input).
 *
 * Which members share the input is decided from what the call can observe, not by the caller: a member that
 * iamf_hip_batch_render would hand to the one- / two-channel limiter kernel as it is (limiter on, one or two output
 * channels, a call of whole 64-sample blocks on 16-byte aligned buffers, no HRTF stage, projection de-mapping, LFE
 * generator or fixed PCM channel stride, an element of 4, 9, 16, 6, 8 or 12 channels) is fusable; if at least two are,
 * they go to one launch that reads the element once (4 * M + sum of the members' output bytes per sample-frame instead
 * of 4 * M per member).  Every other member is rendered as iamf_hip_batch_render renders it, in member order, on the
 * same stream.  *n_fused (may be NULL) receives the number of members the shared launch rendered: 0 or
 * 2 .. IAMF_HIP_FANOUT_MAX — the caller's traffic accounting.
 *
 * Returns IAMF_HIP_OK or a negative IAMF_HIP_ERR_*.  Every argument and state check runs before the first launch; a call
 * they refuse changes no member.
 *   IAMF_HIP_ERR_BAD_ARG           n_batches outside 1 .. IAMF_HIP_FANOUT_MAX; a NULL pointer (n_fused excepted); the same
 *                                  batch twice; members that differ in n_streams, frame_size or input channel count;
 *                                  whatever iamf_hip_batch_render refuses for a member with these arguments (a batch with a
 *                                  down-mixer, a demixer or a second element needs the records of iamf_hip_batch_render_ex)
 *   IAMF_HIP_ERR_BUFFER_TOO_SMALL  as the single call, per member
 *   IAMF_HIP_ERR_INVALID_STATE     wrong current device; members that do not all stand at the same position for every
 *                                  stream; a flushed stream
 * The count and NULL checks need no device.  A device error in the middle (IAMF_HIP_ERR_DEVICE) is as for the single
 * call: members already queued have advanced. */
#define IAMF_HIP_FANOUT_MAX 4
int iamf_hip_batch_render_fanout(iamf_hip_batch *const *batches, int32_t n_batches, const float *d_in,
                                 int64_t in_stream_stride, int64_t in_frame_stride, int32_t n_frames, void *const *d_pcm,
                                 const int64_t *pcm_stream_stride_bytes, void *stream, int32_t *n_emitted /* host, [n_batches] */,
                                 int32_t *n_fused /* host, one int, may be NULL */);
/* ... for the streams [stream0, stream0 + n_streams) of every member only: iamf_hip_batch_render_range per member.  The
 * streams of the range must stand at one position in every member and be unflushed (IAMF_HIP_ERR_INVALID_STATE); a member
 * of kind FIR with a proper sub-range is IAMF_HIP_ERR_UNIMPLEMENTED, as for the single call; stream0 < 0, n_streams <= 0
 * (checked without a device) or a range outside the members IAMF_HIP_ERR_BAD_ARG.  Buffers and strides are still indexed
 * by the stream's number in the batch; PCM rows outside the range are not written. */
int iamf_hip_batch_render_fanout_range(iamf_hip_batch *const *batches, int32_t n_batches, const float *d_in,
                                       int64_t in_stream_stride, int64_t in_frame_stride, int32_t n_frames, void *const *d_pcm,
                                       const int64_t *pcm_stream_stride_bytes, void *stream, int32_t *n_emitted /* host, [n_batches] */,
                                       int32_t *n_fused /* host, one int, may be NULL */, int32_t stream0, int32_t n_streams);

/* ------------------------------------------------------------------------------------------
 * Sample-rate converter for a batch of streams (the decoder's speexdsp-derived resampler at
 * quality 4, src/iamf_dec/resample.c; the decoder only creates one when the stream rate differs
 * from the requested output rate, IAMF_decoder.c:3193-3199).  Buffers are interleaved f32
 * [sample-frame][channel] on the device: the output of a batch with IAMF_HIP_FMT_F32, the input
 * of a batch with frame_size 1.
 * ---------------------------------------------------------------------------------------- */
typedef struct iamf_hip_resampler iamf_hip_resampler;
/* replaces speex_resampler_init(channels, in, out, 4) + speex_resampler_skip_zeros as
 * iamf_stream_resampler_open calls them (IAMF_decoder.c:1892-1909); one state per stream */
int iamf_hip_resampler_create(int n_streams, int channels, int in_rate, int out_rate,
                              iamf_hip_resampler **out);
/* Create is synchronous: it waits for the null stream, and the tables and zeroed histories are in
 * place on return, for a first call on any stream.  The resampler records no event: destroy frees
 * at once, so the caller first waits for the calls it queued on it. */
void iamf_hip_resampler_destroy(iamf_hip_resampler *r);
/* sample-frames the output buffer must hold for ns input frames: ns * (out/in + 1), integer
 * division, as iamf_resample asks (IAMF_decoder.c:3225-3226) */
int iamf_hip_resampler_out_capacity(const iamf_hip_resampler *r, int ns);
int iamf_hip_resampler_flush_capacity(const iamf_hip_resampler *r);
/* replaces iamf_resample / speex_resampler_process_interleaved_float (IAMF_decoder.c:3223-3248,
 * resample.c:974-997).  Stream strides in floats.  Returns sample-frames produced per stream. */
int iamf_hip_resampler_process(iamf_hip_resampler *r, const float *d_in, int64_t in_stream_stride,
                               int ns, float *d_out, int64_t out_stream_stride, void *stream);
/* end of stream (rest_flag 2, IAMF_decoder.c:3227-3232): drains the filter latency */
int iamf_hip_resampler_flush(iamf_hip_resampler *r, float *d_out, int64_t out_stream_stride, void *stream);
/* The same for the streams [stream0, stream0 + n_streams) only (buffers and strides are indexed by the stream's number in
 * the resampler): every stream keeps its own phase and history, so streams need not advance in step — a range must consist
 * of streams in ONE state (iamf_hip_resampler_same_state; IAMF_HIP_ERR_INVALID_STATE otherwise): streams that have
 * consumed the same sequence of call lengths always are. */
int iamf_hip_resampler_process_range(iamf_hip_resampler *r, const float *d_in, int64_t in_stream_stride, int ns, float *d_out,
                                     int64_t out_stream_stride, void *stream, int32_t stream0, int32_t n_streams);
int iamf_hip_resampler_flush_range(iamf_hip_resampler *r, float *d_out, int64_t out_stream_stride, void *stream, int32_t stream0,
                                   int32_t n_streams);
int iamf_hip_resampler_same_state(const iamf_hip_resampler *r, int32_t stream_a, int32_t stream_b);

/* Forgets all stream state (new IA sequence: limiter re-initialised as in
 * iamf_decoder_internal_configure, IAMF_decoder.c:3809-3815).  Synchronous: waits for the whole
 * device (every stream), and the fresh state is in place on return, for a next render on any stream. */
int iamf_hip_batch_reset(iamf_hip_batch *b);

/* ------------------------------------------------------------------------------------------
 * Per-stream lifecycle: streams of one batch need not live and die in step.
 * The range calls above let the streams of a batch ADVANCE independently; these let them start, end and move
 * independently: a slot whose stream ended is restarted for the next programme while its neighbours go on rendering
 * (each reference handle is closed and opened on its own, IAMF_decoder.c:3809-3815), its gains are set without stopping
 * anybody, and a live stream's state is exported into a blob of plain bytes and imported into another slot, another
 * batch, or a batch on another device, where it continues bit for bit.
 *
 * All entries below are STREAM-ORDERED and never make the host wait for the device: `stream` first waits (on the
 * device) for the event the batch records behind every call, so the entry is ordered behind every render or flush
 * already queued on the batch whatever stream that used; the entry then records the event behind itself, so that the
 * synchronous setters and destroy wait for it in turn.  Renders queued AFTER an entry are ordered behind it the way
 * renders are ordered among themselves: by being issued on the same stream (or behind an event of the caller's).
 * Every argument is checked before the first device call; a refused call changes nothing, on the host or the device.
 * IAMF_HIP_ERR_INVALID_STATE unless the batch's device is current.
 *
 * What travels: the limiter's state and look-ahead rings, the HOA LFE generator's filter state when the batch OWNS it
 * (a batch that borrowed it through iamf_hip_batch_share_lfe_state leaves it alone, as iamf_hip_batch_reset does), the
 * stream's gains, its position.  What does not: the matrices and every other per-batch constant (the target batch has
 * its own), and the stage state the CALLER holds — iamf_hip_dmx_state and iamf_hip_demix_state are the caller's own
 * host data and travel with the caller.
 * ---------------------------------------------------------------------------------------- */
typedef struct {            /* host arrays of n_streams (of the RANGE) floats each; NULL = leave that gain as it is */
  const float *element_gain, *output_gain, *loudness_gain, *element2_gain;
} iamf_hip_stream_gains;

/* iamf_hip_batch_set_gains for the streams [stream0, stream0 + n_streams), without the host wait: the new values hold
 * for every render queued after the call and for none queued before it; the host arrays may be reused on return (the
 * values travel in kernel arguments).  element2_gain on a batch without a second element: IAMF_HIP_ERR_BAD_ARG. */
int iamf_hip_batch_set_gains_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams,
                                   const iamf_hip_stream_gains *gains, void *stream);
/* Leaves the streams of the range exactly as iamf_hip_batch_create leaves them (position 0, not flushed, limiter idle,
 * rings and filter histories zero) and stores the new gains where `gains` names some; streams outside the range and
 * batch-wide state are not touched.  Over the whole batch it is iamf_hip_batch_reset without the device-wide wait.
 * Serves batches of kind FIR too (both history buffers of the range are cleared). */
int iamf_hip_batch_restart_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams,
                                 const iamf_hip_stream_gains *gains /* may be NULL */, void *stream);

typedef struct {            /* host-side ticket of one exported stream; plain data, may be stored or sent */
  uint32_t magic, version;  /* layout of this struct and of the blob */
  uint32_t kind;            /* 1 = batch stream, 2 = resampler stream */
  uint32_t signature;       /* hash of everything the blob's layout and meaning depend on */
  int64_t bytes;            /* bytes of the device blob for this stream */
  int64_t cursor[2];        /* batch: {samples consumed, flushed}; resampler: {last_sample, frac} */
} iamf_hip_stream_state;

/* Bytes of one stream's blob, a multiple of 16; negative IAMF_HIP_ERR_UNIMPLEMENTED for batches of kind FIR (their
 * history is a batch-wide ping-pong and their parity is unpinned), IAMF_HIP_ERR_BAD_ARG for NULL.  Needs no device. */
int64_t iamf_hip_batch_stream_state_bytes(const iamf_hip_batch *b);
/* Export reads only: stream stream0 + i of the batch -> the blob at d_state + i * state_stream_stride_bytes (device,
 * 16-byte aligned, stride a multiple of 16 and >= the blob's bytes), gathered on `stream`; tickets[i] is filled at call
 * time (the batch tracks positions on the host).  The blob holds no pointers: the caller may copy it anywhere.
 * Import writes the range of any batch whose signature equals the tickets' — same output channel count, limiter
 * setting / threshold / sample rate, owned LFE state or none, second element or none; the matrices, the frame size and
 * the PCM format may differ — sets the streams' positions from the tickets and counts as a first render for the setters
 * that must precede it.  The streams then continue bit for bit as the source would have, and a neighbour that stands at
 * the same position may share a range launch with them.  The blob is the caller's buffer: import reads it on `stream`,
 * behind whatever the caller queued there.
 * IAMF_HIP_ERR_BAD_ARG: a ticket whose magic, version, kind, signature or bytes do not match the target, a stride
 * smaller than the blob, a range outside the batch — nothing is written.  IAMF_HIP_ERR_UNIMPLEMENTED: kind FIR. */
int iamf_hip_batch_export_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, void *d_state,
                                int64_t state_stream_stride_bytes, iamf_hip_stream_state *tickets /* host, [n_streams] */, void *stream);
int iamf_hip_batch_import_range(iamf_hip_batch *b, int32_t stream0, int32_t n_streams, const void *d_state,
                                int64_t state_stream_stride_bytes, const iamf_hip_stream_state *tickets, void *stream);

/* The same for the resampler (tickets of kind 2; the signature covers channels, both rates and the filter length).
 * The resampler keeps no event of its own: like its process calls, these are ordered by the stream they are issued on.
 * Restart: the host phase goes back to what iamf_hip_resampler_create sets and both history rows of the range are
 * zeroed.  Import writes the range's rows into ONE of the two history buffers — the one the stream below the range uses,
 * else the one above it, else the range's first stream's own — so that an imported stream can join its neighbour's
 * launches (iamf_hip_resampler_same_state) when their phases agree. */
int iamf_hip_resampler_restart_range(iamf_hip_resampler *r, int32_t stream0, int32_t n_streams, void *stream);
int64_t iamf_hip_resampler_stream_state_bytes(const iamf_hip_resampler *r);
int iamf_hip_resampler_export_range(iamf_hip_resampler *r, int32_t stream0, int32_t n_streams, void *d_state,
                                    int64_t state_stream_stride_bytes, iamf_hip_stream_state *tickets, void *stream);
int iamf_hip_resampler_import_range(iamf_hip_resampler *r, int32_t stream0, int32_t n_streams, const void *d_state,
                                    int64_t state_stream_stride_bytes, const iamf_hip_stream_state *tickets, void *stream);

/* bytes one output sample occupies for a format (2, 3, 4) */
int iamf_hip_format_bytes(int out_format);
/* library / build identification string (static storage) */
const char *iamf_hip_version(void);

/* ------------------------------------------------------------------------------------------
 * Diagnostics (not part of the render path).  Launches a kernel with the render kernels' HBM traffic
 * SHAPE and no compute: one 256-thread workgroup per stream, per 1024-sample chunk every lane reads
 * `rows` x 16 B (a frame of rows x 4 KiB per chunk, prefetched one chunk ahead) and writes `pieces` x 16 B
 * (1 KiB contiguous per wave and store instruction).  rows = input channels, pieces = out_channels / 2 for
 * s16.  Time it on the caller's stream to know what the memory system delivers for that shape on THOSE
 * buffers (bench.py: roofline.same_traffic_no_compute).  The buffers' contents are read / overwritten.
 * ---------------------------------------------------------------------------------------- */
int iamf_hip_probe_traffic(int n_streams, int chunks, int rows, int pieces, const void *d_in,
                           int64_t in_stream_stride_bytes, void *d_out, int64_t out_stream_stride_bytes,
                           void *stream);
/* Where the stream buffers live matters (NOTEBOOK.md 3): a batch whose input and PCM output lie in
 * device-memory regions of the same kind runs ~14 % slower than one whose buffers lie in regions of different kinds,
 * and hipMalloc does not say which is which.  This times iamf_hip_probe_traffic on every (input candidate, output
 * candidate) pair — one untimed and three timed launches each, the median — and reports the fastest pair in
 * *best_in / *best_out (indices into the candidate arrays); ms, if not NULL, receives the n_in x n_out medians in
 * milliseconds, row-major.  Synchronous; the candidates' contents are read / overwritten.  At most 256 candidates
 * of each. */
int iamf_hip_pick_buffer_pair(int n_streams, int chunks, int rows, int pieces, const void *const *d_in_candidates,
                              int n_in, int64_t in_stream_stride_bytes, void *const *d_out_candidates, int n_out,
                              int64_t out_stream_stride_bytes, void *stream, int *best_in, int *best_out, float *ms);

/* Self-test (diagnostic): the demixer's quotients through a shared reciprocal (q = n r, e = fma(-d, q, n), q' = fma(e, r,
 * q); iac_amd/csrc/render_common.hpp w4_quot) against the IEEE division n / d for ALL 2^32 f32 numerators, on the
 * device.  counts[0] = numerators inside the range the kernels use the fast form for (2^-100 <= |n| < 2^126), counts[1] =
 * those of them whose quotient differs in any bit (must be 0), counts[2] = numerators outside the range that differ
 * (the kernels divide those the IEEE way).  Synchronous. */
int iamf_hip_selftest_shared_divisor(float divisor, uint64_t counts[3]);

/* ------------------------------------------------------------------------------------------
 * Decoder facade extension.  The reference chooses at BUILD time whether scene-based elements feed
 * the LFE of the output layout (-DDISABLE_LFE_HOA=0; default: compiled out, ae_rdr.h:63-65).  This
 * library carries both builds: the switch is per decoder handle (an IAMF_DecoderHandle of this
 * library's IAMF_decoder.h), to be set before IAMF_decoder_configure; its default is off, or on if
 * the environment has IAMF_HIP_LFE_HOA=1 when the handle is opened.
 * ---------------------------------------------------------------------------------------- */
int iamf_hip_decoder_set_hoa_lfe(void *decoder_handle, int enable);
/* Which build of the reference the handle behaves as: IAMF_HIP_VARIANT_SAMSUNG_TV = its tables
 * (m2m_rdr.c:36-830), 12-channel PCM stride (IAMF_decoder.c:3492-3495,3510-3512), always the top layer of a
 * scalable element (:1782-1822).  Before IAMF_decoder_configure; default VARIANT_DEFAULT, or SAMSUNG_TV if
 * the environment has IAMF_HIP_SAMSUNG_TV=1 when the handle is opened. */
int iamf_hip_decoder_set_variant(void *decoder_handle, int variant);

/* ------------------------------------------------------------------------------------------
 * One node, several GPUs, from C (BASELINE north_star: "independent IAMF streams shard embarrassingly
 * across the 8 GPUs of one node with RCCL over xGMI only for the final batched gather").  All state of the path is per
 * decoder handle in the reference (IAMF_decoder_private.h:342-345, audio_effect_peak_limiter.h:48-73), so the streams
 * of a job are split into contiguous blocks, one batch per device, no exchange while rendering.  A shard owns, per
 * device: the batch, a HIP stream for rendering, a second one for the gather, and a host thread that issues that
 * device's launches.  RCCL is loaded with dlopen at the first gather (the library does not link it; a host without it
 * gets IAMF_HIP_ERR_UNIMPLEMENTED from the gather and can still render; IAMF_HIP_RCCL_LIB in the environment names the
 * library to load instead of the system's librccl).
 * ---------------------------------------------------------------------------------------- */
typedef struct iamf_hip_shard iamf_hip_shard;
/* block of streams of device `index` of `n_devices`: sizes differ by at most one, the larger blocks first */
int iamf_hip_shard_split(int n_streams, int n_devices, int index, int *first, int *count);
/* cfg->n_streams = streams of the whole job; devices = n_devices distinct HIP device ordinals (NULL = 0 .. n_devices - 1) */
int iamf_hip_shard_create(const iamf_hip_batch_config *cfg, const int *devices, int n_devices, iamf_hip_shard **out);
void iamf_hip_shard_destroy(iamf_hip_shard *s);
int iamf_hip_shard_devices(const iamf_hip_shard *s);
int iamf_hip_shard_info(const iamf_hip_shard *s, int index, int *device, int *first, int *count);
/* the batch of device `index` (for the per-stream setters: make that device current first) and its render stream */
iamf_hip_batch *iamf_hip_shard_batch(iamf_hip_shard *s, int index);
void *iamf_hip_shard_render_stream(iamf_hip_shard *s, int index);
/* iamf_hip_batch_render / _flush on every device at once: d_in[i] / d_pcm[i] are device i's buffers (its block of streams,
 * strides as for the batch).  Returns sample-frames emitted per stream.  Asynchronous on the devices' render streams. */
int iamf_hip_shard_render(iamf_hip_shard *s, const float *const *d_in, int64_t in_stream_stride, int64_t in_frame_stride,
                          int32_t n_frames, void *const *d_pcm, int64_t pcm_stream_stride_bytes);
int iamf_hip_shard_flush(iamf_hip_shard *s, void *const *d_pcm, int64_t pcm_stream_stride_bytes);
/* The job's one exchange: every device's PCM regions (pcm_stream_stride_bytes per stream) -> d_dst on device
 * `root_index`, stream s of the job at d_dst + s * dst_stream_stride_bytes (the two strides must be equal).  ncclSend /
 * ncclRecv in one group on the gather streams, behind the last render: it overlaps the next iamf_hip_shard_render, which
 * in turn waits for it before overwriting the buffers it reads.  iamf_hip_shard_sync waits for everything. */
int iamf_hip_shard_gather(iamf_hip_shard *s, int root_index, void *d_dst, int64_t dst_stream_stride_bytes,
                          void *const *d_pcm, int64_t pcm_stream_stride_bytes);
/* The same exchange for the ROWS only: bytes_per_stream bytes of every stream's region (what the last render or flush
 * emitted: sample-frames x channels x bytes per sample) instead of the whole region with its padding — a flush moves 240
 * sample-frames per stream, not a call's region.  The strides may differ (each >= bytes_per_stream): rows that are not
 * back to back are packed / spread through staging buffers of the shard on the gather streams. */
int iamf_hip_shard_gather_rows(iamf_hip_shard *s, int root_index, void *d_dst, int64_t dst_stream_stride_bytes,
                               void *const *d_pcm, int64_t pcm_stream_stride_bytes, int64_t bytes_per_stream);
int iamf_hip_shard_sync(iamf_hip_shard *s);
/* What the gather cost device `index` (any pointer may be NULL): bytes it sent in the last gather / in all gathers, bytes it
 * received in the last one (the root: all devices' rows), milliseconds its gather stream spent on its share (pack, send /
 * receive, spread) in the last gather / in all.  Waits for that device's last gather.  SURVEY 8(e): the root's inbound
 * links bound the exchange — this is where a caller reads what each peer put on the wire. */
int iamf_hip_shard_times(iamf_hip_shard *s, int index, int64_t *last_sent_bytes, int64_t *total_sent_bytes,
                         int64_t *last_received_bytes, double *last_gather_ms, double *total_gather_ms);
/* "major.minor.patch" of the RCCL found on this host, "" if none (static storage) */
const char *iamf_hip_shard_rccl_version(void);

/* ------------------------------------------------------------------------------------------
 * LPCM sub-stream packets -> planar f32 element PCM, on the device.
 * Replaces, for a batch of streams, the reference's LPCM decoder (src/iamf_dec/pcm/IAMF_pcm_decoder.c:64-83, 133-149:
 * sample = integer / 2^(bits-1); 16 / 24 / 32 bit; little-endian, or big-endian with the reference's own byte order for
 * 24 bit, bitstream.c:204-208) and the re-ordering from audio-layer order to the renderer's channel order behind it
 * (IAMF_decoder.c:2230-2260).  The caller uploads each stream's packets as they are in the bitstream into a raw region
 * of `raw_stream_stride` bytes per stream, at offsets of its choosing, and describes where output channel c finds its
 * samples: sample i of channel c = the `sample_bytes` bytes at  src_offset[c] + (first + i) * src_step[c]  (src_step = bytes
 * from one sample of the channel to the next: sample_bytes for a mono sub-stream, twice that for a coupled one);
 * src_offset[c] < 0 = a channel no sub-stream carries: silence.  d_first_count: on the device, per stream two int32,
 * `first_count_stride` int32 from one stream's pair to the next (2 for a packed array; raw_stream_stride / 4 for pairs
 * kept at the head of each stream's raw region, so that one upload carries both; 0: one pair for all streams): the first sample to take (a trimmed
 * start, iamf_frame_trim IAMF_decoder.c:1361-1381) and the number of samples to write (0: the stream is left alone);
 * first + count <= frame_size is the caller's to guarantee.  Output:
 * d_out[stream * out_stream_stride + c * frame_size + i], i < count.  Asynchronous on `stream`.
 * Returns IAMF_HIP_OK, IAMF_HIP_ERR_BAD_ARG (a layout that could read outside a stream's raw region, frame_size not a
 * multiple of 4, ...) or IAMF_HIP_ERR_DEVICE.
 * ---------------------------------------------------------------------------------------- */
#define IAMF_HIP_LPCM_MAX_CHANNELS 32
typedef struct iamf_hip_lpcm_layout {
  int32_t sample_bytes;    /* 2, 3, 4 */
  int32_t little_endian;   /* 0: big-endian (codec config sample_format_flags, IAMF_pcm_decoder.c:52-60) */
  int32_t channels;        /* rows written per stream */
  int32_t frame_size;      /* floats per row */
  int32_t src_offset[IAMF_HIP_LPCM_MAX_CHANNELS];
  int32_t src_step[IAMF_HIP_LPCM_MAX_CHANNELS];
} iamf_hip_lpcm_layout;
int iamf_hip_lpcm_unpack(const iamf_hip_lpcm_layout *layout, const void *d_raw, int64_t raw_stream_stride,
                         const int32_t *d_first_count, int64_t first_count_stride, float *d_out, int64_t out_stream_stride,
                         int32_t n_streams, void *stream);

/* Render with element 0 handed over as LPCM packets instead of planar f32: iamf_hip_lpcm_unpack and iamf_hip_batch_render_ex
 * in one call, and for the calls of the headline kernel in one KERNEL — the reference decodes a packet into its f32 decoder
 * buffer (pcm/IAMF_pcm_decoder.c:64-83) and renders from there (IAMF_decoder.c:2550-2640); on the device that f32 copy is
 * 64 of the path's 68 bytes per sample-frame, so the render kernel reads the packets' 16-bit samples itself (32 + 4 bytes)
 * and converts them where it loads them.  d_raw: [n_streams][n_frames] packet rows, frame f of stream s at
 * d_raw + s * raw_stream_stride + f * raw_frame_stride (bytes), described by `layout` exactly as for iamf_hip_lpcm_unpack
 * (offsets relative to the frame's row; layout.channels = the element's channels, layout.frame_size = the batch's).
 * first_sample: with args->n_frames == 1 and args->n_samples > 0, the frame position of the first sample to render (a
 * trimmed start); else 0.  `args` as for iamf_hip_batch_render_ex with d_in == NULL (the in_* strides are not used).
 * Fused when: little-endian, every channel present and a contiguous run, d_raw 16-byte aligned, and
 *   16 bit: src_step == 2, src_offset + 2 * first_sample a multiple of 8 bytes, both strides multiples of 8;
 *   24 bit: src_step == 3, src_offset + 3 * first_sample a multiple of 4 bytes, both strides multiples of 4 (a lane's four
 *           samples are one 12-byte load, which wants dword alignment; 48 + 4 bytes per sample-frame of a 3rd-order
 *           element instead of the 180 of unpack + f32 kernel);
 * and the batch is a plain matrix render of a 1 / 4 / 9 / 16-channel element into one or two channels with the limiter on
 * (no second element, ramps, demixer, down-mixer, de-mapping, FIR or LFE generator; no weight outside 2^-100 .. 2^100).
 * Also fused, 16 bit only: the coupled form of a channel-based element of 2 / 6 / 8 / 10 / 12 channels in playback order
 * (L R [C LFE, then pairs]) under the same batch conditions.  Channels (0,1) and, from six channels on, (4,5) ..
 * (channels-2, channels-1) are coupled sub-streams — src_step == 4 on both, the second's src_offset 2 bytes behind the
 * first's, the first's src_offset + 4 * first_sample a multiple of 8 bytes (a lane's four sample pairs are one 16-byte
 * load) — and channels 2 and 3 mono runs by the 16-bit rule above; strides multiples of 8.  2 * channels + 4 bytes per
 * sample-frame into s16 stereo instead of the 10 * channels + 4 of unpack + f32 kernel.
 * Every other input — 32 bit, big-endian, any other pairing of coupled sub-streams (24-bit pairs included), wide layouts,
 * runs off the grid — takes iamf_hip_lpcm_unpack into a buffer of the batch and then the f32 kernels.  The PCM and the
 * stream state are the same bit for bit either way (tests/test_gpu_lpcm.py, test_gpu_lpcm24.py, test_gpu_lpcm_coupled.py),
 * so fused, unfused and f32 calls may follow one another on a batch; IAMF_HIP_LPCM_UNFUSED=1 in the environment forces the second way.
 * Returns what iamf_hip_batch_render_ex returns. */
typedef struct iamf_hip_lpcm_input {
  const void *d_raw;
  int64_t raw_stream_stride, raw_frame_stride;   /* bytes */
  int32_t first_sample;
  iamf_hip_lpcm_layout layout;
} iamf_hip_lpcm_input;
int iamf_hip_batch_render_lpcm(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *args);
/* ... for the streams [stream0, stream0 + n_streams) of the batch only, as iamf_hip_batch_render_range */
int iamf_hip_batch_render_lpcm_range(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *args,
                                     int32_t stream0, int32_t n_streams);

/* BOTH elements of a two-element mix handed over as LPCM packets: a bed plus a small second element (dialogue, commentary),
 * the one multi-element shape of the base profile (the reference allows two elements per mix presentation).  For a batch
 * with a second element (iamf_hip_batch_set_second_element) the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_lpcm_unpack of in[0] and of in[1] into planar f32, then iamf_hip_batch_render_range with d_in / d_in2 on them
 * would: PCM, the sample-frames emitted and the persisted stream state are the same bit for bit, for every packet layout
 * iamf_hip_lpcm_unpack accepts, every output layout and PCM format, and every combination of ramps — so this call, the
 * single-element packet call and the f32 calls may follow one another on a batch.
 *   in[0], in[1]  element 0 and element 1, each with its own buffer, strides and layout as for iamf_hip_batch_render_lpcm
 *                 (in[1].layout.channels = the second element's channels); both first_sample must be equal.
 *   args          as for iamf_hip_batch_render_lpcm; d_in AND d_in2 must be NULL (the in_* / in2_* strides are not used).
 * One KERNEL when: the batch conditions of iamf_hip_batch_render_lpcm hold except that the second element and ramps are
 * welcome (ramps 16-byte aligned, ramp_stream_stride a multiple of 4); no fixed PCM channel stride; element 0 has the 16-bit
 * form that call fuses (mono-coded runs of 1 / 4 / 9 / 16 channels, or the coupled form of 2 / 6 / 8 / 10 / 12); element 1 is
 * 16-bit little-endian on the same grid (d_raw 16-byte aligned, strides multiples of 8) and is either mono-coded runs of 1 or
 * 4 channels or ONE coupled stereo pair; and no weight of either matrix lies outside 2^-100 .. 2^100.  Then the render kernel
 * reads both elements' packets itself: 2 * (channels + channels2) + 4 bytes per sample-frame into s16 stereo instead of the
 * 10 * (channels + channels2) + 4 of two unpack passes and the f32 mixing kernel.  Every other input — 24-bit or big-endian
 * packets on either side, a stereo second element coded as two mono runs, wide layouts, limiter off, ... — is unpacked into
 * two buffers of the batch and takes the f32 kernels; IAMF_HIP_LPCM_UNFUSED=1 forces that.
 * Returns the sample-frames emitted per stream, as iamf_hip_batch_render_lpcm_range.  IAMF_HIP_ERR_BAD_ARG, before anything
 * is queued, allocated or changed: a batch without a second element, non-NULL args.d_in or args.d_in2, a NULL d_raw in
 * either input, different first_sample in the two inputs, a bad range; and, with its own code, whatever
 * iamf_hip_batch_render_range refuses. */
typedef struct {
  iamf_hip_lpcm_input in[2];
  iamf_hip_render_args args;
} iamf_hip_lpcm_mix_call;
int iamf_hip_batch_render_lpcm_mix(iamf_hip_batch *b, const iamf_hip_lpcm_mix_call *call, int32_t stream0, int32_t n_streams);

/* Ordinary interleaved f32 PCM of ANY call length: the limiter stage behind a rate converter (iamf_hip_resampler_process
 * hands out 1114 or 1115 sample-frames for 1024 at 44.1 -> 48 kHz), or any caller that holds interleaved float PCM.  On a
 * batch created with frame_size == 1 the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_range(b, &call->args, stream0, n_streams)
 * does, bit for bit, persisted stream state included — so calls of either entry, flushes, restarts, exports and imports may
 * follow one another on one batch.
 *   args      as for iamf_hip_batch_render_range with frame_size == 1: d_in is [stream][sample-frame][channel] f32,
 *             in_frame_stride the floats from one sample-frame to the next, n_frames the sample-frames of the call (any
 *             number >= 1; 0 does nothing).
 *   reserved  0.
 * One pass of the FOUR-samples-per-lane kernel (IAMF_HIP_ROUTE_FAST_INTERLEAVED) when: limiter on; one or two input channels
 * into one or two output channels; no second element, ramps, down-mixer, demixer, projection, HRTF stage, LFE generator,
 * reduced out_gain_channels or fixed PCM channel stride; dense sample-frames (in_frame_stride == channels); d_in 16-byte
 * aligned and in_stream_stride a multiple of 4 floats; d_pcm and pcm_stream_stride_bytes multiples of 16; the streams'
 * position a multiple of 16 or at least 240; the call shorter than 2^29 / channels sample-frames.  Every other call takes
 * exactly the path of iamf_hip_batch_render_range (the one-sample-per-lane kernel); IAMF_HIP_INTERLEAVED_UNFUSED=1 forces that.
 * Returns the sample-frames emitted per stream.  IAMF_HIP_ERR_BAD_ARG, before anything is queued, allocated or changed: a NULL
 * batch or call, non-zero reserved, a batch whose frame_size is not 1; and, with its own code, whatever
 * iamf_hip_batch_render_range refuses. */
typedef struct {
  iamf_hip_render_args args;
  int32_t reserved[4];
} iamf_hip_interleaved_call;
int iamf_hip_batch_render_interleaved(iamf_hip_batch *b, const iamf_hip_interleaved_call *call, int32_t stream0, int32_t n_streams);

/* Planar f32 PCM of ANY call length: a live service that renders one frame of 1000, 480 or 120 samples per call, or the
 * first or last frame of a stream, which arrives trimmed (n_frames == 1, n_samples set).  On any batch the call leaves the
 * batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_range(b, &call->args, stream0, n_streams)
 * does, bit for bit, persisted stream state included — so calls of either entry, flushes, restarts, gain changes, exports and
 * imports may follow one another on one batch.
 *   args      as for iamf_hip_batch_render_range.
 *   reserved  0.
 * One pass of the FOUR-samples-per-lane kernel (IAMF_HIP_ROUTE_FAST_RAGGED) when the call's samples per stream (n_frames *
 * frame_size, or n_samples) are at least 1 and NO multiple of 64, and: limiter on; an element of 1, 2, 4, 6, 8, 9, 10, 12 or 16
 * channels into one or two output channels; no second element, ramps, down-mixer, demixer, projection, pre-matrix, HRTF
 * stage, LFE generator, reduced out_gain_channels or fixed PCM channel stride; frame_size a multiple of 4; d_in 16-byte
 * aligned, in_stream_stride and in_frame_stride multiples of 4 floats; d_pcm and pcm_stream_stride_bytes multiples of 16; the
 * streams' position a multiple of 16 or at least 240; (n_frames + 2) * in_frame_stride * 4 + 100 * frame_size below 2^31.
 * The kernel loads whole quads of four floats: for a frame trimmed to n_samples it loads up to 3 floats BEHIND n_samples in
 * every channel's row, which must therefore be readable — every channel row of a frame is frame_size floats from d_in on, as
 * the layout of iamf_hip_render_args has it, trimmed or not.  It reads no float outside those rows [0, frame_size) of the
 * call's frames, and what lies behind n_samples — NaN and Inf included — changes nothing.  Every other call, a call of whole 64-sample blocks included,
 * takes exactly the path of iamf_hip_batch_render_range; IAMF_HIP_RAGGED_UNFUSED=1 forces that.
 * Returns the sample-frames emitted per stream.  IAMF_HIP_ERR_BAD_ARG, before anything is queued, allocated or changed: a NULL
 * batch or call, non-zero reserved; and, with its own code, whatever iamf_hip_batch_render_range refuses. */
typedef struct {
  iamf_hip_render_args args;
  int32_t reserved[4];
} iamf_hip_ragged_call;
int iamf_hip_batch_render_ragged(iamf_hip_batch *b, const iamf_hip_ragged_call *call, int32_t stream0, int32_t n_streams);

/* Element 0 as LPCM packets, every packet form the fused kernels read: what iamf_hip_batch_render_lpcm_range takes and, beyond
 * it, 24-bit packets of a channel-based element whose channel pairs are coupled sub-streams.  On any batch and any packet
 * layout the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_lpcm_range(b, &call->in, &call->args, stream0, n_streams)
 * does, bit for bit, persisted stream state included — so calls of either entry, flushes, restarts, exports and imports may
 * follow one another on one batch.
 *   in        as for iamf_hip_batch_render_lpcm.
 *   args      as for iamf_hip_batch_render_lpcm: d_in and d_in2 NULL.
 *   reserved  0.
 * One pass of the headline kernel over the packets as they lie (IAMF_HIP_ROUTE_LPCM24_COUPLED, 3 * channels + 4 instead of
 * 11 * channels + 4 bytes per sample-frame into s16 stereo) when the packets have the coupled 24-bit form: little-endian
 * 24-bit samples of 2, 6, 8, 10 or 12 channels in playback order, every channel present; channels (0,1) and, from six
 * channels on, (4,5) .. (n-2, n-1) each ONE run of interleaved samples (src_step 6, the partner's src_offset 3 bytes behind the
 * first's), channels 2 and 3 (C, LFE) contiguous runs (src_step 3); d_raw 16-byte aligned, both strides multiples of 4; a
 * pair's src_offset + 6 * first_sample and a mono run's src_offset + 3 * first_sample multiples of 4 — and the call is one
 * the fused 16-bit coupled form would take: one or two output channels, limiter on, whole 64-sample blocks, no second
 * element, ramps, down-mixer, demixer, projection, pre-matrix, HRTF stage or LFE generator, the streams' position a multiple
 * of 16 or at least 240, (n_frames + 2) * raw_frame_stride + 2^24 below 2^31.  Every other call takes exactly the path of
 * iamf_hip_batch_render_lpcm_range, its fused forms included; IAMF_HIP_LPCM_UNFUSED=1 forces the unpacker and the f32
 * kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  IAMF_HIP_ERR_BAD_ARG, before anything is queued, allocated or changed: a NULL
 * batch or call, non-zero reserved, a non-NULL d_in or d_in2; and, with its own code, whatever
 * iamf_hip_batch_render_lpcm_range refuses. */
typedef struct {
  iamf_hip_lpcm_input in;
  iamf_hip_render_args args;   /* d_in, d_in2 NULL */
  int32_t reserved[4];         /* 0 */
} iamf_hip_packet_call;
int iamf_hip_batch_render_packets(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams);

/* Element 0 as LPCM packets of ANY call length: an LPCM stream whose frames hold 1000, 480, 240 or 120 samples, rendered frame
 * by frame, or the first or last frame of any stream, which arrives trimmed (n_frames == 1, n_samples set, first_sample).  On
 * any batch, any packet layout and any length the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_packets(b, call, stream0, n_streams)
 * does, bit for bit, persisted stream state included — so calls of every entry, flushes, restarts, gain changes, exports and
 * imports may follow one another on one batch.
 *   call      as for iamf_hip_batch_render_packets.
 * One pass of the FOUR-samples-per-lane kernel over the packets as they lie (IAMF_HIP_ROUTE_PACKETS_RAGGED) when the call's
 * samples per stream (n_frames * frame_size, or n_samples) are at least 1 and NO multiple of 64, and:
 *   - the packets have one of the four forms the fused whole-block kernels read, little-endian, every channel present, d_raw
 *     16-byte aligned: 16-bit mono-coded (1, 4, 9 or 16 contiguous runs, src_step 2; both strides and every src_offset + 2 *
 *     first_sample multiples of 8), 16-bit coupled (2, 6, 8, 10 or 12 channels in playback order, pairs (0,1), (4,5) ..
 *     interleaved with src_step 4 and the partner 2 bytes behind, C and LFE runs of src_step 2; strides, a pair's src_offset +
 *     4 * first_sample and a run's src_offset + 2 * first_sample multiples of 8), 24-bit mono-coded (src_step 3; strides and
 *     src_offset + 3 * first_sample multiples of 4) or 24-bit coupled (src_step 6 / 3, the partner 3 bytes behind; strides, a
 *     pair's src_offset + 6 * first_sample and a run's src_offset + 3 * first_sample multiples of 4);
 *   - limiter on; one or two output channels; no second element, ramps, down-mixer, demixer, projection, pre-matrix, HRTF
 *     stage, LFE generator, reduced out_gain_channels or fixed PCM channel stride; matrix weights that take the packets'
 *     scale (as the whole-block forms); frame_size a multiple of 4; d_pcm and pcm_stream_stride_bytes multiples of 16; the
 *     streams' position a multiple of 16 or at least 240; (n_frames + 2) * raw_frame_stride + 2^24 below 2^31;
 *   - for a frame trimmed to n_samples: first_sample + ((n_samples + 3) & ~3) <= frame_size.
 * The kernel loads whole quads of four samples: for a frame trimmed to n_samples it reads up to 3 packet samples BEHIND
 * n_samples in every run, which must therefore be readable — a frame's runs hold frame_size samples each from src_offset on,
 * whether the frame is trimmed or not, as iamf_hip_lpcm_layout has it.  It reads no byte outside those runs of the call's
 * frames, and what lies behind n_samples or between the runs changes nothing.  Every other call, a call of whole 64-sample
 * blocks included, takes exactly the path of iamf_hip_batch_render_packets, that entry's fused whole-block forms included;
 * IAMF_HIP_PACKETS_RAGGED_UNFUSED=1 forces that, and IAMF_HIP_LPCM_UNFUSED=1 the unpacker and the f32 kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  Refusals are those of iamf_hip_batch_render_packets, with their codes,
 * before anything is queued, allocated or changed. */
int iamf_hip_batch_render_packets_ragged(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams);

/* BOTH elements of a two-element mix as LPCM packets, every packet form the fused kernels read: what
 * iamf_hip_batch_render_lpcm_mix takes and, beyond it, 24-bit packets on both elements.  On any batch with a second element
 * and any packet layouts the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_lpcm_mix on {call->in[0], call->in[1], call->args}, stream0, n_streams
 * does, bit for bit, persisted stream state included — so calls of either entry, the single-element packet calls, the f32
 * calls, flushes, restarts, exports and imports may follow one another on one batch.
 *   in[0], in[1]  as for iamf_hip_batch_render_lpcm_mix; both first_sample must be equal.
 *   args          as for iamf_hip_batch_render_lpcm_mix: d_in and d_in2 NULL.
 *   reserved      0.
 * One pass of the headline kernel over both elements' packets as they lie (IAMF_HIP_ROUTE_LPCM24_MIX, 3 * (channels +
 * channels2) + 4 instead of 11 * (channels + channels2) + 4 bytes per sample-frame into s16 stereo) when both elements hold
 * little-endian 24-bit samples: element 0 mono-coded runs of 1 / 4 / 9 / 16 channels (the 24-bit form of
 * iamf_hip_batch_render_lpcm) or the coupled form of 2 / 6 / 8 / 10 / 12 (iamf_hip_batch_render_packets); element 1 with
 * d_raw 16-byte aligned and both strides multiples of 4, either mono-coded runs of 1 or 4 channels (src_step 3, src_offset +
 * 3 * first_sample a multiple of 4) or ONE coupled stereo pair (src_step 6, the partner's src_offset 3 bytes behind the
 * first's, src_offset + 6 * first_sample a multiple of 4) — and the call is one the fused 16-bit mix would take: one or two
 * output channels, limiter on, whole 64-sample blocks, no fixed PCM channel stride, ramps 16-byte aligned with
 * ramp_stream_stride a multiple of 4, no down-mixer, demixer, projection, pre-matrix, HRTF stage or LFE generator, no weight
 * of either matrix outside 2^-100 .. 2^100, the streams' position a multiple of 16 or at least 240, (n_frames + 2) *
 * raw_frame_stride + 2^24 below 2^31 for both elements.  Every other call — 16 bits on one element and 24 on the other,
 * big-endian or 32-bit samples, a stereo second element coded as two mono runs, a trimmed start off a form's grid, ... —
 * takes exactly the path of iamf_hip_batch_render_lpcm_mix, its fused 16-bit form included; IAMF_HIP_LPCM_UNFUSED=1 forces
 * the two unpacks and the f32 kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  IAMF_HIP_ERR_BAD_ARG, before anything is queued, allocated or changed: a NULL
 * batch or call, non-zero reserved, a non-NULL d_in or d_in2; and, with its own code, whatever
 * iamf_hip_batch_render_lpcm_mix refuses. */
typedef struct {
  iamf_hip_lpcm_input in[2];
  iamf_hip_render_args args;   /* d_in, d_in2 NULL */
  int32_t reserved[4];         /* 0 */
} iamf_hip_packet_mix_call;
int iamf_hip_batch_render_packets_mix(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams);

/* BOTH elements of a two-element mix as LPCM packets, a call of ANY length: a mix whose frames hold 1000, 480, 240 or 120
 * samples, rendered frame by frame, or the first or last frame of any stream, which arrives trimmed (n_frames == 1, n_samples
 * set, first_sample).  On any batch, any pair of packet layouts and any length the call leaves the batch, d_pcm and its
 * return value exactly as
 *   iamf_hip_batch_render_packets_mix(b, call, stream0, n_streams)
 * does, bit for bit, persisted stream state included — so calls of every entry, flushes, restarts, gain changes, exports and
 * imports may follow one another on one batch.
 *   call      as for iamf_hip_batch_render_packets_mix.
 * One pass of the FOUR-samples-per-lane kernel over both elements' packets as they lie (IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED) when
 * the call's samples per stream (n_frames * frame_size, or n_samples) are at least 1 and NO multiple of 64, and:
 *   - both elements hold little-endian samples of one size, 16 or 24 bit, every channel present, each d_raw 16-byte aligned, each
 *     in a form the whole-block mix kernels read (iamf_hip_batch_render_lpcm_mix, iamf_hip_batch_render_packets_mix): element 0
 *     mono-coded runs of 1 / 4 / 9 / 16 channels or the coupled form of 2 / 6 / 8 / 10 / 12; element 1 mono-coded runs of 1 or
 *     4 channels or ONE coupled stereo pair; strides and every run's src_offset + src_step * first_sample multiples of 8 (16
 *     bit) or 4 (24 bit);
 *   - limiter on; one or two output channels; no down-mixer, demixer, projection, pre-matrix, HRTF stage, LFE generator,
 *     reduced out_gain_channels or fixed PCM channel stride; matrix weights of both elements that take the packets' scale (as
 *     the whole-block forms); frame_size a multiple of 4; d_pcm and pcm_stream_stride_bytes multiples of 16; the streams'
 *     position a multiple of 16 or at least 240; (n_frames + 2) * raw_frame_stride + 2^24 below 2^31 for both elements;
 *   - ramps (d_element_ramp, d_element2_ramp, d_output_ramp), where given, 16-byte aligned with ramp_stream_stride a
 *     multiple of 4: they are fused as in the whole-block forms;
 *   - for a frame trimmed to n_samples: first_sample + ((n_samples + 3) & ~3) <= frame_size.
 * The kernel loads whole quads of four samples: for a frame trimmed to n_samples it reads up to 3 packet samples BEHIND
 * n_samples in every run of BOTH elements, which must therefore be readable — a frame's runs hold frame_size samples each
 * from src_offset on, whether the frame is trimmed or not, as iamf_hip_lpcm_layout has it.  It reads no byte outside those
 * runs of the call's frames, and what lies behind n_samples or between the runs changes nothing.  It reads NO ramp float
 * behind the call's last sample: a ramp row need hold the call's samples per stream and not one float more, as for every
 * other entry.  Every other call, a call of whole 64-sample blocks included, takes exactly the path of
 * iamf_hip_batch_render_packets_mix, that entry's fused whole-block forms included; IAMF_HIP_PACKETS_MIX_RAGGED_UNFUSED=1
 * forces that, and IAMF_HIP_LPCM_UNFUSED=1 the unpacker and the f32 kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  Refusals are those of iamf_hip_batch_render_packets_mix, with their codes,
 * before anything is queued, allocated or changed. */
int iamf_hip_batch_render_packets_mix_ragged(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0,
                                             int32_t n_streams);

/* Element 0 as LPCM packets on a batch WITHOUT the peak limiter: the first stage of a rate-converting stream (render ->
 * resampler -> limiter) and the whole render of a stream whose limiter is switched off.  On any batch, any packet layout and
 * any length the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_packets_ragged(b, call, stream0, n_streams)
 * does, bit for bit, the stream position included.
 *   call      as for iamf_hip_batch_render_packets.
 * One pass of the four-samples-per-lane limiter-less kernel over the packets as they lie (IAMF_HIP_ROUTE_NOLIM_PACKETS), with no
 * f32 copy of the element, when:
 *   - the batch has the limiter off and one matrix-rendered element: no second element, ramps, down-mixer, demixer, projection,
 *     pre-matrix, HRTF stage, LFE generator, reduced out_gain_channels or fixed PCM channel stride;
 *   - the packets have one of the four forms iamf_hip_batch_render_packets_ragged lists (16- or 24-bit little-endian, mono-coded
 *     1, 4, 9 or 16 runs or the coupled 2, 6, 8, 10 or 12 channels, on the form's grid with first_sample counted in);
 *   - frame_size and the call's samples per stream (n_frames * frame_size, or n_samples) are multiples of 4 and at least 4;
 *     for a frame trimmed to n_samples, first_sample + n_samples <= frame_size (which every accepted call has);
 *   - d_pcm and pcm_stream_stride_bytes are multiples of 16; out_channels * bytes per PCM sample is a multiple of 4 and at
 *     most 60 (any of the four PCM formats, up to 15 channels of f32).
 * The kernel reads no byte outside the samples of the call.  The weights need no rule: the samples are converted to f32 as
 * iamf_hip_lpcm_unpack converts them and every product is the f32 path's.  Every other call — a limiter-on batch included —
 * takes exactly the path of iamf_hip_batch_render_packets_ragged; IAMF_HIP_NOLIM_PACKETS_UNFUSED=1 forces that, and
 * IAMF_HIP_LPCM_UNFUSED=1 the unpacker and the f32 kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  Refusals are those of iamf_hip_batch_render_packets_ragged, with their
 * codes, before anything is queued, allocated or changed. */
int iamf_hip_batch_render_packets_nolim(iamf_hip_batch *b, const iamf_hip_packet_call *call, int32_t stream0, int32_t n_streams);

/* Both elements of a mix as LPCM packets on a batch WITHOUT the peak limiter: a bed plus dialogue or commentary as the first
 * stage of a rate-converting stream, or as the whole render of a stream whose limiter is switched off.  On any batch, any pair
 * of packet layouts and any length the call leaves the batch, d_pcm and its return value exactly as
 *   iamf_hip_batch_render_packets_mix_ragged(b, call, stream0, n_streams)
 * does, bit for bit, the stream position included.
 *   call      as for iamf_hip_batch_render_packets_mix.
 * One pass of the four-samples-per-lane limiter-less kernel over both elements' packets as they lie
 * (IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX), with no f32 copy of either element, when:
 *   - the batch has the limiter off and a second element, and no down-mixer, demixer, projection, pre-matrix, HRTF stage, LFE
 *     generator, reduced out_gain_channels or fixed PCM channel stride;
 *   - both elements hold little-endian samples of one size, 16 or 24 bit: element 0 in one of the four forms
 *     iamf_hip_batch_render_packets_nolim lists, element 1 as 1 or 4 mono-coded runs or as ONE coupled stereo pair, each on its
 *     form's grid (8 bytes for 16-bit samples, 4 for 24-bit ones) with first_sample counted in, in[1].d_raw a multiple of 16;
 *   - d_element_ramp, d_element2_ramp and d_output_ramp, where given, are multiples of 16 and ramp_stream_stride is a
 *     multiple of 4 (any of the three, or none);
 *   - frame_size and the call's samples per stream (n_frames * frame_size, or n_samples) are multiples of 4 and at least 4;
 *     for a frame trimmed to n_samples, first_sample + n_samples <= frame_size (which every accepted call has);
 *   - d_pcm and pcm_stream_stride_bytes are multiples of 16; out_channels * bytes per PCM sample is a multiple of 4 and at
 *     most 60 (any of the four PCM formats, up to 15 channels of f32).
 * The kernel reads no byte outside the samples of the call, and no float of a ramp behind the call's last sample.  The weights
 * need no rule: the samples are converted to f32 as iamf_hip_lpcm_unpack converts them and every product is the f32 path's.
 * Every other call — a limiter-on batch, 16-bit packets beside 24-bit ones, big-endian samples, a stereo second element held
 * as two mono runs, a trim that is no multiple of 4 — takes exactly the path of iamf_hip_batch_render_packets_mix_ragged;
 * IAMF_HIP_NOLIM_PACKETS_MIX_UNFUSED=1 forces that, and IAMF_HIP_LPCM_UNFUSED=1 the unpacker and the f32 kernels, as everywhere.
 * Returns the sample-frames emitted per stream.  Refusals are those of iamf_hip_batch_render_packets_mix_ragged, with their
 * codes, before anything is queued, allocated or changed. */
int iamf_hip_batch_render_packets_mix_nolim(iamf_hip_batch *b, const iamf_hip_packet_mix_call *call, int32_t stream0, int32_t n_streams);

/* One element, held as LPCM packets, rendered into several batches with ONE pass over the packets where that is possible:
 * iamf_hip_batch_render_fanout for the input form of iamf_hip_batch_render_lpcm, over a range of streams.
 *
 * Meaning: for every j the call leaves batches[j] and d_pcm[j] exactly as
 *   n_emitted[j] = iamf_hip_batch_render_lpcm_range(batches[j], in, &args_j, stream0, n_streams)
 * with args_j = {n_frames, n_samples, d_pcm[j], pcm_stream_stride_bytes[j], stream} would, called for j = 0 .. in turn: bit
 * for bit, for every packet form (16 / 24 / 32 bit, either byte order, coupled sub-streams), every PCM format, gains,
 * threshold, limiter on or off.  in->first_sample and n_samples follow the single call's rules.  This call, the f32
 * fan-out and the single-batch calls may be mixed freely on the same batches.
 *
 * What runs is decided from what the call can observe, in this order:
 *   1. A member is packet-fusable when the packets have the 16-bit form the single call fuses (see above; the single
 *      call's 24-bit form and its coupled 16-bit form are not ones this entry fuses: such packets go by 3.), the member's single
 *      call would run the packet-fed kernel, the element has 4, 9 or 16 channels, and the member is one the f32 fan-out
 *      would fuse (no fixed PCM channel stride).  If at least two members are packet-fusable they share one launch that
 *      reads the packets once: 2 * M + sum of the members' output bytes per sample-frame instead of 2 * M per member.
 *   2. A remaining member whose single call runs the packet-fed kernel gets that call.
 *   3. All other members need f32: the range's packets are unpacked ONCE (iamf_hip_lpcm_unpack), into the buffer of the
 *      first such member, and those members go through iamf_hip_batch_render_fanout_range on it — so 24-bit packets and
 *      coupled 5.1 / 7.1 / 7.1.4 elements get the f32 fan-out's saving and one unpack pass instead of one per member.
 * *report (may be NULL) says what ran.
 *
 * Errors: those of iamf_hip_batch_render_fanout_range plus those of iamf_hip_batch_render_lpcm_range.  Every argument and
 * state check runs before the first launch; a refused call changes no member and writes neither n_emitted nor *report.
 * The count, NULL and n_streams <= 0 checks need no device.
 * (24-bit packets and coupled 5.1 / 7.1 / 7.1.4 elements are read once by iamf_hip_batch_render_fanout_packets, below.) */
typedef struct iamf_hip_fanout_report {
  int32_t n_fused;      /* members the shared launch rendered: 0 or 2..IAMF_HIP_FANOUT_MAX (the packet launch's where both
                           a packet launch and an f32 launch ran) */
  int32_t input_fused;  /* 1: that launch read the packets itself; 0: it read f32 (or there was none) */
  int32_t n_unpacks;    /* passes of iamf_hip_lpcm_unpack over the range's packets queued by this call: 0 or 1 */
  int32_t reserved;
} iamf_hip_fanout_report;
int iamf_hip_batch_render_fanout_lpcm(iamf_hip_batch *const *batches, int32_t n_batches, const iamf_hip_lpcm_input *in,
                                      int32_t n_frames, int32_t n_samples, void *const *d_pcm,
                                      const int64_t *pcm_stream_stride_bytes, void *stream, int32_t stream0, int32_t n_streams,
                                      int32_t *n_emitted /* host, [n_batches] */, iamf_hip_fanout_report *report /* may be NULL */);

/* The same for every packet form a fused kernel reads: iamf_hip_batch_render_fanout for the input form of
 * iamf_hip_batch_render_packets.  It takes that entry's call block, as every packet entry since does — the packets in call->in,
 * and of call->args n_frames, n_samples and stream; every other field of call->args is NULL / 0 (the members' PCM buffers travel
 * beside the block, one per member), as are the reserved words — and otherwise the parameters of
 * iamf_hip_batch_render_fanout_lpcm.
 *
 * Meaning: for every j the call leaves batches[j], d_pcm[j] and n_emitted[j] exactly as
 *   iamf_hip_batch_render_packets(batches[j], &call_j, stream0, n_streams)
 * with call_j = *call but args.d_pcm = d_pcm[j], args.pcm_stream_stride_bytes = pcm_stream_stride_bytes[j] would, called for j = 0 .. in turn:
 * bit for bit, PCM and persisted stream state.  The entry is total — it takes every call the entry above takes — and may be
 * mixed freely with it, the f32 fan-out and the single-batch calls on the same batches.
 *
 * What runs is decided from what the call can observe, in this order:
 *   1. Where the packets have the 24-bit mono-coded, the coupled 16-bit or the coupled 24-bit form (little-endian; what
 *      iamf_hip_batch_render_packets fuses), a member is packet-fusable when its single call would run that form's packet-fed
 *      kernel (IAMF_HIP_ROUTE_LPCM24 / _LPCM_COUPLED / _LPCM24_COUPLED), nothing is re-laid behind the kernel (no fixed PCM
 *      channel stride) and the element has 4, 9 or 16 channels (24-bit mono-coded) or 6, 8, 10 or 12 (coupled).  Two or more such
 *      members share one launch (IAMF_HIP_ROUTE_FANOUT_PACKETS) that reads the packets once: 3 * M (2 * M) + sum of the
 *      members' output bytes per sample-frame instead of 3 * M (2 * M) per member.  *report: input_fused = 1.  How many share
 *      it at a given number of streams follows a measured rule (a size at which the launch does not beat the
 *      single calls is not fused); the members left over go by 2.
 *   2. A remaining member whose single call runs a packet-fed kernel gets that call.
 *   3. Every other member takes the path of iamf_hip_batch_render_fanout_lpcm: one unpack pass and the f32 fan-out.
 *   4. A call whose packets have the 16-bit mono-coded form or none a kernel reads (big-endian, 32 bit, a loudspeaker layout as
 *      mono sub-streams, runs off the grid, a call that is not whole 64-sample blocks) is iamf_hip_batch_render_fanout_lpcm's,
 *      whole: its routes, its report.
 * Not fused (out of scope): stereo elements, members of more than two output channels, calls that are not whole 64-sample
 * blocks.  IAMF_HIP_FANOUT_PACKETS_UNFUSED=1 forces the path of iamf_hip_batch_render_fanout_lpcm for every call, and
 * IAMF_HIP_LPCM_UNFUSED=1 the unpacker and the f32 kernels, as everywhere.
 *
 * Errors, the order of the checks and *report: as iamf_hip_batch_render_fanout_lpcm, a NULL call block, a non-zero reserved word
 * or a field of call->args other than the three named answering IAMF_HIP_ERR_BAD_ARG behind the member count.  Every check runs
 * before the first launch; a refused call changes no member and writes neither n_emitted nor *report. */
int iamf_hip_batch_render_fanout_packets(iamf_hip_batch *const *batches, int32_t n_batches, const iamf_hip_packet_call *call,
                                         void *const *d_pcm, const int64_t *pcm_stream_stride_bytes, int32_t stream0, int32_t n_streams,
                                         int32_t *n_emitted /* host, [n_batches] */, iamf_hip_fanout_report *report /* may be NULL */);

/* Host -> device by a kernel that reads pinned host memory (hipHostMalloc) over PCIe, 16 bytes per lane: the bytes of a
 * hipMemcpyAsync without leaving the compute queue, for callers that put a small upload between kernels (a pinned
 * hipMemcpyAsync costs ~9 us per call and the hand-over between copy engine and compute queue ~12 us each way on
 * MI355X; the kernel moves 8 MB as fast as the engine).  Both pointers 16-byte aligned, `bytes` a multiple of 16.
 * IAMF_HIP_OK, IAMF_HIP_ERR_BAD_ARG or IAMF_HIP_ERR_DEVICE. */
int iamf_hip_upload_by_kernel(const void *h_pinned, void *d_dst, size_t bytes, void *stream);
/* A one-lane kernel on `stream` that stores `seq` to a word of PINNED host memory behind a system-scope fence: a host
 * that has just queued a few microseconds of work and wants its result spins on the word instead of calling
 * hipStreamSynchronize (MI355X, tools/debug/sync_probe.hip: 14.8 instead of 18.1 us per launch-and-wait).  What was queued
 * before it on the stream has completed and is visible to the host when the word reads `seq`.  The caller bounds its
 * spin and falls back to hipStreamSynchronize (which also reports a device error).  IAMF_HIP_OK / _BAD_ARG / _DEVICE. */
int iamf_hip_stream_signal(void *stream, volatile uint32_t *h_pinned_flag, uint32_t seq);
/* f32 sample-frames [stream][sample][channels] — what a batch with out_format IAMF_HIP_FMT_F32 writes — to planar
 * [stream][channel][dst_channel_stride], the form a batch reads element PCM in: how one batch's rendered frame becomes
 * another batch's (second) element, e.g. a presentation both of whose elements need a per-stream stage (the reference
 * mixes rendered frames, iamf_mixer_mix, IAMF_decoder.c:2702-2733).  Strides in floats; channels <= 24.
 * IAMF_HIP_OK / _BAD_ARG / _DEVICE. */
int iamf_hip_deinterleave_f32(const float *d_src, int64_t src_stream_stride, int32_t channels, int32_t n_streams,
                              int32_t n_samples, float *d_dst, int64_t dst_stream_stride, int64_t dst_channel_stride, void *stream);

/* ------------------------------------------------------------------------------------------
 * Which kernel ran.  Every render kernel is exact and the general kernel takes what the others refuse, so results alone
 * do not show which instance a call launched.  The library lists the kernel instances it holds and counts, process-wide,
 * every launch per instance: a test resets the tally, makes its calls and reads which instances ran.
 *   family: IAMF_HIP_ROUTE_* below (stable numbers).  The other fields, per family (0 where not named):
 *     GENERIC, NOLIM       m = inputs
 *     FAST                 variant 1 = mixing (second element / ramps), m, c = output channels (1, 2)
 *     FAST_DOWN, WIDE4_DEMIX, WIDE4_DOWN   m, c = output channels
 *     WIDE                 variant 1 = MFMA projection, m
 *     WIDE4, WIDE4_MIX, WIDE4_LFE          variant 1 = MFMA projection, m, c
 *     LPCM                 variant 1 = early per-channel prefetch, 0 = late; m, c
 *     LPCM24               the same for 24-bit samples (table 2 of iamf_hip_route_table_instances only)
 *     LPCM_COUPLED         the same for the coupled 16-bit form (iamf_hip_route_family_instances only)
 *     LPCM_MIX             both elements of a mix as 16-bit packets (iamf_hip_batch_render_lpcm_mix): m, c of element 0 as LPCM /
 *                          LPCM_COUPLED, k = form of element 1 (1 mono-coded runs, 2 a coupled pair); variant 0
 *                          (iamf_hip_route_family_instances only)
 *     FAST_INTERLEAVED     interleaved f32 of any call length (iamf_hip_batch_render_interleaved): m, c; variant 0
 *                          (iamf_hip_route_family_instances only)
 *     FAST_RAGGED          planar f32 of any call length (iamf_hip_batch_render_ragged): m, c; variant 0
 *                          (iamf_hip_route_family_instances only)
 *     LPCM24_COUPLED       the coupled 24-bit form (iamf_hip_batch_render_packets): variant, m, c as LPCM
 *                          (iamf_hip_route_family_instances only)
 *     LPCM24_MIX           both elements as 24-bit packets (iamf_hip_batch_render_packets_mix): m, c, k as LPCM_MIX;
 *                          variant 0 (iamf_hip_route_family_instances only)
 *     PACKETS_RAGGED       one element as packets of any call length (iamf_hip_batch_render_packets_ragged): m (1, 4, 9, 16:
 *                          mono-coded; 2, 6, 8, 10, 12: coupled), c, k = bytes per packet sample (2, 3); variant 0
 *                          (iamf_hip_route_family_instances only)
 *     PACKETS_MIX_RAGGED   both elements as packets of any call length (iamf_hip_batch_render_packets_mix_ragged): m, c, k as
 *                          LPCM_MIX; variant = bytes per packet sample (2, 3) (iamf_hip_route_family_instances only)
 *     NOLIM_PACKETS        the limiter-less renderer over one element's packets (iamf_hip_batch_render_packets_nolim): m (1,
 *                          4, 9, 16: mono-coded; 2, 6, 8, 10, 12: coupled), k = bytes per packet sample (2, 3); variant 0,
 *                          c 0 (iamf_hip_route_family_instances only)
 *     NOLIM_PACKETS_MIX    the limiter-less renderer over both elements' packets (iamf_hip_batch_render_packets_mix_nolim): m as
 *                          NOLIM_PACKETS, variant = bytes per packet sample (2, 3), k = the second element's form (1: mono-
 *                          coded runs, 2: one coupled pair); c 0 (iamf_hip_route_family_instances only)
 *     FANOUT               m, k = members of the fused launch
 *     FANOUT_LPCM          m, k = members of the fused launch (extension table: iamf_hip_route_instances_ext)
 *     FANOUT_PACKETS       the fan-out fed with 24-bit or coupled packets (iamf_hip_batch_render_fanout_packets): m, k = members
 *                          of the fused launch; variant bit 0 = 24-bit samples, bit 1 = coupled pairs (1 / 2 / 3 = 24-bit
 *                          mono-coded / 16-bit coupled / 24-bit coupled); c 0 (iamf_hip_route_family_instances only)
 *     FIR_SPLIT            m (the FFT stage as its own kernel; the FAST <2, 2> launch behind it is counted as FAST)
 *     FIR_FUSED            variant = stage (3 FFT, 2 split-f16 MFMA, 1 f32 MFMA), m
 *     RS_PLAIN             resample_kernel
 *     RS_TILE              resample_tile_kernel, variant 1 = direct mode, 0 = interpolated
 *     RS_BLOCK             resample_block_kernel<C, R>: c = C, k = R
 *     RS_DIRECT            resample_direct_kernel<C, N, NUMP, R>: m = N, c = C, variant = NUMP, k = R
 *   A launch counts after it succeeded.  Counters are relaxed atomics: any thread may launch while another reads.
 * ---------------------------------------------------------------------------------------- */
enum {
  IAMF_HIP_ROUTE_NONE = 0,   /* tally only: launches of an instance the listing does not hold (a defect) */
  IAMF_HIP_ROUTE_GENERIC = 1,
  IAMF_HIP_ROUTE_NOLIM = 2,
  IAMF_HIP_ROUTE_FAST = 3,
  IAMF_HIP_ROUTE_FAST_DOWN = 4,
  IAMF_HIP_ROUTE_WIDE = 5,
  IAMF_HIP_ROUTE_WIDE4 = 6,
  IAMF_HIP_ROUTE_WIDE4_DEMIX = 7,
  IAMF_HIP_ROUTE_WIDE4_DOWN = 8,
  IAMF_HIP_ROUTE_WIDE4_MIX = 9,
  IAMF_HIP_ROUTE_WIDE4_LFE = 10,
  IAMF_HIP_ROUTE_LPCM = 11,
  IAMF_HIP_ROUTE_FANOUT = 12,
  IAMF_HIP_ROUTE_FIR_SPLIT = 13,
  IAMF_HIP_ROUTE_FIR_FUSED = 14,
  IAMF_HIP_ROUTE_FANOUT_LPCM = 15,   /* extension table only */
  IAMF_HIP_ROUTE_LPCM24 = 16,        /* table 2 only */
  IAMF_HIP_ROUTE_LPCM_COUPLED = 17,  /* no table: iamf_hip_route_family_instances / _family_tally */
  IAMF_HIP_ROUTE_RS_PLAIN = 20,
  IAMF_HIP_ROUTE_RS_TILE = 21,
  IAMF_HIP_ROUTE_RS_BLOCK = 22,
  IAMF_HIP_ROUTE_RS_DIRECT = 23,
  IAMF_HIP_ROUTE_LPCM_MIX = 25,      /* no table: iamf_hip_route_family_instances / _family_tally (18, 19, 24: unused) */
  IAMF_HIP_ROUTE_FAST_INTERLEAVED = 27,  /* no table either (26: unused) */
  IAMF_HIP_ROUTE_FAST_RAGGED = 29,       /* no table either (28: unused) */
  IAMF_HIP_ROUTE_LPCM24_COUPLED = 31,    /* no table either (30 stays unused) */
  IAMF_HIP_ROUTE_LPCM24_MIX = 33,        /* no table either (32 stays unused) */
  IAMF_HIP_ROUTE_PACKETS_RAGGED = 37,    /* no table either (34, 35 and 36 stay unused) */
  IAMF_HIP_ROUTE_PACKETS_MIX_RAGGED = 39, /* no table either (38 stays unused) */
  IAMF_HIP_ROUTE_NOLIM_PACKETS = 43,     /* no table either (40, 41 and 42 stay unused) */
  IAMF_HIP_ROUTE_NOLIM_PACKETS_MIX = 47, /* no table either (44, 45 and 46 stay unused) */
  IAMF_HIP_ROUTE_FANOUT_PACKETS = 51     /* no table either (48, 49 and 50 stay unused) */
};
typedef struct {
  int32_t family, variant, m, c, k;
  int32_t reserved;
  int64_t launches;   /* iamf_hip_route_instances: 0 */
} iamf_hip_route_row;
/* Every kernel instance this build holds, in a fixed order; needs no device.  Writes min(cap, count) rows (rows may be NULL
 * with cap 0) and returns the count. */
int iamf_hip_route_instances(iamf_hip_route_row *rows, int cap);
/* The instances launched since the last reset, with their counts, in the listing's order; reset != 0 zeroes the counters
 * as it reads them.  Writes min(cap, count) rows and returns the count (rows NULL, cap 0, reset 1: just reset). */
int iamf_hip_route_tally(iamf_hip_route_row *rows, int cap, int reset);
/* The extension table: kernel instances added after the listing above was pinned by its callers (FANOUT_LPCM).  The same
 * row type and the same semantics, rows and counters of its own: a launch of one of these instances shows in
 * iamf_hip_route_tally_ext only, never as a NONE row of iamf_hip_route_tally. */
int iamf_hip_route_instances_ext(iamf_hip_route_row *rows, int cap);
int iamf_hip_route_tally_ext(iamf_hip_route_row *rows, int cap, int reset);
/* The indexed form of the two pairs above, for tables added since: both listings' row sets are pinned by their callers.
 * iamf_hip_route_tables() tables; table 0 IS the base listing and table 1 the extension listing (the same rows and the
 * same counters as the symbols above, which stay); table 2: LPCM24 rows (variant, m, c as LPCM), counters of its own — a
 * launch of one of these instances shows in table 2 only, never as a NONE row of another tally.  Semantics per table as
 * above; a table number outside 0 .. tables - 1: IAMF_HIP_ERR_BAD_ARG. */
int iamf_hip_route_tables(void);
int iamf_hip_route_table_instances(int table, iamf_hip_route_row *rows, int cap);
int iamf_hip_route_table_tally(int table, iamf_hip_route_row *rows, int cap, int reset);
/* The listing by kernel family, open-ended: a family added later needs no new entry and no new table (the three tables'
 * row sets are pinned by their callers).  family: IAMF_HIP_ROUTE_*.  For a family of tables 0 .. 2 these give that family's
 * rows of its table — the SAME counters, so a reset here resets them there; for LPCM_COUPLED its rows (variant, m, c as
 * LPCM), which no table lists and whose launches show in no table's tally.  _instances: every row of the family;
 * _tally: the rows launched since their last reset (reset != 0 clears them).  Both return the number of such rows and
 * fill at most cap of them (rows may be NULL); -1 for a family no instance belongs to.  No GPU needed.  LPCM_MIX is listed
 * the same way: rows and counters of its own, in no table; so are FAST_INTERLEAVED, FAST_RAGGED, LPCM24_COUPLED,
 * LPCM24_MIX, PACKETS_RAGGED, PACKETS_MIX_RAGGED, NOLIM_PACKETS, NOLIM_PACKETS_MIX and FANOUT_PACKETS. */
int iamf_hip_route_family_instances(int family, iamf_hip_route_row *rows, int cap);
int iamf_hip_route_family_tally(int family, iamf_hip_route_row *rows, int cap, int reset);

/* ------------------------------------------------------------------------------------------
 * A group of decoder handles: callers of the reference API get the batch renderer's throughput.
 * The reference renders one handle, one frame per call (IAMF_decoder_decode, include/IAMF_decoder.h:82-99, driver loop
 * src/iamf_dec/IAMF_decoder.c:3303-3525).  N configured handles (IAMF_DecoderHandle of this library's IAMF_decoder.h) of ONE
 * topology — same codec configuration, elements, output layout, bit depth and limiter settings; their mix gains,
 * loudness and parameter streams may differ — that have not decoded yet hand their rendering to one batch:
 *     iamf_hip_decoder_group_decode(g, data, sizes, rsizes, pcm, results)
 * is, for every i, exactly  results[i] = IAMF_decoder_decode(handles[i], data[i], sizes[i], &rsizes[i], pcm[i])
 * (data[i] == NULL flushes handle i; rsizes may be NULL): parsing and the parameter timelines run per handle on
 * `host_threads` threads (0 = up to 16), which also copy each handle's LPCM packets, as they are, into pinned staging; then
 * ONE upload, the device unpacks (iamf_hip_lpcm_unpack above), one render launch over the streams that completed a
 * temporal unit, one download.  The handles need not advance in step.  While grouped, a handle refuses
 * IAMF_decoder_decode / _configure / _close with IAMF_ERR_INVALID_STATE; destroying the group releases the handles
 * (which are then closed with IAMF_decoder_close as usual).  Returns IAMF_OK, or for create: IAMF_ERR_BAD_ARG (handles
 * of different topologies), IAMF_ERR_INVALID_STATE (not configured / already decoding / a resampler inherited from an earlier IA sequence).  The group's own return value reports device failures only
 * (IAMF_ERR_INTERNAL): such a round is half applied — the library waits for what it had in flight, and every later
 * _decode of the group returns IAMF_ERR_INVALID_STATE; the valid call after a failure is _destroy.
 * ---------------------------------------------------------------------------------------- */
typedef struct iamf_hip_decoder_group iamf_hip_decoder_group;
int iamf_hip_decoder_group_create(void *const *handles, int n, int host_threads, iamf_hip_decoder_group **out);
/* where the group's calls spent their time so far, seconds: [0] host parsing + packet staging (the thread pool), [1] enqueueing
 * the uploads, the unpack and render launches and the download, [2] waiting for the device, [3] handing every handle its PCM;
 * *rounds (may be NULL) = rounds submitted (calls of iamf_hip_decoder_group_decode or _submit).  IAMF_OK or IAMF_ERR_BAD_ARG. */
int iamf_hip_decoder_group_times(const iamf_hip_decoder_group *g, double *seconds4, int64_t *rounds);
int iamf_hip_decoder_group_decode(iamf_hip_decoder_group *g, const uint8_t *const *data, const int32_t *sizes,
                                  uint32_t *rsizes, void *const *pcm, int32_t *results);
void iamf_hip_decoder_group_destroy(iamf_hip_decoder_group *g);

/* ------------------------------------------------------------------------------------------
 * A group's round in two halves: hand in the next round's packets while the previous round still renders (the send /
 * receive split of avcodec_send_packet / avcodec_receive_frame).  iamf_hip_decoder_group_decode is _submit followed by
 * _complete; split, the host's parsing of round k + 1 overlaps the device's rendering of round k.
 *   Equivalence: any interleaving of _submit and _complete with at most IAMF_HIP_GROUP_MAX_IN_FLIGHT rounds outstanding
 *     gives every handle exactly the results, rsizes, PCM bytes and metadata that the same rounds through
 *     iamf_hip_decoder_group_decode give, which is what IAMF_decoder_decode on each handle gives.
 *   Ordering errors return IAMF_ERR_INVALID_STATE and consume or change nothing: a _submit while
 *     IAMF_HIP_GROUP_MAX_IN_FLIGHT rounds are outstanding; a _complete of a ticket that is not the oldest outstanding one
 *     (never issued, already completed, or a later one); iamf_hip_decoder_group_decode while any round is outstanding.
 *   Destroy with rounds outstanding waits for their device work, writes nothing into those rounds' pcm buffers and
 *     releases the handles as usual (a temporal unit that is still incomplete keeps its packets).
 *   Device failure: a failure found by _submit or _complete returns IAMF_ERR_INTERNAL and latches the group; every later
 *     call returns IAMF_ERR_INVALID_STATE and _destroy is the valid call.  _poll reads a pinned word and nothing else: a
 *     device that has failed shows as a round that never becomes ready, and its _complete reports the failure.
 *   Metadata: a handle's clocks and IAMF_decoder_get_last_metadata advance at _submit.  Once every submitted round is
 *     complete they equal the synchronous path's; while a later round is outstanding they already describe that round.
 *   Timing (iamf_hip_decoder_group_times): [0] and [1] are accumulated in _submit, [2] (waiting) and [3] (hand-out) in
 *     _complete; *rounds counts submits.
 *   Threading: a group's calls must not run concurrently with each other.
 * ---------------------------------------------------------------------------------------- */
#define IAMF_HIP_GROUP_MAX_IN_FLIGHT 2
/* Host half of iamf_hip_decoder_group_decode: parse, stage, move the parameter clocks, enqueue the round's device work.
 * On return, results[i] and rsizes[i] are final.  data[i] may be reused.  pcm[i] belongs to the library until the
 * round's _complete returns (the array pcm itself may be reused).  *ticket identifies the round (increasing, from 1).
 * IAMF_OK, IAMF_ERR_BAD_ARG, IAMF_ERR_INVALID_STATE, IAMF_ERR_INTERNAL. */
int iamf_hip_decoder_group_submit(iamf_hip_decoder_group *g, const uint8_t *const *data, const int32_t *sizes,
                                  uint32_t *rsizes, void *const *pcm, int32_t *results, uint64_t *ticket);
/* 1: the round's PCM is ready (its _complete will not wait).  0: not yet.  IAMF_ERR_INVALID_STATE: the ticket is not
 * outstanding, or the group has failed.  Never blocks. */
int iamf_hip_decoder_group_poll(iamf_hip_decoder_group *g, uint64_t ticket);
/* Waits for the round's device work (that round only, not rounds submitted after it) and copies each handle's PCM into
 * the pcm[i] given at submit.  Rounds are completed in submit order.  IAMF_OK, IAMF_ERR_BAD_ARG, IAMF_ERR_INVALID_STATE,
 * IAMF_ERR_INTERNAL. */
int iamf_hip_decoder_group_complete(iamf_hip_decoder_group *g, uint64_t ticket);

#ifdef __cplusplus
}
#endif
#endif /* IAMF_HIP_H */
