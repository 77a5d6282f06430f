/*
 * facade_tu.h — what one temporal unit needs that is plain arithmetic: shared by the decoder facade's single handle
 * (iamf_decoder_facade.c) and its decoder group (iamf_decoder_group.inc), and checked on the host by
 * tests/facade_host/facade_host_check.c.  Plain C over integers, arrays and pointers; no decoder struct, no device call.
 */
#ifndef IAMF_FACADE_TU_H
#define IAMF_FACADE_TU_H

#include <stdint.h>
#include <string.h>

#include "iamf_hip.h"

enum { FTU_MAX_SUBSTREAMS = 24 };
enum { FTU_CHANNEL_BASED = 0, FTU_SCENE_BASED = 1 }; /* AudioElementType (IAMF_defines.h) */
enum { FTU_OK = 0, FTU_DROPPED = 1 };

/* ---- the trim window of a unit of ns samples (iamf_frame_trim, IAMF_decoder.c:1361-1381) ---- */
typedef struct {
  int s0, keep, te; /* first kept sample, samples kept, samples cut off the end */
  int rendered;     /* a unit that is cut away completely: the reference rendered it before it cut it, unless the start or
                       the end trim alone covers the whole frame of fs samples (IAMF_decoder.c:3354-3357) */
} ftu_window;

/* The trims are LEB128 fields of the OBU header: compared as uint64 BEFORE narrowing.  The reference refuses
 * start < 0 || end < 0 || samples - start - end < 0 (:1364-1370).  FTU_OK, FTU_DROPPED (keep <= 0) or IAMF_HIP_ERR_BAD_ARG. */
static inline int ftu_trim_window(int ns, uint64_t trim_start, uint64_t trim_end, int fs, ftu_window *w) {
  if (trim_start > (uint64_t)ns || trim_end > (uint64_t)ns || trim_start + trim_end > (uint64_t)ns) return IAMF_HIP_ERR_BAD_ARG;
  w->s0 = (int)trim_start;
  w->te = (int)trim_end;
  w->keep = ns - w->s0 - w->te;
  w->rendered = !(trim_start == (uint64_t)fs || trim_end == (uint64_t)fs) && ns > 0;
  return w->keep > 0 ? FTU_OK : FTU_DROPPED;
}

/* ---- the sub-streams of an element: width (2 = a coupled pair) and first decoded channel of each ---- */
typedef struct {
  int nsub, channels; /* sub-streams walked, decoded channels they give */
  int width[FTU_MAX_SUBSTREAMS], first[FTU_MAX_SUBSTREAMS];
} ftu_walk;

/* Audio-layer order: coupled sub-streams first, then singles — of the element (channel-based: nb_coupled; projection-mode
 * ambisonics: amb_coupled; else none), or with a demixer (n_layers > 0) of every layer in turn, over the layers' own
 * sub-streams (iamf_stream_scale_decoder_decode, IAMF_decoder.c:2276-2322; nsub is not used then).  0, or
 * IAMF_HIP_ERR_BAD_ARG for no sub-stream or more than FTU_MAX_SUBSTREAMS. */
static inline int ftu_walk_substreams(int type, int nsub, int nb_coupled, int amb_projection, int amb_coupled, int n_layers,
                                      const int *layer_nsub, const int *layer_ncoupled, ftu_walk *w) {
  const int coupled = type == FTU_CHANNEL_BASED ? nb_coupled : amb_projection ? amb_coupled : 0;
  memset(w, 0, sizeof(*w));
  for (int l = 0; l < (n_layers > 0 ? n_layers : 1); ++l) {
    const int n = n_layers > 0 ? layer_nsub[l] : nsub, nc = n_layers > 0 ? layer_ncoupled[l] : coupled;
    if (n < 0 || w->nsub + n > FTU_MAX_SUBSTREAMS) return IAMF_HIP_ERR_BAD_ARG;
    for (int j = 0; j < n; ++j, ++w->nsub) {
      w->width[w->nsub] = j < nc ? 2 : 1;
      w->first[w->nsub] = w->channels;
      w->channels += w->width[w->nsub];
    }
  }
  return w->nsub > 0 ? 0 : IAMF_HIP_ERR_BAD_ARG;
}

/* The decoded channel the renderer's channel p comes from: audio-layer -> playback order of a channel-based layout
 * (al_of_pl: its row of k_al_of_pl; IAMF_utils.c:117-133 vs :181-196) or the mono mapping of a scene-based element;
 * -1: no sub-stream carries it, the channel is zero. */
static inline int ftu_channel_source(int type, int p, const int *al_of_pl, const uint8_t *amb_map, int decoded) {
  const int src = type == FTU_CHANNEL_BASED ? al_of_pl[p] : amb_map[p];
  return src < decoded ? src : -1;
}

/* A raw row holds an element's packets as they are: `head` bytes, then sub-stream s at slot_off[s] (may be NULL), each
 * frame_size * width * sample bytes.  *L says where the device finds every channel in it: the decoded channels in their
 * order (decoded_order: projection de-mapping or a demixer follows on the device), else the renderer's `channels` through
 * ftu_channel_source.  Returns the row's bytes, or -1 for more channels than a layout holds. */
static inline int ftu_raw_layout(const ftu_walk *w, int decoded_order, int type, int channels, const int *al_of_pl,
                                 const uint8_t *amb_map, int bps, int little_endian, int fs, int head, int *slot_off,
                                 iamf_hip_lpcm_layout *L) {
  int off = head, ch_off[2 * FTU_MAX_SUBSTREAMS], ch_step[2 * FTU_MAX_SUBSTREAMS];
  for (int s = 0; s < w->nsub; ++s) {
    if (slot_off) slot_off[s] = off;
    for (int k = 0; k < w->width[s]; ++k) {
      ch_off[w->first[s] + k] = off + k * bps;
      ch_step[w->first[s] + k] = w->width[s] * bps;
    }
    off += w->width[s] * bps * fs;
  }
  memset(L, 0, sizeof(*L));
  L->sample_bytes = bps;
  L->little_endian = little_endian;
  L->frame_size = fs;
  L->channels = decoded_order ? w->channels : channels;
  if (L->channels > IAMF_HIP_LPCM_MAX_CHANNELS) return -1;
  for (int p = 0; p < L->channels; ++p) {
    const int src = decoded_order ? p : ftu_channel_source(type, p, al_of_pl, amb_map, w->channels);
    L->src_offset[p] = src < 0 ? -1 : ch_off[src];
    L->src_step[p] = src < 0 ? bps : ch_step[src];
  }
  return off;
}

/* ---- iamf_hip_render_args of one element's stage for one (possibly trimmed) frame ----
 * d_in: the element's planar rows [in_channels][fs] (NULL: the packets go to the kernel themselves).  An element that
 * feeds the HOA LFE generator (lfe) keeps its whole frame — the reference renders first and trims the result
 * (IAMF_decoder.c:3424-3430), so the generator's filter runs over the trimmed samples too: d_in moves to the first kept
 * sample and the stage is told how many lie in front of and behind the call.  Every other element's rows start at the
 * first kept sample already.  dmx / demix: the frame records of the stage in front of the renderer, or NULL. */
static inline void ftu_element_stage_args(iamf_hip_render_args *a, const float *d_in, int in_channels, int fs, int lfe, int s0,
                                          int te, int keep, const iamf_hip_dmx_frame *dmx, const iamf_hip_demix_frame *demix,
                                          void *stream) {
  memset(a, 0, sizeof(*a));
  a->d_in = d_in && lfe ? d_in + s0 : d_in;
  a->in_stream_stride = a->in_frame_stride = (int64_t)in_channels * fs;
  if (lfe) {
    a->lfe_pre_samples = s0;
    a->lfe_post_samples = te;
  }
  a->d_dmx_frames = dmx;
  if (demix) {
    a->d_demix_frames = demix;
    a->demix_sample0 = s0;
  }
  a->n_frames = 1;
  a->n_samples = keep < fs ? keep : 0;
  a->stream = stream;
}

/* ---- the last stage behind the resampler: loudness, limiter and PCM pack over interleaved f32 ---- */
/* the identity over oc channels: 0 + 1 * y[c] + 0 * y[..] is y[c] for every finite y.  eye: caller-owned float[24 * 24] */
static inline void ftu_identity_matrix(int oc, float *eye, iamf_hip_matrix *m) {
  for (int i = 0; i < oc; ++i)
    for (int j = 0; j < oc; ++j) eye[i * oc + j] = i == j ? 1.f : 0.f;
  memset(m, 0, sizeof(*m));
  m->kind = IAMF_HIP_KIND_M2M;
  m->m = m->n = m->channels = oc;
  m->lfe1 = m->lfe2 = -1;
  m->mat = eye;
}

static inline void ftu_last_stage_config(iamf_hip_batch_config *c, float *eye, int n_streams, int out_rate, int oc, int out_format,
                                         int pcm_stride, int limiter_on, float limiter_db, int loudness_on) {
  memset(c, 0, sizeof(*c));
  c->n_streams = n_streams;
  c->frame_size = 1; /* interleaved f32 in */
  c->sample_rate = out_rate;
  c->out_channels = oc;
  c->out_format = out_format;
  c->pcm_stride_channels = pcm_stride;
  ftu_identity_matrix(oc, eye, &c->matrix);
  c->limiter_enable = limiter_on;
  c->limiter_threshold_db = limiter_db;
  c->loudness_enable = loudness_on;
  c->projection = IAMF_HIP_PROJ_EXACT;
}

/* n_frames sample-frames per stream of what the resampler left at d_res + stream * res_stride -> PCM */
static inline void ftu_last_stage_args(iamf_hip_render_args *a, const float *d_res, int64_t res_stride, int oc, int n_frames,
                                       void *d_pcm, int64_t pcm_stream_stride_bytes, void *stream) {
  memset(a, 0, sizeof(*a));
  a->d_in = d_res;
  a->in_stream_stride = res_stride;
  a->in_frame_stride = oc;
  a->n_frames = n_frames;
  a->stream = stream;
  a->d_pcm = d_pcm;
  a->pcm_stream_stride_bytes = pcm_stream_stride_bytes;
}

#endif
