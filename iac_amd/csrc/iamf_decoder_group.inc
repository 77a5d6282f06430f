/*
 * iamf_decoder_group.inc — N decoder handles of ONE topology behind ONE batch (included at the end of
 * iamf_decoder_facade.c; include/iamf_hip.h: iamf_hip_decoder_group_*).
 *
 * The reference's only entry renders one handle, one frame per call (include/IAMF_decoder.h:99, driver loop
 * src/iamf_dec/IAMF_decoder.c:3303-3525); the single-handle facade above keeps that shape literally and pays three
 * small copies, a launch and a synchronisation per 1024 samples.  A caller that serves many streams of one kind (the
 * BASELINE's "4096 concurrent mix presentations") hands their handles to a group and calls ONE function per round of
 * temporal units:
 *     iamf_hip_decoder_group_decode(g, data[], sizes[], rsizes[], pcm[], results[])
 * which is, per handle i, exactly IAMF_decoder_decode(handle[i], data[i], sizes[i], &rsizes[i], pcm[i]) -> results[i]:
 * OBU parsing and the parameter timelines run per handle on a pool of host threads, which copy the handle's LPCM
 * packets AS THEY ARE into pinned staging (one fixed slot per sub-stream); then one upload, the device unpacks them to
 * [stream][channel][frame size] f32 in the renderer's channel order (iamf_hip_lpcm_unpack: the conversion cost the host
 * 3 ns per sample and was most of a round; the upload is half the bytes for 16-bit streams), one render launch over all
 * streams that completed a temporal unit, one download.  Handles need not advance in step: a stream whose unit is still incomplete is left out of the
 * launch, a trimmed frame or a flush is rendered by a range launch of its own (iamf_hip_batch_render_range), so every
 * handle's PCM is what it would have returned alone (tests/test_gpu_group.py: the e2e goldens over 64 handles).
 *
 * Streams of one mono-coded ambisonics element in 16-bit LPCM into one or two channels skip the unpacker: the render kernel reads
 * the uploaded packets itself (iamf_hip_batch_render_packets_ragged; IAMF_HIP_GROUP_UNPACK=1 in the environment: unpack first).
 * So do streams of two elements whose packets the two-element forms read (iamf_hip_batch_render_packets_mix_ragged; lp_worth_asking).
 *
 * Handles that resample (stream rate != output rate: IAMF_decoder.c:3193-3199,3223-3248) render through three stages as the
 * single handle does — the batch into planar-per-stream f32, the resampler (one phase and history per stream,
 * iamf_hip_resampler_process_range), a second batch for loudness / limiter / pack — and a launch then covers streams that
 * also agree in their resampler state and in the second batch's position.  The HOA LFE generator's pre-pass takes the
 * range of a launch (round 4; both were refused before).
 */
#include <pthread.h>
#include <sched.h>

enum { GA_NONE = 0, GA_RENDER = 1, GA_FLUSH = 2, GA_ADVANCE = 3 /* a unit trimmed away completely: the LFE generator's filter only */ };
enum { kRawHead = 16 };

struct iamf_hip_decoder_group {
  int n;
  struct IAMF_Decoder **d;
  iamf_hip_batch *batch;
  /* both elements behind a stage of their own (IAMF_Decoder::aux): element 1's batch for n streams, its frame as written
   * [n][fs][out_ch] and planar [n][out_ch][fs] (the render batch's second element, identity matrix), its stage records,
   * and a row of ones per stream — element 1's mix gain is applied by `aux` through ramp row 1 */
  iamf_hip_batch *aux;
  float *d_aux_il, *d_aux_pl, *d_ones;
  iamf_hip_dmx_frame *h_dmx1, *d_dmx1;       /* [n] (h_dmx1: the current slot's, group_use_slot) */
  iamf_hip_demix_frame *h_demix1, *d_demix1; /* [n] */
  /* resampling handles: the stages behind the render batch (as IAMF_Decoder::rs / batch3 / d_mid / d_res, for n streams) */
  iamf_hip_batch *batch3;
  iamf_hip_resampler *rs;
  float *d_mid, *d_res;           /* [n][mid_stride] interleaved f32 of a frame; [n][res_stride] after the resampler */
  int64_t mid_stride, res_stride; /* floats per stream */
  int64_t *pos3;                  /* sample-frames the stream has pushed into batch3 */
  float *loud3;                   /* [n] the loudness gain batch3 holds per stream (1 once the stream has been flushed) */
  int out_ch, limiter_on;
  hipStream_t stream;
  int fs, nel, in_ch[2], bytes;
  size_t pcm_cap;                 /* bytes per stream in h_pcm */
  float *d_in[2];                 /* [n][ch][fs], written by the device unpacker */
  /* LPCM packets as uploaded: per element [n][raw_stride] bytes, sub-stream s of a handle at slot_off[s] */
  iamf_hip_lpcm_layout lay[2];
  const ftu_walk *walk[2];        /* handle 0's: the sub-streams of element e and their widths */
  int slot_off[2][MAX_SUBSTREAMS];
  size_t raw_stride[2];
  uint8_t *h_raw[2];
  void *d_raw[2];
  /* every raw row starts with kRawHead bytes: int32 first sample (a trimmed start), int32 samples to unpack (0: not this round) */
  float *cgain[3];                /* [n]: this frame's constant gain of stage k where the stage is not on a ramp */
  int lp_ok;                      /* element 0's packets can go straight into the render kernel (iamf_hip_batch_render_packets_ragged) */
  int chunk, nchunks;             /* handles per upload chunk; the uploads of chunk c run beside the parsing of chunk c + 1 */
  int *chunk_done;                /* [nchunks]: handles of the chunk the pool has finished (atomic) */
  int job;                        /* what the pool does this time: 0 parse + stage, 1 hand out the PCM */
  void **pcm_out;
  float *h_ramp[3], *d_ramp[3];   /* [n][fs] */
  iamf_hip_dmx_frame *h_dmx, *d_dmx;       /* [n] */
  iamf_hip_demix_frame *h_demix, *d_demix; /* [n] */
  uint8_t *h_pcm;                 /* pinned; the render kernels write it directly */
  float *gain_cur, *gain_new;     /* [2][n]: element / output constant gains on the device, and this call's */
  /* per handle, per call */
  int *action, *keep, *s0, *result, *rampf;  /* rampf: bit k = stage k is a per-sample ramp in this frame */
  int *te;                        /* samples trimmed off the END of the frame (the LFE generator's filter runs over them) */
  int lfe[2];                     /* element e feeds the HOA LFE generator: its frames are unpacked whole (group_prepare_tu) */
  int rampu, unpacked;            /* of the round: stages applied through their ramp rows (bits); the device unpacker has run */
  int64_t *pos;                   /* samples the stream has consumed in the batch */
  const uint8_t *const *data;
  const int32_t *sizes;
  uint32_t *rsizes;
  /* Two rounds in flight (iamf_hip_decoder_group_submit / _complete): everything the host writes in a round and the
   * device or the copy engine reads later has one copy per slot; round `ticket` uses slot ticket & 1, and the fields
   * above that name such a buffer (h_raw, h_ramp, h_dmx, h_demix, h_dmx1, h_demix1, h_pcm, action .. te, pcm_out) point
   * at the slot the call is working on (group_use_slot).  Device buffers stay single: the group's one in-order stream
   * runs round k + 1's upload and launches after round k's last kernel, so round k + 1 can only overwrite d_raw, d_in,
   * d_ramp, ... once round k has read them; only what the HOST writes before round k's kernels have run needs two. */
  struct {
    uint8_t *h_raw[2];
    float *h_ramp[3];
    iamf_hip_dmx_frame *h_dmx, *h_dmx1;
    iamf_hip_demix_frame *h_demix, *h_demix1;
    uint8_t *h_pcm;
    int *action, *keep, *s0, *result, *rampf, *te;
    void **pcm_out;   /* [n]: the caller's pcm[] of the round, copied at submit */
    int dev;          /* the round queued device work: its completion is signalled (h_sig) */
  } slot[2];
  uint64_t issued, done;      /* tickets: the last submitted, the last completed (issued - done = rounds outstanding) */
  volatile uint32_t *h_sig;   /* pinned word: iamf_hip_stream_signal writes a round's ticket behind its last launch */
  /* host thread pool: workers take handle indices from `next` */
  int nthreads;
  pthread_t *threads;
  pthread_mutex_t mu;
  pthread_cond_t cv_work, cv_done;
  int generation, pending, stop;
  volatile int next;
  int failed;        /* a device call of a round failed: the round is half applied; every later decode is refused */
  double t_phase[4]; /* seconds spent in: host parse + staging, uploads + launches (enqueue), waiting for the device, copy-out */
  int64_t rounds;
};

static double group_now(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

int iamf_hip_decoder_group_times(const iamf_hip_decoder_group *g, double *seconds4, int64_t *rounds) {
  if (!g || !seconds4) return IAMF_ERR_BAD_ARG;
  for (int k = 0; k < 4; ++k) seconds4[k] = g->t_phase[k];
  if (rounds) *rounds = g->rounds;
  return IAMF_OK;
}

/* the round-local fields name slot `sl`'s buffers from here on (a round's submit, its complete) */
static void group_use_slot(iamf_hip_decoder_group *g, int sl) {
  for (int e = 0; e < 2; ++e) g->h_raw[e] = g->slot[sl].h_raw[e];
  for (int k = 0; k < 3; ++k) g->h_ramp[k] = g->slot[sl].h_ramp[k];
  g->h_dmx = g->slot[sl].h_dmx;
  g->h_dmx1 = g->slot[sl].h_dmx1;
  g->h_demix = g->slot[sl].h_demix;
  g->h_demix1 = g->slot[sl].h_demix1;
  g->h_pcm = g->slot[sl].h_pcm;
  g->action = g->slot[sl].action;
  g->keep = g->slot[sl].keep;
  g->s0 = g->slot[sl].s0;
  g->result = g->slot[sl].result;
  g->rampf = g->slot[sl].rampf;
  g->te = g->slot[sl].te;
  g->pcm_out = g->slot[sl].pcm_out;
}

static int group_parse_one(iamf_hip_decoder_group *g, int i);
/* A device call of a round failed (ADVICE r3): packets are consumed and clocks partly moved, so the round cannot be
 * repeated.  Wait for what is in flight (upload kernels still read the pinned rows the next parse would overwrite), mark
 * the group: every later iamf_hip_decoder_group_decode returns IAMF_ERR_INVALID_STATE; destroy is the valid call. */
static int group_fail(iamf_hip_decoder_group *g) {
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  g->failed = 1;
  return IAMF_ERR_INTERNAL;
}
static void group_copy_out_one(iamf_hip_decoder_group *g, int i);

static void group_do(iamf_hip_decoder_group *g, int i) {
  if (g->job == 0) {
    g->result[i] = group_parse_one(g, i);
    __atomic_fetch_add(&g->chunk_done[i / g->chunk], 1, __ATOMIC_RELEASE); /* the row of handle i is complete */
  } else {
    group_copy_out_one(g, i);
  }
}

static void group_relax(void) {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  __asm__ volatile("" ::: "memory");
#endif
}
enum { kGroupSpin = 20000 }; /* polls before a thread goes to sleep on its condition variable (~0.3 ms) */

/* A worker waits for the next job by polling first: the jobs of one round (parse, hand out) and the next round of a
 * caller that is busy decoding follow each other within a fraction of a millisecond, and waking fifteen sleeping
 * threads costs 30-60 us each time (64 handles: 88 us per round in a phase with 25 us of work). */
static void *group_worker(void *arg) {
  iamf_hip_decoder_group *g = (iamf_hip_decoder_group *)arg;
  int seen = 0;
  for (;;) {
    for (int spin = 0; spin < kGroupSpin; ++spin) {
      if (__atomic_load_n(&g->generation, __ATOMIC_ACQUIRE) != seen || __atomic_load_n(&g->stop, __ATOMIC_ACQUIRE)) break;
      group_relax();
    }
    pthread_mutex_lock(&g->mu);
    while (!g->stop && g->generation == seen) pthread_cond_wait(&g->cv_work, &g->mu);
    if (g->stop) {
      pthread_mutex_unlock(&g->mu);
      return 0;
    }
    seen = g->generation;
    pthread_mutex_unlock(&g->mu);
    for (;;) {
      int i = __atomic_fetch_add(&g->next, 1, __ATOMIC_RELAXED);
      if (i >= g->n) break;
      group_do(g, i);
    }
    if (__atomic_sub_fetch(&g->pending, 1, __ATOMIC_ACQ_REL) == 0) {
      pthread_mutex_lock(&g->mu);
      pthread_cond_signal(&g->cv_done);
      pthread_mutex_unlock(&g->mu);
    }
  }
}

/* start job `job` over all handles on the pool; with `help` the calling thread takes handles too.  group_join waits. */
static void group_start(iamf_hip_decoder_group *g, int job) {
  g->job = job;
  for (int c = 0; c < g->nchunks; ++c) g->chunk_done[c] = 0;
  if (g->nthreads <= 0) return;
  pthread_mutex_lock(&g->mu);
  g->next = 0;
  __atomic_store_n(&g->pending, g->nthreads, __ATOMIC_RELAXED);
  __atomic_store_n(&g->generation, g->generation + 1, __ATOMIC_RELEASE); /* publishes job, next, pending, chunk_done */
  pthread_cond_broadcast(&g->cv_work);
  pthread_mutex_unlock(&g->mu);
}

static void group_help(iamf_hip_decoder_group *g) { /* the calling thread works too */
  if (g->nthreads <= 0) {
    for (int i = 0; i < g->n; ++i) group_do(g, i);
    return;
  }
  for (;;) {
    int i = __atomic_fetch_add(&g->next, 1, __ATOMIC_RELAXED);
    if (i >= g->n) break;
    group_do(g, i);
  }
}

static void group_join(iamf_hip_decoder_group *g) {
  if (g->nthreads <= 0) return;
  for (int spin = 0; spin < kGroupSpin; ++spin) {
    if (!__atomic_load_n(&g->pending, __ATOMIC_ACQUIRE)) return;
    group_relax();
  }
  pthread_mutex_lock(&g->mu);
  while (__atomic_load_n(&g->pending, __ATOMIC_ACQUIRE)) pthread_cond_wait(&g->cv_done, &g->mu);
  pthread_mutex_unlock(&g->mu);
}

/* Where the device unpacker finds every channel of element ei: sub-stream s of a handle is copied to a fixed slot of the
 * handle's raw row, behind the row's head (element_raw_layout: the single handle's packet row is laid out by the same) */
static int group_build_layout(iamf_hip_decoder_group *g, const struct IAMF_Decoder *d, int ei) {
  const int row = (g->fs & 3) ? -1 : element_raw_layout(d, ei, kRawHead, g->slot_off[ei], &g->lay[ei]);
  if (row < 0 || g->lay[ei].channels > g->in_ch[ei]) return 1;
  g->walk[ei] = &d->walk[ei];
  g->raw_stride[ei] = ((size_t)row + 255) & ~(size_t)255;
  return 0;
}

/* unpack_element's checks, and the packets of handle i's element ei into its raw row; returns samples per channel */
static int group_stage_raw(iamf_hip_decoder_group *g, int i, int ei) {
  const struct IAMF_Decoder *d = g->d[i];
  const int bps = (int)d->sample_size / 8, fs = g->fs;
  uint8_t *row = g->h_raw[ei] + (size_t)i * g->raw_stride[ei];
  int ns = -1;
  for (int s = 0; s < g->walk[ei]->nsub; ++s) {
    const int w = g->walk[ei]->width[s];
    const int n = (int)(d->pkt_len[ei][s] / (uint32_t)(w * bps));
    if (ns < 0) ns = n;
    if (n != ns || n > fs) return IAMF_ERR_INVALID_PACKET;
    if (!d->pkt_in_ext[ei][s]) memcpy(row + g->slot_off[ei][s], d->pkt[ei][s], (size_t)n * w * bps); /* else decode_parse put it there */
  }
  if (ns < 0) return IAMF_ERR_INVALID_PACKET;
  return ns;
}

/* what two handles must share to sit in one batch: everything build_stages derives the batches from, and the walk of
 * their sub-streams (element_walk) */
static int group_compatible(const struct IAMF_Decoder *a, const struct IAMF_Decoder *b) {
  if (a->frame_size != b->frame_size || a->rate != b->rate || a->out_rate != b->out_rate || a->sample_size != b->sample_size ||
      a->little_endian != b->little_endian || /* the batch's one unpack layout is built from handle 0's byte order */
      a->bit_depth != b->bit_depth || a->out_type != b->out_type || a->out_ss != b->out_ss || a->limiter_on != b->limiter_on ||
      a->limiter_db != b->limiter_db || (a->norm_loudness != 0.f) != (b->norm_loudness != 0.f) || a->tv != b->tv ||
      a->lfe_hoa != b->lfe_hoa || a->sel->nel != b->sel->nel || a->pre[0].use_dmx != b->pre[0].use_dmx || a->pre[0].use_demix != b->pre[0].use_demix)
    return 0;
  if (memcmp(&a->cfg_sig, &b->cfg_sig, sizeof(a->cfg_sig))) return 0;
  if (a->pre[0].use_demix && (memcmp(&a->pre[0].dc_sig, &b->pre[0].dc_sig, sizeof(a->pre[0].dc_sig)) || a->pre[0].demix_layer != b->pre[0].demix_layer)) return 0;
  if (!a->aux != !b->aux) return 0;
  if (a->aux && (memcmp(&a->aux_sig, &b->aux_sig, sizeof(a->aux_sig)) || a->aux_mat != b->aux_mat ||
                 a->pre[1].use_dmx != b->pre[1].use_dmx || a->pre[1].use_demix != b->pre[1].use_demix ||
                 (a->pre[1].use_demix && (memcmp(&a->pre[1].dc_sig, &b->pre[1].dc_sig, sizeof(a->pre[1].dc_sig)) ||
                                          a->pre[1].demix_layer != b->pre[1].demix_layer))))
    return 0;
  for (int e = 0; e < a->sel->nel; ++e) {
    const Element *x = a->sel_el[e], *y = b->sel_el[e];
    if (x->type != y->type || x->layout != y->layout || x->channels != y->channels || x->nsub != y->nsub ||
        x->nb_coupled != y->nb_coupled || x->amb_projection != y->amb_projection || x->amb_coupled != y->amb_coupled ||
        x->nlayers != y->nlayers || element_in_channels(x) != element_in_channels(y))
      return 0;
    if (x->type == AUDIO_ELEMENT_SCENE_BASED) {
      if (x->amb_projection) {
        if (memcmp(x->proj, y->proj, sizeof(float) * (size_t)element_in_channels(x) * x->channels)) return 0;
      } else if (memcmp(x->amb_map, y->amb_map, sizeof(x->amb_map[0]) * x->channels)) {
        return 0;
      }
    }
    for (int l = 0; l < x->nlayers; ++l)
      if (x->layer[l].layout != y->layer[l].layout || x->layer[l].nsub != y->layer[l].nsub ||
          x->layer[l].ncoupled != y->layer[l].ncoupled || x->layer[l].recon_flag != y->layer[l].recon_flag)
        return 0;
  }
  return 1;
}

void iamf_hip_decoder_group_destroy(iamf_hip_decoder_group *g) {
  if (!g) return;
  if (g->threads) {
    pthread_mutex_lock(&g->mu);
    __atomic_store_n(&g->stop, 1, __ATOMIC_RELEASE); /* the polling workers read it without the lock */
    pthread_cond_broadcast(&g->cv_work);
    pthread_mutex_unlock(&g->mu);
    for (int t = 0; t < g->nthreads; ++t) pthread_join(g->threads[t], 0);
    free(g->threads);
    pthread_mutex_destroy(&g->mu);
    pthread_cond_destroy(&g->cv_work);
    pthread_cond_destroy(&g->cv_done);
  }
  /* rounds still outstanding: their device work is waited for, their PCM is never handed out (the caller's pcm buffers
   * of those rounds stay as they are); their clocks had moved at submit, as they would have by their _complete */
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  for (int i = 0; i < g->n && g->d; ++i)
    if (g->d[i] && g->d[i]->group == g) {
      struct IAMF_Decoder *d = g->d[i];
      d->group = 0;
      for (int e = 0; e < 2; ++e)
        for (int s2 = 0; s2 < MAX_SUBSTREAMS; ++s2) {
          /* a packet of a temporal unit that is still incomplete lives in the row that is about to go (the slot of the
           * handle's last submit: group_parse_one moves it along): back to the heap */
          if (d->pkt_in_ext[e][s2] && d->pkt_have[e][s2] && d->pkt_ext[e][s2]) {
            const uint32_t len = d->pkt_len[e][s2];
            if (len > d->pkt_cap[e][s2]) {
              uint8_t *nb = (uint8_t *)realloc(d->pkt[e][s2], len ? len : 1);
              if (nb) {
                d->pkt[e][s2] = nb;
                d->pkt_cap[e][s2] = len ? len : 1;
              } else {
                d->pkt_have[e][s2] = 0; /* out of memory: the unit is lost, the stream goes on with the next */
              }
            }
            if (d->pkt_have[e][s2]) memcpy(d->pkt[e][s2], d->pkt_ext[e][s2], len);
          }
          d->pkt_ext[e][s2] = 0;
          d->pkt_ext_cap[e][s2] = 0;
          d->pkt_in_ext[e][s2] = 0;
        }
    }
  if (g->aux) iamf_hip_batch_destroy(g->aux); /* (before `batch`, whose LFE filter state it may share) */
  if (g->batch) iamf_hip_batch_destroy(g->batch);
  if (g->d_aux_il) (void)hipFree(g->d_aux_il);
  if (g->d_aux_pl) (void)hipFree(g->d_aux_pl);
  if (g->d_ones) (void)hipFree(g->d_ones);
  if (g->d_dmx1) (void)hipFree(g->d_dmx1);
  if (g->d_demix1) (void)hipFree(g->d_demix1);
  if (g->batch3) iamf_hip_batch_destroy(g->batch3);
  if (g->rs) iamf_hip_resampler_destroy(g->rs);
  if (g->d_mid) (void)hipFree(g->d_mid);
  if (g->d_res) (void)hipFree(g->d_res);
  free(g->pos3);
  free(g->loud3);
  for (int e = 0; e < 2; ++e) {
    if (g->d_raw[e]) (void)hipFree(g->d_raw[e]);
    if (g->d_in[e]) (void)hipFree(g->d_in[e]);
  }
  for (int k = 0; k < 3; ++k) free(g->cgain[k]);
  free(g->chunk_done);
  for (int k = 0; k < 3; ++k)
    if (g->d_ramp[k]) (void)hipFree(g->d_ramp[k]);
  if (g->d_dmx) (void)hipFree(g->d_dmx);
  if (g->d_demix) (void)hipFree(g->d_demix);
  for (int sl = 0; sl < 2; ++sl) {
    for (int e = 0; e < 2; ++e)
      if (g->slot[sl].h_raw[e]) (void)hipHostFree(g->slot[sl].h_raw[e]);
    for (int k = 0; k < 3; ++k)
      if (g->slot[sl].h_ramp[k]) (void)hipHostFree(g->slot[sl].h_ramp[k]);
    if (g->slot[sl].h_dmx) (void)hipHostFree(g->slot[sl].h_dmx);
    if (g->slot[sl].h_dmx1) (void)hipHostFree(g->slot[sl].h_dmx1);
    if (g->slot[sl].h_demix) (void)hipHostFree(g->slot[sl].h_demix);
    if (g->slot[sl].h_demix1) (void)hipHostFree(g->slot[sl].h_demix1);
    if (g->slot[sl].h_pcm) (void)hipHostFree(g->slot[sl].h_pcm);
    free(g->slot[sl].action);
    free(g->slot[sl].keep);
    free(g->slot[sl].s0);
    free(g->slot[sl].result);
    free(g->slot[sl].rampf);
    free(g->slot[sl].te);
    free(g->slot[sl].pcm_out);
  }
  if (g->h_sig) (void)hipHostFree((void *)g->h_sig);
  if (g->stream) (void)hipStreamDestroy(g->stream);
  free(g->gain_cur);
  free(g->gain_new);
  free(g->pos);
  free(g->d);
  free(g);
}

/* ---- iamf_hip_decoder_group_create's steps: validate, host arrays, stages, staging, threads ---- */

static int group_validate(void *const *handles, int n) {
  for (int i = 0; i < n; ++i) {
    const struct IAMF_Decoder *d = (const struct IAMF_Decoder *)handles[i];
    if (!d) return IAMF_ERR_BAD_ARG;
    if (!d->configured || d->need_reconf || d->group || d->timestamp != 0 || d->flushed) return IAMF_ERR_INVALID_STATE;
    if (d->rs_inherited) return IAMF_ERR_INVALID_STATE; /* its resampler carries an earlier IA sequence's history (inherit_resampler) */
    for (int k = 0; k < i; ++k)
      if (handles[k] == handles[i]) return IAMF_ERR_BAD_ARG;
  }
  for (int i = 1; i < n; ++i)
    if (!group_compatible((const struct IAMF_Decoder *)handles[0], (const struct IAMF_Decoder *)handles[i])) return IAMF_ERR_BAD_ARG;
  return IAMF_OK;
}

/* what the group knows of its handles' one topology (handle 0's), and its per-handle host arrays */
static int group_alloc_host(iamf_hip_decoder_group *g, const struct IAMF_Decoder *d0) {
  const size_t n = (size_t)g->n;
  int ok = 1;
  g->fs = (int)d0->frame_size;
  g->nel = d0->sel->nel;
  g->bytes = (int)d0->bit_depth / 8;
  g->lfe[0] = d0->cfg_sig.lfe_hoa;
  g->lfe[1] = d0->aux && d0->aux_sig.lfe_hoa;
  g->out_ch = d0->out_channels;
  g->limiter_on = d0->limiter_on;
  g->d = (struct IAMF_Decoder **)calloc(n, sizeof(*g->d));
  for (int sl = 0; sl < 2; ++sl) {
    int **per[6] = {&g->slot[sl].action, &g->slot[sl].keep, &g->slot[sl].s0, &g->slot[sl].result, &g->slot[sl].rampf, &g->slot[sl].te};
    for (int k = 0; k < 6; ++k) ok &= (*per[k] = (int *)calloc(n, sizeof(int))) != 0;
    ok &= (g->slot[sl].pcm_out = (void **)calloc(n, sizeof(void *))) != 0;
  }
  g->pos = (int64_t *)calloc(n, sizeof(int64_t));
  g->pos3 = (int64_t *)calloc(n, sizeof(int64_t));
  g->gain_cur = (float *)malloc(sizeof(float) * 2 * n);
  g->gain_new = (float *)malloc(sizeof(float) * 2 * n);
  return ok && g->d && g->pos && g->pos3 && g->gain_cur && g->gain_new ? IAMF_OK : IAMF_ERR_ALLOC_FAIL;
}

/* element 1's stage for n streams (aux_stage_create, as a handle's), with what a group launch of it reads */
static int group_create_aux(iamf_hip_decoder_group *g, struct IAMF_Decoder *d0, const float *ones) {
  const size_t n = (size_t)g->n, row = sizeof(float) * n * g->fs;
  float *h1;
  if (aux_stage_create(d0, g->n, 0, g->batch, ones, &g->aux, &g->d_aux_il, &g->d_aux_pl)) return 1;
  if (hipMalloc((void **)&g->d_ones, row) != hipSuccess || hipMalloc((void **)&g->d_dmx1, sizeof(iamf_hip_dmx_frame) * n) != hipSuccess ||
      hipMalloc((void **)&g->d_demix1, sizeof(iamf_hip_demix_frame) * n) != hipSuccess)
    return 1;
  for (int sl = 0; sl < 2; ++sl)
    if (hipHostMalloc((void **)&g->slot[sl].h_dmx1, sizeof(iamf_hip_dmx_frame) * n, 0) != hipSuccess ||
        hipHostMalloc((void **)&g->slot[sl].h_demix1, sizeof(iamf_hip_demix_frame) * n, 0) != hipSuccess)
      return 1;
  /* the ones, through the ramp rows' own upload path (h_ramp is not allocated yet: a scratch vector) */
  if (!(h1 = (float *)malloc(row))) return 1;
  for (size_t k = 0; k < n * g->fs; ++k) h1[k] = 1.f;
  const int rc = hipMemcpy(g->d_ones, h1, row, hipMemcpyHostToDevice) != hipSuccess;
  free(h1);
  return rc;
}

/* the stages behind the render batch for n streams (last_stage_create, as a handle's) and the buffers between them.
 * Loudness belongs to the last stage: ones[n ..] go there and are 1 afterwards, for the render batch */
static int group_create_last(iamf_hip_decoder_group *g, const struct IAMF_Decoder *d0, float *ones) {
  const int n = g->n;
  if (last_stage_create(d0, n, &g->rs, &g->batch3)) return 1;
  g->mid_stride = (int64_t)g->fs * g->out_ch;
  /* (a multiple of 4 floats: every stream's row on the 16-byte grid, which the last stage's fast form wants — render_last_stage) */
  g->res_stride = ((int64_t)(iamf_hip_resampler_out_capacity(g->rs, g->fs) + iamf_hip_resampler_flush_capacity(g->rs) + 512) * g->out_ch + 3) & ~(int64_t)3;
  if (hipMalloc((void **)&g->d_mid, sizeof(float) * (size_t)n * g->mid_stride) != hipSuccess ||
      hipMalloc((void **)&g->d_res, sizeof(float) * (size_t)n * g->res_stride) != hipSuccess)
    return 1;
  if (iamf_hip_batch_set_gains(g->batch3, ones, ones, ones + n) || !(g->loud3 = (float *)malloc(sizeof(float) * (size_t)n))) return 1;
  for (int i = 0; i < n; ++i) {
    g->loud3[i] = ones[n + i];
    ones[n + i] = 1.f;
  }
  return 0;
}

/* the handles' batches, for n streams: the render batch (build_stages) with element 0's stage, element 1's, the last */
static int group_create_stages(iamf_hip_decoder_group *g, void *const *handles) {
  struct IAMF_Decoder *d0 = (struct IAMF_Decoder *)handles[0];
  iamf_hip_batch_config cfg = d0->cfg_sig;
  const int n = g->n;
  float *ones;
  int rc = 0;
  cfg.n_streams = n;
  cfg.matrix.mat = d0->cfg_mat;
  if (iamf_hip_batch_create(&cfg, &g->batch) || stage_attach(d0, 0, g->batch)) return 1;
  if (!(ones = (float *)malloc(sizeof(float) * 2 * n))) return 1;
  for (int i = 0; i < n; ++i) {
    ones[i] = 1.f;
    ones[n + i] = db2lin(((struct IAMF_Decoder *)handles[i])->norm_loudness - ((struct IAMF_Decoder *)handles[i])->mix_loudness);
  }
  if (g->nel == 2 && !d0->aux) {
    iamf_hip_matrix m2;
    rc = element_matrix(d0, d0->sel_el[1], &m2) || iamf_hip_batch_set_second_element(g->batch, &m2, ones);
  }
  if (!rc && d0->aux) rc = group_create_aux(g, d0, ones);
  if (!rc && d0->rs) rc = group_create_last(g, d0, ones);
  rc = rc || iamf_hip_batch_set_gains(g->batch, ones, ones, ones + n);
  for (int i = 0; i < 2 * n; ++i) g->gain_cur[i] = 1.f;
  free(ones);
  return rc;
}

/* the stream, the device buffers of a round and the pinned rows of its two slots; the handles' packets go straight to
 * their rows from here on */
static int group_alloc_staging(iamf_hip_decoder_group *g, void *const *handles) {
  struct IAMF_Decoder *d0 = (struct IAMF_Decoder *)handles[0];
  const size_t n = (size_t)g->n;
  if (hipStreamCreate(&g->stream) != hipSuccess) return 1;
  for (int e = 0; e < g->nel; ++e) {
    g->in_ch[e] = element_in_channels(d0->sel_el[e]);
    if (group_build_layout(g, d0, e)) return 1;
    /* rows of channels that no sub-stream carries in a projection / demixer element are never written: keep them defined */
    if (hipMalloc((void **)&g->d_in[e], sizeof(float) * n * g->in_ch[e] * g->fs) != hipSuccess ||
        hipMemset(g->d_in[e], 0, sizeof(float) * n * g->in_ch[e] * g->fs) != hipSuccess)
      return 1;
    for (int sl = 0; sl < 2; ++sl) {
      if (hipHostMalloc((void **)&g->slot[sl].h_raw[e], g->raw_stride[e] * n, 0) != hipSuccess) return 1;
      memset(g->slot[sl].h_raw[e], 0, g->raw_stride[e] * n);
    }
    if (hipMalloc(&g->d_raw[e], g->raw_stride[e] * n) != hipSuccess) return 1;
  }
  /* element 0's packets straight into the render kernel (iamf_hip_batch_render_packets_ragged: no unpacked copy, no unpack
   * launch): when asking is worth it is the single handle's question too */
  g->lp_ok = lp_worth_asking(d0, g->lay, "IAMF_HIP_GROUP_UNPACK"); /* (two elements: both rows, iamf_hip_batch_render_packets_mix_ragged) */
  for (int k = 0; k < 3; ++k)
    if (!(g->cgain[k] = (float *)calloc(n, sizeof(float)))) return 1;
  /* upload chunks: at most eight per round, at least eight handles each (an upload call costs ~4 us of host time) */
  g->chunk = (g->n + 7) / 8 < 8 ? 8 : (g->n + 7) / 8;
  g->nchunks = (g->n + g->chunk - 1) / g->chunk;
  if (!(g->chunk_done = (int *)calloc((size_t)g->nchunks, sizeof(int)))) return 1;
  for (int k = 0; k < 3; ++k)
    if (hipMalloc((void **)&g->d_ramp[k], sizeof(float) * n * g->fs) != hipSuccess) return 1;
  if (hipMalloc((void **)&g->d_dmx, sizeof(iamf_hip_dmx_frame) * n) != hipSuccess ||
      hipMalloc((void **)&g->d_demix, sizeof(iamf_hip_demix_frame) * n) != hipSuccess)
    return 1;
  for (int sl = 0; sl < 2; ++sl) {
    for (int k = 0; k < 3; ++k)
      if (hipHostMalloc((void **)&g->slot[sl].h_ramp[k], sizeof(float) * n * g->fs, 0) != hipSuccess) return 1;
    if (hipHostMalloc((void **)&g->slot[sl].h_dmx, sizeof(iamf_hip_dmx_frame) * n, 0) != hipSuccess ||
        hipHostMalloc((void **)&g->slot[sl].h_demix, sizeof(iamf_hip_demix_frame) * n, 0) != hipSuccess)
      return 1;
  }
  /* one call emits at most one frame (or the 240-sample tail) per stream */
  g->pcm_cap = (size_t)g->bytes * ((size_t)(g->fs > 240 ? g->fs : 240) * d0->pcm_stride + d0->pcm_extra);
  if (g->rs) { /* a frame through the resampler, or its tail + the limiter's */
    const size_t a = (size_t)iamf_hip_resampler_out_capacity(g->rs, g->fs), b = (size_t)iamf_hip_resampler_flush_capacity(g->rs) + 240;
    g->pcm_cap = (size_t)g->bytes * ((a > b ? a : b) * d0->pcm_stride + d0->pcm_extra);
  }
  g->pcm_cap = (g->pcm_cap + 255) & ~(size_t)255;
  for (int sl = 0; sl < 2; ++sl)
    if (hipHostMalloc((void **)&g->slot[sl].h_pcm, g->pcm_cap * n, 0) != hipSuccess) return 1;
  if (hipHostMalloc((void **)&g->h_sig, 64, 0) != hipSuccess) return 1;
  *g->h_sig = 0;
  group_use_slot(g, 0);
  for (int i = 0; i < g->n; ++i) {
    struct IAMF_Decoder *d = (struct IAMF_Decoder *)handles[i];
    g->d[i] = d;
    d->group = g;
    for (int e = 0; e < g->nel; ++e) /* decode_parse copies a packet straight into its slot of the handle's row */
      for (int s2 = 0; s2 < g->walk[e]->nsub; ++s2) {
        d->pkt_ext[e][s2] = g->h_raw[e] + (size_t)i * g->raw_stride[e] + g->slot_off[e][s2];
        d->pkt_ext_cap[e][s2] = (uint32_t)(g->walk[e]->width[s2] * ((int)d->sample_size / 8) * g->fs);
        d->pkt_in_ext[e][s2] = 0;
      }
  }
  return 0;
}

/* host threads: 0 = as many as the process may run on (its CPU quota less two), at most 16 and at most one per 4 handles */
static int group_start_threads(iamf_hip_decoder_group *g, int host_threads) {
  int nt = host_threads;
  if (nt <= 0) {
    long c = sysconf(_SC_NPROCESSORS_ONLN);
    FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r"); /* a container's CPU quota: workers that poll beyond it get the whole group throttled */
    if (f) {
      long q = 0, per = 0;
      if (fscanf(f, "%ld %ld", &q, &per) == 2 && q > 0 && per > 0 && q / per < c) c = q / per;
      fclose(f);
    }
    c -= 2; /* the calling thread and the HIP runtime's own */
    nt = c > 16 ? 16 : (c < 1 ? 1 : (int)c);
  }
  if (nt > (g->n + 3) / 4) nt = (g->n + 3) / 4;
  g->nthreads = nt - 1; /* the calling thread is one of them */
  if (g->nthreads <= 0) return 0;
  pthread_mutex_init(&g->mu, 0);
  pthread_cond_init(&g->cv_work, 0);
  pthread_cond_init(&g->cv_done, 0);
  g->threads = (pthread_t *)calloc((size_t)g->nthreads, sizeof(pthread_t));
  if (!g->threads) return 1;
  for (int t = 0; t < g->nthreads; ++t)
    if (pthread_create(&g->threads[t], 0, group_worker, g)) {
      g->nthreads = t;
      return 1;
    }
  return 0;
}

int iamf_hip_decoder_group_create(void *const *handles, int n, int host_threads, iamf_hip_decoder_group **out) {
  iamf_hip_decoder_group *g;
  int rc;
  if (!handles || n <= 0 || !out) return IAMF_ERR_BAD_ARG;
  *out = 0;
  if ((rc = group_validate(handles, n))) return rc;
  g = (iamf_hip_decoder_group *)calloc(1, sizeof(*g));
  if (!g) return IAMF_ERR_ALLOC_FAIL;
  g->n = n;
  rc = group_alloc_host(g, (const struct IAMF_Decoder *)handles[0]);
  if (!rc && (group_create_stages(g, handles) || group_alloc_staging(g, handles) || group_start_threads(g, host_threads)))
    rc = IAMF_ERR_INTERNAL;
  if (rc) {
    iamf_hip_decoder_group_destroy(g);
    return rc;
  }
  *out = g;
  return IAMF_OK;
}

/* The host half of a temporal unit for handle i — render_tu's, up to its launches, over the same pieces (ftu_trim_window,
 * dropped_unit_advance, frame_gain_plan, pre_frame): packets, trim, this frame's gains and parameter records go to the
 * group's staging rows.  Returns 1 if the stream has a frame to render (g->keep / g->s0 / g->rampf set), 2 if only the LFE
 * generator's filter runs, else the value IAMF_decoder_decode returns for this call (0 or an error). */
static int group_prepare_tu(iamf_hip_decoder_group *g, int i) {
  struct IAMF_Decoder *d = g->d[i];
  const int fs = g->fs;
  ftu_window w;
  int ns = 0, rc, ramp[3];
  float cgain[3], set[2];
  float *row[3] = {g->h_ramp[0] + (size_t)i * fs, g->h_ramp[1] + (size_t)i * fs, g->h_ramp[2] + (size_t)i * fs};
  for (int e = 0; e < d->sel->nel; ++e) {
    int r = group_stage_raw(g, i, e);
    if (r < 0) return r;
    ns = r;
  }
  for (int e = 0; e < d->sel->nel; ++e)
    for (int s = 0; s < d->sel_el[e]->nsub; ++s) d->pkt_have[e][s] = 0;
  rc = ftu_trim_window(ns, d->tu_trim_start, d->tu_trim_end, fs, &w);
  if (rc < 0) {
    d->timestamp += fs;
    return IAMF_ERR_BAD_ARG;
  }
  if (rc == FTU_DROPPED) { /* nothing is emitted, but the reference has decoded and (mostly) rendered the unit */
    iamf_hip_dmx_frame *fr[2] = {&g->h_dmx[i], g->aux ? &g->h_dmx1[i] : 0};
    iamf_hip_demix_frame *dm[2] = {&g->h_demix[i], g->aux ? &g->h_demix1[i] : 0};
    const int rendered = dropped_unit_advance(d, w.rendered, fr, dm);
    d->timestamp += fs;
    if (!rendered || !(g->lfe[0] || g->lfe[1])) return 0;
    for (int e = 0; e < d->sel->nel; ++e) { /* the generator's filter runs over the whole frame: unpacked whole, no render */
      int32_t *head = (int32_t *)(g->h_raw[e] + (size_t)i * g->raw_stride[e]);
      head[0] = 0;
      head[1] = g->lfe[e] ? ns : 0;
    }
    g->keep[i] = 0;
    g->s0[i] = 0;
    g->te[i] = ns;
    return 2;
  }
  meta_note_frame(d, w.s0, d->tu_trim_end);
  for (int e = 0; e < d->sel->nel; ++e) { /* iamf_frame_trim: the device unpacker starts at the first kept sample */
    int32_t *head = (int32_t *)(g->h_raw[e] + (size_t)i * g->raw_stride[e]);
    /* ... except for an element that feeds the LFE generator, whose filter runs over the whole frame (ftu_element_stage_args) */
    head[0] = g->lfe[e] ? 0 : w.s0;
    head[1] = g->lfe[e] ? ns : w.keep;
  }
  /* A constant gain travels as a row only if some handle of the round is on a ramp in that stage: the row is written once
   * all are parsed (group_upload_params) from g->cgain; element 1's row is always written (frame_gain_plan) */
  frame_gain_plan(d, w.s0, w.keep, row, ramp, cgain, set);
  g->rampf[i] = ramp[0] | ramp[1] << 1 | ramp[2] << 2; /* bit k = stage k is a per-sample ramp in this frame */
  for (int k = 0; k < 3; ++k) g->cgain[k][i] = cgain[k];
  g->gain_new[i] = set[0];
  g->gain_new[g->n + i] = set[1];
  for (int k = 0; k < d->sel->nel; ++k) { /* in the order the reference renders its streams (dmx_shared_coefficients) */
    const int e = d->sel->swapped ? d->sel->nel - 1 - k : k;
    if (e == 0) pre_frame(d, 0, &g->h_dmx[i], &g->h_demix[i]);
    else if (g->aux) pre_frame(d, 1, &g->h_dmx1[i], &g->h_demix1[i]);
  }
  g->keep[i] = w.keep;
  g->s0[i] = w.s0;
  g->te[i] = w.te;
  return 1;
}


/* the end of IAMF_decoder_decode for handle i: its PCM (the clocks have moved at submit, group_advance_clocks) */
static void group_copy_out_one(iamf_hip_decoder_group *g, int i) {
  const struct IAMF_Decoder *d = g->d[i];
  if (g->action[i] == GA_NONE || g->action[i] == GA_ADVANCE) return; /* (a unit trimmed away: IAMF_decoder_decode returned 0) */
  if (g->result[i] > 0)
    memcpy(g->pcm_out[i], g->h_pcm + g->pcm_cap * (size_t)i, ((size_t)g->result[i] * d->pcm_stride + d->pcm_extra) * g->bytes);
}

/* The rest of the end of IAMF_decoder_decode: the parameter clocks (IAMF_decoder.c:3471), the stream time, the metadata
 * of the output.  Every value is known once the round's launches are queued (g->result is the count a launch returned on
 * the host), so this runs at the end of the submit: the next round's parse (group_prepare_tu reads d->timestamp and the
 * parameter queues) must see it, and it may start before this round's PCM is back. */
static void group_advance_clocks(iamf_hip_decoder_group *g) {
  for (int i = 0; i < g->n; ++i) {
    struct IAMF_Decoder *d = g->d[i];
    if (g->action[i] == GA_NONE || g->action[i] == GA_ADVANCE) continue;
    if (g->action[i] == GA_RENDER) {
      params_time_elapse(d, (uint64_t)g->keep[i]); /* the mixed frame's length */
      d->timestamp += g->fs;
    }
    meta_note_output(d, g->result[i]); /* a rendered unit or the flushed tail: IAMF_decoder.c:3521-3522 */
  }
}

/* IAMF_decoder_decode's parsing half for handle i (IAMF_decoder.c:2871-2995): sets g->action[i]; returns the call's
 * result if it is already known (no frame this time, an error), else 0 */
static int group_parse_one(iamf_hip_decoder_group *g, int i) {
  struct IAMF_Decoder *d = g->d[i];
  const uint8_t *data = g->data[i];
  const int32_t size = g->sizes[i];
  uint32_t *rsize = g->rsizes ? &g->rsizes[i] : 0;
  int ready = 0, rc;
  g->action[i] = GA_NONE;
  /* decode_parse writes packets straight into this round's slot of the handle's row.  A temporal unit whose sub-stream
   * packets arrived over earlier calls has them in the slot of the handle's last submit (which a round in flight may
   * still upload from: it is only read here): they move along into this slot's row */
  for (int e = 0; e < g->nel; ++e)
    for (int s2 = 0; s2 < g->walk[e]->nsub; ++s2) {
      uint8_t *mine = g->h_raw[e] + (size_t)i * g->raw_stride[e] + g->slot_off[e][s2];
      if (d->pkt_ext[e][s2] == mine) continue;
      if (d->pkt_in_ext[e][s2] && d->pkt_have[e][s2]) memcpy(mine, d->pkt_ext[e][s2], d->pkt_len[e][s2]);
      d->pkt_ext[e][s2] = mine;
    }
  for (int e = 0; e < g->nel; ++e) ((int32_t *)(g->h_raw[e] + (size_t)i * g->raw_stride[e]))[1] = 0; /* nothing to unpack yet */
  if (rsize) *rsize = 0;
  if (!d->configured || d->need_reconf) return IAMF_ERR_INVALID_STATE;
  if (!data || size <= 0) {
    if (d->flushed) return 0;
    d->flushed = 1;
    if (!d->limiter_on && !g->rs) return 0;
    g->action[i] = GA_FLUSH;
    return 0;
  }
  rc = decode_parse(d, data, size, rsize, &ready);
  if (rc || !ready) return rc;
  rc = group_prepare_tu(g, i);
  if (rc == 2) {
    g->action[i] = GA_ADVANCE;
    return 0;
  }
  if (rc != 1) return rc;
  g->action[i] = GA_RENDER;
  return 0;
}

/* Round `ticket`'s host half: parse, stage into slot ticket & 1, queue the device work, move the clocks.  Every device
 * call of a round goes to g->stream; the batch and the resampler take what a launch needs by value (the kernels'
 * parameter structs) or from device buffers they advance in stream order (iamf_render.hip: p.fir_hist / fir_cur,
 * d_lim, d_lfe_state; iamf_resample.hip: d_hist[cur], whose host-side phase walk is the only host state), so a launch
 * reads no host memory after it returns — which a round already relied on: it queues several range launches with no
 * synchronisation between them.  What they read from the host is the group's pinned staging (h_raw through
 * iamf_hip_upload_by_kernel, h_ramp / h_dmx / h_demix through hipMemcpyAsync), and that has a copy per slot.  The
 * exceptions synchronise themselves: iamf_hip_batch_set_gains waits for the batch's last render (quiesce) — in a round
 * whose constant gains change it therefore waits for the round before it, a bubble in the pipeline — and a buffer that
 * grows with the largest call seen is replaced after a hipStreamSynchronize. */
/* ---- group_submit_round's steps.  Each returns nonzero if a device call failed (the caller: group_fail) ---- */

/* Parse, packet staging, parameter timelines: per handle, on the pool.  The calling thread uploads each chunk of rows
 * as soon as the pool has completed it, so the PCIe time of chunk c lies beside the parsing of chunk c + 1 (256
 * handles: 0.21 ms of host work and 0.17 ms of upload per round, one after the other before); it takes handles itself
 * only when there is no pool.  The upload is a KERNEL that reads the pinned rows over PCIe (iamf_hip_upload_by_kernel):
 * everything of a round stays on the compute queue.  Measured on the GPU box (tools/debug/copy_latency_probe.hip):
 * a pinned hipMemcpyAsync costs 8-9 us per call on top of its bytes, a copy -> kernel -> copy sequence 22-26 us for the
 * hand-overs between the copy engine and the compute queue, and a kernel reads pinned memory as fast as the engine
 * copies it (8 MB + a kernel + the download: 172 us against 187).  For the same reason the render kernel writes its
 * PCM straight into the pinned buffer the handles are served from: no download. */
static int group_upload_chunks(iamf_hip_decoder_group *g) {
  int dev_err = 0;
  group_start(g, 0);
  if (g->nthreads <= 0) group_help(g);
  for (int c = 0; c < g->nchunks; ++c) {
    const int c0 = c * g->chunk, cn = c0 + g->chunk <= g->n ? g->chunk : g->n - c0;
    int wanted = 0;
    for (int spin = 0; __atomic_load_n(&g->chunk_done[c], __ATOMIC_ACQUIRE) < cn; ++spin) {
      if (spin < kGroupSpin) group_relax(); else sched_yield();
    }
    for (int i = c0; i < c0 + cn; ++i) wanted |= g->action[i] == GA_RENDER || g->action[i] == GA_ADVANCE;
    if (!wanted || dev_err) continue;
    for (int e = 0; e < g->nel && !dev_err; ++e) {
      const size_t off = (size_t)c0 * g->raw_stride[e];
      if (iamf_hip_upload_by_kernel(g->h_raw[e] + off, (uint8_t *)g->d_raw[e] + off, g->raw_stride[e] * (size_t)cn, g->stream)) dev_err = 1;
    }
  }
  group_join(g);
  return dev_err;
}

/* what the round's render launches read beside the packets: ramp rows, stage records, constant gains */
static int group_upload_params(iamf_hip_decoder_group *g, int gains_changed) {
  const struct IAMF_Decoder *d0 = g->d[0];
  const size_t n = (size_t)g->n;
  /* a stage that is on a ramp in SOME stream is applied through its rows in all: the others' rows carry their constant */
  for (int k = 0; k < 3; ++k)
    if ((g->rampu >> k) & 1 && !(k == 1 && g->nel > 1))
      for (int i = 0; i < g->n; ++i)
        if (g->action[i] == GA_RENDER && !((g->rampf[i] >> k) & 1)) {
          float *row = g->h_ramp[k] + (size_t)i * g->fs;
          const float c = g->cgain[k][i];
          for (int j = 0; j < g->keep[i]; ++j) row[j] = c;
        }
  if (g->nel > 1) g->rampu |= 2; /* element 1 takes its gain through its ramp row, constant or not */
  for (int k = 0; k < 3; ++k)
    if ((g->rampu >> k) & 1 &&
        hipMemcpyAsync(g->d_ramp[k], g->h_ramp[k], sizeof(float) * n * g->fs, hipMemcpyHostToDevice, g->stream) != hipSuccess)
      return 1;
  if (d0->pre[0].use_dmx && hipMemcpyAsync(g->d_dmx, g->h_dmx, sizeof(iamf_hip_dmx_frame) * n, hipMemcpyHostToDevice, g->stream) != hipSuccess)
    return 1;
  if (d0->pre[0].use_demix && hipMemcpyAsync(g->d_demix, g->h_demix, sizeof(iamf_hip_demix_frame) * n, hipMemcpyHostToDevice, g->stream) != hipSuccess)
    return 1;
  if (g->aux && d0->pre[1].use_dmx && hipMemcpyAsync(g->d_dmx1, g->h_dmx1, sizeof(iamf_hip_dmx_frame) * n, hipMemcpyHostToDevice, g->stream) != hipSuccess)
    return 1;
  if (g->aux && d0->pre[1].use_demix && hipMemcpyAsync(g->d_demix1, g->h_demix1, sizeof(iamf_hip_demix_frame) * n, hipMemcpyHostToDevice, g->stream) != hipSuccess)
    return 1;
  if (gains_changed) { /* constant gains of the streams that are not on a ramp this time (synchronous, rare) */
    if (iamf_hip_batch_set_gains(g->batch, g->gain_new, g->gain_new + n, 0)) return 1;
    memcpy(g->gain_cur, g->gain_new, sizeof(float) * 2 * n);
  }
  return 0;
}

/* The device unpacker over every row, once per round and only if a launch reads its output (it is skipped when every
 * launch reads the packets itself).  (Rows of chunks that had nothing to render were not uploaded: the device still holds
 * their previous round's, and the unpacker may rewrite element PCM that no launch of this round reads) */
static int group_unpack_once(iamf_hip_decoder_group *g) {
  for (int e = 0; e < g->nel && !g->unpacked; ++e)
    if (iamf_hip_lpcm_unpack(&g->lay[e], g->d_raw[e], (int64_t)g->raw_stride[e], (const int32_t *)g->d_raw[e],
                             (int64_t)(g->raw_stride[e] / 4), g->d_in[e], (int64_t)g->in_ch[e] * g->fs, g->n, g->stream))
      return 1;
  g->unpacked = 1;
  return 0;
}

/* the launchers, one per kind of run: streams [i, j) do the same thing from the same position */

/* the LFE generator's filter over frames that are trimmed away completely (te = their length) */
static int group_run_advance(iamf_hip_decoder_group *g, int i, int j) {
  if (group_unpack_once(g)) return 1;
  if (g->aux && g->lfe[1] && iamf_hip_batch_lfe_advance(g->aux, g->d_in[1], (int64_t)g->in_ch[1] * g->fs, g->te[i], g->stream, i, j - i))
    return 1;
  if (g->lfe[0] && iamf_hip_batch_lfe_advance(g->batch, g->d_in[0], (int64_t)g->in_ch[0] * g->fs, g->te[i], g->stream, i, j - i))
    return 1;
  for (int s = i; s < j; ++s) g->result[s] = 0;
  return 0;
}

static int group_run_flush(iamf_hip_decoder_group *g, int i, int j) {
  const int r = iamf_hip_batch_flush_range(g->batch, g->h_pcm, (int64_t)g->pcm_cap, g->stream, i, j - i);
  for (int s = i; s < j && r >= 0; ++s) {
    g->result[s] = r;
    g->pos[s] += 240;
  }
  return r < 0;
}

/* n2 sample-frames per stream of the run behind the resampler through the last stage; returns what it emits */
static int group_last_stage(iamf_hip_decoder_group *g, int i, int j, int n2) {
  iamf_hip_render_args a3;
  if (n2 <= 0) return 0;
  ftu_last_stage_args(&a3, g->d_res, g->res_stride, g->out_ch, n2, g->h_pcm, (int64_t)g->pcm_cap, g->stream);
  return render_last_stage(g->batch3, &a3, i, j - i); /* (iamf_hip_batch_render_interleaved where the device layer has it) */
}

/* iamf_delay_buffer_handle, IAMF_decoder.c:3250-3301: the resampler's tail + the limiter's (flush_tail) */
static int group_run_flush_resampled(iamf_hip_decoder_group *g, int i, int j) {
  const int extra = g->limiter_on ? 240 : 0;
  int n2, r;
  if (hipMemsetAsync(g->d_res + (size_t)i * g->res_stride, 0, sizeof(float) * (size_t)(j - i) * g->res_stride, g->stream) != hipSuccess)
    return 1;
  n2 = iamf_hip_resampler_flush_range(g->rs, g->d_res, g->res_stride, g->stream, i, j - i);
  if (n2 < 0) return 1;
  if (g->d[i]->norm_loudness != 0.f) { /* the resampler's tail is not normalised (flush_tail; IAMF_decoder.c:3271-3287) */
    for (int s = i; s < j; ++s) g->loud3[s] = 1.f;
    if (iamf_hip_batch_set_gains(g->batch3, 0, 0, g->loud3)) return 1;
  }
  r = group_last_stage(g, i, j, n2 + extra);
  for (int s = i; s < j && r >= 0; ++s) {
    g->result[s] = r;
    g->pos3[s] += n2 + extra;
  }
  return r < 0;
}

/* behind the run's render call, which returned r: with a resampler the two stages behind it (d_mid -> d_res -> PCM), and the
 * run's results and positions */
static int group_run_behind(iamf_hip_decoder_group *g, int i, int j, int r) {
  if (r < 0) return 1;
  if (g->rs) {
    const int n2 = iamf_hip_resampler_process_range(g->rs, g->d_mid, g->mid_stride, r, g->d_res, g->res_stride, g->stream, i, j - i);
    if (n2 < 0 || (r = group_last_stage(g, i, j, n2)) < 0) return 1;
    for (int s = i; s < j; ++s) g->pos3[s] += n2;
  }
  for (int s = i; s < j; ++s) {
    g->result[s] = r;
    g->pos[s] += g->keep[s];
  }
  return 0;
}

/* the run's packets straight into the render kernel: first kept sample s0, keep samples (uniform over the run).  A first stage
 * (a resampler behind, or the limiter off: lp_worth_asking) asks the packet-fed limiter-less renderer, into d_mid where the
 * resampler follows */
static int group_run_lpcm(iamf_hip_decoder_group *g, int i, int j) {
  iamf_hip_packet_call c; /* (the entries are total: any number of kept samples, render_launch of the single handle) */
  memset(&c, 0, sizeof(c));
  c.in.d_raw = g->d_raw[0];
  c.in.raw_stream_stride = c.in.raw_frame_stride = (int64_t)g->raw_stride[0];
  c.in.first_sample = g->s0[i];
  c.in.layout = g->lay[0];
  ftu_element_stage_args(&c.args, 0, 0, g->fs, 0, g->s0[i], g->te[i], g->keep[i], 0, 0, g->stream);
  c.args.d_pcm = g->rs ? (void *)g->d_mid : (void *)g->h_pcm;
  c.args.pcm_stream_stride_bytes = g->rs ? (int64_t)sizeof(float) * g->mid_stride : (int64_t)g->pcm_cap;
  return group_run_behind(g, i, j, g->rs || !g->limiter_on ? render_packets_first_stage(g->batch, &c, i, j - i)
                                                           : render_packets_any_length(g->batch, &c, i, j - i));
}

/* a two-element run's packets, both elements', straight into the render kernel (lp_worth_asking has seen the entry: no batch
 * of its own for element 1).  Element 1 takes its gain through its ramp row, constant or not, as in group_run_f32; the other two
 * stages through theirs where the round applies them so (rampu).  A first stage (a resampler behind, or the limiter off:
 * lp_worth_asking, which has seen that entry too) asks iamf_hip_batch_render_packets_mix_nolim */
static int group_run_lpcm_mix(iamf_hip_decoder_group *g, int i, int j) {
  iamf_hip_packet_mix_call c;
  memset(&c, 0, sizeof(c));
  for (int e = 0; e < 2; ++e) {
    c.in[e].d_raw = g->d_raw[e];
    c.in[e].raw_stream_stride = c.in[e].raw_frame_stride = (int64_t)g->raw_stride[e];
    c.in[e].first_sample = g->s0[i];
    c.in[e].layout = g->lay[e];
  }
  ftu_element_stage_args(&c.args, 0, 0, g->fs, 0, g->s0[i], g->te[i], g->keep[i], 0, 0, g->stream);
  c.args.d_element2_ramp = g->d_ramp[1];
  if (g->rampu & 1) c.args.d_element_ramp = g->d_ramp[0];
  if (g->rampu & 4) c.args.d_output_ramp = g->d_ramp[2];
  c.args.ramp_stream_stride = g->fs;
  c.args.d_pcm = g->rs ? (void *)g->d_mid : (void *)g->h_pcm;
  c.args.pcm_stream_stride_bytes = g->rs ? (int64_t)sizeof(float) * g->mid_stride : (int64_t)g->pcm_cap;
  /* (a first stage asks the two-element form of the limiter-less renderer, into d_mid where the resampler follows) */
  return group_run_behind(g, i, j, g->rs || !g->limiter_on ? iamf_hip_batch_render_packets_mix_nolim(g->batch, &c, i, j - i)
                                                           : iamf_hip_batch_render_packets_mix_ragged(g->batch, &c, i, j - i));
}

/* the run from unpacked f32: element 1 through its own batch first (stage, matrix, its gain row -> planar f32), the render
 * batch, and behind a resampler render (f32) -> resample -> loudness / limiter / pack — render_tu's launches, as ranges */
static int group_run_f32(iamf_hip_decoder_group *g, int i, int j) {
  const struct IAMF_Decoder *d0 = g->d[0];
  const int fs = g->fs, s0 = g->s0[i], te = g->te[i], keep = g->keep[i];
  iamf_hip_render_args a;
  if (group_unpack_once(g)) return 1;
  ftu_element_stage_args(&a, g->d_in[0], g->in_ch[0], fs, g->lfe[0], s0, te, keep, d0->pre[0].use_dmx ? g->d_dmx : 0,
                         d0->pre[0].use_demix ? g->d_demix : 0, g->stream);
  if (g->aux) {
    iamf_hip_render_args b;
    const int64_t st = (int64_t)fs * g->out_ch;
    ftu_element_stage_args(&b, g->d_in[1], g->in_ch[1], fs, g->lfe[1], s0, te, keep, d0->pre[1].use_dmx ? g->d_dmx1 : 0,
                           d0->pre[1].use_demix ? g->d_demix1 : 0, g->stream);
    b.d_element_ramp = g->d_ramp[1];
    b.ramp_stream_stride = fs;
    b.d_pcm = g->d_aux_il;
    b.pcm_stream_stride_bytes = (int64_t)sizeof(float) * st;
    if (iamf_hip_batch_render_range(g->aux, &b, i, j - i) != keep) return 1;
    if (iamf_hip_deinterleave_f32(g->d_aux_il + (int64_t)i * st, st, g->out_ch, j - i, keep, g->d_aux_pl + (int64_t)i * st, st, fs, g->stream))
      return 1;
    a.d_in2 = g->d_aux_pl;
    a.in2_stream_stride = a.in2_frame_stride = st;
    a.d_element2_ramp = g->d_ones;
  } else if (g->nel > 1) {
    a.d_in2 = g->d_in[1];
    a.in2_stream_stride = a.in2_frame_stride = (int64_t)g->in_ch[1] * fs;
    a.d_element2_ramp = g->d_ramp[1];
  }
  if (g->rampu & 1) a.d_element_ramp = g->d_ramp[0];
  if (g->rampu & 4) a.d_output_ramp = g->d_ramp[2];
  a.ramp_stream_stride = fs;
  a.d_pcm = g->rs ? (void *)g->d_mid : (void *)g->h_pcm;
  a.pcm_stream_stride_bytes = g->rs ? (int64_t)sizeof(float) * g->mid_stride : (int64_t)g->pcm_cap;
  return group_run_behind(g, i, j, iamf_hip_batch_render_range(g->batch, &a, i, j - i));
}

/* the end of the run that starts at stream i: neighbouring streams that do the same thing from the same position */
static int group_run_end(const iamf_hip_decoder_group *g, int i) {
  int j = i + 1;
  while (j < g->n && g->action[j] == g->action[i] && g->pos[j] == g->pos[i] &&
         (g->action[i] == GA_FLUSH || (g->keep[j] == g->keep[i] && g->s0[j] == g->s0[i] &&
                                       (!(g->lfe[0] || g->lfe[1]) || g->te[j] == g->te[i]))) &&
         /* resampling: one launch = one phase of the resampler and one position of the last stage */
         (!g->rs || (g->pos3[j] == g->pos3[i] && iamf_hip_resampler_same_state(g->rs, i, j))))
    ++j;
  while (g->action[i] == GA_ADVANCE && j < g->n && g->action[j] == GA_ADVANCE && g->te[j] == g->te[i]) ++j;
  return j;
}

/* Round `ticket`'s host half: parse, stage into slot ticket & 1, queue the device work, move the clocks.  Every device
 * call of a round goes to g->stream; the batch and the resampler take what a launch needs by value (the kernels'
 * parameter structs) or from device buffers they advance in stream order (iamf_render.hip: p.fir_hist / fir_cur,
 * d_lim, d_lfe_state; iamf_resample.hip: d_hist[cur], whose host-side phase walk is the only host state), so a launch
 * reads no host memory after it returns — which a round already relied on: it queues several range launches with no
 * synchronisation between them.  What they read from the host is the group's pinned staging (h_raw through
 * iamf_hip_upload_by_kernel, h_ramp / h_dmx / h_demix through hipMemcpyAsync), and that has a copy per slot.  The
 * exceptions synchronise themselves: iamf_hip_batch_set_gains waits for the batch's last render (quiesce) — in a round
 * whose constant gains change it therefore waits for the round before it, a bubble in the pipeline — and a buffer that
 * grows with the largest call seen is replaced after a hipStreamSynchronize. */
static int group_submit_round(iamf_hip_decoder_group *g, const uint8_t *const *data, const int32_t *sizes, uint32_t *rsizes,
                              void *const *pcm, int32_t *results) {
  int any_render = 0, any = 0, gains_changed = 0;
  const int n = g->n;
  const int sl = (int)((g->issued + 1) & 1);
  double t0 = group_now(), t1;
  group_use_slot(g, sl);
  memcpy(g->pcm_out, pcm, sizeof(void *) * (size_t)n);
  g->slot[sl].dev = 0;
  g->data = data;
  g->sizes = sizes;
  g->rsizes = rsizes;
  g->rampu = g->unpacked = 0;
  const int dev_err = group_upload_chunks(g);
  t1 = group_now();
  g->t_phase[0] += t1 - t0;
  t0 = t1;
  ++g->rounds;
  if (dev_err) return group_fail(g);
  for (int i = 0; i < n; ++i) {
    results[i] = g->result[i];
    if (g->action[i] == GA_RENDER) {
      any_render = 1;
      g->rampu |= g->rampf[i];
      if (g->gain_new[i] != g->gain_cur[i] || g->gain_new[n + i] != g->gain_cur[n + i]) gains_changed = 1;
    } else { /* not rendered: its constant gains stay what they are */
      g->gain_new[i] = g->gain_cur[i];
      g->gain_new[n + i] = g->gain_cur[n + i];
    }
    any |= g->action[i] != GA_NONE;
  }
  if (!any) {
    g->t_phase[1] += group_now() - t0;
    return IAMF_OK;
  }
  if (any_render && group_upload_params(g, gains_changed)) return group_fail(g);
  for (int i = 0, j; i < n; i = j) { /* launches: maximal runs */
    if (g->action[i] == GA_NONE) {
      j = i + 1;
      continue;
    }
    j = group_run_end(g, i);
    if (g->action[i] == GA_ADVANCE ? group_run_advance(g, i, j)
        : g->action[i] == GA_FLUSH ? (g->rs ? group_run_flush_resampled(g, i, j) : group_run_flush(g, i, j))
        : g->lp_ok && g->nel > 1 && !(g->s0[i] & 3) ? group_run_lpcm_mix(g, i, j) /* (the mix forms take ramps) */
        : g->lp_ok && !g->rampu && !(g->s0[i] & 3) ? group_run_lpcm(g, i, j)
                                                                         : group_run_f32(g, i, j))
      return group_fail(g);
  }
  /* the round is queued: a one-lane kernel behind its last launch writes the ticket into the pinned word (what _complete
   * and _poll wait for: this round only, not the one submitted after it) */
  if (iamf_hip_stream_signal(g->stream, g->h_sig, (uint32_t)(g->issued + 1)) != IAMF_HIP_OK) return group_fail(g);
  g->slot[sl].dev = 1;
  group_advance_clocks(g);
  for (int i = 0; i < n; ++i)
    if (g->action[i] != GA_NONE) results[i] = g->result[i];
  g->t_phase[1] += group_now() - t0;
  return IAMF_OK;
}


int iamf_hip_decoder_group_submit(iamf_hip_decoder_group *g, const uint8_t *const *data, const int32_t *sizes,
                                  uint32_t *rsizes, void *const *pcm, int32_t *results, uint64_t *ticket) {
  int rc;
  if (!g || !data || !sizes || !pcm || !results || !ticket) return IAMF_ERR_BAD_ARG;
  for (int i = 0; i < g->n; ++i)
    if (!pcm[i]) return IAMF_ERR_BAD_ARG;
  if (g->failed || g->issued - g->done >= IAMF_HIP_GROUP_MAX_IN_FLIGHT) return IAMF_ERR_INVALID_STATE;
  rc = group_submit_round(g, data, sizes, rsizes, pcm, results);
  if (rc) return rc;
  *ticket = ++g->issued;
  return IAMF_OK;
}

/* the round's device work has completed: the signal word has reached its ticket (an acquire load: the PCM the kernels
 * wrote before the signal is visible once it reads so) */
static int group_round_done(const iamf_hip_decoder_group *g, uint64_t ticket) {
  return !g->slot[ticket & 1].dev || (int32_t)(__atomic_load_n(g->h_sig, __ATOMIC_ACQUIRE) - (uint32_t)ticket) >= 0;
}
enum { kGroupWaitUs = 100000 }; /* spin on the signal word at most this long, then hipStreamSynchronize */

int iamf_hip_decoder_group_poll(iamf_hip_decoder_group *g, uint64_t ticket) {
  if (!g) return IAMF_ERR_BAD_ARG;
  if (g->failed || ticket <= g->done || ticket > g->issued) return IAMF_ERR_INVALID_STATE;
  return group_round_done(g, ticket);
}

int iamf_hip_decoder_group_complete(iamf_hip_decoder_group *g, uint64_t ticket) {
  double t0, t1;
  if (!g) return IAMF_ERR_BAD_ARG;
  if (g->failed || ticket != g->done + 1 || ticket > g->issued) return IAMF_ERR_INVALID_STATE;
  t0 = group_now();
  if (!group_round_done(g, ticket)) {
    /* a bounded spin; a round that takes longer (or a device that has failed: the signal never comes) ends in
     * hipStreamSynchronize, which also waits for the round after it and reports a device error */
    for (int spin = 0; !group_round_done(g, ticket); ++spin) {
      if (spin < kGroupSpin) {
        group_relax();
      } else {
        if (group_now() - t0 > 1e-6 * kGroupWaitUs) {
          if (hipStreamSynchronize(g->stream) != hipSuccess) return group_fail(g);
          break;
        }
        sched_yield();
      }
    }
  }
  t1 = group_now();
  g->t_phase[2] += t1 - t0;
  /* every handle's share of the pinned PCM to its caller's buffer: on the pool */
  group_use_slot(g, (int)(ticket & 1));
  group_start(g, 1);
  group_help(g);
  group_join(g);
  g->done = ticket;
  g->t_phase[3] += group_now() - t1;
  return IAMF_OK;
}

int iamf_hip_decoder_group_decode(iamf_hip_decoder_group *g, const uint8_t *const *data, const int32_t *sizes,
                                  uint32_t *rsizes, void *const *pcm, int32_t *results) {
  uint64_t ticket = 0;
  int rc;
  if (!g || !data || !sizes || !pcm || !results) return IAMF_ERR_BAD_ARG;
  if (g->issued != g->done) return IAMF_ERR_INVALID_STATE; /* rounds outstanding: complete them first */
  rc = iamf_hip_decoder_group_submit(g, data, sizes, rsizes, pcm, results, &ticket);
  if (rc) return rc;
  return iamf_hip_decoder_group_complete(g, ticket);
}
