/*
 * TEST INFRASTRUCTURE — not a CPU path of the product.
 *
 * Device stand-ins whose work is DEFERRED, for the pipelined decoder group (iamf_hip_decoder_group_submit / _complete):
 * copies, iamf_hip_upload_by_kernel, the unpacker, the render / flush / resampler / LFE calls and iamf_hip_stream_signal
 * are queued per stream and run in stream order later — at hipStreamSynchronize, at a synchronous call that waits for
 * them as the runtime's does (hipMemcpy, hipFree, iamf_hip_batch_set_gains waits for its batch's last render), or on a
 * background thread once they are due: an operation is due a random 1-3 ms after it was queued, or as soon as the
 * next round has been queued behind it (two signals at or after it), so the work of a round with a successor runs only
 * after the host has parsed and staged that successor.  A host buffer that the facade rewrites before the work that reads it has run
 * therefore changes the output: the render stand-in writes PCM that is a hash of everything the stream has read so far
 * (its input rows, ramp rows, gains, packets).
 *
 * The layout / matrix / down-mix helpers and the batch bookkeeping come from tests/facade_stub/device_stub.c, included
 * below with the deferred entry points renamed out of the way.
 *
 * stub_async_stats(): how many queued operations a hipStreamSynchronize ran that lie behind a signal it also ran (the work
 * of a later round drained by a wait for an earlier one — what a wait with stream semantics would do).
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include "iamf_hip.h"

#define hipMemcpyAsync sync_hipMemcpyAsync
#define hipMemcpy sync_hipMemcpy
#define hipMemset sync_hipMemset
#define hipMemsetAsync sync_hipMemsetAsync
#define hipFree sync_hipFree
#define hipHostFree sync_hipHostFree
#define hipStreamCreate sync_hipStreamCreate
#define hipStreamDestroy sync_hipStreamDestroy
#define hipStreamSynchronize sync_hipStreamSynchronize
#define iamf_hip_batch_create sync_batch_create
#define iamf_hip_batch_destroy sync_batch_destroy
#define iamf_hip_batch_set_gains sync_batch_set_gains
#define iamf_hip_batch_lfe_advance sync_batch_lfe_advance
#define iamf_hip_batch_render sync_batch_render
#define iamf_hip_batch_render_range sync_batch_render_range
#define iamf_hip_batch_render_ex sync_batch_render_ex
#define iamf_hip_batch_flush_range sync_batch_flush_range
#define iamf_hip_batch_flush sync_batch_flush
#define iamf_hip_deinterleave_f32 sync_deinterleave_f32
#define iamf_hip_stream_signal sync_stream_signal
#define iamf_hip_upload_by_kernel sync_upload_by_kernel
#define iamf_hip_lpcm_unpack sync_lpcm_unpack
#define iamf_hip_batch_render_lpcm_range sync_batch_render_lpcm_range
#define iamf_hip_batch_render_lpcm sync_batch_render_lpcm
#define iamf_hip_resampler_process sync_resampler_process
#define iamf_hip_resampler_flush sync_resampler_flush
#define iamf_hip_resampler_process_range sync_resampler_process_range
#define iamf_hip_resampler_flush_range sync_resampler_flush_range
#include "../facade_stub/device_stub.c"
#undef hipMemcpyAsync
#undef hipMemcpy
#undef hipMemset
#undef hipMemsetAsync
#undef hipFree
#undef hipHostFree
#undef hipStreamCreate
#undef hipStreamDestroy
#undef hipStreamSynchronize
#undef iamf_hip_batch_create
#undef iamf_hip_batch_destroy
#undef iamf_hip_batch_set_gains
#undef iamf_hip_batch_lfe_advance
#undef iamf_hip_batch_render
#undef iamf_hip_batch_render_range
#undef iamf_hip_batch_render_ex
#undef iamf_hip_batch_flush_range
#undef iamf_hip_batch_flush
#undef iamf_hip_deinterleave_f32
#undef iamf_hip_stream_signal
#undef iamf_hip_upload_by_kernel
#undef iamf_hip_lpcm_unpack
#undef iamf_hip_batch_render_lpcm_range
#undef iamf_hip_batch_render_lpcm
#undef iamf_hip_resampler_process
#undef iamf_hip_resampler_flush
#undef iamf_hip_resampler_process_range
#undef iamf_hip_resampler_flush_range

/* ---- the queue ---- */
enum { OP_COPY, OP_SET, OP_UNPACK, OP_RENDER, OP_LPCM, OP_FLUSH, OP_LFE, OP_DEINT, OP_RESAMPLE, OP_SIGNAL };
typedef struct Op {
  int kind;
  struct Op *next;
  iamf_hip_batch *b;
  void *dst;
  const void *src;
  size_t bytes;
  int value;
  iamf_hip_render_args a;
  iamf_hip_lpcm_input in;
  iamf_hip_lpcm_layout lay;
  int64_t i64[4];
  int32_t s0, cnt;
  double due; /* the background thread runs it from then on */
  int64_t need[]; /* OP_RENDER / OP_LPCM / OP_FLUSH: PCM bytes per stream of the range */
} Op;
typedef struct Queue {
  Op *head, *tail;
  struct Queue *next_q;
} Queue;

static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
static Queue *queues;
static pthread_t worker;
static int worker_on, worker_stop;
static long late_drained;
static unsigned seed = 12345;

static double now_s(void) {
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

/* per batch: its gains as the device holds them, and one running hash per stream (what the "kernels" have read) */
typedef struct Dev {
  iamf_hip_batch *b;
  int ns;
  float *gains;
  uint64_t *h;
  struct Dev *next;
} Dev;
static Dev *devs;
static Dev *dev_of(iamf_hip_batch *b) {
  for (Dev *d = devs; d; d = d->next)
    if (d->b == b) return d;
  abort();
}

static uint64_t mix(uint64_t h, uint64_t v) {
  h ^= v + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  return h * 0xff51afd7ed558ccdull;
}
static uint64_t mix_f(uint64_t h, float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return mix(h, u);
}

static void write_pcm(Dev *d, int s, uint8_t *p, int64_t need) {
  uint64_t h = d->h[s];
  for (int64_t k = 0; k < need; ++k) {
    if (!(k & 7)) h = mix(h, (uint64_t)k);
    p[k] = (uint8_t)(h >> ((k & 7) * 8));
  }
  d->h[s] = h;
}

static void run_op(Op *o) {
  switch (o->kind) {
    case OP_COPY: memcpy(o->dst, o->src, o->bytes); break;
    case OP_SET: memset(o->dst, o->value, o->bytes); break;
    case OP_UNPACK: sync_lpcm_unpack(&o->lay, o->src, o->i64[0], (const int32_t *)o->src, o->i64[1], (float *)o->dst, o->i64[2], o->cnt, 0); break;
    case OP_DEINT:
      sync_deinterleave_f32((const float *)o->src, o->i64[0], o->value, o->cnt, (int32_t)o->i64[1], (float *)o->dst, o->i64[2], o->i64[3], 0);
      break;
    case OP_RESAMPLE: { /* out row = a function of the in row */
      const float *in = (const float *)o->src;
      float *out = (float *)o->dst;
      const int64_t iss = o->i64[0], oss = o->i64[1], nin = o->i64[2], nout = o->i64[3];
      for (int s = o->s0; s < o->s0 + o->cnt; ++s)
        for (int64_t k = 0; k < nout; ++k) out[s * oss + k] = in[s * iss + (nin ? k % nin : 0)] * 0.5f + (float)(k & 15);
      break;
    }
    case OP_SIGNAL: __atomic_store_n((volatile uint32_t *)o->dst, (uint32_t)o->value, __ATOMIC_RELEASE); break;
    case OP_LFE: {
      Dev *d = dev_of(o->b);
      for (int s = o->s0; s < o->s0 + o->cnt; ++s)
        for (int i = 0; i < o->value; ++i) d->h[s] = mix_f(d->h[s], ((const float *)o->src)[s * o->i64[0] + i]);
      break;
    }
    case OP_RENDER:
    case OP_LPCM:
    case OP_FLUSH: {
      Dev *d = dev_of(o->b);
      const iamf_hip_render_args *a = &o->a;
      const int n = (int)o->i64[0], m = o->b->cfg.matrix.m, ns = d->ns;
      for (int s = o->s0; s < o->s0 + o->cnt; ++s) {
        uint64_t h = d->h[s];
        h = mix_f(mix_f(mix_f(h, d->gains[s]), d->gains[ns + s]), d->gains[2 * ns + s]);
        if (o->kind == OP_RENDER) {
          if (a->d_in && o->b->cfg.matrix.kind != IAMF_HIP_KIND_DMX)
            for (int64_t i = 0; i < (int64_t)m * n; ++i) h = mix_f(h, a->d_in[s * a->in_stream_stride + i]);
          for (int i = 0; i < n; ++i) {
            if (a->d_element_ramp) h = mix_f(h, a->d_element_ramp[s * a->ramp_stream_stride + i]);
            if (a->d_output_ramp) h = mix_f(h, a->d_output_ramp[s * a->ramp_stream_stride + i]);
            if (a->d_element2_ramp) h = mix_f(h, a->d_element2_ramp[s * a->ramp_stream_stride + i]);
          }
          if (a->d_in2)
            for (int c = 0; c < o->b->m2; ++c)
              for (int i = 0; i < n; ++i) h = mix_f(h, a->d_in2[s * a->in2_stream_stride + (int64_t)c * o->b->cfg.frame_size + i]);
          if (a->d_dmx_frames) {
            h = mix(h, (uint64_t)a->d_dmx_frames[s].offset);
            for (int k = 0; k < 5; ++k) h = mix_f(mix_f(h, a->d_dmx_frames[s].prev[k]), a->d_dmx_frames[s].cur[k]);
          }
          if (a->d_demix_frames) h = mix(h, (uint64_t)a->d_demix_frames[s].n_recon);
        } else if (o->kind == OP_LPCM) {
          const iamf_hip_lpcm_input *in = &o->in;
          for (int c = 0; c < in->layout.channels; ++c)
            for (int i = 0; i < n && in->layout.src_offset[c] >= 0; ++i) {
              const uint8_t *p = (const uint8_t *)in->d_raw + (int64_t)s * in->raw_stream_stride + in->layout.src_offset[c] +
                                 (int64_t)(in->first_sample + i) * in->layout.src_step[c];
              for (int k = 0; k < in->layout.sample_bytes; ++k) h = mix(h, p[k]);
            }
        }
        d->h[s] = h;
        write_pcm(d, s, (uint8_t *)o->dst + (int64_t)s * o->i64[1], o->need[s - o->s0]);
      }
      break;
    }
  }
}

/* with the lock held */
static void drain(Queue *q, Op *upto) {
  int seen_signal = 0;
  while (q->head) {
    Op *o = q->head;
    q->head = o->next;
    if (!q->head) q->tail = 0;
    if (seen_signal && o->kind != OP_SIGNAL) ++late_drained;
    if (o->kind == OP_SIGNAL) seen_signal = 1;
    run_op(o);
    const int last = o == upto;
    free(o);
    if (last) break;
  }
}
static void drain_all(void) {
  for (Queue *q = queues; q; q = q->next_q)
    while (q->head) {
      Op *o = q->head;
      q->head = o->next;
      if (!q->head) q->tail = 0;
      run_op(o);
      free(o);
    }
}

static void *worker_main(void *arg) {
  (void)arg;
  for (;;) {
    struct timespec t = {0, 50000};
    nanosleep(&t, 0);
    pthread_mutex_lock(&mu);
    if (worker_stop) {
      pthread_mutex_unlock(&mu);
      return 0;
    }
    const double now = now_s();
    for (Queue *q = queues; q; q = q->next_q) {
      int signals = 0;
      for (Op *o = q->head; o && signals < 2; o = o->next) signals += o->kind == OP_SIGNAL;
      while (q->head && (q->head->due <= now || signals >= 2)) {
        signals -= q->head->kind == OP_SIGNAL;
        Op *o = q->head;
        q->head = o->next;
        if (!q->head) q->tail = 0;
        run_op(o);
        free(o);
      }
    }
    pthread_mutex_unlock(&mu);
  }
}

static Op *op_new(int kind, size_t extra) {
  Op *o = (Op *)calloc(1, sizeof(Op) + extra);
  if (!o) abort();
  o->kind = kind;
  return o;
}
static void push(hipStream_t st, Op *o) {
  Queue *q = (Queue *)st;
  pthread_mutex_lock(&mu);
  o->due = now_s() + 1e-6 * (double)(1000 + rand_r(&seed) % 2000);
  if (!q) { /* the null stream: run now, behind everything */
    drain_all();
    run_op(o);
    free(o);
  } else {
    if (q->tail) q->tail->next = o;
    else q->head = o;
    q->tail = o;
  }
  pthread_mutex_unlock(&mu);
}

/* ---- the runtime ---- */
hipError_t hipStreamCreate(hipStream_t *s) {
  Queue *q = (Queue *)calloc(1, sizeof(Queue));
  pthread_mutex_lock(&mu);
  q->next_q = queues;
  queues = q;
  if (!worker_on && !getenv("STUB_NO_WORKER")) {
    worker_on = 1;
    pthread_create(&worker, 0, worker_main, 0);
  }
  pthread_mutex_unlock(&mu);
  *s = (hipStream_t)q;
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  pthread_mutex_lock(&mu);
  drain((Queue *)s, 0);
  for (Queue **p = &queues; *p; p = &(*p)->next_q)
    if (*p == (Queue *)s) {
      *p = ((Queue *)s)->next_q;
      break;
    }
  pthread_mutex_unlock(&mu);
  free(s);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
  pthread_mutex_lock(&mu);
  if (s) drain((Queue *)s, 0);
  else drain_all();
  pthread_mutex_unlock(&mu);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st) {
  (void)k;
  Op *o = op_new(OP_COPY, 0);
  o->dst = d;
  o->src = s;
  o->bytes = n;
  push(st, o);
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st) {
  Op *o = op_new(OP_SET, 0);
  o->dst = d;
  o->value = v;
  o->bytes = n;
  push(st, o);
  return hipSuccess;
}
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k) { return hipMemcpyAsync(d, s, n, k, 0); }
hipError_t hipMemset(void *d, int v, size_t n) { return hipMemsetAsync(d, v, n, 0); }
hipError_t hipFree(void *p) {
  pthread_mutex_lock(&mu);
  drain_all();
  pthread_mutex_unlock(&mu);
  free(p);
  return hipSuccess;
}
hipError_t hipHostFree(void *p) { return hipFree(p); }

int iamf_hip_upload_by_kernel(const void *h, void *d, size_t n, void *st) {
  if (!h || !d || !n || (n & 15)) return IAMF_HIP_ERR_BAD_ARG;
  return hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, (hipStream_t)st) == hipSuccess ? IAMF_HIP_OK : IAMF_HIP_ERR_DEVICE;
}
int iamf_hip_stream_signal(void *st, volatile uint32_t *flag, uint32_t seq) {
  Op *o = op_new(OP_SIGNAL, 0);
  o->dst = (void *)flag;
  o->value = (int)seq;
  push((hipStream_t)st, o);
  return IAMF_HIP_OK;
}
int iamf_hip_lpcm_unpack(const iamf_hip_lpcm_layout *lay, const void *d_raw, int64_t raw_stride, const int32_t *fc, int64_t fcs,
                         float *out, int64_t out_stride, int32_t n, void *st) {
  if (!lay || !d_raw || !fc || !out || n <= 0 || lay->channels <= 0 || lay->channels > IAMF_HIP_LPCM_MAX_CHANNELS) return IAMF_HIP_ERR_BAD_ARG;
  if ((const void *)fc != d_raw) return IAMF_HIP_ERR_BAD_ARG; /* the group keeps the frame counts in the rows' heads */
  Op *o = op_new(OP_UNPACK, 0);
  o->lay = *lay;
  o->src = d_raw;
  o->i64[0] = raw_stride;
  o->i64[1] = fcs;
  o->i64[2] = out_stride;
  o->dst = out;
  o->cnt = n;
  push((hipStream_t)st, o);
  return IAMF_HIP_OK;
}
int iamf_hip_deinterleave_f32(const float *src, int64_t sss, int32_t ch, int32_t ns, int32_t n, float *dst, int64_t dss, int64_t dcs,
                              void *st) {
  if (!src || !dst || ch <= 0 || ch > 24 || ns <= 0 || n < 0 || dcs < n) return IAMF_HIP_ERR_BAD_ARG;
  Op *o = op_new(OP_DEINT, 0);
  o->src = src;
  o->dst = dst;
  o->value = ch;
  o->cnt = ns;
  o->i64[0] = sss;
  o->i64[1] = n;
  o->i64[2] = dss;
  o->i64[3] = dcs;
  push((hipStream_t)st, o);
  return IAMF_HIP_OK;
}

/* ---- the batch ---- */
int iamf_hip_batch_create(const iamf_hip_batch_config *c, iamf_hip_batch **out) {
  int rc = sync_batch_create(c, out);
  if (rc) return rc;
  Dev *d = (Dev *)calloc(1, sizeof(Dev));
  d->b = *out;
  d->ns = c->n_streams;
  d->gains = (float *)malloc(sizeof(float) * 3 * (size_t)c->n_streams);
  d->h = (uint64_t *)calloc((size_t)c->n_streams, sizeof(uint64_t));
  for (int k = 0; k < 3 * c->n_streams; ++k) d->gains[k] = 1.f;
  pthread_mutex_lock(&mu);
  d->next = devs;
  devs = d;
  pthread_mutex_unlock(&mu);
  return 0;
}
void iamf_hip_batch_destroy(iamf_hip_batch *b) {
  if (!b) return;
  pthread_mutex_lock(&mu);
  drain_all();
  for (Dev **p = &devs; *p; p = &(*p)->next)
    if ((*p)->b == b) {
      Dev *d = *p;
      *p = d->next;
      free(d->gains);
      free(d->h);
      free(d);
      break;
    }
  pthread_mutex_unlock(&mu);
  sync_batch_destroy(b);
}
/* as the library's: waits for the batch's last queued render (quiesce), then writes the gains the next one reads */
int iamf_hip_batch_set_gains(iamf_hip_batch *b, const float *eg, const float *og, const float *lg) {
  pthread_mutex_lock(&mu);
  for (Queue *q = queues; q; q = q->next_q) {
    Op *last = 0;
    for (Op *o = q->head; o; o = o->next)
      if (o->b == b) last = o;
    if (last) drain(q, last);
  }
  Dev *d = dev_of(b);
  if (eg) memcpy(d->gains, eg, sizeof(float) * d->ns);
  if (og) memcpy(d->gains + d->ns, og, sizeof(float) * d->ns);
  if (lg) memcpy(d->gains + 2 * d->ns, lg, sizeof(float) * d->ns);
  pthread_mutex_unlock(&mu);
  return 0;
}
/* the host half of a launch: the counts the batch returns (the limiter's withheld samples are host bookkeeping) */
static int count_range(iamf_hip_batch *b, int kind, int s0, int cnt, int n, void *pcm, int64_t cap, void *st,
                       const iamf_hip_render_args *a, const iamf_hip_lpcm_input *in) {
  if (s0 < 0 || cnt <= 0 || s0 + cnt > b->cfg.n_streams) return IAMF_HIP_ERR_BAD_ARG;
  Op *o = op_new(kind, sizeof(int64_t) * (size_t)cnt);
  int r = 0;
  const int sc = b->cfg.pcm_stride_channels > 0 ? b->cfg.pcm_stride_channels : b->cfg.out_channels;
  for (int s = s0; s < s0 + cnt; ++s) {
    int m = n;
    if (kind == OP_FLUSH) {
      m = b->cfg.limiter_enable ? 240 - b->pad_left[s] : 0;
      b->pad_left[s] = 0;
    } else {
      const int skip = m < b->pad_left[s] ? m : b->pad_left[s];
      b->pad_left[s] -= skip;
      m -= skip;
    }
    const int64_t need = ((int64_t)m * sc + (m > 0 && b->cfg.out_channels > sc ? b->cfg.out_channels - sc : 0)) *
                         iamf_hip_format_bytes(b->cfg.out_format);
    if (need > cap) {
      free(o);
      return IAMF_HIP_ERR_BAD_ARG;
    }
    o->need[s - s0] = need;
    r = m;
  }
  o->b = b;
  o->s0 = s0;
  o->cnt = cnt;
  o->dst = pcm;
  o->i64[0] = n;
  o->i64[1] = cap;
  if (a) o->a = *a;
  if (in) o->in = *in;
  push((hipStream_t)st, o);
  return r;
}
int iamf_hip_batch_render_range(iamf_hip_batch *b, const iamf_hip_render_args *a, int32_t s0, int32_t cnt) {
  const int n = a->n_samples ? a->n_samples : a->n_frames * b->cfg.frame_size;
  return count_range(b, OP_RENDER, s0, cnt, n, a->d_pcm, a->pcm_stream_stride_bytes, a->stream, a, 0);
}
int iamf_hip_batch_render_ex(iamf_hip_batch *b, const iamf_hip_render_args *a) {
  return iamf_hip_batch_render_range(b, a, 0, b->cfg.n_streams);
}
int iamf_hip_batch_render(iamf_hip_batch *b, const float *in, int64_t ss, int64_t fs, int32_t nf, void *pcm, int64_t cap, void *st) {
  iamf_hip_render_args a;
  memset(&a, 0, sizeof(a));
  a.d_in = in;
  a.in_stream_stride = ss;
  a.in_frame_stride = fs;
  a.n_frames = nf;
  a.d_pcm = pcm;
  a.pcm_stream_stride_bytes = cap;
  a.stream = st;
  return iamf_hip_batch_render_ex(b, &a);
}
int iamf_hip_batch_render_lpcm_range(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *a, int32_t s0,
                                     int32_t cnt) {
  const int n = a->n_samples ? a->n_samples : a->n_frames * b->cfg.frame_size;
  if (!in || !in->d_raw || a->d_in || a->n_frames != 1 || in->first_sample < 0 || in->first_sample + n > b->cfg.frame_size)
    return IAMF_HIP_ERR_BAD_ARG;
  return count_range(b, OP_LPCM, s0, cnt, n, a->d_pcm, a->pcm_stream_stride_bytes, a->stream, a, in);
}
int iamf_hip_batch_render_lpcm(iamf_hip_batch *b, const iamf_hip_lpcm_input *in, const iamf_hip_render_args *a) {
  return iamf_hip_batch_render_lpcm_range(b, in, a, 0, b->cfg.n_streams);
}
int iamf_hip_batch_flush_range(iamf_hip_batch *b, void *pcm, int64_t cap, void *st, int32_t s0, int32_t cnt) {
  return count_range(b, OP_FLUSH, s0, cnt, 0, pcm, cap, st, 0, 0);
}
int iamf_hip_batch_flush(iamf_hip_batch *b, void *pcm, int64_t cap, void *st) {
  return iamf_hip_batch_flush_range(b, pcm, cap, st, 0, b->cfg.n_streams);
}
int iamf_hip_batch_lfe_advance(iamf_hip_batch *b, const float *in, int64_t ss, int32_t n, void *st, int32_t s0, int32_t cnt) {
  if (!b || !in || n <= 0 || n > b->cfg.frame_size || s0 < 0 || cnt <= 0 || s0 + cnt > b->cfg.n_streams) return IAMF_HIP_ERR_BAD_ARG;
  Op *o = op_new(OP_LFE, 0);
  o->b = b;
  o->src = in;
  o->i64[0] = ss;
  o->value = n;
  o->s0 = s0;
  o->cnt = cnt;
  push((hipStream_t)st, o);
  return IAMF_HIP_OK;
}

/* ---- the resampler: counts on the host, rows on the "device" ---- */
int iamf_hip_resampler_process_range(iamf_hip_resampler *r, const float *in, int64_t iss, int n, float *out, int64_t oss, void *st,
                                     int32_t s0, int32_t cnt) {
  const int m = (int)((int64_t)n * r->out / r->in);
  if ((int64_t)m * r->ch > oss) return IAMF_HIP_ERR_BAD_ARG;
  Op *o = op_new(OP_RESAMPLE, 0);
  o->src = in;
  o->dst = out;
  o->i64[0] = iss;
  o->i64[1] = oss;
  o->i64[2] = (int64_t)n * r->ch;
  o->i64[3] = (int64_t)m * r->ch;
  o->s0 = s0;
  o->cnt = cnt;
  push((hipStream_t)st, o);
  return m;
}
int iamf_hip_resampler_process(iamf_hip_resampler *r, const float *in, int64_t iss, int n, float *out, int64_t oss, void *st) {
  return iamf_hip_resampler_process_range(r, in, iss, n, out, oss, st, 0, 1);
}
int iamf_hip_resampler_flush_range(iamf_hip_resampler *r, float *out, int64_t oss, void *st, int32_t s0, int32_t cnt) {
  (void)r; (void)out; (void)oss; (void)st; (void)s0; (void)cnt;
  return 0;
}
int iamf_hip_resampler_flush(iamf_hip_resampler *r, float *out, int64_t oss, void *st) { return iamf_hip_resampler_flush_range(r, out, oss, st, 0, 1); }

/* for the driver: stop the background thread; queued operations that lay behind a signal a stream wait also ran */
long stub_async_stats(void) {
  pthread_mutex_lock(&mu);
  const long v = late_drained;
  pthread_mutex_unlock(&mu);
  return v;
}
void stub_async_shutdown(void) {
  pthread_mutex_lock(&mu);
  worker_stop = 1;
  const int on = worker_on;
  pthread_mutex_unlock(&mu);
  if (on) pthread_join(worker, 0);
}
