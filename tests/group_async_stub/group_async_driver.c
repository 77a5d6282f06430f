/* TEST INFRASTRUCTURE: drives iamf_hip_decoder_group over one .iamf file with N handles, built with sanitizers against
 * the deferred device stand-ins (async_stub.c), either through iamf_hip_decoder_group_decode ("sync") or with two rounds
 * always in flight through _submit / _complete ("pipe").  Handles are out of step: handle i is starved (one byte, no
 * complete OBU) in round r when (r + i) % 3 == 0, and a handle flushes once it has eaten its stream.  With a block size,
 * handle i gets a window of block + 97 * i bytes a round, widened by that much while it holds no complete OBU (the
 * player's block loop: the sub-stream packets of a temporal unit arrive over several calls).
 * Prints one digest per handle (its PCM bytes and return values); tests/test_group_async_cpu.py compares the two modes.
 * In "pipe" mode every round's data is a private copy that is overwritten with garbage as soon as _submit returns, and
 * the pcm buffers of an outstanding round hold a sentinel that only its _complete may change.
 * usage: group_async_driver file.iamf <sound system id | b> bits N threads sync|pipe block */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "IAMF_decoder.h"
#include "iamf_hip.h"

long stub_async_stats(void);
void stub_async_shutdown(void);

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
  for (size_t k = 0; k < n; ++k) h = (h ^ ((const uint8_t *)p)[k]) * 0x100000001b3ull;
  return h;
}

int main(int argc, char **argv) {
  if (argc < 8) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *buf = (uint8_t *)malloc(size ? size : 1);
  if (fread(buf, 1, size, f) != (size_t)size) return 2;
  fclose(f);
  const int bits = atoi(argv[3]), N = atoi(argv[4]), threads = atoi(argv[5]), pipe = !strcmp(argv[6], "pipe"), block = atoi(argv[7]);
  int ch = 2;
  void **h = (void **)calloc(N, sizeof(void *));
  uint32_t *used = (uint32_t *)calloc(N, sizeof(uint32_t)), *rs = (uint32_t *)calloc(N, sizeof(uint32_t));
  uint64_t *dig = (uint64_t *)calloc(N, sizeof(uint64_t));
  long *total = (long *)calloc(N, sizeof(long));
  int *done = (int *)calloc(N, sizeof(int)), *win = (int *)calloc(N, sizeof(int));
  size_t pcm_bytes = 0;
  void **pcm[2];
  uint8_t **copy[2];
  const uint8_t **data = (const uint8_t **)calloc(N, sizeof(uint8_t *));
  int32_t *sizes = (int32_t *)calloc(N, sizeof(int32_t)), *res[2];
  int32_t *sz[2];
  for (int i = 0; i < N; ++i) {
    IAMF_DecoderHandle d = IAMF_decoder_open();
    h[i] = d;
    IAMF_decoder_set_bit_depth(d, bits);
    if (argv[2][0] == 'b') {
      IAMF_decoder_output_layout_set_binaural(d);
    } else {
      IAMF_decoder_output_layout_set_sound_system(d, (IAMF_SoundSystem)atoi(argv[2]));
      ch = IAMF_layout_sound_system_channels_count((IAMF_SoundSystem)atoi(argv[2]));
    }
    uint32_t r0 = 0;
    if (IAMF_decoder_configure(d, buf, (uint32_t)size, &r0) != IAMF_OK) {
      printf("configure failed\n");
      return 3;
    }
    used[i] = r0;
    win[i] = block + 97 * i;
    dig[i] = 0xcbf29ce484222325ull;
    const size_t b = (size_t)(bits / 8) * IAMF_decoder_get_stream_info(d)->max_frame_size * 24;
    if (b > pcm_bytes) pcm_bytes = b;
  }
  for (int k = 0; k < 2; ++k) {
    pcm[k] = (void **)calloc(N, sizeof(void *));
    copy[k] = (uint8_t **)calloc(N, sizeof(uint8_t *));
    res[k] = (int32_t *)calloc(N, sizeof(int32_t));
    sz[k] = (int32_t *)calloc(N, sizeof(int32_t));
    for (int i = 0; i < N; ++i) {
      pcm[k][i] = malloc(pcm_bytes);
      copy[k][i] = (uint8_t *)malloc((size_t)size + 1);
    }
  }
  iamf_hip_decoder_group *g = 0;
  int rc = iamf_hip_decoder_group_create(h, N, threads, &g);
  if (rc) {
    printf("group_create %d\n", rc);
    return 3;
  }
  int left = N, violations = 0, errors = 0;
  uint64_t tickets[2] = {0, 0};
  int outstanding = 0; /* rounds in flight (pipe) */
  long rounds = 0;
  /* round r uses pcm / res / copy set r & 1; its results are final at submit, its PCM at complete */
  for (int round = 0; (left > 0 || outstanding) && round < 100000; ++round) {
    const int k = round & 1;
    if (left > 0) {
      for (int i = 0; i < N; ++i) {
        sz[k][i] = 0;
        if (done[i]) {
          data[i] = buf;
          sizes[i] = 1;
        } else if (used[i] >= (uint32_t)size) {
          data[i] = 0;
          sizes[i] = 0;
        } else if ((round + i) % 3 == 0) {
          data[i] = buf + used[i];
          sizes[i] = 1;
        } else {
          int32_t w = (int32_t)(size - used[i]);
          if (block > 0 && w > win[i]) w = win[i];
          if (w > 98304) w = 98304; /* (a few temporal units: bounds the copies below) */
          data[i] = buf + used[i];
          sizes[i] = w;
        }
        sz[k][i] = sizes[i];
        if (pipe && data[i]) { /* a private copy, garbage once submitted */
          memcpy(copy[k][i], data[i], (size_t)sizes[i]);
          data[i] = copy[k][i];
        }
        memset(pcm[k][i], 0xA5, pcm_bytes);
      }
      if (pipe) {
        uint64_t t = 0;
        rc = iamf_hip_decoder_group_submit(g, data, sizes, rs, pcm[k], res[k], &t);
        if (rc) {
          printf("submit %d\n", rc);
          errors++;
          break;
        }
        for (int i = 0; i < N; ++i)
          if (data[i]) memset(copy[k][i], 0x5A ^ (round & 0xff), (size_t)sizes[i]);
        tickets[k] = t;
        ++outstanding;
      } else {
        rc = iamf_hip_decoder_group_decode(g, data, sizes, rs, pcm[k], res[k]);
        if (rc) {
          printf("decode %d\n", rc);
          errors++;
          break;
        }
      }
      ++rounds;
      /* the next round's data from this round's rsizes (final at submit) */
      for (int i = 0; i < N; ++i) {
        if (done[i]) continue;
        if (!sz[k][i] && used[i] >= (uint32_t)size) {
          done[i] = 1;
          --left;
          continue;
        }
        if (sz[k][i] == 1) continue;
        used[i] += rs[i];
        if (block > 0 && !rs[i] && sz[k][i] < (int32_t)(size - used[i])) { /* no complete OBU in the window: widen it */
          win[i] += block + 97 * i;
          continue;
        }
        win[i] = block + 97 * i;
        if (!rs[i] || res[k][i] == IAMF_ERR_INVALID_STATE) used[i] = (uint32_t)size;
      }
    }
    /* complete: in pipe mode the older round once two are out (or at the end), the only one in sync mode */
    int kc = -1;
    if (pipe && (outstanding == 2 || (left == 0 && outstanding > 0))) {
      /* the oldest outstanding round: of two the lower ticket, of one the round submitted last */
      kc = outstanding == 2 ? (tickets[0] < tickets[1] ? 0 : 1) : (tickets[0] > tickets[1] ? 0 : 1);
      rc = iamf_hip_decoder_group_complete(g, tickets[kc]);
      if (rc) {
        printf("complete %d\n", rc);
        errors++;
        break;
      }
      --outstanding;
      if (outstanding == 1) { /* the other round is still out: its pcm buffers must still hold the sentinel */
        for (int i = 0; i < N; ++i)
          for (size_t b = 0; b < pcm_bytes; ++b)
            if (((uint8_t *)pcm[kc ^ 1][i])[b] != 0xA5) {
              ++violations;
              break;
            }
      }
    } else if (!pipe) {
      kc = k;
    }
    if (kc >= 0)
      for (int i = 0; i < N; ++i) {
        dig[i] = fnv(dig[i], &res[kc][i], 4);
        if (res[kc][i] > 0) {
          const size_t nb = (size_t)res[kc][i] * ch * (bits / 8);
          dig[i] = fnv(dig[i], pcm[kc][i], nb);
          total[i] += res[kc][i];
        }
      }
    if (!pipe && left == 0) break;
  }
  printf("rounds %ld errors %d sentinel_violations %d late_drained %ld\n", rounds, errors, violations, stub_async_stats());
  for (int i = 0; i < N; ++i) printf("h%d total %ld digest %016llx\n", i, total[i], (unsigned long long)dig[i]);
  {
    double sec[4];
    int64_t nr = 0;
    iamf_hip_decoder_group_times(g, sec, &nr);
    printf("times_rounds %lld\n", (long long)nr);
  }
  iamf_hip_decoder_group_destroy(g);
  for (int i = 0; i < N; ++i) IAMF_decoder_close((IAMF_DecoderHandle)h[i]);
  stub_async_shutdown();
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i < N; ++i) {
      free(pcm[k][i]);
      free(copy[k][i]);
    }
    free(pcm[k]);
    free(copy[k]);
    free(res[k]);
    free(sz[k]);
  }
  free(h); free(used); free(rs); free(dig); free(total); free(done); free(win); free(data); free(sizes); free(buf);
  return 0;
}
