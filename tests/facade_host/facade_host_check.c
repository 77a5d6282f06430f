/* TEST INFRASTRUCTURE: iac_amd/csrc/facade_tu.h — the pieces of one temporal unit that the decoder facade's single handle
 * and its decoder group share — compiled alone with the host compiler (and the sanitizers) and checked against values
 * written out by hand.  tests/test_facade_host.py builds and runs it. */
#include <stdio.h>

#include "facade_tu.h"

static int cases, wrong;
#define CHECK(what, cond)                                     \
  do {                                                        \
    ++cases;                                                  \
    if (!(cond)) {                                            \
      ++wrong;                                                \
      printf("WRONG %s:%d %s: %s\n", __FILE__, __LINE__, what, #cond); \
    }                                                         \
  } while (0)

static int same_ints(const int *a, const int *b, int n) {
  for (int i = 0; i < n; ++i)
    if (a[i] != b[i]) return 0;
  return 1;
}

/* audio-layer channel of playback channel p, as the facade's k_al_of_pl holds it for 7.1.4 (IAMF_utils.c:117-133 vs :181-196) */
static const int k_al_of_pl_714[12] = {0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9};

static void trim_window(void) {
  ftu_window w;
  const uint64_t acc[4][2] = {{0, 0}, {1024, 0}, {0, 1024}, {512, 512}};
  for (int i = 0; i < 4; ++i) {
    const int rc = ftu_trim_window(1024, acc[i][0], acc[i][1], 1024, &w);
    CHECK("trim accepted", rc == (i == 0 ? FTU_OK : FTU_DROPPED));
    CHECK("trim window", w.s0 == (int)acc[i][0] && w.te == (int)acc[i][1] && w.keep == (i == 0 ? 1024 : 0));
  }
  /* a dropped unit was rendered by the reference unless one trim alone covers the frame */
  CHECK("rendered (512, 512)", ftu_trim_window(1024, 512, 512, 1024, &w) == FTU_DROPPED && w.rendered == 1);
  CHECK("rendered (1024, 0)", ftu_trim_window(1024, 1024, 0, 1024, &w) == FTU_DROPPED && w.rendered == 0);
  CHECK("rendered (0, 1024)", ftu_trim_window(1024, 0, 1024, 1024, &w) == FTU_DROPPED && w.rendered == 0);
  CHECK("trim (513, 512)", ftu_trim_window(1024, 513, 512, 1024, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("trim (2^64 - 1, 2): no wrapped sum", ftu_trim_window(1024, UINT64_MAX, 2, 1024, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("trim (2, 2^64 - 1)", ftu_trim_window(1024, 2, UINT64_MAX, 1024, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("trim (0, 1025)", ftu_trim_window(1024, 0, 1025, 1024, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("short last frame", ftu_trim_window(300, 4, 40, 1024, &w) == FTU_OK && w.s0 == 4 && w.keep == 256 && w.te == 40);
}

static void substream_walk(void) {
  ftu_walk w;
  iamf_hip_lpcm_layout L;
  int slot[FTU_MAX_SUBSTREAMS];
  uint8_t map[16];
  for (int c = 0; c < 16; ++c) map[c] = (uint8_t)c;
  { /* 16 mono ambisonics sub-streams */
    int ok = ftu_walk_substreams(FTU_SCENE_BASED, 16, 0, 0, 0, 0, 0, 0, &w) == 0 && w.nsub == 16 && w.channels == 16;
    for (int s = 0; s < 16; ++s) ok = ok && w.width[s] == 1 && w.first[s] == s;
    for (int p = 0; p < 16; ++p) ok = ok && ftu_channel_source(FTU_SCENE_BASED, p, 0, map, w.channels) == p;
    CHECK("16 mono ambisonics sub-streams", ok);
    /* their raw row, 16 bit, 64 samples a frame, no head: sub-stream s at s * 128 */
    ok = ftu_raw_layout(&w, 0, FTU_SCENE_BASED, 16, 0, map, 2, 1, 64, 0, slot, &L) == 16 * 128 && L.channels == 16 && L.sample_bytes == 2 &&
         L.frame_size == 64 && L.little_endian == 1;
    for (int p = 0; p < 16; ++p) ok = ok && slot[p] == p * 128 && L.src_offset[p] == p * 128 && L.src_step[p] == 2;
    CHECK("16 mono ambisonics sub-streams: raw row", ok);
  }
  { /* projection: 2 coupled + 2 single sub-streams -> 6 decoded channels, handed on in decoded order */
    const int width[4] = {2, 2, 1, 1}, first[4] = {0, 2, 4, 5};
    const int off[6] = {16, 19, 16 + 384, 19 + 384, 16 + 768, 16 + 960}, step[6] = {6, 6, 6, 6, 3, 3};
    int ok = ftu_walk_substreams(FTU_SCENE_BASED, 4, 0, 1, 2, 0, 0, 0, &w) == 0 && w.nsub == 4 && w.channels == 6;
    CHECK("projection 2 + 2", ok && same_ints(w.width, width, 4) && same_ints(w.first, first, 4));
    /* 24 bit, 64 samples, a 16-byte head: a pair takes 384 bytes, a single 192 */
    ok = ftu_raw_layout(&w, 1, FTU_SCENE_BASED, 4, 0, map, 3, 0, 64, 16, slot, &L) == 16 + 2 * 384 + 2 * 192 && L.channels == 6;
    CHECK("projection 2 + 2: raw row", ok && slot[0] == 16 && slot[1] == 400 && slot[2] == 784 && slot[3] == 976 &&
                                           same_ints(L.src_offset, off, 6) && same_ints(L.src_step, step, 6) && L.little_endian == 0);
    /* without projection mode the same numbers couple nothing */
    CHECK("mono mapping ignores amb_coupled", ftu_walk_substreams(FTU_SCENE_BASED, 4, 0, 0, 2, 0, 0, 0, &w) == 0 && w.channels == 4);
  }
  { /* 7.1.4 channel-based: 7 sub-streams, 5 coupled; audio-layer order L R SL SR BL BR HFL HFR HBL HBR C LFE */
    const int width[7] = {2, 2, 2, 2, 2, 1, 1}, first[7] = {0, 2, 4, 6, 8, 10, 11};
    int ok = ftu_walk_substreams(FTU_CHANNEL_BASED, 7, 5, 0, 0, 0, 0, 0, &w) == 0 && w.nsub == 7 && w.channels == 12;
    CHECK("7.1.4", ok && same_ints(w.width, width, 7) && same_ints(w.first, first, 7));
    ok = 1;
    for (int p = 0; p < 12; ++p) ok = ok && ftu_channel_source(FTU_CHANNEL_BASED, p, k_al_of_pl_714, 0, w.channels) == k_al_of_pl_714[p];
    CHECK("7.1.4: playback channels 2 and 3 (C, LFE) are the last two decoded ones",
          ok && ftu_channel_source(FTU_CHANNEL_BASED, 2, k_al_of_pl_714, 0, 12) == 10 && ftu_channel_source(FTU_CHANNEL_BASED, 3, k_al_of_pl_714, 0, 12) == 11);
    /* 16 bit, 64 samples, no head: pair s at s * 256 with its halves 2 bytes apart, C at 1280, LFE at 1408 */
    ok = ftu_raw_layout(&w, 0, FTU_CHANNEL_BASED, 12, k_al_of_pl_714, 0, 2, 1, 64, 0, 0, &L) == 12 * 128 && L.channels == 12;
    ok = ok && L.src_offset[0] == 0 && L.src_offset[1] == 2 && L.src_step[0] == 4 && L.src_step[1] == 4;  /* L, R */
    ok = ok && L.src_offset[2] == 1280 && L.src_step[2] == 2 && L.src_offset[3] == 1408 && L.src_step[3] == 2; /* C, LFE */
    ok = ok && L.src_offset[4] == 256 && L.src_offset[5] == 258 && L.src_offset[10] == 1024 && L.src_offset[11] == 1026 && L.src_step[11] == 4;
    CHECK("7.1.4: raw row in the renderer's order", ok);
  }
  { /* scalable stack with the demixer on: layers of (nsub, ncoupled) = (1, 1), (2, 1), (2, 2) */
    const int ln[3] = {1, 2, 2}, lc[3] = {1, 1, 2};
    const int width[5] = {2, 2, 1, 2, 2}, first[5] = {0, 2, 4, 5, 7};
    int ok = ftu_walk_substreams(FTU_CHANNEL_BASED, 99, 1, 0, 0, 3, ln, lc, &w) == 0 && w.nsub == 5 && w.channels == 9;
    CHECK("3-layer stack", ok && same_ints(w.width, width, 5) && same_ints(w.first, first, 5));
    /* decoded up to the second layer only */
    CHECK("3-layer stack, two decoded", ftu_walk_substreams(FTU_CHANNEL_BASED, 99, 1, 0, 0, 2, ln, lc, &w) == 0 && w.nsub == 3 && w.channels == 5);
    /* the demixer takes the decoded order: channel l of the row is decoded channel l */
    ok = ftu_raw_layout(&w, 1, FTU_CHANNEL_BASED, 6, 0, 0, 2, 1, 64, 16, slot, &L) == 16 + 5 * 128 && L.channels == 5;
    CHECK("3-layer stack: raw row in decoded order", ok && L.src_offset[0] == 16 && L.src_offset[1] == 18 && L.src_offset[2] == 272 &&
                                                         L.src_offset[3] == 274 && L.src_offset[4] == 528 && L.src_step[3] == 4 && L.src_step[4] == 2);
  }
  { /* an ambisonics map that names a channel no sub-stream carries: source -1, zero fill */
    const uint8_t holes[4] = {0, 3, 1, 255};
    int ok = ftu_walk_substreams(FTU_SCENE_BASED, 3, 0, 0, 0, 0, 0, 0, &w) == 0 && w.channels == 3;
    ok = ok && ftu_channel_source(FTU_SCENE_BASED, 0, 0, holes, 3) == 0 && ftu_channel_source(FTU_SCENE_BASED, 1, 0, holes, 3) == -1 &&
         ftu_channel_source(FTU_SCENE_BASED, 2, 0, holes, 3) == 1 && ftu_channel_source(FTU_SCENE_BASED, 3, 0, holes, 3) == -1;
    CHECK("map with holes", ok);
    ok = ftu_raw_layout(&w, 0, FTU_SCENE_BASED, 4, 0, holes, 2, 1, 64, 16, 0, &L) == 16 + 3 * 128 && L.channels == 4;
    CHECK("map with holes: raw row", ok && L.src_offset[0] == 16 && L.src_offset[1] == -1 && L.src_offset[2] == 144 && L.src_offset[3] == -1 &&
                                         L.src_step[1] == 2);
  }
  CHECK("no sub-stream", ftu_walk_substreams(FTU_SCENE_BASED, 0, 0, 0, 0, 0, 0, 0, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("too many sub-streams", ftu_walk_substreams(FTU_SCENE_BASED, FTU_MAX_SUBSTREAMS + 1, 0, 0, 0, 0, 0, 0, &w) == IAMF_HIP_ERR_BAD_ARG);
  CHECK("24 sub-streams", ftu_walk_substreams(FTU_SCENE_BASED, FTU_MAX_SUBSTREAMS, 0, 0, 0, 0, 0, 0, &w) == 0 && w.channels == 24);
}

static void element_stage(void) {
  static float in[16 * 1024];
  static iamf_hip_dmx_frame dmx;
  static iamf_hip_demix_frame demix;
  iamf_hip_render_args a;
  int tag;
  ftu_element_stage_args(&a, in, 16, 1024, 0, 4, 40, 980, 0, 0, &tag);
  CHECK("LFE off", a.d_in == in && a.lfe_pre_samples == 0 && a.lfe_post_samples == 0);
  CHECK("strides", a.in_stream_stride == 16 * 1024 && a.in_frame_stride == 16 * 1024);
  CHECK("keep < fs", a.n_frames == 1 && a.n_samples == 980 && a.stream == &tag);
  CHECK("null records", a.d_dmx_frames == 0 && a.d_demix_frames == 0 && a.demix_sample0 == 0);
  CHECK("the rest is zero", a.d_in2 == 0 && a.d_element_ramp == 0 && a.d_element2_ramp == 0 && a.d_output_ramp == 0 && a.d_pcm == 0 &&
                                a.ramp_stream_stride == 0 && a.pcm_stream_stride_bytes == 0 && a.reserved0 == 0);
  ftu_element_stage_args(&a, in, 16, 1024, 1, 4, 40, 980, &dmx, &demix, 0);
  CHECK("LFE on", a.d_in == in + 4 && a.lfe_pre_samples == 4 && a.lfe_post_samples == 40);
  CHECK("records", a.d_dmx_frames == &dmx && a.d_demix_frames == &demix && a.demix_sample0 == 4);
  ftu_element_stage_args(&a, in, 4, 1024, 0, 0, 0, 1024, 0, &demix, 0);
  CHECK("keep == fs", a.n_samples == 0 && a.n_frames == 1 && a.in_stream_stride == 4096 && a.demix_sample0 == 0);
  ftu_element_stage_args(&a, 0, 4, 1024, 1, 8, 0, 64, 0, 0, 0);
  CHECK("packets instead of rows", a.d_in == 0 && a.lfe_pre_samples == 8 && a.n_samples == 64);
}

static void last_stage(void) {
  static float eye[24 * 24], res[64];
  static char pcm[64];
  const int ocs[2] = {2, 12};
  for (int t = 0; t < 2; ++t) {
    const int oc = ocs[t];
    iamf_hip_batch_config c;
    int ok = 1;
    ftu_last_stage_config(&c, eye, 7, 48000, oc, 24, 12, 1, -1.5f, 1);
    for (int i = 0; i < oc; ++i)
      for (int j = 0; j < oc; ++j) ok = ok && eye[i * oc + j] == (i == j ? 1.f : 0.f);
    CHECK("identity", ok && c.matrix.mat == eye && c.matrix.kind == IAMF_HIP_KIND_M2M && c.matrix.m == oc && c.matrix.n == oc &&
                          c.matrix.channels == oc);
    CHECK("lfe1 = lfe2 = -1", c.matrix.lfe1 == -1 && c.matrix.lfe2 == -1);
    CHECK("frame_size = 1", c.frame_size == 1 && c.n_streams == 7 && c.sample_rate == 48000 && c.out_channels == oc);
    CHECK("output", c.out_format == 24 && c.pcm_stride_channels == 12 && c.limiter_enable == 1 && c.limiter_threshold_db == -1.5f &&
                        c.loudness_enable == 1 && c.projection == IAMF_HIP_PROJ_EXACT && c.lfe_hoa == 0 && c.out_gain_channels == 0);
  }
  {
    iamf_hip_render_args a;
    int tag;
    ftu_last_stage_args(&a, res, 4096, 2, 441, pcm, 8192, &tag);
    CHECK("last-stage call", a.d_in == res && a.in_stream_stride == 4096 && a.in_frame_stride == 2 && a.n_frames == 441 && a.n_samples == 0 &&
                                 a.d_pcm == pcm && a.pcm_stream_stride_bytes == 8192 && a.stream == &tag && a.d_in2 == 0);
  }
}

int main(void) {
  trim_window();
  substream_walk();
  element_stage();
  last_stage();
  printf("%d cases, %d wrong\n%s\n", cases, wrong, wrong ? "FAILED" : "OK");
  return wrong != 0;
}
