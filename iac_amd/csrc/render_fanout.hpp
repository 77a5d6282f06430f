// render_fanout.hpp — one element, several renditions, one pass over the input: render_fanout_kernel<M, K, LP> renders the
// M-channel element of a stream into K member batches, each with its own matrix, gains, limiter and PCM format, and reads
// the element ONCE.  ONE kernel body with two input paths, chosen at compile time as in render_fast_kernel<.., LP>:
//   LP = false  planar f32 element PCM (FanParams; iamf_hip_batch_render_fanout, iamf_render.hip).  Every workload of the
//               plain kernel (render_fast.hpp) is bound by the 4 * M bytes per sample-frame it reads; K renditions of one
//               element cost 4 * M + sum(out bytes) here instead of K * 4 * M + sum(out bytes).
//   LP = true   the 16-bit LPCM packets of a mono-coded ambisonics element, read by the kernel itself (FanLpParams;
//               iamf_hip_batch_render_fanout_lpcm): 2 * M + sum(out bytes) instead of K * 2 * M + sum(out bytes) for K
//               calls of render_fast_kernel<.., LP>, or 2 * M + 8 * M + sum(out bytes) for an unpack pass and LP = false.
// The two differ in six places, each an `if constexpr (LP)` below: the staged weights' scale, the stream's base pointer,
// the per-channel input registers, load_one, the fill of lanes past the end of the call, and where channel m is consumed.
// Everything else — member state, rings, window maximum, limiter rounds, PCM stores, persistence — is written once.
//
// The geometry is render_fast_kernel's — one workgroup of 256 lanes per stream, 1024-sample chunks, four consecutive
// samples per lane — so the persisted state (LimState, ring_y, ring_pm: the generic kernel's format) is read and written
// by the same lane <-> sample mapping, and a batch may go through either form of this kernel, render_fast_kernel with or
// without LP and the generic kernel in any order.  Per chunk:
//   1. the element's channels are consumed one by one (non-temporal buffer loads, one resource per stream); while
//      channel m is live every output slot of every member adds its product — ascending channel order, one rounding per
//      product and per sum: the plain kernel's and the reference's arithmetic — and channel m of the NEXT chunk is
//      requested as soon as channel m has been consumed, so the loads fly under everything below.  When there is no next
//      chunk the requests go through a resource of zero records, which answers every load with zeros; lanes past the end
//      of the call hold zeros;
//   2. member by member: gains in the reference's order, max |y|, the member's LDS rings, the 240-sample window
//      maximum, the limiter gains (hypothesis, workgroup vote, limiter_wave for the blocks that trigger), delayed
//      samples * gain -> the member's PCM in the member's format.
// The input path of LP = false: one 16-byte load per channel and lane, a float4 per channel.  Of LP = true
// (render_fast_kernel<.., LP>'s, render_fast.hpp):
//   - the resource lies over the stream's packet region, the lane's byte offset is in one register for all channels and
//     the channel's run offset (lpcm_off[m]) is the load's scalar offset: one 8-byte load per channel and lane;
//   - two dwords are kept per channel (four 16-bit samples as they lie in memory) instead of a float4 — half the live
//     input registers — and (float)(int16) happens where channel m is consumed;
//   - the decoder's "/ 32768" is folded into every slot's staged weights: (w * 2^-15) * (float)s has the bits of
//     w * (s * 2^-15) for the matrices the host admits (iamf_hip_batch::lp_scale_ok: a power of two commutes with
//     rounding as long as neither the scaled weight nor a product leaves the normal range), so each product and each sum
//     is rounded once, in ascending channel order: the reference's arithmetic.
// LP with LPB / LPC (their meaning in render_fast_kernel; iamf_hip_batch_render_fanout_packets): the other three packet forms
// of lpcm_form.hpp, in the same six places and nowhere else.
//   - LPB == 3 (S24): three dwords per channel (four 24-bit samples as they lie in memory), one 12-byte load per channel and
//     lane at 3 * i, cut where channel m is consumed — a[23:0], {b[15:0], a[31:24]}, {c[7:0], b[31:16]}, c[31:8], sign-extended —
//     and "/ 2^23" folded into the staged weights (the argument at mat[t] in render_fast.hpp, under the same host check);
//   - LPC (S16C, S24C): the pairs of lpcm_coupled_paired(M, m) lie interleaved sample by sample.  A pair is loaded once, when
//     its first channel is named — one 16-byte load at 4 * i, or two 12-byte loads at 6 * i — into its two channels'
//     registers; L is cut out of the low halves (triples 0 and 2) where channel m is consumed, R one channel later out of the
//     high halves (triples 1 and 3), and the pair's next chunk is requested once its SECOND channel has been consumed.  C and
//     LFE are mono runs under the form's mono rule.
//   The cut and convert expressions restate render_fast.hpp's (LP3, LPC there): that kernel keeps them inline, between its own
//   ordering fences, and lifting them into device functions moved its instances' instructions.
// A member has one or two output channels (a run-time property: the instantiations are <M, K, LP, LPB, LPC> only; a mono member's
// second slot carries zero weights).  The rings and the staged limiter-table window / head are per member; the array of
// window maxima the limiter walk reads — and overwrites, block by block, with its gains — is transient and serves the
// members in turn.  Of max |y| only what the next call needs is kept (the last 256 samples; the window maximum reads the
// per-16 suffix and block maxima): 25.7 KB per member, so that THREE members still run two workgroups per CU.
//
// The parameter block is passed by value and read in place (p.x): no reference or pointer to `p` as a whole is taken and
// it is passed to no function, so that its fields stay scalar loads from the kernel-argument segment where they are used.
#pragma once

constexpr int kFanMax = IAMF_HIP_FANOUT_MAX;

struct FanMember {          // what differs between the renditions
  uint8_t *pcm;             // packed output (device)
  int64_t pcm_stream_stride;  // bytes
  const float *matrix;      // device, feed-major [n_feeds][M]
  const float *gains;       // device [3][n_streams]: element, output, loudness
  const float *ctab;        // device limiter coefficient table [n_end + 1]
  LimState *lim;            // device [n_streams]
  float *ring_y;            // device [n_streams][out_ch][kSave]
  float *ring_pm;           // device [n_streams][kSave]
  const int32_t *src_feed;  // device [out_ch]
  int32_t out_ch;           // 1 or 2
  int32_t out_format;
  int32_t loudness_on;
  int32_t n_atk, n_end;
  float thr;
};

struct FanParams {          // what the renditions share, then the members
  const float *in;          // planar f32 element PCM (device)
  int64_t in_stream_stride; // floats
  int64_t in_frame_stride;  // floats
  int64_t pos0;             // samples of each stream consumed before this call (the same for every member)
  int32_t total;            // samples to process in this call: a multiple of 64
  int32_t frame_size;
  int32_t n_streams;        // streams of every member batch (the per-stream arrays' extent)
  int32_t stream0, n_launch;  // workgroup i takes stream stream0 + i
  FanMember mem[kFanMax];
};

struct FanLpParams {        // LP: the packets, what the renditions share, then the members
  const uint8_t *lpcm;      // packet rows (device): stream s, frame f at lpcm + s * stream stride + f * frame stride
  int64_t lpcm_stream_stride;  // bytes, a multiple of 8
  int64_t lpcm_frame_stride;   // bytes, a multiple of 8
  int32_t lpcm_off[16];     // byte offset of channel m's run of little-endian 16-bit samples in a row, a multiple of 8
  int64_t pos0;             // samples of each stream consumed before this call (the same for every member)
  int32_t total;            // samples to process in this call: a multiple of 64
  int32_t frame_size;
  int32_t n_streams;        // streams of every member batch (the per-stream arrays' extent)
  int32_t stream0, n_launch;  // workgroup i takes stream stream0 + i
  FanMember mem[kFanMax];
};

// LDS floats of one member: ring_y [2][R], ring_suf [R], ring_bm [2][R/16], pm_tail [kSave], win [kFWin], head [kFWin]
__host__ __device__ constexpr int fan_member_floats() { return 3 * kFRing + 2 * (kFRing / 16) + kSave + 2 * kFWin; }
// ... and of a workgroup: the members, arr_p [1024], the 2 * K slots' matrix rows, misc [16]
__host__ __device__ constexpr int fan_lds_floats(int k, int m) {
  return k * fan_member_floats() + kFChunk + ((2 * k * m + 15) & ~15) + 16;
}

template <int M, int K, bool LP, int LPB = 2, bool LPC = false>
__global__ __launch_bounds__(256, K <= 3 ? 2 : 1) void render_fanout_kernel(const std::conditional_t<LP, FanLpParams, FanParams> p) {
  static_assert(!LP || M <= 16, "one run offset per channel");
  static_assert(LPB == 2 || (LP && LPB == 3), "packet samples of 16 or 24 bits");
  static_assert(!LPC || (LP && lpcm_coupled_m(M)), "coupled pairs: 16- or 24-bit packets of a loudspeaker layout");
  constexpr bool LP3 = LP && LPB == 3;
  static_assert(K >= 2 && K <= kFanMax, "two to four members");
  extern __shared__ float lds[];
  constexpr int R = kFRing;
  constexpr int NB = R / 16;
  constexpr int MB = fan_member_floats();
  constexpr int NS = 2 * K;                 // output slots: two per member
  // member j: ring_y = lds + j * MB, then ring_suf, ring_bm, pm_tail, win, head
  constexpr int oSuf = 2 * R, oBm = 3 * R, oPm = 3 * R + 2 * NB, oWin = oPm + kSave, oHead = oWin + kFWin;
  // pm_tail: max |y| of the last 256 samples seen, sample k of the call (k = -256 + t: saved entry t) at k & 255
  float *arr_p = lds + K * MB;              // [1024]   window maxima of the chunk (the member at work)
  // The limiter wave's gains go where it has read the window maxima: limiter_wave takes a block's maxima into registers
  // before it writes the block's gains, a later walk only reads blocks no walk has reached yet, and the hypothesis
  // rounds keep their maxima in registers.
  float *arr_g = arr_p;
  float *mat = arr_p + kFChunk;             // [NS][M]  matrix rows of the slots
  float *misc = mat + ((NS * M + 15) & ~15);  // [16]
  constexpr bool kWG = (M % 4) == 0;        // weights read four input channels at a time

  const int s = blockIdx.x + p.stream0;
  const int t = (int)threadIdx.x;
  const int wave = t >> 6;
  const int lane = t & 63;
  const int q = t & 3;
  const int fs = p.frame_size;
  // ring position of the chunk's first sample (a multiple of 16; see render_fast.hpp): the same for every member
  int base = (int)((p.pos0 & ~(int64_t)15) % R);

  // ---- stream state and constants of every member -> LDS (persisted format is the generic kernel's) ----
  float g_cur[K], gs[K], ge[K], m_eg[K], m_og[K], m_lg[K];
  int n_st[K];
  bool any_gain[K], live[K][2];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const FanMember &mb = p.mem[j];
    float *my = lds + j * MB;
    const int oc = mb.out_ch;
    const float *sy = mb.ring_y + (int64_t)s * oc * kSave;
    const float *spm = mb.ring_pm + (int64_t)s * kSave;
    const int rp = ring_wrap(base - kSave + t);  // saved entry t is sample pos0 - 256 + t
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (c < oc) my[c * R + rp] = sy[c * kSave + t];
    const float pm = spm[t];
    my[oPm + t] = pm;
    float sfx = pm;
    sfx = fmaxf(sfx, __shfl_down(sfx, 1, 16));
    sfx = fmaxf(sfx, __shfl_down(sfx, 2, 16));
    sfx = fmaxf(sfx, __shfl_down(sfx, 4, 16));
    sfx = fmaxf(sfx, __shfl_down(sfx, 8, 16));
    my[oSuf + rp] = sfx;
    if ((t & 15) == 0) my[oBm + (rp >> 4)] = my[oBm + (rp >> 4) + NB] = sfx;
    const int n_end = mb.n_end;
    for (int i = t; i < kFWin; i += 256) my[oHead + i] = mb.ctab[i < n_end ? i : n_end];
    if (t < 2 * M) {
      const int c = t / M, m = t - c * M;
      const int f = c < oc ? mb.src_feed[c] : -1;
      if constexpr (LP3)  // 24-bit samples: "/ 2^23", by the same argument and under the same host check
        mat[2 * j * M + t] = (f >= 0 ? mb.matrix[f * M + m] : 0.f) * (1.0f / 8388608.0f);
      else if constexpr (LP)   // the LPCM decoder's "sample / 32768.f" folded into the weight (the host has checked lp_scale_ok)
        mat[2 * j * M + t] = (f >= 0 ? mb.matrix[f * M + m] : 0.f) * (1.0f / 32768.0f);
      else
        mat[2 * j * M + t] = f >= 0 ? mb.matrix[f * M + m] : 0.f;
    }
    const LimState ls = mb.lim[s];
    g_cur[j] = ls.g, gs[j] = ls.gs, ge[j] = ls.ge, n_st[j] = ls.n;
    const float eg = mb.gains[s], og = mb.gains[p.n_streams + s], lg = mb.gains[2 * p.n_streams + s];
    const bool eg_on = (eg != 1.f && eg > 0.f);
    const bool og_on = (og != 1.f && og > 0.f);
    const bool lg_on = mb.loudness_on && (lg != 1.0f);
    m_eg[j] = eg_on ? eg : 1.f, m_og[j] = og_on ? og : 1.f, m_lg[j] = lg_on ? lg : 1.f;
    any_gain[j] = eg_on || og_on || lg_on;
#pragma unroll
    for (int c = 0; c < 2; ++c) live[j][c] = c < oc && mb.src_feed[c] >= 0;
  }
  chain_wave_publish(misc + 12);

  const int64_t out_base = p.pos0 > kDelay ? p.pos0 - kDelay : 0;
  const void *in_s;
  if constexpr (LP)
    in_s = p.lpcm + (int64_t)s * p.lpcm_stream_stride;
  else
    in_s = p.in + (int64_t)s * p.in_stream_stride;

  // ---- the element's input: buffer loads, one resource per stream (render_fast.hpp).  Per channel a float4, or (LP) the
  //      packets' samples as they lie in memory: four 16-bit samples in two dwords ----
  using lp_u2 = __attribute__((ext_vector_type(2))) unsigned;
  std::conditional_t<LP, lp_u2, float4> x[LP3 ? 1 : M];
  // LPB == 3: four 24-bit samples in three dwords.  (LPC: a pair's {L0:R0} .. {L3:R3} in x[m], x[m + 1], m even; with 24-bit
  // samples L0 R0 L1 R1 in x3[m] and L2 R2 L3 R3 in x3[m + 1])
  struct lp_u3 {
    unsigned a, b, c;
  };
  lp_u3 x3[LP3 ? M : 1];
  const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(in_s), 0, 0x7fffffff, 0x00020000);
  // (zero records: every load through it is answered with zeros — the requests for "the next chunk" when there is none)
  const __amdgpu_buffer_rsrc_t rs_none = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(in_s), 0, 0, 0x00020000);
  const bool fr_uni = (fs & (kFChunk - 1)) == 0;   // a chunk lies in ONE frame: workgroup-uniform counters
  int fu = 0, iu = 0;
  auto frame_pos = [&](int kq, int &f, int &i) {
    if (fr_uni) {
      f = fu;
      i = iu + 4 * t;
    } else {
      f = kq / fs;
      i = kq - f * fs;
    }
  };
  auto load_one = [&](int m, int f, int i, __amdgpu_buffer_rsrc_t rs) {
    if constexpr (LP3 && LPC) {
      // (24 bytes on the dword grid: the pair's run offset is a multiple of 4 — lpcm_form.hpp, S24C — and 6 * i one of 24;
      //  M is even for every coupled layout, so a pair's second channel exists)
      if (lpcm_coupled_paired(M, m)) {
        if (!(m & 1)) {
          const int vo = f * (int)p.lpcm_frame_stride + 6 * i;
          const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, vo, p.lpcm_off[m], 2 /* nt */);
          const auto w = __builtin_amdgcn_raw_buffer_load_b96(rs, vo + 12, p.lpcm_off[m], 2 /* nt */);
          const int m1 = m + 1 < M ? m + 1 : m;
          x3[m].a = v[0], x3[m].b = v[1], x3[m].c = v[2];
          x3[m1].a = w[0], x3[m1].b = w[1], x3[m1].c = w[2];
        }
      } else {
        const int vo = f * (int)p.lpcm_frame_stride + 3 * i;
        const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, vo, p.lpcm_off[m], 2 /* nt */);
        x3[m] = lp_u3{v[0], v[1], v[2]};
      }
    } else if constexpr (LP3) {
      // (dword-aligned: the stream's base, the frame stride and the run offsets are multiples of 4 — lpcm_form.hpp, S24 —
      //  and 3 * i is one of 12)
      const int vo = f * (int)p.lpcm_frame_stride + 3 * i;
      const auto v = __builtin_amdgcn_raw_buffer_load_b96(rs, vo, p.lpcm_off[m], 2 /* nt */);
      x3[m] = lp_u3{v[0], v[1], v[2]};
    } else if constexpr (LPC) {
      // (16 bytes on the 8-byte grid: the pair's run offset is a multiple of 8 — lpcm_form.hpp, S16C — and 4 * i one of 16)
      if (lpcm_coupled_paired(M, m)) {
        if (!(m & 1)) {
          const int vo = f * (int)p.lpcm_frame_stride + 4 * i;
          const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, p.lpcm_off[m], 2 /* nt */);
          x[m] = lp_u2{v[0], v[1]};
          x[m + 1 < M ? m + 1 : m] = lp_u2{v[2], v[3]};
        }
      } else {
        const int vo = f * (int)p.lpcm_frame_stride + 2 * i;
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo, p.lpcm_off[m], 2 /* nt */);
        x[m] = lp_u2{v[0], v[1]};
      }
    } else if constexpr (LP) {
      const int vo = f * (int)p.lpcm_frame_stride + 2 * i;
      const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo, p.lpcm_off[m], 2 /* nt */);
      x[m] = lp_u2{v[0], v[1]};
    } else {
      const int vo = 4 * (f * (int)p.in_frame_stride + i);
      const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, 4 * m * fs, 2 /* nt */);
      x[m] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    }
  };
  {
    const int k = 4 * t;
    if (k < p.total) {
      int f, i;
      frame_pos(k, f, i);
#pragma unroll
      for (int m = 0; m < M; ++m) load_one(m, f, i, rs_in);
    } else {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if constexpr (LP3)
          x3[m] = lp_u3{0u, 0u, 0u};
        else if constexpr (LP)
          x[m] = lp_u2{0u, 0u};
        else
          x[m] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  __syncthreads();
  const int cw = chain_wave_pick(misc + 12);

  // Table window member j's next chunk can reach without a trigger: win[i] = ctab[min(n_st + 1 + i, n_end)]; fetched
  // before the member's PCM stores are issued, written to LDS at the top of the next chunk (render_fast.hpp)
  float wv[K][5];
  auto fetch_window = [&](int j, int n0) {
    const FanMember &mb = p.mem[j];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const int i = n0 + 1 + t + 256 * r;
      wv[j][r] = 1.0f;
      if (n0 < mb.n_end && t + 256 * r < kFWin) wv[j][r] = mb.ctab[i < mb.n_end ? i : mb.n_end];
    }
  };
#pragma unroll
  for (int j = 0; j < K; ++j) fetch_window(j, n_st[j]);

  for (int c0 = 0; c0 < p.total; c0 += kFChunk) {
    const int cnt = p.total - c0 < kFChunk ? p.total - c0 : kFChunk;  // multiple of 64
    const int k = c0 + 4 * t;
    const bool valid = 4 * t < cnt;
    const int64_t gk = p.pos0 + k;
    const int rp = ring_wrap(base + 4 * t);
    const int rd = ring_wrap(base + 4 * t - kDelay);  // ring position of sample gk - 240
    const int nblk = cnt >> 6;

    // the members' table windows -> LDS (their loads are older than anything still in flight), then the place of the
    // next chunk: the projection requests it channel by channel
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
      for (int r = 0; r < 5; ++r)
        if (t + 256 * r < kFWin) lds[j * MB + oWin + t + 256 * r] = wv[j][r];
    int pf_f = 0, pf_i = 0;
    __amdgpu_buffer_rsrc_t rs_pf = rs_none;
    {
      const int kn = k + kFChunk;
      iu += kFChunk;
      if (iu >= fs) {
        iu -= fs;
        ++fu;
      }
      if (c0 + kFChunk < p.total) rs_pf = rs_in;   // workgroup-uniform: there is a next chunk
      frame_pos(kn, pf_f, pf_i);
      if (kn >= p.total) pf_f = pf_i = 0;   // a lane past the end of the call requests the stream's first samples (unused)
    }

    // ---- every member's projection, input channel by input channel (pairs of samples: two f32 products or sums per
    //      packed instruction, each rounded on its own) ----
    using f2 = __attribute__((ext_vector_type(2))) float;
    f2 prj[2 * NS];
#pragma unroll
    for (int c = 0; c < 2 * NS; ++c) prj[c] = f2{0.f, 0.f};
    {
      float wg[NS][4];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        if constexpr (kWG) {
          if ((m & 3) == 0) {
#pragma unroll
            for (int c = 0; c < NS; ++c) {
              const float4 w4 = *reinterpret_cast<const float4 *>(&mat[c * M + m]);
              wg[c][0] = w4.x, wg[c][1] = w4.y, wg[c][2] = w4.z, wg[c][3] = w4.w;
            }
          }
        }
        // channel m is taken up — LP: its packets converted — when channel m - 1 has been added up: the weights of one
        // group of four channels (LP: and ONE converted channel) are all that is live beside the samples and the sums
#pragma unroll
        for (int c = 0; c < 2 * NS; ++c) asm volatile("" : "+v"(prj[c]));
        f2 xa, xb;
        if constexpr (LP3 && LPC) {
          if (lpcm_coupled_paired(M, m)) {   // (m is a constant of the unrolled loop)
            // half m & 1 of the pair whose six dwords lie in x3[m & ~1], x3[m | 1]: the fence covers all six (the partner's half
            // is still to be, or has just been, cut out of them); each triple is cut as the 24-bit form's, L takes its samples 0
            // and 2, R 1 and 3
            const int m0 = m & ~1, m1 = (m | 1) < M ? (m | 1) : m;
            asm volatile("" : "+v"(x3[m0].a), "+v"(x3[m0].b), "+v"(x3[m0].c), "+v"(x3[m1].a), "+v"(x3[m1].b), "+v"(x3[m1].c));
            const unsigned a = x3[m0].a, b = x3[m0].b, c = x3[m0].c, d = x3[m1].a, e = x3[m1].b, g = x3[m1].c;
            if ((m & 1) == 0) {
              xa = f2{(float)((int)(a << 8) >> 8), (float)((int)(__builtin_amdgcn_alignbit(c, b, 16) << 8) >> 8)};
              xb = f2{(float)((int)(d << 8) >> 8), (float)((int)(__builtin_amdgcn_alignbit(g, e, 16) << 8) >> 8)};
            } else {
              xa = f2{(float)((int)(__builtin_amdgcn_alignbit(b, a, 24) << 8) >> 8), (float)((int)c >> 8)};
              xb = f2{(float)((int)(__builtin_amdgcn_alignbit(e, d, 24) << 8) >> 8), (float)((int)g >> 8)};
            }
          } else {   // C, LFE: a mono run, the 24-bit form's conversion below
            asm volatile("" : "+v"(x3[m].a), "+v"(x3[m].b), "+v"(x3[m].c));
            const unsigned a = x3[m].a, b = x3[m].b, c = x3[m].c;
            xa = f2{(float)((int)(a << 8) >> 8), (float)((int)(__builtin_amdgcn_alignbit(b, a, 24) << 8) >> 8)};
            xb = f2{(float)((int)(__builtin_amdgcn_alignbit(c, b, 16) << 8) >> 8), (float)((int)c >> 8)};
          }
        } else if constexpr (LP3) {
          asm volatile("" : "+v"(x3[m].a), "+v"(x3[m].b), "+v"(x3[m].c));
          const unsigned a = x3[m].a, b = x3[m].b, c = x3[m].c;   // (the scale 2^-23 sits in the weights)
          // sign-extended from 24 bits: a bit-field extract of the dword (or of the two dwords' funnel) the sample lies in
          xa = f2{(float)((int)(a << 8) >> 8), (float)((int)(__builtin_amdgcn_alignbit(b, a, 24) << 8) >> 8)};
          xb = f2{(float)((int)(__builtin_amdgcn_alignbit(c, b, 16) << 8) >> 8), (float)((int)c >> 8)};
        } else if constexpr (LPC) {
          if (lpcm_coupled_paired(M, m)) {   // (m is a constant of the unrolled loop)
            // half m & 1 of the pair whose four dwords lie in x[m & ~1], x[m | 1]: the fence covers all four
            const int m0 = m & ~1, m1 = (m | 1) < M ? (m | 1) : m;
            asm volatile("" : "+v"(x[m0].x), "+v"(x[m0].y), "+v"(x[m1].x), "+v"(x[m1].y));
            const unsigned a = x[m0].x, b = x[m0].y, c = x[m1].x, d = x[m1].y;   // (the scale 2^-15 sits in the weights)
            if ((m & 1) == 0) {
              xa = f2{(float)(int)(short)(a & 0xffffu), (float)(int)(short)(b & 0xffffu)};
              xb = f2{(float)(int)(short)(c & 0xffffu), (float)(int)(short)(d & 0xffffu)};
            } else {
              xa = f2{(float)((int)a >> 16), (float)((int)b >> 16)};
              xb = f2{(float)((int)c >> 16), (float)((int)d >> 16)};
            }
          } else {   // C, LFE: a mono run, the 16-bit form's conversion below
            asm volatile("" : "+v"(x[m].x), "+v"(x[m].y));
            const unsigned pa = x[m].x, pb = x[m].y;
            xa = f2{(float)(int)(short)(pa & 0xffffu), (float)((int)pa >> 16)};
            xb = f2{(float)(int)(short)(pb & 0xffffu), (float)((int)pb >> 16)};
          }
        } else if constexpr (LP) {
          asm volatile("" : "+v"(x[m].x), "+v"(x[m].y));
          const unsigned pa = x[m].x, pb = x[m].y;   // (the scale 2^-15 sits in the weights: see where `mat` is filled)
          xa = f2{(float)(int)(short)(pa & 0xffffu), (float)((int)pa >> 16)};
          xb = f2{(float)(int)(short)(pb & 0xffffu), (float)((int)pb >> 16)};
        } else {
          asm volatile("" : "+v"(x[m].x), "+v"(x[m].y), "+v"(x[m].z), "+v"(x[m].w));
          xa = f2{x[m].x, x[m].y};
          xb = f2{x[m].z, x[m].w};
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) {
          const float w = kWG ? wg[c][m & 3] : mat[c * M + m];
          const f2 w2 = {w, w};
          prj[2 * c] = prj[2 * c] + w2 * xa;
          prj[2 * c + 1] = prj[2 * c + 1] + w2 * xb;
        }
        // channel m's registers are free: its samples of the next chunk are requested now (LPC: a pair's, once its SECOND
        // channel has been consumed)
        if constexpr (LPC) {
          if (!lpcm_coupled_paired(M, m)) load_one(m, pf_f, pf_i, rs_pf);
          else if (m & 1) load_one(m - 1, pf_f, pf_i, rs_pf);
        } else {
          load_one(m, pf_f, pf_i, rs_pf);
        }
      }
    }

    // ---- member by member: gains, rings, window maximum, limiter, PCM ----
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const FanMember &mb = p.mem[j];
      float *ring_y = lds + j * MB;
      float *pm_tail = ring_y + oPm;
      float *ring_suf = ring_y + oSuf;
      float *ring_bm = ring_y + oBm;
      const float *win = ring_y + oWin;
      const float *head = ring_y + oHead;
      const int oc = mb.out_ch;
      const float thr = mb.thr;
      const int n_atk = mb.n_atk, n_end = mb.n_end;

      float4 y[2];
      float4 pm = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[j][c]) v = make_float4(prj[2 * (2 * j + c)].x, prj[2 * (2 * j + c)].y, prj[2 * (2 * j + c) + 1].x, prj[2 * (2 * j + c) + 1].y);
        if (any_gain[j]) {  // a skipped gain is a multiplication by exactly 1 (render_fast.hpp)
          v.x = ((v.x * m_eg[j]) * m_og[j]) * m_lg[j];
          v.y = ((v.y * m_eg[j]) * m_og[j]) * m_lg[j];
          v.z = ((v.z * m_eg[j]) * m_og[j]) * m_lg[j];
          v.w = ((v.w * m_eg[j]) * m_og[j]) * m_lg[j];
        }
        y[c] = v;   // (a mono member's second slot is not live: zeros, which leave the maxima alone)
        pm.x = fmaxf(pm.x, fabsf(v.x));
        pm.y = fmaxf(pm.y, fabsf(v.y));
        pm.z = fmaxf(pm.z, fabsf(v.z));
        pm.w = fmaxf(pm.w, fabsf(v.w));
      }

      // ---- per-16 prefix / suffix / block maxima: 4 lanes x 4 samples = one aligned block ----
      float4 pre_ex;
      {
        const float i0 = pm.x, i1 = fmaxf(i0, pm.y), i2 = fmaxf(i1, pm.z), i3 = fmaxf(i2, pm.w);
        const float s3 = pm.w, s2 = fmaxf(pm.z, s3), s1 = fmaxf(pm.y, s2), s0 = fmaxf(pm.x, s1);
        const float qa = dpp_quad_bcast0(i3), qb = dpp_quad_bcast1(i3), qc = dpp_quad_bcast2(i3), qd = dpp_quad_bcast3(i3);
        const float before = fmaxf(fmaxf(q >= 1 ? qa : 0.f, q >= 2 ? qb : 0.f), q >= 3 ? qc : 0.f);
        const float after = fmaxf(fmaxf(q <= 2 ? qd : 0.f, q <= 1 ? qc : 0.f), q <= 0 ? qb : 0.f);
        pre_ex = make_float4(before, fmaxf(before, i0), fmaxf(before, i1), fmaxf(before, i2));
        if (valid) {
#pragma unroll
          for (int c = 0; c < 2; ++c) *reinterpret_cast<float4 *>(&ring_y[c * R + rp]) = y[c];
          if (4 * t >= cnt - kSave) *reinterpret_cast<float4 *>(&pm_tail[(c0 + 4 * t) & (kSave - 1)]) = pm;
          *reinterpret_cast<float4 *>(&ring_suf[rp]) =
              make_float4(fmaxf(s0, after), fmaxf(s1, after), fmaxf(s2, after), fmaxf(s3, after));
          if (q == 0) ring_bm[rp >> 4] = ring_bm[(rp >> 4) + NB] = fmaxf(fmaxf(qa, qb), fmaxf(qc, qd));
        }
      }
      __syncthreads();   // (also: the previous member is done with arr_p, arr_g and misc)

      // ---- 240-sample window maximum = tail of block b-15, blocks b-14..b-1, head of block b ----
      float4 g = make_float4(1.f, 1.f, 1.f, 1.f);
      float4 pk4;
      {
        const float *bm = ring_bm + ((rp >> 4) + NB - 14 + (q < 3 ? 4 * q : 10));
        float w14 = fmaxf(fmaxf(bm[0], bm[1]), fmaxf(bm[2], bm[3]));
        w14 = fmaxf(w14, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w14), 0xB1, 0xf, 0xf, true)));  // quad_perm [1,0,3,2]
        w14 = fmaxf(w14, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(w14), 0x4E, 0xf, 0xf, true)));  // quad_perm [2,3,0,1]
        const float4 so = *reinterpret_cast<const float4 *>(&ring_suf[rd]);
        pk4.x = fmaxf(fmaxf(so.x, w14), pre_ex.x);
        pk4.y = fmaxf(fmaxf(so.y, w14), pre_ex.y);
        pk4.z = fmaxf(fmaxf(so.z, w14), pre_ex.z);
        pk4.w = fmaxf(fmaxf(so.w, w14), pre_ex.w);
        *reinterpret_cast<float4 *>(&arr_p[4 * t]) = pk4;
      }

      // ---- limiter gains in rounds: hypothesis "no trigger from block bs on", workgroup vote, the chain wave walks the
      //      blocks that trigger and one more, the next round re-evaluates the rest (render_fast.hpp) ----
      const int n_chunk = n_st[j];  // what the staged table window is based on
      auto look = [&](int ci) {     // before the chunk's first trigger: the window; after one: the head
        const int d = ci - n_chunk - 1;
        return (d >= 0 && d < kFWin) ? win[d] : head[ci < kFWin ? ci : kFWin - 1];
      };
      int bs = 0;
      while (true) {
        {
          int kfirst = kBig;
          const int o0 = 4 * t - 64 * bs;   // the lane's first sample, counted from the round's start state
          if (o0 >= 0) {
            const int n0 = __builtin_amdgcn_readfirstlane(n_st[j]);
            const int last = n0 + (cnt - 64 * bs) - 1;   // step count of the chunk's last sample under the hypothesis
            float gh[4] = {1.f, 1.f, 1.f, 1.f};
            if (n0 < n_end) {
              const float *tb = (bs == 0 ? win : head + (n0 + 1)) + o0;
              const float cf[4] = {tb[0], tb[1], tb[2], tb[3]};
              if (n0 >= n_atk && last < n_end) {   // release throughout: ge + c * (1 - ge)
                const float r1 = 1.0f - ge[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) gh[i] = ge[j] + cf[i] * r1;
              } else {
                const int nb = n0 + o0;
                const float a1 = gs[j] - ge[j], r1 = 1.0f - ge[j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  const float ga = gs[j] - cf[i] * a1, gr = ge[j] + cf[i] * r1;
                  gh[i] = nb + i < n_atk ? ga : (nb + i < n_end ? gr : 1.0f);
                }
              }
            }
            g = make_float4(gh[0], gh[1], gh[2], gh[3]);
            // the first sample that contradicts the hypothesis: sought only in a wave that has one
            const float px = pk4.x * g.x, py = pk4.y * g.y, pz = pk4.z * g.z, pw = pk4.w * g.w;
            const bool hit = valid && fmaxf(fmaxf(px, py), fmaxf(pz, pw)) > thr;
            if (__ballot(hit) != 0ull && hit) {
              if (pw > thr) kfirst = 4 * t + 3;
              if (pz > thr) kfirst = 4 * t + 2;
              if (py > thr) kfirst = 4 * t + 1;
              if (px > thr) kfirst = 4 * t + 0;
            }
            if (4 * t + 4 == cnt) misc[8] = g.w;  // gain of the chunk's last sample under the hypothesis
          }
          const unsigned long long any = __ballot(kfirst != kBig);
          if (lane == 0) misc[wave] = __int_as_float(any ? __builtin_amdgcn_readlane(kfirst, __builtin_ctzll(any)) : kBig);
        }
        __syncthreads();
        int kf = __float_as_int(misc[0]);
        kf = min(kf, __float_as_int(misc[1]));
        kf = min(kf, __float_as_int(misc[2]));
        kf = min(kf, __float_as_int(misc[3]));
        if (kf == kBig) {  // the hypothesis holds for the rest of the chunk
          g_cur[j] = misc[8];
          n_st[j] = n_st[j] + (cnt - 64 * bs) < n_end ? n_st[j] + (cnt - 64 * bs) : n_end;
          break;
        }
        const int b0 = kf >> 6;
        if (wave == cw) {
          int ln = n_st[j] + 64 * (b0 - bs) < n_end ? n_st[j] + 64 * (b0 - bs) : n_end;
          float lgs = gs[j], lge = ge[j], lgl = g_cur[j];
          const int be = limiter_wave(arr_p, arr_g, look, b0, nblk, ln, lgs, lge, lgl, thr, n_atk, n_end, true);
          if (lane == 0) {
            misc[4] = lgl;
            misc[5] = lgs;
            misc[6] = lge;
            misc[7] = __int_as_float(ln);
            misc[9] = __int_as_float(be);
          }
        }
        __syncthreads();
        const int be = __float_as_int(misc[9]);
        if (4 * t >= 64 * b0 && 4 * t < 64 * be) g = *reinterpret_cast<const float4 *>(&arr_g[4 * t]);
        g_cur[j] = misc[4];
        gs[j] = misc[5];
        ge[j] = misc[6];
        n_st[j] = __float_as_int(misc[7]);
        bs = be;
        if (bs >= nblk) break;
      }

      if (c0 + kFChunk < p.total) fetch_window(j, n_st[j]);  // for the next chunk, ahead of the stores

      // ---- emit 4 delayed samples * gain as interleaved PCM in the member's format ----
      const int64_t j0 = gk - kDelay;
      if (valid && j0 >= 0) {
        const int fmt = mb.out_format;
        const int bytes = fmt == IAMF_HIP_FMT_S16 ? 2 : (fmt == IAMF_HIP_FMT_S24 ? 3 : 4);
        float4 o[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float4 d = *reinterpret_cast<const float4 *>(&ring_y[c * R + rd]);   // (c >= oc: not used)
          o[c] = make_float4(d.x * g.x, d.y * g.y, d.z * g.z, d.w * g.w);
        }
        uint8_t *dst = mb.pcm + (int64_t)s * mb.pcm_stream_stride + (j0 - out_base) * (int64_t)oc * bytes;
        if (fmt == IAMF_HIP_FMT_S16) {
          int v[2][4];
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            v[c][0] = (int)to_scaled(o[c].x, 32768.f, -32768.f, 32767.f);
            v[c][1] = (int)to_scaled(o[c].y, 32768.f, -32768.f, 32767.f);
            v[c][2] = (int)to_scaled(o[c].z, 32768.f, -32768.f, 32767.f);
            v[c][3] = (int)to_scaled(o[c].w, 32768.f, -32768.f, 32767.f);
          }
          if (oc == 2) {
            uint4 w;
            w.x = (uint32_t)(v[0][0] & 0xffff) | ((uint32_t)v[1][0] << 16);
            w.y = (uint32_t)(v[0][1] & 0xffff) | ((uint32_t)v[1][1] << 16);
            w.z = (uint32_t)(v[0][2] & 0xffff) | ((uint32_t)v[1][2] << 16);
            w.w = (uint32_t)(v[0][3] & 0xffff) | ((uint32_t)v[1][3] << 16);
            *reinterpret_cast<uint4 *>(dst) = w;
          } else {
            uint2 w;
            w.x = (uint32_t)(v[0][0] & 0xffff) | ((uint32_t)v[0][1] << 16);
            w.y = (uint32_t)(v[0][2] & 0xffff) | ((uint32_t)v[0][3] << 16);
            *reinterpret_cast<uint2 *>(dst) = w;
          }
        } else if (fmt == IAMF_HIP_FMT_S24) {
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            if (c < oc) {
              const float ov[4] = {o[c].x, o[c].y, o[c].z, o[c].w};
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int vv = (int)to_scaled(ov[i], 8388608.f, -8388608.f, 8388607.f);
                uint8_t *d3 = dst + (i * oc + c) * 3;
                d3[0] = (uint8_t)(vv & 0xff);
                d3[1] = (uint8_t)((vv >> 8) & 0xff);
                d3[2] = (uint8_t)(((vv >> 16) & 0x7f) | ((vv >> 24) & 0x80));
              }
            }
          }
        } else if (fmt == IAMF_HIP_FMT_S32) {
          int32_t *d32 = reinterpret_cast<int32_t *>(dst);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            if (c < oc) {
              const float ov[4] = {o[c].x, o[c].y, o[c].z, o[c].w};
#pragma unroll
              for (int i = 0; i < 4; ++i)
                d32[i * oc + c] = (int32_t)(long long)to_scaled(ov[i], 2147483648.f, -2147483648.f, 2147483647.f);
            }
          }
        } else {
          float *df = reinterpret_cast<float *>(dst);
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            if (c < oc) {
              df[0 * oc + c] = o[c].x;
              df[1 * oc + c] = o[c].y;
              df[2 * oc + c] = o[c].z;
              df[3 * oc + c] = o[c].w;
            }
          }
        }
      }
    }
    base = base + cnt >= R ? base + cnt - R : base + cnt;
    __syncthreads();  // ring / arr slots are rewritten by the next chunk
  }

  // ---- persist every member's stream state (same format as the generic kernel) ----
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const FanMember &mb = p.mem[j];
    const float *my = lds + j * MB;
    const int oc = mb.out_ch;
    float *sy = mb.ring_y + (int64_t)s * oc * kSave;
    float *spm = mb.ring_pm + (int64_t)s * kSave;
    const int rp = ring_wrap(base - kSave + t);  // base = ring position of sample pos0 + total
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (c < oc) sy[c * kSave + t] = my[c * R + rp];
    spm[t] = my[oPm + ((p.total + t) & (kSave - 1))];   // sample total - 256 + t of the call
    if (t == 0) {
      LimState o;
      o.g = g_cur[j];
      o.gs = gs[j];
      o.ge = ge[j];
      o.n = n_st[j];
      mb.lim[s] = o;
    }
  }
}
