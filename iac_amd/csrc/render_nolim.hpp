// render_nolim.hpp — the element renderer WITHOUT the peak limiter (IAMF_decoder_peak_limiter_enable(handle, 0), the
// player's -disable_limiter; also the first of the three launches of a rate-converting stream: render -> iamf_resample ->
// limiter, IAMF_decoder.c:3459-3500, and a second element's batch).  With the limiter off there is no delay line and no
// state: every (stream, sample) is independent.  The general kernel serves it one sample per lane with element-wise
// stores (TOA -> stereo 45, 7.1.4 -> J 28 Gsamples/s, tools/debug/shape_cliff_probe.py); this one takes the plain case —
// one matrix-rendered element, constant gains — four consecutive samples per lane (16-byte loads), the workgroup's 1024
// sample-frames packed in LDS in the output format and written as one contiguous run of 16-byte pieces.
// The same operations in the same order as render_kernel<M> (render_generic.hpp): acc from 0 over the inputs in order,
// element gain, `0.f + y` (iamf_mixer_mix), output gain, loudness gain, the format's conversion.
// One kernel template, two input forms: render_nolim_kernel<M> reads planar f32 rows, render_nolim_kernel<M, LPB, LPC> the
// element's LPCM packets as they lie (iamf_render_nolim_packets*.hip).  Only the loads differ (nolim_load_packets).
// A third form, render_nolim_kernel<M, LPB, LPC, LP2>, mixes a SECOND element's packets in (iamf_render_nolim_packets*_mix.hip):
// a bed plus dialogue or commentary on a batch without the limiter.  It takes RenderMixParams, loads element 1 beside element 0
// (nolim_load_packets2) and runs the general kernel's mixing steps, operation for operation (render_generic.hpp): element 0's
// ramp or gain, `0.f + y`, element 1's acc from 0, its ramp or gain, `y + y2`, the output ramp or gain, the loudness gain.  The
// three per-sample ramps are optional per call: wave-uniform run-time branches, one float4 per lane where given.
#pragma once

// (kNlChunk, kNlMaxFrameBytes, nolim_shape_ok, nolim_packets_shape_ok and nolim_packets_mix_shape_ok, what the kernels'
//  addressing needs: render_route.hpp)

// The lane's four samples of the M inputs, frame f, position i (a multiple of 4) -> x, from LPCM packets
// LPB == 2 / 3: LPCM packets (p.lpcm) of 16-bit / 24-bit little-endian samples in one of the four single-element shapes of
// lpcm_form.hpp, p.lpcm_off[m] = src_offset + src_step * first_sample.  A mono run: 8 / 12 bytes at lpcm_off[m] + LPB * i.  LPC, the
// pairs of lpcm_coupled_paired(M, m): ONE run of interleaved samples per pair, 16 bytes / 2 x 12 bytes at lpcm_off[m] + 2 * LPB * i,
// loaded when the pair's first channel is named; C and LFE are mono runs.  Conversion: (float)sample * (1 / 32768) or * (1 /
// 8388608) — the expression of iamf_hip_lpcm_unpack (iamf_unpack.hip) and of the reference (pcm/IAMF_pcm_decoder.c:64-83), NOT
// folded into the weights: every product behind it is the f32 path's product.
// The loads are as wide as the shape's own grid allows (lpcm_form.hpp): 8-byte aligned for 16-bit samples, dword-aligned for
// 24-bit ones, hence the element types below.
struct alignas(8) nl_u2 {
  unsigned a, b;
};
struct alignas(4) nl_u3 {
  unsigned a, b, c;
};
struct alignas(8) nl_u4 {
  unsigned a, b, c, d;
};
__device__ __forceinline__ float nl_s16(unsigned half) { return (float)(int)(short)half * (1.0f / 32768.0f); }
__device__ __forceinline__ float nl_s24(int sample) { return (float)sample * (1.0f / 8388608.0f); }
// four 24-bit samples in three dwords — a[23:0], {b[15:0], a[31:24]}, {c[7:0], b[31:16]}, c[31:8] — sign-extended
__device__ __forceinline__ void nl_cut24(const nl_u3 &v, int (&s)[4]) {
  s[0] = (int)(v.a << 8) >> 8;
  s[1] = (int)(__builtin_amdgcn_alignbit(v.b, v.a, 24) << 8) >> 8;
  s[2] = (int)(__builtin_amdgcn_alignbit(v.c, v.b, 16) << 8) >> 8;
  s[3] = (int)v.c >> 8;
}

// one mono run's quad at q -> x; one coupled pair's quad at q -> xl, xr
template <int LPB>
__device__ __forceinline__ void nl_load_run(const uint8_t *q, float4 &x) {
  if constexpr (LPB == 2) {
    const nl_u2 v = *reinterpret_cast<const nl_u2 *>(q);
    x = make_float4(nl_s16(v.a), nl_s16(v.a >> 16), nl_s16(v.b), nl_s16(v.b >> 16));
  } else {
    int u[4];
    nl_cut24(*reinterpret_cast<const nl_u3 *>(q), u);
    x = make_float4(nl_s24(u[0]), nl_s24(u[1]), nl_s24(u[2]), nl_s24(u[3]));
  }
}
template <int LPB>
__device__ __forceinline__ void nl_load_pair(const uint8_t *q, float4 &xl, float4 &xr) {
  if constexpr (LPB == 2) {   // {L0:R0} .. {L3:R3}: L the low halves, R the high ones
    const nl_u4 v = *reinterpret_cast<const nl_u4 *>(q);
    xl = make_float4(nl_s16(v.a), nl_s16(v.b), nl_s16(v.c), nl_s16(v.d));
    xr = make_float4(nl_s16(v.a >> 16), nl_s16(v.b >> 16), nl_s16(v.c >> 16), nl_s16(v.d >> 16));
  } else {                    // L0 R0 L1 R1 | L2 R2 L3 R3: L takes samples 0 and 2 of each triple, R 1 and 3
    int u[4], w[4];
    nl_cut24(*reinterpret_cast<const nl_u3 *>(q), u);
    nl_cut24(*reinterpret_cast<const nl_u3 *>(q + 12), w);
    xl = make_float4(nl_s24(u[0]), nl_s24(u[2]), nl_s24(w[0]), nl_s24(w[2]));
    xr = make_float4(nl_s24(u[1]), nl_s24(u[3]), nl_s24(w[1]), nl_s24(w[3]));
  }
}

template <int M, int LPB, bool LPC>
__device__ __forceinline__ void nolim_load_packets(const RenderParams &p, int s, int f, int i, float4 (&x)[M]) {
  static_assert(LPB == 2 || LPB == 3, "packet samples of 16 or 24 bits");
  const uint8_t *src = p.lpcm + (int64_t)s * p.lpcm_stream_stride + (int64_t)f * p.lpcm_frame_stride;
#pragma unroll
  for (int m = 0; m < M; ++m) {
    if (LPC && lpcm_coupled_paired(M, m)) {   // (m is a constant of the unrolled loop)
      if (m & 1) continue;                    // loaded with its partner
      nl_load_pair<LPB>(src + p.lpcm_off[m] + 2 * LPB * i, x[m], x[m + 1 < M ? m + 1 : m]);
    } else {
      nl_load_run<LPB>(src + p.lpcm_off[m] + LPB * i, x[m]);
    }
  }
}

// The same for the SECOND element of a mix (RenderMixParams: lpcm2, its strides in bytes, lpcm2_off = src_offset + src_step *
// first_sample), of element 0's sample size.  LP2 == 1: p.m2 = 1 or 4 mono runs (a wave-uniform run-time value: the runs a
// one-channel element does not have are not read), 8 / 12 bytes at lpcm2_off[m] + LPB * i.  LP2 == 2: ONE coupled stereo pair,
// 16 bytes / 2 x 12 bytes at lpcm2_off[0] + 2 * LPB * i, cut exactly as nolim_load_packets cuts a pair.
template <int LPB, int LP2>
__device__ __forceinline__ void nolim_load_packets2(const RenderMixParams &p, int s, int f, int i, float4 (&x2)[LP2 == 2 ? 2 : 4]) {
  static_assert(LP2 == 1 || LP2 == 2, "mono-coded runs or one coupled pair");
  const uint8_t *src = p.lpcm2 + (int64_t)s * p.lpcm2_stream_stride + (int64_t)f * p.lpcm2_frame_stride;
  if constexpr (LP2 == 2) {
    nl_load_pair<LPB>(src + p.lpcm2_off[0] + 2 * LPB * i, x2[0], x2[1]);
  } else {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      x2[m] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (m < p.m2) nl_load_run<LPB>(src + p.lpcm2_off[m] + LPB * i, x2[m]);
    }
  }
}

// the parameter block of an instance: the second element's packets travel behind RenderParams
template <int LP2>
struct NlParams {
  using type = RenderMixParams;
};
template <>
struct NlParams<0> {
  using type = RenderParams;
};

// LPB == 0: planar f32 rows (p.in).  LPB == 2 / 3, LPC: the element's LPCM packets (nolim_load_packets; M in LpcmCoupledM with
// LPC, else in LpcmM).  Everything behind the loads is one body.  LP2 == 1 / 2 (with LPB != 0): a second element's packets are
// mixed in (nolim_load_packets2) and the three ramps apply where the call gives them; LP2 == 0 is the body as it stood.
template <int M, int LPB = 0, bool LPC = false, int LP2 = 0>
__global__ __launch_bounds__(256) void render_nolim_kernel(const typename NlParams<LP2>::type p) {
  static_assert(LP2 == 0 || LPB != 0, "a second element comes as packets beside a packet-fed element 0");
  extern __shared__ float nl_lds[];
  uint8_t *tile = reinterpret_cast<uint8_t *>(nl_lds);   // [1024 sample-frames][out_ch * bytes]
  const int s = blockIdx.x + p.stream0;
  const int t = threadIdx.x;
  const int fs = p.frame_size, oc = p.out_ch;
  const int bytes = p.out_format == IAMF_HIP_FMT_S16 ? 2 : (p.out_format == IAMF_HIP_FMT_S24 ? 3 : 4);
  const int c0 = (int)blockIdx.y * kNlChunk;
  const int k = c0 + 4 * t;          // this lane's first sample of the call
  const bool valid = k < p.total;    // total % 4 == 0: all four or none
  const float eg = p.gains[s], og = p.gains[p.n_streams + s], lg = p.gains[2 * p.n_streams + s];
  const bool eg_on = (eg != 1.f && eg > 0.f);
  const bool og_on = (og != 1.f && og > 0.f);
  const bool lg_on = p.loudness_on && (lg != 1.0f);
  if constexpr (LP2 != 0) {
    // The stream state a mixing call leaves behind.  What such a call ran before — the general kernel, render_generic.hpp —
    // persists its LDS ring whether the limiter is on or not: ring_y[s][c][e], e < kSave, the last kSave rendered samples of the
    // stream (entry e is sample total - kSave + e of the call, or, in a call shorter than kSave, what was saved before, moved up
    // by `total`), and ring_pm[s][e], which no limiter-off call writes: the ring's slot of that sample, a zero where the slot
    // was cleared at the call's start ((total - kSave + e) mod kRing < kSave), else the entry saved before that the slot held.
    // The state exported behind the call is that kernel's, bit for bit; LimState is written back as read.  The samples' own
    // entries are stored where they are computed, below.  (One workgroup per stream does this: chunk 0, and a call shorter
    // than kSave has no other.  The tile is free until the projection fills it: kSave floats per channel fit, oc * bytes >= 4.)
    if (blockIdx.y == 0) {
      float *sy = p.ring_y + (int64_t)s * oc * kSave;
      float *spm = p.ring_pm + (int64_t)s * kSave;
      const int d = (p.total - kSave + t) & (kRing - 1);
      const float pm_keep = d < kSave ? 0.f : spm[d - kSave];
      if (p.total < kSave) {   // wave-uniform
        float *stage = nl_lds;
        for (int c = 0; c < oc; ++c) stage[c * kSave + t] = sy[c * kSave + t];
        __syncthreads();
        if (t + p.total < kSave)
          for (int c = 0; c < oc; ++c) sy[c * kSave + t] = stage[c * kSave + t + p.total];
      }
      __syncthreads();
      spm[t] = pm_keep;
      __syncthreads();   // the staged entries are read before the tile is written
    }
  }
  float4 x[M];
  if (valid) {
    const int f = k / fs, i = k - f * fs;   // fs % 4 == 0: the four samples lie in one frame
    if constexpr (LPB == 0) {
      const float *src = p.in + (int64_t)s * p.in_stream_stride + (int64_t)f * p.in_frame_stride + i;
#pragma unroll
      for (int m = 0; m < M; ++m) x[m] = *reinterpret_cast<const float4 *>(src + (int64_t)m * fs);
    } else {
      nolim_load_packets<M, LPB, LPC>(p, s, f, i, x);
    }
    // the second element's quad, its constant gain and the call's ramps: one float4 each at ramp + s * ramp_stream_stride + k
    // (k a multiple of 4 below total: no float behind the call's last sample is read)
    float4 x2[LP2 == 2 ? 2 : 4];
    float er[4], er2[4], orr[4];
    float eg2 = 1.f;
    if constexpr (LP2 != 0) {
      nolim_load_packets2<LPB, LP2>(p, s, f, i, x2);
      eg2 = p.gains2[s];
      const int64_t ro = (int64_t)s * p.ramp_stream_stride + k;
      const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
      const float4 r0 = p.elem_ramp ? *reinterpret_cast<const float4 *>(p.elem_ramp + ro) : one;
      const float4 r1 = p.elem2_ramp ? *reinterpret_cast<const float4 *>(p.elem2_ramp + ro) : one;
      const float4 r2 = p.out_ramp ? *reinterpret_cast<const float4 *>(p.out_ramp + ro) : one;
      er[0] = r0.x, er[1] = r0.y, er[2] = r0.z, er[3] = r0.w;
      er2[0] = r1.x, er2[1] = r1.y, er2[2] = r1.z, er2[3] = r1.w;
      orr[0] = r2.x, orr[1] = r2.y, orr[2] = r2.z, orr[3] = r2.w;
    }
    uint8_t *mine = tile + (size_t)(4 * t) * oc * bytes;
    for (int c = 0; c < oc; ++c) {
      const int fd = p.src_feed[c];
      float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (fd >= 0) {
        const float *row = p.matrix + fd * M;  // wave-uniform -> scalar loads
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int m = 0; m < M; ++m) {
          acc.x = acc.x + row[m] * x[m].x;
          acc.y = acc.y + row[m] * x[m].y;
          acc.z = acc.z + row[m] * x[m].z;
          acc.w = acc.w + row[m] * x[m].w;
        }
        y = acc;
      }
      float v[4] = {y.x, y.y, y.z, y.w};
      float v2[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (LP2 != 0) {   // element 1: acc2 from 0 over its m2 inputs in order
        const int fd2 = p.src_feed2[c];
        if (fd2 >= 0) {
          const float *row2 = p.matrix2 + fd2 * p.m2;
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int m = 0; m < (LP2 == 2 ? 2 : 4); ++m) {
            if (LP2 == 2 || m < p.m2) {
              acc.x = acc.x + row2[m] * x2[m].x;
              acc.y = acc.y + row2[m] * x2[m].y;
              acc.z = acc.z + row2[m] * x2[m].z;
              acc.w = acc.w + row2[m] * x2[m].w;
            }
          }
          v2[0] = acc.x, v2[1] = acc.y, v2[2] = acc.z, v2[3] = acc.w;
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z = v[q];
        if constexpr (LP2 != 0) {
          if (p.elem_ramp) {
            z = z * er[q];  // iamf_frame_gain with a gains[] array: unconditional (IAMF_decoder.c:1401-1405)
          } else if (eg_on) {
            z = z * eg;
          }
        } else {
          if (eg_on) z = z * eg;
        }
        z = 0.f + z;  // iamf_mixer_mix: memset 0 then += (IAMF_decoder.c:2719-2730)
        if constexpr (LP2 != 0) {
          float z2 = v2[q];
          if (p.elem2_ramp) {
            z2 = z2 * er2[q];
          } else if (eg2 != 1.f && eg2 > 0.f) {
            z2 = z2 * eg2;
          }
          z = z + z2;
          if (p.out_ramp) {
            z = z * orr[q];
          } else if (og_on) {
            z = z * og;
          }
        } else {
          if (og_on) z = z * og;
        }
        if (lg_on) z = z * lg;
        if constexpr (LP2 != 0) {   // one of the call's last kSave samples: its entry of the saved ring (above)
          const int e = k + q - (p.total - kSave);
          if (e >= 0) p.ring_y[((int64_t)s * oc + c) * kSave + e] = z;
        }
        uint8_t *d = mine + (size_t)(q * oc + c) * bytes;
        if (p.out_format == IAMF_HIP_FMT_S16) {
          *reinterpret_cast<int16_t *>(d) = (int16_t)(int)to_scaled(z, 32768.f, -32768.f, 32767.f);
        } else if (p.out_format == IAMF_HIP_FMT_S24) {
          const int w = (int)to_scaled(z, 8388608.f, -8388608.f, 8388607.f);
          d[0] = (uint8_t)(w & 0xff);
          d[1] = (uint8_t)((w >> 8) & 0xff);
          d[2] = (uint8_t)(((w >> 16) & 0x7f) | ((w >> 24) & 0x80));
        } else if (p.out_format == IAMF_HIP_FMT_S32) {
          // +full scale wraps to INT32_MIN as in the reference (IAMF_decoder.c:114-119)
          *reinterpret_cast<int32_t *>(d) = (int32_t)(long long)to_scaled(z, 2147483648.f, -2147483648.f, 2147483647.f);
        } else {
          *reinterpret_cast<float *>(d) = z;
        }
      }
    }
  }
  __syncthreads();
  // the tile's valid part -> PCM, 16 bytes per lane and round: one contiguous run
  const int n_here = p.total - c0 < kNlChunk ? p.total - c0 : kNlChunk;
  const int pieces = (n_here * oc * bytes) >> 4;   // (n_here % 4 == 0 and out_ch * bytes % 4 == 0: whole pieces)
  uint8_t *dst = p.pcm + (int64_t)s * p.pcm_stream_stride + (int64_t)c0 * oc * bytes;
  using u4 = __attribute__((ext_vector_type(4))) unsigned;
  for (int q = t; q < pieces; q += 256) *reinterpret_cast<u4 *>(dst + (size_t)q * 16) = *reinterpret_cast<const u4 *>(tile + (size_t)q * 16);
}
