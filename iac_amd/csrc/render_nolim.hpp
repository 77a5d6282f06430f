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
#pragma once

// (kNlChunk, kNlMaxFrameBytes, nolim_shape_ok and nolim_packets_shape_ok, what the kernels' addressing needs: render_route.hpp)

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

template <int M, int LPB, bool LPC>
__device__ __forceinline__ void nolim_load_packets(const RenderParams &p, int s, int f, int i, float4 (&x)[M]) {
  {
    static_assert(LPB == 2 || LPB == 3, "packet samples of 16 or 24 bits");
    const uint8_t *src = p.lpcm + (int64_t)s * p.lpcm_stream_stride + (int64_t)f * p.lpcm_frame_stride;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if (LPC && lpcm_coupled_paired(M, m)) {   // (m is a constant of the unrolled loop)
        if (m & 1) continue;                    // loaded with its partner
        const uint8_t *q = src + p.lpcm_off[m] + 2 * LPB * i;
        float4 &xl = x[m], &xr = x[m + 1 < M ? m + 1 : m];
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
      } else {
        const uint8_t *q = src + p.lpcm_off[m] + LPB * i;
        if constexpr (LPB == 2) {
          const nl_u2 v = *reinterpret_cast<const nl_u2 *>(q);
          x[m] = make_float4(nl_s16(v.a), nl_s16(v.a >> 16), nl_s16(v.b), nl_s16(v.b >> 16));
        } else {
          int u[4];
          nl_cut24(*reinterpret_cast<const nl_u3 *>(q), u);
          x[m] = make_float4(nl_s24(u[0]), nl_s24(u[1]), nl_s24(u[2]), nl_s24(u[3]));
        }
      }
    }
  }
}

// LPB == 0: planar f32 rows (p.in).  LPB == 2 / 3, LPC: the element's LPCM packets (nolim_load_packets; M in LpcmCoupledM with
// LPC, else in LpcmM).  Everything behind the loads is one body.
template <int M, int LPB = 0, bool LPC = false>
__global__ __launch_bounds__(256) void render_nolim_kernel(const RenderParams p) {
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
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float z = v[q];
        if (eg_on) z = z * eg;
        z = 0.f + z;  // iamf_mixer_mix: memset 0 then += (IAMF_decoder.c:2719-2730)
        if (og_on) z = z * og;
        if (lg_on) z = z * lg;
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
