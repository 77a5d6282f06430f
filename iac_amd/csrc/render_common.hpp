// render_common.hpp — what every render translation unit shares: the parameter block (render_params.hpp), the instance
// lists and the routing decision (render_route.hpp), the launch helper for kernels with more than 64 KiB of LDS, and
// small device helpers.  Included inside the unit's anonymous namespace, in front of the kernel headers.
#pragma once

#include "render_params.hpp"
#include "render_route.hpp"

// Opting a kernel into more than 64 KiB of dynamic LDS is a PER-DEVICE attribute: one flag per device
// ordinal, set only when every hipFuncSetAttribute of the group succeeded (a failed opt-in is retried
// and surfaces as a launch error instead of being remembered as done).  Host threads may drive batches on
// different devices at once: the begin..end bracket keeps its device and result per THREAD and only the
// done flags are shared (atomic; opting in twice is harmless).  Ordinals >= kMaxDevices opt in on every launch.
constexpr int kMaxDevices = 64;
struct OptIn {
  std::atomic<bool> done[kMaxDevices] = {};
  struct Bracket {
    int dev;
    bool ok;
  };
  static Bracket &cur() {
    static thread_local Bracket b{0, true};
    return b;
  }
  bool begin() {  // true if this device still has to opt in
    Bracket &b = cur();
    if (hipGetDevice(&b.dev) != hipSuccess || b.dev < 0) b.dev = kMaxDevices;
    b.ok = true;
    return b.dev >= kMaxDevices || !done[b.dev].load(std::memory_order_acquire);
  }
  void set(const void *fn, int bytes) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) cur().ok = false;
  }
  void end() {
    const Bracket &b = cur();
    if (b.dev < kMaxDevices && b.ok) done[b.dev].store(true, std::memory_order_release);
  }
};

// Launches Kernel with `lds` bytes of dynamic LDS, of which it may take up to Cap: more than 64 KiB has to be opted into
// per kernel (gfx950 has 160 KiB per CU).  The opt-in flag belongs to the kernel, so what is opted in is what is launched.
template <auto Kernel, int Cap, class... Args>
void launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args &...args) {
  static OptIn opted;
  if (opted.begin()) {
    opted.set(reinterpret_cast<const void *>(Kernel), Cap);
    opted.end();
  }
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
}

// One gain step evaluated for a hypothetical pre-state n_pre (no trigger since the state was
// set): audio_effect_peak_limiter.c:241-255 with currentTC = T[n_pre].
__device__ __forceinline__ float gain_at(int n_pre, float gs, float ge, float c, int n_atk, int n_end) {
  float g = 1.0f;
  if (n_pre < n_atk) {
    g = gs - c * (gs - ge);
  } else if (n_pre < n_end) {
    g = ge + c * (1.0f - ge);
  }
  return g;
}

__device__ __forceinline__ float to_scaled(float x, float scale, float lo, float hi) {
  x = x * scale;
  x = x > lo ? x : lo;
  x = x < hi ? x : hi;
  return rintf(x);  // v_rndne_f32: ties to even, like lrintf in the default rounding mode
}

// float -> the integer render_wide.hpp and render_wide4.hpp hand to v_cvt_pk_i16 (rint, then saturate == the reference's
// clamp, then lrintf: the bounds are integers).  NaN: the reference's clamp `x > lo ? x : lo` (IAMF_decoder.c:100-119) makes
// it lo, the conversion alone 0; maxnum returns its other operand for a NaN and leaves every other value's result alone.
__device__ __forceinline__ int to_s16_sat(float x) { return (int)rintf(__builtin_fmaxf(x, -32768.f)); }

// Quotients that share a divisor (the demixer of scalable channel audio divides 8 numerators each by delta, beta and
// gamma of the frame: demixer.c:205-214,255-267,357-366).  With r = RN(1 / d) — ONE IEEE division per divisor —
//     q = n * r;  e = fma(-d, q, n);  q' = fma(e, r, q)
// is the correctly rounded n / d, bit for bit, for every f32 numerator with 2^-100 <= |n| < 2^126 and every divisor the
// demixing modes can produce (1, 0.707f, 0.866f: IAMF_utils.c:236-240); outside that range the residual e underflows or
// q overflows, and -0 comes out as +0.  Proven by an exhaustive sweep of all 2^32 numerators per divisor ON THE DEVICE
// (iamf_hip_selftest_shared_divisor, tests/test_gpu_wide4.py) and on the host.  w4_quot returns q' and clears *ok for a
// numerator outside the range; the caller then redoes its divisions the slow way (a wave-uniform, rare branch: digital
// silence takes it).  Three instructions per quotient instead of the ~10 of an IEEE division.
__device__ __forceinline__ float w4_quot(float n, float d, float r, bool &ok) {
  const float an = __builtin_fabsf(n);
  ok = ok && an >= 0x1p-100f && an < 0x1p126f;
  const float q = n * r;
  const float e = __builtin_fmaf(-d, q, n);
  return __builtin_fmaf(e, r, q);
}
