// render_fir_launch.hpp — launchers of the HRTF stage's kernels, shared by the two units that instantiate them:
// iamf_render.hip (ambisonics elements, FirHomeM) and iamf_render_fir_m2b.hip (channel-based ones, FirM2bM).
// Included behind render_fast.hpp.
#pragma once

// render_fast_kernel<M, 2, stage>: stage as fir_stage_choice (3 FFT, 2 split-f16 MFMA, 1 f32 MFMA; the split form, 4, is
// launch_fft_m and the matrix kernel behind it)
template <int M>
void launch_fir_m(const RenderParams &p, int stage, hipStream_t st) {
  const dim3 grid((unsigned)p.n_launch);
  if (stage == 3) {
    static_assert(fast_lds_floats(2, M, 3) * 4 <= 80 * 1024, "two workgroups per CU");
    launch_big_lds<&render_fast_kernel<M, 2, 3>, 120 * 1024>(grid, dim3(256), sizeof(float) * (size_t)fast_lds_floats(2, M, 3), st, p);
  } else if (stage == 2) {
    static_assert(fast_lds_floats(2, M, 2) * 4 <= 80 * 1024, "two workgroups per CU");
    launch_big_lds<&render_fast_kernel<M, 2, 2>, 120 * 1024>(grid, dim3(256), sizeof(float) * (size_t)fast_lds_floats(2, M, 2), st, p);
  } else {
    launch_big_lds<&render_fast_kernel<M, 2, 1>, 120 * 1024>(grid, dim3(512), sizeof(float) * (size_t)fast_lds_floats(2, M, 1), st, p);
  }
}

template <int M>
void launch_fft_m(const RenderParams &p, hipStream_t st) {   // render_fir_fft.hpp: fir_fft_kernel
  const dim3 g((unsigned)((p.total + kFftSpan - 1) / kFftSpan), (unsigned)p.n_launch);
  // (whole frames only: past a call that ends inside a frame the two-base fetch would read what the caller left in the rest
  //  of the frame — harmless to the samples that are kept unless it is a NaN, which a transform spreads over its block)
  if ((M & 1) == 0 && p.fir_pre && p.fir_pre_next && p.total % p.frame_size == 0 && !getenv("IAMF_HIP_FIR_GENERAL_FETCH"))
    hipLaunchKernelGGL((fir_fft_kernel<M, (M & 1) == 0>), g, dim3(256), sizeof(float) * (size_t)kFftLdsFloats, st, p, p.fir_y, 2 * (int64_t)p.total);
  else
    hipLaunchKernelGGL((fir_fft_kernel<M, false>), g, dim3(256), sizeof(float) * (size_t)kFftLdsFloats, st, p, p.fir_y, 2 * (int64_t)p.total);
}
