// render_fanout_pk_unit.hpp — what the three units that instantiate render_fanout_kernel<M, K, true, LPB, LPC> share
// (iamf_render_fanout_pk24.hip, _fanout_pk16c.hip, _fanout_pk24c.hip): the launcher over one form's (M, K) list.  Included
// inside the unit's namespace, behind render_fanout.hpp.  One unit per form, so that the forms build in parallel; the
// existing fan-out units instantiate nothing of this and their code generation does not move.
#pragma once

// LDS per workgroup is the f32-fed form's (fan_lds_floats): two, two, one workgroup per CU for K = 2 / 3 / 4
template <int LPB, bool LPC, int M, int K>
void launch_fan_pk_mk(const FanLpParams &p, hipStream_t st) {
  static_assert(FanK::has(K) && K <= kFanMax, "K lies inside FanK");
  static_assert(LPC ? LpcmCoupledM::has(M) && M != 2 : LpcmM::has(M), "an element shape the form's single call takes, stereo left out");
  constexpr size_t lds = sizeof(float) * (size_t)fan_lds_floats(K, M);
  launch_big_lds<&render_fanout_kernel<M, K, true, LPB, LPC>, (int)lds>(dim3((unsigned)p.n_launch), dim3(256), lds, st, p);
}

// 1 if it launched, 0 if (m, k) is not in the form's list or the block is not one the kernel takes
template <int LPB, bool LPC, class MK>
int fan_pk_launch(MK, const void *params, int m, int k, hipStream_t st) {
  FanLpParams p;
  memcpy(&p, params, sizeof(p));
  if (!p.lpcm || p.n_launch <= 0 || m < 0 || k < 0) return 0;
  for (int j = 0; j < k && j < kFanMax; ++j)
    if (p.mem[j].out_ch < 1 || p.mem[j].out_ch > 2) return 0;
  return dispatch(MK{}, mc(m, k), [&](auto V) { launch_fan_pk_mk<LPB, LPC, mc_m(V.value), mc_c(V.value)>(p, st); });
}
