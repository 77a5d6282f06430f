// lpcm_form.hpp — which packet form of an LPCM call the fused kernels read (render_fast_kernel<.., LP, .., LPB>,
// render_fast.hpp).  Plain C++ like render_route.hpp (included inside the unit's namespace, behind <stdint.h> and
// include/iamf_hip.h), so that tests/route_host can pin the rules without a GPU.  The caller has checked that the layout
// is well-formed (iamf_render.hip, lpcm_form_check: every run inside its packet row); what is decided here is only whether
// a kernel can LOAD the runs as they lie: a contiguous little-endian run per channel, aligned for the lane's one load of
// four consecutive samples.
#pragma once

enum class LpcmForm {
  None,   // not fusable: iamf_hip_lpcm_unpack, then the f32 kernels
  S16,    // 16-bit samples, 8-byte loads
  S24,    // 24-bit samples, 12-byte loads (dword-aligned)
};

// sample bytes of a fusable form (RenderParams::lpcm_bytes), 0 for None
inline int lpcm_form_bytes(LpcmForm f) { return f == LpcmForm::S16 ? 2 : (f == LpcmForm::S24 ? 3 : 0); }

// L: the call's layout of `ch` channels; strides in bytes; raw_bits: the packet buffer's address (its low bits are looked
// at); first: iamf_hip_lpcm_input::first_sample (the kernels start at sample `first` of every run).
inline LpcmForm lpcm_form(const iamf_hip_lpcm_layout &L, int ch, int64_t raw_stream_stride, int64_t raw_frame_stride,
                          uintptr_t raw_bits, int first) {
  if (!L.little_endian || ch > 16 || (raw_bits & 15)) return LpcmForm::None;
  if (L.sample_bytes != 2 && L.sample_bytes != 3) return LpcmForm::None;   // (32 bit: w * 2^-31 can be subnormal)
  const int sb = L.sample_bytes;
  // a lane's four consecutive samples are one load: 8 bytes, 8-byte aligned / 12 bytes, dword-aligned.  With the frame
  // size a multiple of 4, sb * 4 * k keeps the grid; the buffer, the strides and the runs' starts have to be on it.
  const int grid = sb == 2 ? 7 : 3;
  if ((raw_stream_stride & grid) || (raw_frame_stride & grid)) return LpcmForm::None;
  for (int c = 0; c < ch; ++c) {
    if (L.src_offset[c] < 0) return LpcmForm::None;     // a channel no sub-stream carries
    if (L.src_step[c] != sb) return LpcmForm::None;     // coupled sub-streams: samples interleaved
    if ((L.src_offset[c] + sb * first) & grid) return LpcmForm::None;
  }
  return sb == 2 ? LpcmForm::S16 : LpcmForm::S24;
}
