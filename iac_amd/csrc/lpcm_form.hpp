// lpcm_form.hpp — which packet form of an LPCM call the fused kernels read (render_fast_kernel<.., LP, .., LPB>,
// render_fast.hpp).  Plain C++ like render_route.hpp (included inside the unit's namespace, behind <stdint.h>,
// include/iamf_hip.h and render_route.hpp, whose coupled pairing it asks), so that tests/route_host can pin the rules
// without a GPU.  The caller has checked that the layout is well-formed (iamf_render.hip, lpcm_form_check: every run
// inside its packet row); what is decided here is only whether
// a kernel can LOAD the runs as they lie: a contiguous little-endian run per channel, aligned for the lane's one load of
// four consecutive samples — or, for the coupled form, a pair of channels interleaved sample by sample, aligned for the
// lane's one load of four consecutive sample pairs.
#pragma once

enum class LpcmForm {
  None,   // not fusable: iamf_hip_lpcm_unpack, then the f32 kernels
  S16,    // 16-bit samples, 8-byte loads
  S24,    // 24-bit samples, 12-byte loads (dword-aligned)
  S16C,   // 16-bit samples, the loudspeaker layouts' canonical coupling: pairs interleaved sample by sample (16-byte loads,
          // 8-byte aligned), C and LFE mono runs as S16
  S24C,   // 24-bit samples, the same coupling: a pair's four sample-frames are 24 bytes on the dword grid (two 12-byte loads), C
          // and LFE mono runs as S24.  Answered by lpcm_form_packets() only (iamf_hip_batch_render_packets): lpcm_form() keeps
          // None for such packets, and with it every entry that asks lpcm_form() its route
};

// sample bytes of a fusable form (RenderParams::lpcm_bytes), 0 for None
inline int lpcm_form_bytes(LpcmForm f) {
  return (f == LpcmForm::S16 || f == LpcmForm::S16C) ? 2 : ((f == LpcmForm::S24 || f == LpcmForm::S24C) ? 3 : 0);
}

// S16C: every pair of lpcm_coupled_paired() (render_route.hpp) is ONE run of interleaved samples (step 4, the partner 2 bytes on) whose
// lane quads — 16 bytes — start on the 8-byte grid; channels 2 and 3 are mono runs under the S16 rule.
inline bool lpcm_form_coupled(const iamf_hip_lpcm_layout &L, int ch, int first) {
  if (!lpcm_coupled_m(ch)) return false;
  for (int c = 0; c < ch; ++c) {
    if (L.src_offset[c] < 0) return false;              // a channel no sub-stream carries
    if (!lpcm_coupled_paired(ch, c)) {
      if (L.src_step[c] != 2 || ((L.src_offset[c] + 2 * first) & 7)) return false;
    } else if (!(c & 1)) {
      if (L.src_step[c] != 4 || L.src_step[c + 1] != 4) return false;
      if (L.src_offset[c + 1] != L.src_offset[c] + 2) return false;
      if ((L.src_offset[c] + 4 * first) & 7) return false;
    }
  }
  return true;
}

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
  // 16-bit packets of a loudspeaker layout's channel count: the coupled form or none (no kernel is built for such an element
  // coded as mono sub-streams or paired otherwise: it is unpacked)
  if (sb == 2 && lpcm_coupled_m(ch)) return lpcm_form_coupled(L, ch, first) ? LpcmForm::S16C : LpcmForm::None;
  for (int c = 0; c < ch; ++c) {
    if (L.src_offset[c] < 0) return LpcmForm::None;     // a channel no sub-stream carries
    if (L.src_step[c] != sb) return LpcmForm::None;     // coupled sub-streams other than S16C's: samples interleaved
    if ((L.src_offset[c] + sb * first) & grid) return LpcmForm::None;
  }
  return sb == 2 ? LpcmForm::S16 : LpcmForm::S24;
}

// S24C: every pair of lpcm_coupled_paired() is ONE run of interleaved 24-bit samples (step 6, the partner 3 bytes on) whose
// lane quads — 24 bytes at 6 * i, i a multiple of 4 — start on the dword grid; channels 2 and 3 are mono runs under the S24
// rule.  Any other 24-bit pairing (six mono runs, a pair on (1,2), step 6 with the partner elsewhere) is no form.
inline bool lpcm_form_coupled24(const iamf_hip_lpcm_layout &L, int ch, int first) {
  if (!lpcm_coupled_m(ch)) return false;
  for (int c = 0; c < ch; ++c) {
    if (L.src_offset[c] < 0) return false;              // a channel no sub-stream carries
    if (!lpcm_coupled_paired(ch, c)) {
      if (L.src_step[c] != 3 || ((L.src_offset[c] + 3 * first) & 3)) return false;
    } else if (!(c & 1)) {
      if (L.src_step[c] != 6 || L.src_step[c + 1] != 6) return false;
      if (L.src_offset[c + 1] != L.src_offset[c] + 3) return false;
      if ((L.src_offset[c] + 6 * first) & 3) return false;
    }
  }
  return true;
}

// What iamf_hip_batch_render_packets asks: lpcm_form()'s answer where that is a form, else S24C where its rules hold —
// little-endian 24-bit samples of a loudspeaker layout's channel count, d_raw 16-byte aligned, both strides on the dword
// grid, the layout as lpcm_form_coupled24() says.  The same arguments as lpcm_form().
inline LpcmForm lpcm_form_packets(const iamf_hip_lpcm_layout &L, int ch, int64_t raw_stream_stride, int64_t raw_frame_stride,
                                  uintptr_t raw_bits, int first) {
  const LpcmForm f = lpcm_form(L, ch, raw_stream_stride, raw_frame_stride, raw_bits, first);
  if (f != LpcmForm::None) return f;
  if (!L.little_endian || L.sample_bytes != 3 || (raw_bits & 15) || (raw_stream_stride & 3) || (raw_frame_stride & 3)) return LpcmForm::None;
  return lpcm_form_coupled24(L, ch, first) ? LpcmForm::S24C : LpcmForm::None;
}
