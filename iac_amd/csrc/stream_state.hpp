// stream_state.hpp — the per-stream lifecycle kernels: restart, export and import of ONE stream's persisted state next to
// running neighbours (iamf_hip_batch_restart_range / _set_gains_range / _export_range / _import_range and the resampler's
// counterparts).  Like every render_*.hpp it is included INSIDE the including unit's anonymous namespace.
//
// One list of fields describes what a stream persists between calls: where a field lies, how many floats of it belong to
// one stream, what a fresh stream holds there and whether it travels in an exported blob.  The three jobs walk the SAME
// list, so a field that is added to the list is restarted, exported and imported, or none of them.
//
// Not render kernels: they go through neither launch() nor the instance listing (as lpcm_unpack_kernel and
// restride_kernel).  One workgroup of 256 lanes per stream of the range; rows whose start and length are multiples of
// 16 bytes (the ring rows: kSave = 256 floats) move 16 bytes per lane, everything else one float per lane.
#pragma once

constexpr int kStateMaxFields = 16;
constexpr int kStateChunk = 64;        // streams of one launch whose per-stream values travel in the kernel arguments
constexpr uint32_t kStateMagic = 0x53534149u;   // "IASS"
constexpr uint32_t kStateVersion = 1;

enum { kFreshZero = 0, kFreshLim = 1, kFreshValue = 2 };

struct StateField {
  float *ptr;            // device; nullptr = this batch does not have the field
  // stream s starts at ptr + (s / group) * group_stride + (s % group) * stream_stride; its `rows` rows of `row_floats`
  // floats lie `row_stride` floats apart.  A plain [n_streams][floats] array: group 1, group_stride = floats, one row.
  int64_t group_stride;
  int32_t group, stream_stride;
  int32_t rows, row_floats, row_stride;
  int32_t vec;           // every row starts on a 16-byte boundary and is a multiple of 16 bytes long
  int32_t fresh;         // what a fresh stream holds: kFreshZero, kFreshLim (LimState {1, -1, -1, lim_n}), kFreshValue
  int32_t value_row;     // kFreshValue: the row of StateValues the stream's value comes from
  int32_t blob_off;      // floats from the start of the stream's blob, a multiple of 4; -1 = restart only
};

struct StateFields {
  StateField f[kStateMaxFields];
  int32_t n;
  int32_t lim_n;         // LimState::n of a fresh stream (n_end: idle)
};

struct StateValues {     // restart: per-stream values of the launch's streams (the gains)
  float v[4][kStateChunk];
};

// ---- host: building the list ----

inline void state_add_rows(StateFields &fl, float *ptr, int group, int64_t group_stride, int stream_stride, int rows,
                           int row_floats, int row_stride, int fresh, int value_row, bool in_blob) {
  StateField &f = fl.f[fl.n++];
  f.ptr = ptr;
  f.group_stride = group_stride;
  f.group = group;
  f.stream_stride = stream_stride;
  f.rows = rows;
  f.row_floats = row_floats;
  f.row_stride = row_stride;
  f.vec = ((reinterpret_cast<uintptr_t>(ptr) & 15) == 0 && (group_stride & 3) == 0 && (stream_stride & 3) == 0 &&
           (row_floats & 3) == 0 && (row_stride & 3) == 0)
              ? 1
              : 0;
  f.fresh = fresh;
  f.value_row = value_row;
  f.blob_off = in_blob ? 0 : -1;   // state_layout() places it
}

// a plain [n_streams][floats] array
inline void state_add(StateFields &fl, float *ptr, int floats, int fresh, int value_row, bool in_blob) {
  state_add_rows(fl, ptr, 1, floats, 0, 1, floats, floats, fresh, value_row, in_blob);
}

// places the blob's fields (each on a 16-byte boundary, absent ones take no room) and returns the blob's bytes per stream
inline int64_t state_layout(StateFields &fl) {
  int64_t off = 0;
  for (int i = 0; i < fl.n; ++i) {
    StateField &f = fl.f[i];
    if (f.blob_off < 0 || !f.ptr) continue;
    f.blob_off = (int32_t)off;
    off += ((int64_t)f.rows * f.row_floats + 3) & ~(int64_t)3;
  }
  return off * (int64_t)sizeof(float);
}

// FNV-1a over 32-bit words: the ticket's signature
inline uint32_t state_hash(const uint32_t *w, int n) {
  uint32_t h = 2166136261u;
  for (int i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) {
      h ^= (w[i] >> (8 * b)) & 0xffu;
      h *= 16777619u;
    }
  return h;
}

// ---- device ----

enum class StateJob { Restart, Export, Import };

// Workgroup i serves stream stream0 + i; its blob lies at blob + i * blob_stride (floats, a multiple of 4; blob 16-byte
// aligned).  Bit k of `mask`: field k takes part.  Every lane of a workgroup walks the same fields (uniform branches).
template <StateJob J>
__global__ __launch_bounds__(256) void stream_state_kernel(StateFields fl, uint32_t mask, int stream0, float *blob,
                                                           int64_t blob_stride, StateValues vals) {
  const int i = blockIdx.x, s = stream0 + i, t = threadIdx.x;
  float *bl = J == StateJob::Restart ? nullptr : blob + (int64_t)i * blob_stride;
  for (int k = 0; k < fl.n; ++k) {
    const StateField &f = fl.f[k];
    if (!f.ptr || !((mask >> k) & 1u)) continue;
    if (J != StateJob::Restart && f.blob_off < 0) continue;
    float *base = f.ptr + (int64_t)(s / f.group) * f.group_stride + (int64_t)(s % f.group) * f.stream_stride;
    const int n = f.rows * f.row_floats;
    if (f.vec) {
      float4 fresh = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f.fresh == kFreshLim) fresh = make_float4(1.0f, -1.0f, -1.0f, __int_as_float(fl.lim_n));
      for (int e = 4 * t; e < n; e += 4 * 256) {
        const int r = e / f.row_floats, j = e - r * f.row_floats;
        float4 *d = reinterpret_cast<float4 *>(base + (int64_t)r * f.row_stride + j);
        if constexpr (J == StateJob::Restart) *d = fresh;
        else if constexpr (J == StateJob::Export) *reinterpret_cast<float4 *>(bl + f.blob_off + e) = *d;
        else *d = *reinterpret_cast<const float4 *>(bl + f.blob_off + e);
      }
    } else {
      const float fresh = f.fresh == kFreshValue ? vals.v[f.value_row & 3][i & (kStateChunk - 1)] : 0.f;
      for (int e = t; e < n; e += 256) {
        const int r = e / f.row_floats, j = e - r * f.row_floats;
        float *d = base + (int64_t)r * f.row_stride + j;
        if constexpr (J == StateJob::Restart) *d = fresh;
        else if constexpr (J == StateJob::Export) bl[f.blob_off + e] = *d;
        else *d = bl[f.blob_off + e];
      }
    }
  }
}

// one launch over the streams [stream0, stream0 + count) — the caller has checked the range against the fields' extent
template <StateJob J>
inline void stream_state_launch(const StateFields &fl, uint32_t mask, int stream0, int count, float *blob, int64_t blob_stride,
                                const StateValues &vals, hipStream_t st) {
  hipLaunchKernelGGL(stream_state_kernel<J>, dim3((unsigned)count), dim3(256), 0, st, fl, mask, stream0, blob, blob_stride, vals);
}
