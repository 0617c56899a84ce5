// Stage-3 batch assembly: what jatts/datasets/tts_dataset.py:69-145 (one HDF5 read + StandardScaler.transform per utterance and step)
// and jatts/collaters/fastspeech2.py:17-107 (pad_list on the CPU, then .to(device) in the trainers) do for one batch, as ONE gather
// launch over stores that already sit on the device, normalised (jatts_amd/data.py: ResidentDataset).
//
// Per field f and batch slot b, with u = utt[b]: the utterance's rows are one contiguous run of row_len[u] * dim elements behind
// src + row_start[u] * dim, and the slot is one contiguous run of t_max * dim elements behind dst + b * t_max * dim.  So a slot is a flat copy of
// n_valid 32-bit words followed by zero words (elem_bytes is 4 or 8: an int64 is two words; bits move, nothing is interpreted: -0.0 and NaN payloads
// survive).  Padding words are STORED as zero, never loaded and masked: nothing behind the utterance in the store is read past the last 16-byte unit
// that lies wholly inside it, and that unit's neighbours are picked word by word.
//
// Geometry: workgroup = 256 threads x 4 units of 16 bytes = 4096 words of one slot; a 1-D grid over sum_f n_batch * ceil(slot words / 4096)
// workgroups (gridDim.x: 2^31 - 1; n_batch * t_max never meets a 65 535-limited dimension), fields one behind the other: the table, with each field's
// first workgroup, travels by value in the kernel arguments, and a workgroup finds its field by comparing its index with at most eight numbers.
// Access (cdna_hip_programming.md §2 "Global memory coalescing", Guideline 13; MI355X_MICROARCH.md "Memory hierarchy" / "HBM"): lane i of a wave
// touches bytes 16 i .. 16 i + 15 of a 1 KiB run in every load and every store when the slot's source and destination both start on 16 bytes
// (dim = 80 f32: every row start does); otherwise the same runs word by word, lane i at word i: still fully coalesced, a quarter of the bytes per
// instruction.  A bandwidth-bound copy: no LDS, no atomics, four independent loads in flight per thread before the first store.
#include "common.h"

namespace {

constexpr int NT = 256;                 // threads of a workgroup
constexpr int UPT = 4;                  // 16-byte units per thread
constexpr int WG_WORDS = NT * UPT * 4;  // 32-bit words of a slot one workgroup writes

struct CollateArgs {
  jatts_collate_field f[JATTS_COLLATE_MAX_FIELDS];
  uint32_t wg0[JATTS_COLLATE_MAX_FIELDS];      // first workgroup of the field
  int32_t wg_per_slot[JATTS_COLLATE_MAX_FIELDS];
  int32_t n_fields;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(NT) void collate_kernel(const CollateArgs a, const int32_t* __restrict__ utt) {
  const uint32_t wg = blockIdx.x;
  int fi = 0;
#pragma unroll
  for (int i = 1; i < JATTS_COLLATE_MAX_FIELDS; ++i)
    if (i < a.n_fields && wg >= a.wg0[i]) fi = i;
  const jatts_collate_field& f = a.f[fi];
  const uint32_t local = wg - a.wg0[fi];
  const int b = (int)(local / (uint32_t)a.wg_per_slot[fi]);
  const int chunk = (int)(local - (uint32_t)b * (uint32_t)a.wg_per_slot[fi]);

  const int wpr = f.dim * (f.elem_bytes >> 2);                   // words of a row
  const int tw = f.t_max * wpr;                                  // words of a slot (the launcher checked that it fits an int)
  const int u = utt[b];
  int rl = f.row_len[u];
  rl = rl < 0 ? 0 : (rl > f.t_max ? f.t_max : rl);               // (the wrapper refuses t_max < row_len; a slot is never overrun)
  const int nvw = rl * wpr;                                      // words that come from the store
  const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(f.src) + f.row_start[u] * (int64_t)wpr;
  uint32_t* __restrict__ d = reinterpret_cast<uint32_t*>(f.dst) + (int64_t)b * tw;
  const int w0 = chunk * WG_WORDS, tid = threadIdx.x;

  if (((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 15) == 0) {
    u32x4 v[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int i = w0 + (k * NT + tid) * 4;
      v[k] = u32x4{0u, 0u, 0u, 0u};
      if (i + 4 <= nvw) {
        v[k] = *reinterpret_cast<const u32x4*>(s + i);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < nvw) v[k][e] = s[i + e];
      }
    }
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int i = w0 + (k * NT + tid) * 4;
      if (i + 4 <= tw) {
        *reinterpret_cast<u32x4*>(d + i) = v[k];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i + e < tw) d[i + e] = v[k][e];
      }
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < UPT * 4; ++k) {
      const int j = w0 + k * NT + tid;
      if (j < tw) d[j] = j < nvw ? s[j] : 0u;
    }
  }
}

}  // namespace

extern "C" int jatts_collate(const jatts_collate_field* fields, int32_t n_fields, const int32_t* utt, int32_t n_batch, void* stream) {
  if (n_fields < 1 || n_fields > JATTS_COLLATE_MAX_FIELDS) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: n_fields outside 1..JATTS_COLLATE_MAX_FIELDS");
  if (n_batch < 1) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: n_batch < 1");
  if (!fields || !utt) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: null pointer");
  CollateArgs a = {};
  a.n_fields = n_fields;
  uint64_t total = 0;
  for (int i = 0; i < n_fields; ++i) {
    const jatts_collate_field& f = fields[i];
    if (f.dim < 1 || f.t_max < 1) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: dim < 1 or t_max < 1");
    if (f.elem_bytes != 4 && f.elem_bytes != 8) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: elem_bytes is 4 (f32) or 8 (i64)");
    if (!f.src || !f.row_start || !f.row_len || !f.dst) return jatts_set_error_msg(JATTS_ERR_ARG, "collate: null pointer in a field");
    if ((reinterpret_cast<uintptr_t>(f.src) | reinterpret_cast<uintptr_t>(f.dst)) % (uintptr_t)f.elem_bytes)
      return jatts_set_error_msg(JATTS_ERR_ARG, "collate: src / dst not aligned to the element");
    const int64_t tw = (int64_t)f.t_max * f.dim * (f.elem_bytes / 4);
    if (tw > 0x7fffffff - WG_WORDS) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "collate: a slot of 2^31 words or more");
    a.f[i] = f;
    a.wg0[i] = (uint32_t)total;
    a.wg_per_slot[i] = (int32_t)((tw + WG_WORDS - 1) / WG_WORDS);
    total += (uint64_t)a.wg_per_slot[i] * (uint64_t)n_batch;
    if (total > 0x7fffffffull) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "collate: launch too large (split the batch)");
  }
  hipLaunchKernelGGL(collate_kernel, dim3((unsigned)total), dim3(NT), 0, (hipStream_t)stream, a, utt);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
