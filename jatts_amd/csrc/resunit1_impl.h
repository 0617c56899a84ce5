// Fused HiFi-GAN SINGLE-CONV dilation unit  y = x + conv_d(lrelu(x)) + b1  (ResBlocks built with use_additional_convs=False: HiFi-GAN V3).
// The unit of resunit_impl.h without its second conv: same packed ragged geometry, same LDS image of the x tile, same MFMA inner loops
// (conv_tiles.h) and the same row-contiguous store pass with the optional MRF mean (unit_store_pass).  Instantiated per dtype in resunit1_*.hip.
//
// What is simpler without the second conv: there is no h tile and no discarded column -- a window of WGCOLS columns stores all WGCOLS of them,
// and its x tile is WGCOLS + (k - 1) dil rows (row r <-> position t0 - p1 + r).  The tile is a function of (channels, k_w, dil) alone.
#pragma once
#include "resunit_impl.h"

namespace {

// RREG: the residual x of this lane's output elements is read from the RAW x tile into registers before the tile is activated in place
// (x fetched from HBM once; f32 tiles, as in resunit_kernel).
template <typename T, int C, int WGCOLS, int WN, int NT, int KCGMAX = 8, int OCC = 0, bool RREG = false>
__global__ __launch_bounds__(WN*(WGCOLS / (NT * 32)) * 64, OCC ? OCC : ((C <= 256 && (C / (WN * 32)) * NT * 16 <= 128) ? 2 : 1)) void resunit1_kernel(jatts_resunit_desc d, unsigned bias_off) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WT = WGCOLS / (NT * 32);
  constexpr int NF = C / (WN * 32);
  constexpr int KC16 = C / 16, NFR = C / 32;
  constexpr int pitch = C * (int)sizeof(T) + 16;
  constexpr int KCG = sizeof(T) == 4 ? 2 : (KC16 < KCGMAX ? KC16 : KCGMAX);  // ring depth = group size
  constexpr int NTHR = WN * WT * 64;
  static_assert(WT * NT * 32 == WGCOLS && NF * WN * 32 == C, "tile shape");
  const int K = d.k_w, dil = d.dil;
  const int p1 = (K - 1) / 2 * dil;

  // unit_window_of (unit_frame.h), kept as this kernel's own copy: the helper's exits cost the smallest f16 tile 12 instructions, 1.06 % (profiles/r14_notes.md)
  int b = blockIdx.y, bx = blockIdx.x;
  if (ragged_is_1d(d.rg) && !ragged_locate(d.rg, WGCOLS, blockIdx.x, b, bx)) return;   // 1-D grid over the real tiles of a ragged batch
  const int row_b = d.rg.cu_rows[b];
  const int L = (d.rg.cu_rows[b + 1] - row_b) * d.rg.len_mul;
  const int t0 = bx * WGCOLS;
  if (t0 >= L) return;
  const int64_t seq_row0 = (int64_t)row_b * d.rg.len_mul;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wn = wave / WT, wt = wave % WT;
  const int g = lane >> 5;
  const int col0 = wt * NT * 32;
  const int nf0 = wn * NF;

  const int rx = WGCOLS + 2 * p1;   // x tile rows: row r <-> position t0 - p1 + r
  char* xs = smem;
  float* bs = reinterpret_cast<float*>(smem + bias_off);   // b1 behind the tile: one ds_read_b128 per channel quad
  for (int u = threadIdx.x; u < C; u += NTHR) bs[u] = d.b1[u];

  // f16: the weight ring's first group is fetched under the x staging (f32: 64-cycle MFMAs and a two-deep ring hide the fill already)
  constexpr bool STREAM = sizeof(T) == 2;
  WStream<T, NF, KCG> ws;
  if constexpr (STREAM) ws.prefetch((const T*)d.w1, NFR, nf0, lane);
  {
    constexpr int UBX = ((WGCOLS + 64) * (C / 8) + NTHR - 1) / NTHR;   // covers halos up to 32 rows a side in one batch; longer ones take a second pass
    stage_unit<T, (UBX < 8 ? 8 : (UBX < 24 ? UBX : 24)), NTHR>(xs, pitch, rx, C / 8, t0 - p1, L, seq_row0, (const T*)d.x, C, !RREG, d.slope);
  }
  __syncthreads();
  // x at (output column, channel quad) of this lane, C-fragment layout
  typedef T resid_t __attribute__((ext_vector_type(4)));
  resid_t resid[RREG ? NF : 1][RREG ? NT : 1][4];
  if constexpr (RREG) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = col0 + t * 32 + (lane & 31);   // output column col <-> x tile row col + p1
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          resid[f][t][q] = *reinterpret_cast<const resid_t*>(xs + (size_t)(col + p1) * pitch + (size_t)((nf0 + f) * 32 + 8 * q + 4 * g) * sizeof(T));
    }
    __syncthreads();
    for (int u = threadIdx.x; u < rx * (C / 8); u += NTHR) {   // tile <- lrelu(tile), in place
      char* p = xs + (size_t)(u / (C / 8)) * pitch + (size_t)(u % (C / 8)) * 8 * sizeof(T);
      typename Elem<T>::vec8 v = Vec8IO<T>::lds(p);
      lrelu8(v, d.slope);
      Vec8IO<T>::sts(p, v);
    }
    __syncthreads();
  }

  // the accumulators start at the bias (C layout: register 4q+e of fragment f <-> channel 32(nf0+f) + 8q + 4g + e)
  f32x16 acc[NF][NT];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bs + (nf0 + f) * 32 + 8 * q + 4 * g);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[f][t][4 * q + e] = bb[e];
    }
  if constexpr (STREAM) conv_full_ws<T, NF, NT, KC16, KCG>(acc, ws, (const T*)d.w1, nullptr, K, dil, xs, pitch, col0, lane);
  else conv_full<T, NF, NT, KC16, KCG>(acc, (const T*)d.w1, NFR, nf0, K, dil, xs, pitch, col0, lane);

  // epilogue: acc (+ b1, already in) is assembled in LDS over the dead x tile and the residual (and the MRF mean) are added in the
  // row-contiguous 16-byte store pass: in MFMA fragment order the x re-read and the y store would scatter every 128-byte line
  __syncthreads();
  char* ys = smem;
  const int vrows = min(WGCOLS, L - t0);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = col0 + t * 32 + (lane & 31);
    if (col >= vrows) continue;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int n0 = (nf0 + f) * 32 + 8 * q + 4 * g;
        char* p = ys + (size_t)col * pitch + (size_t)n0 * sizeof(T);
        if constexpr (sizeof(T) == 2) {
          f16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc[f][t][4 * q + e];
            if constexpr (RREG) v += (float)resid[f][t][q][e];
            o[e] = (f16)v;
          }
          *reinterpret_cast<f16x4*>(p) = o;
        } else {
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            o[e] = acc[f][t][4 * q + e];
            if constexpr (RREG) o[e] += (float)resid[f][t][q][e];
          }
          *reinterpret_cast<f32x4*>(p) = o;
        }
      }
  }
  __syncthreads();
  {
    const int64_t g0 = (seq_row0 + t0) * (int64_t)C;  // the valid rows are contiguous in y: unit u <-> 8 elements at g0 + 8u
    unit_store<T, C, NTHR, !RREG>(d, ys, pitch, vrows, g0);
  }
}

// LDS bytes of a <T, C, WGCOLS> window at this halo: the x tile (the y tile overlays it) + b1
template <typename T, int C, int WGCOLS>
constexpr size_t resunit1_lds(int halo) { return (size_t)(WGCOLS + halo) * (C * sizeof(T) + 16) + C * sizeof(float); }

template <typename T, int C, int WGCOLS, int WN, int NT, int KCGMAX = 8, int OCC = 0, bool RREG = false>
int launch_resunit1(const jatts_resunit_desc& d, hipStream_t s) {
  constexpr int WT = WGCOLS / (NT * 32);
  const int halo = (d.k_w - 1) / 2 * d.dil * 2;
  const size_t lds = resunit1_lds<T, C, WGCOLS>(halo);
  constexpr auto kern = resunit1_kernel<T, C, WGCOLS, WN, NT, KCGMAX, OCC, RREG>;
  return unit_launch<kern>(JATTS_SITE("resunit (single conv): tile exceeds 160 KiB LDS"), WN * WT * 64, lds, WGCOLS, d.rg, s, d, (unsigned)(lds - C * sizeof(float)));
}

}  // namespace
