// The framed exact-f32 contraction of stage 1: Y[t][col] = sum_{k < K} X_t[k] * W[k][col] over "frames" X_t that are overlapping spans of a
// waveform, never materialised.  stft_mag_kernel (features.hip: frames of n_fft samples under numpy's reflect rule, a cosine and a sine plane)
// and resample_kernel (resample.hip: blocks of outputs, zeros beyond both ends, one plane of taps) are this loop with their own sample rule,
// plane count and epilogue.  What to try next on it is tried here, once.
//   * A operand = frames.  A workgroup stages FT = 64 frames x KC = 64 samples of the current K-chunk into an LDS tile [64][64 + 4],
//     double-buffered, one barrier per chunk; rows that overlap are re-read from L2.
//     LDS banks of the A fragment reads (ds_read_b128, banks (a / 4) mod 64, lane groups {0-3, 12-15, 20-27} ...): lane (f, h) reads 4 floats
//     at f * 68 + 16 s + 8 h (+ 4): bank 4 f mod 64 + const for the 16 different f of a group -- 16 distinct 4-bank slots, conflict-free
//     (row bytes + 16 is what PITCH = KC + 4 buys);
//   * B operand = the table, straight from L2 into registers one k-step ahead: lane l of k-step s reads W[16 s + 8 (l >> 5) + j][col0 + (l & 31)]
//     of every plane, 128 contiguous bytes per half wave.  A workgroup owns BW = 128 columns (4 waves x 32);
//   * v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain, the arithmetic of every exact kernel here.  Lane half h consumes
//     k = 16 s + 8 h + j in MFMA j -- the same samples meet the same table rows in both operands, the order of the sum is fixed.
//     The sum has TWO levels: every 64-sample chunk is a chain of its own, started at zero, and the chunks are added in order (v_add_f32,
//     64 per 128 MFMAs).  One 2048-term chain rounds 2048 times at the magnitude of the growing sum (error ~ sqrt(K)); with chunks it is 64
//     roundings at a chunk's magnitude plus 32 at the sum's.  A CPU emulation of both orders on the STFT's test signals: one chain 6.0-7.6 x
//     the float32-FFT error on mel bins relative to their frame's maximum, chunks of 64 1.2-1.5 x (profiles/r15_notes.md).  The order is part
//     of both kernels' contract: their outputs are pinned bit for bit.
#pragma once
#include "common.h"

constexpr int FT = 64;         // frames per workgroup (two 32-row MFMA tiles)
constexpr int KC = 64;         // samples per staged K-chunk
constexpr int PITCH = KC + 4;  // floats; row bytes + 16
constexpr int BW = 128;        // table columns per workgroup (4 waves x 32)

// Work of a wave inside workgroup (frame tile t0 / FT, column tile blockIdx.z) of a table nbp columns wide: one 32-column tile x both frame
// tiles.  The last workgroup of a row of column tiles may own fewer than four; with one or two, its (column tile, frame tile) pairs are dealt one
// per wave, which halves its time.  A frame tile wholly past the utterance's end (T frames) is skipped.
struct framed_wave {
  int slot;          // the wave's column tile inside the workgroup
  int col0;          // its first table column
  unsigned fmask;    // the frame tiles it computes (wave-uniform, held in an SGPR); 0: a wave without work only helps staging
};
__device__ __forceinline__ framed_wave framed_deal(int nbp, int t0, int T) {
  const int wave = threadIdx.x >> 6;
  const int ntl = min(4, (nbp >> 5) - (int)blockIdx.z * 4);
  const bool pairs = ntl <= 2;
  const int slot = pairs ? wave >> 1 : wave;
  const unsigned fmask = __builtin_amdgcn_readfirstlane(slot >= ntl ? 0u : (pairs ? 1u << (wave & 1) : 3u) & (t0 + 32 < T ? 3u : 1u));
  return {slot, (int)blockIdx.z * BW + slot * 32, fmask};
}

// acc[f][q] = the 32 x 32 C fragment (col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) of frame tile f against plane q, for the
// frame tiles of fmask; the others stay zero.  sample(t, k): element k of frame t, asked for t < T only (frames at or past T are staged as zeros).
// tb: the lane's table pointer, W[0][col0 + (lane & 31)] of plane 0 (any valid address where fmask is 0); ldt: floats between table rows;
// plane: floats between planes.  K is a multiple of KC.
// Called by all 256 threads of the workgroup, after the kernel's own early exit (it holds barriers).  It ends behind a barrier: every read of
// the tile is over when it returns, and the caller may reuse tile[0].
template <int NQ, typename Sample>
__device__ __forceinline__ void framed_contract(float (&tile)[2][FT * PITCH], int t0, int T, int K, const float* tb, int ldt, int plane,
                                                unsigned fmask, Sample sample, f32x16 (&acc)[2][NQ]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = lane >> 5, c = lane & 31;
  const bool live = fmask != 0;

  // staging map: thread -> sample column tid & 63 of frames (tid >> 6) + 4 i (a wave writes one 256-byte row: conflict-free)
  const int sn = tid & 63, sf = tid >> 6;
  float xr[16];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = t0 + sf + 4 * i;
      xr[i] = t < T ? sample(t, k0 + sn) : 0.f;
    }
  };
  auto stash = [&](float* buf) {
#pragma unroll
    for (int i = 0; i < 16; ++i) buf[(sf + 4 * i) * PITCH + sn] = xr[i];
  };

  auto load_b = [&](int s, f32x8 (&w)[NQ]) {
    const float* p = tb + (int64_t)(16 * s + 8 * h) * ldt;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int q = 0; q < NQ; ++q) w[q][j] = p[(int64_t)j * ldt + q * plane];
  };

#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[f][q][r] = 0.f;

  const int n_chunks = K / KC, n_steps = K / 16;
  f32x8 bw[NQ], nw[NQ];
  if (live) load_b(0, nw);
  fetch(0);
  stash(tile[0]);
  __syncthreads();
  for (int ch = 0; ch < n_chunks; ++ch) {
    const float* cur = tile[ch & 1];
    if (ch + 1 < n_chunks) fetch((ch + 1) * KC);
    if (live) {
      f32x16 part[2][NQ];      // this chunk's 64-term chains, started at zero
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
          for (int r = 0; r < 16; ++r) part[f][q][r] = 0.f;
#pragma unroll
      for (int ss = 0; ss < KC / 16; ++ss) {
        const int s = ch * (KC / 16) + ss;
#pragma unroll
        for (int q = 0; q < NQ; ++q) bw[q] = nw[q];
        load_b(s + 1 < n_steps ? s + 1 : s, nw);      // one step ahead; the last step is read twice
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          if (!(fmask >> f & 1)) continue;
          const float* p = cur + (f * 32 + c) * PITCH + 16 * ss + 8 * h;
          const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
          const f32x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
          for (int q = 0; q < NQ; ++q) mma32(a, bw[q], part[f][q]);
        }
      }
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int q = 0; q < NQ; ++q) acc[f][q] += part[f][q];      // chunks in order: the second level of the sum
    }
    if (ch + 1 < n_chunks) stash(tile[(ch + 1) & 1]);       // last read two barriers ago
    __syncthreads();
  }
}
