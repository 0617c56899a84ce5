// Sample-rate conversion of stage 1: what read_audio (jatts/utils/utils.py:201-234) gets from librosa.load(sr=...), here a
// Kaiser-windowed-sinc polyphase FIR of our own definition (jatts_amd.features.resample_taps), pinned on scipy.signal.resample_poly;
// parity with librosa / soxr_hq is UNPINNED.
//
// resample_kernel: y[m] = sum_n h[m * down - n * up + half_len] * x[n], zeros beyond both ends of the utterance, as ONE exact-f32 framed
// contraction (framed_contract<1>, framed_contraction.h: the loop, its LDS tile, the wave dealing and the order of the sum live there).  The
// frame = a BLOCK of Nb = up * r consecutive outputs (every block meets the taps in the same phase pattern, so one table serves them all):
//   Y[q][c] = sum_i X_q[i] * W[i][c],  X_q[i] = x[q * hop_b - L + i],  W[i][c] = h[c * down - (i - L) * up + half_len] or 0,
//   hop_b = down * r, L = half_len / up, i < K.  Row q of Y is outputs q * Nb .. q * Nb + Nb - 1: the rows concatenated are the waveform.
//   * A operand = blocks, zeros for samples outside the utterance;
//   * B operand = the table [K][Nbp] (jatts_amd.features.resample_table), one plane; the grid runs block tiles fastest.  With one or two column
//     tiles (up <= 64: every 2:1, 3:1, 3:2 conversion) the (column tile, block tile) pairs are dealt one per wave;
//   * no atomics: an utterance's bits depend on its own samples and the table only, not on its place in the batch;
//   * outputs at or beyond n_out are never stored.
// wave_gain_peak_kernel: the two checks of read_audio (utils.py:221-232) and its gain without a read-back per utterance.
#include "framed_contraction.h"

namespace {

struct resample_geom {
  int r, nb, nbp, hop_b, L, K;
};

// The block form of include/jatts_hip.h (and of jatts_amd.features.resample_geometry).  false: beyond the kernel's limits.
bool resample_geometry(int64_t up, int64_t down, int64_t half_len, resample_geom* g) {
  const int64_t r = up < 32 ? (32 + up - 1) / up : 1;
  const int64_t nb = up * r, hop_b = down * r, L = half_len / up;
  const int64_t K = ((((nb - 1) * down + half_len) / up + L + 1) + 63) / 64 * 64;
  const int64_t nbp = (nb + 31) / 32 * 32;
  if (K > 2048 || nbp > 512 || hop_b > (1 << 20)) return false;
  *g = {(int)r, (int)nb, (int)nbp, (int)hop_b, (int)L, (int)K};
  return true;
}

__global__ __launch_bounds__(256, 2) void resample_kernel(const int32_t* __restrict__ cu_in, const int32_t* __restrict__ cu_out,
                                                         const float* __restrict__ x, const float* __restrict__ table, int K, int hop_b, int L,
                                                         int nb, int nbp, float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float tile[2][FT * PITCH];
  const int b = blockIdx.y;
  const int o0 = cu_out[b], n_out = cu_out[b + 1] - o0;
  const int T = (n_out + nb - 1) / nb;          // blocks of this utterance
  const int t0 = blockIdx.x * FT;
  if (t0 >= T) return;
  const int s0 = cu_in[b], n_in = cu_in[b + 1] - s0;
  const float* xb = x + s0;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, c = lane & 31;
  const framed_wave w = framed_deal(nbp, t0, T);
  const int col0 = w.col0;
  const unsigned fmask = w.fmask;

  f32x16 acc[2][1];     // [block tile][the one plane]
  framed_contract<1>(tile, t0, T, K, table + (fmask ? col0 + c : 0), nbp, 0, fmask,
                     [&](int t, int k) {
                       const int p = t * hop_b - L + k;
                       return (p >= 0 && p < n_in) ? xb[p] : 0.f;      // zeros lie beyond both ends
                     },
                     acc);

  // epilogue: C fragment col = lane & 31 (table column), row = (r & 3) + 8 (r >> 2) + 4 h (block): 128-byte segments per half wave, and
  // consecutive blocks are consecutive in the waveform
  const int col = col0 + c;
  if (col >= nb) return;
  float* yb = y + o0;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!(fmask >> f & 1)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fl = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const int m = (t0 + fl) * nb + col;
      if (m < n_out) yb[m] = acc[f][0][r];
    }
  }
}

// NaN-propagating maximum (numpy's): once a NaN, always a NaN
__device__ __forceinline__ float peak_max(float m, float a) { return (a > m || a != a) ? a : m; }

// One workgroup per utterance: peak[b][0] = max |y_b|, y_b *= gain (one f32 multiply), peak[b][1] = max |y_b| afterwards.
__global__ __launch_bounds__(1024) void wave_gain_peak_kernel(const int32_t* __restrict__ cu, float* __restrict__ y, float gain,
                                                             float* __restrict__ peak) {
  __shared__ float red[2][16];
  const int b = blockIdx.x;
  const int s0 = cu[b], n = cu[b + 1] - s0;
  float m0 = 0.f, m1 = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float v = y[s0 + i];
    const float w = __fmul_rn(v, gain);
    m0 = peak_max(m0, fabsf(v));
    m1 = peak_max(m1, fabsf(w));
    y[s0 + i] = w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m0 = peak_max(m0, __shfl_xor(m0, o));
    m1 = peak_max(m1, __shfl_xor(m1, o));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = m0;
    red[1][threadIdx.x >> 6] = m1;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    float m = red[threadIdx.x][0];
    for (int j = 1; j < 16; ++j) m = peak_max(m, red[threadIdx.x][j]);
    peak[2 * b + threadIdx.x] = m;
  }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int jatts_resample(int32_t n_seq, const int32_t* cu_in, const int32_t* cu_out, const int32_t* host_in, const float* x,
                              const float* table, int32_t up, int32_t down, int32_t half_len, int32_t table_rows, float* y, void* stream) {
  if (!cu_in || !cu_out || !host_in || !x || !table || !y) return jatts_set_error_msg(JATTS_ERR_ARG, "resample: null pointer");
  if (up < 1 || down < 1 || half_len < 1) return jatts_set_error_msg(JATTS_ERR_ARG, "resample: up, down and half_len must be positive");
  resample_geom g;
  if (!resample_geometry(up, down, half_len, &g))
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resample: table beyond K = 2048 rows or Nbp = 512 columns (reduce the ratio's terms or zeros)");
  if (table_rows != g.K) return jatts_set_error_msg(JATTS_ERR_ARG, "resample: the table does not have the K rows of this up, down and half_len");
  if (n_seq <= 0) return JATTS_OK;
  if (n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resample: more than 65535 utterances (split the batch)");
  int64_t total_in = 0, total_out = 0, max_blocks = 0;
  for (int b = 0; b < n_seq; ++b) {
    const int64_t n = host_in[b];
    if (n < 0) return jatts_set_error_msg(JATTS_ERR_ARG, "resample: negative length");
    const int64_t n_out = (n * up + down - 1) / down, blocks = (n_out + g.nb - 1) / g.nb;
    total_in += n;
    total_out += n_out;
    max_blocks = blocks > max_blocks ? blocks : max_blocks;
  }
  if (total_in >= (int64_t)1 << 30 || total_out >= (int64_t)1 << 30) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resample: launch too large (2^30 samples)");
  if (max_blocks == 0) return JATTS_OK;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((max_blocks + FT - 1) / FT), (unsigned)n_seq, (unsigned)((g.nbp + BW - 1) / BW)), dim3(256), 0, S_,
                     cu_in, cu_out, x, table, g.K, g.hop_b, g.L, g.nb, g.nbp, y);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_wave_gain_peak(int32_t n_seq, const int32_t* cu, float* y, float gain, float* peak, void* stream) {
  if (!cu || !y || !peak) return jatts_set_error_msg(JATTS_ERR_ARG, "wave_gain_peak: null pointer");
  if (n_seq <= 0) return JATTS_OK;
  hipLaunchKernelGGL(wave_gain_peak_kernel, dim3((unsigned)n_seq), dim3(1024), 0, S_, cu, y, gain, peak);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
