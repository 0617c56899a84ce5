// Griffin-Lim phase reconstruction: what the reference would run where a config has no `vocoder:` entry (its Spectrogram2Waveform,
// tts_decode.py:190-200, tts_train.py:316-325; the module itself does not exist there), here a definition of this project's own -- the "fast
// Griffin-Lim" loop with momentum on a zero-padded centred STFT and its windowed least-squares inverse -- pinned on a float64 restatement
// (tests/griffinlim_reference.py).  Parity with librosa.griffinlim / ESPnet's logmel2linear is UNPINNED.
//
//   X_0 = S P0; C_-1 = 0;  per iteration  x = ISTFT(X), C = STFT(x), A = C - beta C_prev, X = S A / (|A| + 2^-126);  y = ISTFT(X)
//
// Both transforms are framed_contract (framed_contraction.h: the loop, its LDS tile, the wave dealing and the two-level order of the sum).
// gl_stft_project_kernel: framed_contract<2> over frames of n_fft samples hop apart, ZEROS outside [0, (T - 1) hop) (not the reflect rule of
//   stft_mag_kernel), table = features.dft_table.  The projection is the epilogue, in registers: neither the frame matrix, nor C before it
//   replaces C_prev, nor A reaches HBM.
// gl_istft_kernel: the overlap-add written as ONE span contraction per output row.  With n + n_fft / 2 = m hop + r and J = ceil(n_fft / hop),
//   num[m][r] = sum_{j < J} sum_k Xflat[m - j][k] Tab[j][k][r]: j descending, the J rows m - J + 1 .. m of Xflat (row = [re 0..nbp) | im 0..nbp)],
//   pitch 2 nbp, a multiple of 64) are one contiguous span, zeros where the row lies outside the utterance -- resample_kernel's sample rule.
//   The epilogue multiplies by the reciprocal envelope 1 / sum_j w^2[j hop + r] over the frames that exist, (j_lo, j_hi) = (max(0, m - T + 1),
//   min(J - 1, m)): a host float64 table [J][J][hopp].  No atomics and no overlap-add pass: a sample's bits depend on its own utterance only.
// The row-wise kernels: base ** (c scale + mean), max(eps, .) behind the pseudo-inverse mel projection (a jatts_conv1d launch), X_0 = S P0.
#include "framed_contraction.h"

namespace {

constexpr int GL_MAX_J = 64;      // frames that overlap one sample: bounds the envelope table (J * J * hopp floats) and K = J * 2 nbp

__global__ __launch_bounds__(256, 2) void gl_stft_project_kernel(jatts_ragged rg, const float* __restrict__ x, const float* __restrict__ table,
                                                                int n_fft, int hop, int n_bins, int nbp, const float* __restrict__ S, int lds,
                                                                float beta, float* __restrict__ c_prev, float* __restrict__ x_next) {
  __shared__ __attribute__((aligned(16))) float tile[2][FT * PITCH];
  const int b = blockIdx.y;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const int t0 = blockIdx.x * FT;
  if (t0 >= T) return;
  const int L = (T - 1) * hop;                                 // samples of the utterance; they start at row0 * hop
  const float* xb = x + (int64_t)row0 * hop;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, c = lane & 31;
  const framed_wave w = framed_deal(nbp, t0, T);
  const int bin0 = w.col0;
  const unsigned fmask = w.fmask;
  const int half = n_fft >> 1;

  f32x16 acc[2][2];     // [frame tile][re | im]
  framed_contract<2>(tile, t0, T, n_fft, table + (fmask ? bin0 + c : 0), 2 * nbp, nbp, fmask,
                     [&](int t, int k) {
                       const int p = t * hop + k - half;
                       return (p >= 0 && p < L) ? xb[p] : 0.f;      // zeros lie beyond both ends
                     },
                     acc);

  // epilogue: C fragment col = lane & 31 (bin), row = (r & 3) + 8 (r >> 2) + 4 h (frame).  Spelled out: nothing is left to contract.
  const int bin = bin0 + c;
  const float tiny = 1.17549435e-38f;      // 2^-126
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!(fmask >> f & 1)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fl = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (t0 + fl >= T) continue;
      const int64_t row = row0 + t0 + fl;
      const int64_t i = row * (2 * nbp) + bin;
      float xr = 0.f, xi = 0.f, re = 0.f, im = 0.f;
      if (bin < n_bins) {
        re = acc[f][0][r];
        im = acc[f][1][r];
        float ar = fmaf(-beta, c_prev[i], re), ai = fmaf(-beta, c_prev[i + nbp], im);
        // |A| below 2^-60: its squares would leave the normal range.  S A k / (|A| k + tiny k) with k = 2^96 is the same quotient, and
        // both scalings are exact (powers of two); above 2^-60 the squares are normal numbers.  (|A| up to 2^63: no overflow.)
        const bool small = fmaxf(fabsf(ar), fabsf(ai)) < 0x1p-60f;
        const float k = small ? 0x1p96f : 1.f;
        ar = __fmul_rn(ar, k);
        ai = __fmul_rn(ai, k);
        const float mag = sqrtf(fmaf(ar, ar, __fmul_rn(ai, ai)));
        const float q = __fdiv_rn(S[row * lds + bin], __fadd_rn(mag, small ? 0x1p-30f : tiny));
        xr = __fmul_rn(q, ar);
        xi = __fmul_rn(q, ai);
      }
      c_prev[i] = re;
      c_prev[i + nbp] = im;
      x_next[i] = xr;
      x_next[i + nbp] = xi;
    }
  }
}

__global__ __launch_bounds__(256, 2) void gl_istft_kernel(jatts_ragged rg, const float* __restrict__ X, const float* __restrict__ table,
                                                         const float* __restrict__ renv, int n_fft, int hop, int hopp, int nbp, int J, int packed,
                                                         float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float tile[2][FT * PITCH];
  const int b = blockIdx.y;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  if (T < 2) return;                                           // one frame: an empty waveform
  const int L = (T - 1) * hop, half = n_fft >> 1;
  const int m_lo = half / hop, Tm = (half + L - 1) / hop - m_lo + 1;      // the output rows that hold a sample of [0, L)
  const int t0 = blockIdx.x * FT;
  if (t0 >= Tm) return;
  const int ldx = 2 * nbp;
  const float* xb = X + (int64_t)row0 * ldx;
  const int span = T * ldx, base = (m_lo - (J - 1)) * ldx;     // output row m_lo + t contracts Xflat[base + t ldx .. + J ldx)
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, c = lane & 31;
  const framed_wave w = framed_deal(hopp, t0, Tm);
  const int col0 = w.col0;
  const unsigned fmask = w.fmask;

  f32x16 acc[2][1];
  framed_contract<1>(tile, t0, Tm, J * ldx, table + (fmask ? col0 + c : 0), hopp, 0, fmask,
                     [&](int t, int k) {
                       const int p = base + t * ldx + k;
                       return (p >= 0 && p < span) ? xb[p] : 0.f;      // frames before the first and after the last are zeros
                     },
                     acc);

  const int col = col0 + c;
  if (col >= hop) return;
  float* yb = y + (int64_t)(packed ? row0 - b : row0) * hop;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!(fmask >> f & 1)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fl = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const int m = m_lo + t0 + fl;
      const int n = m * hop + col - half;
      if (n < 0 || n >= L) continue;
      const int jlo = max(0, m - T + 1), jhi = min(J - 1, m);
      yb[n] = __fmul_rn(acc[f][0][r], renv[(jlo * J + jhi) * hopp + col]);
    }
  }
}

// out[row][k] = base ** fmaf(c[row][k], scale[k], mean[k]) for k < n_mels, 0 up to ldo.  The power is taken in double and rounded once.
__global__ __launch_bounds__(256) void gl_exp_kernel(const float* c, int ldc, int n_mels, int64_t rows, const float* scale, const float* mean, int base,
                                                     float* out, int ldo) {
  const int64_t total = rows * ldo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / ldo;
    const int k = (int)(i - r * ldo);
    float v = 0.f;
    if (k < n_mels) {
      const double e = (double)fmaf(c[r * ldc + k], scale[k], mean[k]);
      v = (float)(base == 10 ? exp10(e) : base == 2 ? exp2(e) : exp(e));
    }
    out[i] = v;
  }
}

// out[row][k] = max(eps, lin[row][k]) for k < n_bins, 0 up to ldo
__global__ __launch_bounds__(256) void gl_floor_kernel(const float* lin, int ldl, int n_bins, int64_t rows, float eps, float* out, int ldo) {
  const int64_t total = rows * ldo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / ldo;
    const int k = (int)(i - r * ldo);
    out[i] = k < n_bins ? fmaxf(eps, lin[r * ldl + k]) : 0.f;
  }
}

// X[row] = [S re(P0) | S im(P0)], zeros in the padding bins of both planes.  p0: complex64, (rows, n_bins) interleaved.
__global__ __launch_bounds__(256) void gl_init_kernel(const float* S, int lds, const float* p0, int n_bins, int nbp, int64_t rows, float* X) {
  const int64_t total = rows * nbp;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / nbp;
    const int k = (int)(i - r * nbp);
    float re = 0.f, im = 0.f;
    if (k < n_bins) {
      const float s = S[r * lds + k];
      re = __fmul_rn(s, p0[2 * (r * n_bins + k)]);
      im = __fmul_rn(s, p0[2 * (r * n_bins + k) + 1]);
    }
    X[r * 2 * nbp + k] = re;
    X[r * 2 * nbp + nbp + k] = im;
  }
}

// The checks both transforms share.  -> JATTS_OK with *rows, *max_frames filled, or the error code.
int gl_geometry(const char* who, const jatts_ragged* rg, const int32_t* host_frames, int n_fft, int hop, int64_t* rows, int* max_frames) {
  char msg[160];
  if (n_fft < 64 || n_fft > 2048 || n_fft % 64) {
    snprintf(msg, sizeof msg, "%s: n_fft must be a multiple of 64, at most 2048", who);
    return jatts_set_error_msg(JATTS_ERR_ARG, msg);
  }
  if (hop < 1 || hop > n_fft) {
    snprintf(msg, sizeof msg, "%s: hop must lie in [1, n_fft]", who);
    return jatts_set_error_msg(JATTS_ERR_ARG, msg);
  }
  if ((n_fft + hop - 1) / hop > GL_MAX_J) {
    snprintf(msg, sizeof msg, "%s: more than %d overlapping frames per sample (hop < n_fft / %d)", who, GL_MAX_J, GL_MAX_J);
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, msg);
  }
  if (rg->n_seq > 65535) {
    snprintf(msg, sizeof msg, "%s: more than 65535 utterances (split the batch)", who);
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, msg);
  }
  *rows = 0;
  *max_frames = 0;
  for (int b = 0; b < rg->n_seq; ++b) {
    const int T = host_frames[b];
    if (T < 1) {
      snprintf(msg, sizeof msg, "%s: an utterance without a frame", who);
      return jatts_set_error_msg(JATTS_ERR_ARG, msg);
    }
    *rows += T;
    *max_frames = T > *max_frames ? T : *max_frames;
  }
  if (rg->n_seq > 0 && *max_frames != rg->max_len) {
    snprintf(msg, sizeof msg, "%s: host_frames does not match the frame geometry", who);
    return jatts_set_error_msg(JATTS_ERR_ARG, msg);
  }
  const int nbp = (n_fft / 2 + 1 + 31) & ~31;
  if (*rows * (2 * nbp) >= (int64_t)1 << 31 || *rows * hop >= (int64_t)1 << 31) {
    snprintf(msg, sizeof msg, "%s: launch too large", who);
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, msg);
  }
  return JATTS_OK;
}

unsigned rowwise_blocks(int64_t total) {
  const int64_t blocks = (total + 255) / 256;
  return (unsigned)(blocks < 4096 ? blocks : 4096);
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int jatts_gl_stft_project(const jatts_ragged* rg_frames, const int32_t* host_frames, const float* x, const float* table, int32_t n_fft,
                                     int32_t hop, const float* S, int32_t lds, float beta, float* c_prev, float* x_next, int32_t ldx,
                                     void* stream) {
  if (!rg_frames || !host_frames || !x || !table || !S || !c_prev || !x_next) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_stft_project: null pointer");
  int64_t rows;
  int max_frames;
  if (const int rc = gl_geometry("gl_stft_project", rg_frames, host_frames, n_fft, hop, &rows, &max_frames)) return rc;
  const int n_bins = n_fft / 2 + 1, nbp = (n_bins + 31) & ~31;
  if (lds < n_bins) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_stft_project: lds < n_bins");
  if (ldx != 2 * nbp) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_stft_project: the spectrum pitch is not 2 * round_up(n_bins, 32), what the tables are built for");
  if (!(beta >= 0.f && beta < 1.f)) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_stft_project: beta must lie in [0, 1)");
  if (c_prev == x_next || x == x_next || x == c_prev || S == x_next || S == c_prev)
    return jatts_set_error_msg(JATTS_ERR_ARG, "gl_stft_project: x, S, c_prev and x_next must be distinct buffers");
  if (rg_frames->n_seq <= 0 || rows == 0) return JATTS_OK;
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  hipLaunchKernelGGL(gl_stft_project_kernel, dim3((unsigned)((max_frames + FT - 1) / FT), (unsigned)rg.n_seq, (unsigned)((nbp + BW - 1) / BW)), dim3(256), 0,
                     S_, rg, x, table, n_fft, hop, n_bins, nbp, S, lds, beta, c_prev, x_next);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gl_istft(const jatts_ragged* rg_frames, const int32_t* host_frames, const float* X, int32_t ldx, const float* table,
                              int32_t table_rows, int32_t table_cols, const float* renv, int32_t n_fft, int32_t hop, int32_t packed, float* y,
                              void* stream) {
  if (!rg_frames || !host_frames || !X || !table || !renv || !y) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_istft: null pointer");
  int64_t rows;
  int max_frames;
  if (const int rc = gl_geometry("gl_istft", rg_frames, host_frames, n_fft, hop, &rows, &max_frames)) return rc;
  const int n_bins = n_fft / 2 + 1, nbp = (n_bins + 31) & ~31, J = (n_fft + hop - 1) / hop, hopp = (hop + 31) & ~31;
  if (ldx != 2 * nbp) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_istft: the spectrum pitch is not 2 * round_up(n_bins, 32), what the tables are built for");
  if (table_rows != J * 2 * nbp || table_cols != hopp)
    return jatts_set_error_msg(JATTS_ERR_ARG, "gl_istft: the table is not (ceil(n_fft / hop) * 2 nbp, round_up(hop, 32)) of this n_fft and hop");
  if ((const void*)X == (const void*)y) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_istft: X and y must be distinct buffers");
  if (rg_frames->n_seq <= 0 || max_frames < 2) return JATTS_OK;
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  const int half = n_fft / 2;
  const int max_rows = (half + (max_frames - 1) * hop - 1) / hop - half / hop + 1;
  hipLaunchKernelGGL(gl_istft_kernel, dim3((unsigned)((max_rows + FT - 1) / FT), (unsigned)rg.n_seq, (unsigned)((hopp + BW - 1) / BW)), dim3(256), 0, S_, rg,
                     X, table, renv, n_fft, hop, hopp, nbp, J, packed ? 1 : 0, y);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gl_exp(const float* c, int32_t ldc, int32_t n_mels, int64_t rows, const float* scale, const float* mean, int32_t log_base,
                            float* out, int32_t ldo, void* stream) {
  if (!c || !scale || !mean || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_exp: null pointer");
  if (n_mels < 1 || ldc < n_mels || ldo < n_mels) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_exp: bad strides");
  if (log_base != 0 && log_base != 2 && log_base != 10) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_exp: log_base must be 0 (e), 2 or 10");
  if (c == out) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_exp: c and out must be distinct buffers");
  if (rows <= 0) return JATTS_OK;
  hipLaunchKernelGGL(gl_exp_kernel, dim3(rowwise_blocks(rows * ldo)), dim3(256), 0, S_, c, ldc, n_mels, rows, scale, mean, log_base, out, ldo);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gl_floor(const float* lin, int32_t ldl, int32_t n_bins, int64_t rows, float eps, float* out, int32_t ldo, void* stream) {
  if (!lin || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_floor: null pointer");
  if (n_bins < 1 || ldl < n_bins || ldo < n_bins) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_floor: bad strides");
  if (lin == out) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_floor: lin and out must be distinct buffers");
  if (rows <= 0) return JATTS_OK;
  hipLaunchKernelGGL(gl_floor_kernel, dim3(rowwise_blocks(rows * ldo)), dim3(256), 0, S_, lin, ldl, n_bins, rows, eps, out, ldo);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gl_init(const float* S, int32_t lds, const float* p0, int32_t n_fft, int64_t rows, float* X, int32_t ldx, void* stream) {
  if (!S || !p0 || !X) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_init: null pointer");
  if (n_fft < 64 || n_fft > 2048 || n_fft % 64) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_init: n_fft must be a multiple of 64, at most 2048");
  const int n_bins = n_fft / 2 + 1, nbp = (n_bins + 31) & ~31;
  if (lds < n_bins) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_init: lds < n_bins");
  if (ldx != 2 * nbp) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_init: the spectrum pitch is not 2 * round_up(n_bins, 32), what the tables are built for");
  if (S == X || p0 == X) return jatts_set_error_msg(JATTS_ERR_ARG, "gl_init: S, p0 and X must be distinct buffers");
  if (rows <= 0) return JATTS_OK;
  if (rows * ldx >= (int64_t)1 << 31) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "gl_init: launch too large");
  hipLaunchKernelGGL(gl_init_kernel, dim3(rowwise_blocks(rows * nbp)), dim3(256), 0, S_, S, lds, p0, n_bins, nbp, rows, X);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
