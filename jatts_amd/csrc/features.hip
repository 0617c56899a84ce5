// Stage-1 features of the recipes: the magnitude STFT behind jatts/modules/feature_extract/mel.py:44-52 and
// energy.py:77-89 (librosa.stft, center=True, pad_mode="reflect", np.abs) as ONE exact-f32 contraction over raw samples, and the row-wise
// pieces around it: log of the mel projection (mel.py:64-73), frame energy (energy.py:89), length adjustment (energy.py:116-122) and the
// token average (energy.py:103-114).  The mel projection itself is a jatts_conv1d launch (k = 1, exact f32).
//
// stft_mag_kernel: out[frame][bin] = | sum_n x[refl(frame * hop + n - n_fft / 2)] * (w[n] cos(2 pi n bin / N) - i w[n] sin(2 pi n bin / N)) |
//   * the window is folded into the table on the host (float64, rounded once): table[n][col], col < nbp the cosines, nbp + col the sines;
//   * the contraction itself is framed_contract<2> (framed_contraction.h: tile staging, the banking argument, the wave dealing and why the
//     sum runs in 64-term chunks added in order): A operand = frames of n_fft samples hop apart, read under numpy's reflect rule while they are
//     staged.  Reading span[f * hop + n] from one staged span instead would put the 32 frame lanes hop floats apart: at hop 256 all on one bank.
//     Neither the frame matrix nor the complex spectrum ever reaches HBM;
//   * B operand = the table, both planes of a bin in the same lane (cosine and sine tile of the same 32 bins per wave), so |.| is the epilogue.
//     The table is the traffic (16.8 MB at n_fft 2048 against 1.2 KB of samples per frame, n_fft / hop reads per sample): the grid runs frame
//     tiles fastest, bin tiles slowest, so the workgroups resident at any time walk the same 2 MB slice of the table together;
//   * pow_sum: per (workgroup, frame) the sum of re^2 + im^2 over the workgroup's bins in a fixed tree (lanes, then waves), stored to the
//     reduction scratch; a second launch adds the bin tiles in order.  No atomics: a frame's bits depend on its own samples only.
#include "det_reduce.h"
#include "framed_contraction.h"

namespace {

__device__ __forceinline__ int reflect_index(int p, int L) {
  p = p < 0 ? -p : p;
  p = p >= L ? 2 * (L - 1) - p : p;
  return min(max(p, 0), L - 1);     // (never taken for frames t <= L / hop of an utterance with L > n_fft / 2: the entry point's conditions)
}

__global__ __launch_bounds__(256, 2) void stft_mag_kernel(jatts_ragged rg, const int32_t* __restrict__ cu_samples, const float* __restrict__ x,
                                                         const float* __restrict__ table, int n_fft, int hop, int n_bins, int nbp,
                                                         float* __restrict__ out, int ldo, float* __restrict__ pow_part) {
  __shared__ __attribute__((aligned(16))) float tile[2][FT * PITCH];
  const int b = blockIdx.y;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const int t0 = blockIdx.x * FT;
  if (t0 >= T) return;
  const int s0 = cu_samples[b], L = cu_samples[b + 1] - s0;
  const float* xb = x + s0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = lane >> 5, c = lane & 31;
  const framed_wave w = framed_deal(nbp, t0, T);      // one 32-bin tile (n_bins = n_fft / 2 + 1: ONE in the last workgroup at every power of two)
  const int slot = w.slot, bin0 = w.col0;
  const unsigned fmask = w.fmask;
  const int half = n_fft >> 1;

  f32x16 acc[2][2];     // [frame tile][re | im]
  framed_contract<2>(tile, t0, T, n_fft, table + (fmask ? bin0 + c : 0), 2 * nbp, nbp, fmask,
                     [&](int t, int k) { return xb[reflect_index(t * hop + k - half, L)]; }, acc);

  // epilogue: C fragment col = lane & 31 (bin), row = (r & 3) + 8 (r >> 2) + 4 h (frame): 128-byte row segments per half wave
  const int bin = bin0 + c;
  float* red = tile[0];          // [4 bin tiles][64 frames] partial power sums (every tile read is behind the loop's last barrier)
  if (pow_part) {
    red[tid] = 0.f;              // bin tiles this workgroup does not have, frame tiles it skipped
    __syncthreads();
  }
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!(fmask >> f & 1)) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fl = f * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const float re = acc[f][0][r], im = acc[f][1][r];
      float p = bin < n_bins ? fmaf(re, re, im * im) : 0.f;      // (spelled out: the contraction is not left to the compiler)
      if (bin < n_bins && t0 + fl < T) out[(int64_t)(row0 + t0 + fl) * ldo + bin] = sqrtf(p);
      if (pow_part) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) p += __shfl_xor(p, o);     // within the half wave: fixed tree
        if (c == 0) red[slot * FT + fl] = p;
      }
    }
  }
  if (blockIdx.z == 0) {        // the zero columns n_bins .. ldo - 1
    const int zc = ldo - n_bins;
    for (int i = tid; i < FT * zc; i += 256) {
      const int fl = i / zc, k = i - fl * zc;
      if (t0 + fl < T) out[(int64_t)(row0 + t0 + fl) * ldo + n_bins + k] = 0.f;
    }
  }
  if (pow_part) {
    __syncthreads();
    if (tid < FT && t0 + tid < T)
      pow_part[(int64_t)blockIdx.z * rg.total_rows + row0 + t0 + tid] = ((red[tid] + red[FT + tid]) + red[2 * FT + tid]) + red[3 * FT + tid];
  }
}

// pow_sum[row] = sum over the bin tiles, in tile order
__global__ __launch_bounds__(256) void pow_finish_kernel(const float* part, int n_tiles, int rows, float* pow_sum) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  float s = part[r];
  for (int j = 1; j < n_tiles; ++j) s += part[(int64_t)j * rows + r];
  pow_sum[r] = s;
}

// out = log_b(max(eps, mel)); base: 0 = e, 2, 10; columns n_mels .. ldo - 1 = 0
__global__ __launch_bounds__(256) void logmel_post_kernel(const float* mel, int ldm, int n_mels, int64_t rows, float eps, int base, float* out, int ldo) {
  const int64_t total = rows * ldo;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / ldo;
    const int k = (int)(i - r * ldo);
    float v = 0.f;
    if (k < n_mels) {
      // through double: the f32 result is the correctly rounded logarithm (log10f / logf are 1-2 ulp; 80 values per frame cost nothing)
      const double m = (double)fmaxf(eps, mel[r * ldm + k]);
      v = (float)(base == 10 ? log10(m) : base == 2 ? log2(m) : log(m));
    }
    out[i] = v;
  }
}

__global__ __launch_bounds__(256) void energy_frames_kernel(const float* pow_sum, int64_t rows, float* e) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < rows) e[i] = sqrtf(fmaxf(pow_sum[i], 1.0e-10f));
}

// out_b[t] = t < len_in_b ? e_b[t] : 0 for t < len_out_b
__global__ __launch_bounds__(256) void energy_adjust_kernel(jatts_ragged rg_in, jatts_ragged rg_out, const float* e, float* out) {
  const int b = blockIdx.y;
  const int i0 = rg_in.cu_rows[b], Ti = rg_in.cu_rows[b + 1] - i0;
  const int o0 = rg_out.cu_rows[b], To = rg_out.cu_rows[b + 1] - o0;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < To; t += gridDim.x * 256) out[o0 + t] = t < Ti ? e[i0 + t] : 0.f;
}

// Per token: the mean of the strictly positive values of its span of d frames, 0 when there are none.  One thread per token walks its span
// in frame order (spans are a handful of frames).  cum[tok] = end of the token's span relative to its utterance: the inclusive scan of the
// durations, which the host holds anyway (it checks their sum against the adjusted length).
__global__ __launch_bounds__(256) void token_average_kernel(jatts_ragged rg_tok, jatts_ragged rg_frames, const int32_t* cum, const float* e,
                                                            float* out) {
  const int b = blockIdx.y;
  const int k0 = rg_tok.cu_rows[b], K = rg_tok.cu_rows[b + 1] - k0;
  const int f0 = rg_frames.cu_rows[b], T = rg_frames.cu_rows[b + 1] - f0;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < K; k += gridDim.x * 256) {
    const int a = k ? cum[k0 + k - 1] : 0;
    const int z = min(cum[k0 + k], T);
    float s = 0.f;
    int n = 0;
    for (int t = max(a, 0); t < z; ++t) {
      const float v = e[f0 + t];
      if (v > 0.f) { s += v; ++n; }
    }
    out[k0 + k] = n ? s / (float)n : 0.f;
  }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int jatts_stft_mag(const jatts_ragged* rg_frames, const int32_t* cu_samples, const int32_t* host_samples, const float* x,
                              const float* table, int32_t n_fft, int32_t hop, float* mag, int32_t ldo, float* pow_sum, const jatts_scratch* scratch,
                              void* stream) {
  if (!rg_frames || !cu_samples || !host_samples || !x || !table || !mag) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: null pointer");
  if (n_fft < 64 || n_fft > 2048 || n_fft % 64) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: n_fft must be a multiple of 64, at most 2048");
  if (hop < 1 || hop > n_fft) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: hop must lie in [1, n_fft]");
  const int n_bins = n_fft / 2 + 1, nbp = (n_bins + 31) & ~31;
  if (ldo < n_bins) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: ldo < n_bins");
  if (rg_frames->n_seq <= 0) return JATTS_OK;
  if (rg_frames->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "stft_mag: more than 65535 utterances (split the batch)");
  int64_t rows = 0;
  int max_frames = 0;
  for (int b = 0; b < rg_frames->n_seq; ++b) {
    const int L = host_samples[b];
    if (L <= n_fft / 2) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: an utterance no longer than n_fft / 2 cannot be reflect-padded");
    const int T = 1 + L / hop;
    rows += T;
    max_frames = T > max_frames ? T : max_frames;
  }
  if (max_frames != rg_frames->max_len) return jatts_set_error_msg(JATTS_ERR_ARG, "stft_mag: frame geometry is not 1 + n_samples / hop");
  if (rows >= (int64_t)1 << 31) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "stft_mag: launch too large");
  const int n_tiles = (nbp + BW - 1) / BW;
  jatts_ws_t ws = {nullptr, nullptr};       // slabs only: one float per (bin tile, frame), summed per frame by pow_finish_kernel
  if (pow_sum)
    if (const int rc = jatts_ws_need(scratch, 0, (int64_t)n_tiles * rows, &ws)) return rc;
  float* part = ws.slabs;
  jatts_ragged rg = *rg_frames;
  rg.total_rows = (int32_t)rows;
  rg.host_lens = nullptr;
  hipLaunchKernelGGL(stft_mag_kernel, dim3((unsigned)((max_frames + FT - 1) / FT), (unsigned)rg.n_seq, (unsigned)n_tiles), dim3(256), 0, S_, rg,
                     cu_samples, x, table, n_fft, hop, n_bins, nbp, mag, ldo, part);
  JATTS_CHECK_LAUNCH();
  if (pow_sum) {
    hipLaunchKernelGGL(pow_finish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S_, part, n_tiles, (int)rows, pow_sum);
    JATTS_CHECK_LAUNCH();
  }
  return JATTS_OK;
}

extern "C" int jatts_logmel_post(const float* mel, int32_t ldm, int32_t n_mels, int64_t rows, float eps, int32_t log_base, float* out,
                                 int32_t ldo, void* stream) {
  if (!mel || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "logmel_post: null pointer");
  if (n_mels < 1 || ldm < n_mels || ldo < n_mels) return jatts_set_error_msg(JATTS_ERR_ARG, "logmel_post: bad strides");
  if (log_base != 0 && log_base != 2 && log_base != 10) return jatts_set_error_msg(JATTS_ERR_ARG, "logmel_post: log_base must be 0 (e), 2 or 10");
  if (rows <= 0) return JATTS_OK;
  const int64_t blocks = (rows * ldo + 255) / 256;
  hipLaunchKernelGGL(logmel_post_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, S_, mel, ldm, n_mels, rows, eps, log_base,
                     out, ldo);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_energy_frames(const float* pow_sum, int64_t rows, float* e, void* stream) {
  if (!pow_sum || !e) return jatts_set_error_msg(JATTS_ERR_ARG, "energy_frames: null pointer");
  if (rows <= 0) return JATTS_OK;
  if (rows >= (int64_t)1 << 31) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "energy_frames: launch too large");
  hipLaunchKernelGGL(energy_frames_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, S_, pow_sum, rows, e);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_energy_adjust(const jatts_ragged* rg_in, const jatts_ragged* rg_out, const float* e, float* out, void* stream) {
  if (!rg_in || !rg_out || !e || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "energy_adjust: null pointer");
  if (rg_in->n_seq != rg_out->n_seq) return jatts_set_error_msg(JATTS_ERR_ARG, "energy_adjust: the two geometries differ in n_seq");
  if (rg_out->n_seq <= 0 || rg_out->max_len <= 0) return JATTS_OK;
  if (rg_out->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "energy_adjust: more than 65535 utterances");
  const int gx = (rg_out->max_len + 255) / 256;
  hipLaunchKernelGGL(energy_adjust_kernel, dim3((unsigned)(gx < 64 ? gx : 64), (unsigned)rg_out->n_seq), dim3(256), 0, S_, *rg_in, *rg_out, e, out);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_token_average(const jatts_ragged* rg_tokens, const jatts_ragged* rg_frames, const int32_t* cum, const float* e, float* out,
                                   void* stream) {
  if (!rg_tokens || !rg_frames || !cum || !e || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "token_average: null pointer");
  if (rg_tokens->n_seq != rg_frames->n_seq) return jatts_set_error_msg(JATTS_ERR_ARG, "token_average: the two geometries differ in n_seq");
  if (rg_tokens->n_seq <= 0 || rg_tokens->max_len <= 0) return JATTS_OK;
  if (rg_tokens->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "token_average: more than 65535 utterances");
  const int gx = (rg_tokens->max_len + 255) / 256;
  hipLaunchKernelGGL(token_average_kernel, dim3((unsigned)(gx < 64 ? gx : 64), (unsigned)rg_tokens->n_seq), dim3(256), 0, S_, *rg_tokens, *rg_frames,
                     cum, e, out);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
