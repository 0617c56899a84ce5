// Pitch of stage 1: what jatts/modules/feature_extract/dio.py:100-146 gets from pyworld (DIO + StoneMask), here an
// autocorrelation F0 estimator of this project's own definition -- Boersma's 1993 method on the frames the STFT already forms -- pinned on a
// float64 restatement (tests/pitch_reference.py); parity with DIO / StoneMask is UNPINNED.  The steps after the raw track
// (_convert_to_continuous_f0, the log, _adjust_num_frames, _average_by_duration) ARE pinned on the real Dio.forward (tests/golden/pitch_post_kat.npz).
//
// The definition, for one utterance x (f32) at sr with n_fft, hop, f0min, f0max:
//   1. geometry: lo = ceil(sr / f0max), hi = floor(sr / f0min), W = min(3 hi, n_fft - hi - 1) rounded down to even; refused (on the host, before any
//      launch) when W < 2 hi or lo < 2.  W + hi < n_fft keeps the circular autocorrelation from wrapping;
//   2. frames: the STFT's own (center=True, numpy reflect, T = 1 + L / hop) under a periodic Hann window of length W centred in n_fft
//      (jatts_stft_mag with that window's table); P_t[k] = |X_t[k]|^2, k <= n_fft / 2;
//   3. autocorrelation: r_t(tau) = (1 / n_fft) sum_k c_k P_t[k] cos(2 pi k tau / n_fft), c_0 = c_{n_fft/2} = 1, else 2, tau = 0 .. hi + 1;
//      rho_t(tau) = r_t(tau) / max(r_t(0), 1e-30) * rw(0) / rw(tau), rw the window's own autocorrelation (float64);
//   4. candidates: every tau in [lo, hi] with rho(tau) >= rho(tau - 1) and rho(tau) > rho(tau + 1); with a, b, c = rho(tau - 1), rho(tau),
//      rho(tau + 1), den = a - 2 b + c: off = clip(0.5 (a - c) / den, -0.5, 0.5) if den < 0 else 0, peak = b - 0.25 (a - c) off,
//      score = peak - octave_cost * log2((tau + off) f0min / sr); the highest score wins, equal scores go to the smallest tau;
//   5. voicing: a candidate exists, peak >= voicing_threshold and sqrt(r_t(0) / sum w^2) >= silence_threshold * max |x| over the utterance;
//      f0_t = sr / (tau + off) when voiced, else 0;
//   6. Dio.forward's own steps (dio.py:110-159).
//
// acf_from_mag_kernel: step 3 as ONE exact-f32 framed contraction (framed_contract<1>, framed_contraction.h: the loop, its LDS tile, the wave
//   dealing and the two-level order of the sum live there).  The frame = one row of the magnitude spectrum (rows do not overlap), the sample
//   rule squares it (one f32 multiply); the table [K][Lp] (jatts_amd.features.acf_table) holds c_k cos(.) / n_fft * rw(0) / rw(tau), folded in
//   float64 and rounded once, zeros in its padding rows and columns.  No atomics: a frame's bits depend on its own row and the table only.
// pitch_pick_kernel: steps 4-5, one wave per frame, lanes stride the lags (three coalesced reads of the frame's row, no LDS); a lane keeps its
//   best candidate (lags ascend inside a lane: a later one must be strictly better), then a butterfly over (score, tau) under the tie rule.
// f0_continuous_log_kernel: step 6's first two parts, one workgroup per utterance: previous voiced frame = inclusive max-scan of (voiced ? t : -1),
//   next voiced frame = inclusive min-scan from the end of (voiced ? t : INT_MAX); the interpolation is f32.
#include "framed_contraction.h"

namespace {

__global__ __launch_bounds__(256, 2) void acf_from_mag_kernel(jatts_ragged rg, const float* __restrict__ mag, int ldm,
                                                             const float* __restrict__ table, int K, int Lp, float* __restrict__ r) {
  __shared__ __attribute__((aligned(16))) float tile[2][FT * PITCH];
  const int b = blockIdx.y;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const int t0 = blockIdx.x * FT;
  if (t0 >= T) return;
  const float* mb = mag + (int64_t)row0 * ldm;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, c = lane & 31;
  const framed_wave w = framed_deal(Lp, t0, T);
  const int col0 = w.col0;
  const unsigned fmask = w.fmask;

  f32x16 acc[2][1];     // [frame tile][the one plane]
  framed_contract<1>(tile, t0, T, K, table + (fmask ? col0 + c : 0), Lp, 0, fmask,
                     [&](int t, int k) {
                       const float m = mb[(int64_t)t * ldm + k];
                       return __fmul_rn(m, m);      // the power spectrum, one rounding
                     },
                     acc);

  // epilogue: C fragment col = lane & 31 (lag), row = (r & 3) + 8 (r >> 2) + 4 h (frame): 128-byte row segments per half wave
  if (!fmask) return;
  const int col = col0 + c;      // < Lp: the wave's tile is one of the table's
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    if (!(fmask >> f & 1)) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int fl = f * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (t0 + fl < T) r[(int64_t)(row0 + t0 + fl) * Lp + col] = acc[f][0][i];
    }
  }
}

struct pick_params {
  int lo, hi;
  float sr, f0min, sum_w2, voicing, silence, octave;
};

// (score, tau) order of step 4: the higher score, then the smaller lag
__device__ __forceinline__ bool pick_better(float s, int t, float s0, int t0) { return s > s0 || (s == s0 && t < t0); }

__global__ __launch_bounds__(256) void pitch_pick_kernel(jatts_ragged rg, const float* __restrict__ r, int ldr, const float* __restrict__ peak,
                                                        int peak_stride, pick_params p, float* __restrict__ f0, int32_t* __restrict__ tau_out) {
  const int b = blockIdx.y;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);      // wave-uniform
  if (t >= T) return;
  const int lane = threadIdx.x & 63;
  const float* rr = r + (int64_t)(row0 + t) * ldr;
  const float r0 = rr[0];
  const float d0 = fmaxf(r0, 1.0e-30f);

  float best_s = -INFINITY, best_off = 0.f, best_pk = 0.f;
  int best_tau = INT_MAX;
  for (int tau = p.lo + lane; tau <= p.hi; tau += 64) {
    const float a = rr[tau - 1] / d0, bb = rr[tau] / d0, c = rr[tau + 1] / d0;
    if (!(bb >= a && bb > c)) continue;
    const float den = (a - 2.f * bb) + c;
    float off = 0.f;
    if (den < 0.f) off = fminf(fmaxf(0.5f * (a - c) / den, -0.5f), 0.5f);
    const float pk = bb - 0.25f * (a - c) * off;
    const float s = pk - p.octave * log2f(((float)tau + off) * p.f0min / p.sr);
    if (s > best_s) {      // lags ascend inside a lane: an equal score stays with the smaller one
      best_s = s;
      best_tau = tau;
      best_off = off;
      best_pk = pk;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s = __shfl_xor(best_s, o), of = __shfl_xor(best_off, o), pk = __shfl_xor(best_pk, o);
    const int ta = __shfl_xor(best_tau, o);
    if (pick_better(s, ta, best_s, best_tau)) {
      best_s = s;
      best_tau = ta;
      best_off = of;
      best_pk = pk;
    }
  }
  if (lane == 0) {
    const bool cand = best_tau != INT_MAX;
    const bool voiced = cand && best_pk >= p.voicing && sqrtf(r0 / p.sum_w2) >= p.silence * peak[(int64_t)b * peak_stride];
    f0[row0 + t] = voiced ? p.sr / ((float)best_tau + best_off) : 0.f;
    if (tau_out) tau_out[row0 + t] = cand ? best_tau : 0;
  }
}

constexpr int SCAN_THREADS = 1024;

// One workgroup per utterance.  Pass 1 (chunks ascending): prev[t] = the last voiced frame <= t, parked in out[t] as an integer.  Pass 2
// (chunks descending): next[t] = the first voiced frame >= t, then the value.  A thread reads back only what it wrote itself.
__global__ __launch_bounds__(SCAN_THREADS) void f0_continuous_log_kernel(jatts_ragged rg, const float* __restrict__ f0, int use_continuous,
                                                                       int use_log, float* __restrict__ out) {
  __shared__ int wave_tot[SCAN_THREADS / 64];
  const int b = blockIdx.x;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const float* fb = f0 + row0;
  float* ob = out + row0;
  int* pb = reinterpret_cast<int*>(ob);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_chunks = (T + SCAN_THREADS - 1) / SCAN_THREADS;

  if (use_continuous) {
    int carry = -1;
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int t = ch * SCAN_THREADS + tid;
      int v = (t < T && fb[t] != 0.f) ? t : -1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o);
        if (lane >= o) v = max(v, u);
      }
      if (lane == 63) wave_tot[wv] = v;
      __syncthreads();
      int before = carry;
      for (int j = 0; j < wv; ++j) before = max(before, wave_tot[j]);
      int all = carry;
      for (int j = 0; j < SCAN_THREADS / 64; ++j) all = max(all, wave_tot[j]);
      if (t < T) pb[t] = max(v, before);
      carry = all;
      __syncthreads();
    }
  }
  int carry = INT_MAX;
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int t = ch * SCAN_THREADS + tid;
    float val = t < T ? fb[t] : 0.f;
    if (use_continuous) {
      int v = (t < T && val != 0.f) ? t : INT_MAX;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_down(v, o);
        if (lane + o < 64) v = min(v, u);
      }
      if (lane == 0) wave_tot[wv] = v;
      __syncthreads();
      int after = carry;
      for (int j = wv + 1; j < SCAN_THREADS / 64; ++j) after = min(after, wave_tot[j]);
      int all = carry;
      for (int j = 0; j < SCAN_THREADS / 64; ++j) all = min(all, wave_tot[j]);
      carry = all;
      __syncthreads();
      if (t < T && val == 0.f) {
        const int nx = min(v, after), pv = pb[t];
        if (pv < 0 && nx == INT_MAX) val = 0.f;                 // all unvoiced: left as zeros (dio.py:127-129)
        else if (pv < 0) val = fb[nx];                          // the lead takes the first voiced value
        else if (nx == INT_MAX) val = fb[pv];                   // the tail the last
        else {
          const float y0 = fb[pv], y1 = fb[nx];
          val = fmaf((float)(t - pv), (y1 - y0) / (float)(nx - pv), y0);      // scipy's interp1d: slope * (x - x_lo) + y_lo
        }
      }
    }
    if (t < T) {
      // through double: the f32 result is the correctly rounded logarithm (as logmel_post_kernel)
      if (use_log && val != 0.f) val = (float)log((double)val);
      ob[t] = val;
    }
  }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int jatts_acf_from_mag(const jatts_ragged* rg_frames, const float* mag, int32_t ldm, const float* table, int32_t K, int32_t Lp,
                                  float* r, void* stream) {
  if (!rg_frames || !mag || !table || !r) return jatts_set_error_msg(JATTS_ERR_ARG, "acf_from_mag: null pointer");
  if (K < KC || K % KC || K > 1088) return jatts_set_error_msg(JATTS_ERR_ARG, "acf_from_mag: K must be a multiple of 64, at most 1088");
  if (Lp < 32 || Lp % 32 || Lp > 2048) return jatts_set_error_msg(JATTS_ERR_ARG, "acf_from_mag: Lp must be a multiple of 32, at most 2048");
  if (ldm < K) return jatts_set_error_msg(JATTS_ERR_ARG, "acf_from_mag: ldm < K (the spectrum's rows must be padded to K, padding zero)");
  if (rg_frames->n_seq <= 0 || rg_frames->max_len <= 0) return JATTS_OK;
  if (rg_frames->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "acf_from_mag: more than 65535 utterances (split the batch)");
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  hipLaunchKernelGGL(acf_from_mag_kernel, dim3((unsigned)((rg.max_len + FT - 1) / FT), (unsigned)rg.n_seq, (unsigned)((Lp + BW - 1) / BW)), dim3(256), 0,
                     S_, rg, mag, ldm, table, K, Lp, r);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_pitch_pick(const jatts_ragged* rg_frames, const float* r, int32_t ldr, const float* peak, int32_t peak_stride, int32_t lo,
                                int32_t hi, float sr, float f0min, float sum_w2, float voicing_threshold, float silence_threshold,
                                float octave_cost, float* f0, int32_t* tau, void* stream) {
  if (!rg_frames || !r || !peak || !f0) return jatts_set_error_msg(JATTS_ERR_ARG, "pitch_pick: null pointer");
  if (lo < 2 || hi < lo || ldr < hi + 2) return jatts_set_error_msg(JATTS_ERR_ARG, "pitch_pick: 2 <= lo <= hi and ldr >= hi + 2 expected");
  if (peak_stride < 1 || !(sr > 0.f) || !(f0min > 0.f) || !(sum_w2 > 0.f))
    return jatts_set_error_msg(JATTS_ERR_ARG, "pitch_pick: peak_stride, sr, f0min and sum_w2 must be positive");
  if (rg_frames->n_seq <= 0 || rg_frames->max_len <= 0) return JATTS_OK;
  if (rg_frames->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "pitch_pick: more than 65535 utterances (split the batch)");
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  const pick_params p = {lo, hi, sr, f0min, sum_w2, voicing_threshold, silence_threshold, octave_cost};
  hipLaunchKernelGGL(pitch_pick_kernel, dim3((unsigned)((rg.max_len + 3) / 4), (unsigned)rg.n_seq), dim3(256), 0, S_, rg, r, ldr, peak, peak_stride, p,
                     f0, tau);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_f0_continuous_log(const jatts_ragged* rg_frames, const float* f0, int32_t use_continuous, int32_t use_log, float* out,
                                       void* stream) {
  if (!rg_frames || !f0 || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "f0_continuous_log: null pointer");
  if (f0 == out) return jatts_set_error_msg(JATTS_ERR_ARG, "f0_continuous_log: out must not alias f0");
  if (rg_frames->n_seq <= 0 || rg_frames->max_len <= 0) return JATTS_OK;
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  hipLaunchKernelGGL(f0_continuous_log_kernel, dim3((unsigned)rg.n_seq), dim3(SCAN_THREADS), 0, S_, rg, f0, use_continuous, use_log, out);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
