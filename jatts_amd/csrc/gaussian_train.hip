// Masked Gaussian upsampling for the MAS trainers (MatchaTTS_MAS, mel-VITS): the training form of GaussianUpsampling.forward
// (modules/length_regulator.py:111-154) on the padded batch, forward and the gradient for hs.
//   c_j = cumsum(ds)_j - ds_j / 2;  frame f < kvo[b] sits at t = f, a padded frame at t = 0 (the reference multiplies t by the frame mask);
//   p[b,f,j] = softmax_j(-delta (t - c_j)^2) over the tokens j < kv[b], 0 at the others;  out[b,f,:] = sum_j p[b,f,j] hs[b,j,:] for ALL To frames.
// The weights never reach HBM: the forward computes them once per (frame, token) into LDS (one expf per pair) and keeps (max, 1 / denominator) per
// frame; the backward recomputes p = expf(e - max) / denominator from those (again one expf per pair, no second reduction).  Both contractions run on
// the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32, the fragment layout of jatts_bgemm): no f16 / bf16 operand anywhere.  Every sum has one fixed
// order (tokens / frames increasing inside one workgroup; no split over the contraction, no atomics), so two runs are bit-identical.
#include "common.h"

namespace {

constexpr int GU_TMAX = 512;        // tokens per utterance, as jatts_alignment_logp
constexpr int GU_FT = 64;           // forward: frames per workgroup (two 32-row fragments per wave)
constexpr int GU_PP = GU_FT + 1;    // pitch of the weight tile ps[token][frame]: lanes-along-tokens stores hit 64 distinct banks
constexpr int GB_TT = 32;           // backward: tokens per workgroup (one fragment)
constexpr int GB_NT = 128;          //           channels per workgroup (one 32-column fragment per wave)
constexpr int GB_FK = 32;           //           frames per staged chunk
constexpr int GB_PP = GB_FK + 1;

// cen[j] = cumsum(ds)_j - ds_j / 2 for j < Tm (float).  256 threads, two tokens each: a wave scan, then the four wave totals in order.  The durations
// are integer-valued (MAS counts), so the partial sums are exact whatever their order.  The caller puts a barrier behind it.
__device__ __forceinline__ void gu_centres(const float* __restrict__ ds, int Tm, float* cen, float* wtot) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float a = 2 * t < Tm ? ds[2 * t] : 0.f, b = 2 * t + 1 < Tm ? ds[2 * t + 1] : 0.f;
  float s = a + b;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(s, o);
    if (lane >= o) s += v;
  }
  float excl = __shfl_up(s, 1);
  if (lane == 0) excl = 0.f;
  if (lane == 63) wtot[wave] = s;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  const float ca = base + excl + a, cb = ca + b;
  if (2 * t < Tm) cen[2 * t] = ca - a / 2;
  if (2 * t + 1 < Tm) cen[2 * t + 1] = cb - b / 2;
}

// energy and un-normalised weight of one (frame, token) pair, each operation rounded on its own: FMA contraction is switched OFF for these lines (hipcc's
// default contracts, and __fmul_rn / __fsub_rn are plain operators in HIP).  The backward must reproduce the forward's values bit for bit: contracted into
// fma(-delta, d^2, -max) its e - max differs from the forward's by up to half an ulp of e -- 2e-6 of every weight of a frame at |e| = 60 (frames far behind
// the last centre), against a denominator that was summed from the uncontracted values.
__device__ __forceinline__ float gu_energy(float delta, float t, float c) {
#pragma clang fp contract(off)
  const float d = t - c;
  const float dd = d * d;
  return -delta * dd;
}
__device__ __forceinline__ float gu_weight(float e, float mx) {
#pragma clang fp contract(off)
  const float x = e - mx;
  return expf(x);
}

__global__ __launch_bounds__(256) void gauss_up_fwd_kernel(const float* __restrict__ hs, const float* __restrict__ ds, const int32_t* __restrict__ kv,
                                                           const int32_t* __restrict__ kvo, int Tm, int To, int C, float delta,
                                                           float* __restrict__ out, float* __restrict__ stat) {
  extern __shared__ __attribute__((aligned(16))) float gu_sm[];
  float* cen = gu_sm;               // [GU_TMAX]
  float* ps = gu_sm + GU_TMAX;      // [round_up(Tm, 2)][GU_PP]
  __shared__ float wtot[4];
  const int b = blockIdx.y, f0 = blockIdx.x * GU_FT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kvb = min(max(kv[b], 0), Tm), nfr = kvo[b];      // (nfr is only compared with frame indices: no clamp needed; kvb == 0 -> zero rows)
  const int K2 = (kvb + 1) & ~1;    // contraction length, rounded up to the K = 2 of one MFMA: the extra row carries zero weights
  gu_centres(ds + (int64_t)b * Tm, Tm, cen, wtot);
  __syncthreads();
  for (int fi = wave; fi < GU_FT; fi += 4) {
    const int f = f0 + fi;
    const float t = f < nfr ? (float)f : 0.f;
    float e[GU_TMAX / 64];
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < GU_TMAX / 64; ++s) {
      const int j = lane + 64 * s;
      e[s] = -INFINITY;
      if (j < kvb) {
        e[s] = gu_energy(delta, t, cen[j]);
        mx = fmaxf(mx, e[s]);
      }
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < GU_TMAX / 64; ++s) {
      const int j = lane + 64 * s;
      e[s] = j < kvb ? gu_weight(e[s], mx) : 0.f;
      sum += e[s];
    }
    sum = wave_sum(sum);
    const float inv = kvb > 0 ? 1.f / sum : 0.f;
#pragma unroll
    for (int s = 0; s < GU_TMAX / 64; ++s) {
      const int j = lane + 64 * s;
      if (j < K2) ps[j * GU_PP + fi] = e[s] * inv;
    }
    if (lane == 0 && f < To) {
      stat[((int64_t)b * To + f) * 2] = mx;
      stat[((int64_t)b * To + f) * 2 + 1] = inv;
    }
  }
  __syncthreads();
  // out tile (64 frames x C) = ps^T (64 x K2) hs (K2 x C): a wave takes 32 channels at a time and both frame fragments, so an hs row is read once per
  // workgroup.  A operand: lane l holds p[frame l & 31][token 2 q + (l >> 5)]; B operand: hs[token 2 q + (l >> 5)][channel l & 31], straight from global
  // memory (128 contiguous bytes per half-wave), eight K-pairs in flight.  Every load is unconditional from a clamped address and masked afterwards.
  const int lo = lane & 31, hi = lane >> 5;
  const float* hb = hs + (int64_t)b * Tm * C;
  for (int n0 = 32 * wave; n0 < C; n0 += 128) {
    const int n = n0 + lo;
    const bool nok = n < C;
    const int nc = nok ? n : C - 1;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    for (int k0 = 0; k0 < K2; k0 += 16) {
      float bv[8], a0[8], a1[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int k = k0 + 2 * q + hi;
        const int kc = k < kvb ? k : kvb - 1;      // (K2 > 0 implies kvb >= 1)
        const float v = hb[(int64_t)kc * C + nc];
        bv[q] = (k < kvb && nok) ? v : 0.f;
        const int ka = k < K2 ? k : K2 - 1;        // rows below K2 are initialised and finite; their partner bv is 0 past kvb
        a0[q] = ps[ka * GU_PP + lo];
        a1[q] = ps[ka * GU_PP + 32 + lo];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[q], bv[q], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[q], bv[q], acc1, 0, 0, 0);
      }
    }
    // C/D map: column (lane & 31) = channel, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = frame
    if (nok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (f0 + m < To) out[((int64_t)b * To + f0 + m) * C + n] = acc0[r];
        if (f0 + 32 + m < To) out[((int64_t)b * To + f0 + 32 + m) * C + n] = acc1[r];
      }
    }
  }
}

// d_hs tile (32 tokens x 128 channels of one utterance) = sum over ALL To frames, in increasing order, of p[f][j] g[f][:].  The weights of 32 frames x 32
// tokens are recomputed into a double-buffered LDS chunk (four pairs per thread, one barrier per chunk); g comes straight from global memory.
__global__ __launch_bounds__(256) void gauss_up_bwd_kernel(const float* __restrict__ g, const float* __restrict__ ds, const float* __restrict__ stat,
                                                           const int32_t* __restrict__ kv, const int32_t* __restrict__ kvo, int Tm, int To, int C,
                                                           float delta, float* __restrict__ dhs) {
  __shared__ float cen[GU_TMAX];
  __shared__ float wtot[4];
  __shared__ float ps[2][GB_FK * GB_PP];      // [frame][token]
  const int b = blockIdx.z, j0 = blockIdx.x * GB_TT, c0 = blockIdx.y * GB_NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kvb = min(max(kv[b], 0), Tm), nfr = kvo[b];
  float* ob = dhs + (int64_t)b * Tm * C;
  if (j0 >= kvb) {      // a tile of padded tokens: exact zeros
    for (int u = tid; u < GB_TT * GB_NT; u += 256) {
      const int j = j0 + u / GB_NT, n = c0 + u % GB_NT;
      if (j < Tm && n < C) ob[(int64_t)j * C + n] = 0.f;
    }
    return;
  }
  gu_centres(ds + (int64_t)b * Tm, Tm, cen, wtot);
  __syncthreads();
  const int lo = lane & 31, hi = lane >> 5;
  const int n = c0 + 32 * wave + lo;
  const bool nok = n < C;
  const int nc = nok ? n : C - 1;
  const int tj = tid & 31, fq = tid >> 5;      // this thread's pairs: token j0 + tj, frames f0 + fq + 8 s
  const bool jok = j0 + tj < kvb;
  const float cj = jok ? cen[j0 + tj] : 0.f;
  const float* gb = g + (int64_t)b * To * C;
  const f32x2* sb = reinterpret_cast<const f32x2*>(stat) + (int64_t)b * To;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int f0 = 0; f0 < To; f0 += GB_FK) {
    float* pc = ps[(f0 / GB_FK) & 1];
    f32x2 st[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = f0 + fq + 8 * s;
      st[s] = sb[f < To ? f : To - 1];
    }
    float bv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int f = f0 + 2 * q + hi;
      const float v = gb[(int64_t)(f < To ? f : To - 1) * C + nc];
      bv[q] = (f < To && nok) ? v : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int f = f0 + fq + 8 * s;
      const float t = f < nfr ? (float)f : 0.f;
      const float p = gu_weight(gu_energy(delta, t, cj), st[s][0]) * st[s][1];
      pc[(fq + 8 * s) * GB_PP + tj] = (f < To && jok) ? p : 0.f;
    }
    __syncthreads();      // (the buffer written two chunks on was last read before the barrier of the chunk in between)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pc[(2 * q + hi) * GB_PP + lo], bv[q], acc, 0, 0, 0);
  }
  if (nok) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * hi;
      if (j < Tm) ob[(int64_t)j * C + n] = j < kvb ? acc[r] : 0.f;      // padded tokens: exact zeros
    }
  }
}

int gu_check(const char* who, const void* p0, const void* p1, const void* p2, const void* p3, const void* p4, const void* p5, const void* p6, int B, int Tm,
             int To, int C) {
  static thread_local char msg[160];
  if (!p0 || !p1 || !p2 || !p3 || !p4 || !p5 || !p6) {
    snprintf(msg, sizeof msg, "%s: null pointer", who);
    return jatts_set_error_msg(JATTS_ERR_ARG, msg);
  }
  if (B < 0 || Tm < 0 || To < 0 || C < 0 || B > 65535) {
    snprintf(msg, sizeof msg, "%s: bad size", who);
    return jatts_set_error_msg(JATTS_ERR_ARG, msg);
  }
  if (Tm > GU_TMAX) {
    snprintf(msg, sizeof msg, "%s: text length must be <= 512", who);
    return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, msg);
  }
  return JATTS_OK;
}

}  // namespace

extern "C" int jatts_gaussian_upsample_fwd(const float* hs, const float* ds, const int32_t* kv, const int32_t* kvo, int32_t B, int32_t Tm, int32_t To,
                                           int32_t C, float delta, float* out, float* stat, void* stream) {
  const int rc = gu_check("gaussian_upsample_fwd", hs, ds, kv, kvo, out, stat, stat, B, Tm, To, C);
  if (rc != JATTS_OK) return rc;
  if (B == 0 || Tm == 0 || To == 0 || C == 0) return JATTS_OK;
  const size_t lds = ((size_t)GU_TMAX + (size_t)((Tm + 1) & ~1) * GU_PP) * sizeof(float);
  JATTS_RAISE_LDS_LIMIT(gauss_up_fwd_kernel);
  hipLaunchKernelGGL(gauss_up_fwd_kernel, dim3((unsigned)((To + GU_FT - 1) / GU_FT), (unsigned)B), dim3(256), lds, (hipStream_t)stream, hs, ds, kv, kvo,
                     Tm, To, C, delta, out, stat);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gaussian_upsample_bwd(const float* g, const float* ds, const float* stat, const int32_t* kv, const int32_t* kvo, int32_t B,
                                           int32_t Tm, int32_t To, int32_t C, float delta, float* d_hs, void* stream) {
  const int rc = gu_check("gaussian_upsample_bwd", g, ds, stat, kv, kvo, d_hs, d_hs, B, Tm, To, C);
  if (rc != JATTS_OK) return rc;
  if (B == 0 || Tm == 0 || C == 0) return JATTS_OK;
  if (To == 0) return jatts_set_error_msg(JATTS_ERR_ARG, "gaussian_upsample_bwd: no frames");
  if ((C + GB_NT - 1) / GB_NT > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "gaussian_upsample_bwd: too many channels");
  hipLaunchKernelGGL(gauss_up_bwd_kernel, dim3((unsigned)((Tm + GB_TT - 1) / GB_TT), (unsigned)((C + GB_NT - 1) / GB_NT), (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, g, ds, stat, kv, kvo, Tm, To, C, delta, d_hs);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
