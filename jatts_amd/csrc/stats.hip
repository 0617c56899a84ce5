// Stage-1 statistics of the recipes: what jatts/bin/compute_statistics.py:75-103 does with one sklearn StandardScaler per feature
// (partial_fit per utterance, float64 throughout) and what jatts/datasets/tts_dataset.py:69-145 does with the result (StandardScaler.transform).
//
// State per column, float64, on the device for the accumulator's whole life: state[0][c] = n (samples seen), state[1][c] = mean,
// state[2][c] = M2 = sum (x - mean)^2.  One jatts_col_moments call = one partial_fit of rows x dim values:
//   * ONE pass over x.  The batch's moments are taken about a shift s[c] close to its mean: the running mean once the state holds samples,
//     the call's own first row before that.  With d = (double)x - s, S1 = sum d and S2 = sum d^2 the Chan / Golub / LeVeque pairwise update
//     (sklearn's _incremental_mean_and_var) of (n_a, mean_a, M2_a) with the batch (n_b, mean_b = s + S1 / n_b, M2_b = S2 - S1^2 / n_b),
//         M2 = M2_a + M2_b + (mean_b - mean_a)^2 n_a n_b / N,   N = n_a + n_b,
//     collapses, for s = mean_a, to   mean = s + S1 / N,   M2 = M2_a + S2 - S1^2 / N   (and the same two lines with M2_a = 0 are the first
//     call's).  |S1| / N is of the order of a standard deviation / sqrt(N), so S1^2 / N never cancels against S2 the way sum x^2 - N mean^2
//     does: a column of mean 1000 and spread 1e-3 keeps its variance to ~1e-13 where the raw sum of squares has no correct digit;
//   * FIXED ORDER.  The row range is cut into groups of JATTS_STATS_ROWS_PER_GROUP rows.  moments_part_kernel: one workgroup per (group,
//     column tile of 4 * cq columns), cq = the quads of four columns side by side in a workgroup (1, 2, 4 or 8: the next power of two of
//     dim / 4), 256 / cq row lanes.  A thread owns four consecutive columns of every (256 / cq)-th row of the group, in row order; the row
//     lanes are joined by a butterfly inside the wave (dim = 1: all 64 lanes of a wave hold rows, none idles on a missing column), the four
//     waves in wave order through LDS.  The workgroup writes S1 and S2 of its columns to the CALLER's workspace with plain stores.
//     moments_finish_kernel, ONE workgroup, a launch of its own behind it: adds the groups in group order (contiguous group ranges per
//     thread, then a fixed tree, when there are fewer columns than threads) and updates the state.  No atomics, no tickets: the state's
//     bits are a function of the sequence of calls, their rows and dim, never of ld, alignment or scheduling;
//   * the columns dim .. ld - 1 (LogMelExtractor's zero padding, or garbage) may ride along in a 16-byte load but never reach a sum
//     that is stored.
// NaN / infinity are not skipped (sklearn skips NaN): they poison the column's state, which FeatureStatistics.finalize refuses.
#include "common.h"

namespace {

constexpr int R = JATTS_STATS_ROWS_PER_GROUP;
constexpr int UNR = 8;            // rows a thread has in flight
constexpr int FT = 1024;          // threads of the finishing workgroup

__device__ __forceinline__ double shift_of(const double* state, int dim, const float* x, int c) {
  return state[c] > 0.0 ? state[dim + c] : (double)x[c];
}

__device__ __forceinline__ double wave_xor_add(double v, int o) { return v + __shfl_xor(v, o); }

// part[(g * 2 + k) * dim + c]: k = 0: S1, k = 1: S2 of the rows [g R, min(rows, (g + 1) R))
__global__ __launch_bounds__(256) void moments_part_kernel(const float* __restrict__ x, int ld, int dim, int64_t rows, const double* __restrict__ state,
                                                          int cq, int vec, double* __restrict__ part) {
  __shared__ double red[4][8][8];          // [wave][quad][S1 x 4 | S2 x 4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = tid & (cq - 1), rl = tid / cq, n_rl = 256 / cq;
  const int c0 = ((int)blockIdx.y * cq + q) * 4;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(rows - r0 < R ? rows - r0 : R);       // rows of this group (>= 1)
  const int nc = c0 < dim ? (dim - c0 < 4 ? dim - c0 : 4) : 0;   // live columns of this thread's quad

  double s[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < nc) s[e] = shift_of(state, dim, x, c0 + e);

  if (nc > 0) {
    const float* p = x + r0 * ld + c0;
    for (int i0 = rl; i0 < nr; i0 += UNR * n_rl) {
      f32x4 v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int i = i0 + u * n_rl;
        v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < nr) {
          const float* pr = p + (int64_t)i * ld;
          if (vec) {
            v[u] = *reinterpret_cast<const f32x4*>(pr);      // c0 + 3 < ld: ld % 4 == 0 and c0 < dim <= ld
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (e < nc) v[u][e] = pr[e];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (i0 + u * n_rl < nr) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double d = (double)v[u][e] - s[e];
            s1[e] += d;
            s2[e] = fma(d, d, s2[e]);
          }
        }
      }
    }
  }
  // row lanes of a wave: lanes q, q + cq, q + 2 cq ... (cq <= 8 divides 64)
  for (int o = 32; o >= cq; o >>= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s1[e] = wave_xor_add(s1[e], o);
      s2[e] = wave_xor_add(s2[e], o);
    }
  }
  if (lane < cq) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[wave][lane][e] = s1[e];
      red[wave][lane][4 + e] = s2[e];
    }
  }
  __syncthreads();
  if (tid < cq * 8) {
    const int qq = tid >> 3, k = tid & 7, e = k & 3;
    const int c = ((int)blockIdx.y * cq + qq) * 4 + e;
    if (c < dim) {
      const double t = ((red[0][qq][k] + red[1][qq][k]) + red[2][qq][k]) + red[3][qq][k];
      part[((int64_t)blockIdx.x * 2 + (k >> 2)) * dim + c] = t;
    }
  }
}

// One workgroup of FT threads.  cw = min(FT, next power of two of dim) column lanes, FT / cw group lanes: a single workgroup pulling sums that other
// XCDs wrote is latency-bound, so the groups are spread over as many lanes as the workgroup has (dim 80: eight lanes of six groups at the bench geometry).
__global__ __launch_bounds__(FT) void moments_finish_kernel(const float* __restrict__ x, int dim, int64_t rows, const double* __restrict__ part,
                                                            int n_groups, int cw, double* __restrict__ state) {
  __shared__ double red[2][FT];
  const int tid = threadIdx.x;
  const int cl = tid & (cw - 1), g_l = tid / cw, n_gl = FT / cw;
  const int g0 = (int)((int64_t)g_l * n_groups / n_gl), g1 = (int)((int64_t)(g_l + 1) * n_groups / n_gl);
  for (int cb = 0; cb < dim; cb += cw) {
    const int c = cb + cl;
    double a1 = 0.0, a2 = 0.0;
    if (c < dim) {
      const double* p = part + (int64_t)g0 * 2 * dim + c;
      int g = g0;
      for (; g + 4 <= g1; g += 4, p += 8 * (int64_t)dim) {          // eight loads in flight, added in group order
        double t1[4], t2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          t1[j] = p[(int64_t)(2 * j) * dim];
          t2[j] = p[(int64_t)(2 * j + 1) * dim];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a1 += t1[j];
          a2 += t2[j];
        }
      }
      for (; g < g1; ++g, p += 2 * (int64_t)dim) {
        a1 += p[0];
        a2 += p[dim];
      }
    }
    if (n_gl > 1) {             // (then cw >= dim: a single pass of the column loop)
      red[0][tid] = a1;
      red[1][tid] = a2;
      for (int h = n_gl >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (g_l < h) {
          red[0][tid] += red[0][tid + h * cw];
          red[1][tid] += red[1][tid + h * cw];
        }
      }
      a1 = red[0][tid];
      a2 = red[1][tid];
    }
    if (g_l == 0 && c < dim) {
      const double na = state[c], m2a = state[2 * dim + c];
      const double s = shift_of(state, dim, x, c);
      const double n = na + (double)rows;
      state[c] = n;
      state[dim + c] = s + a1 / n;
      const double m2b = a2 - a1 * a1 / n;                     // >= 0 up to rounding; NaN goes through
      state[2 * dim + c] = m2a + (m2b < 0.0 ? 0.0 : m2b);
    }
  }
}

// state <- state (+) other, the general pairwise update (either side may be empty)
__global__ __launch_bounds__(256) void moments_merge_kernel(double* __restrict__ state, const double* __restrict__ other, int dim) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= dim) return;
  const double na = state[c], nb = other[c];
  if (!(nb > 0.0)) return;
  const double mb = other[dim + c], m2b = other[2 * dim + c];
  if (!(na > 0.0)) {
    state[c] = nb;
    state[dim + c] = mb;
    state[2 * dim + c] = m2b;
    return;
  }
  const double ma = state[dim + c], m2a = state[2 * dim + c];
  const double n = na + nb, dl = mb - ma;
  state[c] = n;
  state[dim + c] = ma + dl * (nb / n);
  state[2 * dim + c] = (m2a + m2b) + dl * dl * (na * (nb / n));
}

// y = (x - mean[c]) / scale[c]: one correctly rounded subtract, one correctly rounded divide (no reciprocal, no contraction)
template <bool VEC>
__global__ __launch_bounds__(256) void standardize_kernel(const float* __restrict__ x, int ldx, int dim, int64_t rows, const float* __restrict__ mean,
                                                         const float* __restrict__ scale, float* __restrict__ y, int ldy) {
  if (VEC) {
    const int nq = ldy >> 2;
    const int64_t total = rows * nq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int64_t r = i / nq;
      const int c0 = (int)(i - r * nq) * 4;
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (c0 + 4 <= dim) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ldx + c0);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mean + c0), s = *reinterpret_cast<const f32x4*>(scale + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fdiv_rn(__fsub_rn(v[e], m[e]), s[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < dim) o[e] = __fdiv_rn(__fsub_rn(x[r * ldx + c0 + e], mean[c0 + e]), scale[c0 + e]);
      }
      *reinterpret_cast<f32x4*>(y + r * ldy + c0) = o;
    }
  } else {
    const int64_t total = rows * ldy;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
      const int64_t r = i / ldy;
      const int c = (int)(i - r * ldy);
      y[i] = c < dim ? __fdiv_rn(__fsub_rn(x[r * ldx + c], mean[c]), scale[c]) : 0.f;
    }
  }
}

inline int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int32_t jatts_stats_rows_per_group(void) { return R; }

extern "C" int jatts_col_moments(const float* x, int32_t ld, int32_t dim, int64_t rows, double* state, double* ws, int64_t ws_doubles, void* stream) {
  if (dim < 1 || ld < dim) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments: need 1 <= dim <= ld");
  if (rows < 0) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments: negative row count");
  if (rows == 0) return JATTS_OK;
  if (!x || !state || !ws) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments: null pointer");
  const int64_t n_groups = (rows + R - 1) / R;
  if (n_groups > 0x7fffffff) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "col_moments: launch too large (split the call)");
  if (ws_doubles < n_groups * 2 * dim) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments: workspace smaller than ceil(rows / JATTS_STATS_ROWS_PER_GROUP) * 2 * dim doubles");
  const int cq = pow2_ceil((dim + 3) / 4) < 8 ? pow2_ceil((dim + 3) / 4) : 8;
  const int n_ct = (dim + 4 * cq - 1) / (4 * cq);
  if (n_ct > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "col_moments: more than 2 097 120 columns");
  const int vec = (ld % 4 == 0) && (reinterpret_cast<uintptr_t>(x) % 16 == 0);
  hipLaunchKernelGGL(moments_part_kernel, dim3((unsigned)n_groups, (unsigned)n_ct), dim3(256), 0, S_, x, ld, dim, rows, state, cq, vec, ws);
  JATTS_CHECK_LAUNCH();
  const int cw = dim >= FT ? FT : pow2_ceil(dim);
  hipLaunchKernelGGL(moments_finish_kernel, dim3(1), dim3(FT), 0, S_, x, dim, rows, ws, (int)n_groups, cw, state);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_col_moments_merge(double* state, const double* other, int32_t dim, void* stream) {
  if (!state || !other) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments_merge: null pointer");
  if (dim < 1) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments_merge: dim < 1");
  if (state == other) return jatts_set_error_msg(JATTS_ERR_ARG, "col_moments_merge: a state cannot be merged into itself");
  hipLaunchKernelGGL(moments_merge_kernel, dim3((unsigned)((dim + 255) / 256)), dim3(256), 0, S_, state, other, dim);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_standardize(const float* x, int32_t ldx, int32_t dim, int64_t rows, const float* mean, const float* scale, float* y, int32_t ldy,
                                 void* stream) {
  if (dim < 1 || ldx < dim || ldy < dim) return jatts_set_error_msg(JATTS_ERR_ARG, "standardize: bad strides");
  if (rows < 0) return jatts_set_error_msg(JATTS_ERR_ARG, "standardize: negative row count");
  if (rows == 0) return JATTS_OK;
  if (!x || !mean || !scale || !y) return jatts_set_error_msg(JATTS_ERR_ARG, "standardize: null pointer");
  auto al16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; };
  const bool vec = ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && al16(mean) && al16(scale);
  const int64_t items = vec ? rows * (ldy / 4) : rows * ldy;
  const int64_t blocks = (items + 255) / 256;
  const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192));
  if (vec) hipLaunchKernelGGL(standardize_kernel<true>, grid, dim3(256), 0, S_, x, ldx, dim, rows, mean, scale, y, ldy);
  else hipLaunchKernelGGL(standardize_kernel<false>, grid, dim3(256), 0, S_, x, ldx, dim, rows, mean, scale, y, ldy);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
