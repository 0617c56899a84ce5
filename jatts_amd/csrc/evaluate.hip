// Stage 5 (objective evaluation): what jatts/evaluate/dtw_based.py gets from fastdtw + scipy on the host, here the EXACT dynamic
// time warping of this project's own definition, with the frame selection in front of it and the reductions along the warping path behind it.
// Every kernel is pinned on a float64 / exact restatement (tests/evaluate_reference.py); parity with fastdtw (an approximation of the DTW built
// here), WORLD and librosa is UNPINNED.  All entries are ragged over a batch of utterances or pairs, take a stream, allocate nothing, use no
// atomics and give the same bits on every run.
//
// frame_select_kernel: one workgroup per utterance.  The threshold (mode 0: factor x the float64 mean, summed thread-strided then by a fixed
//   LDS tree; mode 1: zero; mode 2: factor x the maximum) is compared in float64; the selected frame indices are compacted in ascending order
//   by a chunked ballot scan (modes 0, 1) or reduced to (first, last) (mode 2).
// gather_rows_kernel: dst[cu_out[b] + k][:] = src[cu_src[b] + idx[cu_src[b] + k]][:], the selected rows packed.
// pairwise_dist_kernel: c[i][j] = sqrtf(sum_c (a_i[c] - b_j[c])^2), direct differences (the expanded |a|^2 + |b|^2 - 2 a.b form cancels: two
//   near rows would come out at the rounding noise of their norms), 64 x 64 output tiles from two LDS tiles of odd pitch.
// dtw_kernel<SLOTS>: one workgroup of 256 threads per pair, an anti-diagonal wavefront.  Thread t owns rows i = t + 256 m (m < SLOTS) and keeps
//   D[i][.] of the current diagonal in registers (float64); the previous diagonal lives in LDS indexed by row, double-buffered, so that row i
//   reads D[i - 1][j] from it and carries last diagonal's read on as D[i - 1][j - 1]: one barrier per diagonal.  A thread walks its own cost
//   row left to right, DTW_PF columns ahead through a register ring (as mas_kernel's MAS_PF), so no load sits on a diagonal's critical path.
//   Decisions (0 diagonal, 1 (i - 1, j), 2 (i, j - 1); ties in that order) go out 2 bits a cell, sixteen cells a 32-bit word, each row on its
//   own words (pitch ceil(M / 16)): a word has one writer.  A slot whose rows the diagonal does not touch is skipped (uniform).  Then one
//   thread walks the decisions back from (N - 1, M - 1) and the workgroup reverses the path in place.
// dtw_path_stats_kernel: one workgroup per pair, thread-strided float64 sums along the path joined by a fixed LDS tree.
#include "common.h"

namespace {

constexpr int EV_THREADS = 256;

// fixed tree over the workgroup's 256 partial values (LDS, the same order on every run); the result in every thread
__device__ __forceinline__ double block_tree_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = __dadd_rn(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(EV_THREADS) void frame_select_kernel(jatts_ragged rg, const float* __restrict__ val, int mode, double factor,
                                                                 int32_t* __restrict__ count, int32_t* __restrict__ idx) {
  __shared__ double red[EV_THREADS];
  __shared__ int wave_tot[EV_THREADS / 64];
  const int b = blockIdx.x;
  const int row0 = rg.cu_rows[b], T = rg.cu_rows[b + 1] - row0;
  const float* v = val + row0;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  double thr = 0.0;
  if (mode == 0) {
    double s = 0.0;
    for (int t = tid; t < T; t += EV_THREADS) s = __dadd_rn(s, (double)v[t]);
    s = block_tree_sum(s, red);
    thr = factor * (s / (double)max(T, 1));
  } else if (mode == 2) {
    double m = -INFINITY;
    for (int t = tid; t < T; t += EV_THREADS) m = fmax(m, (double)v[t]);
    __syncthreads();
    red[tid] = m;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
      __syncthreads();
    }
    thr = factor * red[0];
  }

  if (mode == 2) {      // (first, last) selected frame, -1 / -1 when none
    int first = INT_MAX, last = -1;
    for (int t = tid; t < T; t += EV_THREADS)
      if ((double)v[t] > thr) {
        first = min(first, t);
        last = max(last, t);
      }
    int* ired = reinterpret_cast<int*>(red);
    __syncthreads();
    ired[tid] = first;
    ired[EV_THREADS + tid] = last;
    __syncthreads();
    for (int s = EV_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        ired[tid] = min(ired[tid], ired[tid + s]);
        ired[EV_THREADS + tid] = max(ired[EV_THREADS + tid], ired[EV_THREADS + tid + s]);
      }
      __syncthreads();
    }
    if (tid == 0) {
      count[2 * b] = ired[0] == INT_MAX ? -1 : ired[0];
      count[2 * b + 1] = ired[EV_THREADS];
    }
    return;
  }

  int base = 0;      // selected frames before this chunk (uniform)
  for (int t0 = 0; t0 < T; t0 += EV_THREADS) {
    const int t = t0 + tid;
    const bool sel = t < T && (double)v[t] > thr;
    const unsigned long long m = __ballot(sel);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wv] = __popcll(m);
    __syncthreads();
    int off = base, all = base;
    for (int j = 0; j < EV_THREADS / 64; ++j) {
      if (j < wv) off += wave_tot[j];
      all += wave_tot[j];
    }
    if (sel) idx[row0 + off + before] = t;      // off + before < T: at most one entry per frame
    base = all;
    __syncthreads();
  }
  if (tid == 0) count[b] = base;
}

__global__ __launch_bounds__(EV_THREADS) void gather_rows_kernel(jatts_ragged rg_out, const int32_t* __restrict__ cu_src,
                                                                const int32_t* __restrict__ idx, const float* __restrict__ src, int lds,
                                                                int dim, float* __restrict__ dst, int ldd) {
  const int b = blockIdx.y;
  const int out0 = rg_out.cu_rows[b], n = rg_out.cu_rows[b + 1] - out0;
  const int src0 = cu_src[b], n_src = cu_src[b + 1] - src0;
  const int per = EV_THREADS / 64;      // one wave per row
  const int k = blockIdx.x * per + (threadIdx.x >> 6);
  if (k >= n) return;
  const int r = idx[src0 + k];
  if (r < 0 || r >= n_src) return;      // (never for indices jatts_frame_select wrote)
  for (int c = threadIdx.x & 63; c < dim; c += 64) dst[(int64_t)(out0 + k) * ldd + c] = src[(int64_t)(src0 + r) * lds + c];
}

// per pair: N, M, first row of a, first row of b, offset of c (floats)
constexpr int PD_T = 64;       // output tile
constexpr int PD_DMAX = 64;

__global__ __launch_bounds__(EV_THREADS) void pairwise_dist_kernel(const int64_t* __restrict__ tab, const float* __restrict__ a, int lda,
                                                                  const float* __restrict__ bm, int ldb, int dim, float* __restrict__ c) {
  __shared__ float sa[PD_T * (PD_DMAX + 1)];
  __shared__ float sb[PD_T * (PD_DMAX + 1)];
  const int64_t* tp = tab + (int64_t)blockIdx.z * 5;
  const int N = (int)tp[0], M = (int)tp[1];
  const int i0 = blockIdx.y * PD_T, j0 = blockIdx.x * PD_T;
  if (i0 >= N || j0 >= M) return;
  const float* ap = a + tp[2] * lda;
  const float* bp = bm + tp[3] * ldb;
  float* cp = c + tp[4];
  const int P = dim + 1 - (dim & 1);     // odd pitch (dim even -> dim + 1, dim odd -> dim): rows land on distinct banks
  for (int u = threadIdx.x; u < PD_T * dim; u += EV_THREADS) {
    const int r = u / dim, k = u - r * dim;
    sa[r * P + k] = ap[(int64_t)min(i0 + r, N - 1) * lda + k];
    sb[r * P + k] = bp[(int64_t)min(j0 + r, M - 1) * ldb + k];
  }
  __syncthreads();
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;      // rows 4 ty + r, columns tx + 16 q
  float s[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[r][q] = 0.f;
  for (int k = 0; k < dim; ++k) {
    float av[4], bv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) av[r] = sa[(4 * ty + r) * P + k];
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[q] = sb[(tx + 16 * q) * P + k];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float d = av[r] - bv[q];
        s[r][q] = __fadd_rn(s[r][q], __fmul_rn(d, d));
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * ty + r;
    if (i >= N) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx + 16 * q;
      if (j < M) cp[(int64_t)i * M + j] = sqrtf(s[r][q]);
    }
  }
}

constexpr int DTW_PF = 8;            // cost columns prefetched ahead (registers)
constexpr int DTW_MAX_SLOTS = 16;    // rows per pair <= 256 * 16 = 4096 (20 s at 5 ms)

// per pair: N, M, offset of the cost matrix (floats), of the decision words (uint32), of the path arrays (int32)
template <int SLOTS>
__global__ __launch_bounds__(EV_THREADS) void dtw_kernel(const int64_t* __restrict__ tab, const float* __restrict__ cost,
                                                        uint32_t* __restrict__ dec, int32_t* __restrict__ path_i, int32_t* __restrict__ path_j,
                                                        int32_t* __restrict__ path_len, double* __restrict__ total) {
  extern __shared__ __attribute__((aligned(16))) double dbuf[];      // [2][256 * SLOTS]: the previous diagonal by row
  __shared__ int s_len;
  constexpr int ROWS = EV_THREADS * SLOTS;
  const int pair = blockIdx.x;
  const int64_t* tp = tab + (int64_t)pair * 5;
  const int N = (int)tp[0], M = (int)tp[1];
  if (N <= 0 || M <= 0 || N > ROWS) {      // (N > ROWS: refused by the launcher; nothing is touched)
    if (threadIdx.x == 0) path_len[pair] = 0;
    return;
  }
  const float* cp = cost + tp[2];
  uint32_t* dp = dec + tp[3];
  int32_t* pi = path_i + tp[4];
  int32_t* pj = path_j + tp[4];
  const int W = (M + 15) >> 4;      // decision words per row
  const int tid = threadIdx.x;
  const double INF = INFINITY;

  double D[SLOTS], upd[SLOTS];      // D[i][j - 1] of the last diagonal; last diagonal's D[i - 1][.] read = this one's D[i - 1][j - 1]
  uint32_t word[SLOTS];
  float pf[DTW_PF][SLOTS];
#pragma unroll
  for (int m = 0; m < SLOTS; ++m) {
    D[m] = INF;
    upd[m] = INF;
    word[m] = 0u;
  }
#pragma unroll
  for (int p = 0; p < DTW_PF; ++p)
#pragma unroll
    for (int m = 0; m < SLOTS; ++m) {
      const int i = tid + EV_THREADS * m, j = p - i;
      pf[p][m] = (i < N && j >= 0 && j < M) ? cp[(int64_t)i * M + j] : 0.f;
    }

  const int n_diag = N + M - 1;
  for (int d0 = 0; d0 < n_diag; d0 += DTW_PF) {
#pragma unroll
    for (int p = 0; p < DTW_PF; ++p) {
      const int d = d0 + p;
      if (d >= n_diag) break;                                   // uniform
      const double* prev = dbuf + ((d - 1) & 1) * ROWS;
      double* cur = dbuf + (d & 1) * ROWS;
#pragma unroll
      for (int m = 0; m < SLOTS; ++m) {
        const int r0 = EV_THREADS * m;
        if (r0 >= N) break;                                     // uniform: slots past the last row
        if (r0 > d + DTW_PF || r0 + EV_THREADS - 1 + M - 1 < d) continue;      // uniform: the band has not reached / has left the slot
        const int i = r0 + tid, j = d - i;
        const bool valid = i < N && j >= 0 && j < M;
        const double up = (valid && i > 0) ? prev[i - 1] : INF;                // D[i - 1][j], written on diagonal d - 1
        if (valid) {
          double best = (i > 0 && j > 0) ? upd[m] : INF;                        // D[i - 1][j - 1]
          uint32_t k = 0u;
          if (up < best) { best = up; k = 1u; }
          const double left = j > 0 ? D[m] : INF;                              // D[i][j - 1]
          if (left < best) { best = left; k = 2u; }
          if (i == 0 && j == 0) best = 0.0;
          const double v = __dadd_rn((double)pf[p][m], best);
          D[m] = v;
          cur[i] = v;
          word[m] |= k << (2 * (j & 15));
          if ((j & 15) == 15 || j == M - 1) {
            dp[(int64_t)i * W + (j >> 4)] = word[m];
            word[m] = 0u;
          }
        }
        upd[m] = up;
        const int jn = j + DTW_PF;                                            // refill this ring slot with diagonal d + DTW_PF
        pf[p][m] = (i < N && jn >= 0 && jn < M) ? cp[(int64_t)i * M + jn] : 0.f;
      }
      __syncthreads();
    }
  }

  // D[N - 1][M - 1] sits in the register of the last row's owner
  const int il = N - 1;
  if (tid == (il & (EV_THREADS - 1))) {
#pragma unroll
    for (int m = 0; m < SLOTS; ++m)
      if (m == il / EV_THREADS) total[pair] = D[m];
  }
  __threadfence_block();
  __syncthreads();      // every decision word is visible to the walker
  if (tid == 0) {
    int i = N - 1, j = M - 1, n = 0;
    int64_t wpos = -1;
    uint32_t w = 0u;
    while (true) {      // at most N + M - 1 steps: every step lowers i + j
      pi[n] = i;
      pj[n] = j;
      ++n;
      if (i == 0 && j == 0) break;
      const int64_t q = (int64_t)i * W + (j >> 4);
      if (q != wpos) {
        w = dp[q];
        wpos = q;
      }
      const uint32_t k = (w >> (2 * (j & 15))) & 3u;
      if (k == 0u) { --i; --j; }
      else if (k == 1u) --i;
      else --j;
      if (i < 0 || j < 0) break;      // (unreachable: column 0 only steps up, row 0 only left)
    }
    s_len = n;
    path_len[pair] = n;
  }
  __syncthreads();
  const int L = s_len;
  for (int k = tid; k < L / 2; k += EV_THREADS) {      // reverse in place: thread k owns the pair (k, L - 1 - k)
    const int a0 = pi[k], a1 = pi[L - 1 - k], b0 = pj[k], b1 = pj[L - 1 - k];
    pi[k] = a1;
    pi[L - 1 - k] = a0;
    pj[k] = b1;
    pj[L - 1 - k] = b0;
  }
}

// per pair: first row of a / x, first row of b / y, offset of the path arrays
__global__ __launch_bounds__(EV_THREADS) void dtw_path_stats_kernel(const int64_t* __restrict__ tab, const int32_t* __restrict__ path_i,
                                                                   const int32_t* __restrict__ path_j, const int32_t* __restrict__ path_len,
                                                                   const float* __restrict__ a, int lda, const float* __restrict__ bm, int ldb,
                                                                   int dim, const float* __restrict__ x, const float* __restrict__ y,
                                                                   double* __restrict__ out) {
  __shared__ double red[EV_THREADS];
  const int pair = blockIdx.x;
  const int64_t* tp = tab + (int64_t)pair * 3;
  const int L = path_len[pair];
  const int32_t* pi = path_i + tp[2];
  const int32_t* pj = path_j + tp[2];
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // sqrt term, x, y, x^2, y^2, x y, (x - y)^2
  for (int k = threadIdx.x; k < L; k += EV_THREADS) {
    const int64_t ra = tp[0] + pi[k], rb = tp[1] + pj[k];
    if (a) {
      const float* ar = a + ra * lda;
      const float* br = bm + rb * ldb;
      double s = 0.0;
      for (int c = 0; c < dim; ++c) {
        const double df = (double)ar[c] - (double)br[c];      // exact
        s = __dadd_rn(s, __dmul_rn(df, df));
      }
      acc[0] = __dadd_rn(acc[0], sqrt(__dmul_rn(2.0, s)));
    }
    if (x) {
      const double xv = (double)x[ra], yv = (double)y[rb], df = xv - yv;
      acc[1] = __dadd_rn(acc[1], xv);
      acc[2] = __dadd_rn(acc[2], yv);
      acc[3] = __dadd_rn(acc[3], __dmul_rn(xv, xv));
      acc[4] = __dadd_rn(acc[4], __dmul_rn(yv, yv));
      acc[5] = __dadd_rn(acc[5], __dmul_rn(xv, yv));
      acc[6] = __dadd_rn(acc[6], __dmul_rn(df, df));
    }
  }
  double* o = out + (int64_t)pair * 8;
#pragma unroll
  for (int q = 0; q < 7; ++q) {
    const double v = block_tree_sum(acc[q], red);
    if (threadIdx.x == 0) o[1 + q] = v;
  }
  if (threadIdx.x == 0) o[0] = (double)L;
}

template <int SLOTS>
int launch_dtw(int n_pairs, const int64_t* tab, const float* cost, uint32_t* dec, int32_t* path_i, int32_t* path_j, int32_t* path_len,
               double* total, hipStream_t s) {
  const size_t lds = (size_t)2 * EV_THREADS * SLOTS * sizeof(double);
  JATTS_RAISE_LDS_LIMIT(dtw_kernel<SLOTS>);
  hipLaunchKernelGGL(dtw_kernel<SLOTS>, dim3((unsigned)n_pairs), dim3(EV_THREADS), lds, s, tab, cost, dec, path_i, path_j, path_len, total);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int32_t jatts_dtw_max_rows(void) { return EV_THREADS * DTW_MAX_SLOTS; }

extern "C" int jatts_frame_select(const jatts_ragged* rg_frames, const float* val, int32_t mode, double factor, int32_t* count, int32_t* idx,
                                  void* stream) {
  if (!rg_frames || !rg_frames->cu_rows || !val || !count) return jatts_set_error_msg(JATTS_ERR_ARG, "frame_select: null pointer");
  if (mode < 0 || mode > 2) return jatts_set_error_msg(JATTS_ERR_ARG, "frame_select: mode must be 0 (mean), 1 (positive) or 2 (maximum)");
  if (mode != 2 && !idx) return jatts_set_error_msg(JATTS_ERR_ARG, "frame_select: modes 0 and 1 write the index list");
  if (mode != 1 && !(factor >= 0.0)) return jatts_set_error_msg(JATTS_ERR_ARG, "frame_select: factor must be >= 0");
  if (rg_frames->n_seq <= 0) return JATTS_OK;
  jatts_ragged rg = *rg_frames;
  rg.host_lens = nullptr;
  hipLaunchKernelGGL(frame_select_kernel, dim3((unsigned)rg.n_seq), dim3(EV_THREADS), 0, S_, rg, val, mode, factor, count, idx);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_gather_rows(const jatts_ragged* rg_out, const int32_t* cu_src, const int32_t* idx, const float* src, int32_t ld_src,
                                 int32_t dim, float* dst, int32_t ld_dst, void* stream) {
  if (!rg_out || !rg_out->cu_rows || !cu_src || !idx || !src || !dst) return jatts_set_error_msg(JATTS_ERR_ARG, "gather_rows: null pointer");
  if (dim < 1 || ld_src < dim || ld_dst < dim) return jatts_set_error_msg(JATTS_ERR_ARG, "gather_rows: 1 <= dim <= ld_src, ld_dst expected");
  if (rg_out->n_seq <= 0 || rg_out->max_len <= 0) return JATTS_OK;
  if (rg_out->n_seq > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "gather_rows: more than 65535 utterances (split the batch)");
  jatts_ragged rg = *rg_out;
  rg.host_lens = nullptr;
  const int per = EV_THREADS / 64;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((rg.max_len + per - 1) / per), (unsigned)rg.n_seq), dim3(EV_THREADS), 0, S_, rg, cu_src,
                     idx, src, ld_src, dim, dst, ld_dst);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_pairwise_dist(int32_t n_pairs, const int64_t* tab, int32_t max_n, int32_t max_m, const float* a, int32_t lda,
                                   const float* b, int32_t ldb, int32_t dim, float* c, void* stream) {
  if (!tab || !a || !b || !c) return jatts_set_error_msg(JATTS_ERR_ARG, "pairwise_dist: null pointer");
  if (dim < 1 || dim > PD_DMAX || lda < dim || ldb < dim) return jatts_set_error_msg(JATTS_ERR_ARG, "pairwise_dist: 1 <= dim <= 64 and dim <= lda, ldb expected");
  if (n_pairs <= 0 || max_n <= 0 || max_m <= 0) return JATTS_OK;
  if (n_pairs > 65535 || (max_n + PD_T - 1) / PD_T > 65535) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "pairwise_dist: more than 65535 pairs or row tiles (split the batch)");
  hipLaunchKernelGGL(pairwise_dist_kernel, dim3((unsigned)((max_m + PD_T - 1) / PD_T), (unsigned)((max_n + PD_T - 1) / PD_T), (unsigned)n_pairs),
                     dim3(EV_THREADS), 0, S_, tab, a, lda, b, ldb, dim, c);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

extern "C" int jatts_dtw(int32_t n_pairs, const int64_t* tab, int32_t max_n, const float* cost, uint32_t* decisions, int32_t* path_i,
                         int32_t* path_j, int32_t* path_len, double* total, void* stream) {
  if (!tab || !cost || !decisions || !path_i || !path_j || !path_len || !total) return jatts_set_error_msg(JATTS_ERR_ARG, "dtw: null pointer");
  if (max_n > EV_THREADS * DTW_MAX_SLOTS) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "dtw: more than 4096 rows in a pair");
  if (n_pairs <= 0) return JATTS_OK;
  if (max_n <= EV_THREADS) return launch_dtw<1>(n_pairs, tab, cost, decisions, path_i, path_j, path_len, total, S_);
  if (max_n <= 2 * EV_THREADS) return launch_dtw<2>(n_pairs, tab, cost, decisions, path_i, path_j, path_len, total, S_);
  if (max_n <= 4 * EV_THREADS) return launch_dtw<4>(n_pairs, tab, cost, decisions, path_i, path_j, path_len, total, S_);
  if (max_n <= 8 * EV_THREADS) return launch_dtw<8>(n_pairs, tab, cost, decisions, path_i, path_j, path_len, total, S_);
  return launch_dtw<16>(n_pairs, tab, cost, decisions, path_i, path_j, path_len, total, S_);
}

extern "C" int jatts_dtw_path_stats(int32_t n_pairs, const int64_t* tab, const int32_t* path_i, const int32_t* path_j, const int32_t* path_len,
                                    const float* a, int32_t lda, const float* b, int32_t ldb, int32_t dim, const float* x, const float* y,
                                    double* out, void* stream) {
  if (!tab || !path_i || !path_j || !path_len || !out) return jatts_set_error_msg(JATTS_ERR_ARG, "dtw_path_stats: null pointer");
  if ((a == nullptr) != (b == nullptr) || (x == nullptr) != (y == nullptr) || (!a && !x))
    return jatts_set_error_msg(JATTS_ERR_ARG, "dtw_path_stats: two matrices, two tracks or both expected");
  if (a && (dim < 1 || lda < dim || ldb < dim)) return jatts_set_error_msg(JATTS_ERR_ARG, "dtw_path_stats: 1 <= dim <= lda, ldb expected");
  if (n_pairs <= 0) return JATTS_OK;
  hipLaunchKernelGGL(dtw_path_stats_kernel, dim3((unsigned)n_pairs), dim3(EV_THREADS), 0, S_, tab, path_i, path_j, path_len, a, lda, b, ldb, dim, x, y,
                     out);
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
