// Fused HiFi-GAN SINGLE-CONV dilation unit  y = x + conv_d(lrelu(x)) + b1  on f32-EQUIVALENT EMULATED operands (JATTS_F32E / JATTS_F32E6: three exact bf16
// terms per value, seven / six partial products per product) issued as v_mfma_f32_16x16x32_bf16 -- the windowed unit of resunit_emul16_impl.h without its
// second conv.  Same LDS image of the x tile ([row][8-channel unit][b0 | b1 | b2]), same weights (w_layout = 1), same K-step (conv16 / step16), same store
// pass.  The seven-product form keeps the two accumulators per fragment (leading product | the six small ones), joined by one correctly rounded add.
//
// Without the second conv there is no h tile, no discarded column and no halo to carry: a window of WGCOLS columns stores all of them (windowed form only),
// and its x tile is WGCOLS + (k - 1) dil rows (row r <-> position t0 - p1 + r).  The f32 y tile overlays the dead x tile at its own pitch (C * 4 + 16).
#pragma once
#include "resunit_emul16_impl.h"

namespace {

// KSPLIT: the x tile one channel half at a time (the second half's loads in flight under the first half's MFMAs); RREG: the raw x of the stored columns
// stays in registers from the staging to the store pass (x fetched from HBM once)
template <typename T, int C, int WGCOLS, int WN, int WT, int OCC, bool KSPLIT = false, bool RREG = false>      // T = bf3 (seven partial products) or bf3f (six)
__global__ __launch_bounds__(WN* WT * 64, OCC) void resunit1_emul16_kernel(jatts_resunit_desc d, unsigned bias_off) {
  typedef typename Elem<T>::vec8 V8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NF = C / (WN * 16), NT = WGCOLS / (WT * 16);
  constexpr int KC32 = C / 32, NFR16 = C / 16;
  constexpr int pitch = C * 6 + 16;
  constexpr int pitch_x = KSPLIT ? (C / 2) * 6 + 16 : pitch;
  constexpr int pitch_y = C * 4 + 16;
  constexpr int NTHR = WN * WT * 64;
  static_assert(NF * WN * 16 == C && NT * WT * 16 == WGCOLS && C % 32 == 0, "tile shape");
  static_assert(sizeof(T) == 6, "bf3 is three packed bf16");
  static_assert(!(KSPLIT && RREG), "the residual registers go with the one-piece x tile");
  static_assert(!KSPLIT || KC32 % 2 == 0, "channel halves are whole K-steps");
  constexpr int MAXI = RREG ? (WGCOLS * (C / 8) + NTHR - 1) / NTHR : 1;      // interior units per thread
  f32x8 xk[MAXI];
  const int K = d.k_w, dil = d.dil;
  const int p1 = (K - 1) / 2 * dil;

  // unit_window_of (unit_frame.h), kept as this kernel's own copy: timed slower than the parent at some shapes with the helper (profiles/r14_notes.md)
  int b = blockIdx.y, bx = blockIdx.x;
  if (ragged_is_1d(d.rg) && !ragged_locate(d.rg, WGCOLS, blockIdx.x, b, bx)) return;   // 1-D grid over the real tiles of a ragged batch
  const int row_b = d.rg.cu_rows[b];
  const int L = (d.rg.cu_rows[b + 1] - row_b) * d.rg.len_mul;
  const int t0 = bx * WGCOLS;
  if (t0 >= L) return;
  const int64_t seq_row0 = (int64_t)row_b * d.rg.len_mul;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wn = wave / WT, wt = wave % WT;
  const int g4 = lane >> 4;                 // which 4 of a fragment's 16 channels this lane owns in C / D
  const int col0 = wt * NT * 16;
  const int nf0 = wn * NF;
  const int tid = threadIdx.x;

  const int rx = WGCOLS + 2 * p1;   // x tile rows: row r <-> position t0 - p1 + r
  char* xs = smem;                  // bf3 lrelu(x) tile; finally the f32 y tile
  float* bs = reinterpret_cast<float*>(smem + bias_off);   // b1
  for (int u = tid; u < C; u += NTHR) bs[u] = d.b1[u];
  const int nvalid = min(WGCOLS, L - t0);

  WStream16<T, NF> ws;
  typename Acc16<T>::type acc[NF][NT];
  auto bias_acc = [&](const float* bv) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bv + (nf0 + f) * 16 + 4 * g4);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc16_set(acc[f][t], e, bb[e]);
    }
  };
  auto to_planes = [&](f32x8 v) {
    lrelu8(v, d.slope);
    V8 o;
    bf3_split8(v, o);
    return o;
  };
  const float* x = (const float*)d.x;

  ws.bind((const T*)d.w1, KC32, NFR16, nf0, lane);
  ws.fetch(0, 0);                  // the first K-step, under the staging
  const int pos0 = t0 - p1;
  if constexpr (!KSPLIT) {
    constexpr int UPR = C / 8;
    constexpr int UB = 8;
    const int total = rx * UPR;
    if constexpr (RREG) {
      const int r_in = p1, n_in = WGCOLS * UPR;   // x rows of the stored outputs [t0, t0 + WGCOLS)
#pragma unroll
      for (int j = 0; j < MAXI; ++j) {
        const int v = tid + j * NTHR;
        const int ro = v / UPR, cu = v - ro * UPR;
        const int pos = t0 + ro;
        if (v < n_in && pos < L) xk[j] = Vec8IO<float>::ldg(x + (seq_row0 + pos) * (int64_t)C + cu * 8);
        else xk[j] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
      const int n_halo = (rx - WGCOLS) * UPR;
      for (int base = tid; base < n_halo; base += NTHR * UB) {
        f32x8 v[UB];
#pragma unroll
        for (int j = 0; j < UB; ++j) {
          const int u = base + j * NTHR;
          int r = u / UPR;
          const int cu = u - r * UPR;
          if (r >= r_in) r += WGCOLS;
          const int pos = pos0 + r;
          if (u < n_halo && pos >= 0 && pos < L) v[j] = Vec8IO<float>::ldg(x + (seq_row0 + pos) * (int64_t)C + cu * 8);
          else v[j] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < UB; ++j) {
          const int u = base + j * NTHR;
          if (u >= n_halo) continue;
          int r = u / UPR;
          const int cu = u - r * UPR;
          if (r >= r_in) r += WGCOLS;
          Vec8IO<T>::sts(xs + (size_t)r * pitch + (size_t)cu * 48, to_planes(v[j]));
        }
      }
#pragma unroll
      for (int j = 0; j < MAXI; ++j) {
        const int v = tid + j * NTHR;
        if (v >= n_in) continue;
        const int ro = v / UPR, cu = v - ro * UPR;
        Vec8IO<T>::sts(xs + (size_t)(r_in + ro) * pitch + (size_t)cu * 48, to_planes(xk[j]));
      }
    } else {
      // the WHOLE tile in one batch of loads (halos up to 32 rows a side; longer ones take a second pass): the accumulators are not live yet
      constexpr int UBX = ((WGCOLS + 64) * UPR + NTHR - 1) / NTHR;
      for (int base = tid; base < total; base += NTHR * UBX) {
        f32x8 v[UBX];
#pragma unroll
        for (int j = 0; j < UBX; ++j) {
          const int u = base + j * NTHR;
          const int r = u / UPR, cu = u - r * UPR;
          const int pos = pos0 + r;
          if (u < total && pos >= 0 && pos < L) v[j] = Vec8IO<float>::ldg(x + (seq_row0 + pos) * (int64_t)C + cu * 8);
          else v[j] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int j = 0; j < UBX; ++j) {
          const int u = base + j * NTHR;
          if (u >= total) continue;
          const int r = u / UPR, cu = u - r * UPR;
          Vec8IO<T>::sts(xs + (size_t)r * pitch + (size_t)cu * 48, to_planes(v[j]));
        }
      }
    }
    __syncthreads();
    bias_acc(bs);
    conv16<T, NF, NT, KC32>(acc, ws, 0, K, dil, xs, pitch, col0, lane, nullptr);
  } else {
    constexpr int UPR = C / 16;                                            // 8-element units per row of one channel half
    constexpr int MAXU = ((WGCOLS + 64) * UPR + NTHR - 1) / NTHR;         // halos up to 32 rows a side (the launcher refuses more)
    const int total = rx * UPR;
    f32x8 xv[MAXU];
    auto load_half = [&](int half) {
#pragma unroll
      for (int j = 0; j < MAXU; ++j) {
        const int u = tid + j * NTHR;
        const int r = u / UPR, cu = u - r * UPR;
        const int pos = pos0 + r;
        if (u < total && pos >= 0 && pos < L) xv[j] = Vec8IO<float>::ldg(x + (seq_row0 + pos) * (int64_t)C + half * (C / 2) + cu * 8);
        else xv[j] = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
    };
    auto store_half = [&]() {
#pragma unroll
      for (int j = 0; j < MAXU; ++j) {
        const int u = tid + j * NTHR;
        if (u < total) Vec8IO<T>::sts(xs + (size_t)(u / UPR) * pitch_x + (size_t)(u % UPR) * 48, to_planes(xv[j]));
      }
    };
    load_half(0);
    store_half();
    load_half(1);                 // in flight under the first half's MFMAs
    __syncthreads();
    bias_acc(bs);
    // first channel half: weight steps 0 .. KC32 / 2 - 1 of every tap; the stream continues with the second half's first step
    conv16<T, NF, NT, KC32 / 2>(acc, ws, 0, K, dil, xs, pitch_x, col0, lane, ws.wl + (size_t)(KC32 / 2) * ws.kc_stride);
    lds_barrier();                // every wave is done reading the first half
    store_half();
    lds_barrier();
    conv16<T, NF, NT, KC32 / 2>(acc, ws, KC32 / 2, K, dil, xs, pitch_x, col0, lane, nullptr);
  }
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc16_finish(acc[f][t]);

  // ---- epilogue: acc (+ b1, already in) assembled as an f32 tile in LDS over the dead x tile; the residual (and the MRF mean) are added in the
  // row-contiguous store pass
  __syncthreads();
  char* ys = smem;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = col0 + t * 16 + (lane & 15);
    if (col >= nvalid) continue;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int n0 = (nf0 + f) * 16 + 4 * g4;
      *reinterpret_cast<f32x4*>(ys + (size_t)col * pitch_y + (size_t)n0 * 4) = acc16_val(acc[f][t]);
    }
  }
  __syncthreads();
  {
    const int64_t g0 = (seq_row0 + t0) * (int64_t)C;
    if constexpr (RREG) {
      float* yg = (float*)d.y;
      constexpr int UPR = C / 8;
      const int n_out = nvalid * UPR;
      const bool has_add1 = d.add0 != nullptr && d.add1 != nullptr;
      f32x8 a0[MAXI], a1[MAXI];
      if (d.add0) {
#pragma unroll
        for (int j = 0; j < MAXI; ++j) {
          const int v = tid + j * NTHR;
          if (v < n_out) {
            a0[j] = Vec8IO<float>::ldg((const float*)d.add0 + g0 + (int64_t)v * 8);
            if (has_add1) a1[j] = Vec8IO<float>::ldg((const float*)d.add1 + g0 + (int64_t)v * 8);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < MAXI; ++j) {
        const int v = tid + j * NTHR;
        if (v >= n_out) continue;
        const int ro = v / UPR, cu = v - ro * UPR;
        f32x8 o = Vec8IO<float>::lds(ys + (size_t)ro * pitch_y + (size_t)cu * 32);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = o[e] + xk[j][e];          // residual
        if (d.add0) {
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = (o[e] + a0[j][e] + (has_add1 ? a1[j][e] : 0.f)) * d.out_scale;
        }
        float* dst = yg + g0 + (int64_t)v * 8;
        *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
      }
    } else {
      unit_store<float, C, NTHR>(d, ys, pitch_y, nvalid, g0);
    }
  }
}

// LDS bytes of the x / y region of a <C, WGCOLS> window at this halo (KSPLIT: x tile rows of one channel half)
template <int C, int WGCOLS, bool KSPLIT = false>
constexpr size_t resunit1_emul16_region(int halo) {
  const size_t px = (KSPLIT ? C / 2 : C) * 6 + 16, x = (size_t)(WGCOLS + halo) * px, y = (size_t)WGCOLS * (C * 4 + 16);
  return x > y ? x : y;
}

template <typename T, int C, int WGCOLS, int WN, int WT, int OCC = 2, bool KSPLIT = false, bool RREG = false>
int launch_resunit1_emul16(const jatts_resunit_desc& d, hipStream_t s) {
  const int halo = (d.k_w - 1) / 2 * d.dil * 2;
  if (KSPLIT && halo > 64) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "resunit (single conv, emulated, channel halves): halo beyond 32 rows a side");
  const size_t region = resunit1_emul16_region<C, WGCOLS, KSPLIT>(halo);
  const size_t lds = region + C * sizeof(float);            // + b1
  constexpr auto kern = resunit1_emul16_kernel<T, C, WGCOLS, WN, WT, OCC, KSPLIT, RREG>;
  return unit_launch<kern>(JATTS_SITE("resunit (single conv): tile exceeds 160 KiB LDS"), WN * WT * 64, lds, WGCOLS, d.rg, s, d, (unsigned)region);
}

}  // namespace
