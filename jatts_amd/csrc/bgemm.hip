// Batched f32 GEMM on the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32) for the TRAINING step's attention products (round 4):
//   C[b] (M x N) = alpha * op(A[b]) (M x K) * op(B[b]) (K x N)
// q k^T, q p^T, P v and their gradients (attention.py:164-206 under autograd) went to rocBLAS through torch.matmul -- the one library GEMM
// inside a SURVEY row counted as implemented (missing #5).  A two-level batch index (outer, inner) with independent strides per
// operand covers (B, H, ...) tensors with an operand shared over B (the position projection p_h: outer stride 0).
//
// One workgroup = 4 waves = a 128 x 128 (or 128 x 64) tile of C (each wave 64 x 64 = 2 x 2 fragments, or 64 x 32); K runs in chunks of 32
// through a double-buffered LDS pair As[k][m], Bs[k][n] (pitch 132: the transposing store of a K-contiguous operand hits 64 distinct
// banks); the loads of chunk i + 1 are issued before the MFMAs of chunk i.  A fragment operand is one ds_read_b32 per lane and K-pair.
#include "common.h"
#include "resunit_emul16_impl.h"   // acc2x4 / mma16p: the seven-product rule of the emulated convs, shared with bgemm_emul_kernel below

#ifndef JATTS_BGEMM_DIAG
#define JATTS_BGEMM_DIAG 0   // timing probes only (wrong results): 1 = no operand loads in the chunk loop, 2 = no LDS stores in it, 4 = no barriers in it
#endif

namespace {

// Tile rows BM = 64 MF (MF = 32-row fragments per wave along m: 2 -> 128 rows, 1 -> 64), LDS pitch of the A tile BP = BM + 4 floats; BN = 64 / 128 / 192 and
// the chunk depth BK are template parameters too

struct BgemmArgs {
  const float* a;
  const float* b;
  float* c;
  int64_t sa_o, sa_i, sb_o, sb_i, sc_o, sc_i;   // element strides of the (outer, inner) batch index
  int lda, ldb, ldc, ta, tb;
  int n_inner, M, N, K;
  float alpha;
  int accumulate;
  int n_batch, gx, gy;      // XCD-aware 1-D grid: workgroup id -> (matrix, tile), see bgemm_kernel
};

// One operand chunk (RW rows of the "long" dimension from r0, BK contraction steps from k0) -> registers, 16 bytes per load.  k_contig = the
// operand is stored with K contiguous (A untransposed / B transposed): a thread takes 4 consecutive k of one row per load; otherwise the
// long dimension is contiguous: 4 consecutive rows of one k.
// MAP: which 16-byte piece a thread takes in the VEC path.  0 = the exact kernel's (pieces dealt out in memory order).  1 = the emulated kernel's (BK = 32, see
// bgemm_emul_kernel): a K-contiguous operand deals the pieces out row by row with every second and third row of four swapped (the two rows of a 16-lane
// ds_write_b64 group then sit two apart: disjoint banks); a long-dimension-contiguous operand gives a thread the SAME four rows at two consecutive k per
// pair of loads (2 j, 2 j + 1), which the split turns into stored bf16 pairs.
template <int RW, int BK, int PITCH, bool KC, bool VEC, int MAP = 0>      // KC: K contiguous in memory; VEC: 16-byte loads allowed (compile time: a
struct Chunk {                                               // run-time flag made hipcc emit every combination inside one kernel, waits and all)
  static_assert(MAP == 0 || (BK == 32 && RW % 64 == 0), "the emulated kernel's piece map: 32-deep chunks of 64 n rows");
  static constexpr int NL = (RW * BK / 4 + 255) / 256;      // 16-byte loads per thread
  static constexpr int TOTAL = RW * BK / 4;
  f32x4 v[NL];
  // vec (the matrix starts on a 16-byte boundary and ld % 4 == 0: every attention operand): ALL loads are issued unconditionally from clamped
  // addresses and masked afterwards -- a load inside a per-element branch makes hipcc wait vmcnt(0) right behind it, i.e. one L2 round trip
  // per 16 bytes, eight times per chunk (the first version of this kernel spent 4/5 of its time there).  A 16-byte piece that straddles the
  // edge (k + 3 >= K or r + 3 >= R) stays inside its row because ld % 4 == 0.
  __device__ __forceinline__ void load(const float* base, int ld, int r0, int R, int k0, int K) {
    constexpr bool k_contig = KC;
    if constexpr (VEC) {
      int lim[NL], at[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int u = (int)threadIdx.x + 256 * j;
        int r, k;
        if constexpr (MAP == 1) {
          if (k_contig) { const int t = u >> 3; r = r0 + ((t & ~3) | ((t & 1) << 1) | ((t >> 1) & 1)); k = k0 + 4 * (u & 7); }
          else { const int w = (int)threadIdx.x + 256 * (j >> 1); k = k0 + 2 * (w & 15) + (j & 1); r = r0 + 4 * (w >> 4); }
        } else if (k_contig) { r = r0 + u / (BK / 4); k = k0 + 4 * (u % (BK / 4)); }
        else { k = k0 + u / (RW / 4); r = r0 + 4 * (u % (RW / 4)); }
        const bool in = (TOTAL % 256 == 0 || u < TOTAL) && r < R && k < K;
        const int rc = r < R ? r : R - 1, kc = k < K ? k : K - 1;
        // vector index along the contiguous dimension: clamp to the last full-or-partial piece of the row
        const int64_t off = k_contig ? (int64_t)rc * ld + (kc & ~3) : (int64_t)kc * ld + (rc & ~3);
        v[j] = *reinterpret_cast<const f32x4*>(base + off);
        at[j] = k_contig ? k : r;
        lim[j] = in ? (k_contig ? K : R) : -1;      // component e is valid iff at + e < lim
      }
#pragma unroll
      for (int j = 0; j < NL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] = at[j] + e < lim[j] ? v[j][e] : 0.f;
      return;
    }
    // element loads (a matrix that starts off a 16-byte boundary or ld % 4 != 0: a padded batch length T with T % 4 != 0 puts P v and its
    // gradients here): the same discipline -- every load unconditional from a clamped address, masks afterwards.  (The first version loaded
    // inside per-element branches: one exec-masked load and one L2 round trip per element.)
    // Element (j, e) of a thread is element tid + 256 (4 j + e) of the chunk counted along the CONTIGUOUS dimension first, so one wave
    // instruction reads 64 consecutive floats of a row (or 64 / BK rows of BK): the 4-consecutive-elements-per-lane map of the 16-byte
    // path would touch four times the cache lines per instruction here.
    bool ok[NL][4];
#pragma unroll
    for (int j = 0; j < NL; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = (int)threadIdx.x + 256 * (4 * j + e);
        const int re = r0 + (k_contig ? idx / BK : idx % RW), ke = k0 + (k_contig ? idx % BK : idx / RW);
        ok[j][e] = (RW * BK % 1024 == 0 || idx < RW * BK) && re < R && ke < K;
        const int rc = re < R ? re : R - 1, kc = ke < K ? ke : K - 1;
        v[j][e] = base[k_contig ? (int64_t)rc * ld + kc : (int64_t)kc * ld + rc];
      }
#pragma unroll
    for (int j = 0; j < NL; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[j][e] = ok[j][e] ? v[j][e] : 0.f;
  }
  __device__ __forceinline__ void store(float* s) const {
    constexpr bool k_contig = KC;
    if constexpr (!VEC) {      // (the element map of load(): consecutive lanes = consecutive k at pitch 132 = 64 distinct banks, or consecutive r)
#pragma unroll
      for (int j = 0; j < NL; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int idx = (int)threadIdx.x + 256 * (4 * j + e);
          if (RW * BK % 1024 != 0 && idx >= RW * BK) continue;
          const int r = k_contig ? idx / BK : idx % RW, k = k_contig ? idx % BK : idx / RW;
          s[k * PITCH + r] = v[j][e];
        }
      return;
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int u = (int)threadIdx.x + 256 * j;
      if (TOTAL % 256 != 0 && u >= TOTAL) continue;
      if (k_contig) {      // transpose on the way in: s[k][r]
        const int r = u / (BK / 4), k = 4 * (u % (BK / 4));
#pragma unroll
        for (int e = 0; e < 4; ++e) s[(k + e) * PITCH + r] = v[j][e];
      } else {
        const int k = u / (RW / 4), r = 4 * (u % (RW / 4));
        *reinterpret_cast<f32x4*>(s + k * PITCH + r) = v[j];
      }
    }
  }
};

// WNF = 32-column fragments per wave along n: 1 -> 128 x 64 tile, 2 -> 128 x 128, 3 -> 128 x 192 (n = d_k = 192 in ONE tile: the T x T operand of
// P v and of the key / value gradients is then read once instead of once per n tile).
// 1-D grid in XCD-aware order: workgroup id lands on XCD id % 8 (each with its own L2), so matrix b = 8 (m / tiles) + id % 8 with m = id / 8 --
// all tiles of a matrix run on ONE XCD, back to back, and its operands are fetched from HBM once instead of once per XCD that happens to
// hold one of its tiles (the first version, a 3-D grid, ran at 45-65 TFLOP/s against rocBLAS' 100-110).
// MF = 1: 64-row tiles for launches whose 128-row tiles would not fill the two-per-CU slots evenly (P v and the key / value gradients at T = 768: 384
// workgroups of 128 x 192 on 512 slots = half the CUs carrying two and half one; 768 of 64 x 192 = three each)
template <int WNF, int BK, bool AK, bool BKC, bool VEC, int MF = 2>      // AK / BKC: K contiguous in A (trans_a == 0) / in B (trans_b != 0)
__global__ __launch_bounds__(256, 2) void bgemm_kernel(BgemmArgs g) {
  constexpr int BN = 64 * WNF, BPN = BN + 4, BM = 64 * MF, BP = BM + 4;
  extern __shared__ __attribute__((aligned(16))) float sm_raw[];      // [buffer][A: BK x BP | B: BK x BPN]
  constexpr int BUF = BK * (BP + BPN);
  const int xcd = (int)(blockIdx.x & 7u), mloc = (int)(blockIdx.x >> 3);
  const int tiles = g.gx * g.gy;
  const int bz = 8 * (mloc / tiles) + xcd, tile = mloc % tiles;
  if (bz >= g.n_batch) return;
  const int bo = bz / g.n_inner, bi = bz - bo * g.n_inner;
  const float* A = g.a + bo * g.sa_o + bi * g.sa_i;
  const float* B = g.b + bo * g.sb_o + bi * g.sb_i;
  float* C = g.c + bo * g.sc_o + bi * g.sc_i;
  const int m0 = (tile / g.gx) * BM, n0 = (tile % g.gx) * BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32 * MF, wn = (wave & 1) * 32 * WNF;
  const int lo = lane & 31, hi = lane >> 5;

  f32x16 acc[MF][WNF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < WNF; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  Chunk<BM, BK, BP, AK, VEC> ra;
  Chunk<BN, BK, BPN, BKC, VEC> rb;
  ra.load(A, g.lda, m0, g.M, 0, g.K);
  rb.load(B, g.ldb, n0, g.N, 0, g.K);
  ra.store(sm_raw);
  rb.store(sm_raw + BK * BP);
  __syncthreads();
  const int n_chunks = (g.K + BK - 1) / BK;
  for (int ci = 0; ci < n_chunks; ++ci) {
    const bool more = ci + 1 < n_chunks;
    if (more && !(JATTS_BGEMM_DIAG & 1)) {
      ra.load(A, g.lda, m0, g.M, (ci + 1) * BK, g.K);
      rb.load(B, g.ldb, n0, g.N, (ci + 1) * BK, g.K);
    }
    const float* as = sm_raw + (ci & 1) * BUF + hi * BP + wm + lo;
    const float* bs = sm_raw + (ci & 1) * BUF + BK * BP + hi * BPN + wn + lo;
    // fragments of 8 K-pairs at a time into registers, THEN their MFMAs: a ds_read right in front of its MFMA exposes the LDS latency 16 times
    // per chunk (the first version ran at 55-63 TFLOP/s)
#pragma unroll
    for (int k8 = 0; k8 < BK / 2; k8 += 8) {
      float av[8][MF], bv[8][WNF];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int i = 0; i < MF; ++i) av[q][i] = as[2 * (k8 + q) * BP + 32 * i];
#pragma unroll
        for (int j = 0; j < WNF; ++j) bv[q][j] = bs[2 * (k8 + q) * BPN + 32 * j];
      }
      __builtin_amdgcn_sched_barrier(0);      // (hipcc otherwise sinks every read next to its MFMA behind an lgkmcnt(0))
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int j = 0; j < WNF; ++j) {
#pragma unroll
          for (int i = 0; i < MF; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[q][i], bv[q][j], acc[i][j], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more && !(JATTS_BGEMM_DIAG & 2)) {
      ra.store(sm_raw + ((ci + 1) & 1) * BUF);
      rb.store(sm_raw + ((ci + 1) & 1) * BUF + BK * BPN * 0 + BK * BP);
    }
    if (!(JATTS_BGEMM_DIAG & 4)) __syncthreads();
  }
  // C/D map: column (lane & 31) = n, row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) = m
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < WNF; ++j) {
      const int n = n0 + wn + 32 * j + lo;
      if (n >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * hi;
        if (m < g.M) {
          float* o = C + (int64_t)m * g.ldc + n;
          *o = g.accumulate ? *o + g.alpha * acc[i][j][r] : g.alpha * acc[i][j][r];
        }
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// The same batched GEMM on the f32-EQUIVALENT emulated arithmetic (JATTS_F32E, common.h): every f32 value of BOTH operands is split into its three exact
// bf16 terms between the global load and the LDS store (bf3_split2, no scales), seven of the nine partial products run on v_mfma_f32_16x16x32_bf16, the
// leading product into one f32 accumulator and the six small ones into a second (acc2x4 / mma16p, the rule of conv1d_emul16.h and of
// conv_wgrad_emul_kernel), joined by ONE add per output in the epilogue; alpha and accumulate are applied after that add.
//
// LDS image.  Three planes per operand, [plane][row][k] bf16 with K fastest, one 32-deep chunk (= one K-step) at a time: a 16 x 16 x 32 fragment operand
// is one ds_read_b128 per plane (lane l: row l & 15, K-group l >> 4).  The row pitch is COMPUTED (emul_pitch below): the smallest multiple of 16 bytes that
// holds a row and for which (a) every 16-lane group of that ds_read_b128 touches 16 distinct 16-byte segments, (b) the ds_write_b64 of a K-contiguous
// operand (Chunk MAP 1: 8 lanes per row, the group's two rows two apart) is conflict-free and (c) the ds_write_b32 of the TRANSPOSING store -- an operand
// whose long dimension is contiguous: a thread holds four rows at two consecutive k, the split's result is already the stored pair -- is at most 2-way,
// which a ds_write_b32 absorbs (its 4 issue cycles cover 2 x 2 LDS-array cycles).  That is 96 bytes = 32 x 3: (a) forces 32 x odd, and with any such pitch
// rows four apart alias, so a 32-lane store group that spans two row quads cannot do better than 2-way -- the map keeps it there instead of the 16-way of
// lanes-along-rows.  The element path (operands off the 16-byte grid) splits value by value and stores 2 bytes at a time: correct, and slow (its masks and
// addresses do not fit 256 registers next to the accumulators, so it runs one workgroup per CU rather than spill).
//
// Tiles and occupancy.  Four waves, 2 x 2; a wave owns (32 MF) x (32 WNF) outputs = 2 MF x 2 WNF fragments x 4 registers x 2 accumulators: 128 registers at
// 128 x 128.  The three planes of a 128 x 128 x 32 chunk at pitch 96 are 72 KB; double-buffered that is 144 KB = ONE workgroup of four waves per CU, with
// nobody to cover its barriers.  Chosen instead: ONE LDS buffer and the next chunk prefetched into registers (Chunk, 32 more registers; the exact kernel's
// scheme), which keeps 128 + 32 + 48 (A fragments) + 12 (one B fragment) + addressing under the 256 registers of two waves per SIMD, and 2 x 72 KB under the
// CU's 160 KB: two workgroups per CU, one computing while the other stages.  The 128 x 192 tile (192 accumulator registers, 90 KB) runs one per CU; the
// 64 x 192 one is back at two.
// K order per output: chunk by chunk, one K-step per chunk, the seven products smallest first -- the same instruction sequence per accumulator in every tile
// variant and load path, so an output's bits do not depend on which variant computed it.  No split-K, no atomics.
constexpr int EK = 32;      // chunk depth = one K-step of v_mfma_f32_16x16x32_bf16

// most distinct addresses on one bank inside one lane group: lanes[i] -> first dword addr[i], `nd` dwords each, `banks` banks
constexpr int emul_ways(const int* addr, int n, int nd, int banks) {
  int worst = 0;
  for (int b = 0; b < banks; ++b) {
    int c = 0;
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < nd; ++d) c += (addr[i] + d) % banks == b;
    worst = c > worst ? c : worst;
  }
  return worst;
}
constexpr bool emul_pitch_ok(int pitch) {
  if (pitch % 16 != 0 || pitch < EK * 2) return false;
  // (a) ds_read_b128: four groups of 16 lanes, 64 banks
  constexpr int grp[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                              {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  for (int q = 0; q < 4; ++q) {
    int a[16] = {};
    for (int i = 0; i < 16; ++i) a[i] = ((grp[q][i] & 15) * pitch + (grp[q][i] >> 4) * 16) / 4;
    if (emul_ways(a, 16, 4, 64) > 1) return false;
  }
  // (b) ds_write_b64 of a K-contiguous operand: 16 consecutive pieces u, 32 banks (Chunk MAP 1: row = u >> 3 with bits 0 and 1 swapped, k = 4 (u & 7))
  for (int u0 = 0; u0 < 64; u0 += 16) {
    int a[16] = {};
    for (int i = 0; i < 16; ++i) {
      const int t = (u0 + i) >> 3, row = (t & ~3) | ((t & 1) << 1) | ((t >> 1) & 1);
      a[i] = (row * pitch + 8 * ((u0 + i) & 7)) / 4;
    }
    if (emul_ways(a, 16, 2, 32) > 1) return false;
  }
  // (c) ds_write_b32 of the transposing store: 32 consecutive pair units w (k pair w & 15, row quad w >> 4), row e of the quad; 2-way is free
  for (int e = 0; e < 4; ++e) {
    int a[32] = {};
    for (int i = 0; i < 32; ++i) a[i] = ((4 * (i >> 4) + e) * pitch + 4 * (i & 15)) / 4;
    if (emul_ways(a, 32, 1, 32) > 2) return false;
  }
  return true;
}
constexpr int emul_pitch() {
  for (int p = EK * 2; p < 4 * EK * 2; p += 16)
    if (emul_pitch_ok(p)) return p;
  return 0;
}
constexpr int EP = emul_pitch();      // bytes per LDS row
static_assert(EP == 96, "row pitch of the emulated tiles: 32 x 3 bytes");

// One operand chunk, registers -> the three LDS planes (plane stride `pl` bytes), split on the way.  The maps are Chunk::load's (MAP 1).
template <int RW, bool KC, bool VEC>
__device__ __forceinline__ void emul_commit(const Chunk<RW, EK, 0, KC, VEC, 1>& c, char* s, int pl) {
  typedef Chunk<RW, EK, 0, KC, VEC, 1> CH;
  if constexpr (!VEC) {
#pragma unroll
    for (int j = 0; j < CH::NL; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int idx = (int)threadIdx.x + 256 * (4 * j + e);
        if (RW * EK % 1024 != 0 && idx >= RW * EK) continue;
        const int r = KC ? idx / EK : idx % RW, k = KC ? idx % EK : idx / RW;
        bf16 b0, b1, b2;
        bf3_split(c.v[j][e], b0, b1, b2);
        char* p = s + r * EP + k * 2;
        *reinterpret_cast<bf16*>(p) = b0;
        *reinterpret_cast<bf16*>(p + pl) = b1;
        *reinterpret_cast<bf16*>(p + 2 * pl) = b2;
      }
  } else if constexpr (KC) {      // four consecutive k of one row: one ds_write_b64 per plane
#pragma unroll
    for (int j = 0; j < CH::NL; ++j) {
      const int u = (int)threadIdx.x + 256 * j, t = u >> 3;
      const int r = (t & ~3) | ((t & 1) << 1) | ((t >> 1) & 1);
      bf16x2 a0, a1, a2, b0, b1, b2;
      bf3_split2(c.v[j][0], c.v[j][1], a0, a1, a2);
      bf3_split2(c.v[j][2], c.v[j][3], b0, b1, b2);
      char* p = s + r * EP + 8 * (u & 7);
      *reinterpret_cast<uint2*>(p) = make_uint2(__builtin_bit_cast(unsigned, a0), __builtin_bit_cast(unsigned, b0));
      *reinterpret_cast<uint2*>(p + pl) = make_uint2(__builtin_bit_cast(unsigned, a1), __builtin_bit_cast(unsigned, b1));
      *reinterpret_cast<uint2*>(p + 2 * pl) = make_uint2(__builtin_bit_cast(unsigned, a2), __builtin_bit_cast(unsigned, b2));
    }
  } else {                        // the transposing store: four rows at k, k + 1 -> one ds_write_b32 per row and plane
    static_assert(CH::NL % 2 == 0, "pairs of loads");
#pragma unroll
    for (int jj = 0; jj < CH::NL / 2; ++jj) {
      const int w = (int)threadIdx.x + 256 * jj;
      char* p = s + 4 * (w >> 4) * EP + 4 * (w & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        bf16x2 p0, p1, p2;
        bf3_split2(c.v[2 * jj][e], c.v[2 * jj + 1][e], p0, p1, p2);
        *reinterpret_cast<unsigned*>(p + e * EP) = __builtin_bit_cast(unsigned, p0);
        *reinterpret_cast<unsigned*>(p + e * EP + pl) = __builtin_bit_cast(unsigned, p1);
        *reinterpret_cast<unsigned*>(p + e * EP + 2 * pl) = __builtin_bit_cast(unsigned, p2);
      }
    }
  }
}

template <int WNF, bool AK, bool BKC, bool VEC, int MF>
__global__ __launch_bounds__(256, VEC && MF * WNF <= 4 ? 2 : 1) void bgemm_emul_kernel(BgemmArgs g) {
  constexpr int BM = 64 * MF, BN = 64 * WNF, FA = 2 * MF, FB = 2 * WNF;      // FA x FB fragments of 16 x 16 per wave
  constexpr int APL = BM * EP, BPL = BN * EP;                                // plane strides
  extern __shared__ __attribute__((aligned(16))) char esm[];                // [A: 3 planes | B: 3 planes]
  char* const asb = esm;
  char* const bsb = esm + 3 * APL;
  const int xcd = (int)(blockIdx.x & 7u), mloc = (int)(blockIdx.x >> 3);    // XCD-aware 1-D grid: see bgemm_kernel
  const int tiles = g.gx * g.gy;
  const int bz = 8 * (mloc / tiles) + xcd, tile = mloc % tiles;
  if (bz >= g.n_batch) return;
  const int bo = bz / g.n_inner, bi = bz - bo * g.n_inner;
  const float* A = g.a + bo * g.sa_o + bi * g.sa_i;
  const float* B = g.b + bo * g.sb_o + bi * g.sb_i;
  float* C = g.c + bo * g.sc_o + bi * g.sc_i;
  const int m0 = (tile / g.gx) * BM, n0 = (tile % g.gx) * BN;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32 * MF, wn = (wave & 1) * 32 * WNF;

  acc2x4 acc[FA][FB];
#pragma unroll
  for (int i = 0; i < FA; ++i)
#pragma unroll
    for (int j = 0; j < FB; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc16_set(acc[i][j], r, 0.f);

  Chunk<BM, EK, 0, AK, VEC, 1> ra;
  Chunk<BN, EK, 0, BKC, VEC, 1> rb;
  ra.load(A, g.lda, m0, g.M, 0, g.K);      // (the K edge arrives as zeros: the split of 0 is three zeros)
  rb.load(B, g.ldb, n0, g.N, 0, g.K);
  // fragment addresses: lane supplies row / column (lane & 15) and k = 8 (lane >> 4) .. + 7 of the K-step
  const char* ap = asb + (wm + (lane & 15)) * EP + (lane >> 4) * 16;
  const char* bp = bsb + (wn + (lane & 15)) * EP + (lane >> 4) * 16;
  const int n_chunks = (g.K + EK - 1) / EK;
  for (int ci = 0; ci < n_chunks; ++ci) {
    if (!(JATTS_BGEMM_DIAG & 2) || ci == 0) {
      emul_commit(ra, asb, APL);
      emul_commit(rb, bsb, BPL);
    }
    if (!(JATTS_BGEMM_DIAG & 4) || ci == 0) __syncthreads();
    if (ci + 1 < n_chunks && !(JATTS_BGEMM_DIAG & 1)) {      // the next chunk's loads fly under this chunk's MFMAs
      ra.load(A, g.lda, m0, g.M, (ci + 1) * EK, g.K);
      rb.load(B, g.ldb, n0, g.N, (ci + 1) * EK, g.K);
    }
    bf3px8<7> a[FA];
#pragma unroll
    for (int f = 0; f < FA; ++f) {
      const char* p = ap + f * 16 * EP;
      a[f].b0 = *reinterpret_cast<const bf16x8*>(p);
      a[f].b1 = *reinterpret_cast<const bf16x8*>(p + APL);
      a[f].b2 = *reinterpret_cast<const bf16x8*>(p + 2 * APL);
    }
#pragma unroll
    for (int j = 0; j < FB; ++j) {
      bf3px8<7> b;
      const char* p = bp + j * 16 * EP;
      b.b0 = *reinterpret_cast<const bf16x8*>(p);
      b.b1 = *reinterpret_cast<const bf16x8*>(p + BPL);
      b.b2 = *reinterpret_cast<const bf16x8*>(p + 2 * BPL);
      // product by product over the column's fragments: consecutive MFMAs never share an accumulator
#define JATTS_BE_P(P_)                \
  _Pragma("unroll") for (int i = 0; i < FA; ++i) mma16p<P_>(a[i], b, acc[i][j]);
      JATTS_BE_P(0) JATTS_BE_P(1) JATTS_BE_P(2) JATTS_BE_P(3) JATTS_BE_P(4) JATTS_BE_P(5) JATTS_BE_P(6)
#undef JATTS_BE_P
    }
    if (!(JATTS_BGEMM_DIAG & 4)) __syncthreads();
  }
  // C / D map of the 16 x 16 fragment: column (lane & 15) = n, rows 4 (lane >> 4) + reg = m.  M and N edges are masked here.
#pragma unroll
  for (int i = 0; i < FA; ++i)
#pragma unroll
    for (int j = 0; j < FB; ++j) {
      acc16_finish(acc[i][j]);      // the ONE add that joins the leading product's accumulator and the small products'
      const f32x4 v = acc16_val(acc[i][j]);
      const int n = n0 + wn + 16 * j + (lane & 15);
      if (n >= g.N) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * (lane >> 4) + r;
        if (m < g.M) {
          float* o = C + (int64_t)m * g.ldc + n;
          *o = g.accumulate ? *o + g.alpha * v[r] : g.alpha * v[r];
        }
      }
    }
}

}  // namespace

extern "C" int jatts_bgemm(const float* a, int64_t sa_outer, int64_t sa_inner, int32_t lda, int32_t trans_a, const float* b, int64_t sb_outer,
                           int64_t sb_inner, int32_t ldb, int32_t trans_b, float* c, int64_t sc_outer, int64_t sc_inner, int32_t ldc,
                           int32_t n_outer, int32_t n_inner, int32_t m, int32_t n, int32_t k, float alpha, int32_t accumulate, void* stream) {
  if (!a || !b || !c) return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm: null pointer");
  if (n_outer < 1 || n_inner < 1 || m < 1 || n < 1 || k < 1 || lda < 1 || ldb < 1 || ldc < 1)
    return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm: bad geometry");
  BgemmArgs g{a, b, c, sa_outer, sa_inner, sb_outer, sb_inner, sc_outer, sc_inner, lda, ldb, ldc, trans_a, trans_b, n_inner, m, n, k, alpha, accumulate, 0, 0, 0};
  // n tile: 192 in one piece (n = d_k = 192), else 64-wide where a 128-wide tile would be more than a quarter empty
  const int n_batch = n_outer * n_inner;
  auto launch = [&](auto kern, int bn, int bk, int bm) -> int {
    const int lds = 2 * bk * (bm + 4 + bn + 4) * (int)sizeof(float);
    g.n_batch = n_batch;
    g.gx = (n + bn - 1) / bn;
    g.gy = (m + bm - 1) / bm;
    const int64_t total = (int64_t)8 * ((n_batch + 7) / 8) * g.gx * g.gy;
    if (total >= (int64_t)1 << 31) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "bgemm: launch too large");
    hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), lds, (hipStream_t)stream, g);
    return JATTS_OK;
  };
  const int n128 = (n + 127) / 128 * 128, n64 = (n + 63) / 64 * 64;
  // 16-byte loads when EVERY matrix of both operands starts on a 16-byte boundary with a leading dimension of 4 k elements
  const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 &&
                   ((sa_outer | sa_inner | sb_outer | sb_inner | (int64_t)lda | (int64_t)ldb) & 3) == 0;
  const int tile = (n > 128 && n <= 192) ? 3 : (n64 * 4 <= n128 * 3 ? 1 : 2);
  int rc = JATTS_ERR_UNSUPPORTED;
  // (the dynamic-LDS limit is raised here, not in the lambda: a static there would be one for every kernel of this signature)
#define JATTS_BGEMM_CASE(WNF, BKC_, AKv, BKv, VECv, MFv)                                 \
  do {                                                                                   \
    JATTS_RAISE_LDS_LIMIT((bgemm_kernel<WNF, BKC_, AKv, BKv, VECv, MFv>));               \
    rc = launch(bgemm_kernel<WNF, BKC_, AKv, BKv, VECv, MFv>, 64 * WNF, BKC_, 64 * MFv); \
  } while (0)
#define JATTS_BGEMM_ORIENT(WNF, BKC_, VECv, MFv)                                         \
  do {                                                                                   \
    if (!trans_a && trans_b) JATTS_BGEMM_CASE(WNF, BKC_, true, true, VECv, MFv);         \
    else if (!trans_a && !trans_b) JATTS_BGEMM_CASE(WNF, BKC_, true, false, VECv, MFv);  \
    else if (trans_a && !trans_b) JATTS_BGEMM_CASE(WNF, BKC_, false, false, VECv, MFv);  \
    else JATTS_BGEMM_CASE(WNF, BKC_, false, true, VECv, MFv);                            \
  } while (0)
  // 64-row tiles when the 128-row tiling leaves fewer than two rounds of the 512 two-per-CU slots (see bgemm_kernel)
  const int64_t wg128 = (int64_t)n_batch * ((m + 127) / 128) * ((n + 191) / 192);
  const bool half_m = m > 64 && wg128 < 1024;
  if (!vec && tile == 3) JATTS_BGEMM_ORIENT(3, 16, false, 1);     // (n = d_k = 192 in one 64 x 192 tile here too: the T x T operand is read once)
  else if (!vec) JATTS_BGEMM_ORIENT(2, 16, false, 2);            // element loads: any alignment (a padded batch length T % 4 != 0 takes it for P v and its gradients)
  else if (tile == 3 && half_m) JATTS_BGEMM_ORIENT(3, 16, true, 1);
  else if (tile == 3) JATTS_BGEMM_ORIENT(3, 16, true, 2);
  else if (tile == 1) JATTS_BGEMM_ORIENT(1, 32, true, 2);
  else JATTS_BGEMM_ORIENT(2, 32, true, 2);
#undef JATTS_BGEMM_ORIENT
#undef JATTS_BGEMM_CASE
  if (rc != JATTS_OK) return rc;
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}

// The same product on the f32-EQUIVALENT emulated arithmetic (bgemm_emul_kernel).  `tile` (internal, tests): 0 = the dispatcher's choice, else WNF | MF << 4.
static int bgemm_emul_launch(BgemmArgs g, int n_outer, int trans_a, int trans_b, bool vec, int force, void* stream) {
  const int m = g.M, n = g.N;
  const int n_batch = n_outer * g.n_inner;
  auto launch = [&](auto kern, int bn, int bm) -> int {
    const int lds = 3 * EP * (bm + bn);
    g.n_batch = n_batch;
    g.gx = (n + bn - 1) / bn;
    g.gy = (m + bm - 1) / bm;
    const int64_t total = (int64_t)8 * ((n_batch + 7) / 8) * g.gx * g.gy;
    if (total >= (int64_t)1 << 31) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "bgemm_emul: launch too large");
    hipLaunchKernelGGL(kern, dim3((unsigned)total), dim3(256), lds, (hipStream_t)stream, g);
    return JATTS_OK;
  };
  int rc = JATTS_ERR_UNSUPPORTED;
#define JATTS_BE_CASE(WNF, AKv, BKv, VECv, MFv)                                  \
  do {                                                                           \
    JATTS_RAISE_LDS_LIMIT((bgemm_emul_kernel<WNF, AKv, BKv, VECv, MFv>));        \
    rc = launch(bgemm_emul_kernel<WNF, AKv, BKv, VECv, MFv>, 64 * WNF, 64 * MFv); \
  } while (0)
#define JATTS_BE_ORIENT(WNF, VECv, MFv)                                          \
  do {                                                                           \
    if (!trans_a && trans_b) JATTS_BE_CASE(WNF, true, true, VECv, MFv);          \
    else if (!trans_a && !trans_b) JATTS_BE_CASE(WNF, true, false, VECv, MFv);   \
    else if (trans_a && !trans_b) JATTS_BE_CASE(WNF, false, false, VECv, MFv);   \
    else JATTS_BE_CASE(WNF, false, true, VECv, MFv);                             \
  } while (0)
  // the cases of jatts_bgemm: n <= 64 | n <= 128 | 128 < n <= 192 in one piece | 64-row tiles where 128-row ones would leave fewer than two rounds of the
  // 512 two-per-CU slots
  const int n128 = (n + 127) / 128 * 128, n64 = (n + 63) / 64 * 64;
  int wnf = (n > 128 && n <= 192) ? 3 : (n64 * 4 <= n128 * 3 ? 1 : 2);
  const int64_t wg128 = (int64_t)n_batch * ((m + 127) / 128) * ((n + 191) / 192);
  int mf = (wnf == 3 && m > 64 && wg128 < 1024) || (wnf == 3 && !vec) ? 1 : 2;
  if (force) { wnf = force & 15; mf = force >> 4; }
  if (wnf == 1 && mf == 2) { if (vec) JATTS_BE_ORIENT(1, true, 2); else JATTS_BE_ORIENT(1, false, 2); }
  else if (wnf == 2 && mf == 2) { if (vec) JATTS_BE_ORIENT(2, true, 2); else JATTS_BE_ORIENT(2, false, 2); }
  else if (wnf == 3 && mf == 2) { if (vec) JATTS_BE_ORIENT(3, true, 2); else JATTS_BE_ORIENT(3, false, 2); }
  else if (wnf == 3 && mf == 1) { if (vec) JATTS_BE_ORIENT(3, true, 1); else JATTS_BE_ORIENT(3, false, 1); }
  else return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm_emul: no such tile");
#undef JATTS_BE_ORIENT
#undef JATTS_BE_CASE
  return rc;
}

extern "C" int jatts_bgemm_emul(const float* a, int64_t sa_outer, int64_t sa_inner, int32_t lda, int32_t trans_a, const float* b, int64_t sb_outer,
                                int64_t sb_inner, int32_t ldb, int32_t trans_b, float* c, int64_t sc_outer, int64_t sc_inner, int32_t ldc,
                                int32_t n_outer, int32_t n_inner, int32_t m, int32_t n, int32_t k, float alpha, int32_t accumulate, int32_t arith,
                                void* stream) {
  const int force = arith >> 8;      // (internal: bits 8.. force a tile, see bgemm_emul_launch; the arithmetic code is the low byte)
  arith &= 255;
  if (arith == JATTS_F32E6) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, "bgemm_emul: the six-product arithmetic (JATTS_F32E6) has no batched GEMM");
  if (arith != JATTS_F32E) return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm_emul: arith must be JATTS_F32E");
  if (!a || !b || !c) return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm_emul: null pointer");
  if (n_outer < 1 || n_inner < 1 || m < 1 || n < 1 || k < 1 || lda < 1 || ldb < 1 || ldc < 1)
    return jatts_set_error_msg(JATTS_ERR_ARG, "bgemm_emul: bad geometry");
  BgemmArgs g{a, b, c, sa_outer, sa_inner, sb_outer, sb_inner, sc_outer, sc_inner, lda, ldb, ldc, trans_a, trans_b, n_inner, m, n, k, alpha, accumulate, 0, 0, 0};
  const bool vec = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 &&
                   ((sa_outer | sa_inner | sb_outer | sb_inner | (int64_t)lda | (int64_t)ldb) & 3) == 0;
  const int rc = bgemm_emul_launch(g, n_outer, trans_a, trans_b, vec, force, stream);
  if (rc != JATTS_OK) return rc;
  JATTS_CHECK_LAUNCH();
  return JATTS_OK;
}
