// What every fused HiFi-GAN unit kernel (resunit*_impl.h, resblock*_impl.h) does AROUND its arithmetic, once: the window a workgroup owns
// (unit_window_of), the residual / MRF store pass (unit_store), the launch rules (unit_launch) and the phase trace (JATTS_TRACE_*; the
// register-streamed conv, conv1d_direct.h, writes the same record; conv1d_emul16.h's DIAG trace is a record of its own and takes only the
// hardware-id reads from here).  Staging, MFMA loops and epilogues stay with their kernels.
// Reserved names: the macros JATTS_TRACE_BEGIN / JATTS_STAMP / JATTS_TRACE_END / JATTS_TRACE_HWID / JATTS_SITE stay defined in every translation unit
// that includes this header, and JATTS_TRACE_BEGIN declares the locals trace_, wg_lin and tracing in the kernel that uses it.
#pragma once
#include "conv_tiles.h"

extern unsigned long long* jatts_g_trace;  // profiling hook (conv_api.hip: jatts_debug_trace)
extern unsigned jatts_g_trace_cap;

// ---------------------------------------------------------------- phase trace
// Profiling hook (jatts_debug_trace): thread 0 of the first `cap` workgroups writes a record of 16 slots at trace + 16 wg --
// [hw id | XCC id << 32, s_memtime at JATTS_STAMP(1 .. 7), realtime at BEGIN, realtime at END, JATTS_STAMP(10 .. 12), -, -, -]; what a
// stamp index means is the kernel's (tools/trace_unit.py, tools/trace_conv.py).  Macros, not functions: the stamps must not move a single
// instruction of the kernel around them, and `wg` is the kernel's own expression for its linear workgroup index.
#define JATTS_TRACE_HWID(hwid, xcc)                                          \
  unsigned hwid, xcc;                                                        \
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));         \
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc))
#define JATTS_TRACE_BEGIN(trace, cap, wg)                                                         \
  unsigned long long* const trace_ = (trace);                                                     \
  const unsigned wg_lin = (wg);                                                                   \
  const bool tracing = trace_ != nullptr && wg_lin < (cap) && threadIdx.x == 0;                   \
  if (tracing) {                                                                                  \
    JATTS_TRACE_HWID(hwid, xcc);                                                                  \
    trace_[(size_t)wg_lin * 16] = ((unsigned long long)xcc << 32) | hwid;                         \
    trace_[(size_t)wg_lin * 16 + 8] = __builtin_amdgcn_s_memrealtime();                           \
  }                                                                                               \
  JATTS_STAMP(1)
#define JATTS_STAMP(i) do { if (tracing) trace_[(size_t)wg_lin * 16 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#define JATTS_TRACE_END() do { if (tracing) trace_[(size_t)wg_lin * 16 + 9] = __builtin_amdgcn_s_memrealtime(); } while (0)

namespace {

// ---------------------------------------------------------------- window frame
// The window of this workgroup in a launch over rg with `tt` output positions per window: sequence b, its length L (in positions: rows x
// len_mul), the window's first position t0 and the sequence's first row of x / y.  Grid: rectangular (windows of the longest sequence x
// sequences) or, for a ragged batch with host lengths, 1-D over the real windows (unit_launch).  false: no work -- a workgroup past the last
// window, or a window past its sequence's end.
// Two rules for the caller: (1) call it in converged code with all 64 lanes of every wave active -- ragged_locate is a wave-wide prefix sum;
// (2) call it, and return on false, BEFORE the kernel's first barrier: the exits are uniform over the workgroup, but a wave that left behind a
// barrier others still wait at would hang them.
struct unit_window {
  int b, L, t0;
  int64_t seq_row0;
};
__device__ __forceinline__ bool unit_window_of(const jatts_ragged& rg, int tt, unit_window& w) {
  int b = blockIdx.y, bx = blockIdx.x;
  if (ragged_is_1d(rg) && !ragged_locate(rg, tt, blockIdx.x, b, bx)) return false;   // 1-D grid over the real tiles of a ragged batch
  const int row_b = rg.cu_rows[b];
  w.b = b;
  w.L = (rg.cu_rows[b + 1] - row_b) * rg.len_mul;
  w.t0 = bx * tt;
  if (w.t0 >= w.L) return false;
  w.seq_row0 = (int64_t)row_b * rg.len_mul;
  return true;
}

// ---------------------------------------------------------------- store pass
// Unit-kernel output pass: y = (acc + b2 tile in LDS) + x [+ MRF partners] with row-contiguous 16-byte accesses;
// all global reads of a batch are issued before any is consumed (one round trip per batch, not per unit).
template <typename T, int C, int UB, bool ADD, int NTHR, bool RESID = true>
__device__ __forceinline__ void unit_store_pass(const void* add0, const void* add1, float out_scale, const char* ys, int pitch,
                                                int vrows, const T* xg, T* yg, int64_t g0) {
  typedef typename Elem<T>::vec8 V8;
  constexpr int UPR = C / 8;
  const int total = vrows * UPR;
  const bool has_add1 = ADD && add1 != nullptr;
  for (int u0 = threadIdx.x; u0 < total; u0 += UB * NTHR) {
    V8 xr[UB], a0[ADD ? UB : 1], a1[ADD ? UB : 1];
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const int u = u0 + i * NTHR;
      if (u < total) {
        if (RESID && JATTS_ABLATE != 3) xr[i] = Vec8IO<T>::ldg(xg + g0 + (int64_t)u * 8);
        if (ADD) {
          a0[i] = Vec8IO<T>::ldg((const T*)add0 + g0 + (int64_t)u * 8);
          if (has_add1) a1[i] = Vec8IO<T>::ldg((const T*)add1 + g0 + (int64_t)u * 8);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const int u = u0 + i * NTHR;
      if (u >= total) continue;
      const int r = u / UPR, cu = u - r * UPR;
      V8 v = Vec8IO<T>::lds(ys + (size_t)r * pitch + (size_t)cu * 8 * sizeof(T));
      if (RESID && JATTS_ABLATE != 3) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = from_f32<T>(to_f32(v[e]) + to_f32(xr[i][e]));  // residual
      }
      if (ADD) {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          v[e] = from_f32<T>((to_f32(v[e]) + to_f32(a0[i][e]) + (has_add1 ? to_f32(a1[i][e]) : 0.f)) * out_scale);
      }
      T* dst = yg + g0 + (int64_t)u * 8;
      if ((JATTS_ABLATE != 4 && JATTS_ABLATE != 12) || to_f32(v[0]) == 12345.678f) {
        if (sizeof(T) == 2) *reinterpret_cast<f16x8*>(dst) = *reinterpret_cast<const f16x8*>(&v);
        else {
          *reinterpret_cast<f32x4*>(dst) = f32x4{to_f32(v[0]), to_f32(v[1]), to_f32(v[2]), to_f32(v[3])};
          *reinterpret_cast<f32x4*>(dst + 4) = f32x4{to_f32(v[4]), to_f32(v[5]), to_f32(v[6]), to_f32(v[7])};
        }
      }
    }
  }
}

// The store pass of descriptor d (a unit's or a ResBlock's) over the `vrows` rows of the tile `ys`, which are contiguous in y from element g0
// (unit u <-> 8 elements at g0 + 8u); T = the type of x / y in HBM.  With MRF partners (d.add0: + the fused mean) the batch is half as long: they
// take the registers.  Small-channel kernels live on occupancy (up to 6 workgroups per CU) and keep the batch short either way.
template <typename T, int C, int NTHR, bool RESID = true, typename D>
__device__ __forceinline__ void unit_store(const D& d, const char* ys, int pitch, int vrows, int64_t g0) {
  constexpr bool keep_small = C <= 64;
  const T* xg = (const T*)d.x;
  T* yg = (T*)d.y;
  if (d.add0) unit_store_pass<T, C, keep_small ? 2 : 4, true, NTHR, RESID>(d.add0, d.add1, d.out_scale, ys, pitch, vrows, xg, yg, g0);
  else unit_store_pass<T, C, keep_small ? 4 : 8, false, NTHR, RESID>(d.add0, d.add1, d.out_scale, ys, pitch, vrows, xg, yg, g0);
}

// ---------------------------------------------------------------- launch rules
// The launcher's side of an error: its refusal text for a tile beyond the LDS, and its own file / line for a HIP error (jatts_set_error)
struct unit_site {
  const char* what;
  const char* file;
  int line;
};
#define JATTS_SITE(what) unit_site{what, __FILE__, __LINE__}

// A tile of `lds` bytes of dynamic LDS is refused beyond the CU's 160 KiB, else kernel Kern's limit is raised to it (jatts_raise_lds_limit).  Kern is
// a template ARGUMENT, so the limit cache is one per kernel instantiation.
template <auto Kern>
int unit_lds_ready(const unit_site& at, size_t lds) {
  if (lds > 160 * 1024) return jatts_set_error_msg(JATTS_ERR_UNSUPPORTED, at.what);
  static std::atomic<uint64_t> lds_done{0};
  const hipError_t e = jatts_raise_lds_limit(lds_done, (const void*)Kern);
  return e == hipSuccess ? JATTS_OK : jatts_set_error(e, at.file, at.line);
}

// Launch Kern(args...) with `nthr` threads and `lds` bytes per workgroup over the windows of rg, `tt` output positions each: the grid
// unit_window_of decodes -- windows of the longest sequence x sequences, or 1-D over exactly the real windows of a ragged batch.
template <auto Kern, typename... Args>
int unit_launch(const unit_site& at, int nthr, size_t lds, int tt, const jatts_ragged& rg, hipStream_t s, Args... args) {
  if (const int rc = unit_lds_ready<Kern>(at, lds)) return rc;
  const int64_t maxL = (int64_t)rg.max_len * rg.len_mul;
  dim3 grid((unsigned)((maxL + tt - 1) / tt), (unsigned)rg.n_seq);
  if (const int64_t n1 = ragged_tiles_1d(rg, tt)) grid = dim3((unsigned)n1);
  hipLaunchKernelGGL(Kern, grid, dim3(nthr), lds, s, args...);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? JATTS_OK : jatts_set_error(e, at.file, at.line);
}

}  // namespace
