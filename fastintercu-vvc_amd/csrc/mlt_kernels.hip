// mlt_kernels.hip -- hand-written gfx950 (CDNA4) kernels of the MLT-CNN split predictor.
//
// Arithmetic spec: /root/reference/mlt-cnn-python/codes/models/archs/mlt_ctu_or_pq_arch.py:32-57,273-299
// and mlt_cu_or_pq_arch.py:96-128; preprocessing: vtm-mlt-cpp/source/Lib/EncoderLib/EncCu.cpp:810-877.
//
// Data layout: activations NHWC fp16 in HBM; weights BN-folded, fp16, pre-packed on the host in
// MFMA A-fragment order (mlt_model.cpp) so a wave fetches one fragment as 64 x 16 contiguous bytes
// (LDS-DMA friendly, conflict-free ds_read_b128).  Accumulation, bias, residual add, global average
// pooling and the heads are fp32.
//
// MFMA orientation: D[cout][pixel] = sum_k W[cout][k] * X[k][pixel]  (weights = A, activations = B).
// With v_mfma_f32_32x32x16_f16 lane l (p = l&31, h = l>>5) supplies B[k = 8h+j][col p] = 8 consecutive
// input channels of pixel p -> ONE ds_read_b128 from the [pixel][cin] LDS patch, and receives
// D rows (i&3) + 8*(i>>2) + 4h of column p -> 4 consecutive output channels per register quad
// -> packed 8-byte NHWC stores.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include <atomic>
#include <cstdio>
#include <initializer_list>
#include <utility>

#include "mlt_kernels.h"

// build-time tuning knobs (scripts/sweep_cfg.py)
#ifndef CFG_ASM_PIPE  // 1: fragment ds_reads issued from inline asm, 2 items ahead, with counted lgkmcnt waits (fast arithmetic)
#define CFG_ASM_PIPE 1
#endif
#ifndef CFG_S2_BIAS_EARLY  // ... of the stride-2 ring kernels (two bias sets = 64 VGPRs)
#define CFG_S2_BIAS_EARLY 1
#endif
#ifndef CFG_DMA_SPREAD  // DMA mode: issue one patch piece every N fragment items of the MFMA loop (0: all before the loop)
#define CFG_DMA_SPREAD 5
#endif
#ifndef CFG_RING_FD16  // fragment prefetch distance of the 16-wave ring kernels (1 or 2 items): same speed, 16 VGPRs fewer at 1
#define CFG_RING_FD16 1
#endif
#ifndef CFG_RING_RES_EARLY
#define CFG_RING_RES_EARLY 1
#endif
#ifndef CFG_BIAS_EARLY  // 1: bias loads before the MFMA phase (latency hidden, +16..32 VGPRs); 0: at the epilogue
#define CFG_BIAS_EARLY 1
#endif

// -DMLT_PHASE_TIMING: wave 0 of every conv_mfma_kernel workgroup accumulates s_memtime deltas per phase into g_phase
// (debug builds only, scripts/phase_timing.py; perturbs the pipelining slightly)
#ifdef MLT_PHASE_TIMING
__device__ unsigned long long g_phase[16][8];
__device__ unsigned long long g_phase_chain[4][16];  // chain_kernel: [C == 256][S2] x 16 phases (see scripts/phase_timing.py)
extern "C" __attribute__((visibility("default"))) int mlt_debug_phase_read(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(g_phase)) != hipSuccess) return 1;
  if (reset) {
    static unsigned long long z[16][8];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
__device__ unsigned long long g_phase_l0[4][8];      // layer0_stream_kernel: stage x {top, reads + MFMA, epilogue, step end}
extern "C" __attribute__((visibility("default"))) int mlt_debug_phase_read_l0(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_l0), sizeof(g_phase_l0)) != hipSuccess) return 1;
  if (reset) {
    static unsigned long long z[4][8];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_l0), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
extern "C" __attribute__((visibility("default"))) int mlt_debug_phase_read_chain(unsigned long long *out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_chain), sizeof(g_phase_chain)) != hipSuccess) return 1;
  if (reset) {
    static unsigned long long z[4][16];
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_chain), z, sizeof(z)) != hipSuccess) return 1;
  }
  return 0;
}
// (one asm statement per stamp: s_memtime counts on lgkmcnt and returns out of order with LDS reads, so it must not be in flight
// inside the sections with counted lgkmcnt waits)
#define PHC_STAMP(t_) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory")
#define PHC_DECL unsigned int phc_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long phc_t; PHC_STAMP(phc_t)
#define PHC_MARK(i) do { unsigned long long n_; PHC_STAMP(n_); phc_acc[i] += (unsigned int)(n_ - phc_t); phc_t = n_; } while (0)
#define PHC_FLUSH(id) do { if (threadIdx.x == 0) { for (int i_ = 0; i_ < 16; ++i_) atomicAdd(&g_phase_chain[id][i_], (unsigned long long)phc_acc[i_]); } } while (0)
#define PH_DECL unsigned long long ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ph_t = __builtin_readcyclecounter()
#define PH_MARK(i) do { unsigned long long n_ = __builtin_readcyclecounter(); ph_acc[i] += n_ - ph_t; ph_t = n_; } while (0)
#define PH_FLUSH(id) do { if (threadIdx.x == 0) { for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_phase[id][i_], ph_acc[i_]); } } while (0)
#else
#define PH_DECL
#define PH_MARK(i)
#define PH_FLUSH(id)
#define PHC_DECL
#define PHC_MARK(i)
#define PHC_FLUSH(id)
#endif

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef float float4v __attribute__((ext_vector_type(4)));

#define LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))
#define GLB_PTR(p) ((const __attribute__((address_space(1))) void *)(p))

// one wave-instruction: 64 lanes x 16 B global -> 1 KiB of LDS at a wave-uniform base (lane-linear).
__device__ __forceinline__ void glds16(const void *gsrc_lane, void *lds_wave_base) {
  __builtin_amdgcn_global_load_lds(GLB_PTR(gsrc_lane), LDS_PTR(lds_wave_base), 16, 0, 0);
}

// compile-time loop: f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N-1>), so that the index can
// feed asm immediates and if constexpr
template <int... I, class F> __device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F &&f) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> __device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f));
}

// Fragment reads from inline asm.  While an LDS-DMA (global_load_lds) is pending the compiler makes every LDS wait an
// s_waitcnt lgkmcnt(0) and sinks the reads of the next item below the MFMAs of the current one, i.e. read -> full
// drain -> MFMA with the LDS latency exposed every item (seen in the ISA of every weight-ring kernel).  Reads issued
// here are invisible to that logic: they stay where they are written, and lds_wait<N>() + lds_touch() state exactly
// how many younger reads may still be in flight when a fragment is consumed (LDS operations of a wave return in order).
template <int OFF> __device__ __forceinline__ void lds_read128(half8 &dst, uint32_t addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds_read offset field is 16 bits");
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int N> __device__ __forceinline__ void lds_wait() {
  static_assert(N >= 0 && N <= 15, "lgkmcnt is 4 bits");
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void lds_touch(half8 &v) { asm volatile("" : "+v"(v)); }  // orders the consumer after lds_wait

// Phase stagger for persistent kernels: identical workgroups started together stay in lock-step chip-wide, so every CU
// reaches its memory-heavy phase (epilogue residual reads + stores) at the same moment and the launch takes
// T_compute + T_memory instead of max(...).  Delaying workgroup b by (b mod phases) * units * ~4 us spreads the phases.
__device__ __forceinline__ void stagger_start(int phases, int units) {
  const int k = ((int)blockIdx.x % phases) * units;
  for (int i = 0; i < k; ++i) __builtin_amdgcn_s_sleep(127);
}

// n / d for d >= 2 with magic = ceil(2^32 / d); exact while n * d < 2^32 (patch indices are < 2^16)
__device__ __forceinline__ uint32_t udiv_magic(uint32_t n, uint32_t magic) { return magic ? __umulhi(n, magic) : n; }  // magic 0: d == 1

// (org, |org - pred|) as an exact-integer fp16 pair: EncCu.cpp:816,827 (u16 cast), :833 (absdiff),
// :848-867 (clip to [0,1] after the 1/1023 scale == clip the integer to [0,1023]; the scale itself
// lives in the stem weights).
__device__ __forceinline__ uint32_t prep_pair(int16_t so, int16_t sp) {
  uint16_t o = (uint16_t)so, q = (uint16_t)sp;
  uint16_t r = o > q ? o - q : q - o;
  o = o > 1023 ? 1023 : o;
  r = r > 1023 ? 1023 : r;
  half2v hv;
  hv[0] = (_Float16)(float)o;
  hv[1] = (_Float16)(float)r;
  return *(uint32_t *)&hv;
}


// Flat-content guard statistic of one aligned quad (mlt_kernels.h: MLT_FLAT_RANGE): w[j] = prep_pair() of its four pixels, i.e. exact
// integers <= 1023 as fp16 pairs (org, |org - pred|) -> packed min / max / add / subtract are exact (|values| <= 2046).  A plane of the
// quad is "coherent" when its four values span <= MLT_FLAT_RANGE (constant, dither, low contrast) OR are linear to within one step
// (both second differences <= 1 in magnitude: ramps of any slope -- every pixel of a perfect gradient sees the same local pattern,
// so its rounding errors are as coherent as a constant area's); the quad counts when BOTH planes are.
// Returns bit 0: near-flat, bit 1: exactly flat (each plane constant or exactly linear; implies near-flat).
__device__ __forceinline__ int quad_flat_bits(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  const half2v a = *(half2v *)&w0, b = *(half2v *)&w1, c = *(half2v *)&w2, d = *(half2v *)&w3;
  const half2v mx = __builtin_elementwise_max(__builtin_elementwise_max(a, b), __builtin_elementwise_max(c, d));
  const half2v mn = __builtin_elementwise_min(__builtin_elementwise_min(a, b), __builtin_elementwise_min(c, d));
  const half2v r = mx - mn;
  const half2v d1 = (a + c) - (b + b), d2 = (b + d) - (c + c);
  const half2v l = __builtin_elementwise_max(__builtin_elementwise_max(d1, -d1), __builtin_elementwise_max(d2, -d2));
  const _Float16 R = (_Float16)MLT_FLAT_RANGE, one = (_Float16)1, zero = (_Float16)0;
  const bool near = (r[0] <= R || l[0] <= one) && (r[1] <= R || l[1] <= one);
  const bool exact = (r[0] == zero || l[0] == zero) && (r[1] == zero || l[1] == zero);
  return (near ? 1 : 0) | (exact ? 2 : 0);
}

// ---- FP8 lo products (round 4; hi+lo-weights forms on 64-channel chunks) ----
// The lo product of a (tap, 64-channel chunk) is ONE v_mfma_scale_f32_32x32x64_f8f6f4 (e4m3 x e4m3, twice the fp16 rate): its A operand is
// the FP8 lo plane (mlt_model.cpp: byte j of lane (r, h) = lo[cout r][cin 32 h + j]), its B operand channels 32 h .. 32 h + 31 of the lane's
// pixel from an e4m3 image of the activation (two ds_read_b128).  Lane (x, h) of A meets lane (y, h) of B byte for byte (probed with exact
// integer data: scripts/probes/f8_mfma_layout_probe.hip), so any channel order works as long as both operands use the same one.
typedef int int8v __attribute__((ext_vector_type(8)));
typedef short short2v __attribute__((ext_vector_type(2)));
// 8 fp16 activations (>= 0: every chain input is a ReLU output) -> 8 e4m3 bytes (2 dwords), clamped to e4m3's largest finite value
__device__ __forceinline__ void cvt_frag_fp8(const half8 &v, uint32_t &d0, uint32_t &d1) {
  const half2v top = {(_Float16)448, (_Float16)448};
  const half2v *h = (const half2v *)&v;
  short2v r = {0, 0};
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, __builtin_elementwise_min(h[0], top), 1.0f, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, __builtin_elementwise_min(h[1], top), 1.0f, true);
  d0 = *(uint32_t *)&r;
  short2v q = {0, 0};
  q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, __builtin_elementwise_min(h[2], top), 1.0f, false);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, __builtin_elementwise_min(h[3], top), 1.0f, true);
  d1 = *(uint32_t *)&q;
}
__device__ __forceinline__ float16v mfma_lo8(const half8 &a_lo, const half8 &a_hi, const half8 &b_lo, const half8 &b_hi, const float16v &c, int scale_a) {
  int8v a, b;
  const uint32_t *pl = (const uint32_t *)&a_lo, *ph = (const uint32_t *)&a_hi, *ql = (const uint32_t *)&b_lo, *qh = (const uint32_t *)&b_hi;
#pragma unroll
  for (int e = 0; e < 4; ++e) { a[e] = (int)pl[e]; a[4 + e] = (int)ph[e]; b[e] = (int)ql[e]; b[4 + e] = (int)qh[e]; }
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, scale_a, 0, 0x7F7F7F7F);  // fp8 x fp8; A scaled by 2^-lo8_exp, B by 1
}

// ---- exact-lite (NSPLIT == 6, round 5): both cross terms of the (hi, lo) product in ONE scaled FP8 MFMA ----
// lo parts of 8 fp16 activations (signed, |lo| <= 2^-11 |x|) * 2^12 -> 8 e4m3 bytes; clamped so that neither the fp16 product nor the e4m3
// conversion overflows (activations beyond ~220 lose part of their lo term; the calibration measures the outcome like any other tier's)
#define MLT_XL_LO_EXP 12
__device__ __forceinline__ void cvt_frag_fp8_lo(const half8 &v, uint32_t &d0, uint32_t &d1) {
  const half2v top = {(_Float16)0.109375, (_Float16)0.109375}, mul = {(_Float16)4096, (_Float16)4096};  // 448 / 4096
  const half2v *h = (const half2v *)&v;
  short2v r = {0, 0}, q = {0, 0};
  auto prep = [&](half2v x) { return __builtin_elementwise_max(__builtin_elementwise_min(x, top), -top) * mul; };
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, prep(h[0]), 1.0f, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, prep(h[1]), 1.0f, true);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, prep(h[2]), 1.0f, false);
  q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, prep(h[3]), 1.0f, true);
  d0 = *(uint32_t *)&r;
  d1 = *(uint32_t *)&q;
}
// A = [e4m3 Wl | e4m3 Wh] (lanes 0-31 | 32-63), B = [e4m3 Xh ; e4m3 Xl]; scale_a / scale_b: this LANE's E8M0 byte (replicated) for its 32 K elements
__device__ __forceinline__ float16v mfma_xl8(const half8 &a_lo, const half8 &a_hi, const half8 &b_lo, const half8 &b_hi, const float16v &c, int scale_a, int scale_b) {
  int8v a, b;
  const uint32_t *pl = (const uint32_t *)&a_lo, *ph = (const uint32_t *)&a_hi, *ql = (const uint32_t *)&b_lo, *qh = (const uint32_t *)&b_hi;
#pragma unroll
  for (int e = 0; e < 4; ++e) { a[e] = (int)pl[e]; a[4 + e] = (int)ph[e]; b[e] = (int)ql[e]; b[4 + e] = (int)qh[e]; }
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, scale_a, 0, scale_b);
}

// ---- 16-byte epilogue I/O -------------------------------------------------------------------------------------
// After a 32x32 MFMA lane l = (p, h) holds, per register quad q, output channels 8q+4h .. 8q+4h+3 of pixel p, so
// lanes p and p+32 own the two 8-byte halves of one 16-byte span.  v_permlane32_swap exchanges the upper half-wave
// of its first operand with the lower half-wave of its second: applied to quads (q, q+1) it leaves lanes 0-31 with
// channels 8q..8q+7 and lanes 32-63 with channels 8(q+1)..8(q+1)+7 -> ONE dwordx4 access per quad pair instead of
// two dwordx2 (half the memory instructions / requests, same bytes; cdna_hip_programming.md T21).
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4v pair16(half4 qa, half4 qb) {
  uint32_t ax = ((uint32_t *)&qa)[0], ay = ((uint32_t *)&qa)[1], bx = ((uint32_t *)&qb)[0], by = ((uint32_t *)&qb)[1];
  auto r0 = __builtin_amdgcn_permlane32_swap(ax, bx, false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(ay, by, false, false);
  uint4v v;
  v[0] = r0[0]; v[1] = r1[0]; v[2] = r0[1]; v[3] = r1[1];
  return v;
}
__device__ __forceinline__ void unpair16(uint4v v, half4 &qa, half4 &qb) {  // inverse of pair16 (the swap is an involution)
  auto r0 = __builtin_amdgcn_permlane32_swap(v[0], v[2], false, false);
  auto r1 = __builtin_amdgcn_permlane32_swap(v[1], v[3], false, false);
  ((uint32_t *)&qa)[0] = r0[0]; ((uint32_t *)&qa)[1] = r1[0];
  ((uint32_t *)&qb)[0] = r0[1]; ((uint32_t *)&qb)[1] = r1[1];
}

// Four accumulators -> four activated fp16 values, in packed arithmetic: v_pk_fma_f32 (acc * scale + bias), v_pk_add_f32 (+ residual),
// v_cvt_pk_f16_f32, v_pk_max_f16 -- 6 VALU ops per 4 values instead of 14 (the epilogues are VALU-bound phases in which no MFMA runs).
// The ReLU is applied AFTER the rounding: max(0, .) commutes with a monotonic rounding, so the values are those of fmaxf before it.
// x4 (optional) receives the fp32 values before the ReLU (GAP sums).
typedef float float2v __attribute__((ext_vector_type(2)));
template <int Q, class ACC = float16v> __device__ __forceinline__ half4 act_quad(const ACC &A, float scale, const float4v &b, bool has_res, const half4 &r, bool relu, float *x4 = nullptr) {
  half4 out;
#pragma unroll
  for (int ep = 0; ep < 2; ++ep) {
    float2v a2 = {A[4 * Q + 2 * ep], A[4 * Q + 2 * ep + 1]};
    const float2v b2 = {b[2 * ep], b[2 * ep + 1]};
    float2v x2 = a2 * scale + b2;
    if (has_res) {
      const float2v r2 = {(float)r[2 * ep], (float)r[2 * ep + 1]};
      x2 += r2;
    }
    if (x4) { x4[2 * ep] = x2[0]; x4[2 * ep + 1] = x2[1]; }
    half2v h2 = __builtin_convertvector(x2, half2v);
    if (relu) h2 = __builtin_elementwise_max(h2, (half2v){(_Float16)0, (_Float16)0});
    out[2 * ep] = h2[0];
    out[2 * ep + 1] = h2[1];
  }
  return out;
}

// ---- the kernels (one translation unit; split by family for readability) ----
#include "mlt_conv_kernels.inc"   // conv_epilogue, conv_mfma_kernel, conv_ring_dma_kernel
#include "mlt_chain_kernel.inc"   // chain_kernel (+ KARG)
#include "mlt_front_kernels.inc"  // block32_kernel, stem5_kernel, stem_block_kernel
#include "mlt_layer0_kernel.inc"  // layer0_stream_kernel
#include "mlt_layer1_kernel.inc"  // layer1_stream_kernel
#include "mlt_tail_kernels.inc"   // heads_kernel, flat_stat / guard kernels
#include "mlt_picture_kernels.inc"  // picture_gather_kernel, picture_gather_multi_kernel
#include "mlt_motion_kernels.inc"  // motion_search_kernel, picture_compensate_kernel
#include "mlt_tree_kernels.inc"  // tree_expand_kernel, tree_raster_kernel, tree_pack_kernel; tree sweeps: tree_expand_sweep_kernel, tree_sweep_raster / _rank / _pack_kernel

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per device: remember which device ordinals a kernel has been
// configured on (a process may hold contexts on several GPUs; concurrent first launches at worst set it twice).
struct DeviceOnce {
  std::atomic<uint64_t> mask[4] = {};
  bool need(int *dev) const {
    if (hipGetDevice(dev) != hipSuccess) *dev = 0;
    return !(mask[(*dev >> 6) & 3].load(std::memory_order_acquire) & (1ull << (*dev & 63)));
  }
  void done(int dev) { mask[(dev >> 6) & 3].fetch_or(1ull << (dev & 63), std::memory_order_release); }
};
constexpr int kBigLds = 160 * 1024;  // all of a CU's LDS
// THE launch path of every kernel that needs more than the default 64 KiB of LDS: raise the kernel's limit once per device, launch, report.
template <class K, class ARGS> static hipError_t launch_big_lds(K kern, DeviceOnce &once, dim3 grid, dim3 block, int lds, hipStream_t st, const ARGS &a) {
  int dev = 0;
  if (once.need(&dev)) {
    if (hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kBigLds); e != hipSuccess) return e;
    once.done(dev);
  }
  hipLaunchKernelGGL(kern, grid, block, lds, st, a);
  return hipGetLastError();
}
// ... with the once-flag as the kernel's own: this function, and its static with it, is instantiated per kernel, so no call site numbers a flag
template <auto KERN, class ARGS> static hipError_t launch_big_lds(dim3 grid, dim3 block, int lds, hipStream_t st, const ARGS &a) {
  static DeviceOnce once;
  return launch_big_lds(KERN, once, grid, block, lds, st, a);
}

// ---- the per-conv kernels: ONE row per instantiation of conv_mfma_kernel / conv_ring_dma_kernel ----
// A row is the key mlt_launch_conv selects it by and the kernel's template arguments, in the kernel's parameter order.  Everything else is derived
// from the row: the selection (select_row), the launch geometry (row_threads / row_grid_y / row_lds / row_accepts), the host's view of a layer's
// packing and tiling (mlt_conv_cfg), the ring bytes the dispatcher budgets patches against (mlt_conv_ring_bytes) and the text of
// mlt_debug_conv_table.  A tiling that several instantiations share is one description (add_fast / add_exact below); what a row must share with the rows
// the host reads and is not copied from them, table_consistent() checks at compile time.
// Measurement history of the tilings: docs/KERNEL_NOTES.md ("Per-conv tilings").
struct ConvRow {
  int cin, cout, stride, nsplit, variant;  // key.  nsplit: 1 fast, 2 exact (weights and activations hi+lo), 4 weights hi+lo on the FAST packing (MLT_MODEL_W2),
                                           // 6 exact-lite; variant: MLT_CONV_*
  bool ring;                               // conv_ring_dma_kernel (else conv_mfma_kernel)
  int taps; bool sc; int kc, kn, wcb, wpb, wc, wp, gt, rb, un, minw; bool dma; int cbp; bool kmaj;  // TAPS SC KC NSPLIT WCB WPB WAVES_C WAVES_P GT RB UN|UNP MINW DMA CBP KMAJ
  int nwl, fd;                             // ring only: NWL FD
  constexpr int cbt() const { return wcb * wc; }        // 32-cout blocks per workgroup tile
  constexpr int mt() const { return 32 * wpb * wp; }    // pixels per workgroup tile
};
constexpr ConvRow mfma_row(int cin, int cout, int stride, int nsplit, int variant, int taps, bool sc, int kc, int kn, int wcb, int wpb, int wc, int wp, int gt, int rb, int un,
                           int minw, bool dma = false, int cbp = 0, bool kmaj = false) {
  return {cin, cout, stride, nsplit, variant, false, taps, sc, kc, kn, wcb, wpb, wc, wp, gt, rb, un, minw, dma, cbp, kmaj, 0, 0};
}
constexpr ConvRow ring_row(int cin, int cout, int stride, int nsplit, int variant, bool sc, int kc, int wcb, int wpb, int wc, int wp, int gt, int rb, int unp, int minw, int nwl, int fd) {
  return {cin, cout, stride, nsplit, variant, true, 9, sc, kc, 1, wcb, wpb, wc, wp, gt, rb, unp, minw, true, 0, false, nwl, fd};
}
constexpr int DEF = MLT_CONV_DEFAULT, DMA = MLT_CONV_DMA, LAT = MLT_CONV_LATENCY, CEN = MLT_CONV_CENTRE;
// stride-2 convs always carry their block's projection shortcut (layer0.0's lives in stem5_kernel).
// A tiling that several instantiations share is written ONCE and copied by add_fast / add_exact:
//  - the exact tiling of a layer (nsplit 2) also runs exact-lite (6): the host sizes tiles and patches of both from the nsplit-2 row, so they are one description;
//  - the hi+lo-weights tier (nsplit 4) of a layer whose cin chunk is 32 in both packings has a DEFAULT row with the FAST tiling (all taps resident + persistent
//    workgroups for the 32-channel layers; w2_gt taps per ring step for the two big stride-2 layers: two weight planes, 5 would not fit the ring) -- the host sizes
//    its tiles from the fast row.  Its kernel is the NSPLIT = 3 form (weights hi+lo, fp16 lo plane).
// Every row is a kernel some caller can ask for: mlt_launch_conv is asked with nsplit 1, 2, 4 or 6, and no row has another.
struct ConvTable {
  ConvRow r[64] = {};  // (make_table fills 61)
  int n = 0;
  constexpr void add(ConvRow x) { r[n++] = x; }
  constexpr const ConvRow *begin() const { return r; }
  constexpr const ConvRow *end() const { return r + n; }
  constexpr void add_fast(ConvRow x, int w2_gt = 0) {  // x: the nsplit-1 DEFAULT row; w2_gt > 0: + the hi+lo-weights tier on this tiling
    add(x);
    if (w2_gt) { x.nsplit = 4; x.kn = 3; x.gt = w2_gt; add(x); }
  }
  constexpr void add_exact(ConvRow x) {  // x: the nsplit-2 row (DEFAULT or LATENCY)
    add(x);
    x.nsplit = x.kn = 6;
    add(x);
  }
};
constexpr ConvTable make_table() {
  ConvTable t;
  // ---- throughput tilings.  Fast: the layer's own tiling.  Exact: 32-channel chunks, two-deep ring; the >= 128-channel stride-1 layers on 128-pixel tiles
  // (these kernels serve the small-CU models, whose maps are tiny).
  //                  cin cout s  ns var TAPS SC    KC NS WCB WPB WC WP GT RB UN MINW   w2_gt
  t.add_fast(mfma_row(32, 32, 1, 1, DEF, 9, false, 32, 1, 1, 2, 1, 8, 9, 1, 5, 1), 9);       // all nine taps resident, persistent workgroups
  t.add_exact(mfma_row(32, 32, 1, 2, DEF, 9, false, 32, 2, 1, 2, 1, 8, 3, 2, 5, 1));         // UN 5: the 128 model's tiles have 4.4 - 4.8 patch items per lane
  t.add_fast(mfma_row(32, 64, 2, 1, DEF, 9, true, 32, 1, 1, 1, 2, 4, 10, 1, 5, 1), 10);      // all ten weight taps resident
  t.add_exact(mfma_row(32, 64, 2, 2, DEF, 9, true, 32, 2, 1, 1, 2, 4, 2, 2, 5, 1));          // 2 taps per step: 5 do not fit the LDS beside two activation planes
  t.add_fast(mfma_row(64, 64, 1, 1, DEF, 9, false, 64, 1, 2, 1, 1, 8, 9, 2, 6, 1));          // all weights of a 64-channel chunk resident (chain_kernel<64> reads this packing)
  t.add_exact(mfma_row(64, 64, 1, 2, DEF, 9, false, 32, 2, 2, 1, 1, 8, 1, 2, 3, 1));
  t.add_fast(mfma_row(64, 128, 2, 1, DEF, 9, true, 32, 1, 2, 1, 2, 4, 2, 2, 5, 1), 2);
  t.add_exact(mfma_row(64, 128, 2, 2, DEF, 9, true, 32, 2, 2, 1, 2, 4, 2, 2, 3, 1));         // UN 3: the 64 / 128-channel stride-2 layers lose with 5
  t.add_fast(mfma_row(128, 128, 1, 1, DEF, 9, false, 64, 1, 2, 1, 2, 8, 3, 2, 3, 1));        // one 16-wave workgroup per CU on 256-pixel tiles, 48 KiB weight steps (chain_kernel<128> reads this packing)
  t.add_exact(mfma_row(128, 128, 1, 2, DEF, 9, false, 32, 2, 2, 1, 2, 4, 1, 2, 2, 1));
  t.add_fast(mfma_row(128, 256, 2, 1, DEF, 9, true, 32, 1, 2, 1, 2, 4, 5, 2, 5, 1), 2);
  t.add_exact(mfma_row(128, 256, 2, 2, DEF, 9, true, 32, 2, 2, 1, 2, 4, 2, 2, 3, 1));
  t.add_fast(mfma_row(256, 256, 1, 1, DEF, 9, false, 64, 1, 2, 1, 2, 8, 3, 2, 4, 1));        // (chain_kernel<256> reads this packing)
  t.add_exact(mfma_row(256, 256, 1, 2, DEF, 9, false, 32, 2, 2, 1, 2, 4, 1, 2, 2, 1));
  // CU model (planes 32 / 64 / 96 / 128 / 256)
  t.add_fast(mfma_row(64, 96, 2, 1, DEF, 9, true, 32, 1, 3, 1, 1, 4, 1, 2, 5, 1));
  t.add_exact(mfma_row(64, 96, 2, 2, DEF, 9, true, 32, 2, 3, 1, 1, 4, 2, 2, 3, 1));
  t.add_fast(mfma_row(96, 96, 1, 1, DEF, 9, false, 32, 1, 3, 1, 1, 4, 3, 2, 3, 1));
  t.add_exact(mfma_row(96, 96, 1, 2, DEF, 9, false, 32, 2, 3, 1, 1, 4, 1, 2, 2, 1));
  t.add_fast(mfma_row(96, 128, 2, 1, DEF, 9, true, 32, 1, 2, 2, 2, 2, 2, 2, 5, 1));
  t.add_exact(mfma_row(96, 128, 2, 2, DEF, 9, true, 32, 2, 2, 2, 2, 2, 2, 2, 3, 1));
  // ---- LDS-DMA patch staging (fast arithmetic): resident weights for 64@32 on the tiles of its DEFAULT row, conv_ring_dma_kernel for the two big stride-2
  // layers (one workgroup per CU, its own pixel tiling: mlt_conv_cfg's mt_dma)
  //                                                                                     DMA
  t.add(mfma_row(64, 64, 1, 1, DMA, 9, false, 64, 1, 2, 1, 1, 8, 9, 1, 6, 1, true));   // UN 6: 10 x 34 pixels x 8 slots / (8 waves x 64 lanes) = 5.3 LDS-DMA instructions per wave and tile
  //             cin cout  s ns var SC    KC WCB WPB WC WP GT RB UNP MINW NWL FD
  t.add(ring_row(64, 128, 2, 1, DMA, true, 32, 2, 1, 2, 4, 5, 2, 20, 2, 0, 2));
  t.add(ring_row(128, 256, 2, 1, DMA, true, 32, 2, 1, 2, 4, 5, 2, 20, 2, 0, 2));
  // ---- latency variants (small launches): 32 couts x 128 pixels per 4-wave workgroup -- 4x the workgroups, a quarter of the weight bytes each -- on the
  // weights as the throughput row packs them (CBP: its 32-cout blocks per tile).  Per accumulator the order of the large tiles, so the same bits.
  //                                                                             DMA   CBP KMAJ
  t.add(mfma_row(64, 64, 1, 1, LAT, 9, false, 64, 1, 1, 1, 1, 4, 9, 1, 6, 1, false, 2));
  t.add(mfma_row(128, 128, 1, 1, LAT, 9, false, 64, 1, 1, 1, 1, 4, 9, 2, 6, 1, false, 4));   // GT 9: fastest of 1 / 3 / 9 in the batch-1 sweep
  t.add(mfma_row(256, 256, 1, 1, LAT, 9, false, 64, 1, 1, 1, 1, 4, 9, 2, 6, 1, false, 4));
  t.add(mfma_row(64, 128, 2, 1, LAT, 9, true, 32, 1, 1, 1, 1, 4, 10, 2, 10, 1, false, 4, true));   // all 10 weight taps of a chunk per step, k-step-major: the whole-stage kernel's accumulation order
  t.add(mfma_row(128, 256, 2, 1, LAT, 9, true, 32, 1, 1, 1, 1, 4, 10, 2, 10, 1, false, 4, true));
  t.add_exact(mfma_row(64, 64, 1, 2, LAT, 9, false, 32, 2, 1, 1, 1, 4, 1, 2, 4, 1, false, 2));
  t.add_exact(mfma_row(128, 128, 1, 2, LAT, 9, false, 32, 2, 1, 1, 1, 4, 1, 2, 4, 1, false, 4));
  t.add_exact(mfma_row(256, 256, 1, 2, LAT, 9, false, 32, 2, 1, 1, 1, 4, 1, 2, 4, 1, false, 4));
  t.add_exact(mfma_row(64, 128, 2, 2, LAT, 9, true, 32, 2, 1, 1, 1, 4, 2, 2, 5, 1, false, 4));
  t.add_exact(mfma_row(128, 256, 2, 2, LAT, 9, true, 32, 2, 1, 1, 1, 4, 2, 2, 5, 1, false, 4));
  // hi+lo weights on the FAST packing: the stride-1 layers with >= 64 channels (kc = 64) have this ONE per-conv form at any launch size -- large launches go
  // through chain_kernel<..., W2>, and this is its bit-identical per-conv form.  Kernel NSPLIT 3: fp16 lo plane (mlt_model.cpp), 5: FP8 lo plane
  t.add(mfma_row(64, 64, 1, 4, LAT, 9, false, 64, 3, 1, 1, 1, 4, 9, 1, 6, 1, false, 2));
  t.add(mfma_row(128, 128, 1, 4, LAT, 9, false, 64, 5, 1, 1, 1, 4, 3, 2, 6, 1, false, 4));
  t.add(mfma_row(256, 256, 1, 4, LAT, 9, false, 64, 5, 1, 1, 1, 4, 3, 2, 6, 1, false, 4));
  // ---- centre tap only (TAPS = 1): the small-CU models' layers on 1x1 maps, 128 samples per tile; stride 2: centre tap + projection shortcut on the same pixel
  t.add(mfma_row(128, 128, 1, 1, CEN, 1, false, 64, 1, 2, 1, 2, 8, 1, 1, 2, 1));
  t.add(mfma_row(128, 128, 1, 2, CEN, 1, false, 32, 2, 2, 1, 2, 4, 1, 1, 2, 1));
  t.add(mfma_row(128, 256, 2, 1, CEN, 1, true, 32, 1, 2, 1, 2, 4, 1, 2, 5, 1));
  t.add(mfma_row(128, 256, 2, 2, CEN, 1, true, 32, 2, 2, 1, 2, 4, 1, 2, 3, 1));
  t.add(mfma_row(256, 256, 1, 1, CEN, 1, false, 64, 1, 2, 1, 2, 8, 1, 1, 2, 1));
  t.add(mfma_row(256, 256, 1, 2, CEN, 1, false, 32, 2, 2, 1, 2, 4, 1, 1, 2, 1));
  return t;
}
constexpr ConvTable kTable = make_table();
constexpr int kNumRows = kTable.n;
constexpr const ConvRow (&kRows)[64] = kTable.r;  // (rows kNumRows .. 63 are unused)

constexpr int find_row(int cin, int cout, int stride, int nsplit, int variant) {
  for (int i = 0; i < kNumRows; ++i)
    if (kRows[i].cin == cin && kRows[i].cout == cout && kRows[i].stride == stride && kRows[i].nsplit == nsplit && kRows[i].variant == variant) return i;
  return -1;
}
// The row of a key, or -1: a pure function of the key.  A variant without a row of its own for the key is refused, except that DMA falls back to the
// DEFAULT row -- but not for nsplit 4: the hi+lo-weights tier has no LDS-DMA staging, and run_conv never asks for it.
constexpr int select_row(int cin, int cout, int stride, int nsplit, int variant) {
  const int i = find_row(cin, cout, stride, nsplit, variant);
  return (i < 0 && variant == MLT_CONV_DMA && nsplit != 4) ? find_row(cin, cout, stride, nsplit, MLT_CONV_DEFAULT) : i;
}

// launch geometry of a row
constexpr int row_threads(const ConvRow &r) { return 64 * (r.wc * r.wp + r.nwl); }
constexpr int row_grid_y(const ConvRow &r) { return r.cout / (32 * r.cbt()); }
constexpr int row_ring_bytes(const ConvRow &r) {  // the weight ring: slots x (weight planes of one step [+ the FP8 lo plane])
  const int plane = r.gt * (r.kc / 16) * r.cbt() * 1024;
  if (r.ring) return r.rb * plane;
  const int nbuf = (r.taps + (r.sc ? 1 : 0)) / r.gt > 1 ? r.rb : 1;
  return nbuf * ((r.kn == 2 || r.kn == 3 || r.kn == 6 ? 2 : 1) * plane + (r.kn == 5 ? r.gt * r.cbt() * 2048 : 0));
}
constexpr int row_lds(const ConvRow &r, int patch_bytes) {
  if (r.ring) return 2 * patch_bytes + row_ring_bytes(r) + (r.nwl ? 32 * r.cbt() * 4 * (r.sc ? 2 : 1) : 0);
  // (kernel NSPLIT 5: + the e4m3 copy of the patch, 80 bytes per pixel of the fp16 patch's KC * 2 + 16)
  const int patch8 = r.kn == 5 ? ((patch_bytes / (r.kc * 2 + 16) + 1) * (r.kc + 16) + 1023) / 1024 * 1024 : 0;
  return ((r.dma || r.kn == 2 || r.kn == 6) ? 2 : 1) * patch_bytes + row_ring_bytes(r) + patch8;
}
constexpr bool row_accepts(const ConvRow &r, int patch_bytes) {
  if (row_lds(r, patch_bytes) > kBigLds) return false;
  const int nw = r.wc * r.wp, nwp = r.nwl ? r.nwl - r.nwl / 2 : nw - nw / 2;  // ring: the patch waves issue at most UNP 1 KiB pieces each per stage
  return !r.ring || (patch_bytes >> 10) <= r.un * nwp;
}

// What the compiler checks for a new or edited row.  The host (mlt_conv_cfg -> PackedConv -> run_conv) reads the packing and the tile of a layer from its
// nsplit-1 / nsplit-2 DEFAULT rows only and uses that view for every other row of the layer; whatever a row shares with them and is not copied by
// add_fast / add_exact is held equal here:
constexpr bool weights_resident(const ConvRow &r, int gt) { return gt == r.taps + (r.sc ? 1 : 0) && r.cin == r.kc; }  // (the kernels' W_RESIDENT: persistent workgroups)
constexpr bool table_consistent() {
  for (const ConvRow &r : kTable) {
    // -- the weights: every row reads them as the DEFAULT row of its packing (fast: nsplit 1 and 4; exact: 2 and 6) tiles them -- same cin chunk, same
    //    32-cout blocks per tile; a latency row's narrower tile names the packed tile's blocks in CBP (128-cout tiles, 64 for the 64-channel layer)
    const bool fast_packing = r.nsplit == 1 || r.nsplit == 4;
    const int b = find_row(r.cin, r.cout, r.stride, fast_packing ? 1 : 2, MLT_CONV_DEFAULT);
    if (b < 0 || r.kc != kRows[b].kc || (r.cbp ? r.cbp : r.cbt()) != kRows[b].cbt()) return false;
    if (r.cout % (32 * r.cbt()) != 0 || r.cin % r.kc != 0 || (r.taps + (r.sc ? 1 : 0)) % r.gt != 0) return false;
    // -- the tile and the persistence decision: run_conv cuts tiles of pc.mt pixels (128 for a latency launch, mt_dma = the ring row's own for ring-DMA) and
    //    caps the grid when pc.gt says the weights are resident (centre tap: gt 1)
    if (r.variant == MLT_CONV_LATENCY) {
      if (r.mt() != 128 || weights_resident(r, r.gt) != weights_resident(r, kRows[b].gt)) return false;
    } else if (r.variant == MLT_CONV_CENTRE) {
      const int d = find_row(r.cin, r.cout, r.stride, r.nsplit, MLT_CONV_DEFAULT);
      if (d < 0 || r.gt != 1 || r.mt() != kRows[d].mt()) return false;
    } else if (!r.ring) {
      // (the tiles of a hi+lo-weights row -- nsplit 4 -- are the fast row's; its taps per step reach the host as gt_w2, read from the row itself)
      if (r.mt() != kRows[b].mt() || (r.nsplit != 4 && r.gt != kRows[b].gt)) return false;
    }
    if (r.variant == MLT_CONV_DEFAULT && r.nsplit == 1) {
      // -- every layer has the fast, the exact and the exact-lite arithmetic; where the hi+lo-weights tier runs on this tiling (a (nsplit 4, DEFAULT) row), the
      //    layer has ONE tiling of the weights for both packings (same kc / ct), so that tier finds the bytes it expects in either
      const int e = find_row(r.cin, r.cout, r.stride, 2, MLT_CONV_DEFAULT);
      if (e < 0 || find_row(r.cin, r.cout, r.stride, 6, MLT_CONV_DEFAULT) < 0) return false;
      if (find_row(r.cin, r.cout, r.stride, 4, MLT_CONV_DEFAULT) >= 0 && (r.kc != kRows[e].kc || r.cbt() != kRows[e].cbt())) return false;
    }
  }
  return true;
}
static_assert(table_consistent(), "a conv row disagrees with the packing or the tile of the rows the host reads for its layer (see table_consistent)");

template <int I> static hipError_t launch_row(const ConvArgs &a, int grid_x, hipStream_t st) {
  constexpr ConvRow r = kRows[I];
  if (!row_accepts(r, a.patch_bytes)) return hipErrorInvalidValue;
  const dim3 grid(grid_x, row_grid_y(r)), block(row_threads(r));
  const int lds = row_lds(r, a.patch_bytes);
  if constexpr (r.ring)
    return launch_big_lds<conv_ring_dma_kernel<r.cin, r.cout, r.stride, r.sc, r.kc, r.wcb, r.wpb, r.wc, r.wp, r.gt, r.rb, r.un, r.minw, r.nwl, r.fd>>(grid, block, lds, st, a);
  else
    return launch_big_lds<conv_mfma_kernel<r.cin, r.cout, r.stride, r.taps, r.sc, r.kc, r.kn, r.wcb, r.wpb, r.wc, r.wp, r.gt, r.rb, r.un, r.minw, r.dma, r.cbp, r.kmaj>>(grid, block, lds, st, a);
}
template <size_t... I> static hipError_t launch_rows(int row, std::index_sequence<I...>, const ConvArgs &a, int grid_x, hipStream_t st) {
  hipError_t e = hipErrorInvalidValue;
  (void)((row == (int)I && ((e = launch_row<(int)I>(a, grid_x, st)), true)) || ...);
  return e;
}
hipError_t mlt_launch_conv(int cin, int cout, int stride, int nsplit, int variant, const ConvArgs &a, int grid_x, hipStream_t st) {
  return launch_rows(select_row(cin, cout, stride, nsplit, variant), std::make_index_sequence<kNumRows>(), a, grid_x, st);
}

bool mlt_conv_has_centre_variant(int cin, int cout) {
  for (const ConvRow &r : kTable)
    if (r.variant == MLT_CONV_CENTRE && r.cin == cin && r.cout == cout) return true;
  return false;
}
int mlt_conv_ring_bytes(int cin, int cout, int stride, int nsplit, int variant) {
  const int i = select_row(cin, cout, stride, nsplit, variant);
  return i < 0 ? -1 : row_ring_bytes(kRows[i]);
}
// The host's view of a layer (packing, patch sizing): read off the rows the launcher selects
bool mlt_conv_cfg(int cin, int cout, int stride, int exact, ConvCfg *out) {
  const int ns = exact ? 2 : 1, i = find_row(cin, cout, stride, ns, MLT_CONV_DEFAULT);
  if (i < 0) return false;
  const ConvRow &r = kRows[i];
  const int d = find_row(cin, cout, stride, 1, MLT_CONV_DMA);  // LDS-DMA staging (fast arithmetic only): 1 resident weights (conv_mfma_kernel), 2 conv_ring_dma_kernel
  out->kc = r.kc; out->ct = 32 * r.cbt(); out->mt = r.mt(); out->gt = r.gt;
  out->dma = (exact || d < 0) ? 0 : kRows[d].ring ? 2 : 1;
  out->mt_dma = (d >= 0 && kRows[d].ring) ? kRows[d].mt() : out->mt;
  out->lat = find_row(cin, cout, stride, ns, MLT_CONV_LATENCY) >= 0 ? 1 : 0;
  const int w = find_row(cin, cout, stride, 4, MLT_CONV_DEFAULT);  // the hi+lo-weights tier on the fast tiling: its own taps per step (0: the layer has no such row)
  out->gt_w2 = w < 0 ? 0 : kRows[w].gt;
  return true;
}

// Host-only hook (not a product entry; no HIP call, no device): the table as text -- for the ten layer shapes, nsplit 1 / 2 / 3 / 4 / 6 and the four variants what
// mlt_launch_conv selects (kernel family <template arguments in parameter order>, threads per workgroup, grid.y, dynamic LDS bytes at patch_bytes 1024 / 32768,
// ring kernels: the largest patch_bytes, in KiB steps, the launcher accepts) or "rejected" (nsplit 3, which once had rows, for every key), and mlt_conv_cfg's view per shape.  tests/test_conv_table_cpu.py
// compares it with the text the launchers produced before they were table-driven.  Returns the length, or -1 when `cap` is too small.
extern "C" __attribute__((visibility("default"))) int mlt_debug_conv_table(char *out, size_t cap) {
  static const char *const kVariant[] = {"default", "dma", "latency", "centre"};
  size_t pos = 0;
  bool ok = out != nullptr;
  auto put = [&](const char *fmt, auto... v) {
    const int k = ok ? std::snprintf(out + pos, cap - pos, fmt, v...) : -1;
    if (k < 0 || (size_t)k >= cap - pos) ok = false; else pos += (size_t)k;
  };
  for (const ConvRow &s : kTable) {
    if (s.nsplit != 1 || s.variant != MLT_CONV_DEFAULT) continue;  // one fast DEFAULT row per layer shape
    for (int exact = 0; exact < 2; ++exact) {
      ConvCfg c{};
      mlt_conv_cfg(s.cin, s.cout, s.stride, exact, &c);
      put("cfg %d->%d s%d exact=%d: kc=%d ct=%d mt=%d mt_dma=%d gt=%d gt_w2=%d dma=%d lat=%d\n", s.cin, s.cout, s.stride, exact, c.kc, c.ct, c.mt, c.mt_dma, c.gt, c.gt_w2, c.dma, c.lat);
    }
    for (int nsplit : {1, 2, 3, 4, 6})
      for (int variant : {MLT_CONV_DEFAULT, MLT_CONV_DMA, MLT_CONV_LATENCY, MLT_CONV_CENTRE}) {
        put("conv %d->%d s%d nsplit=%d %s: ", s.cin, s.cout, s.stride, nsplit, kVariant[variant]);
        const int i = select_row(s.cin, s.cout, s.stride, nsplit, variant);
        if (i < 0) { put("%s", "rejected\n"); continue; }
        const ConvRow &r = kRows[i];
        if (r.ring) put("ring<%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d>", r.cin, r.cout, r.stride, (int)r.sc, r.kc, r.wcb, r.wpb, r.wc, r.wp, r.gt, r.rb, r.un, r.minw, r.nwl, r.fd);
        else put("mfma<%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d>", r.cin, r.cout, r.stride, r.taps, (int)r.sc, r.kc, r.kn, r.wcb, r.wpb, r.wc, r.wp, r.gt, r.rb, r.un, r.minw, (int)r.dma, r.cbp, (int)r.kmaj);
        put(" threads=%d grid_y=%d lds=%d/%d", row_threads(r), row_grid_y(r), row_lds(r, 1024), row_lds(r, 32768));
        if (r.ring) {
          int kib = kBigLds / 1024;
          while (kib > 0 && !row_accepts(r, kib * 1024)) --kib;
          put(" max_patch=%d", kib * 1024);
        }
        put("%s", "\n");
      }
  }
  if (!ok) return -1;
  return (int)pos;
}

// ---- LDS out-of-range probe: chain_kernel<..., OOBZ = true> lets a tap outside the map read beyond the LDS allocation and relies on
// the hardware returning zeros for such a DS read.  One workgroup with the chain kernels' full 160 KiB allocation reads where they do;
// *ok = 1 iff every lane saw zeros.  Run once per context at mlt_init: a device that answers differently gets the masked kernels. ----
__global__ __launch_bounds__(64) void lds_oob_probe_kernel(int *ok) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  *(uint4v *)(smem + 160 * 1024 - 1024 + lane * 16) = uint4v{0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu};  // (the allocation is really there)
  __syncthreads();
  half8 v;
  lds_read128<96>(v, 0x100000u + (uint32_t)lane * 16);  // same base as the chain kernels, an offset field in use
  lds_wait<0>();
  lds_touch(v);
  const uint4v u = *(const uint4v *)&v;
  const bool zero = (u[0] | u[1] | u[2] | u[3]) == 0;
  const unsigned long long all = __ballot(zero);
  if (lane == 0) *ok = all == ~0ull ? 1 : 0;
}
hipError_t mlt_probe_lds_oob(int *d_ok, hipStream_t st) { return launch_big_lds<lds_oob_probe_kernel>(dim3(1), dim3(64), kBigLds, st, d_ok); }

bool mlt_chain_supported(int c, int h) { return (c == 64 && h == 32) || (c == 128 && h == 16) || (c == 256 && h == 8); }
bool mlt_stage_supported(int c, int h) { return (c == 128 && h == 16) || (c == 256 && h == 8); }  // whole-stage (S2) variant

// fused chain kernels: (channels, map height) -> instantiation; 512 threads, one workgroup per sample (256 channels: per two samples)
template <class K> static hipError_t launch_chain_t(K kern, DeviceOnce &once, const ChainArgs &a, int grid_x, int threads, int lds, hipStream_t st) {
  return launch_big_lds(kern, once, dim3(grid_x), dim3(threads), lds, st, a);
}
template <auto KERN> static hipError_t launch_chain_t(const ChainArgs &a, int grid_x, int lds, hipStream_t st) { return launch_big_lds<KERN>(dim3(grid_x), dim3(512), lds, st, a); }
hipError_t mlt_launch_chain(int c, int h, bool with_s2, bool oob_zero, bool w2, const ChainArgs &a, int grid_x, hipStream_t st) {
  if (a.nconv != 3) return hipErrorInvalidValue;  // the chain is a stage's three stride-1 convs (run_chain3)
  // chain_kernel streams the weights as the stand-alone stride-1 layers' fast DEFAULT rows pack them
  constexpr ConvRow r64 = kRows[find_row(64, 64, 1, 1, MLT_CONV_DEFAULT)], r128 = kRows[find_row(128, 128, 1, 1, MLT_CONV_DEFAULT)], r256 = kRows[find_row(256, 256, 1, 1, MLT_CONV_DEFAULT)];
  static_assert(r64.kc == 64 && r64.wcb == 2 && r64.wc == 1 && r64.gt == 9, "chain_kernel<64,...> reads the packing of the stand-alone 64->64 layer");
  static_assert(r128.kc == 64 && r128.gt == 3 && r128.wcb == 2 && r128.wc == 2 && r256.kc == 64 && r256.gt == 3 && r256.wcb == 2 && r256.wc == 2,
                "chain_kernel reads the packing of the stand-alone 128->128 / 256->256 layers: 128-cout tiles, 64-channel chunks, 3 taps per step");
  constexpr int lds = 64 * 1024 + 2 * (r128.gt * (r128.kc / 16) * r128.cbt() * 1024);  // 64 KiB activation + two 48 KiB weight steps = all of the LDS
  if (w2) {  // hi+lo-weights forms (MLT_MODEL_W2 packing: the fast tiling, two planes): one tap per ring step, conv padding from beyond the LDS only
    if (!oob_zero || with_s2) return hipErrorInvalidValue;
    // ring step = hi fp16 plane + FP8 lo plane (LO8): 8 + 4 KiB per tap (64 channels), 16 + 8 KiB (128 / 256)
    if (c == 64 && h == 32)   // 128 KiB sample + 2 steps of two fp16 planes (8 + 8 KiB)
      return launch_chain_t<chain_kernel<64, 5, 0, 2, 4, 1, 8, 1, 2, 1, 2, 3, true, false, false, true, true, false>>(a, grid_x, 128 * 1024 + 2 * 16 * 1024, st);
    if (c == 128 && h == 16)  // 64 KiB sample + 2 ring steps + the 32 KiB e4m3 image of the sample
      return launch_chain_t<chain_kernel<128, 4, 0, 2, 2, 2, 4, 1, 2, 1, 2, 3, true, false, true, true, true, true>>(a, grid_x, (64 + 2 * 24 + 32) * 1024, st);
    if (c == 256 && h == 8)   // (64 KiB sample + 2 ring steps + the 32 KiB e4m3 image of the sample)
      return launch_chain_t<chain_kernel<256, 3, 1, 2, 1, 2, 4, 1, 2, 1, 2, 3, true, false, true, true, true, true>>(a, grid_x, (64 + 2 * 24 + 32) * 1024, st);
    return hipErrorInvalidValue;
  }
  // oob_zero: conv padding from DS reads beyond the LDS allocation (the probed default) or from zero masks; the kernels off the default path
  // (chains without the stride-2 front conv, MLT_NO_CHAIN_S2) exist in the masked form only
  if (c == 64 && h == 32 && !with_s2) {  // 8 waves x (64 couts x 128 pixels), one 128 KiB sample per workgroup, 2 taps per weight step: 2 x 16 KiB ring, 5 barriers per conv
    constexpr int lds64 = 128 * 1024 + 4 * 8 * 1024;
    if (oob_zero) return launch_chain_t<chain_kernel<64, 5, 0, 2, 4, 1, 8, 2, 2, 1, 2, 3, true, false, false, true>>(a, grid_x, lds64, st);
    return launch_chain_t<chain_kernel<64, 5, 0, 2, 4, 1, 8, 2, 2, 1, 2, 3, true, false, false, false>>(a, grid_x, lds64, st);
  }
  if (c == 128 && h == 16) {  // 8 waves x (64 couts x 64 pixels), one sample per workgroup
    if (with_s2) {
      if (oob_zero) return launch_chain_t<chain_kernel<128, 4, 0, 2, 2, 2, 4, 3, 2, 2, 2, 3, true, true, true, true>>(a, grid_x, lds, st);
      return launch_chain_t<chain_kernel<128, 4, 0, 2, 2, 2, 4, 3, 2, 2, 2, 3, true, true, true, false>>(a, grid_x, lds, st);
    }
    return launch_chain_t<chain_kernel<128, 4, 0, 2, 2, 2, 4, 3, 2, 2, 2, 3, true>>(a, grid_x, lds, st);
  }
  if (c == 256 && h == 8) {   // 8 waves x (64 couts x 32 pixels) x 2 cout passes, two samples per workgroup
    if (with_s2) {
      if (oob_zero) return launch_chain_t<chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true, true, true, true>>(a, grid_x, lds, st);
      return launch_chain_t<chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true, true, true, false>>(a, grid_x, lds, st);
    }
    return launch_chain_t<chain_kernel<256, 3, 1, 2, 1, 2, 4, 3, 2, 2, 2, 3, true>>(a, grid_x, lds, st);
  }
  return hipErrorInvalidValue;
}
hipError_t mlt_launch_stage256_wide(const ChainArgs &a, int grid_x, hipStream_t st) {
  static DeviceOnce once;
  if (a.nconv != 3 || !a.s2_w) return hipErrorInvalidValue;
  return launch_chain_t(stage256_wide_kernel, once, a, grid_x, 512, 160 * 1024, st);
}

hipError_t mlt_launch_stem5(const Stem5Args &a, int nsplit, int grid_x, int lds, hipStream_t st) {
  if (nsplit == 3) hipLaunchKernelGGL(stem5_kernel<3>, dim3(grid_x), dim3(256), lds, st, a);
  else if (nsplit == 2) hipLaunchKernelGGL(stem5_kernel<2>, dim3(grid_x), dim3(256), lds, st, a);
  else hipLaunchKernelGGL(stem5_kernel<1>, dim3(grid_x), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_block32(const Block32Args &a, bool w2, int grid_x, hipStream_t st) {
  if (w2)  // 8 x 32 tiles: X 12 x 36, T 10 x 34 pixels at 80 B + two weight planes per conv
    return launch_big_lds<block32_kernel<3, true>>(dim3(grid_x), dim3(512), (12 * 36 + 10 * 34) * 80 + 4 * 18 * 1024, st, a);
  return launch_big_lds<block32_kernel<4, false>>(dim3(grid_x), dim3(512), (20 * 36 + 18 * 34) * 80 + 2 * 18 * 1024, st, a);
}

hipError_t mlt_launch_stem_block(const StemBlockArgs &a, bool w2, int grid_x, hipStream_t st) {
  // 3 raw + 2 T buffers + conv2 weights (hi+lo-weights form: its LO plane -- the hi plane lives in the consumer waves' registers) + biases +
  // border k-steps (one or two planes) = 149 / 151 KiB
  constexpr int lds = 3 * (39 * 72 * 4 + 16) + 2 * (18 * 34 * 80) + 18 * 1024 + 256 + 2 * 1024;
  const dim3 grid(grid_x), block(128 * CFG_SB_NWS);  // one workgroup per CU, two pipeline stages inside
  if (w2) return launch_big_lds<stem_block_kernel<true>>(grid, block, lds + 2 * 1024, st, a);
  return launch_big_lds<stem_block_kernel<false>>(grid, block, lds, st, a);
}

// fuse5: + layer1's stride-2 conv and shortcut as a fifth stage; mfma32: round 5's MFMA shape (MLT_TUNING=1 MLT_L0_MFMA32=1: same-box A/B; same bits).
// The four-stage form (fuse5 = false: weight sets whose layer1 does not open on the single pass) stays on 32x32x16: its 16x16x32 build reloads three of S2's
// weight fragments from scratch every row (S2 carries two accumulator sets; the five-stage form's register allocation comes out without that), and it
// was the five-stage form the A/B measured.
// xs: the five-stage 16x16x32 form that hands layer1_stream_xs_kernel the shortcut's input instead of the shortcut (a new symbol over the shared body).
hipError_t mlt_launch_layer0_stream(const Layer0Args &a, bool fuse5, bool mfma32, bool xs, int grid_x, hipStream_t st) {
  const dim3 grid(grid_x), block(1024);  // one persistent workgroup per CU slot
  if (xs) {
    if (!fuse5 || mfma32) return hipErrorInvalidValue;
    return launch_big_lds<layer0_stream_xs_kernel>(grid, block, MLT_L0F_LDS_BYTES, st, a);
  }
  if (fuse5) return mfma32 ? launch_big_lds<layer0_stream_kernel<true, false>>(grid, block, MLT_L0F_LDS_BYTES, st, a) : launch_big_lds<layer0_stream_kernel<true, true>>(grid, block, MLT_L0F_LDS_BYTES, st, a);
  return launch_big_lds<layer0_stream_kernel<false, false>>(grid, block, MLT_L0_LDS_BYTES, st, a);
}

hipError_t mlt_launch_layer1_stream(const Layer1Args &a, bool mfma32, bool xs, int grid_x, hipStream_t st) {
  const dim3 grid(grid_x), block(1024);
  if (xs) {      // behind layer0_stream_xs_kernel: a.sc holds the shortcut's input, the loader waves compute the shortcut (32x32x16 form)
    if (!mfma32 || !a.w_sc || !a.bias_sc) return hipErrorInvalidValue;
    return launch_big_lds<layer1_stream_xs_kernel>(grid, block, MLT_L1X_LDS_BYTES, st, a);
  }
  // mfma32 is the default: round 5's form on v_mfma_f32_32x32x16_f16 (MLT_TUNING=1 MLT_L1_MFMA16=1 selects the other; same bits)
  if (mfma32) return launch_big_lds<layer1_stream_kernel<false>>(grid, block, MLT_L1_LDS_BYTES, st, a);
  return launch_big_lds<layer1_stream_kernel<true>>(grid, block, MLT_L1_LDS_BYTES, st, a);
}

hipError_t mlt_launch_heads(const HeadArgs &a, int n, hipStream_t st) {
  if (a.cand || a.cand_cov > 0.f || a.cand_max > 0) hipLaunchKernelGGL(heads_cand_kernel, dim3(n), dim3(256), 0, st, a);
  else if (a.dec || a.min_conf > 0.f) hipLaunchKernelGGL(heads_kernel<true>, dim3(n), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(heads_kernel<false>, dim3(n), dim3(256), 0, st, a);
  return hipGetLastError();
}

// n workgroups: the CUs of the pass (fix-up launches: of the exact re-run)
hipError_t mlt_launch_heads_sweep(const HeadSweepArgs &a, int n, hipStream_t st) {
  if (a.n_qps < 1 || a.n_qps > MLT_SWEEP_MAX_QPS_K || ((a.fix_idx || a.h.g_next) && !a.mask)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sweep_heads_kernel, dim3(n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_flat_stat(const FlatStatArgs &a, bool aligned8, hipStream_t st) {
  if (aligned8) hipLaunchKernelGGL(flat_stat_kernel<true>, dim3(a.n), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(flat_stat_kernel<false>, dim3(a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_guard_select(const GuardSelectArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(guard_select_kernel, dim3(1), dim3(1024), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_guard_gather(const GuardGatherArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(guard_gather_kernel, dim3(a.k, 2), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_guard_scatter(const GuardScatterArgs &a, hipStream_t st) {
  const int items = a.k * (a.n_logits + 1);
  hipLaunchKernelGGL(guard_scatter_kernel, dim3((items + 255) / 256), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The flat grid-stride launch shape of the picture and tree kernels: workgroups of 256 over `items` work items -- enough to fill the device (256 CUs x 8 waves of
// 64 = 8 workgroups of 256 per CU), never more than there are items.
static dim3 flat_grid(size_t items) {
  const size_t want = (items + 255) / 256;
  return dim3((unsigned)(want < 2048 ? want : 2048));
}
// what lives in LDS arrays of the ABI's maxima: the per-picture ranks of the expand kernels, the slices' starts of the sweep pack
static bool tree_counts_ok(int n_pictures, int n_qps = 1) {
  return n_qps >= 1 && n_qps <= MLT_SWEEP_MAX_QPS_K && n_pictures >= 1 && n_pictures <= MLT_TREES_MAX_PICTURES_K;
}

// over 16-byte items (mlt_picture_kernels.inc): two planes x c x S x S / 8
hipError_t mlt_launch_picture_gather(const PictureGatherArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(picture_gather_kernel, flat_grid((size_t)a.c << (2 * a.s_l - 2)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_picture_gather_multi(const PictureGatherMultiArgs &a, hipStream_t st) {
  const size_t items = (size_t)a.c << (2 * a.s_l - 2);
  if (!items) return hipSuccess;
  hipLaunchKernelGGL(picture_gather_multi_kernel, flat_grid(items), dim3(256), 0, st, a);
  return hipGetLastError();
}

// one workgroup per block (mlt_motion_kernels.inc); the LDS follows (block, range) -- window and block are 81,920 bytes at (64, 64), so the launch takes the big-LDS
// path whatever the case
int mlt_motion_search_lds(int block, int range) { const int wn = block + 2 * range; return (wn * wn + block * block) * 2 + 32; }
hipError_t mlt_launch_motion_search(const MotionSearchArgs &a, int by, hipStream_t st) {
  const int block = 1 << a.block_l;
  if (a.block_l < 3 || a.block_l > 6 || a.range < 0 || a.range > 64 || a.bx < 1 || by < 1) return hipErrorInvalidValue;
  return launch_big_lds<motion_search_kernel>(dim3((unsigned)a.bx, (unsigned)by), dim3(256), mlt_motion_search_lds(block, a.range), st, a);
}

// one workgroup per block; 37,120 bytes of LDS at block 64, 3,328 at block 16: the plain launch path
int mlt_motion_refine_lds(int block) { const int wp = block + 8; return wp * block * 4 + 128 + (wp * wp + block * block) * 2; }
hipError_t mlt_launch_motion_refine(const MotionRefineArgs &a, int by, hipStream_t st) {
  if (a.block_l < 3 || a.block_l > 6 || a.subpel < 0 || a.subpel > 2 || a.n_refs < 1 || a.n_refs > MLT_MOTION_MAX_REFS_K || a.bx < 1 || by < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(motion_refine_kernel, dim3((unsigned)a.bx, (unsigned)by), dim3(256), mlt_motion_refine_lds(1 << a.block_l), st, a);
  return hipGetLastError();
}

// one workgroup per tile of at most 16 rows x 64 columns of a block
hipError_t mlt_launch_picture_compensate(PictureCompensateArgs a, hipStream_t st) {
  if (a.block_l < 3 || a.block_l > 6 || a.bx < 1 || a.by < 1) return hipErrorInvalidValue;
  const int block = 1 << a.block_l;
  a.tiles_y = block > MLT_MC_TILE_H ? block / MLT_MC_TILE_H : 1;
  hipLaunchKernelGGL(picture_compensate_kernel, dim3((unsigned)a.bx, (unsigned)(a.by * a.tiles_y)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ONE workgroup: the ordered compaction carries its running base from tile to tile (mlt_tree_kernels.inc)
hipError_t mlt_launch_tree_expand(const TreeExpandArgs &a, hipStream_t st) {
  if (!tree_counts_ok(a.n_pictures)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tree_expand_kernel, dim3(1), dim3(MLT_TREE_TILE), 0, st, a);
  return hipGetLastError();
}

// over the 16 x 16 blocks of the level's nodes
hipError_t mlt_launch_tree_raster(const TreeRasterArgs &a, hipStream_t st) {
  const size_t items = (size_t)a.lvl_n << (2 * a.blk_l);
  if (!items) return hipSuccess;
  hipLaunchKernelGGL(tree_raster_kernel, flat_grid(items), dim3(256), 0, st, a);
  return hipGetLastError();
}

// over the nodes of all levels
hipError_t mlt_launch_trees_pack(const TreesPackArgs &a, hipStream_t st) {
  if (a.total <= 0) return hipSuccess;
  hipLaunchKernelGGL(tree_pack_kernel, flat_grid((size_t)a.total), dim3(256), 0, st, a);
  return hipGetLastError();
}

// tree sweeps -- ONE workgroup, as mlt_launch_tree_expand
hipError_t mlt_launch_tree_expand_sweep(const TreeSweepExpandArgs &a, hipStream_t st) {
  if (!tree_counts_ok(a.n_pictures, a.n_qps)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tree_expand_sweep_kernel, dim3(1), dim3(MLT_TREE_TILE), 0, st, a);
  return hipGetLastError();
}

hipError_t mlt_launch_tree_sweep_raster(const TreeSweepRasterArgs &a, hipStream_t st) {
  const size_t items = (size_t)a.lvl_n << (2 * a.blk_l);
  if (!items) return hipSuccess;
  hipLaunchKernelGGL(tree_sweep_raster_kernel, flat_grid(items), dim3(256), 0, st, a);
  return hipGetLastError();
}

// one workgroup per (entry, point)
hipError_t mlt_launch_tree_sweep_rank(const TreeSweepPackArgs &a, hipStream_t st) {
  if (!tree_counts_ok(a.n_pictures, a.n_qps)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(tree_sweep_rank_kernel, dim3((unsigned)(a.n_pictures * a.n_qps)), dim3(MLT_TREE_TILE), 0, st, a);
  return hipGetLastError();
}

// over (point, union node); at least workgroup 0, which writes first_node[] and union_nodes[]
hipError_t mlt_launch_tree_sweep_pack(const TreeSweepPackArgs &a, hipStream_t st) {
  if (!tree_counts_ok(a.n_pictures, a.n_qps)) return hipErrorInvalidValue;
  size_t items = 0;
  for (int l = 0; l < a.n_levels; ++l) items += (size_t)a.lvl_n[l];
  items *= (size_t)a.n_qps;
  hipLaunchKernelGGL(tree_sweep_pack_kernel, flat_grid(items ? items : 1), dim3(256), 0, st, a);
  return hipGetLastError();
}
