// prims.h — the device primitives shared by the kernel files: vector aliases, the bf16 rounding rule, LDS-DMA, the typed bf16
// MFMA, counted waits, the transposing LDS read, bit casts and the 64-lane butterfly reductions.  ONE definition each; nothing
// that belongs to a single kernel lives here.  Internal; not part of the C ABI.
#pragma once
#include "common.h"

namespace a3vt {

using u16 = unsigned short;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using i32x2 = __attribute__((ext_vector_type(2))) int;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using s16x4 = __attribute__((ext_vector_type(4))) short;
using s16x8 = __attribute__((ext_vector_type(8))) short;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;

// ---- bit casts (by-value arguments: __builtin_bit_cast applied directly to an element of an ext_vector reads element 0 with
// this compiler) ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned f32_bits(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float bits_f32(unsigned v) { return __builtin_bit_cast(float, v); }

// ---- ReLU as torch.relu has it: a NaN stays a NaN (fmaxf returns the other operand, 0), -0 becomes +0, every other value keeps
// its bits.  One unordered compare and a select.  (The GCN stack's epilogues keep their own NaN -> 0 form: DESIGN.md.)
__device__ __forceinline__ float relu_nan(float v) { return !(v <= 0.f) ? v : 0.f; }

// ---- bf16: THE rounding rule of the library (round to nearest even, v_cvt_pk_bf16_f32) -------------------------------------
__device__ __forceinline__ unsigned bf16_pack2(float a, float b) {  // two floats -> one packed pair, a in the low half
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){a, b}, bf16x2));
}
__device__ __forceinline__ u16 bf16_round(float v) { return (u16)(bf16_pack2(v, 0.f) & 0xffffu); }
__device__ __forceinline__ float bf16_lo(unsigned u) { return bits_f32(u << 16); }          // low half of a packed pair
__device__ __forceinline__ float bf16_hi(unsigned u) { return bits_f32(u & 0xffff0000u); }  // high half
__device__ __forceinline__ float bf16_to_f32(u16 h) { return bits_f32((unsigned)h << 16); }
// 4 floats -> the operand of v_mfma_f32_16x16x16_bf16 (a lane's ds_read_b128 holds k = 4q .. 4q+3 of its row)
__device__ __forceinline__ s16x4 cvt_bf16x4(f32x4 v) {
  return __builtin_bit_cast(s16x4, (u32x2){bf16_pack2(v[0], v[1]), bf16_pack2(v[2], v[3])});
}
// 8 floats -> 8 bf16 in one 16-byte register group
__device__ __forceinline__ f32x4 pack_bf16x8(f32x4 lo, f32x4 hi) {
  return __builtin_bit_cast(f32x4, (u32x4){bf16_pack2(lo[0], lo[1]), bf16_pack2(lo[2], lo[3]), bf16_pack2(hi[0], hi[1]),
                                           bf16_pack2(hi[2], hi[3])});
}

// ---- 16-byte LDS-DMA: each active lane copies 16 B from its own global address to lds_wave_base + lane * 16 ----------------
__device__ __forceinline__ void glds16(const void *gsrc, void *lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                   (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// ---- v_mfma_f32_16x16x32_bf16 on operands carried as 16-byte register groups (a ds_read_b128 of 8 bf16 IS the operand) -----
__device__ __forceinline__ f32x4 mfma_bf16x32(f32x4 a, f32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---- counted waits ---------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// ---- transposing LDS read (ds_read_b64_tr_b16) of a 32 x 4 bf16 operand from a row-major image: the address is (the lane's row
// of its first 4-row block, the lane's 4-column quad); the second block sits 16 rows further ------------------------------------
__device__ __forceinline__ bf16x8 tr_operand(const u16 *lds_row0_col, int row_stride_elems) {
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(lds_row0_col));
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) s16x4 *)(lds_row0_col + 16 * row_stride_elems));
  return __builtin_bit_cast(bf16x8, (s16x8){a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]});
}

// ---- 64-lane butterfly reductions; every lane gets the result ------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}

}  // namespace a3vt
