// The bottom layer of the ray kernels (rtx_kernels.hip, whose opening comment has the whole picture): address-space macros, vector typedefs,
// scalar loads, lane and wave primitives.  Layers: rtx_wave.h <- rtx_math.h <- rtx_kernels.hip and the query kernels; each compiles on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rtx_device.h"
#include "rtx_tuning.h"

#pragma clang fp contract(off)

using namespace rtxd;

namespace {

// diagnostics that exist only in the instrumented build (RTX_DBG, rtx_tuning.h)
#if RTX_DBG
#define RTX_DBG_ONLY(...) __VA_ARGS__
#else
#define RTX_DBG_ONLY(...)
#endif
#if RTX_DBG || RTX_WAVE_TRACE
#define RTX_TRACE_ONLY(...) __VA_ARGS__
#else
#define RTX_TRACE_ONLY(...)
#endif

#define RTX_AS4 __attribute__((address_space(4)))
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
typedef float f2 __attribute__((ext_vector_type(2)));

// Wave-uniform loads through the constant address space -> SMEM instructions.
__device__ __forceinline__ uint32_t sload1(const void* p) { return *(const RTX_AS4 uint32_t*)(uintptr_t)p; }
__device__ __forceinline__ u32x8 sload8(const void* p) { return *(const RTX_AS4 u32x8*)(uintptr_t)p; }
__device__ __forceinline__ u32x16 sload16(const void* p) { return *(const RTX_AS4 u32x16*)(uintptr_t)p; }
__device__ __forceinline__ u32x4 sload4(const void* p) { return *(const RTX_AS4 u32x4*)(uintptr_t)p; }
__device__ __forceinline__ float sloadf(const float* p) { return __uint_as_float(sload1(p)); }
__device__ __forceinline__ const void* sloadp(const void* p)
{
	u32x2 v = *(const RTX_AS4 u32x2*)(uintptr_t)p;
	return (const void*)(((uint64_t)v.y << 32) | v.x);
}
#define F(x) __uint_as_float(x)
// Pins a wave-uniform value into SGPRs (v_readfirstlane) so that addresses derived from it select SMEM loads
// even when register pressure made the compiler park it in a VGPR.
__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T> __device__ __forceinline__ const T* uni(const T* p)
{
	const uint64_t a = (uint64_t)p;
	return (const T*)(((uint64_t)uni((uint32_t)(a >> 32)) << 32) | uni((uint32_t)a));
}

__device__ __forceinline__ float unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// lane index, recomputed where it is needed (two VALU instructions) instead of being kept live / spilled across the walk
__device__ __forceinline__ uint32_t laneNow()
{
	uint32_t l;
	asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
	return l;
}
// lane `lane` (wave-uniform) of v := val (wave-uniform); the lane select goes through m0 (constant-bus limit of gfx9)
__device__ __forceinline__ uint32_t writeLane(uint32_t val, uint32_t lane, uint32_t v)
{
	val = __builtin_amdgcn_readfirstlane(val); lane = __builtin_amdgcn_readfirstlane(lane);      // (folded away when already scalar)
	asm("" : "+s"(val));      // a register, never a literal (v_writelane_b32 takes no 32-bit literal on gfx9)
	asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(v) : "s"(val), "s"(lane) : "m0");
	return v;
}
#define RTX_AS1 __attribute__((address_space(1)))
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t ballot(bool b) { return __builtin_amdgcn_ballot_w64(b); }
// x < 0 per lane, compared where it is asked for: one v_cmp into a scalar pair that serves as the condition itself -- never a value that is kept, hoisted or spilled
__device__ __forceinline__ bool negNow(float x)
{
	uint64_t m;
	asm volatile("v_cmp_gt_f32_e64 %0, 0, %1" : "=s"(m) : "v"(x));
	return __builtin_amdgcn_inverse_ballot_w64(m);
}
// the lanes with |x| < bound, likewise
__device__ __forceinline__ uint64_t absBelowNow(float x, float bound)
{
	uint64_t m;
	asm volatile("v_cmp_lt_f32_e64 %0, |%1|, %2" : "=s"(m) : "v"(x), "s"(bound));
	return m;
}

// Ordering of scalar loads.  SMEM returns out of order, so lgkmcnt can only be waited down to zero: a load issued
// before the first use of the previous one is covered by the same wait and nothing overlaps.  after(x, v) is an
// empty asm that makes x depend on the value v having ARRIVED; deriving the next record's address from it forces
//     wait(current) -> issue(next) -> compute(current)
// without emitting an instruction.  The loads stay ordinary IR loads: every s_waitcnt is placed by the compiler.
template <typename T> __device__ __forceinline__ T after(T x, uint32_t v)
{
	asm("" : "+s"(x) : "s"(v));
	return x;
}

// Wave-wide maximum over the lanes (all 64 lanes execute this; lanes that must not contribute pass -inf).  Four DPP
// steps inside each row of 16, two row broadcasts, the result is read from lane 63.
__device__ __forceinline__ float waveMax(float v)
{
	// (one v_max_f32 with a DPP source per step; s_nop 1 = the two wait states before a DPP read of a just-written VGPR)
#define RTX_STEP(ctrl) "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " ctrl "\n\t"
	asm volatile(RTX_STEP("quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf") RTX_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
	             RTX_STEP("row_half_mirror row_mask:0xf bank_mask:0xf") RTX_STEP("row_mirror row_mask:0xf bank_mask:0xf")
	             RTX_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") RTX_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
	             "s_nop 0" : "+v"(v));
#undef RTX_STEP
	return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// max and min of one value over the wave, as two interleaved chains of v_max_f32 / v_min_f32 with a DPP source (one
// instruction per step and chain; s_nop 0 + the other chain's instruction = the two wait states a DPP read of a
// just-written VGPR needs).  Through __builtin_amdgcn_update_dpp every step is v_mov + v_mov_dpp + canonicalising v_max + v_max.
// Both chains start from ONE value v (lanes that must not contribute pass a quiet NaN, which v_max / v_min drop: one select per coordinate
// instead of one per chain).
__device__ __forceinline__ void waveMaxMin(float v, float& hi, float& lo)
{
#define RTX_STEP(ctrl) "v_max_f32_dpp %0, %0, %0 " ctrl "\n\tv_min_f32_dpp %1, %1, %1 " ctrl "\n\ts_nop 0\n\t"
	asm volatile("s_nop 1\n\t"
		"v_max_f32_dpp %0, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\tv_min_f32_dpp %1, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\ts_nop 0\n\t"
		RTX_STEP("quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf")
		RTX_STEP("row_half_mirror row_mask:0xf bank_mask:0xf") RTX_STEP("row_mirror row_mask:0xf bank_mask:0xf")
		RTX_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf") RTX_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
		"s_nop 0" : "=&v"(hi), "=&v"(lo) : "v"(v));
#undef RTX_STEP
	hi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(hi), 63));
	lo = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lo), 63));
}

} // namespace
