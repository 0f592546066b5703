// V3 and the correctly rounded vector maths, the restated powf and the shading helpers of the ray kernels (rtx_kernels.hip's opening comment has the whole picture).
#pragma once
#include "rtx_wave.h"

namespace {

constexpr float kFltMax = 3.402823466e+38f;
// (double)x < 1e-8 for a float x  <=>  x < 0x322bcc78 (the smallest float >= the double 1e-8);
// objects.cpp:76,79,810 compare in double.
#define RTX_EPS8 __uint_as_float(0x322bcc78u)

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator*(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return mk(a.x / s, a.y / s, a.z / s); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }   // geometry.h:84-87
__device__ __forceinline__ float len2(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
// geometry.h:99-102: (float)sqrt((double)len2) == correctly rounded sqrtf (53 >= 2*24+2)
__device__ __forceinline__ float length(V3 a) { return __builtin_sqrtf(len2(a)); }
// geometry.h:104-112: factor = (float)(1 / sqrt((double)len2)).  As written that is ~40 fp64 instructions (an fp64 square root and an fp64 division: two quarter-rate
// transcendentals and two dozen half-rate FMAs), several times per shaded point (the primary direction, the normal, every light's L).  The fast path below
// reaches the SAME float in 16 fp32 instructions: v_rsq_f32, one Newton step whose residual 1 - l2 y^2 is formed exactly (FMA: l2 y = t + te), and the exact
// residual e1 of the candidate y1, which says how far y1 is from the true 1 / sqrt(l2) in units of its own last place: |y1 e1| / 2 < ulp / 2 (1 - 2^-16) means y1 is the
// correctly rounded float of the true value with room to spare, and the reference's value -- the true value rounded to double twice (relative 2^-52), then to
// float -- can only differ from that within 2^-28 ulp of a rounding boundary.  Otherwise (15 inputs in a million), and outside [2^-60, 2^60], the lane takes the
// fp64 path.  Proof by enumeration: tools/research/rsqrt_exhaustive.c tries every mantissa, both exponent parities and every starting value within 3 ulp
// of the truth (352 M cases: accepted => bit-identical; v_rsq_f32 is good to 1 ulp); on the device tests/test_gpu_parity.py runs all 2^24 mantissas.
__device__ __forceinline__ float invLenSlow(float l2) { return (float)(1.0 / __builtin_sqrt((double)l2)); }
__device__ __forceinline__ float invLenD(float l2)
{
	const float y0 = __builtin_amdgcn_rsqf(l2);
	const float t = l2 * y0, te = __builtin_fmaf(l2, y0, -t);
	float e = __builtin_fmaf(-t, y0, 1.0f); e = __builtin_fmaf(-te, y0, e);
	const float y1 = __builtin_fmaf(y0 * 0.5f, e, y0);
	const float t1 = l2 * y1, t1e = __builtin_fmaf(l2, y1, -t1);
	float e1 = __builtin_fmaf(-t1, y1, 1.0f); e1 = __builtin_fmaf(-t1e, y1, e1);
	const float ulp = __uint_as_float((__float_as_uint(y1) & 0x7f800000u) - (23u << 23));
	const bool sure = fabsf(e1 * y1) < ulp * 0.99998474f && l2 >= 0x1p-60f && l2 <= 0x1p60f;      // (NaN compares false: the fp64 path)
	float r = y1;
	if (!sure) r = invLenSlow(l2);
	return r;
}
__device__ __forceinline__ V3 normalized(V3 a)
{
	float l2 = len2(a);
	if (l2 > 0) {
		float f = invLenD(l2);
		a.x *= f; a.y *= f; a.z *= f;
	}
	return a;
}
__device__ __forceinline__ float fminRef(float a, float b) { return (b < a) ? b : a; }   // std::min(a,b)
__device__ __forceinline__ float fmaxRef(float a, float b) { return (a < b) ? b : a; }   // std::max(a,b)
__device__ __forceinline__ float clampRef(float lo, float hi, float v) { return fmaxRef(lo, fminRef(hi, v)); }

// ------------------------------------------------------------------------------------------------
// powf -- glibc 2.35 e_powf.c (ARM optimized-routines) as executed by the x86-64 FMA ifunc variant.
// Tables: __powf_log2_data (16 x {invc, logc}, poly A[5]) and __exp2f_data (32 x u64, shift, poly C[3]).
// ------------------------------------------------------------------------------------------------
__device__ const double kLog2Tab[32] = {
	0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2, 0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2,
	0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2,  0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2,
	0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2, 0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3,
	0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3, 0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4,
	0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5, 0x1p+0, 0x0p+0,
	0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4,  0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3,
	0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3,  0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2,
	0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2,  0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2,
};
__device__ const uint64_t kExp2Tab[32] = {
	0x3ff0000000000000, 0x3fefd9b0d3158574, 0x3fefb5586cf9890f, 0x3fef9301d0125b51, 0x3fef72b83c7d517b,
	0x3fef54873168b9aa, 0x3fef387a6e756238, 0x3fef1e9df51fdee1, 0x3fef06fe0a31b715, 0x3feef1a7373aa9cb,
	0x3feedea64c123422, 0x3feece086061892d, 0x3feebfdad5362a27, 0x3feeb42b569d4f82, 0x3feeab07dd485429,
	0x3feea47eb03a5585, 0x3feea09e667f3bcd, 0x3fee9f75e8ec5f74, 0x3feea11473eb0187, 0x3feea589994cce13,
	0x3feeace5422aa0db, 0x3feeb737b0cdc5e5, 0x3feec49182a3f090, 0x3feed503b23e255d, 0x3feee89f995ad3ad,
	0x3feeff76f2fb5e47, 0x3fef199bdd85529c, 0x3fef3720dcef9069, 0x3fef5818dcfba487, 0x3fef7c97337b9b5f,
	0x3fefa4afa2a490da, 0x3fefd0765b6e4540,
};

// The two tables in LDS (512 bytes per block, copied by fillPowTab at the start of every ray kernel): the lookups are per lane and
// DEPENDENT (the exp2 entry's index comes out of the logarithm) -- from global memory two round trips of a microsecond or two in
// every Phong / mirror / glass shading step, the longest part of a trace round of a scene of spheres (RTX_DBG=3: 12 000 of a
// round's 17 000 cycles).
__shared__ unsigned long long powTab[64];      // [0, 32): kLog2Tab as bits, [32, 64): kExp2Tab
__device__ __forceinline__ void fillPowTab()
{
	if (threadIdx.x < 32) powTab[threadIdx.x] = (unsigned long long)__double_as_longlong(kLog2Tab[threadIdx.x]);
	else if (threadIdx.x < 64) powTab[threadIdx.x] = kExp2Tab[threadIdx.x - 32];
	__syncthreads();
}

__device__ __forceinline__ int powfCheckInt(uint32_t iy)
{
	int e = iy >> 23 & 0xff;
	if (e < 0x7f) return 0;
	if (e > 0x7f + 23) return 2;
	if (iy & ((1u << (0x7f + 23 - e)) - 1)) return 0;
	if (iy & (1u << (0x7f + 23 - e))) return 1;
	return 2;
}
__device__ __forceinline__ bool zeroInfNan(uint32_t i) { return 2 * i - 1 >= 2u * 0x7f800000 - 1; }

__device__ __noinline__ float powfRef(float x, float y)
{
	uint32_t signBias = 0;
	uint32_t ix = __float_as_uint(x), iy = __float_as_uint(y);
	if (ix - 0x00800000 >= 0x7f800000 - 0x00800000 || zeroInfNan(iy)) {
		if (zeroInfNan(iy)) {
			if (2 * iy == 0) return 1.0f;
			if (ix == 0x3f800000) return 1.0f;
			if (2 * ix > 2u * 0x7f800000 || 2 * iy > 2u * 0x7f800000) return x + y;
			if (2 * ix == 2 * 0x3f800000) return 1.0f;
			if ((2 * ix < 2 * 0x3f800000) == !(iy & 0x80000000)) return 0.0f;
			return y * y;
		}
		if (zeroInfNan(ix)) {
			float x2 = x * x;
			if ((ix & 0x80000000) && powfCheckInt(iy) == 1) x2 = -x2;
			return (iy & 0x80000000) ? 1 / x2 : x2;
		}
		if (ix & 0x80000000) {
			int yint = powfCheckInt(iy);
			if (yint == 0) return __uint_as_float(0x7fc00000u);
			if (yint == 1) signBias = 1u << 16;
			ix &= 0x7fffffff;
		}
		if (ix < 0x00800000) {
			ix = __float_as_uint(x * 0x1p23f);
			ix &= 0x7fffffff;
			ix -= 23 << 23;
		}
	}
	uint32_t tmp = ix - 0x3f330000;
	int i = (tmp >> 19) % 16;
	uint32_t top = tmp & 0xff800000;
	uint32_t iz = ix - top;
	int k = (int32_t)top >> 23;
	double invc = __longlong_as_double((long long)powTab[2 * i]), logc = __longlong_as_double((long long)powTab[2 * i + 1]);
	double z = (double)__uint_as_float(iz);
	double r = __builtin_fma(z, invc, -1.0);
	double y0 = logc + (double)k;
	double r2 = r * r;
	double yy = __builtin_fma(0x1.27616c9496e0bp-2, r, -0x1.71969a075c67ap-2);
	double p = __builtin_fma(0x1.ec70a6ca7baddp-2, r, -0x1.7154748bef6c8p-1);
	double r4 = r2 * r2;
	double q = __builtin_fma(0x1.71547652ab82bp+0, r, y0);
	q = __builtin_fma(p, r2, q);
	double logx = __builtin_fma(yy, r4, q);
	double ylogx = (double)y * logx;
	if ((__double_as_longlong(ylogx) >> 47 & 0xffff) >= (0x405f800000000000LL >> 47)) {
		if (ylogx > 0x1.fffffffd1d571p+6) return signBias ? -__builtin_inff() : __builtin_inff();
		if (ylogx <= -150.0) return signBias ? -0.0f : 0.0f;
		if (ylogx < -149.0) return signBias ? -0x1p-149f : 0x1p-149f;
	}
	double kd = ylogx + 0x1.8p+47;
	uint64_t ki = (uint64_t)__double_as_longlong(kd);
	kd -= 0x1.8p+47;
	double rr = ylogx - kd;
	uint64_t t = powTab[32 + ki % 32];
	t += (ki + signBias) << (52 - 5);
	double s = __longlong_as_double((long long)t);
	double zz = __builtin_fma(0x1.c6af84b912394p-5, rr, 0x1.ebfce50fac4f3p-3);
	double rr2 = rr * rr;
	double yv = __builtin_fma(0x1.62e42ff0c52d6p-1, rr, 1.0);
	yv = __builtin_fma(zz, rr2, yv);
	yv = yv * s;
	return (float)yv;
}

// ------------------------------------------------------------------------------------------------
// shading helpers (scene.cpp:672-722, 381-442; lights.cpp:18-38)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ V3 reflectDir(V3 d, V3 n) { float k = 2 * dot(d, n); return d - n * k; }   // scene.cpp:674

__device__ __forceinline__ V3 refractDir(V3 d, V3 n, float ior)      // scene.cpp:677-696
{
	float n1 = 1, n2 = ior;
	float cosi = clampRef(-1, 1, dot(d, n));
	V3 mn = n;
	if (cosi < 0) cosi = -cosi;
	else { float t = n1; n1 = n2; n2 = t; mn = -n; }
	float rri = n1 / n2;
	float k = 1 - rri * rri * (1 - cosi * cosi);
	if (k < 0) return mk(0, 0, 0);
	return d * rri + mn * (rri * cosi - __builtin_sqrtf(k));
}

__device__ __forceinline__ float fresnelKr(V3 d, V3 n, float ior)    // scene.cpp:698-722
{
	float n1 = 1, n2 = ior;
	float cosi = clampRef(-1, 1, dot(d, n));
	if (cosi > 0) { float t = n1; n1 = n2; n2 = t; }
	float sint = n1 / n2 * __builtin_sqrtf(fmaxRef(0.f, 1 - cosi * cosi));
	if (sint >= 1) return 1;
	float cost = __builtin_sqrtf(fmaxRef(0.f, 1 - sint * sint));
	cosi = fabsf(cosi);
	float rs = ((n2 * cosi) - (n1 * cost)) / ((n2 * cosi) + (n1 * cost));
	float rp = ((n1 * cosi) - (n2 * cost)) / ((n1 * cosi) + (n2 * cost));
	return (rs * rs + rp * rp) / 2;
}

__device__ __forceinline__ int toPixel(float v, int mx)               // scene.cpp:387-392
{
	int val = (int)((v + 1.0f) / 2.0f * mx);
	if (val >= mx) val = mx - 1;
	if (val < 0) val = 0;            // hardening only (NaN / degenerate directions index out of bounds in the reference)
	return val;
}
__device__ __forceinline__ V3 load3(const float* p) { return mk(p[0], p[1], p[2]); }
// A pointer that was itself loaded from memory (mesh arrays, texture maps, skybox faces, light sample points) has no
// known address space: the compiler reads through it with flat_load, which counts against the LDS / scalar counter as
// well as the vector-memory one.  These all point to device memory.
typedef const __attribute__((address_space(1))) float* GlobalFloats;
__device__ __forceinline__ GlobalFloats inGlobal(const float* p) { return (GlobalFloats)(uintptr_t)p; }
__device__ __forceinline__ V3 load3(GlobalFloats p) { return mk(p[0], p[1], p[2]); }

// (takes the few fields it needs by value: a kernel-argument struct whose address escapes into a call is copied to scratch)
__device__ __noinline__ V3 skyFetch(const float* const* sky, int W, int H, V3 dir)           // scene.cpp:394-441
{
	float ax = fabsf(dir.x), ay = fabsf(dir.y), az = fabsf(dir.z);
	float m = fmaxRef(ax, fmaxRef(ay, az));
	V3 a; int face, i, j;
	if (m == az) {
		if (dir.z < 0) { a = dir * (1 / -dir.z); face = 1; i = toPixel(a.y, H); j = toPixel(a.x, W); }
		else { a = dir * (1 / dir.z); face = 3; i = toPixel(a.y, H); j = toPixel(-a.x, W); }
	}
	else if (m == ax) {
		if (dir.x < 0) { a = dir * (1 / -dir.x); face = 0; i = toPixel(a.y, H); j = toPixel(-a.z, W); }
		else { a = dir * (1 / dir.x); face = 2; i = toPixel(a.y, H); j = toPixel(a.z, W); }
	}
	else {
		if (dir.y < 0) { a = dir * (1 / -dir.y); face = 5; i = toPixel(a.z, H); j = toPixel(a.x, W); }
		else { a = dir * (1 / dir.y); face = 4; i = toPixel(a.z, H); j = toPixel(a.x, W); }
	}
	return load3(inGlobal(sky[face]) + ((size_t)i * W + j) * 3);
}

__device__ __forceinline__ V3 skyColor(const Params& P, V3 dir)           // scene.cpp:381-442
{
	if (!(P.view.flags & 2u)) return mk(P.view.bg[0], P.view.bg[1], P.view.bg[2]);
	return skyFetch(P.sky, (int)P.skyW, (int)P.skyH, dir);
}

// (int)(dim * coord), clamped on the high side like the reference (objects.cpp:144-147, 156-159).  The low-side clamp is
// hardening only: negative / NaN coordinates are out-of-bounds reads (UB) in the reference.
__device__ __forceinline__ int texel(int dim, float coord) { int v = (int)(dim * coord); if (v >= dim) v = dim - 1; if (v < 0) v = 0; return v; }

// 4*M_PI*len2/1000 attenuation in fp64 (lights.cpp:35; scene.cpp:796,832,875,925)
__device__ __forceinline__ float attenuation(float intensity, float l2)
{
	return fminRef(1.0f, (float)((double)intensity / (4 * 3.14159265358979323846 * (double)l2 / 1000)));
}

} // namespace
