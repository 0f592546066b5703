// The record formulas of a mesh's flatten, written once for the two flattens that must agree bit for bit: the host's (flattenMesh and
// uploadMeshGeometry: rtx_scene_create, rtx_mesh_flatten_probe) and the device's (the kernels of rtx_flatten.hip: rtx_scene_update_mesh), both in
// rtx_flatten.hip.  Each keeps its own traversal; every value it stores comes from here: a leaf reference, a node record and its regular test, the
// aggregate of a subtree, the box and plane records of a wide-node slot, the whole mesh's vmax, the leaf boxes of the cost estimate, the edge term of
// the bundle split, the rounding of Pgen (rtx_source.hip rounds a triangle's the same way).
//
// A prune record a few ulps too small makes the wide walk skip triangles a ray does hit, so the margins here are part of the correctness contract:
// (1 + 2^-20), + 2^-24 big + 1e-37, |w| 2^-22, the 1e-30 scale cut, the "empty" (h = -1e30) and "never pruned" (h = P = inf) records.  Every
// aggregate is a min, a max or an AND in fp64, merged left child first and a leaf's references in order; min(a, b) = b < a ? b : a and
// max(a, b) = a < b ? b : a (std::min / std::max, NaN handling included); nothing may be contracted into an FMA.
// tests/test_flatten_records_cpu.py pins the records to digests taken before the formulas moved here; tests/test_host_cpu.py and
// tests/test_adversarial_meshes_cpu.py check what they bound; tests/test_gpu_adversarial_meshes.py, test_gpu_move_objects.py, test_gpu_objects_edit.py
// and test_gpu_deform.py compare the device's flatten with the host's.  Plain C++: no HIP call, no rtx_scene, no globals.
#pragma once
#include <cmath>
#include <cstdint>

#include "rtx_device.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define RTX_FLAT_HD __host__ __device__ inline
#else
#define RTX_FLAT_HD inline
#endif

namespace rtxflat {

using rtxd::Node; using rtxd::PlaneRec; using rtxd::PruneRec; using rtxd::RefA; using rtxd::RefB; using rtxd::RefC;

constexpr uint32_t kNone = 0xffffffffu;      // no node: behind an unused slot, above the root

template <typename T> RTX_FLAT_HD T minOf(T a, T b) { return b < a ? b : a; }
template <typename T> RTX_FLAT_HD T maxOf(T a, T b) { return a < b ? b : a; }

// (v0, e1, e2, tri) of a leaf reference to triangle `tri` with corners p[0..8] (objects.cpp:70-71: v0v1 = v1 - v0, v0v2 = v2 - v0)
RTX_FLAT_HD void makeRef(const float* p, uint32_t tri, RefA& a, RefB& b, RefC& c)
{
	a.v0x = p[0]; a.v0y = p[1]; a.v0z = p[2]; a.tri = tri;
	b.e1x = p[3] - p[0]; b.e1y = p[4] - p[1]; b.e1z = p[5] - p[2];
	b.e2x = p[6] - p[0]; c.e2y = p[7] - p[1]; c.e2z = p[8] - p[2];
}

// The 32-byte record of a node from the builder's arrays (box lo[3] hi[3]; leafCount < 0: inner, with its skip index).  False when the box is not
// regular (a bound of 1e30 or beyond, a NaN, lo > hi): such a mesh gets no wide tree.
RTX_FLAT_HD bool nodeRecord(const float* box, int32_t skip, int32_t leafBegin, int32_t leafCount, Node& nd)
{
	bool regular = true;
	for (int c = 0; c < 3; c++) {
		nd.b[2 * c] = box[c]; nd.b[2 * c + 1] = box[3 + c];
		if (!(std::fabs(nd.b[2 * c]) < 1e30f && std::fabs(nd.b[2 * c + 1]) < 1e30f && nd.b[2 * c] <= nd.b[2 * c + 1])) regular = false;
	}
	if (leafCount < 0) { nd.link = skip; nd.first = 0; }
	else { nd.link = ~leafCount; nd.first = leafBegin; }
	return regular;
}

// What the prune records need of a subtree: the true box of its triangles as the exact test sees them (v0, v0 + e1, v0 + e2 with the fp32
// differences of makeRef), the largest |e1|_1 |e2|_1, the box of the scaled plane normals q = (e2 x e1) / (|e1|_1 |e2|_1) and the range of the
// offsets v0 . q (planes = 0: some triangle's scale underflowed, no plane bound), the range [rb, re) of leaf references that covers it.
struct Agg { double lo[3], hi[3], ps, qlo[3], qhi[3], wlo, whi; uint32_t planes, rb, re, pad; };

RTX_FLAT_HD void aggInit(Agg& a)
{
	for (int k = 0; k < 3; k++) { a.lo[k] = a.qlo[k] = INFINITY; a.hi[k] = a.qhi[k] = -INFINITY; }
	a.ps = 0; a.wlo = INFINITY; a.whi = -INFINITY; a.planes = 1; a.rb = 0xffffffffu; a.re = 0; a.pad = 0;
}

RTX_FLAT_HD void aggAdd(Agg& a, const RefA& ra, const RefB& rb, const RefC& rc)
{
	const double v0[3] = { ra.v0x, ra.v0y, ra.v0z }, e1[3] = { rb.e1x, rb.e1y, rb.e1z }, e2[3] = { rb.e2x, rc.e2y, rc.e2z };
	double s1 = 0, s2 = 0;
	for (int k = 0; k < 3; k++) {
		const double x1 = v0[k] + e1[k], x2 = v0[k] + e2[k];
		a.lo[k] = minOf(a.lo[k], minOf(v0[k], minOf(x1, x2)));
		a.hi[k] = maxOf(a.hi[k], maxOf(v0[k], maxOf(x1, x2)));
		s1 += std::fabs(e1[k]); s2 += std::fabs(e2[k]);
	}
	a.ps = maxOf(a.ps, s1 * s2);
	// A triangle with a zero edge can never be accepted (det_c = 0 exactly) and bounds nothing; one whose scale underflows spoils the plane bound.
	if (s1 == 0 || s2 == 0) return;
	const double sc = s1 * s2;
	if (!(sc > 1e-30) || !std::isfinite(sc)) { a.planes = 0; return; }
	const double mq[3] = { (e2[1] * e1[2] - e2[2] * e1[1]) / sc, (e2[2] * e1[0] - e2[0] * e1[2]) / sc, (e2[0] * e1[1] - e2[1] * e1[0]) / sc };
	double w = 0;
	for (int k = 0; k < 3; k++) { a.qlo[k] = minOf(a.qlo[k], mq[k]); a.qhi[k] = maxOf(a.qhi[k], mq[k]); w += v0[k] * mq[k]; }
	a.wlo = minOf(a.wlo, w); a.whi = maxOf(a.whi, w);
}

RTX_FLAT_HD void aggMerge(Agg& a, const Agg& b)
{
	a.rb = minOf(a.rb, b.rb); a.re = maxOf(a.re, b.re);
	for (int k = 0; k < 3; k++) {
		a.lo[k] = minOf(a.lo[k], b.lo[k]); a.hi[k] = maxOf(a.hi[k], b.hi[k]);
		a.qlo[k] = minOf(a.qlo[k], b.qlo[k]); a.qhi[k] = maxOf(a.qhi[k], b.qhi[k]);
	}
	a.ps = maxOf(a.ps, b.ps); a.wlo = minOf(a.wlo, b.wlo); a.whi = maxOf(a.whi, b.whi);
	a.planes = (a.planes && b.planes) ? 1u : 0u;
}

// the aggregate of a leaf: its `count` references from `begin`, in order
RTX_FLAT_HD void aggLeaf(Agg& a, uint32_t begin, uint32_t count, const uint32_t* refs, const float* pos)
{
	aggInit(a);
	if (count) { a.rb = begin; a.re = begin + count; }
	for (uint32_t r = begin; r < begin + count; r++) {
		RefA ra; RefB rb; RefC rc;
		makeRef(pos + (size_t)refs[r] * 9, refs[r], ra, rb, rc);
		aggAdd(a, ra, rb, rc);
	}
}

// the aggregate of an inner node: left child, then right child
RTX_FLAT_HD void aggInner(Agg& a, const Agg& left, const Agg& right)
{
	aggInit(a);
	aggMerge(a, left);
	aggMerge(a, right);
}

// |e1|_1 |e2|_1 as a record stores it, rounded up (a slot's P and Pgen; rtx_source.hip: a triangle's)
RTX_FLAT_HD float roundPgen(double ps) { return (float)(ps * (1.0 + 0x1p-20) + 1e-37); }

// The box record of an aggregate: "empty" (nothing can meet it) without triangles, "never pruned" when something is not finite; else
// [c - h, c + h] really contains [lo, hi] (c is rounded, h rounded up).
RTX_FLAT_HD void boxRecord(const Agg& a, PruneRec& pr)
{
	for (int c = 0; c < 3; c++) pr.c[c] = 0.0f;
	pr.P = 0.0f; pr.Pgen = 0.0f;
	pr.h[0] = pr.h[1] = pr.h[2] = -1e30f;
	if (!(a.lo[0] <= a.hi[0])) return;
	bool finite = std::isfinite(a.ps);
	for (int c = 0; c < 3; c++) finite = finite && std::isfinite(a.lo[c]) && std::isfinite(a.hi[c]);
	if (!finite) { pr.h[0] = pr.h[1] = pr.h[2] = INFINITY; pr.P = pr.Pgen = INFINITY; return; }
	for (int c = 0; c < 3; c++) {
		const double mid = 0.5 * (a.lo[c] + a.hi[c]), big = maxOf(std::fabs(a.lo[c]), std::fabs(a.hi[c]));
		pr.c[c] = (float)mid;
		pr.h[c] = (float)((0.5 * (a.hi[c] - a.lo[c]) + std::fabs((double)pr.c[c] - mid)) * (1.0 + 0x1p-20) + 0x1p-24 * big + 1e-37);
	}
	pr.P = pr.Pgen = roundPgen(a.ps);
}

// The records of one wide-node slot and the range of leaf references below it, from the aggregate of the node behind it (nullptr: an unused
// slot -- an empty box record).  Without a plane bound the plane record can never be "dead" whatever the bundle: q = 0 +- 0 (max dir . q + 2 kd
// >= 0), offsets in [-inf, +inf] (planeAlive's three rejections are all false for it; pruneEval8 has no separate "usable" test).
RTX_FLAT_HD void slotRecords(const Agg* node, PruneRec& pr, PlaneRec& pl, uint32_t range[2])
{
	for (int c = 0; c < 3; c++) { pr.c[c] = 0.0f; pl.qc[c] = 0.0f; pl.qr[c] = 0.0f; }
	pr.P = pr.Pgen = 0.0f;
	pr.h[0] = pr.h[1] = pr.h[2] = -1e30f;
	pl.wlo = -INFINITY; pl.whi = INFINITY;
	range[0] = range[1] = 0;
	if (!node) return;
	const Agg& a = *node;
	if (a.rb < a.re) { range[0] = a.rb; range[1] = a.re; }
	boxRecord(a, pr);
	if (!(a.lo[0] <= a.hi[0]) || !std::isfinite(pr.P)) return;
	if (a.planes && a.wlo <= a.whi && std::isfinite(a.wlo) && std::isfinite(a.whi)) {
		for (int c = 0; c < 3; c++) {
			const double mid = 0.5 * (a.qlo[c] + a.qhi[c]);
			pl.qc[c] = (float)mid;
			pl.qr[c] = (float)((0.5 * (a.qhi[c] - a.qlo[c]) + std::fabs((double)pl.qc[c] - mid)) * (1.0 + 0x1p-20) + 0x1p-24);
		}
		pl.wlo = (float)(a.wlo - (std::fabs(a.wlo) * 0x1p-22 + 1e-37)); pl.whi = (float)(a.whi + (std::fabs(a.whi) * 0x1p-22 + 1e-37));
	}
}

// the largest coordinate of the whole mesh, from the root's aggregate (2^40 and beyond, or not finite: nothing is pruned)
RTX_FLAT_HD float meshVmax(const Agg& root)
{
	float v = 0.0f;
	for (int c = 0; c < 3; c++) v = maxOf(v, (float)maxOf(std::fabs(root.lo[c]), std::fabs(root.hi[c])));
	return v;
}

// For the first-frame cost estimate: the TRUE box of a leaf's triangles and its reference count (lo[3], hi[3], count, 0).  False for a leaf
// without references or with a box that is not finite: it has no entry.
RTX_FLAT_HD bool leafBox(int32_t begin, int32_t count, const uint32_t* refs, const float* pos, float box8[8])
{
	if (count <= 0) return false;
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (uint32_t r = (uint32_t)begin; r < (uint32_t)(begin + count); r++) {
		const float* p = pos + (size_t)refs[r] * 9;
		for (int v = 0; v < 9; v++) { lo[v % 3] = minOf(lo[v % 3], p[v]); hi[v % 3] = maxOf(hi[v % 3], p[v]); }
	}
	if (!(std::isfinite(lo[0] + lo[1] + lo[2] + hi[0] + hi[1] + hi[2]))) return false;
	for (int c = 0; c < 3; c++) { box8[c] = lo[c]; box8[3 + c] = hi[c]; }
	box8[6] = (float)count; box8[7] = 0.0f;
	return true;
}

// The bundle split's mean edge length (performance only): every nRefs / 65536-th reference is sampled; one adds its two edges to sum and cnt.
RTX_FLAT_HD uint32_t edgeStride(uint32_t nRefs) { return nRefs > 65536 ? nRefs / 65536 : 1; }
RTX_FLAT_HD void edgeTerm(const RefB& b, const RefC& c, double& sum, uint32_t& cnt)
{
	const double l1 = std::sqrt((double)b.e1x * b.e1x + (double)b.e1y * b.e1y + (double)b.e1z * b.e1z);
	const double l2 = std::sqrt((double)b.e2x * b.e2x + (double)c.e2y * c.e2y + (double)c.e2z * c.e2z);
	if (std::isfinite(l1 + l2)) { sum += l1 + l2; cnt += 2; }
}

} // namespace rtxflat
