// The flatten of a mesh on the device (rtx_scene_update_mesh): what flattenMesh and uploadMeshGeometry (rtx_api.hip) derive on the host
// from a tree and its triangles, computed from the tree the device builder left in device memory (rtx_bvh) and the caller's device
// triangles, bit for bit.  Part of rtx_api.hip's translation unit (included by rtx_edit.hip).
//
// The host builds the wide tree by popping wide nodes in pre-order and giving each popped node's inner slots one block of indices.  Wide
// pre-order is the binary pre-order restricted to the wide roots (the inner binary nodes at depth 0 mod 3), so a wide node's first child
// is 1 + the exclusive scan, over the wide roots in binary order, of their numbers of inner slots.  Every aggregate of the prune records
// is a min, a max or an AND in fp64 (-ffp-contract=off), merged in the host's order per node (left child, then right child; a leaf's
// references in order), so a bottom-up pass by levels gives the host's bits.

namespace rtxflat {

constexpr uint32_t kNone = 0xffffffffu;

// the host's std::min / std::max (min(a, b) = b < a ? b : a; max(a, b) = a < b ? b : a), NaN handling included
__device__ inline double dmin(double a, double b) { return b < a ? b : a; }
__device__ inline double dmax(double a, double b) { return a < b ? b : a; }
__device__ inline float fmin_(float a, float b) { return b < a ? b : a; }
__device__ inline float fmax_(float a, float b) { return a < b ? b : a; }

struct Agg { double lo[3], hi[3], ps, qlo[3], qhi[3], wlo, whi; uint32_t planes, rb, re, pad; };

// control words: [0] bit 0 a box is irregular, bit 1 a box is not inside its parent's; [1] deepest wide level; [2] wide roots; [3] deepest
// binary level; [4] leaf boxes; [8..13] the root box; [16..23] the whole mesh's prune record; [24] vmax; [32..35] the edge sum (double) and count
constexpr int kCtlWords = 64;

// node records (rtx_api.hip flattenMesh), parents, the regular-box flag, the root box
__global__ void __launch_bounds__(256) nodesKernel(const float* bounds, const int32_t* skip, const int32_t* lb, const int32_t* lc, uint32_t n,
                                                   Node* nodes, uint32_t* parent, uint32_t* ctl)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	Node nd;
	bool regular = true;
	for (int c = 0; c < 3; c++) {
		nd.b[2 * c] = bounds[(size_t)i * 6 + c]; nd.b[2 * c + 1] = bounds[(size_t)i * 6 + 3 + c];
		if (!(fabsf(nd.b[2 * c]) < 1e30f && fabsf(nd.b[2 * c + 1]) < 1e30f && nd.b[2 * c] <= nd.b[2 * c + 1])) regular = false;
	}
	if (!regular) atomicOr(&ctl[0], 1u);
	if (lc[i] < 0) {
		nd.link = skip[i]; nd.first = 0;
		if (i + 1 < n) {
			parent[i + 1] = i;
			const uint32_t right = lc[i + 1] >= 0 ? i + 2 : (uint32_t)skip[i + 1];
			if (right < n) parent[right] = i;
		}
	}
	else { nd.link = ~lc[i]; nd.first = lb[i]; }
	nodes[i] = nd;
	if (i == 0) {
		parent[0] = kNone;
		for (int c = 0; c < 6; c++) reinterpret_cast<float*>(ctl)[8 + c] = bounds[c];
	}
}

__device__ inline bool isLeaf(const Node* nodes, uint32_t i) { return nodes[i].link < 0; }
__device__ inline uint32_t rightOf(const Node* nodes, uint32_t i) { return isLeaf(nodes, i + 1) ? i + 2 : (uint32_t)nodes[i + 1].link; }

// depth of every node (root 0), the wide roots, the nested check, the deepest levels
__global__ void __launch_bounds__(256) depthKernel(const Node* nodes, const uint32_t* parent, uint32_t n, uint32_t* depth, uint32_t* isRoot, uint32_t* ctl)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint32_t d = 0;
	for (uint32_t p = parent[i]; p != kNone && d < n; p = parent[p]) d++;
	depth[i] = d;
	const bool root = !isLeaf(nodes, i) && d % 3 == 0;
	isRoot[i] = root ? 1u : 0u;
	atomicMax(&ctl[3], d);
	if (root) { atomicMax(&ctl[1], d / 3 + 1); atomicAdd(&ctl[2], 1u); }
	if (i > 0 && parent[i] == kNone) atomicOr(&ctl[0], 2u);      // (not part of the tree: no wide form)
	else if (i > 0) {
		const Node& c = nodes[i];
		const Node& q = nodes[parent[i]];
		for (int k = 0; k < 3; k++)
			if (!(c.b[2 * k] >= q.b[2 * k] && c.b[2 * k + 1] <= q.b[2 * k + 1])) { atomicOr(&ctl[0], 2u); break; }
	}
}

// the slots of wide root w: the descendants kWideLevels levels below, left to right (a leaf on the way takes a slot itself)
__device__ inline int gatherSlots(const Node* nodes, uint32_t w, uint32_t slots[kWideSlots])
{
	int ns = 0;
	const uint32_t k1[2] = { w + 1, rightOf(nodes, w) };
	for (uint32_t a : k1) {
		if (isLeaf(nodes, a)) { slots[ns++] = a; continue; }
		const uint32_t k2[2] = { a + 1, rightOf(nodes, a) };
		for (uint32_t b : k2) {
			if (isLeaf(nodes, b)) { slots[ns++] = b; continue; }
			slots[ns++] = b + 1; slots[ns++] = rightOf(nodes, b);
		}
	}
	return ns;
}

// per wide root (binary order = wide pre-order): its number of inner slots, at its rank among the wide roots
__global__ void __launch_bounds__(256) innerCountKernel(const Node* nodes, uint32_t n, const uint32_t* isRoot, const uint32_t* rank, uint32_t* count)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !isRoot[i]) return;
	uint32_t slots[kWideSlots];
	const int ns = gatherSlots(nodes, i, slots);
	uint32_t c = 0;
	for (int k = 0; k < ns; k++) c += isLeaf(nodes, slots[k]) ? 0u : 1u;
	count[rank[i]] = c;
}

// the wide index of every inner slot: its parent's block (1 + the scan of the counts) in slot order
__global__ void __launch_bounds__(256) childIndexKernel(const Node* nodes, uint32_t n, const uint32_t* isRoot, const uint32_t* rank, const uint32_t* first,
                                                        uint32_t* wideOf)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !isRoot[i]) return;
	uint32_t slots[kWideSlots];
	const int ns = gatherSlots(nodes, i, slots);
	uint32_t next = 1 + first[rank[i]];
	for (int k = 0; k < ns; k++)
		if (!isLeaf(nodes, slots[k])) wideOf[slots[k]] = next++;
	if (i == 0) wideOf[0] = 0;
}

// the wide nodes: the slots' node records, an inner slot linking to its wide node + 1; the binary node behind every slot
__global__ void __launch_bounds__(256) wideKernel(const Node* nodes, uint32_t n, const uint32_t* isRoot, const uint32_t* wideOf, uint32_t nWide,
                                                  WideNode* wide, uint32_t* slotNode)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	uint32_t slots[kWideSlots];
	int ns;
	uint32_t wi;
	if (n == 1 || (i == 0 && isLeaf(nodes, 0))) { if (i != 0) return; slots[0] = 0; ns = 1; wi = 0; }      // (a leaf root: one wide node, one slot)
	else {
		if (!isRoot[i]) return;
		ns = gatherSlots(nodes, i, slots);
		wi = wideOf[i];
	}
	if (wi >= nWide) return;
	for (int k = 0; k < kWideSlots; k++) {
		Node sl;
		for (int c = 0; c < 6; c++) sl.b[c] = 0.0f;
		sl.link = 0; sl.first = 0;
		uint32_t sn = kNone;
		if (k < ns) {
			sn = slots[k];
			sl = nodes[sn];
			if (!isLeaf(nodes, sn)) { sl.link = (int32_t)wideOf[sn] + 1; sl.first = 0; }
		}
		wide[wi].slot[k] = sl;
		slotNode[(size_t)wi * kWideSlots + k] = sn;
	}
}

__device__ inline void aggInit(Agg& a)
{
	for (int k = 0; k < 3; k++) { a.lo[k] = a.qlo[k] = INFINITY; a.hi[k] = a.qhi[k] = -INFINITY; }
	a.ps = 0; a.wlo = INFINITY; a.whi = -INFINITY; a.planes = 1; a.rb = 0xffffffffu; a.re = 0; a.pad = 0;
}

// a leaf's aggregate over its references (flattenMesh); an inner node's is merged by mergeLevelKernel
__global__ void __launch_bounds__(256) leafAggKernel(const Node* nodes, uint32_t n, const uint32_t* refs, const float* pos, Agg* agg)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !isLeaf(nodes, i)) return;
	Agg a;
	aggInit(a);
	const uint32_t begin = (uint32_t)nodes[i].first, count = (uint32_t)~nodes[i].link;
	if (count) { a.rb = begin; a.re = begin + count; }
	for (uint32_t r = begin; r < begin + count; r++) {
		const float* p = pos + (size_t)refs[r] * 9;
		// (makeRef: v0 and the fp32 differences e1 = v1 - v0, e2 = v2 - v0)
		const float e1f[3] = { p[3] - p[0], p[4] - p[1], p[5] - p[2] }, e2f[3] = { p[6] - p[0], p[7] - p[1], p[8] - p[2] };
		const double v0[3] = { p[0], p[1], p[2] }, e1[3] = { e1f[0], e1f[1], e1f[2] }, e2[3] = { e2f[0], e2f[1], e2f[2] };
		double s1 = 0, s2 = 0;
		for (int k = 0; k < 3; k++) {
			const double x1 = v0[k] + e1[k], x2 = v0[k] + e2[k];
			a.lo[k] = dmin(a.lo[k], dmin(v0[k], dmin(x1, x2)));
			a.hi[k] = dmax(a.hi[k], dmax(v0[k], dmax(x1, x2)));
			s1 += fabs(e1[k]); s2 += fabs(e2[k]);
		}
		a.ps = dmax(a.ps, s1 * s2);
		if (s1 == 0 || s2 == 0) continue;
		const double sc = s1 * s2;
		if (!(sc > 1e-30) || !isfinite(sc)) { a.planes = 0; continue; }
		const double mq[3] = { (e2[1] * e1[2] - e2[2] * e1[1]) / sc, (e2[2] * e1[0] - e2[0] * e1[2]) / sc, (e2[0] * e1[1] - e2[1] * e1[0]) / sc };
		double w = 0;
		for (int k = 0; k < 3; k++) { a.qlo[k] = dmin(a.qlo[k], mq[k]); a.qhi[k] = dmax(a.qhi[k], mq[k]); w += v0[k] * mq[k]; }
		a.wlo = dmin(a.wlo, w); a.whi = dmax(a.whi, w);
	}
	agg[i] = a;
}

__device__ inline void aggMerge(Agg& a, const Agg& b)
{
	a.rb = b.rb < a.rb ? b.rb : a.rb; a.re = a.re < b.re ? b.re : a.re;
	for (int k = 0; k < 3; k++) {
		a.lo[k] = dmin(a.lo[k], b.lo[k]); a.hi[k] = dmax(a.hi[k], b.hi[k]);
		a.qlo[k] = dmin(a.qlo[k], b.qlo[k]); a.qhi[k] = dmax(a.qhi[k], b.qhi[k]);
	}
	a.ps = dmax(a.ps, b.ps); a.wlo = dmin(a.wlo, b.wlo); a.whi = dmax(a.whi, b.whi);
	a.planes = (a.planes && b.planes) ? 1u : 0u;
}

// the inner nodes of binary level d: left child, then right child (their levels are done)
__global__ void __launch_bounds__(256) mergeLevelKernel(const Node* nodes, uint32_t n, const uint32_t* depth, uint32_t d, Agg* agg)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || depth[i] != d || isLeaf(nodes, i)) return;
	Agg a;
	aggInit(a);
	aggMerge(a, agg[i + 1]);
	aggMerge(a, agg[rightOf(nodes, i)]);
	agg[i] = a;
}

__device__ inline void makeRec(const Agg& a, PruneRec& pr)
{
	for (int c = 0; c < 3; c++) pr.c[c] = 0.0f;
	pr.P = 0.0f; pr.Pgen = 0.0f;
	pr.h[0] = pr.h[1] = pr.h[2] = -1e30f;
	if (!(a.lo[0] <= a.hi[0])) return;
	bool finite = isfinite(a.ps);
	for (int c = 0; c < 3; c++) finite = finite && isfinite(a.lo[c]) && isfinite(a.hi[c]);
	if (!finite) { pr.h[0] = pr.h[1] = pr.h[2] = INFINITY; pr.P = pr.Pgen = INFINITY; return; }
	for (int c = 0; c < 3; c++) {
		const double mid = 0.5 * (a.lo[c] + a.hi[c]), big = dmax(fabs(a.lo[c]), fabs(a.hi[c]));
		pr.c[c] = (float)mid;
		pr.h[c] = (float)((0.5 * (a.hi[c] - a.lo[c]) + fabs((double)pr.c[c] - mid)) * (1.0 + 0x1p-20) + 0x1p-24 * big + 1e-37);
	}
	pr.P = pr.Pgen = (float)(a.ps * (1.0 + 0x1p-20) + 1e-37);
}

// one prune record pair and slot range per wide-node slot
__global__ void __launch_bounds__(256) pruneKernel(const uint32_t* slotNode, uint32_t nWide, const Agg* agg, PruneBlock* prune, uint32_t* slotRange)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= nWide * kWideSlots) return;
	const uint32_t wi = t / kWideSlots, k = t % kWideSlots;
	PruneRec pr;
	PlaneRec pl;
	for (int c = 0; c < 3; c++) { pr.c[c] = 0.0f; pl.qc[c] = 0.0f; pl.qr[c] = 0.0f; }
	pr.P = pr.Pgen = 0.0f;
	pr.h[0] = pr.h[1] = pr.h[2] = -1e30f;
	pl.wlo = -INFINITY; pl.whi = INFINITY;
	uint32_t rb = 0, re = 0;
	const uint32_t nd = slotNode[t];
	if (nd != kNone) {
		const Agg& a = agg[nd];
		if (a.rb < a.re) { rb = a.rb; re = a.re; }
		makeRec(a, pr);
		if ((a.lo[0] <= a.hi[0]) && isfinite(pr.P) && a.planes && a.wlo <= a.whi && isfinite(a.wlo) && isfinite(a.whi)) {
			for (int c = 0; c < 3; c++) {
				const double mid = 0.5 * (a.qlo[c] + a.qhi[c]);
				pl.qc[c] = (float)mid;
				pl.qr[c] = (float)((0.5 * (a.qhi[c] - a.qlo[c]) + fabs((double)pl.qc[c] - mid)) * (1.0 + 0x1p-20) + 0x1p-24);
			}
			pl.wlo = (float)(a.wlo - (fabs(a.wlo) * 0x1p-22 + 1e-37)); pl.whi = (float)(a.whi + (fabs(a.whi) * 0x1p-22 + 1e-37));
		}
	}
	prune[wi].box[k] = pr;
	prune[wi].plane[k] = pl;
	slotRange[(size_t)t * 2] = rb; slotRange[(size_t)t * 2 + 1] = re;
}

// the whole mesh's record and vmax (one thread)
__global__ void rootRecKernel(const Agg* agg, uint32_t* ctl)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	PruneRec pr;
	makeRec(agg[0], pr);
	memcpy(&ctl[16], &pr, sizeof(PruneRec));
	float v = 0.0f;
	for (int c = 0; c < 3; c++) v = fmax_(v, (float)dmax(fabs(agg[0].lo[c]), fabs(agg[0].hi[c])));
	memcpy(&ctl[24], &v, 4);
}

// the leaf references (makeRef), three parallel arrays
__global__ void __launch_bounds__(256) refsKernel(const uint32_t* refs, uint32_t nRefs, const float* pos, RefA* ra, RefB* rb, RefC* rc)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nRefs) return;
	const uint32_t t = refs[r];
	const float* p = pos + (size_t)t * 9;
	RefA a; RefB b; RefC c;
	a.v0x = p[0]; a.v0y = p[1]; a.v0z = p[2]; a.tri = t;
	b.e1x = p[3] - p[0]; b.e1y = p[4] - p[1]; b.e1z = p[5] - p[2];
	b.e2x = p[6] - p[0]; c.e2y = p[7] - p[1]; c.e2z = p[8] - p[2];
	ra[r] = a; rb[r] = b; rc[r] = c;
}

// the true box of every non-empty leaf's triangles (cost estimate): flag + box per node, then compacted in node order
__global__ void __launch_bounds__(256) leafBoxKernel(const Node* nodes, uint32_t n, const uint32_t* refs, const float* pos, float* box8, uint32_t* flag)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	flag[i] = 0;
	if (!isLeaf(nodes, i)) return;
	const int32_t count = ~nodes[i].link;
	if (count <= 0) return;
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (uint32_t r = (uint32_t)nodes[i].first; r < (uint32_t)(nodes[i].first + count); r++) {
		const float* p = pos + (size_t)refs[r] * 9;
		for (int v = 0; v < 9; v++) { lo[v % 3] = fmin_(lo[v % 3], p[v]); hi[v % 3] = fmax_(hi[v % 3], p[v]); }
	}
	if (!(isfinite(lo[0] + lo[1] + lo[2] + hi[0] + hi[1] + hi[2]))) return;
	const float b[8] = { lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], (float)count, 0.0f };
	for (int c = 0; c < 8; c++) box8[(size_t)i * 8 + c] = b[c];
	flag[i] = 1;
}

__global__ void __launch_bounds__(256) leafCompactKernel(const float* box8, const uint32_t* flag, const uint32_t* at, uint32_t n, float* out, uint32_t* ctl)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	if (i == n - 1) ctl[4] = at[i] + flag[i];
	if (!flag[i] || !out) return;
	for (int c = 0; c < 8; c++) out[(size_t)at[i] * 8 + c] = box8[(size_t)i * 8 + c];
}

// the mean edge length's sum over the sampled references (bundle splitting, performance only): one block, a fixed order
__global__ void __launch_bounds__(1024) edgeSumKernel(const RefB* rb, const RefC* rc, uint32_t nRefs, uint32_t stride, uint32_t* ctl)
{
	__shared__ double sum[1024];
	__shared__ uint32_t cnt[1024];
	double s = 0; uint32_t c = 0;
	for (size_t r = (size_t)threadIdx.x * stride; r < nRefs; r += (size_t)1024 * stride) {
		const RefB& b = rb[r]; const RefC& e = rc[r];
		const double l1 = sqrt((double)b.e1x * b.e1x + (double)b.e1y * b.e1y + (double)b.e1z * b.e1z);
		const double l2 = sqrt((double)b.e2x * b.e2x + (double)e.e2y * e.e2y + (double)e.e2z * e.e2z);
		if (isfinite(l1 + l2)) { s += l1 + l2; c += 2; }
	}
	sum[threadIdx.x] = s; cnt[threadIdx.x] = c;
	__syncthreads();
	for (uint32_t h = 512; h > 0; h >>= 1) {
		if (threadIdx.x < h) { sum[threadIdx.x] += sum[threadIdx.x + h]; cnt[threadIdx.x] += cnt[threadIdx.x + h]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) { memcpy(&ctl[32], &sum[0], 8); ctl[34] = cnt[0]; }
}

} // namespace rtxflat

namespace {

inline unsigned blocksFor(size_t n) { return n ? (unsigned)((n + 255) / 256) : 1u; }

// uploadMeshGeometry (rtx_api.hip) on the device: the tree of `b` (device builder) and the triangles at pos_dev (n_tris x 9, device) of mesh mi.
// Fills the same fields of dm, sm, leaves and the root box; every allocation that stays goes to `owned` (counted as scene data, but for the sources' scratch).
int deviceMeshGeometry(rtx_scene* s, const rtx_bvh* b, const float* pos_dev, uint32_t nTris, uint32_t mi, uint32_t nLights, DevBag& owned,
                       Mesh& dm, rtx_scene::SrcMesh& sm, rtx_scene::MeshLeaves& leaves, float bounds[6])
{
	using namespace rtxflat;
	const uint32_t n = b->nNodes, nRefs = b->nRefs;
	if (n == 0) return fail(RTX_ERR_DEVICE, "rtx_scene_update_mesh: the build left no nodes");
	hipStream_t st = nullptr;
	// scratch: one allocation kept by the scene, grown when a tree needs more
	const size_t scanTmp = n / 512 + 64;
	const size_t szCtl = kCtlWords * 4, szU = ((size_t)n * 4 + 255) & ~(size_t)255;
	const size_t szAgg = (size_t)n * sizeof(Agg), szBox = (size_t)n * 32, szTmp = scanTmp * 4;
	const size_t need = szCtl + 7 * szU + szAgg + szBox + szTmp;
	HIPCHK(s->flatScratch.reserve(need));
	char* scratch = s->flatScratch;
	uint32_t* ctl = (uint32_t*)scratch;
	uint32_t* parent = (uint32_t*)(scratch + szCtl);
	uint32_t* depth = (uint32_t*)(scratch + szCtl + szU);
	uint32_t* isRoot = (uint32_t*)(scratch + szCtl + 2 * szU);
	uint32_t* rank = (uint32_t*)(scratch + szCtl + 3 * szU);
	uint32_t* count = (uint32_t*)(scratch + szCtl + 4 * szU);      // (per wide root; then the leaf flags)
	uint32_t* wideOf = (uint32_t*)(scratch + szCtl + 5 * szU);
	uint32_t* at = (uint32_t*)(scratch + szCtl + 6 * szU);
	Agg* agg = (Agg*)(scratch + szCtl + 7 * szU);
	float* box8 = (float*)(scratch + szCtl + 7 * szU + szAgg);
	uint32_t* tmp = (uint32_t*)(scratch + szCtl + 7 * szU + szAgg + szBox);
	uint32_t launches = 0;

	// node records, depths, the checks that decide whether a wide tree exists (flattenMesh: boxes regular, nested, not too deep for the stack)
	Node* nodes = nullptr;
	int rc;
	HIPCHK(owned.alloc(&nodes, (size_t)n * sizeof(Node)));
	HIPCHK(hipMemsetAsync(ctl, 0, szCtl, st));
	HIPCHK(hipMemsetAsync(parent, 0xff, (size_t)n * 4, st));      // (kNone: a node no inner node names as its child)
	hipLaunchKernelGGL(nodesKernel, dim3(blocksFor(n)), dim3(256), 0, st, b->bounds, b->skip, b->leafBegin, b->leafCount, n, nodes, parent, ctl);
	hipLaunchKernelGGL(depthKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, (const uint32_t*)parent, n, depth, isRoot, ctl);
	uint32_t c0[16];
	HIPCHK(hipMemcpy(c0, ctl, sizeof(c0), hipMemcpyDeviceToHost));
	const bool boxesRegular = (c0[0] & 1u) == 0, nested = (c0[0] & 2u) == 0;
	const uint32_t depthMax = c0[1], nRoots = c0[2], maxDepth = c0[3];
	memcpy(bounds, &c0[8], 24);
	const bool hasWide = boxesRegular && nested && !((uint32_t)(kWideSlots - 1) * depthMax + 1 > (uint32_t)kWideStackEntries);
	const bool rootLeaf = nRoots == 0;
	const uint32_t nWide = hasWide ? (rootLeaf ? 1u : nRoots) : 0u;

	// the wide tree
	WideNode* wide = nullptr;
	DevArray<uint32_t> slotNode;      // (scratch: gone when this function returns)
	if (nWide) {
		HIPCHK(owned.alloc(&wide, (size_t)nWide * sizeof(WideNode)));
		HIPCHK(slotNode.reserve((size_t)nWide * kWideSlots));
	}
	if (nWide && !rootLeaf) {
		HIPCHK(hipMemcpyAsync(rank, isRoot, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
		if ((rc = scanExclusive(rank, n, tmp, st, launches))) return rc;
		hipLaunchKernelGGL(innerCountKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)isRoot, (const uint32_t*)rank, count);
		if ((rc = scanExclusive(count, nRoots, tmp, st, launches))) return rc;
		hipLaunchKernelGGL(childIndexKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)isRoot, (const uint32_t*)rank, (const uint32_t*)count, wideOf);
	}
	if (nWide) hipLaunchKernelGGL(wideKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)isRoot, (const uint32_t*)wideOf, nWide, wide, slotNode.get());
	dm.wide = wide; dm.nWide = nWide;

	// leaf references, padded by one wave
	RefA* ra = nullptr; RefB* rb = nullptr; RefC* rcr = nullptr;
	const size_t nPad = (size_t)nRefs + 64;
	HIPCHK(owned.alloc(&ra, nPad * sizeof(RefA))); HIPCHK(owned.alloc(&rb, nPad * sizeof(RefB))); HIPCHK(owned.alloc(&rcr, nPad * sizeof(RefC)));
	HIPCHK(hipMemsetAsync(ra, 0, nPad * sizeof(RefA), st)); HIPCHK(hipMemsetAsync(rb, 0, nPad * sizeof(RefB), st)); HIPCHK(hipMemsetAsync(rcr, 0, nPad * sizeof(RefC), st));
	if (nRefs) hipLaunchKernelGGL(refsKernel, dim3(blocksFor(nRefs)), dim3(256), 0, st, (const uint32_t*)b->refs, nRefs, pos_dev, ra, rb, rcr);

	// leaf boxes of the cost estimate
	uint32_t* flag = count;      // (the counts are done with)
	hipLaunchKernelGGL(leafBoxKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)b->refs, pos_dev, box8, flag);
	HIPCHK(hipMemcpyAsync(at, flag, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
	if ((rc = scanExclusive(at, n, tmp, st, launches))) return rc;

	// prune records (every aggregate bottom-up by levels), the whole mesh's record
	const bool pruneOn = nWide && s->knobs.prune;
	if (pruneOn) {
		hipLaunchKernelGGL(leafAggKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)b->refs, pos_dev, agg);
		for (uint32_t d = maxDepth + 1; d-- > 0;)
			hipLaunchKernelGGL(mergeLevelKernel, dim3(blocksFor(n)), dim3(256), 0, st, nodes, n, (const uint32_t*)depth, d, agg);
		hipLaunchKernelGGL(rootRecKernel, dim3(1), dim3(64), 0, st, (const Agg*)agg, ctl);
	}
	const uint32_t stride = nRefs > 65536 ? nRefs / 65536 : 1;
	hipLaunchKernelGGL(edgeSumKernel, dim3(1), dim3(1024), 0, st, (const RefB*)rb, (const RefC*)rcr, nRefs, stride, ctl);
	HIPCHK(hipGetLastError());
	// the leaf count first: the compacted boxes go straight into their own allocation
	hipLaunchKernelGGL(leafCompactKernel, dim3(blocksFor(n)), dim3(256), 0, st, (const float*)box8, (const uint32_t*)flag, (const uint32_t*)at, n, (float*)nullptr, ctl);
	uint32_t c1[kCtlWords];
	HIPCHK(hipMemcpy(c1, ctl, sizeof(c1), hipMemcpyDeviceToHost));
	const uint32_t nLeafBoxes = c1[4];
	float* lb = nullptr;
	if (nLeafBoxes) {
		HIPCHK(owned.alloc(&lb, (size_t)nLeafBoxes * 32));
		hipLaunchKernelGGL(leafCompactKernel, dim3(blocksFor(n)), dim3(256), 0, st, (const float*)box8, (const uint32_t*)flag, (const uint32_t*)at, n, lb, ctl);
	}
	leaves = { lb, nLeafBoxes };

	PruneRec rootRec;
	memset(&rootRec, 0, sizeof(rootRec));
	rootRec.h[0] = rootRec.h[1] = rootRec.h[2] = INFINITY; rootRec.P = INFINITY;
	float vmaxMesh = 0;
	if (pruneOn) { memcpy(&rootRec, &c1[16], sizeof(PruneRec)); memcpy(&vmaxMesh, &c1[24], 4); }

	// prune blocks: copy 0, then the source copies (equal to copy 0 until buildSources patches their P); the slots' reference ranges
	sm = rtx_scene::SrcMesh();
	dm.prune = nullptr;
	DevArray<uint32_t> slotRange;      // (scratch: copied where the source copies are used)
	if (pruneOn) {
		const uint32_t nCopies = s->knobs.sources ? 2u + std::min<uint32_t>(nLights, kMaxSrcLights) : 1u;
		PruneBlock* pb = nullptr;
		HIPCHK(owned.alloc(&pb, (size_t)nCopies * nWide * sizeof(PruneBlock)));
		HIPCHK(slotRange.reserve((size_t)nWide * kWideSlots * 2));
		hipLaunchKernelGGL(pruneKernel, dim3(blocksFor((size_t)nWide * kWideSlots)), dim3(256), 0, st, (const uint32_t*)slotNode, nWide, (const Agg*)agg, pb, slotRange.get());
		for (uint32_t c = 1; c < nCopies; c++) HIPCHK(hipMemcpyAsync(pb + (size_t)c * nWide, pb, (size_t)nWide * sizeof(PruneBlock), hipMemcpyDeviceToDevice, st));
		dm.prune = pb;
		sm.pruneAlloc = pb; sm.pruneWide = nWide;
		if (nCopies > 1) { sm.base = pb; sm.nWide = nWide; }
	}
	dm.vmax = vmaxMesh;
	dm.rootRec = rootRec;
	if (!(vmaxMesh < 0x1p40f)) { dm.prune = nullptr; dm.rootRec.h[0] = dm.rootRec.h[1] = dm.rootRec.h[2] = INFINITY; }      // (huge or non-finite coordinates: nothing is pruned)
	dm.nodes = nodes; dm.refA = ra; dm.refB = rb; dm.refC = rcr;
	if (sm.base && vmaxMesh < 0x1p40f && nRefs) {
		sm.nRefs = nRefs; sm.refA = ra; sm.refB = rb; sm.refC = rcr; sm.vmax = vmaxMesh; sm.meshIndex = mi;
		HIPCHK(owned.copyFrom(slotRange.get(), (size_t)nWide * kWideSlots * 2, &sm.slotRange));
		HIPCHK(owned.alloc(&sm.refP, ((size_t)nRefs + nRefs / 64 + 2) * sizeof(float), false));
		sm.blockP = sm.refP + nRefs;
	}
	else sm.base = nullptr;
	dm.nNodes = n; dm.nRefs = nRefs; dm.nTris = nTris; dm.boxesRegular = boxesRegular ? 1u : 0u;
	{
		// mean edge length of the sampled references -> width above which a ray bundle is split (performance only); the root box's sphere
		double sum;
		memcpy(&sum, &c1[32], 8);
		const uint32_t cnt = c1[34];
		const float factor = s->knobs.fatFactor;
		dm.fatRadius = cnt && factor > 0 ? (float)(sum / (double)cnt) * factor : INFINITY;
		double rad = 0;
		for (int c = 0; c < 3; c++) {
			const double lo = bounds[c], hi = bounds[3 + c];
			dm.centre[c] = (float)(0.5 * (lo + hi)); rad += 0.25 * (hi - lo) * (hi - lo);
		}
		dm.radius = (float)std::sqrt(rad);
		if (!std::isfinite(dm.radius)) { dm.radius = 0; dm.fatRadius = INFINITY; }
	}
	// (everything queued above has finished before the scratch goes)
	HIPCHK(hipStreamSynchronize(st));
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

} // namespace
