// The flatten of a mesh: from a tree and its triangles the 32-byte node records, the wide nodes, the prune blocks of their slots and the whole
// mesh's record, the leaf references, the leaf boxes of the cost estimate and the bundle-split terms.  Twice, with one result bit for bit:
// on the host (flattenMesh, uploadMeshGeometry: rtx_scene_create, the host form of rtx_scene_set_objects, rtx_mesh_flatten_probe) from the
// caller's arrays, and on the device (the kernels of namespace rtxflat, deviceMeshGeometry: rtx_scene_update_mesh, rtx_scene_deform_mesh, the
// device form of rtx_scene_set_objects) from the tree the device builder left in device memory (rtx_bvh.hip) and the caller's device triangles.
// Every record formula is written once, in rtx_flat_records.h; the two differ in their traversal only.  Part of rtx_api.hip's translation unit.
//
// The host builds the wide tree by popping wide nodes in pre-order and giving each popped node's inner slots one block of indices.  Wide
// pre-order is the binary pre-order restricted to the wide roots (the inner binary nodes at depth 0 mod 3), so on the device a wide node's
// first child is 1 + the exclusive scan, over the wide roots in binary order, of their numbers of inner slots.  Every aggregate of the prune
// records is a min, a max or an AND in fp64 (-ffp-contract=off), merged in one order per node (left child, then right child; a leaf's
// references in order), so the device's bottom-up pass by levels gives the bits of the host's bottom-up loop over the pre-order array.

#include "rtx_flat_records.h"

namespace {

// The host side of a mesh's upload, free of any device call (so that it can be checked without a GPU: rtx_mesh_flatten_probe):
// 32-byte node records, the tree with every other level skipped (when every box lies inside its parent's), and the prune
// blocks of its slots (DESIGN_HISTORY.md 3.1c).
struct FlatMesh {
	std::vector<Node> nodes;
	std::vector<WideNode> wide;
	std::vector<PruneBlock> prune;
	std::vector<uint32_t> slotRange;      // per wide-node slot: [begin, end) of leaf references covering the slot's subtree (rtx_source.hip)
	PruneRec rootRec;
	float vmaxMesh = 0;
	bool boxesRegular = true;
};

int flattenMesh(const rtx_mesh& m, bool pruneWanted, FlatMesh& out)
{
	using namespace rtxflat;
	if (!m.node_bounds || !m.node_skip || !m.leaf_begin || !m.leaf_count || (m.n_refs && !m.refs) || (m.n_tris && !m.tri_pos)) return fail(RTX_ERR_ARG, "mesh arrays missing");
	for (uint32_t r = 0; r < m.n_refs; r++)
		if (m.refs[r] >= m.n_tris) return fail(RTX_ERR_ARG, "leaf reference out of range");
	std::vector<Node> nodes(m.n_nodes);
	bool boxesRegular = true;
	for (uint32_t i = 0; i < m.n_nodes; i++) {
		if (m.leaf_count[i] < 0) {
			if (m.node_skip[i] <= (int32_t)i + 1 || m.node_skip[i] > (int32_t)m.n_nodes) return (fail(RTX_ERR_ARG, "bad skip index"));
		}
		else if ((uint32_t)m.leaf_begin[i] + (uint32_t)m.leaf_count[i] > m.n_refs) return (fail(RTX_ERR_ARG, "leaf range out of bounds"));
		if (!nodeRecord(m.node_bounds + (size_t)i * 6, m.node_skip[i], m.leaf_begin[i], m.leaf_count[i], nodes[i])) boxesRegular = false;
	}
	// every inner node has both children inside the array and inside its own subtree [i + 1, skip): the bottom-up passes below index
	// the right child of EVERY node, reachable from the root or not (rtx_mesh_flatten_probe feeds raw arrays in here)
	for (uint32_t i = 0; i < m.n_nodes; i++) {
		if (m.leaf_count[i] >= 0) continue;
		if (i + 1 >= m.n_nodes) return fail(RTX_ERR_ARG, "inner node without children");
		const uint32_t right = m.leaf_count[i + 1] >= 0 ? i + 2 : (uint32_t)m.node_skip[i + 1];
		if (right <= i + 1 || right >= (uint32_t)m.node_skip[i] || right >= m.n_nodes) return fail(RTX_ERR_ARG, "inner node whose right child lies outside its subtree");
	}
	// the tree with every other level skipped (rtxd::WideNode), when every box lies inside its parent's
	std::vector<WideNode> wide;
	std::vector<PruneBlock> prune;
	float vmaxMesh = 0;
	PruneRec rootRec;
	memset(&rootRec, 0, sizeof(rootRec));
	rootRec.h[0] = rootRec.h[1] = rootRec.h[2] = INFINITY; rootRec.P = INFINITY;
	std::vector<std::array<uint32_t, kWideSlots>> slotNode;      // binary node behind every wide-node slot
	std::array<uint32_t, kWideSlots> noSlots; noSlots.fill(kNone);
	if (boxesRegular && m.n_nodes > 0) {
		bool nested = true;
		uint32_t depthMax = 0;
		auto isLeaf = [&](uint32_t i) { return m.leaf_count[i] >= 0; };
		auto rightOf = [&](uint32_t i) { return isLeaf(i + 1) ? i + 2 : (uint32_t)m.node_skip[i + 1]; };     // children of inner node i: i + 1 and this
		auto inside = [&](uint32_t c, uint32_t p) {
			for (int k = 0; k < 3; k++)
				if (!(nodes[c].b[2 * k] >= nodes[p].b[2 * k] && nodes[c].b[2 * k + 1] <= nodes[p].b[2 * k + 1])) return false;
			return true;
		};
		// iterative pre-order construction: (binary node, index of its wide node, depth)
		struct Item { uint32_t node, wideIndex, depth; };
		std::vector<Item> todo;
		wide.emplace_back(); memset(&wide[0], 0, sizeof(WideNode));
		slotNode.push_back(noSlots);
		if (isLeaf(0)) { wide[0].slot[0] = nodes[0]; slotNode[0][0] = 0; }
		else todo.push_back({ 0u, 0u, 1u });
		while (!todo.empty() && nested) {
			const Item it = todo.back(); todo.pop_back();
			depthMax = std::max(depthMax, it.depth);
			// the slots: the descendants kWideLevels levels below the node, left to right (a leaf on the way takes a slot itself)
			uint32_t slots[kWideSlots]; int ns = 0;
			std::function<void(uint32_t, int)> gather = [&](uint32_t node, int levels) {
				if (!nested) return;
				const uint32_t kids[2] = { node + 1, rightOf(node) };
				for (uint32_t c : kids) {
					if (c >= m.n_nodes || !inside(c, node)) { nested = false; return; }
					if (isLeaf(c) || levels == 1) slots[ns++] = c;
					else gather(c, levels - 1);
					if (!nested) return;
				}
			};
			gather(it.node, kWideLevels);
			if (!nested) break;
			// children wide nodes are created in REVERSE so that the vector stays in pre-order when popped; indices are fixed here
			uint32_t childWide[kWideSlots] = { 0 };
			for (int k = 0; k < ns; k++)
				if (!isLeaf(slots[k])) { childWide[k] = (uint32_t)wide.size(); wide.emplace_back(); memset(&wide.back(), 0, sizeof(WideNode)); slotNode.push_back(noSlots); }
			for (int k = ns - 1; k >= 0; k--) {
				slotNode[it.wideIndex][k] = slots[k];
				Node sl = nodes[slots[k]];
				if (!isLeaf(slots[k])) { sl.link = (int32_t)childWide[k] + 1; sl.first = 0; todo.push_back({ slots[k], childWide[k], it.depth + 1 }); }
				wide[it.wideIndex].slot[k] = sl;
			}
		}
		// The walk's stack: while a node of wide level L is visited, every level above it has at most kWideSlots - 1 of its slots waiting and the node
		// pushes at most kWideSlots -- (kWideSlots - 1) (L - 1) + kWideSlots entries.  A tree deeper than the stack allows is walked in the binary form
		// (eight slots, 72 entries: ten wide levels = thirty binary ones need 71; the 250 000-triangle mesh has 27).
		if (!nested || (kWideSlots - 1) * depthMax + 1 > kWideStackEntries) wide.clear();      // (wideStack holds kWideStackEntries per wave)
		if (!wide.empty() && pruneWanted) {
			// Prune records (rtxd::PruneRec): per binary node the aggregate of the triangles its subtree references (bottom-up over the
			// pre-order array), then one record pair and reference range per wide-node slot.
			std::vector<Agg> agg(m.n_nodes);
			for (uint32_t i = m.n_nodes; i-- > 0;) {
				if (isLeaf(i)) aggLeaf(agg[i], (uint32_t)m.leaf_begin[i], (uint32_t)m.leaf_count[i], m.refs, m.tri_pos);
				else aggInner(agg[i], agg[i + 1], agg[rightOf(i)]);
			}
			boxRecord(agg[0], rootRec);
			vmaxMesh = meshVmax(agg[0]);
			prune.resize(wide.size());
			out.slotRange.assign(wide.size() * kWideSlots * 2, 0u);
			for (size_t wi = 0; wi < wide.size(); wi++)
				for (int k = 0; k < kWideSlots; k++) {
					const uint32_t nd = slotNode[wi][k];
					slotRecords(nd == kNone ? nullptr : &agg[nd], prune[wi].box[k], prune[wi].plane[k], &out.slotRange[(wi * kWideSlots + k) * 2]);
				}
		}
	}
	out.nodes.swap(nodes); out.wide.swap(wide); out.prune.swap(prune);
	out.rootRec = rootRec; out.vmaxMesh = vmaxMesh; out.boxesRegular = boxesRegular;
	return RTX_OK;
}

} // namespace

namespace rtxflat {

// control words: [0] bit 0 a box is irregular, bit 1 a box is not inside its parent's; [1] deepest wide level; [2] wide roots; [3] deepest
// binary level; [4] leaf boxes; [8..13] the root box; [16..23] the whole mesh's prune record; [24] vmax; [32..35] the edge sum (double) and count
constexpr int kCtlWords = 64;

// node records, parents, the regular-box flag, the root box
__global__ void __launch_bounds__(256) nodesKernel(const float* bounds, const int32_t* skip, const int32_t* lb, const int32_t* lc, uint32_t n,
                                                   Node* nodes, uint32_t* parent, uint32_t* ctl)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	Node nd;
	if (!nodeRecord(bounds + (size_t)i * 6, skip[i], lb[i], lc[i], nd)) atomicOr(&ctl[0], 1u);
	if (lc[i] < 0 && i + 1 < n) {
		parent[i + 1] = i;
		const uint32_t right = lc[i + 1] >= 0 ? i + 2 : (uint32_t)skip[i + 1];
		if (right < n) parent[right] = i;
	}
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

// a leaf's aggregate over its references; an inner node's is merged by mergeLevelKernel
__global__ void __launch_bounds__(256) leafAggKernel(const Node* nodes, uint32_t n, const uint32_t* refs, const float* pos, Agg* agg)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !isLeaf(nodes, i)) return;
	Agg a;
	aggLeaf(a, (uint32_t)nodes[i].first, (uint32_t)~nodes[i].link, refs, pos);
	agg[i] = a;
}

// the inner nodes of binary level d (their children's levels are done)
__global__ void __launch_bounds__(256) mergeLevelKernel(const Node* nodes, uint32_t n, const uint32_t* depth, uint32_t d, Agg* agg)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || depth[i] != d || isLeaf(nodes, i)) return;
	Agg a;
	aggInner(a, agg[i + 1], agg[rightOf(nodes, i)]);
	agg[i] = a;
}

// one prune record pair and slot range per wide-node slot
__global__ void __launch_bounds__(256) pruneKernel(const uint32_t* slotNode, uint32_t nWide, const Agg* agg, PruneBlock* prune, uint32_t* slotRange)
{
	const uint32_t t = blockIdx.x * 256 + threadIdx.x;
	if (t >= nWide * kWideSlots) return;
	const uint32_t wi = t / kWideSlots, k = t % kWideSlots;
	PruneRec pr;
	PlaneRec pl;
	uint32_t range[2];
	const uint32_t nd = slotNode[t];
	slotRecords(nd == kNone ? nullptr : &agg[nd], pr, pl, range);
	prune[wi].box[k] = pr;
	prune[wi].plane[k] = pl;
	slotRange[(size_t)t * 2] = range[0]; slotRange[(size_t)t * 2 + 1] = range[1];
}

// the whole mesh's record and vmax (one thread)
__global__ void rootRecKernel(const Agg* agg, uint32_t* ctl)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	PruneRec pr;
	boxRecord(agg[0], pr);
	memcpy(&ctl[16], &pr, sizeof(PruneRec));
	const float v = meshVmax(agg[0]);
	memcpy(&ctl[24], &v, 4);
}

// the leaf references, three parallel arrays
__global__ void __launch_bounds__(256) refsKernel(const uint32_t* refs, uint32_t nRefs, const float* pos, RefA* ra, RefB* rb, RefC* rc)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r >= nRefs) return;
	RefA a; RefB b; RefC c;
	makeRef(pos + (size_t)refs[r] * 9, refs[r], a, b, c);
	ra[r] = a; rb[r] = b; rc[r] = c;
}

// the leaf boxes of the cost estimate: flag + box per node, then compacted in node order
__global__ void __launch_bounds__(256) leafBoxKernel(const Node* nodes, uint32_t n, const uint32_t* refs, const float* pos, float* box8, uint32_t* flag)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	float b[8];
	const bool has = isLeaf(nodes, i) && leafBox(nodes[i].first, ~nodes[i].link, refs, pos, b);
	flag[i] = has ? 1u : 0u;
	if (!has) return;
	for (int c = 0; c < 8; c++) box8[(size_t)i * 8 + c] = b[c];
}

__global__ void __launch_bounds__(256) leafCompactKernel(const float* box8, const uint32_t* flag, const uint32_t* at, uint32_t n, float* out, uint32_t* ctl)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	if (i == n - 1) ctl[4] = at[i] + flag[i];
	if (!flag[i] || !out) return;
	for (int c = 0; c < 8; c++) out[(size_t)at[i] * 8 + c] = box8[(size_t)i * 8 + c];
}

// the edge terms of the sampled references, summed by one block in a fixed order
__global__ void __launch_bounds__(1024) edgeSumKernel(const RefB* rb, const RefC* rc, uint32_t nRefs, uint32_t stride, uint32_t* ctl)
{
	__shared__ double sum[1024];
	__shared__ uint32_t cnt[1024];
	double s = 0; uint32_t c = 0;
	for (size_t r = (size_t)threadIdx.x * stride; r < nRefs; r += (size_t)1024 * stride) edgeTerm(rb[r], rc[r], s, c);
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

// ---- what both flattens do once the records exist ----

// Copies of a mesh's prune blocks: copy 0 (any ray), then with the sources on the camera's and the point lights' (rtxd::PruneRec), all equal to
// copy 0 until buildSources patches their P.
uint32_t pruneCopies(const rtx_scene* s, uint32_t nLights) { return s->knobs.sources ? 2u + std::min<uint32_t>(nLights, kMaxSrcLights) : 1u; }

// The prune fields of dm and the mesh's source record from nCopies copies of nWide prune blocks at pb (nullptr: no prune records); dm holds its
// leaf references.  A mesh with huge or non-finite coordinates is not pruned at all.  sm.base is set when the mesh takes source copies: the caller
// then adds sm.slotRange.
int meshPruneFields(DevBag& owned, Mesh& dm, rtx_scene::SrcMesh& sm, PruneBlock* pb, uint32_t nCopies, uint32_t nWide, const PruneRec& rootRec, float vmaxMesh, uint32_t mi)
{
	sm = rtx_scene::SrcMesh();
	dm.prune = pb;
	if (pb) {
		sm.pruneAlloc = pb; sm.pruneWide = nWide;
		if (nCopies > 1) { sm.base = pb; sm.nWide = nWide; }
	}
	dm.vmax = vmaxMesh;
	dm.rootRec = rootRec;
	if (!(vmaxMesh < 0x1p40f)) { dm.prune = nullptr; dm.rootRec.h[0] = dm.rootRec.h[1] = dm.rootRec.h[2] = INFINITY; }
	if (sm.base && vmaxMesh < 0x1p40f && dm.nRefs) {
		sm.nRefs = dm.nRefs; sm.refA = dm.refA; sm.refB = dm.refB; sm.refC = dm.refC; sm.vmax = vmaxMesh; sm.meshIndex = mi;
		if (owned.alloc(&sm.refP, ((size_t)dm.nRefs + dm.nRefs / 64 + 2) * sizeof(float), false) != hipSuccess) return (fail(RTX_ERR_DEVICE, "hipMalloc (source scratch)"));
		sm.blockP = sm.refP + dm.nRefs;
	}
	else sm.base = nullptr;
	return RTX_OK;
}

// The bundle-split terms (performance only): the mean edge length of the sampled references (edgeTerm) times fatFactor -> the width above which
// a ray bundle is split; the sphere of the root box.
void meshBundleTerms(Mesh& dm, double sum, uint32_t cnt, const float bounds[6], float factor)
{
	dm.fatRadius = cnt && factor > 0 ? (float)(sum / (double)cnt) * factor : INFINITY;
	double rad = 0;
	for (int c = 0; c < 3; c++) {
		const double lo = bounds[c], hi = bounds[3 + c];
		dm.centre[c] = (float)(0.5 * (lo + hi)); rad += 0.25 * (hi - lo) * (hi - lo);
	}
	dm.radius = (float)std::sqrt(rad);
	if (!std::isfinite(dm.radius)) { dm.radius = 0; dm.fatRadius = INFINITY; }
}

// The geometry of mesh `mi` as rtx_scene_create uploads it: the flattened tree (flattenMesh), the leaf boxes of the cost estimate, the wide nodes,
// the prune blocks and their source copies, the leaf references, the bundle-splitting terms.  Fills those fields of dm, the mesh's source
// record, its leaves and its root box; every allocation goes to `owned` (counted as scene data, but for the sources' scratch).
int uploadMeshGeometry(rtx_scene* s, const rtx_mesh& m, uint32_t mi, uint32_t nLights, DevBag& owned, Mesh& dm, rtx_scene::SrcMesh& sm,
                       rtx_scene::MeshLeaves& leaves, float bounds[6])
{
	using namespace rtxflat;
	FlatMesh flat;
	{
		const int frc = flattenMesh(m, s->knobs.prune, flat);
		if (frc) return frc;
	}
	// leaf references in the reference's order, three parallel arrays padded by one wave; the edge terms of the sampled ones
	std::vector<RefA> refA((size_t)m.n_refs + 64);
	std::vector<RefB> refB((size_t)m.n_refs + 64);
	std::vector<RefC> refC((size_t)m.n_refs + 64);
	memset(refA.data(), 0, refA.size() * sizeof(RefA)); memset(refB.data(), 0, refB.size() * sizeof(RefB)); memset(refC.data(), 0, refC.size() * sizeof(RefC));
	for (uint32_t r = 0; r < m.n_refs; r++) makeRef(m.tri_pos + (size_t)m.refs[r] * 9, m.refs[r], refA[r], refB[r], refC[r]);
	double edgeSum = 0; uint32_t edgeCount = 0;
	for (size_t r = 0; r < m.n_refs; r += edgeStride(m.n_refs)) edgeTerm(refB[r], refC[r], edgeSum, edgeCount);
	for (int c = 0; c < 6; c++) bounds[c] = m.n_nodes ? m.node_bounds[c] : 0.0f;
	HIPCHK(owned.upload(flat.nodes.data(), flat.nodes.size(), &dm.nodes));
	{
		std::vector<float> lb;
		float box[8];
		for (uint32_t i = 0; i < m.n_nodes; i++)
			if (leafBox(m.leaf_begin[i], m.leaf_count[i], m.refs, m.tri_pos, box)) lb.insert(lb.end(), box, box + 8);
		const float* dev = nullptr;
		HIPCHK(owned.upload(lb.data(), lb.size(), &dev));
		leaves = { dev, (uint32_t)(lb.size() / 8) };
	}
	HIPCHK(owned.upload(flat.wide.data(), flat.wide.size(), &dm.wide));
	dm.nWide = (uint32_t)flat.wide.size();
	const size_t nPrune = flat.prune.size();
	const uint32_t nCopies = pruneCopies(s, nLights);
	PruneBlock* pb = nullptr;
	if (nPrune) {
		if (owned.alloc(&pb, (size_t)nCopies * nPrune * sizeof(PruneBlock)) != hipSuccess) return (fail(RTX_ERR_DEVICE, "hipMalloc (prune blocks)"));
		for (uint32_t c = 0; c < nCopies; c++)
			if (hipMemcpy(pb + (size_t)c * nPrune, flat.prune.data(), nPrune * sizeof(PruneBlock), hipMemcpyHostToDevice) != hipSuccess) return (fail(RTX_ERR_DEVICE, "hipMemcpy (prune blocks)"));
	}
	HIPCHK(owned.upload(refA.data(), refA.size(), &dm.refA));
	HIPCHK(owned.upload(refB.data(), refB.size(), &dm.refB));
	HIPCHK(owned.upload(refC.data(), refC.size(), &dm.refC));
	dm.nNodes = m.n_nodes; dm.nRefs = m.n_refs; dm.nTris = m.n_tris; dm.boxesRegular = flat.boxesRegular ? 1u : 0u;
	int rc;
	if ((rc = meshPruneFields(owned, dm, sm, pb, nCopies, (uint32_t)nPrune, flat.rootRec, flat.vmaxMesh, mi))) return rc;
	if (sm.base) HIPCHK(owned.upload(flat.slotRange.data(), flat.slotRange.size(), &sm.slotRange));
	meshBundleTerms(dm, edgeSum, edgeCount, bounds, s->knobs.fatFactor);
	return RTX_OK;
}

// uploadMeshGeometry on the device: the tree of `b` (device builder) and the triangles at pos_dev (n_tris x 9, device) of mesh mi.
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
	hipLaunchKernelGGL(edgeSumKernel, dim3(1), dim3(1024), 0, st, (const RefB*)rb, (const RefC*)rcr, nRefs, edgeStride(nRefs), ctl);
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

	// prune blocks: copy 0, then the source copies; the slots' reference ranges
	const uint32_t nCopies = pruneCopies(s, nLights);
	PruneBlock* pb = nullptr;
	DevArray<uint32_t> slotRange;      // (scratch: copied where the source copies are used)
	if (pruneOn) {
		HIPCHK(owned.alloc(&pb, (size_t)nCopies * nWide * sizeof(PruneBlock)));
		HIPCHK(slotRange.reserve((size_t)nWide * kWideSlots * 2));
		hipLaunchKernelGGL(pruneKernel, dim3(blocksFor((size_t)nWide * kWideSlots)), dim3(256), 0, st, (const uint32_t*)slotNode, nWide, (const Agg*)agg, pb, slotRange.get());
		for (uint32_t c = 1; c < nCopies; c++) HIPCHK(hipMemcpyAsync(pb + (size_t)c * nWide, pb, (size_t)nWide * sizeof(PruneBlock), hipMemcpyDeviceToDevice, st));
	}
	dm.nodes = nodes; dm.refA = ra; dm.refB = rb; dm.refC = rcr;
	dm.nNodes = n; dm.nRefs = nRefs; dm.nTris = nTris; dm.boxesRegular = boxesRegular ? 1u : 0u;
	if ((rc = meshPruneFields(owned, dm, sm, pb, nCopies, nWide, rootRec, vmaxMesh, mi))) return rc;
	if (sm.base) HIPCHK(owned.copyFrom(slotRange.get(), (size_t)nWide * kWideSlots * 2, &sm.slotRange));
	{
		double sum;
		memcpy(&sum, &c1[32], 8);
		meshBundleTerms(dm, sum, c1[34], bounds, s->knobs.fatFactor);
	}
	// (everything queued above has finished before the scratch goes)
	HIPCHK(hipStreamSynchronize(st));
	HIPCHK(hipGetLastError());
	return RTX_OK;
}

} // namespace
