// Surface points projected into cameras, with visibility (rtx_project_points, include/rtx_project.h): the way back
// from a point of the scene into a camera's pixel grid, and the shadow ray castRay would cast at the point towards a point light at the
// camera.  The front end is the point queries' (rtx_points.hip): forEachRayWave's persistent waves over the order, whose `origin` and
// `direction` are P and N here.
//
// rtxPointProjectKernel: a wave-uniform loop over the cameras, as rtxPointAoKernel's over the directions and the light loop's over the
// lights.  Record c comes through the scalar unit (three loads: 8 + 8 + 4 dwords of its 24) and is the same for all 64 lanes; per lane the
// header's arithmetic -- the point light's dist and L, three dot products with the rows the primary ray multiplies as columns, four IEEE
// divisions -- then one ballot of the lanes to walk and one RTX_ANY_HIT for them: spheres and planes first, the mesh walk for the lanes
// still open.  The source class is 0: a camera of the table has no source copy of the prune records (the scene's own camera copy, class 1,
// is valid for origins AT that camera only, and these rays start at the surface).
// Pixel and depth are stored before the walk, so that only the flags stay alive across it; all stores are per lane at c * n + i --
// consecutive points, consecutive addresses, as long as the batch is not regrouped (from 2^20 points on the order is the sort's, and the
// stores scatter as those of every point query do; the batch is regrouped even when nothing is walked: DESIGN.md 3.28, left for later).
#pragma clang fp contract(off)

struct ProjectArgs {
	const float* cams;      // nCams x 24
	uint32_t nCams;
	uint32_t walk;          // with_visibility != 0 && flags: without it nothing is traced
	float* pixel;           // nCams x n x 2 or nullptr
	float* depth;           // nCams x n or nullptr
	uint8_t* flags;         // nCams x n or nullptr
};

namespace {
// 32 / 16 bytes of a camera record, which need not be aligned beyond its floats (a caller's slice of a larger table)
typedef uint32_t CamWords8 __attribute__((ext_vector_type(8), aligned(4)));
typedef uint32_t CamWords4 __attribute__((ext_vector_type(4), aligned(4)));
} // namespace

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxPointProjectKernel(const Params P, const uint32_t* order, const ProjectArgs A)
{
	Counts cnt = {};
	const uint32_t nCams = uni(A.nCams);
	const bool walk = uni(A.walk) != 0;
	const size_t n = P.nProbe;
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& p, const V3& N) {
		const V3 O = p + N * P.view.bias;                      // castRay's shadow-ray origin (scene.cpp:787)
		Hit h;
		for (uint32_t c = 0; c < nCams; c = uni(c + 1)) {
			const float* rec = uni(A.cams + (size_t)c * 24);
			const CamWords8 r0 = *(const RTX_AS4 CamWords8*)(uintptr_t)rec;              // cam_pos, scale, aspect, width, height, 0
			const CamWords8 m0 = *(const RTX_AS4 CamWords8*)(uintptr_t)(rec + 8);        // cam_matrix [0, 8)
			const CamWords4 m8 = *(const RTX_AS4 CamWords4*)(uintptr_t)(rec + 16);       // cam_matrix [8, 12)
			const float scale = F(r0[3]), aspect = F(r0[4]), width = F(r0[5]), height = F(r0[6]);
			// PointLight::illuminate at the camera's position, lights.cpp:32-38 (rtx_light_loop.h)
			const V3 cv = p - mk(F(r0[0]), F(r0[1]), F(r0[2]));
			const float dist = length(cv);
			const V3 L = normalized(cv);
			// the transpose of viewRay's product (rtx_kernels.hip)
			const float sx = (cv.x * F(m0[0]) + cv.y * F(m0[1])) + cv.z * F(m0[2]);
			const float sy = (cv.x * F(m0[4]) + cv.y * F(m0[5])) + cv.z * F(m0[6]);
			const float sz = (cv.x * F(m8[0]) + cv.y * F(m8[1])) + cv.z * F(m8[2]);
			const float inz = -sz;
			const float xp = sx / inz, yp = sy / inz;
			const float ax = scale * aspect;
			const float px = (xp / ax + 1) * (width * 0.5f) - 1;
			const float py = (1 - yp / scale) * (height * 0.5f) - 1;
			const bool front = sz < 0;
			const bool inside = front && px >= -0.5f && px < width - 1.5f && py >= -0.5f && py < height - 1.5f;      // (NaN compares false)
			const V3 nL = -L;
			const bool facing = dot(N, nL) > 0;                    // strict: a zero or NaN normal never faces
			const size_t at = (size_t)c * n + i;
			if (valid) {
				if (A.pixel) { float* q = A.pixel + at * 2; q[0] = px; q[1] = py; }
				if (A.depth) A.depth[at] = dist;
			}
			uint32_t fl = (front ? RTX_PROJ_FRONT : 0u) | (inside ? RTX_PROJ_INSIDE : 0u) | (facing ? RTX_PROJ_FACING : 0u);
			// rtx_occluded_rays' question for {O, -L} with the range dist (RTX_ANY_HIT, rtx_rays.hip): a NaN range occludes nothing and is not
			// OPEN either (such a lane asks no object)
			const bool asked = walk && valid && inside && !(dist != dist);
			bool open = asked;
			if (ballot(asked) != 0) {
				RTX_ANY_HIT(open, O, nL, dist, RTX_WALK_RANGE(dist), 0u, , )
			}
			if (open) fl |= RTX_PROJ_OPEN;
			if (valid && A.flags) A.flags[at] = (uint8_t)fl;
		}
	});
}
RTX_QUERY_INSTANCES(rtxPointProjectKernel, (const Params, const uint32_t*, const ProjectArgs))
