// Direct light at the hits of caller-supplied rays (rtx_light_rays, include/rtx_light.h): Render::trace of every
// ray of a batch, getSurfaceData at its hit, and castRay's loop over the lights there (scene.cpp:780-846) -- the diffuse and the specular
// sum, each light's term of both and the number of its shadow rays that arrive -- each written at the ray's own index.
//
// First half: the shared steps of rtx_rays.hip (forEachRayWave, traceWave in its trace-only form with the general source class,
// surfaceAtHit), of which P, N and the ray's direction stay alive.  Second half: a wave-uniform loop over the lights, as castRayPlainWave's:
// light i's record comes through the scalar unit and is the same for all 64 lanes, so is the sample point of an area light in the inner
// loop; every bundle the walk is handed is 64 shadow rays towards one source.  The any-hit trace has rtxAoKernel's shape -- spheres and
// planes first, the mesh walk only for the lanes still open -- and is written out here (one site for every kind of light): shared with the
// other kernels it cost them 1-5 %.  The shadow rays of point light i < P.nSrcLights walk with source class 2 + i, the rule
// of advance() in rtx_kernels.hip.  No state machine, no park area, no recursion frames.
#pragma clang fp contract(off)

namespace {
__device__ __forceinline__ bool plusZero(const V3& v) { return (__float_as_uint(v.x) | __float_as_uint(v.y) | __float_as_uint(v.z)) == 0u; }
} // namespace

template <bool MESH, bool BOXES, int CULLK>
__global__ void __launch_bounds__(256) rtxRayLightKernel(const Params P, const uint32_t* order, const rtx_light_buffers out)
{
	fillPowTab();      // (powfRef's tables, in LDS)
	Counts cnt = {};
	// (wave-uniform: what the caller asked for)
	const bool wantD = out.diffuse_dev || out.light_diffuse_dev, wantS = out.specular_dev || out.light_specular_dev;
	const bool wantOpen = out.light_open_dev != nullptr;
	forEachRayWave(P, order, [&](bool valid, uint32_t i, const V3& o, const V3& d) {
		Hit h;
		traceWave<false, MESH, false, BOXES, CULLK>(P, valid, false, o, d, kFltMax, h, cnt);
		if (valid && out.hits_dev) storeHit(P, h, out.hits_dev + (size_t)i * 8);
		if (!(wantD || wantS || wantOpen)) return;
		const bool hit = valid && h.obj >= 0;
		V3 p, n, albedo;
		float ks;
		surfaceAtHit(P, h, o, d, p, n, albedo, ks);          // (of which only p and n are used)
		const float ns = hit ? P.objects[h.obj].nSpecular : 0.f;
		const V3 O = p + n * P.view.bias;                    // castRay's shadow-ray origin (scene.cpp:787)
		V3 diff = mk(0, 0, 0), spec = mk(0, 0, 0);
		const uint32_t nLights = uni(P.nLights);
		for (uint32_t li = 0; li < nLights; li = uni(li + 1)) {
			const u32x16 w = sload16(P.lights + li);
			const int lt = (int)w[0];
			const V3 lcolor = mk(F(w[1]), F(w[2]), F(w[3]));
			const float lint = F(w[4]);
			const V3 lpos = mk(F(w[8]), F(w[9]), F(w[10]));
			const bool area = lt == 3;
			const float* pts = (const float*)(((uint64_t)w[13] << 32) | w[12]);
			const uint32_t nPoints = w[11];
			// DistantLight::illuminate, lights.cpp:18-23; PointLight::illuminate, lights.cpp:32-38; an area light, scene.cpp:796, 832
			const V3 I = lt == 1 ? lcolor * lint : lcolor * attenuation(lint, len2(p - lpos));
			// a: a point / distant light's max0(N . -L), an area light's dsum; b: powf(max0(R . -dir), ns), or ssum
			float a = 0, b = 0;
			uint32_t nOpen = 0;
			const uint32_t nSamples = area ? nPoints : 1u;
			for (uint32_t k = 0; k < nSamples; k = uni(k + 1)) {
				V3 L;
				float dist;
				if (lt == 1) { L = mk(F(w[5]), F(w[6]), F(w[7])); dist = kFltMax; }
				else {
					V3 from = lpos;
					if (area) { const float* pk = uni(pts + (size_t)k * 3); from = mk(sloadf(pk), sloadf(pk + 1), sloadf(pk + 2)); }
					const V3 Lv = p - from;
					dist = length(Lv);
					L = normalized(Lv);
				}
				const V3 nL = -L;
				const float md = fmaxRef(0.f, dot(n, nL));
				const float sd = wantS ? fmaxRef(0.f, dot(reflectDir(L, n), -d)) : 0.f;
				// A shadow ray that cannot change what is written is not walked ("moot"): with no visibility asked for, one whose terms are
				// +0 for either answer -- a sample of an area light adds open * md and open * sd, a point or distant light writes I * a and I * b or +0.
				bool moot;
				if (area) moot = (!wantD || md == 0.f) && (!wantS || sd == 0.f);
				else {
					a = md;
					if (wantS) b = powfRef(sd, ns);
					moot = (!wantD || plusZero(I * a)) && (!wantS || plusZero(I * b));
				}
				const bool lit = hit && (wantOpen || !moot);
				// rtx_occluded_rays' question for {O, -L} with the range dist: a NaN range occludes nothing (such a lane asks no object); a mesh
				// records only t < FLT_MAX, so a range above FLT_MAX is FLT_MAX for its walk, whose bundle limit has to stay finite
				const bool asked = lit && !(dist != dist);
				bool open = asked;
				if (ballot(asked) != 0) {
					const float tmWalk = dist > kFltMax ? kFltMax : dist;
					if (!MESH) {
						traceWave<false, false, false, BOXES, CULLK>(P, open, true, O, nL, dist, h, cnt);
						open = open && h.obj < 0;
					}
					else {
						traceWave<false, false, false, BOXES, CULLK, 1>(P, open, true, O, nL, dist, h, cnt);
						open = open && h.obj < 0;
						if (ballot(open) != 0) {
							// (a light's source copy was derived for shadow-ray origins within srcNmax |bias| of the surface: a longer shading normal,
							// or NaN, falls back to copy 0 -- advance() in rtx_kernels.hip)
							const uint32_t src = (lt == 2 && li < P.nSrcLights && len2(n) <= P.srcNmax2) ? 2u + li : 0u;
							traceWave<false, true, false, BOXES, CULLK, 2>(P, open, true, O, nL, tmWalk, h, cnt, src);
							open = open && h.obj < 0;
						}
					}
				}
				open = lit && (open || !asked);
				nOpen += open ? 1u : 0u;
				if (area) {
					const float vis = open ? 1.0f : 0.0f;
					a += vis * md;                                   // scene.cpp:803, 841
					b += vis * sd;                                   // scene.cpp:843
				}
				else if (!open) { a = 0; b = 0; }                    // (then D and S are set to +0 below)
			}
			V3 D = mk(0, 0, 0), S = mk(0, 0, 0);
			if (area) {
				const float fn = (float)nPoints;
				if (hit && wantD) D = I * (a / fn);                                 // scene.cpp:805, 845
				if (hit && wantS) S = I * powfRef(b / fn, ns);                      // scene.cpp:846
			}
			else if (nOpen != 0) {
				if (wantD) D = I * a;                                               // scene.cpp:788, 820
				if (wantS) S = I * b;                                               // scene.cpp:824
			}
			diff = diff + D; spec = spec + S;
			if (valid) {
				const size_t at = (size_t)i * nLights + li;
				if (out.light_diffuse_dev) store3(out.light_diffuse_dev + at * 3, D);
				if (out.light_specular_dev) store3(out.light_specular_dev + at * 3, S);
				if (out.light_open_dev) out.light_open_dev[at] = nOpen;
			}
		}
		if (valid) {
			if (out.diffuse_dev) store3(out.diffuse_dev + (size_t)i * 3, diff);
			if (out.specular_dev) store3(out.specular_dev + (size_t)i * 3, spec);
		}
	});
}
RTX_QUERY_INSTANCES(rtxRayLightKernel, (const Params, const uint32_t*, const rtx_light_buffers))
