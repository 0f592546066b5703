// castRay's loop over the lights at a hit (scene.cpp:780-846) for a whole wave: the second half of rtxRayLightKernel (rtx_light.hip, whose
// comment describes it) and of rtxRayScatterKernel (rtx_scatter.hip).  Not a header of declarations: this text is included inside the body
// of either kernel's per-wave lambda, where these names are in scope --
//   P, cnt          the kernel's Params and Counts
//   hit             the lane has a hit;  p, n: its point and shading normal;  d: the ray's direction;  ns: the hit object's n_specular
//   wantD, wantS    the lane's diffuse / specular sum is asked for (wave-uniform in rtxRayLightKernel, per lane in rtxRayScatterKernel): what
//                   is not asked for stays +0
//   wantOpen        wave-uniform: every (ray, light) pair is walked
//   h               a Hit the shadow walks may overwrite
//   RTX_LIGHT_LOOP_PER_LIGHT   statements that run once per light after its samples, with li, nLights, D, S and nOpen in scope
//   RTX_LIGHT_LOOP_PARK / RTX_LIGHT_LOOP_UNPARK   optional: statements right before and after the mesh walk of a shadow bundle, for a kernel
//                   that keeps values the walk does not read somewhere else meanwhile (rtx_render_light.hip); absent, they are nothing
// -- and it leaves the sums in diff and spec, which it declares.
// It is text and not a __forceinline__ function because rtxRayLightKernel has to stay the machine code it was: as a function taking a
// callback, all five instances of that kernel came out with another register allocation.
#ifndef RTX_LIGHT_LOOP_PARK
#define RTX_LIGHT_LOOP_PARK
#define RTX_LIGHT_LOOP_UNPARK
#endif
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
				// rtx_occluded_rays' question for {O, -L} with the range dist (RTX_ANY_HIT, rtx_rays.hip): a NaN range occludes nothing (such a
				// lane asks no object).
				// (Source class: a light's source copy was derived for shadow-ray origins within srcNmax |bias| of the surface: a longer shading
				// normal, or NaN, falls back to copy 0 -- advance() in rtx_kernels.hip)
				const bool asked = lit && !(dist != dist);
				bool open = asked;
				if (ballot(asked) != 0) {
					RTX_ANY_HIT(open, O, nL, dist, RTX_WALK_RANGE(dist), (lt == 2 && li < P.nSrcLights && len2(n) <= P.srcNmax2) ? 2u + li : 0u, RTX_LIGHT_LOOP_PARK, RTX_LIGHT_LOOP_UNPARK)
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
			RTX_LIGHT_LOOP_PER_LIGHT
		}
#undef RTX_LIGHT_LOOP_PER_LIGHT
#undef RTX_LIGHT_LOOP_PARK
#undef RTX_LIGHT_LOOP_UNPARK
