"""rtx_render_ao / Scene.render_ao without a GPU: the extension header and its symbol list, sphere_directions, the argument checks, and the
inputs of the GPU tests (tests/test_gpu_ao.py) shown to be non-trivial with the oracle alone: a fair share of the traced rays is
occluded, the radius matters, pixels differ in how many directions they trace, and the transparent-skipping rule decides answers.

The statistics here take the normal decoded from the showNormals colour (tests/util_ao.decoded_normals), which is within an ulp or two of
hitNormal: good enough for shares and counts, not for the bit-exact expectations of the GPU tests, which take N from render_aov."""
import os
import re

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_occlusion as OC

ROOT = U.ROOT
f32 = np.float32


def test_ao_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_ao.h")).read()
    declared = set(re.findall(r"\b(rtx_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(ra.RTX_AO_SYMBOLS) and len(ra.RTX_AO_SYMBOLS) == len(declared)
    for other in (ra.RTX_SYMBOLS, ra.RTX_EDIT_SYMBOLS, ra.RTX_QUERY_SYMBOLS, ra.RTX_AOV_SYMBOLS):
        assert not declared & set(other)
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_render_ao(None, 0, 8, None, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()


def test_sphere_directions(ra):
    for n in (2, 12, 16, 256):
        d = ra.sphere_directions(n)
        assert d.dtype == np.float32 and d.shape == (n, 3)
        assert np.array_equal(d[n // 2:], -d[: n // 2])
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert (d[: n // 2, 2] > 0).all()
        # the formula, restated
        i = np.arange(n // 2) + 0.5
        z = 1 - 2 * i / n
        phi = i * np.pi * (3 - np.sqrt(5))
        want = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1).astype(np.float32)
        assert np.array_equal(d[: n // 2], want)
        # antipodal: any plane through the origin that holds no direction has n / 2 on either side
        for normal in np.random.default_rng(n).normal(size=(8, 3)):
            assert ((d.astype(np.float64) @ normal) > 0).sum() == n // 2
    for bad in (0, 1, 7, -2):
        with pytest.raises(ValueError):
            ra.sphere_directions(bad)


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    d = z((4, 3))
    cases = [
        (dict(dirs=d), "at least one buffer"),
        (dict(dirs=np.zeros((4, 3), np.float32), ao=z((24, 32))), "dirs must be a torch tensor"),
        (dict(dirs=z((4, 3), torch.float64), ao=z((24, 32))), "dirs must be float32"),
        (dict(dirs=z((3, 4)), ao=z((24, 32))), r"dirs must have shape \(K, 3\)"),
        (dict(dirs=z((12,)), ao=z((24, 32))), r"dirs must have shape \(K, 3\)"),
        (dict(dirs=z((4, 6))[:, ::2], ao=z((24, 32))), "dirs must be contiguous"),
        (dict(dirs=d, ao=z((24, 32))), "dirs must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.render_ao(**kw)
    assert s._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


def oracle_rays(oracle, path, w, h, cull, dirs):
    """The traced rays of a frame from the oracle alone (decoded normals): (traced, pix, k, rays, exp)."""
    exp = U.expected_of(path, w, h, cull)
    o = oracle.OracleScene(path, w, h)
    rays = U.primary_rays(o)
    o.close()
    hit = exp["hit"] & U.written_mask(w, h)
    return AO.traced_rays(rays, exp["depth"], AO.decoded_normals(exp), hit, dirs) + (exp,)


# the share of the traced rays that is occluded: [0.15, 0.6] at radius +inf, at least 0.05 at radius 1.0.  What the oracle gives at these
# sizes with the scenes' bias of 1e-4 (culling on / off), printed by the test:
#   coincident         3090 rays         0.241 / 0.250  and  0.100 / 0.115
#   cfg2_smooth_4k     4002 rays         0.457          and  0.167
#   cfg4_textured_256  1416 / 3072 rays  0.369 / 0.396  and  0.337 / 0.388
#   area_light         3306 rays         0.387 / 0.388  and  0.151
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", ["coincident", "cfg2_smooth_4k", "cfg4_textured_256", "area_light"])
def test_a_fair_share_of_the_rays_is_occluded(oracle, tmp_path, name, cull):
    path = "scenes/%s.scene" % name
    w, h = U.size_of(name)
    traced, pix, k, rays, _ = oracle_rays(oracle, path, w, h, cull, AO.DIRS19[:12])
    assert len(rays) >= 1000
    hit, t = OC.opaque_probe(oracle, path, tmp_path, rays, culling=cull)
    whole = OC.expected(hit, t, f32(np.inf))
    near = OC.expected(hit, t, f32(1.0))
    print("%s %dx%d cull %d: %d traced rays, occluded %.3f at +inf, %.3f at 1.0" % (name, w, h, cull, len(rays), whole.mean(), near.mean()))
    assert 0.15 <= whole.mean() <= 0.6
    assert near.mean() >= 0.05 and near.sum() < whole.sum()
    # pixels differ in their answers: neither all open nor all closed
    _, ao = AO.reduce(traced, pix, whole, (h, w))
    assert len(np.unique(ao)) > 4


def test_pixels_trace_different_numbers_of_directions(oracle):
    name = "cfg1_simple_shapes"
    w, h = U.size_of(name)
    traced, pix, k, rays, exp = oracle_rays(oracle, "scenes/%s.scene" % name, w, h, None, AO.DIRS19)
    ntr = traced.sum(1).reshape(h, w)
    m = U.written_mask(w, h) & exp["hit"]
    both = m[:, 1:] & m[:, :-1]
    assert ((ntr[:, 1:] != ntr[:, :-1]) & both).any(), "every pixel traces as many directions as its neighbour"
    assert len(np.unique(ntr[m])) >= 3
    # the plane (object 0, normal (0, 1, 0)): c == 0 exactly for (1, 0, 0) and (0, 0, 1), c < 0 for (0, -1, 0); never the zero and the NaN direction
    plane = (m & (exp["object_id"] == 0)).reshape(-1)
    assert plane.sum() > 50
    t = traced[plane]
    assert not t[:, 12].any() and not t[:, 14].any() and not t[:, 15].any() and t[:, 13].all() and t[:, 18].all()
    assert not traced[:, 16].any() and not traced[:, 17].any()
    assert (traced[m.reshape(-1)][:, 18]).any() and not traced[~m.reshape(-1)].any()


def test_the_transparent_rule_decides_answers(oracle, tmp_path):
    """cfg3_reflective_refractive at 24x40 (its size in the GPU tests): rays whose only blocker is transparent -- a hit in S, none in S'."""
    name = "cfg3_reflective_refractive"
    path = "scenes/%s.scene" % name
    w, h = U.size_of(name)
    assert (w, h) == (24, 40)
    _, dropped = OC.opaque_scene(path, tmp_path)
    assert dropped >= 1
    traced, pix, k, rays, _ = oracle_rays(oracle, path, w, h, None, AO.DIRS19)
    o = oracle.OracleScene(path, 64, 64)
    hs, _ = o.probe(rays, colours=False)
    o.close()
    in_s = hs[:, 0] > 0
    in_s1, _ = OC.opaque_probe(oracle, path, tmp_path, rays)
    only_transparent = in_s & ~in_s1
    print("%s: %d of %d traced rays are blocked by transparent objects only" % (name, only_transparent.sum(), len(rays)))
    assert only_transparent.sum() >= 1
    assert not (in_s1 & ~in_s).any()
