"""rtx_radiance_points (Scene.radiance_points; include/rtx_radiance.h) without a GPU: the extension header against the symbol list, the
argument checks, and tests/util_radiance's restatement of the contract pinned to the oracle alone where the exact normal is known without
a GPU (planes and spheres): fed with the colours OracleScene.probe gives the rays {P + N * bias, d_k}."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util_ao as AO
from tests import util_aov as U
from tests import util_radiance as UR
from tests.test_points_cpu import CASES, case_of

ROOT = U.ROOT
f32 = np.float32


def test_radiance_header_and_symbol_list(ra):
    hdr = open(os.path.join(ROOT, "include", "rtx_radiance.h")).read()
    declared = re.findall(r"^int\s+(rtx_[a-z0-9_]+)\s*\(", hdr, re.M)
    assert declared == list(ra.RTX_RADIANCE_SYMBOLS) == ["rtx_radiance_points"]
    others = [n for n in dir(ra) if re.fullmatch(r"RTX_[A-Z_]*SYMBOLS", n) and n != "RTX_RADIANCE_SYMBOLS"]
    assert len(others) >= 12
    for other in others:
        assert not set(declared) & set(getattr(ra, other)), other
    rtx, _ = ra.load()
    for s in declared:
        assert hasattr(rtx, s), s
    listed, missing = ra.exported_symbols()
    assert not missing and listed == list(ra.RTX_SYMBOLS)
    # the structure of the binding is the header's
    body = re.search(r"typedef struct rtx_radiance_params \{(.*?)\} rtx_radiance_params;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|const float\*|int32_t)\s+(\w+);", body)
    assert fields == [("uint32_t", "n_dirs"), ("const float*", "dirs_dev"), ("const float*", "weights_dev"), ("int32_t", "cosine")]
    assert [n for n, _ in ra.RadianceParams._fields_] == [n for _, n in fields]
    assert [t for _, t in ra.RadianceParams._fields_] == [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32]


def test_c_entry_refuses_a_null_scene(ra):
    rtx, _ = ra.load()
    par = ra.RadianceParams()
    assert rtx.rtx_radiance_points(None, 4, None, None, None, None, None) == -1      # RTX_ERR_ARG
    assert b"NULL" in rtx.rtx_last_error()
    assert rtx.rtx_radiance_points(None, 4, None, C.byref(par), None, None, None) == -1
    assert b"NULL" in rtx.rtx_last_error()


def test_bad_arguments_are_refused_before_the_gpu(ra):
    torch = pytest.importorskip("torch")
    s = ra.Scene("scenes/cfg1_simple_shapes.scene", 32, 24)
    z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt)
    dirs = z((3, 3))
    cases = [
        (dict(points=z((4, 6)), total=False), "radiance_points: nothing to compute"),
        (dict(points=z((24,)), counts=True), r"radiance_points: points must have shape \(n, 6\)"),
        (dict(points=np.zeros((4, 6), np.float32)), "radiance_points: points must be a torch tensor"),
        (dict(points=z((4, 6), torch.float64)), "radiance_points: points must be float32"),
        (dict(points=z((6, 4))), r"radiance_points: points must have shape \(n, 6\)"),
        (dict(points=z((4, 12))[:, ::2]), "radiance_points: points must be contiguous"),
        (dict(points=z((4, 6))), "radiance_points: points must be on cuda:0"),
    ]
    for kw, what in cases:
        with pytest.raises(ValueError, match=what):
            s.radiance_points(**dict(dict(dirs=dirs), **kw))
    # (the points are looked at first, then the directions and the weights: the device is the last thing _check_tensor asks about, so
    # tensors of the host get as far as their device)
    class OnDevice(torch.Tensor):
        """a host tensor that says it is on cuda:0: what the checks after the points' see without a GPU"""
        @property
        def device(self):
            return torch.device("cuda", 0)

    p = z((4, 6)).as_subclass(OnDevice)
    more = [
        (dict(dirs=z((3, 4))), r"radiance_points: dirs must have shape \(K, 3\)"),
        (dict(dirs=z((3, 3), torch.float64)), "radiance_points: dirs must be float32"),
        (dict(dirs=z((3, 3))), "radiance_points: dirs must be on cuda:0"),
        (dict(dirs=z((0, 3)).as_subclass(OnDevice)), r"radiance_points: 1 \.\. 256 directions per call, got 0"),
        (dict(dirs=z((257, 3)).as_subclass(OnDevice)), r"radiance_points: 1 \.\. 256 directions per call, got 257"),
        (dict(dirs=z((3, 3)).as_subclass(OnDevice), weights=z((3,), torch.float64)), "radiance_points: weights must be float32"),
        (dict(dirs=z((3, 3)).as_subclass(OnDevice), weights=z((4,))), r"radiance_points: weights must have shape \(3,\)"),
        (dict(dirs=z((3, 3)).as_subclass(OnDevice), weights=z((6,))[::2]), "radiance_points: weights must be contiguous"),
        (dict(dirs=z((3, 3)).as_subclass(OnDevice), weights=z((3,))), "radiance_points: weights must be on cuda:0"),
    ]
    for kw, what in more:
        with pytest.raises(ValueError, match=what):
            s.radiance_points(p, **kw)
    assert s._gpu is None                  # (the scene was never flattened and uploaded: no GPU call was made)
    s.close()


_probe = {}


def probed(oracle, name, w, h):
    """The points of tests/test_points_cpu.py's case with the oracle's colours of all their rays under DIRS19, computed once per scene
    and shared read-only"""
    if name not in _probe:
        c = case_of(oracle, name, w, h)
        points = c["points"]
        rays, traced = UR.rays(points, AO.DIRS19)
        o = oracle.OracleScene(c["path"], w, h)
        _, col = o.probe(rays)
        o.close()
        col = col.reshape(len(points), len(AO.DIRS19), 3)
        for a in (rays, traced, col):
            a.setflags(write=False)
        _probe[name] = dict(points=points, rays=rays, traced=traced, col=col)
    return _probe[name]


@pytest.mark.parametrize("name,w,h", CASES)
def test_the_restatement_against_the_oracles_colours(oracle, name, w, h):
    c = probed(oracle, name, w, h)
    points, traced, col = c["points"], c["traced"], c["col"]
    n, K = traced.shape
    N = points[:, 3:6]
    # the built rays are util_points' traced rays, in its order
    from tests import util_points as UP
    traced_p, pt, k, rays_p = UP.ao_traced_rays(points, AO.DIRS19)
    assert np.array_equal(traced, traced_p) and np.array_equal(UR.bits(c["rays"].reshape(n, K, 6)[pt, k]), UR.bits(rays_p))
    assert n >= 700 and traced.any(0)[:12].all() and not traced[:, 16].any() and not traced[:, 17].any()
    assert (traced.sum(1) != traced.sum(1)[0]).any()
    # one direction, no weights, no cosine: the probe's colour bit for bit where traced, +0 where not
    for kk in range(K):
        total, counts = UR.reduce(col[:, kk:kk + 1], N, AO.DIRS19[kk:kk + 1])
        assert np.array_equal(counts, traced[:, kk].astype(np.uint32))
        want = np.where(traced[:, kk, None], col[:, kk], f32(0))
        # (+0 + x keeps the bits of x except for x == -0: a colour is never -0)
        assert not (UR.bits(col[:, kk][traced[:, kk]]) == 0x80000000).any()
        assert np.array_equal(UR.bits(total), UR.bits(want)), "direction %d" % kk
    # the full set: a scalar loop over np.float32 values gives the restatement's bits
    rng = np.random.default_rng(0x5AD)
    weights = rng.uniform(0.05, 2.0, K).astype(f32)
    odd = weights.copy()
    odd[1], odd[4], odd[7] = f32(0), f32(-0.75), f32(np.nan)
    sub = np.sort(rng.choice(n, 160, replace=False))
    seen = []
    for wts in (None, weights, odd):
        for cosine in (False, True):
            total, counts = UR.reduce(col, N, AO.DIRS19, wts, cosine)
            assert total.dtype == f32 and counts.dtype == np.uint32 and np.array_equal(counts, traced.sum(1))
            t2, c2 = UR.reduce_scalar(col[sub], N[sub], AO.DIRS19, wts, cosine)
            assert np.array_equal(UR.bits(total[sub]), UR.bits(t2)) and np.array_equal(counts[sub], c2), (wts is not None, cosine)
            seen.append(total)
    assert np.isnan(seen[4]).any() and not np.isnan(seen[2]).any()
    assert not np.array_equal(UR.bits(seen[0]), UR.bits(seen[1])) and not np.array_equal(UR.bits(seen[0]), UR.bits(seen[2]))
    # weights of one are no weights
    for cosine in (False, True):
        a, _ = UR.reduce(col, N, AO.DIRS19, np.ones(K, f32), cosine)
        b, _ = UR.reduce(col, N, AO.DIRS19, None, cosine)
        assert np.array_equal(UR.bits(a), UR.bits(b))
    # a zero and a NaN normal: nothing is traced, the sum is +0
    dead = points[:8].copy()
    dead[:4, 3:6] = 0
    dead[4:, 3] = np.nan
    rays_d, traced_d = UR.rays(dead, AO.DIRS19)
    assert not traced_d.any()
    total, counts = UR.reduce(np.full((8, K, 3), f32(3.5)), dead[:, 3:6], AO.DIRS19, weights, True)
    assert not counts.any() and not UR.bits(total).any()
