"""CPU: is the yardstick of the shading data right, and can the inputs see a fault?  The scene family of tests/util_shading.py (non-square
texture / normal / specular maps, 96 x 40 skybox faces, two to four textured tori per scene) through

* the oracle against the real reference, directly (where oracle/_ref is built) and through committed goldens (everywhere);
* the host loader against the reference's loader, byte for byte (where oracle/_ref is built);
* the normals view of the normal-map scenes against the reference's, within its own walk (tests/util_ulp.NORMAL_MAP_ULP);
* a numpy restatement of the index arithmetic that first proves itself against the oracle and then counts, for each index fault the GPU
  tests are meant to catch, the rays whose fetched value changes -- conditions on the INPUTS, asserted, with the counts in the messages.

That the golden tests have teeth was shown on the CPU, with one fault at a time planted in a scratch copy of oracle/rt_oracle.cpp (never in a
kernel: a wrong stride reads outside a map).  Every faulty oracle failed test_oracle_matches_reference_golden and / or
test_normals_view_matches_reference_golden; differing pass-1 pixels of 12 288 / shading rays of 2048 / sky rays of 148, best scene:

    nW and nH exchanged in the normal-map lookup      plain_nrm 1539 / 366 / 0      mixed_nrm 3005 / 824 / 0   (further than 64 ulp)
    dH as the diffuse map's row stride                plain 1426 / 337 / 0          mixed 1818 / 524 / 0 (+ 115 of 512 mirror rays)
    specular map indexed with the diffuse map's size  phong 337 / 118 / 0           mixed 300 / 73 / 0 (+ 46 mirror rays)
    W and H exchanged on sky face 1                   plain 6697 / 595 / 36         all seven goldens fail
    sky faces 4 and 5 exchanged                       phong 2231 / 230 / 24         mixed 1550 / 382 / 24; plain in its rays only
    sky tie order x before z                          0 / 0 / 36 in every golden with the skybox on (sky_directions() only, as expected)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import util_shading as S
from tests.util_ulp import NORMAL_MAP_ULP, bits, ulp_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
BIND = os.path.join(ROOT, "oracle", "_ref", "ref_binding")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (no /root/reference here)")
needs_binding = pytest.mark.skipif(not os.path.exists(BIND), reason="oracle/_ref/ref_binding not built (no /root/reference here)")
NORMALS_GOLDEN = ["plain_nrm", "mixed_nrm"]


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    d = S.short_dir(tmp_path_factory)
    return d, S.write_family(d)


# ---- the generator itself -----------------------------------------------------------------------------------------------------------------
def test_every_texel_is_unique_and_the_sizes_are_the_awkward_ones():
    sizes = {}
    for name, sp in S.FAMILY.items():
        for m in sp.get("meshes", []):
            per_mesh = [m["maps"][k][:2] for k in m["maps"]]
            assert len(set(per_mesh)) == len(per_mesh), "%s: two maps of one mesh have the same size" % name
            for kind, spec in m["maps"].items():
                sizes.setdefault(kind, set()).add(spec[:2])
                img = S.IMAGE[kind](*spec)
                assert img.shape == (spec[1], spec[0], 3)
                key = img.reshape(-1, 3).astype(np.int64)
                key = key.sum(1) if kind == "s" else key[:, 0] * 65536 + key[:, 1] * 256 + key[:, 2]       # (a specular texel is kept as its mean)
                assert len(np.unique(key)) == spec[0] * spec[1], "%s: %s map %s has equal texels" % (name, kind, spec)
    for kind, ss in sizes.items():
        assert any(w > h for w, h in ss) and any(w < h for w, h in ss), (kind, ss)
        assert all((w & (w - 1)) or (h & (h - 1)) for w, h in ss if w != h), (kind, ss)           # (not both powers of two)
    assert any(min(w, h) == 4 for ss in sizes.values() for w, h in ss) and (36, 36) in sizes["d"]
    faces = np.stack([S.sky_image(k).reshape(-1, 3) for k in range(6)]).reshape(-1, 3).astype(np.int64)
    assert len(np.unique(faces[:, 0] * 65536 + faces[:, 1] * 256 + faces[:, 2])) == 6 * S.SKY_W * S.SKY_H and S.SKY_W != S.SKY_H
    subsets = {tuple(sorted(m["maps"])) for sp in S.FAMILY.values() for m in sp.get("meshes", [])}
    assert {("d", "n", "s"), ("d",), ("n",), ("s",), ("d", "s")} <= subsets


def test_sky_directions_hold_what_they_promise():
    d = S.sky_directions()
    assert np.isfinite(d).all() and (np.abs(d).max(1) > 0).all()
    a = np.sort(np.abs(d), 1)
    assert (a[:, 2] == a[:, 1]).sum() >= 26 and (bits(a[:, 2]) - bits(a[:, 1]) == 1).sum() >= 12       # ties, and one ulp off a tie
    assert np.signbit(d[d == 0]).any() and (~np.signbit(d[d == 0])).any()
    face, idx = S.sky_index(d)
    assert set(face) == set(range(6))
    i, j = idx // S.SKY_W, idx % S.SKY_W
    for k in range(6):                                     # first and last row and column of every face
        assert {0, S.SKY_H - 1} <= set(i[face == k]) and {0, S.SKY_W - 1} <= set(j[face == k]), k


# ---- oracle against the reference -----------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tools import ref_harness as R
from oracle import oracle as O
from tests import util_shading as S
name, path, w, h = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
r = R.RefScene(path, w, h); o = O.OracleScene(path, w, h)
if name.startswith('random'):
    b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    fr = r.pass1(); fo = o.pass1()
    assert np.array_equal(b(fr), b(fo)), 'pass1: %%d pixels' %% int((b(fr) != b(fo)).any(-1).sum())
    d = (b(r.ssaa(fr)) != b(o.ssaa(fo))).any(-1); d[0, :] = False; d[:, 0] = False
    assert not d.any(), 'ssaa'
    rays = S.shading_rays(512)
    hr, cr = r.probe(rays); ho, co = o.probe(rays)
    assert np.array_equal(b(hr), b(ho)) and np.array_equal(b(cr), b(co)), 'probe'
else:
    bad = S.differences(S.results(o, name), S.results(r, name))
    assert not bad, bad
print('OK')
"""


@needs_ref
@pytest.mark.parametrize("name", S.REFERENCE_EXACT)
def test_oracle_bit_identical_to_reference(family, name):
    """Pass 1, the 4-sample frame (border masked), the three ray sets and skybox(d) on sky_directions(): one process per scene."""
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, name, family[1][name], str(S.W), str(S.H)], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@needs_ref
@pytest.mark.parametrize("seed", [s for s in S.RANDOM_SEEDS if not S.random_has_normal_map(s)])
def test_oracle_bit_identical_to_reference_on_random_scenes(family, seed):
    """The seeds of tests/test_gpu_shading_data.py's random scenes that the reference defines (no normal map, uv inside [0,1])."""
    w, h = S.random_size(seed)
    path = os.path.join(family[0], "random%d.scene" % seed)
    with open(path, "w") as f:
        f.write(S.make_shading_scene(seed, w, h, family[0]))
    out = subprocess.run([sys.executable, "-c", CHILD % ROOT, "random%d" % seed, path, str(w), str(h)], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def check_assets(g):
    from rendering_amd import assets
    for item in str(g["assets_md5"]).split(";"):
        n, md5 = item.split("=")
        assert assets.md5(n) == md5, "generated asset %s differs from the one the golden was made with" % n


@pytest.mark.parametrize("name", S.REFERENCE_EXACT)
def test_oracle_matches_reference_golden(oracle, family, name):
    """The same results from tests/golden/shading__<scene>.npz (tools/make_golden_shading.py): runs where the reference does not exist."""
    g = np.load(S.golden_file(name))
    check_assets(g)
    want = S.unpack(g)
    o = oracle.OracleScene(family[1][name], S.W, S.H)
    bad = S.differences(S.results(o, name), want)
    o.close()
    assert not bad, "%s: pixels / rays that differ from the reference: %s" % (name, bad)
    if S.FAMILY[name]["sky"] and "meshes" in S.FAMILY[name]:       # the sky rays met the sky (no plane in the way), the mirror rays the mirror
        assert (want["sky_ray_hits"][:, 0] == 0).mean() > 0.9
    if "mirror_hits" in want:
        assert (want["mirror_hits"][:, 1] == 1).sum() >= 64        # (at least a wave of them)


@pytest.mark.parametrize("name", NORMALS_GOLDEN)
def test_normals_view_matches_reference_golden(oracle, family, name):
    """Normal maps against the reference, through the one view in which its in-place normalisation of a sampled texel (objects.cpp:148) is
    a bounded walk: the oracle's showNormals frame and rays within NORMAL_MAP_ULP = 64 of the reference's.  Measured on these maps (20 x 36,
    100 x 28, 52 x 44), three pass 1s in one reference process: they differ from each other by at most 64 ulp in at most 34 pixels
    (plain_nrm) and 8 ulp in 65 pixels (mixed_nrm); the oracle is within 64 ulp of each of them, in at most 146 of 12 288 pixels.  The 64 is
    ONE ulp of a normal's component near -1 seen through N / 2 + 0.5 where that lands in [2^-8, 2^-7); with maps twice as large (44 x 76,
    124 x 36, 100 x 84) a pixel landed below 2^-8 and the reference differed from itself by 128, so the small maps stay.  The goldens keep the
    first and a later pass 1 of one process.  An oracle with nW and nH exchanged is further than 64 ulp from these goldens in 1539 (plain_nrm)
    and 3005 (mixed_nrm) pass-1 pixels and in 366 / 824 of the 2048 rays."""
    g = np.load(S.golden_file(name, "shading_normals"))
    check_assets(g)
    want = S.unpack(g)
    assert ulp_diff(want["pass1_again"], want["pass1"]).max() <= NORMAL_MAP_ULP, "the reference against itself"
    path = os.path.join(family[0], name + "_normals.scene")
    with open(path, "w") as f:
        f.write(S.scene_text(name, family[0], {"showNormals": 1}))
    o = oracle.OracleScene(path, S.W, S.H)
    got = S.results(o, name)
    o.close()
    bad = S.differences(got, want, NORMAL_MAP_ULP)
    assert not bad, "%s: pixels / rays further than %d ulp from the reference: %s" % (name, NORMAL_MAP_ULP, bad)
    assert (ulp_diff(got["pass1"], want["pass1"]) > 0).mean() < 0.1


def test_oracle_normals_view_on_the_existing_goldens(oracle, tmp_path):
    """The oracle's showNormals (scene.cpp:771-772) on the scenes without a normal map: the reference's frames bit for bit."""
    from tests import ac_heatmap as A
    from tests.util_rays import probe_rays
    from tools.make_golden_debug_views import NORMALS, key, load
    gold = load()
    for name, w, h, extra in NORMALS:
        if name.startswith("cfg4"):
            continue
        k = key("normals", name, extra)
        o = oracle.OracleScene(A.scene_copy(name, str(tmp_path), dict(extra, showNormals=1)), w, h)
        fb = o.pass1()
        assert np.array_equal(bits(fb), bits(gold[k + "__pass1"])), k
        d = (bits(o.ssaa(fb)) != bits(gold[k + "__ssaa"])).any(-1)
        d[0, :] = False; d[:, 0] = False
        assert not d.any(), k
        assert np.array_equal(bits(o.probe(probe_rays(1024))[1]), bits(gold[k + "__probe_colours"])), k
        o.close()


# ---- the host loader against the reference's loader -----------------------------------------------------------------------------------------
@needs_binding
@pytest.mark.parametrize("name", sorted(S.FAMILY))
def test_binding_description_equals_the_hosts(ra, family, tmp_path, name):
    """Map sizes, row order, the three maps of a mesh in their own sizes, the six faces: the serialised rtx_scene_desc of the host equals the
    one filled from the reference's own Scene(path) (tests/test_ref_binding.py), normal-map and uv-wild scenes included."""
    from tests.test_ref_binding import first_difference, host_bytes
    out = tmp_path / "ref.bin"
    r = subprocess.run([BIND, "dump", ROOT, family[1][name], str(S.W), str(S.H), str(out)], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    ref = out.read_bytes()
    mine = host_bytes(ra, family[1][name], S.W, S.H)
    assert ref[:8] == b"RTXD0001" and len(ref) > 200
    assert ref == mine, first_difference(ref, mine)


# ---- can the inputs see a fault? ------------------------------------------------------------------------------------------------------------
MAP_FAULTS = ("wh", "stride", "other")
SKY_FAULTS = ("wh", "ij", "faces", "tie")


def scene_counts(oracle, path, name):
    """Per ray set of the scene ("pixels": the frame's primary rays, "rays": shading_rays(2048)): n, first hits per object, sky lookups per face,
    and per fault the number of rays whose fetched value changes."""
    sp = S.FAMILY[name]
    o = oracle.OracleScene(path, S.W, S.H)
    out = {}
    for label, rays in (("pixels", S.primary_rays(o)), ("rays", S.shading_rays(2048))):
        hits, col = o.probe(rays)
        miss = hits[:, 0] == 0
        c = dict(n=len(rays), objects={}, faces=[0] * 6, faults={})
        if sp["sky"]:
            d = rays[miss, 3:6]
            # the restatement proves itself first: the colour of every miss is the restated lookup, bit for bit
            assert np.array_equal(bits(S.sky_colour(d)), bits(col[miss])), "%s %s: the restated sky lookup differs from the oracle" % (name, label)
            face, idx = S.sky_index(d)
            c["faces"] = [int((face == k).sum()) for k in range(6)]
            for f in SKY_FAULTS:
                f2, i2 = S.sky_index(d, fault=f)
                c["faults"]["sky_" + f] = int(((f2 != face) | (i2 != idx)).sum())
        for i, m in enumerate(sp.get("meshes", [])):
            on = (~miss) & (hits[:, 1] == i)
            c["objects"][i] = int(on.sum())
            if not m["maps"] or not on.any():
                continue
            tx, ty = S.tex_coords(o.bvh(i)["tris"], hits[on, 2].astype(np.int64), hits[on, 4], hits[on, 5])
            sizes = {k: m["maps"][k][:2] for k in m["maps"]}
            for f in MAP_FAULTS:
                changed = np.zeros(int(on.sum()), bool)
                for kind, size in sizes.items():
                    others = [s for k, s in sizes.items() if k != kind]
                    if f == "other" and not others:
                        continue
                    changed |= S.map_index(size, tx, ty) != S.map_index(size, tx, ty, f, others[0] if others else None)
                c["faults"]["map_" + f] = c["faults"].get("map_" + f, 0) + int(changed.sum())
        out[label] = c
    o.close()
    return out


def test_restated_sky_lookup_equals_the_oracle(oracle, family):
    o = oracle.OracleScene(family[1]["plain"], S.W, S.H)
    d = S.sky_directions()
    assert np.array_equal(bits(S.sky_colour(d)), bits(o.skybox(d)))
    o.close()


def test_the_inputs_can_see_each_fault(oracle, family):
    """Conditions on the inputs (not tolerances): every index fault changes the fetched value of at least 1 % of the rays of some scene (frame
    pixels or shading_rays; the tie order of at least 1 % of sky_directions(), the only rays that can tell), every textured mesh is the first hit
    of at least 4 % of a frame's pixels in some scene, the sky of at least 10 %, each of the six faces is returned for at least 1 % of a scene's
    pixels or rays.  Texels are unique, so a value changes exactly where the index does."""
    counts = {name: scene_counts(oracle, family[1][name], name) for name in S.FAMILY}
    report = "\n".join("%s %s: %s" % (n, l, c) for n, per in counts.items() for l, c in per.items())
    best = {}
    for per in counts.values():
        for c in per.values():
            for f, k in c["faults"].items():
                best[f] = max(best.get(f, 0.0), k / c["n"])
    d = S.sky_directions()
    f0, i0 = S.sky_index(d)
    f1, i1 = S.sky_index(d, fault="tie")
    best["sky_tie"] = float(((f0 != f1) | (i0 != i1)).mean())
    for f in ["map_" + x for x in MAP_FAULTS] + ["sky_" + x for x in SKY_FAULTS]:
        assert best.get(f, 0.0) >= 0.01, "fault %s changes at most %.2f %% of a scene's rays\n%s" % (f, 100 * best.get(f, 0.0), report)
    for slot in range(4):
        share = max(per["pixels"]["objects"].get(slot, 0) / per["pixels"]["n"] for n, per in counts.items() if "meshes" in S.FAMILY[n])
        assert share >= 0.04, "mesh %d is the first hit of at most %.2f %% of a frame\n%s" % (slot, 100 * share, report)
    for n, per in counts.items():
        if S.FAMILY[n]["sky"]:
            assert sum(per["pixels"]["faces"]) >= 0.10 * per["pixels"]["n"], "%s: the sky fills less than 10 %% of the frame\n%s" % (n, report)
    for k in range(6):
        share = max(c["faces"][k] / c["n"] for per in counts.values() for c in per.values())
        assert share >= 0.01, "sky face %d is returned for at most %.2f %% of a scene's pixels or rays\n%s" % (k, 100 * share, report)
    # the frames themselves see five faces directly (the sixth, behind the camera, through the mirrors and the rays)
    seen = {k for per in counts.values() for k in range(6) if per["pixels"]["faces"][k] >= 0.01 * per["pixels"]["n"]}
    assert len(seen) >= 5, "%s\n%s" % (seen, report)
