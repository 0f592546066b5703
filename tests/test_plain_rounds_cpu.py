"""CPU companion of tests/test_gpu_plain_rounds.py: the scenes of tests/util_plain_rounds.py are what their names say (on the oracle's own
frame) and hold nothing that rules a PLAIN kernel out (no material other than Diffuse, no area light; that a PLAIN kernel runs is asserted by the
GPU test through rtx_kernel_variant), and -- where oracle/_ref is built -- the oracle the GPU is compared with there is bit-identical to the reference on them: pass 1, the SSAA frame and the frame's primary rays as probe rays."""
import os
import subprocess
import sys

import pytest

from tests import util_plain_rounds as PR
from tests import util_shading as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_harness.so")
needs_ref = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref not built (the reference is not on this machine)")


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = U.short_dir(tmp_path_factory)
    U.write_images(d)
    return d


@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", sorted(PR.SCENES))
def test_scenes_are_what_they_are_named_after(oracle, images, name, cull):
    path = PR.write_scene(name, images, cull)
    o = oracle.OracleScene(path, PR.W, PR.H)
    PR.expectations(name, o, o.pass1())
    o.close()
    text = open(path).read()
    assert "material=" not in text and "type=area" not in text and "type=mesh" in text      # (what rtx_scene_create asks of a PLAIN scene)
    assert ("useBackfaceCulling=%d" % cull) in text


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
from tools import ref_harness as R
from oracle import oracle as O
from tests import util_shading as U
path, w, h = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
r = R.RefScene(path, w, h, workers=1); o = O.OracleScene(path, w, h)
b = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
fr = r.pass1(); fo = o.pass1()
assert np.array_equal(b(fr), b(fo)), 'pass1'
f2r = r.ssaa(fr); f2o = o.ssaa(fo)
d = (b(f2r) != b(f2o)).any(-1); d[0, :] = False; d[:, 0] = False
assert not d.any(), 'ssaa'
rays = U.primary_rays(o)
hr, cr = r.probe(rays); ho, co = o.probe(rays)
assert np.array_equal(b(hr), b(ho)) and np.array_equal(b(cr), b(co)), 'probe'
print('OK')
"""


@needs_ref
@pytest.mark.parametrize("cull", [1, 0])
@pytest.mark.parametrize("name", sorted(PR.SCENES))
def test_oracle_bit_identical_to_reference(images, name, cull):
    # one scene per process: the reference keeps process-global option flags.  One worker (CHILD): with one worker per core the reference's pass 1 of these scenes
    # differed from its own single-worker frame in about one run of thirty -- what is compared here is arithmetic, not the reference's threading
    path = PR.write_scene(name, images, cull)
    for w, h in ((PR.W, PR.H), (136, 200)):
        out = subprocess.run([sys.executable, "-c", CHILD % ROOT, path, str(w), str(h)], cwd=ROOT, capture_output=True, text=True)
        assert out.returncode == 0 and "OK" in out.stdout, "%dx%d: " % (w, h) + out.stdout[-2000:] + out.stderr[-2000:]
