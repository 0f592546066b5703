"""What rtx_render_ao / Scene.render_ao must write (include/rtx_ao.h), built from what is already pinned to the oracle.

The oracle exposes hitNormal only as N / 2 + 0.5, so the exact N and tNear of every pixel come from Scene.render_aov(depth=, normal=,
object_id=) -- existing code, bit for bit the oracle's by tests/test_gpu_aov.py, and not the code under test.  tests/util_aov.primary_rays
gives the rays; P, O and c are restated here in numpy float32 in the order of the contract.  The traced rays {O, d_k} are then answered
either by the CPU oracle (tests/util_occlusion.opaque_probe / expected: yardstick (i)) or by Scene.occluded (yardstick (ii)), and reduced
to `counts` and `ao` in numpy, whose float32 division gives the expected bits of ao."""
import numpy as np

import rendering_amd as RA
from tests import util_aov as U
from tests import util_occlusion as OC

f32 = np.float32
# options.h:9-20 -- Options::bias, which no scene file sets (rtx_view::bias of every scene)
BIAS = f32(0.0001)

# sphere_directions(12); the axes, of which the planes with normal (0, 1, 0) meet two at c == 0 exactly and one at c < 0; a zero and a NaN
# direction (never traced); one that is not of unit length
DIRS19 = np.concatenate([RA.sphere_directions(12),
                         np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, 0], [np.nan, 0, 0], [3, 4, 0]], f32)]).astype(f32)
assert DIRS19.shape == (19, 3)


def traced_rays(rays, depth, normal, hit, dirs, bias=BIAS):
    """Steps 1 and 2 of the contract for the pixels of a frame, row-major.  rays: n x 6 primary rays; depth (n,), normal (n, 3), hit (n,)
    of their first hits.  Returns (traced [n, K] bool, pix, k, out) -- out[j] = {O[pix[j]], dirs[k[j]]}, the traced rays in pixel-major
    order."""
    rays = np.asarray(rays, f32); depth = np.asarray(depth, f32).reshape(-1); N = np.asarray(normal, f32).reshape(-1, 3)
    hit = np.asarray(hit, bool).reshape(-1); dirs = np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        P = rays[:, 0:3] + rays[:, 3:6] * depth[:, None]                 # orig + dir * tNear, per component
        O = P + N * f32(bias)
        c = (N[:, 0:1] * dirs[None, :, 0] + N[:, 1:2] * dirs[None, :, 1]) + N[:, 2:3] * dirs[None, :, 2]
        traced = hit[:, None] & (c > 0)
    assert P.dtype == f32 and O.dtype == f32 and c.dtype == f32
    pix, k = np.nonzero(traced)
    out = np.concatenate([O[pix], dirs[k]], 1).astype(f32)
    return traced, pix, k, np.ascontiguousarray(out)


def reduce(traced, pix, occluded, shape):
    """Step 3: counts (uint32) and ao (float32) of the frame from one byte per traced ray."""
    n = traced.shape[0]
    ntr = traced.sum(1).astype(np.uint32)
    nopen = np.bincount(pix, weights=(np.asarray(occluded) == 0), minlength=n).astype(np.uint32)
    counts = nopen | (ntr << np.uint32(16))
    with np.errstate(all="ignore"):
        ao = np.where(ntr > 0, nopen.astype(f32) / ntr.astype(f32), f32(1)).astype(f32)
    return counts.reshape(shape), ao.reshape(shape)


def first_hits(g):
    """(rays, depth, normal, hit) of Scene g through render_aov, as numpy arrays over the pixels row-major.  Pixels render_aov does not
    write (last row and column) are misses here; no call writes them."""
    import torch
    w, h = g.width, g.height
    depth = torch.full((h, w), float(np.finfo(f32).max), dtype=torch.float32, device="cuda")
    normal = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    obj = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
    g.render_aov(depth=depth, normal=normal, object_id=obj)
    torch.cuda.synchronize()
    return U.primary_rays(g), depth.cpu().numpy().reshape(-1), normal.cpu().numpy().reshape(-1, 3), obj.cpu().numpy().reshape(-1) >= 0


class Expectation:
    """The traced rays of Scene g under `dirs` and their answers: by_oracle(radius) is yardstick (i), by_occluded(radius) yardstick (ii);
    each returns (counts, ao) of the frame.  The oracle is asked once: its (hit', tNear') serves every radius."""

    def __init__(self, g, dirs):
        self.g = g
        self.shape = (g.height, g.width)
        self.dirs = np.asarray(dirs, f32)
        self.traced, self.pix, self.k, self.rays = traced_rays(*first_hits(g), self.dirs)
        self._probe = None

    def probe(self, oracle, path, tmp_path, culling):
        if self._probe is None:
            if len(self.rays):
                self._probe = OC.opaque_probe(oracle, path, tmp_path, self.rays, culling=culling)
            else:
                self._probe = (np.zeros(0, bool), np.zeros(0, f32))
        return self._probe

    def by_oracle(self, oracle, path, tmp_path, culling, radius):
        hit, t = self.probe(oracle, path, tmp_path, culling)
        return reduce(self.traced, self.pix, OC.expected(hit, t, f32(radius)), self.shape)

    def by_occluded(self, radius):
        import torch
        if len(self.rays):
            out = self.g.occluded(torch.from_numpy(self.rays).cuda(), float(radius))
            torch.cuda.synchronize()
            out = out.cpu().numpy()
        else:
            out = np.zeros(0, np.uint8)
        return reduce(self.traced, self.pix, out, self.shape)


def decoded_normals(exp):
    """N of util_aov.expected()'s frame decoded from the showNormals colour, (colour - 0.5) * 2: within an ulp or two of hitNormal, which
    is good enough for statistics and for nothing else."""
    return ((exp["normal_colour"].reshape(-1, 3) - f32(0.5)) * f32(2)).astype(f32)
