"""What rtx_radiance_points / Scene.radiance_points must write (include/rtx_radiance.h), restated in numpy float32.

Step 2 of the contract -- the colour of every ray {O, d_k} -- is an input here: from OracleScene.probe (tests/test_radiance_cpu.py) or from
Scene.trace_rays(colours=True) on the same scene object (tests/test_gpu_radiance.py); neither is the code under test.  rays() builds those
rays with the contract's roundings, reduce() restates steps 1, 3 and 4: products and sums are separate float32 roundings, and the loop
over the directions is sequential."""
import numpy as np

from tests import util_ao as AO

f32 = np.float32
BIAS = AO.BIAS


def cosines(N, dirs):
    """c [n, K] = N . d_k, summed x, y, z"""
    N = np.asarray(N, f32); dirs = np.asarray(dirs, f32)
    with np.errstate(all="ignore"):
        c = (N[:, 0:1] * dirs[None, :, 0] + N[:, 1:2] * dirs[None, :, 1]) + N[:, 2:3] * dirs[None, :, 2]
    assert c.dtype == f32
    return c


def rays(points, dirs, bias=BIAS):
    """All n x K rays {P + N * bias, d_k}, point-major ((n * K, 6): ray j * K + k is point j's direction k), traced or not, and the
    mask traced [n, K] of step 1."""
    points = np.ascontiguousarray(points, f32); dirs = np.asarray(dirs, f32)
    n, K = len(points), len(dirs)
    with np.errstate(all="ignore"):
        O = points[:, 0:3] + points[:, 3:6] * f32(bias)
        traced = cosines(points[:, 3:6], dirs) > 0
    assert O.dtype == f32
    out = np.empty((n, K, 6), f32)
    out[:, :, 0:3] = O[:, None, :]
    out[:, :, 3:6] = dirs[None, :, :]
    return out.reshape(n * K, 6), traced


def reduce(colours, N, dirs, weights=None, cosine=False):
    """Steps 1, 3 and 4: (sum float32 (n, 3), counts uint32 (n,)) from the colours (n, K, 3) of all n x K rays -- those of the rays
    that are not traced are not looked at."""
    colours = np.asarray(colours, f32); dirs = np.asarray(dirs, f32)
    n, K = colours.shape[0], len(dirs)
    assert colours.shape == (n, K, 3)
    c = cosines(N, dirs)
    traced = c > 0
    acc = np.zeros((n, 3), f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            w = np.full(n, f32(1.0) if weights is None else f32(weights[k]), f32)
            if cosine:
                w = w * c[:, k]
            term = colours[:, k, :] * w[:, None]
            acc = np.where(traced[:, k, None], acc + term, acc)
    assert acc.dtype == f32
    return acc, traced.sum(1).astype(np.uint32)


def reduce_scalar(colours, N, dirs, weights=None, cosine=False):
    """reduce() as a scalar Python loop over np.float32 values: one point and one component at a time"""
    colours = np.asarray(colours, f32); N = np.asarray(N, f32); dirs = np.asarray(dirs, f32)
    n, K = colours.shape[0], len(dirs)
    total = np.zeros((n, 3), f32)
    counts = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        for j in range(n):
            acc = [f32(0), f32(0), f32(0)]
            for k in range(K):
                c = f32(f32(N[j, 0] * dirs[k, 0]) + f32(N[j, 1] * dirs[k, 1])) + f32(N[j, 2] * dirs[k, 2])
                if not c > 0:
                    continue
                w = f32(1.0) if weights is None else f32(weights[k])
                if cosine:
                    w = f32(w * c)
                for a in range(3):
                    acc[a] = f32(acc[a] + f32(colours[j, k, a] * w))
                counts[j] += 1
            total[j] = acc
    return total, counts


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)
