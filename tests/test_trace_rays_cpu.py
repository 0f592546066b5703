"""Scene.trace_rays (rtx_trace_rays) without a GPU: the argument checks refuse what the device path cannot take, before any
GPU call, and the C entry point refuses a call without outputs."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

SCENE = "scenes/cfg1_simple_shapes.scene"


@pytest.fixture(scope="module")
def scene(ra):
    s = ra.Scene(SCENE, 32, 32)
    yield s
    s.close()


@pytest.mark.parametrize("rays,what", [
    (lambda: [[0.0] * 6], "torch tensor"),
    (lambda: torch.zeros((4, 6), dtype=torch.float64), "float32"),
    (lambda: torch.zeros((4, 6), dtype=torch.float16), "float32"),
    (lambda: torch.zeros((4, 5), dtype=torch.float32), r"shape \(n, 6\)"),
    (lambda: torch.zeros((24,), dtype=torch.float32), r"shape \(n, 6\)"),
    (lambda: torch.zeros((2, 4, 6), dtype=torch.float32), r"shape \(n, 6\)"),
    (lambda: torch.zeros((6, 8), dtype=torch.float32).t(), "contiguous"),
    (lambda: torch.zeros((8, 12), dtype=torch.float32)[:, ::2], "contiguous"),
    (lambda: torch.zeros((6, 8), dtype=torch.float32)[:, :6], "contiguous"),
    (lambda: torch.zeros((4, 6), dtype=torch.float32), "cuda:0"),
    (lambda: torch.zeros((0, 6), dtype=torch.float32), "cuda:0"),
], ids=["list", "float64", "float16", "n5", "flat", "3d", "transposed", "strided", "sliced", "host", "host_empty"])
def test_bad_rays_are_refused_before_the_gpu(scene, rays, what):
    with pytest.raises(ValueError, match=what):
        scene.trace_rays(rays())
    assert scene._gpu is None              # (the scene was never flattened and uploaded: no GPU call was made)


def test_no_output_is_refused(scene):
    with pytest.raises(ValueError, match="nothing to compute"):
        scene.trace_rays(torch.zeros((4, 6), dtype=torch.float32), hits=False, colours=False)
    assert scene._gpu is None


def test_c_entry_refuses_missing_arguments(ra):
    rtx, _ = ra.load()
    assert rtx.rtx_trace_rays(None, 4, None, None, None, None) == -1      # RTX_ERR_ARG: no scene
    assert b"NULL" in rtx.rtx_last_error()
