"""Helpers of tests/test_gpu_views_aov.py: the batches of rtx_render_views_aov / Scene.render_views_aov in pre-filled buffers, the yardstick
-- resize + set_camera + render_aov per view on a second scene of the same file --, the comparison on the written pixels with the sentinel
everywhere else, and the closure on the ray queries (trace_rays, surface_rays, render_views).  The one-view expectations and masks are
tests/util_aov.py's."""
import numpy as np
import torch

from tests import util_aov as U

# (width, height) and poses relative to the scene's own camera: those of tests/test_gpu_render_views.py -- a tile and less, views without a
# rendered pixel, no multiples of 8, a wide and a tall view, several tiles each way; the two 64 x 48 views also share their pose
SIZES = [(7, 5), (1, 1), (2, 2), (41, 27), (200, 8), (8, 200), (64, 48), (64, 48), (33, 17), (96, 64), (1, 40)]
POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), ((0.15, 0.1, 0.2), (-4.0, 9.0, 2.0)), ((-0.3, 0.25, 0.4), (3.0, -14.0, -1.0)), ((0.0, 0.6, -0.5), (-25.0, 0.0, 0.0)),
         ((0.1, 0.0, 0.3), (0.0, 35.0, 0.0)), ((-0.2, 0.1, 0.1), (10.0, -30.0, 5.0)), ((0.05, 0.2, 0.6), (-6.0, 4.0, 0.0)), ((0.05, 0.2, 0.6), (-6.0, 4.0, 0.0)),
         ((0.3, 0.3, 0.0), (-12.0, 20.0, -8.0)), ((0.0, 0.1, 0.8), (2.0, -3.0, 1.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]

CHANNELS = U.CHANNELS + ("position", "rays")          # the call's eight, in the header's order
GEOMETRY = U.GEOMETRY + ("rays",)                     # no surface fetch
TAIL = {"depth": (), "object_id": (), "triangle_id": (), "uv": (2,), "normal": (3,), "albedo": (3,), "position": (3,), "rays": (6,)}
FILL_F, FILL_I = 7.25, 0x0BADF00D                     # (a finite float: a sentinel ray is still a ray trace_rays takes)


def integer(c):
    return c.endswith("_id")


def fill_of(c):
    return np.int32(FILL_I) if integer(c) else np.float32(FILL_F)


def cams_of(g, poses=POSES):
    base = g.camera_pose()
    return [(tuple(float(x) for x in base[0] + np.float32(p)), tuple(float(x) for x in base[1] + np.float32(r))) for p, r in poses]


def new(shape, c):
    return torch.full(shape + TAIL[c], FILL_I if integer(c) else FILL_F, dtype=torch.int32 if integer(c) else torch.float32, device="cuda")


def batch(g, cams, sizes, names=CHANNELS, keep=False):
    """One call over lists of pre-filled tensors: per view {channel: numpy frame}; with keep also the device tensors, {channel: [tensor]}."""
    bufs = {c: [new((h, w), c) for w, h in sizes] for c in names}
    g.render_views_aov(cams, **bufs)
    torch.cuda.synchronize()
    got = [{c: bufs[c][i].cpu().numpy() for c in names} for i in range(len(sizes))]
    return (got, bufs) if keep else got


def batch_whole(g, cams, w, h, names=CHANNELS):
    """One call over one (N, H, W[, c]) tensor per channel: per view {channel: numpy frame}"""
    bufs = {c: new((len(cams), h, w), c) for c in names}
    g.render_views_aov(cams, **bufs)
    torch.cuda.synchronize()
    host = {c: bufs[c].cpu().numpy() for c in names}
    return [{c: host[c][i] for c in names} for i in range(len(cams))]


def loop(ra, path, cams, sizes, names=U.CHANNELS, setup=None):
    """The yardstick: every view through resize + set_camera + render_aov on a scene of its own (setup(scene): the edits and flags it gets
    first).  Per view {channel: numpy frame}; None for a view under 2 x 2, which the one-view call does not take and which has no pixel."""
    g = ra.Scene(path, 16, 16)
    if setup:
        setup(g)
    out = []
    for (pos, rot), (w, h) in zip(cams, sizes):
        if w < 2 or h < 2:
            out.append(None)
            continue
        g.resize(w, h)
        g.set_camera(pos, rot)
        bufs = {c: new((h, w), c) for c in names}
        g.render_aov(**bufs)
        torch.cuda.synchronize()
        out.append({c: bufs[c].cpu().numpy() for c in names})
    g.close()
    return out


def differing(a, b, mask):
    """pixels of `mask` whose bits differ between two frames of one channel"""
    d = U.bits(a) != U.bits(b)
    d = d.any(-1) if d.ndim == 3 else d
    return int(d[mask].sum())


def touched(a, c, mask):
    """pixels outside `mask` of the frame a of channel c that no longer hold the sentinel"""
    keep = a == fill_of(c)
    keep = keep.all(-1) if keep.ndim == 3 else keep
    return int((~keep[~mask]).sum())


def compare(got, want, sizes, names, label):
    """Every view of `got` equals `want` bit for bit on the pixels the call writes (channels `names`), and every channel `got` has holds
    its sentinel everywhere else -- all of a view under 2 x 2."""
    for i, (w, h) in enumerate(sizes):
        mask = U.written_mask(w, h)
        for c in got[i]:
            n = touched(got[i][c], c, mask)
            assert n == 0, "%s view %d (%d x %d) %s: %d pixels outside the written ones were touched" % (label, i, w, h, c, n)
        if want[i] is None:
            assert not mask.any()
            continue
        for c in names:
            n = differing(got[i][c], want[i][c], mask)
            assert n == 0, "%s view %d (%d x %d) %s: %d pixels differ" % (label, i, w, h, c, n)
        if "depth" in names:      # (the yardstick wrote its pixels: no depth is the sentinel)
            assert (want[i]["depth"][mask] != fill_of("depth")).all(), "%s view %d: the yardstick left pixels unwritten" % (label, i)


def closure(g, got, rays_dev, sizes, cams=None, surface=True, label=""):
    """The batch's own channels against the ray queries on its `rays` channel (rays_dev: the device tensors of that channel, per view):
    trace_rays' hit records are depth / ids / uv, its colours render_views' framebuffer for the same cameras (when cams is given),
    surface_rays' channels are position / normal / albedo, and the origin is the camera's everywhere written."""
    fbs = None
    if cams is not None:
        fbs = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for w, h in sizes]
        g.render_views(cams, fbs)
    for i, (w, h) in enumerate(sizes):
        mask = U.written_mask(w, h)
        if not mask.any():
            continue
        r = rays_dev[i].reshape(-1, 6)
        hits, col = g.trace_rays(r, hits=True, colours=fbs is not None)
        torch.cuda.synchronize()
        hits = hits.cpu().numpy().reshape(h, w, 8)
        me = got[i]
        want = dict(depth=hits[..., 3], object_id=hits[..., 1].astype(np.int32), triangle_id=hits[..., 2].astype(np.int32), uv=np.ascontiguousarray(hits[..., 4:6]))
        if fbs is not None:
            n = differing(col.cpu().numpy().reshape(h, w, 3), fbs[i].cpu().numpy(), mask)
            assert n == 0, "%s view %d: %d colours of trace_rays(rays) differ from render_views" % (label, i, n)
        if surface:
            s = g.surface_rays(r, position=True, normal=True, albedo=True)
            torch.cuda.synchronize()
            want.update({c: s[c].cpu().numpy().reshape(h, w, 3) for c in ("position", "normal", "albedo")})
        for c, wv in want.items():
            if c in me:
                n = differing(me[c], np.ascontiguousarray(wv), mask)
                assert n == 0, "%s view %d (%d x %d) %s: %d pixels differ from the ray query on the batch's rays" % (label, i, w, h, c, n)
        if cams is not None:
            org = np.broadcast_to(np.asarray(g.view_target(cams[i][0], cams[i][1], cams[i][2] if len(cams[i]) == 3 else None, w, h).cam_pos[:], np.float32), (h, w, 3))
            assert differing(np.ascontiguousarray(me["rays"][..., :3]), np.ascontiguousarray(org), mask) == 0, "%s view %d: a ray does not start at the camera" % (label, i)
