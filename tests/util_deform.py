"""OBJ files with their vertices replaced: the reference's meaning of Scene.set_vertices (write the new v / vn lines, load again), a few
deformations in float32, and small hand-written meshes for the loader's quirks."""
import os

import numpy as np

from tests.util_move import fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tag(line):
    """The loader's tag of a line: the first blank-delimited word of its content before a '#'."""
    w = line.split("#", 1)[0].split()
    return w[0] if w else ""


def rewrite_obj(path_in, path_out, V, N=None):
    """path_in with its v lines replaced by the rows of V, in file order, and with N its vn lines by the rows of N; every value printed so
    that strtof gives the same float32 ("%.9g"), every other line byte for byte."""
    V = np.asarray(V, np.float32)
    N = None if N is None else np.asarray(N, np.float32)
    out, iv, inn = [], 0, 0
    with open(path_in, newline="") as f:
        for line in f:
            t = _tag(line)
            if t == "v":
                out.append("v " + fmt(V[iv]).replace(",", " ") + "\n")
                iv += 1
            elif t == "vn" and N is not None:
                out.append("vn " + fmt(N[inn]).replace(",", " ") + "\n")
                inn += 1
            else:
                out.append(line)
    assert iv == len(V) and (N is None or inn == len(N)), "the file has %d v and %d vn lines" % (iv, inn)
    with open(path_out, "w", newline="") as f:
        f.write("".join(out))
    return str(path_out)


def mesh_name(text, index):
    """The name= value of object `index`'s block."""
    lines = text.split("\n")
    b = [i for i, l in enumerate(lines) if l.strip() == "[object]"][index]
    e = next((i for i in range(b + 1, len(lines)) if lines[i].startswith("[")), len(lines))
    return next(lines[i].split("=", 1)[1].strip() for i in range(b + 1, e) if lines[i].split("=")[0].strip() == "name")


def set_mesh_name(text, index, path):
    """`text` with object `index`'s name= pointing at `path` (the loader opens the value as given: an absolute path works)."""
    lines = text.split("\n")
    b = [i for i, l in enumerate(lines) if l.strip() == "[object]"][index]
    e = next((i for i in range(b + 1, len(lines)) if lines[i].startswith("[")), len(lines))
    at = next(i for i in range(b + 1, e) if lines[i].split("=")[0].strip() == "name")
    lines[at] = "name=%s" % path
    return "\n".join(lines)


def deformed_scene(ra, tmp_path, text, index, V, N, tag, w=64, h=48):
    """A fresh Scene of `text` whose object `index` reads its OBJ file rewritten with V (and N: raw normals, None = the file's own)."""
    src = mesh_name(text, index)
    obj = rewrite_obj(src if os.path.isabs(src) else os.path.join(ROOT, src), tmp_path / ("deformed_%s.obj" % tag), V, N)
    p = tmp_path / ("deformed_%s.scene" % tag)
    p.write_text(set_mesh_name(text, index, obj))
    return ra.Scene(str(p), w, h), str(p)


# ---- deformations (float32 in, float32 out) ----------------------------------------------------
def bulge(P, amp=0.15, k=3.0, keep_y=False):
    P = np.asarray(P, np.float32)
    d = (np.float32(amp) * np.sin(np.float32(k) * P[:, [1, 2, 0]])).astype(np.float32)
    if keep_y:
        d[:, 1] = 0
    return (P + d).astype(np.float32)


def scale(P, s=(1.3, 0.7, 1.1)):
    return (np.asarray(P, np.float32) * np.float32(s)).astype(np.float32)


def twist(P, rate=0.8):
    """Rotation about y by rate * y (y itself stays)."""
    P = np.asarray(P, np.float32)
    a = np.float32(rate) * P[:, 1]
    c, s = np.cos(a).astype(np.float32), np.sin(a).astype(np.float32)
    return np.stack([c * P[:, 0] + s * P[:, 2], P[:, 1], c * P[:, 2] - s * P[:, 0]], 1).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- hand-written meshes for the loader's quirks -----------------------------------------------
SCENE = """[options]
width=64
height=48
ac_penalty=1

[light]
type=point
position=0,2,0
color=1,1,1
intensity=1.0

[object]
type=mesh
pos=0.1,0.2,-3
size=%s
rot=%s
color=1,1,1
name=%s

[end]
"""

QUIRKS = {
    # vertices and normals declared after the first face stay unplaced (and unrotated)
    "late": """v 0 0 0
v 1 0 0
v 0 1 0.5
vn 0 0 2
vn 0 3 0
vn 1 0 0
f 1//1 2//2 3//3
v 0.3 0.4 2.0
vn 0 5 5
f 1//1 3//3 4//4
f 2//2 4//4 3//1
""",
    # wholly at negative coordinates: objHi stays FLT_MIN
    "negative": """v -1 -2 -3
v -2 -2.5 -3.5
v -1.5 -4 -5
v -3 -2.25 -4
f 1 2 3
f 1 3 4
""",
    # zero uv determinants: every uv the same (inf * 0 in both columns), and collinear uv (inf * 0 in one, inf in the other)
    "uvdet": """v 0 0 0
v 1 0 0
v 0 1 0
v 1 1 1
vt 0.5 0.5
vt 0.25 0.5
vt 0.75 0.5
vt 0 1
vn 0 0 1
f 1/1/1 2/1/1 3/1/1
f 2/1/1 4/2/1 3/3/1
f 1/1/1 4/4/1 2/2/1
""",
    # minima at zero
    "zeros": """v 0 0 0
v 1 0 0.5
v 0 2 0
v 0.5 1 1
f 1 2 3
f 2 4 3
""",
}


def quirk_scene(tmp_path, name, size="2,1.5,1", rot="20,30,10"):
    """(scene text, path of the OBJ file) of the hand-written mesh `name`."""
    obj = tmp_path / ("%s.obj" % name)
    obj.write_text(QUIRKS[name])
    return SCENE % (size, rot, str(obj)), str(obj)


def probe_cases(ra, tmp_path):
    """Every input the shared formulas are checked on (tests/test_deform_cpu.py against Mesh::place, tests/test_gpu_deform.py device against
    CPU): (label, topology, stored normals, vertices, raw normals or None, pose).  The torus in the three fit branches, the flat quad, the
    rotated mesh, the hand-written quirks with the NaN cases, and one ragged size: the torus without its last 5 faces (1531 triangles)."""
    cases = []

    def of(scene, idx, label, V=None, N=None, **pose):
        P0, N0 = scene.mesh_vertices(idx)
        p = scene.mesh_pose(idx)
        p.update({k: np.float32(v) for k, v in pose.items()})
        cases.append((label, scene.mesh_topology(idx), N0, P0 if V is None else V, N, p))
        return P0, N0

    g = ra.Scene("scenes/cfg4_textured_256.scene", 64, 48)
    P0, N0 = g.mesh_vertices(0)
    V = bulge(twist(P0, 0.4), 0.1, 2.5)
    for axis, size in enumerate(((0.5, 5.0, 5.0), (5.0, 0.2, 5.0), (5.0, 5.0, 0.5))):
        of(g, 0, "torus, fit branch %d" % axis, V, None, size=size, rot=(12, 100, -33))
        of(g, 0, "torus, fit branch %d, raw normals" % axis, V, (N0 * np.float32(2)).astype(np.float32), size=size, rot=(12, 100, -33))
    # the ragged size
    src = os.path.join(ROOT, "scenes", "assets", "torus_1536.obj")
    lines = open(src).read().split("\n")
    faces = [i for i, l in enumerate(lines) if _tag(l) == "f"]
    for i in faces[-5:]:
        lines[i] = ""
    ragged = tmp_path / "torus_ragged.obj"
    ragged.write_text("\n".join(lines))
    text = set_mesh_name(open(os.path.join(ROOT, "scenes", "cfg4_textured_256.scene")).read(), 0, str(ragged))
    p = tmp_path / "ragged.scene"
    p.write_text(text)
    r = ra.Scene(str(p), 64, 48)
    assert r.mesh_topology(0)["corner_pos"].shape[0] % 64 != 0
    of(r, 0, "ragged torus", scale(V, (1.1, 0.8, 1.2)))
    r.close(); g.close()
    g = ra.Scene("scenes/mixed_materials.scene", 64, 48)
    for idx in (0, 1, 2):
        P0, _ = g.mesh_vertices(idx)
        of(g, idx, "mixed_materials object %d" % idx, twist(scale(P0, (1.2, 1.0, 0.8)), 0.6))
    # a flat axis away from zero: placed NaN
    P0, _ = g.mesh_vertices(0)
    V = P0.copy(); V[:, 1] = 1
    of(g, 0, "flat axis at 1 (placed NaN)", V)
    g.close()
    for name in sorted(QUIRKS):
        text, _ = quirk_scene(tmp_path, name)
        p = tmp_path / ("probe_%s.scene" % name)
        p.write_text(text)
        q = ra.Scene(str(p), 64, 48)
        P0, N0 = q.mesh_vertices(0)
        of(q, 0, "quirk " + name, bulge(P0, 0.2, 1.5) if name != "zeros" else None)
        if N0.shape[0]:
            of(q, 0, "quirk %s, raw normals" % name, P0, (N0[::-1] * np.float32(3)).astype(np.float32))
        if name == "zeros":
            for order in ((np.float32(0), np.float32(-0.0)), (np.float32(-0.0), np.float32(0))):
                V = P0.copy()
                V[0, 0], V[2, 0] = order
                V[0, 2], V[2, 2] = order
                V[0, 1], V[1, 1] = order[::-1]
                of(q, 0, "quirk zeros, signs %s" % (np.signbit(order[0]),), V)
        q.close()
    return cases
