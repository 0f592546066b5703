"""Adversarial meshes for the device build (rtx_bvh.hip), the device flatten (rtx_flatten.hip) and the mesh walks (rtx_kernels.hip): one
seeded generator per family, each with a property of its tree that tests/test_adversarial_meshes_cpu.py asserts on the host builder and
the host flatten before tests/test_gpu_adversarial_meshes.py hands the family to a GPU.  A family has a raw form (triangles n x 9 float32
and a root box, for rtx_bvh_build / rtx_scene_update_mesh) and, unless it says otherwise, a scene form (OBJ text and the [object] keys it
is placed with).  tools/bvh_fuzz.py draws its shapes from fuzz_shape below.

Every coordinate here is finite with |x| <= 2^10 (COORD_MAX): the reference's split search halves an interval until it is narrower than
0.1 in absolute units (objects.cpp:676-689) and does not return for anything else.

Scene forms whose property needs exact coordinates are written in the unit cube, pinned by a small triangle touching (0, 0, 0) and one
touching (1, 1, 1) from inside, and placed with rot = 0, a power-of-two size and a power-of-two (or zero) pos: Mesh::place then computes
size * (x - 0.5) + pos without rounding anything but the last sum."""
import numpy as np

from tests.util_objects import add_object

f32 = np.float32
COORD_MAX = 2.0 ** 10
STACKS = (63, 64, 65, 127, 128, 129, 200)
SOUPS = (63, 64, 65, 1023, 1024, 1025, 1100)
W, H = 96, 72


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------

def fuzz_shape(kind, r, nt, ext):
    """The six shapes of tools/bvh_fuzz.py, nt triangles within about +-ext, drawn from the generator r: n x 9 float32."""
    if kind == 0:      # soup of small triangles
        c = r.uniform(-ext, ext, (nt, 1, 3)); tri = c + r.normal(0, ext * 0.02, (nt, 3, 3))
    elif kind == 1:    # clusters
        k = r.integers(1, 6); cent = r.uniform(-ext, ext, (k, 3)); c = cent[r.integers(0, k, nt)][:, None, :] + r.normal(0, ext * 0.05, (nt, 1, 3)); tri = c + r.normal(0, ext * 0.01, (nt, 3, 3))
    elif kind == 2:    # long slivers through the whole box
        a = r.uniform(-ext, ext, (nt, 3)); b = r.uniform(-ext, ext, (nt, 3)); tri = np.stack([a, b, a + r.normal(0, 1e-3, (nt, 3))], 1)
    elif kind == 3:    # many coincident triangles
        base = r.uniform(-ext, ext, (max(nt // 50, 1), 3, 3)); tri = base[r.integers(0, base.shape[0], nt)]
    elif kind == 4:    # flat: all in a plane (an axis of zero extent)
        c = r.uniform(-ext, ext, (nt, 1, 3)); tri = c + r.normal(0, ext * 0.03, (nt, 3, 3)); tri[:, :, int(r.integers(0, 3))] = 0.25
    else:              # a bumpy sheet (neighbours share vertices, like a mesh)
        m = int(np.ceil(np.sqrt(nt / 2))) + 1; u, v = np.meshgrid(np.linspace(-ext, ext, m), np.linspace(-ext, ext, m)); z = 0.2 * ext * np.sin(3 * u / ext) * np.cos(2 * v / ext)
        P = np.stack([u, z, v], -1); a = P[:-1, :-1]; b = P[:-1, 1:]; cc = P[1:, 1:]; d = P[1:, :-1]
        tri = np.concatenate([np.stack([a, b, cc], 2).reshape(-1, 3, 3), np.stack([a, cc, d], 2).reshape(-1, 3, 3)])[:nt]
    return np.ascontiguousarray(tri, np.float32).reshape(-1, 9)


def corner(p, lx, ly=None):
    """A right triangle in a plane z = const: its right angle at p, legs lx along x and ly along y (counter-clockwise seen from +z when
    both have the same sign)."""
    p = np.asarray(p, np.float64) * np.ones(3)
    ly = lx if ly is None else ly
    return np.array([p, p + [lx, 0, 0], p + [0, ly, 0]])


def pins():
    """The two triangles that pin an OBJ's bounds to the unit cube exactly."""
    return [corner(0.0, 2.0 ** -6), corner(1.0, -(2.0 ** -6))]


def obj_text(tris):
    """OBJ text of triangles (n x 3 x 3): every vertex before the first face (the loader places the vertices it has read when it meets
    the first face, like the reference); a triangle whose corners are one point is written `f a a a`.  %.9g: every float32 reads back as itself."""
    vs, fs = [], []
    for t in np.asarray(tris, np.float32).reshape(-1, 3, 3):
        point = (t[0] == t[1]).all() and (t[0] == t[2]).all()
        n = len(vs)
        vs += ["v %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in (t[:1] if point else t)]
        fs.append("f %d %d %d" % ((n + 1,) * 3 if point else (n + 1, n + 2, n + 3)))
    return "\n".join(vs + fs) + "\n"


def placed(tris, size, pos=(0, 0, 0)):
    """Mesh::place of unit-cube triangles with rot = 0 and a uniform size, in float32: (n x 9, root lo, root hi)."""
    t = np.asarray(tris, np.float32).reshape(-1, 3)
    s, p = f32(size), np.asarray(pos, np.float32)
    v = (s * (t - f32(0.5)) + p).astype(np.float32)
    return np.ascontiguousarray(v.reshape(-1, 9)), (p - s / f32(2)).astype(np.float32), (p + s / f32(2)).astype(np.float32)


# ---- the families -----------------------------------------------------------------------------------------------------------------------

def _few(n):
    if n == 1:
        return [np.array([[0, 0, 0], [1, 0, 1], [0, 1, 1]], np.float64)]
    if n == 9:         # crowded towards one corner: leaves one and two levels below the root
        spots = [(0.7, 0.7, 0.7), (0.85, 0.6, 0.8), (0.6, 0.85, 0.9), (0.9, 0.9, 0.6), (0.8, 0.75, 0.95), (0.3, 0.2, 0.1), (0.55, 0.9, 0.75)]
    else:              # spread out: a balanced tree
        spots = [(0.75, 0.25, 0.5), (0.25, 0.75, 0.25), (0.8, 0.8, 0.2), (0.2, 0.2, 0.8), (0.6, 0.4, 0.9)]
    return pins() + [corner(p, 0.09375) for p in spots[:n - 2]]


def _stack(k):
    return pins() + [np.array([[0.25, 0.25, 0.5], [0.75, 0.25, 0.5], [0.25, 0.75, 0.5]], np.float64)] * k


def _slivers(seed=2, n=300):
    r = np.random.default_rng(seed)
    a = r.uniform(0.02, 0.98, (n, 3)); b = r.uniform(0.02, 0.98, (n, 3))
    return pins() + list(np.stack([a, b, a + r.normal(0, 1e-3, (n, 3))], 1))


def _flat(n=12, lift=2.0 ** -16):
    """A grid in the plane y = 1/2.  The scene form lifts one corner by 2^-16: an OBJ without any extent in y is placed at 0 / 0, while
    one whose extent is below the scene's bias (1e-4) has every vertex put at pos.y exactly (Mesh::place), which is the plane again."""
    out = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = [(x / n, 0.5, z / n) for x, z in ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))]
            out += [np.array([a, c, b], np.float64), np.array([a, d, c], np.float64)]
    out[-1][1][1] += lift
    return out


def _degenerate(n=16):
    """A sheet on the lattice k / n with heights in multiples of 1 / 64; every fifth triangle collapsed to a point -- alternately its own
    first corner and a spot well above the sheet, where points are among themselves --, every fifth collinear (a, b and their midpoint)."""
    out, k = pins(), 0
    for j in range(n):
        for i in range(n):
            P = [np.array([x / n * 0.875 + 0.0625, 0.25 + ((3 * x + 5 * z) % 7) / 64.0, z / n * 0.875 + 0.0625]) for x, z in ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))]
            for t in ((P[0], P[2], P[1]), (P[0], P[3], P[2])):
                t = np.array(t)
                if k % 5 == 0:
                    p = t[0] if (k // 5) % 2 else np.array([t[0][0], 0.875, t[0][2]])
                    t = np.array([p, p, p])
                elif k % 5 == 2:
                    t = np.array([t[0], t[1], 0.5 * (t[0] + t[1])])
                out.append(t)
                k += 1
    return out


def _deep(n, m, leg):
    """For j = 2 .. n + 1 and d = 2^-j: m triangles at (1/2 + d) (1, 1, 1) with legs d leg (q + 1) / m, q < m; one at the centre with leg
    2^-(n + 3).  Placed in a box narrower than 0.1 every split is a midpoint, and every level peels one j off."""
    out = pins()
    for j in range(2, n + 2):
        d = 2.0 ** -j
        out += [corner(0.5 + d, d * leg * (q + 1) / m) for q in range(m)]
    out.append(corner(0.5, 2.0 ** -(n + 3)))
    return out


NEAR = dict(pos=(0, 0, -3), size=(2, 2, 2), rot=(0, 0, 0), color=(0.9, 0.8, 0.6))
SMALL = dict(pos=(0, 0, 0), size=(0.0625, 0.0625, 0.0625), rot=(0, 0, 0), color=(0.9, 0.8, 0.6))
DEEP = {"deep_edge": (11, 7, 0.9), "deep_over": (12, 8, 0.9)}
DEEP_WIDE = {"deep_edge": 10, "deep_over": 0}      # wide nodes: a chain of ten; none (eleven levels do not fit the walk's stack)
# family -> (unit-cube triangles, [object] keys, camera position, penalties of the GPU tests)
SCENE_FAMILIES = {}
for _name, _n in (("one", 1), ("two", 2), ("seven", 7), ("nine", 9)):
    SCENE_FAMILIES[_name] = (lambda n=_n: _few(n), NEAR, (0, 0, 0), (1,))
for _k in STACKS:
    SCENE_FAMILIES["stack_%d" % _k] = (lambda k=_k: _stack(k), NEAR, (0, 0, 0), (1, 3) if _k == 129 else (1,))
SCENE_FAMILIES["slivers"] = (_slivers, NEAR, (0, 0, 0), (1, 3))
SCENE_FAMILIES["flat"] = (_flat, dict(NEAR, pos=(0, -0.5, -3), size=(2, 0, 2)), (0, 0, 0), (1,))
SCENE_FAMILIES["degenerate"] = (_degenerate, NEAR, (0, 0, 0), (1,))
for _name, _a in DEEP.items():
    SCENE_FAMILIES[_name] = (lambda a=_a: _deep(*a), SMALL, (0, 0, 0.09375), (1,))
SCENE_NAMES = sorted(SCENE_FAMILIES)
# the moves of the live edits: a rotation with a non-uniform size for every family, and for the deep ones a step that only changes pos
TURN = dict(rot=(20, 30, 10), size=(1.5, 2.5, 2.0))
TURN_SMALL = dict(rot=(20, 30, 10), size=(0.046875, 0.078125, 0.0625))
SHIFT = dict(pos=(0.03125, 0, -0.0625))
CASES = [(name, cull, pen) for name in SCENE_NAMES for pen in SCENE_FAMILIES[name][3] for cull in (1, 0)]


def scene_triangles(name):
    """The unit-cube triangles of a scene family: n x 3 x 3 float32."""
    return np.asarray(SCENE_FAMILIES[name][0](), np.float32).reshape(-1, 3, 3)


def moves(name):
    """[(tag, move_object keys)] after the add_object of the live edits"""
    if name in DEEP:
        return [("shift", SHIFT), ("turn", TURN_SMALL)]
    return [("turn", TURN)]


def base_scene(name, cull=1, penalty=1):
    """One plane, a point light and a distant light, seen from the family's camera."""
    cam = SCENE_FAMILIES[name][2]
    far = 0.125 if name in DEEP else 1.5
    c = lambda v: ",".join("%r" % float(x) for x in v)
    return ("[options]\nwidth=%d\nheight=%d\nfov=60\nposition=%s\nuseBackfaceCulling=%d\nac_penalty=%d\nimage_name=output/adversarial\n\n"
            "[light]\ntype=point\nposition=%s\ncolor=1,0.8,0.6\nintensity=0.9\n\n[light]\ntype=distant\ndirection=0.3,-1,-0.4\ncolor=0.4,0.6,1\nintensity=0.5\n\n"
            "[object]\ntype=plane\npos=%s\nnormal=0,1,0\ncolor=1,1,1\n\n[end]\n") % (
        W, H, c(cam), cull, penalty, c((cam[0] + far, cam[1] + 2 * far, cam[2] - far / 2)), c((0, -far, 0)))


def mesh_keys(name, obj_path):
    return dict(SCENE_FAMILIES[name][1], name=str(obj_path))


def scene_form(name, dirpath, cull=1, penalty=1):
    """Writes the family's OBJ into dirpath; returns (the base scene's text, the add_object keys, the text with the mesh added: it is
    object 1)."""
    obj = dirpath / ("%s.obj" % name)
    obj.write_text(obj_text(scene_triangles(name)))
    keys = mesh_keys(name, obj)
    base = base_scene(name, cull, penalty)
    return base, keys, add_object(base, "mesh", None, **keys)


def _soup(n, seed):
    return fuzz_shape(0, np.random.default_rng(seed), n, 2.0)


def _tiny(seed=5):
    """A soup and eight triangles with edges of 1e-16 next to the origin: |e1|_1 |e2|_1 = 1e-32 spoils the plane bound of every slot above them."""
    t = [_soup(300, seed).reshape(-1, 3, 3)]
    for k in range(8):
        p = np.array([k % 2, (k // 2) % 2, k // 4], np.float64) * 1e-15
        t.append(corner(p, 1e-16)[None])
    return np.concatenate(t).astype(np.float32).reshape(-1, 9)


def raw_form(name):
    """(triangles n x 9 float32, root lo, root hi, penalties).  A scene family's raw form is its placement; a stack's is the stack alone."""
    if name.startswith("soup_"):
        t = _soup(int(name[5:]), int(name[5:]))
        return t, t.reshape(-1, 3).min(0) - f32(1e-3), t.reshape(-1, 3).max(0) + f32(1e-3), (1, 3)
    if name == "tiny":
        t = _tiny()
        return t, t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0), (1,)
    tris, keys, _, pens = SCENE_FAMILIES[name]
    tris = np.asarray(tris(), np.float32).reshape(-1, 3, 3)
    if name.startswith("stack_"):
        tris = tris[2:]
    if name in ("one", "flat"):          # (no unit cube to place: as written, in their own bounds; the plane without its lifted corner)
        t = np.ascontiguousarray((np.asarray(_flat(lift=0.0), np.float32) if name == "flat" else tris).reshape(-1, 9))
        return t, t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0), pens
    t, lo, hi = placed(tris, keys["size"][0], keys["pos"])
    if name.startswith("stack_"):
        lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    return t, lo, hi, pens


RAW_NAMES = SCENE_NAMES + ["tiny"] + ["soup_%d" % n for n in SOUPS]


# ---- what the properties are read from --------------------------------------------------------------------------------------------------

def links(wide):
    """link of every slot of the wide nodes (mesh_flatten_probe's first array): > 0 inner, < 0 leaf, 0 empty"""
    return np.ascontiguousarray(wide[:, :, 6]).view(np.int32)


def wide_levels(wide):
    """wide level of every wide node (the root's is 1) and, per wide node, the (node, slot) that links to it (the root: None)"""
    lk = links(wide)
    level, parent = np.zeros(len(wide), np.int32), [None] * len(wide)
    if len(wide):
        level[0] = 1
    for w in range(len(wide)):          # (pre-order: a parent comes before its children)
        for k in np.nonzero(lk[w] > 0)[0]:
            level[lk[w, k] - 1] = level[w] + 1
            parent[lk[w, k] - 1] = (w, int(k))
    return level, parent


def sizes(bvh, flat):
    """The numbers the summary lists: triangles, nodes, references, levels, wide nodes, wide levels, largest leaf."""
    lv = wide_levels(flat[0])[0]
    return dict(tris=len(bvh["tris"]) if "tris" in bvh else None, nodes=int(bvh["n_nodes"]), refs=int(bvh["n_refs"]), levels=int(bvh["max_depth"]),
                wide=len(flat[0]), wide_levels=int(lv.max()) if len(lv) else 0, largest_leaf=int(bvh["leaf_count"].max()))


def zero_edge(tris9):
    """per triangle: an edge a -> b or a -> c of length zero (the plane record skips it: s1 == 0 or s2 == 0)"""
    t = np.asarray(tris9, np.float32).reshape(-1, 3, 3)
    return (t[:, 1] == t[:, 0]).all(1) | (t[:, 2] == t[:, 0]).all(1)


def stack_hits(name, tree, hits):
    """(the rays whose hit record names the family's mesh, object 1, and a triangle of the stack; the stack's first triangle in leaf order)"""
    k = int(name[6:])
    leaf = int(np.nonzero(tree["leaf_count"] == k)[0][0])
    stack = tree["refs"][tree["leaf_begin"][leaf]:tree["leaf_begin"][leaf] + k]
    return (hits[:, 0] > 0) & (hits[:, 1] == 1) & np.isin(hits[:, 2].astype(np.int64), stack), int(stack[0])


def ray_seed(name):
    return 101 + SCENE_NAMES.index(name)


def aimed_rays(ray_families, tris9, seed, n_tri=24, n_waves=156):
    """The ray families of tests/test_gpu_margins.py at n_tri of these triangles, thinned to n_waves whole waves of 64 (about 10 000 rays)."""
    rng = np.random.default_rng(seed)
    rays = ray_families(np.asarray(tris9, np.float32), rng, n_tri).reshape(-1, 64, 6)
    if len(rays) > n_waves:
        rays = rays[np.sort(rng.choice(len(rays), n_waves, replace=False))]
    return np.ascontiguousarray(rays.reshape(-1, 6))
