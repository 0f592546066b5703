"""Scene files with their object list edited: the reference's meaning of Scene.add_object / remove_object (write or delete an [object]
block, load again), and the read-backs an object edit is checked through."""
import numpy as np

# the order Scene.add_object applies an object's keys in (a mesh's OBJ is placed with the pos, size and rot read before its name)
ORDER = ("pos", "size", "rot", "color", "material", "radius", "normal", "name", "diffuse_map", "normal_map", "specular_map")
KEYS = {"sphere": ("pos", "color", "material", "radius"), "plane": ("pos", "color", "material", "normal"),
        "mesh": ("pos", "size", "rot", "color", "material", "name", "diffuse_map", "normal_map", "specular_map")}
TEXT = ("material", "name", "diffuse_map", "normal_map", "specular_map")


def fmt(v):
    """A float32 value as text that parses back to the same float32."""
    return ",".join("%.9g" % x for x in np.asarray(v, np.float32).reshape(-1))


def _blocks(lines):
    """[begin, end) of every [object] block, in file order"""
    out = []
    for b in (i for i, l in enumerate(lines) if l.strip() == "[object]"):
        out.append((b, next((i for i in range(b + 1, len(lines)) if lines[i].startswith("[")), len(lines))))
    return out


def n_objects(text):
    return len(_blocks(text.split("\n")))


def object_type(text, index):
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    return next(l.split("=", 1)[1].strip() for l in lines[b + 1:e] if l.startswith("type="))


def mesh_objects(text):
    """the indices of the mesh objects, in file order (mesh m of the scene is object mesh_objects(text)[m])"""
    return [i for i in range(n_objects(text)) if object_type(text, i) == "mesh"]


def add_object(text, kind, at=None, **keys):
    """`text` with a new [object] block before object `at`'s (None: after the last one; before [end] when there is none)."""
    lines = text.split("\n")
    blocks = _blocks(lines)
    assert all(k in KEYS[kind] for k in keys), (kind, sorted(keys))
    if at is not None and at < len(blocks):
        where = blocks[at][0]
    elif blocks:
        where = blocks[-1][1]
    else:
        where = next((i for i, l in enumerate(lines) if l.strip() == "[end]"), len(lines))
    new = ["[object]", "type=%s" % kind] + ["%s=%s" % (k, keys[k] if k in TEXT else fmt(keys[k])) for k in ORDER if k in keys] + [""]
    return "\n".join(lines[:where] + new + lines[where:])


def remove_object(text, index):
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    return "\n".join(lines[:b] + lines[e:])


def apply_step(scene, text, step):
    """One step of an edit sequence on a live Scene and on its scene text: ("add", type, at, keys) or ("remove", index).  Returns the new text."""
    if step[0] == "add":
        _, kind, at, keys = step
        index = scene.add_object(kind, at, **keys)
        before = n_objects(text)
        text = add_object(text, kind, at, **keys)
        assert index == (before if at is None else at) and scene.n_objects == n_objects(text) == before + 1
        return text
    assert step[0] == "remove"
    scene.remove_object(step[1])
    text = remove_object(text, step[1])
    assert scene.n_objects == n_objects(text)
    return text


def write_scene(tmp_path, text, tag):
    p = tmp_path / ("objects_%s.scene" % tag)
    p.write_text(text)
    return str(p)


# the blocks the sequences add
BUMPY = dict(pos=(0.9, -0.2, -3.4), size=(1.3, 1.3, 1.3), rot=(10, 25, 0), color=(0.9, 0.8, 0.6), name="scenes/assets/bumpy_4k.obj")
TORUS_MAPS = dict(pos=(-1.1, 0.3, -3.6), size=(1.7, 1.7, 1.7), rot=(35, 20, 0), color=(1, 1, 1), name="scenes/assets/torus_1536.obj",
                  diffuse_map="scenes/assets/diffuse_256.bmp", normal_map="scenes/assets/normal_256.bmp", specular_map="scenes/assets/specular_256.bmp")
TORUS_GLASS = dict(pos=(1.2, 0.2, -2.6), size=(1.5, 1.5, 1.5), rot=(60, 0, 20), color=(1, 1, 1), material="transparent,1.3",
                   name="scenes/assets/torus_1536.obj")
LONG_PLANE = dict(pos=(0, 0, -9), normal=(0, 0, 2.5), color=(0.6, 0.7, 0.6))
