"""Scene files with an object moved: the reference's meaning of Scene.move_object (edit the object's [object] block, load again)."""
import numpy as np

KEYS = ("pos", "rot", "size", "radius", "normal")


def fmt(v):
    """A float32 value as text that parses back to the same float32."""
    return ",".join("%.9g" % x for x in np.asarray(v, np.float32).reshape(-1))


def edit_scene(text, index, **values):
    """`text` with object `index`'s keys set to `values` (None: unchanged); a key the block lacks goes right after its type= line
    (a mesh reads pos / rot / size before its name= line)."""
    lines = text.split("\n")
    starts = [i for i, l in enumerate(lines) if l.strip() == "[object]"]
    b = starts[index]
    e = next((i for i in range(b + 1, len(lines)) if lines[i].startswith("[")), len(lines))
    for k, v in values.items():
        if v is None:
            continue
        assert k in KEYS, k
        at = [i for i in range(b + 1, e) if lines[i].split("=")[0].strip() == k]
        if at:
            lines[at[0]] = "%s=%s" % (k, fmt(v))
        else:
            t = next(i for i in range(b + 1, e) if lines[i].startswith("type="))
            lines.insert(t + 1, "%s=%s" % (k, fmt(v)))
            e += 1
    return "\n".join(lines)


def write_scene(tmp_path, text, tag):
    p = tmp_path / ("moved_%s.scene" % tag)
    p.write_text(text)
    return str(p)


STRUCT = ("bounds", "skip", "leaf_begin", "leaf_count", "refs", "tris", "n_nodes", "n_leaves", "n_refs", "max_depth", "n_tris")


def same_structure(a, b):
    """bvh() of two scenes equal bit for bit (not build_ms / built_on_device)."""
    for k in STRUCT:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
                return k
        elif x != y:
            return k
    return None
