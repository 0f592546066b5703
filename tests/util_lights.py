"""Scene files with their lights edited: the reference's meaning of Scene.set_light / add_light / remove_light (rewrite, append or delete a
[light] block, load again), and the read-backs a light edit is checked through."""
import ctypes as C

import numpy as np

KEYS = {"point": ("position", "color", "intensity"), "distant": ("direction", "color", "intensity"),
        "area": ("pos", "i", "j", "samples", "color", "intensity")}


def fmt(v):
    """A float32 value as text that parses back to the same float32."""
    return ",".join("%.9g" % x for x in np.asarray(v, np.float32).reshape(-1))


def _value(k, v):
    return "%d" % int(v) if k == "samples" else fmt(v)


def _blocks(lines):
    """[begin, end) of every [light] block, in file order"""
    out = []
    for b in (i for i, l in enumerate(lines) if l.strip() == "[light]"):
        out.append((b, next((i for i in range(b + 1, len(lines)) if lines[i].startswith("[")), len(lines))))
    return out


def light_type(text, index):
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    return next(l.split("=", 1)[1].strip() for l in lines[b + 1:e] if l.startswith("type="))


def n_lights(text):
    return len(_blocks(text.split("\n")))


def set_light(text, index, **values):
    """`text` with the keys of light `index`'s block set to `values`; a key the block lacks goes to its end."""
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    kind = light_type(text, index)
    for k, v in values.items():
        assert k in KEYS[kind], (kind, k)
        at = [i for i in range(b + 1, e) if lines[i].split("=")[0].strip() == k]
        if at:
            lines[at[0]] = "%s=%s" % (k, _value(k, v))
        else:
            last = max(i for i in range(b, e) if lines[i].strip())       # (before the blank lines that close the block)
            lines.insert(last + 1, "%s=%s" % (k, _value(k, v)))
            e += 1
    return "\n".join(lines)


def add_light(text, kind, **values):
    """`text` with a new [light] block after the last one (before the first [object] block when there is no light)."""
    lines = text.split("\n")
    blocks = _blocks(lines)
    if blocks:
        at = blocks[-1][1]
    else:
        at = next(i for i, l in enumerate(lines) if l.strip() in ("[object]", "[end]"))
    assert all(k in KEYS[kind] for k in values), (kind, sorted(values))
    new = ["[light]", "type=%s" % kind] + ["%s=%s" % (k, _value(k, v)) for k, v in values.items()] + [""]
    return "\n".join(lines[:at] + new + lines[at:])


def remove_light(text, index):
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    return "\n".join(lines[:b] + lines[e:])


def replace_light(text, index, kind, **values):
    """`text` with light `index`'s block replaced by one of another type, at the same place in the light order."""
    lines = text.split("\n")
    b, e = _blocks(lines)[index]
    assert all(k in KEYS[kind] for k in values), (kind, sorted(values))
    new = ["[light]", "type=%s" % kind] + ["%s=%s" % (k, _value(k, v)) for k, v in values.items()] + [""]
    return "\n".join(lines[:b] + new + lines[e:])


def apply_step(scene, text, step):
    """One step of an edit sequence on a live Scene and on its scene text: ("set", index, keys), ("add", type, keys) or ("remove", index).
    Returns the new text."""
    if step[0] == "set":
        scene.set_light(step[1], **step[2])
        return set_light(text, step[1], **step[2])
    if step[0] == "add":
        at = scene.add_light(step[1], **step[2])
        text = add_light(text, step[1], **step[2])
        assert at == n_lights(text) - 1 == scene.n_lights - 1
        return text
    assert step[0] == "remove"
    scene.remove_light(step[1])
    return remove_light(text, step[1])


def write_scene(tmp_path, text, tag):
    p = tmp_path / ("lights_%s.scene" % tag)
    p.write_text(text)
    return str(p)


def serialized(ra, scene):
    """The scene's description as rtx_desc_serialize's byte string (every scalar and array rtx_scene_create reads, area points included)."""
    rtx, host = ra.load()
    flat = C.c_void_p(host.rah_flatten(scene.h))
    try:
        desc = C.c_void_p(host.rah_flat_desc(flat))
        rtx.rtx_desc_serialize.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        need = C.c_size_t(0)
        assert rtx.rtx_desc_serialize(desc, None, 0, C.byref(need)) == 0
        buf = np.zeros(need.value, np.uint8)
        assert rtx.rtx_desc_serialize(desc, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(need)) == 0
        return buf.tobytes()
    finally:
        host.rah_flat_free(flat)
