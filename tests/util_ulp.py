"""Distances in units in the last place between float32 arrays, and the one tolerance of the suite: the reference's normal-map walk."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# The reference normalises a normal-map texel IN PLACE at every sample (objects.cpp:148): a 1-ulp random walk whose state depends on
# how often (and in which thread order) the texel was sampled before -- three pass 1s in one reference process differ from each other
# in ~500 of cfg4's 19 200 pixels, by up to 32 ulp.  The device and the oracle normalise the texel as loaded.  So where a
# normal map shows, the normals view is pinned to within that walk; everything else bit for bit.
NORMAL_MAP_ULP = 64


def ulp_diff(got, want):
    a = bits(got).view(np.int32).astype(np.int64); b = bits(want).view(np.int32).astype(np.int64)
    return np.abs(a - b).max(-1) if a.ndim > 1 else np.abs(a - b)
