"""The oracle's powf (powfRestated in oracle/rt_oracle.cpp, the yardstick of the device's powfRef) pinned to glibc 2.35's over the domains of
tests/util_device_math.py: 18 350 080 grid inputs (every exponent of x, both signs, against 35 values of y), seven sweeps of all 2^23 mantissas
and 294 912 inputs that vary y -- 77 365 248 in all.

Everywhere: the SHA-256 of the oracle's outputs per sub-domain equals the one tools/make_golden_powf.py took from glibc 2.35's libm (x86-64 FMA
variant) into tests/golden/powf_domain.json.  Where the host's glibc is 2.35, libm's powf is also called element by element and the first
difference reported.  The one known difference -- powf(signalling NaN, +-0): glibc x + y, the restatement 1 -- is asserted as it stands, so it
stays a documented limit and not a surprise: arithmetic never produces a signalling NaN, so no shading input is one.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from tests import util_device_math as DM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "powf_domain.json")


def libc_version():
    try:
        libc = ctypes.CDLL(None)
        libc.gnu_get_libc_version.restype = ctypes.c_char_p
        return libc.gnu_get_libc_version().decode()
    except (OSError, AttributeError):
        return None


def test_oracle_powf_matches_glibc_235_digests(oracle):
    doc = json.load(open(GOLDEN))
    names, total, wrong = [], 0, []
    for name, x, y in DM.powf_subdomains():
        names.append(name)
        total += x.size
        got = oracle.powf_n(x, y)
        if hashlib.sha256(DM.canonical(got).astype("<u4").tobytes()).hexdigest() != doc["sha256"].get(name):
            wrong.append(name)
    assert sorted(names) == sorted(doc["sha256"]), "the fixture's sub-domains are not the builders'"
    assert total == doc["elements"] == 77365248
    assert not wrong, "the oracle's powf differs from glibc 2.35's on %d sub-domains: %s" % (len(wrong), wrong[:8])


def test_oracle_powf_matches_this_libm_elementwise(oracle):
    """element by element, where this machine's libm is the restated one (elsewhere the digests above carry the same information)"""
    if libc_version() != "2.35":
        return
    for name, x, y in DM.powf_subdomains():
        msg = DM.first_difference(x, y, oracle.powf_n(x, y), oracle.libm_powf_n(x, y))
        assert msg is None, "%s: %s (second number: libm)" % (name, msg)


def test_signalling_nan_limit_is_as_documented(oracle):
    x, y = DM.signalling_nans()
    assert x.size == 8192 and np.isnan(x).all() and (DM.bits(x) & DM.QNAN_BIT == 0).all() and (y == 0).all()
    assert np.signbit(y).sum() == 4096
    assert (DM.bits(oracle.powf_n(x, y)) == 0x3f800000).all(), "the restatement returns 1 for a NaN to the power +-0"
    if libc_version() == "2.35":
        assert np.isnan(oracle.libm_powf_n(x, y)).all(), "glibc 2.35 returns x + y for a signalling NaN"
    # made quiet, as the grid holds them, the two agree again
    q = DM.quieted(DM.bits(x)).view(np.float32)
    assert (DM.bits(oracle.powf_n(q, y)) == 0x3f800000).all()
    if libc_version() == "2.35":
        assert (DM.bits(oracle.libm_powf_n(q, y)) == 0x3f800000).all()


def test_batch_call_is_the_scalar_call(oracle):
    """orc_powf_n is a loop over orc_powf: the same bits on a sample that visits every branch"""
    x = DM.grid_x()[::4099]
    for y in DM.Y_LIST:
        one = np.array([oracle.powf(float(a), float(y)) for a in x], np.float32)
        assert DM.same(one, oracle.powf_n(x, y)).all()
