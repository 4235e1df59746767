"""autocorr without a GPU: the reference's recorded outputs meet the
per-output bound (it is reachable), the segmented form the kernel uses meets
it, the running-sum form misses it (the checker is pinned), and the built
library exports the whole autocorr interface."""
import ctypes
import re

import numpy as np
import pytest

import autocorr_model as AM
import liquidmi as LQ

FIX = AM.load_fixture()
CASES = FIX["cases"]
# windows and delays of the issue's table, on a burst stream
FORMS = [("cccf", 1, 1), ("cccf", 33, 5), ("cccf", 64, 7), ("rrrf", 300, 16), ("cccf", 1000, 2048), ("rrrf", 64, 1)]
N_FORMS = 6000


def burst_stream(kind, W, d):
    env = AM.envelope("burst", N_FORMS, seams=(2048, 4096))
    return AM.noise(kind, env, 77 + 1000 * W + d)


def test_fixture_covers_the_cases():
    assert [(c["kind"], c["W"], c["d"], c["drive"]) for c in CASES] == AM.CASES
    assert all(c["n"] == AM.NOUT and len(c["y"]) == AM.NOUT for c in CASES)
    assert any(c["drive"] == "push" for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=AM.case_name)
def test_reference_meets_the_bound(c):
    x = AM.case_input(c)
    y64, A, _ = AM.reference64(c["kind"], c["W"], c["d"], x)
    AM.check("reference " + AM.case_name(c), c["kind"], c["W"], c["y"], y64, A)


@pytest.mark.parametrize("c", CASES, ids=AM.case_name)
def test_reference_energy(c):
    """get_energy of the reference is a running add and subtract
    (autocorr.c:123-127): within the bound of the float64 value, or this
    prints by how much it has drifted.  Nothing is asserted of the drift: the
    library computes the sum afresh and does not replay it."""
    x = AM.case_input(c)
    e64 = AM.reference64(c["kind"], c["W"], c["d"], x)[2][-1:]
    r = AM.report_e2(c["kind"], c["W"], np.array([c["energy"]], np.float32), e64)
    if r["failing"]:
        print("autocorr %s: the reference's energy %.9g against %.9g in float64: drifted to %.4g x the bound"
              % (AM.case_name(c), c["energy"], e64[0], r["worst"]))
    else:
        print("autocorr %s: the reference's energy is within the bound (%.4g of it)" % (AM.case_name(c), r["worst"]))
    assert np.isfinite(c["energy"])


@pytest.mark.parametrize("kind,W,d", FORMS)
def test_segmented_form_meets_the_bound(kind, W, d):
    x = burst_stream(kind, W, d)
    y64, A, _ = AM.reference64(kind, W, d, x)
    AM.check("direct32 %s W=%d d=%d" % (kind, W, d), kind, W, AM.direct32(kind, W, d, x), y64, A)
    AM.check("segmented32 %s W=%d d=%d" % (kind, W, d), kind, W, AM.segmented32(kind, W, d, x), y64, A)


@pytest.mark.parametrize("c", CASES, ids=AM.case_name)
def test_segmented_form_on_fixture_streams(c):
    x = AM.case_input(c)
    y64, A, _ = AM.reference64(c["kind"], c["W"], c["d"], x)
    AM.check("segmented32 " + AM.case_name(c), c["kind"], c["W"], AM.segmented32(c["kind"], c["W"], c["d"], x), y64, A)


@pytest.mark.parametrize("kind,W,d", [("cccf", 64, 7), ("rrrf", 300, 16)])
def test_running_sum_misses_the_bound(kind, W, d):
    """add the newest product, subtract the oldest: the rounding error of the
    first burst stays in every later output, so most of the stream fails"""
    x = burst_stream(kind, W, d)
    y64, A, _ = AM.reference64(kind, W, d, x)
    r = AM.report(kind, W, AM.running32(kind, W, d, x), y64, A)
    print("autocorr running sum %s W=%d d=%d: worst %.4g x the bound, %d of %d outputs fail"
          % (kind, W, d, r["worst"], r["failing"], r["n"]))
    assert r["failing"] > r["n"] // 2


def test_library_exports_the_interface():
    """every autocorr_{cccf,rrrf}_* function the header declares, and the two
    getters, by a ctypes lookup in the built library"""
    names = [n for n in LQ.header_functions() if re.match(r"autocorr_(cccf|rrrf)_", n)]
    want = ["create", "destroy", "reset", "print", "push", "execute", "execute_block", "get_energy",
            "execute_block_dev", "device_eligible", "set_stream", "synchronize"]
    assert sorted(names) == sorted("autocorr_%s_%s" % (t, w) for t in ("cccf", "rrrf") for w in want)
    L = ctypes.CDLL(LQ.LIB_PATH)
    for n in names + ["liquid_mi355x_autocorr_tile", "liquid_mi355x_autocorr_max_window"]:
        assert hasattr(L, n), n
    L.liquid_mi355x_autocorr_tile.restype = ctypes.c_uint
    L.liquid_mi355x_autocorr_max_window.restype = ctypes.c_uint
    assert L.liquid_mi355x_autocorr_tile() >= 64
    assert L.liquid_mi355x_autocorr_max_window() >= 4096
