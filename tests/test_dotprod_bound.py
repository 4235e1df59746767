"""tests/dotprod_bound.py on the CPU: the oracle meets the bound on every
batch the GPU tests run (the bound is reachable, zero rows give exact zeros),
the batches are what they say, the route table is the launch's own decision
with the pass counts of a capped grid, and the checker is pinned -- it fails
on the faults the GPU tests are there to catch, where the older normwise
criterion does not.  No GPU.
"""
import numpy as np
import pytest

import dotprod_bound as DB
import liquidmi as LQ

BATCH_ROWS = DB.LADDER_VEC + DB.LADDER_SCALAR
SMALL = 300   # rows of the small versions of the capped-grid batches


def _oracle_ok(c):
    r = c.check_bound(c.ref)
    assert r["worst"] == c.oracle_worst < 0.5   # room: a kernel at the bound is not this computation
    assert r["nonzero_zeros"] == 0
    z = c.rows("zero")
    assert len(z) and np.all(c.A[z] == 0) and np.all(c.ref[z] == 0)
    return r


@pytest.mark.parametrize("row", BATCH_ROWS, ids=DB.row_id)
def test_oracle_meets_the_bound_on_the_ladder(row):
    _oracle_ok(DB.case(row[0], row[1]))


@pytest.mark.parametrize("row", DB.CAPPED, ids=DB.row_id)
def test_oracle_meets_the_bound_on_small_capped_batches(row):
    _oracle_ok(DB.case(row[0], row[1], SMALL, tag="capped"))


@pytest.mark.parametrize("row", DB.LONG, ids=DB.row_id)
def test_oracle_meets_the_bound_on_one_long_row(row):
    c = DB.Case(row[0], row[1], 3, DB.LONG_PATTERN)
    r = _oracle_ok(c)
    assert list(c.cls) == ["full", "quiet", "zero"]
    assert r["worst"] < 1e-3   # the hard bound is loose here: the margin is what binds


@pytest.mark.parametrize("n", DB.SINGLE_LENGTHS)
@pytest.mark.parametrize("t", DB.KINDS)
def test_oracle_meets_the_bound_on_the_one_vector_batches(t, n):
    _oracle_ok(DB.case(t, n, DB.SINGLE_ROWS, tag="single"))


@pytest.mark.parametrize("t", DB.KINDS)
def test_no_samples_give_zeros(t):
    c = DB.case(t, 0, 40)
    assert c.X.shape == (40, 0) and np.all(c.A == 0) and np.all(c.ref == 0)
    assert c.report(c.ref)["failing"] == 0
    assert c.report(np.full(40, 1e-30, c.ref.dtype))["nonzero_zeros"] == 40


@pytest.mark.parametrize("t,n", [("rrrf", 6), ("crcf", 16), ("cccf", 16), ("cccf", 1), ("cccf", 1024)])
def test_batches_are_what_they_say(t, n):
    c = DB.case(t, n)
    assert c.nvec == DB.NVEC and c.period == 7 == DB.PERIOD
    assert all(64 // G % c.period != 0 and c.period % (64 // G) != 0 for G in (1, 2, 4, 8, 16))
    assert all(DB.NVEC % (256 // G) != 0 for G in (1, 2, 4, 8, 16))
    # any 4 consecutive rows -- a wave at G = 16, part of one at a smaller G -- hold the first three classes
    for a in range(0, 2 * c.period):
        assert {"full", "quiet", "zero"} <= set(c.cls[a:a + 4])
    full, quiet, zero, cancel = (c.rows(k) for k in ("full", "quiet", "zero", "cancel"))
    assert len(full) + len(quiet) + len(zero) + len(cancel) == c.nvec
    assert np.all(c.X[zero] == 0)
    assert 0 < np.max(np.abs(c.X[quiet])) <= 0.5 * np.sqrt(2) * DB.QUIET
    assert np.max(np.abs(c.X[full])) > 0.4 and abs(c.h[n - 1]) >= 0.25
    if n == 1:
        assert len(cancel) == 0
    else:   # |y64| << A: the bound scales with A, not with |y|
        assert len(cancel) in (c.nvec // 7, c.nvec // 7 + 1)
        assert np.all(np.abs(c.y64[cancel]) < 2.0 ** -22 * c.A[cancel])
        assert np.median(np.abs(c.y64[full]) / c.A[full]) > 0.01
    # the last RAGGED rows of any batch hold a quiet, a zero and a cancelling row
    assert {"quiet", "zero", "cancel"} <= set(DB.row_classes(16, 10 ** 6 + DB.RAGGED)[-DB.RAGGED:])


# ------------------------------------------------------------------ routes
def test_route_table_is_the_launch_decision():
    cap = LQ.dotprod_block_cap()
    assert cap >= 1
    for t, n, kernel, G in DB.LADDER_VEC + DB.LADDER_SCALAR:
        assert LQ.dotprod_route(t, n, True, DB.NVEC) == (kernel, G, 1), (t, n)
    # every rung of both kernels is walked
    assert {(r[2], r[3]) for r in BATCH_ROWS} == {(k, G) for k in ("vec", "scalar") for G in (1, 2, 4, 8, 16)}
    # work 64 is the last under gmax = 16; even rrrf lengths that are no multiple of 4 are scalar
    assert LQ.dotprod_route("cccf", 128, True, DB.NVEC)[:2] == ("vec", 8)
    assert LQ.dotprod_route("cccf", 130, True, DB.NVEC)[:2] == ("vec", 16)
    for n in (2, 6, 130):
        assert LQ.dotprod_route("rrrf", n, True, DB.NVEC)[0] == "scalar"
    for t, n, off, G in DB.UNALIGNED:
        assert off % 16 and LQ.dotprod_route(t, n, True, DB.NVEC)[0] == "vec"
        assert LQ.dotprod_route(t, n, False, DB.NVEC) == ("scalar", G, 1), (t, n)
    for t, n, kernel, G in DB.CAPPED:
        for passes in (2, 3):
            nvec = DB.capped_nvec(cap, G, passes)
            assert LQ.dotprod_route(t, n, True, nvec) == (kernel, G, passes), (t, n, passes)
            # one whole pass fewer is exact; the ragged rows alone make the next
            assert LQ.dotprod_route(t, n, True, nvec - DB.RAGGED)[2] == passes - 1
            assert LQ.dotprod_route(t, n, True, nvec - DB.RAGGED + 1)[2] == passes
    for t, n, kernel, G in DB.LONG:
        assert LQ.dotprod_route(t, n, True, 3) == (kernel, G, 1), (t, n)
    for t in DB.KINDS:
        assert LQ.dotprod_route(t, 0, True, 40)[1:] == (1, 1)
    assert LQ.lib().liquid_mi355x_dotprod_route(3, 16, 1, 1) == -1   # no such kind


def test_staging_seams_come_from_the_library():
    pin, out = LQ.pinned_input_max(), LQ.copyout_max()
    # whole cccf n = 16 rows either side of both seams, and the result seam needs a DMA input
    assert pin % (16 * 8) == 0 and out % 8 == 0
    assert out // 8 * 16 * 8 > pin


# ------------------------------------------------------------- the checker, pinned
def _fails(c, z, failing=None):
    r = c.report(z)
    with pytest.raises(AssertionError):
        c.check_bound(z)
    if failing is not None:
        assert r["failing"] == failing
    return r


def test_checker_fails_on_a_neighbour_row_leaking_into_quiet_rows():
    """(a) 2^-22 of the full-scale row before it: invisible normwise."""
    c = DB.case("cccf", 16)
    z = DB.leak_into_quiet(c, c.ref)
    assert DB.normwise(z, c.ref) < DB.NRM
    _fails(c, z, len(c.rows("quiet")))


def test_checker_fails_on_tiny_values_in_zero_rows():
    """(b)"""
    c = DB.case("cccf", 16)
    z = DB.tiny_zero_rows(c, c.ref)
    assert DB.normwise(z, c.ref) < DB.NRM
    r = _fails(c, z, len(c.rows("zero")))
    assert r["nonzero_zeros"] == len(c.rows("zero"))


def test_checker_fails_on_quiet_rows_the_ragged_last_pass_left_out():
    """(c) at the size the GPU runs: one full pass of a capped grid and 37 rows."""
    t, n, kernel, G = DB.CAPPED[1]
    nvec = DB.capped_nvec(LQ.dotprod_block_cap(), G, 2)
    assert LQ.dotprod_route(t, n, True, nvec) == (kernel, G, 2)
    c = DB.Case(t, n, nvec)
    _oracle_ok(c)
    first = nvec - DB.RAGGED
    left = np.count_nonzero(c.cls[first:] == "quiet")
    assert left >= 5
    z = DB.drop_quiet_of_last_pass(c, c.ref, first)
    assert DB.normwise(z, c.ref) < DB.NRM
    r = _fails(c, z, left)
    assert r["index"] >= first


def test_margin_fails_on_products_cut_to_16_bits():
    """(d) within the hard bound -- it is loose at n = 1024 -- and normwise
    invisible, but more than 4 times the oracle's own error."""
    c = DB.case("cccf", 1024)
    z = DB.truncated_sum(c, 16)
    assert DB.normwise(z, c.ref) < DB.NRM
    r = c.check_bound(z)
    assert r["failing"] == 0 and r["worst"] > DB.MARGIN * c.oracle_worst
    with pytest.raises(AssertionError, match="more than 4 x the oracle"):
        c.check(z)
    c.check(c.ref)                            # the oracle itself passes both
    c.check(DB.truncated_sum(c, 23))          # and so does the same sum with nothing cut
    assert np.array_equal(DB.truncated_sum(c, 23), c.ref)


def test_checker_fails_on_nan():
    c = DB.case("rrrf", 6)
    z = c.ref.copy()
    z[1234] = np.nan
    assert c.report(z)["nonfinite"] == 1
    _fails(c, z, 1)
