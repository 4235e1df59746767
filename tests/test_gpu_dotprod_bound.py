"""Every route and grid pass of lqk_dotprod_batch, the host-pointer staging
seams and the one-vector calls of dotprod_{rrrf,crcf,cccf} against the direct
form's per-row error bound and the oracle's own error (tests/dotprod_bound.py)
(`-m gpu`).

Each row first asserts the launch its shape takes
(liquid_mi355x_dotprod_route, the launch's own decision: k_dot_vec or
k_dot_scalar, the lanes per row G, the passes of the grid over the rows), then
that every row of the batch is within (T + 8) 2^-23 A[v] of the float64 result
-- exactly 0 where A[v] = 0 -- then that the worst row is within 4 times the
oracle's worst on the same batch.  The batches mix full-scale, quiet (2^-17),
zero and cancelling rows so that every wave holds a loud, a quiet and a zero
row.  Device results land in buffers filled with NaN, with guard elements
either side: a row the kernel does not write, or a write outside the rows,
fails.  No row is left out of a check.
"""
import numpy as np
import pytest

import dotprod_bound as DB
import liquidmi as LQ

pytestmark = pytest.mark.gpu

GUARD = 4   # result elements either side of the rows that must stay as they were


def _route(t, n, aligned, nvec, expect):
    r = LQ.dotprod_route(t, n, aligned, nvec)
    print("dotprod route %s n=%d nvec=%d aligned=%d: %s G=%d passes=%d" % ((t, n, nvec, aligned) + r))
    assert r == expect, (t, n, nvec, r, expect)


def _dev(q, X, off=0, yoff=0):
    """The rows of X through execute_batch_dev: X `off` bytes past a 16-byte
    boundary, the result `yoff` elements past one."""
    nvec = X.shape[0]
    bx = LQ.DeviceBuffer(X.nbytes + 32)
    assert bx.p % 16 == 0
    if X.nbytes:
        LQ.lib().liquid_mi355x_memcpy_h2d(bx.p + off, LQ.ptr(X), X.nbytes)
    fill = np.full(GUARD + yoff + nvec + GUARD, np.nan, X.dtype)
    by = LQ.DeviceBuffer.from_array(fill)
    a = GUARD + yoff
    assert by.p % 16 == 0 and ((by.p + a * X.itemsize) % 16 == 0) == (yoff * X.itemsize % 16 == 0)
    q.execute_batch_dev(bx.p + off, nvec, by.p + a * X.itemsize)
    LQ.lib().liquid_mi355x_device_synchronize()
    out = by.to_array(X.dtype, len(fill))
    bx.free()
    by.free()
    assert np.all(np.isnan(out[:a])) and np.all(np.isnan(out[a + nvec:])), "a write outside the rows"
    return out[a:a + nvec]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ group ladder
@pytest.mark.parametrize("row", DB.LADDER_VEC + DB.LADDER_SCALAR, ids=DB.row_id)
def test_group_ladder(row):
    """G = 1, 2, 4, 8, 16 on both kernels, 4099 rows: the last block part
    full.  The same rows through host pointers take the same launch and give
    the same bits."""
    t, n, kernel, G = row
    c = DB.case(t, n)
    _route(t, n, True, c.nvec, (kernel, G, 1))
    q = LQ.DotProd(t, c.h)
    y = _dev(q, c.X)
    c.check(y, "%s G=%d" % (kernel, G))
    assert _same_bits(q.execute_batch(c.X, fill=np.nan), y)


@pytest.mark.parametrize("t", DB.KINDS)
def test_no_samples_give_exact_zeros(t):
    """n = 0 on the device call and on the host call; the object comes from n
    = 16 by recreate, its result buffer full of the call before."""
    c16, c0 = DB.case(t, 16, 40), DB.case(t, 0, 40)
    q = LQ.DotProd(t, c16.h)
    c16.check(q.execute_batch(c16.X, fill=np.nan), "before n = 0")
    q.recreate(c0.h)
    _route(t, 0, True, 40, ("vec", 1, 1))
    y = q.execute_batch(c0.X, nvec=40, fill=np.nan)
    assert np.all(y == 0)
    c0.check(y, "host")
    y = _dev(q, c0.X)
    assert np.all(y == 0)
    c0.check(y, "device")


# ------------------------------------------------------------------ alignment
@pytest.mark.parametrize("row", DB.UNALIGNED, ids=DB.row_id)
def test_unaligned_input_takes_the_scalar_kernel(row):
    """A vector-eligible length on an input pointer one, two or three samples
    (rrrf) or one sample (complex) past a 16-byte boundary, the result one
    element past one."""
    t, n, off, G = row
    c = DB.case(t, n)
    assert LQ.dotprod_route(t, n, True, c.nvec)[0] == "vec"
    _route(t, n, False, c.nvec, ("scalar", G, 1))
    assert off % c.X.itemsize == 0 and off % 16
    c.check(_dev(LQ.DotProd(t, c.h), c.X, off=off, yoff=1), "%d bytes off" % off)


def test_unaligned_result_on_the_vector_kernel():
    """The vector kernel keeps its route on a result pointer one element off."""
    for t, n, G in (("rrrf", 16, 4), ("crcf", 16, 8), ("cccf", 130, 16)):
        c = DB.case(t, n)
        _route(t, n, True, c.nvec, ("vec", G, 1))
        c.check(_dev(LQ.DotProd(t, c.h), c.X, yoff=1), "result one element off")


# ------------------------------------------------------------------ capped grid
@pytest.mark.parametrize("passes", [2, 3])
@pytest.mark.parametrize("row", DB.CAPPED, ids=DB.row_id)
def test_capped_grid_ragged_last_pass(row, passes):
    """One and two whole passes of the capped grid and 37 rows more: in the
    last pass the first 37 groups work on while the rest of their waves, and
    every other wave, are done."""
    t, n, kernel, G = row
    cap = LQ.dotprod_block_cap()
    nvec = DB.capped_nvec(cap, G, passes)
    _route(t, n, True, nvec, (kernel, G, passes))
    assert LQ.dotprod_route(t, n, True, nvec - DB.RAGGED)[2] == passes - 1
    c = DB.Case(t, n, nvec)
    assert {"quiet", "zero", "cancel"} <= set(c.cls[-DB.RAGGED:])
    c.check(_dev(LQ.DotProd(t, c.h), c.X), "%s G=%d %d passes" % (kernel, G, passes))


# ------------------------------------------------------------------ one long row
@pytest.mark.parametrize("row", DB.LONG, ids=DB.row_id)
def test_one_long_row(row):
    """Three rows (full, quiet, zero) of 2^20 and a few samples: 16 lanes walk
    65536 chunks each.  The hard bound is loose here -- (T + 8) 2^-23 A is
    some 10^7 times the error of a float32 tree sum -- so the margin against
    the oracle's serial sum is the assertion that binds."""
    t, n, kernel, G = row
    c = DB.Case(t, n, 3, DB.LONG_PATTERN)
    _route(t, n, True, 3, (kernel, G, 1))
    q = LQ.DotProd(t, c.h)
    y = _dev(q, c.X)
    c.check(y, "%s one long row" % kernel)
    assert _same_bits(q.execute_batch(c.X, fill=np.nan), y)


# ------------------------------------------------------------------ staging seams
def test_host_pointer_staging_seams():
    """cccf n = 16 through host pointers with the input at
    liquid_mi355x_pinned_input_max bytes and one row past it (pinned, read in
    place / DMA), and the result at liquid_mi355x_copyout_max bytes and one
    row past it (copy-out kernel / DMA and sync), as consecutive calls on one
    object, large, small, large: the paths alternate and the device buffers
    regrow.  Every call starts at another row of the batch, and its result is
    the bits of those rows through execute_batch_dev."""
    t, n = "cccf", 16
    rin, rout = LQ.pinned_input_max() // (n * 8), LQ.copyout_max() // 8
    assert rin * n * 8 == LQ.pinned_input_max() and rout * 8 == LQ.copyout_max() and rout > rin + 1
    calls = [rout + 1, rin, rout + 1, rin + 1, rout, rin, rout + 1]
    step = 9
    c = DB.case(t, n, rout + 1 + step * len(calls), tag="seams")
    _route(t, n, True, c.nvec, ("vec", 8, 1))
    ydev = _dev(LQ.DotProd(t, c.h), c.X)
    c.check(ydev, "device")
    q = LQ.DotProd(t, c.h)
    for k, cnt in enumerate(calls):
        a = k * step
        y = q.execute_batch(c.X[a:a + cnt], fill=np.nan)
        assert _same_bits(y, ydev[a:a + cnt]), (k, cnt)


# ------------------------------------------------------------------ one-vector calls
@pytest.fixture(params=[False, True], ids=["gpu-singles", "host-singles"])
def small_calls(request):
    old = LQ.get_small_calls()
    LQ.set_small_calls(request.param)
    try:
        yield request.param
    finally:
        LQ.set_small_calls(old)


@pytest.mark.parametrize("n", DB.SINGLE_LENGTHS)
@pytest.mark.parametrize("t", DB.KINDS)
def test_one_vector_calls(t, n, small_calls):
    """_execute (k_dot_single's 256 lanes with under one, one and more than
    one element each, or the host's sum) on every row of a 21-row batch, one
    call per row: bound and margin, and the same bits from a second call;
    _run and _run4 on the same rows: the bound, and the same bits as each
    other."""
    c = DB.case(t, n, DB.SINGLE_ROWS, tag="single")
    assert LQ.get_small_calls() == small_calls
    q = LQ.DotProd(t, c.h)
    y = np.array([q.execute(x) for x in c.X], c.X.dtype)
    c.check(y, "_execute, small calls on the %s" % ("host" if small_calls else "GPU"))
    assert _same_bits(np.array([q.execute(x) for x in c.X], c.X.dtype), y)
    r1 = np.array([LQ.dotprod_run(t, c.h, x) for x in c.X], c.X.dtype)
    r4 = np.array([LQ.dotprod_run4(t, c.h, x) for x in c.X], c.X.dtype)
    c.check_bound(r1)
    assert _same_bits(r1, r4)


# ------------------------------------------------------------------ recreate
@pytest.mark.parametrize("t", DB.KINDS)
def test_recreate_to_other_lengths(t):
    """One object from n = 1024 to 7 to 130, fresh taps each time (d_h is
    reallocated), a checked device and host batch after each step; then a
    _run of another kind and length -- the shared scratch object behind the
    free functions -- between two calls of the object."""
    q = None
    for n, route in ((1024, ("vec", 16, 1)), (7, ("scalar", 4, 1)),
                     (130, ("scalar", 16, 1) if t == "rrrf" else ("vec", 16, 1))):
        c = DB.case(t, n)
        if q is None:
            q = LQ.DotProd(t, c.h)
        else:
            q.recreate(c.h)
        _route(t, n, True, c.nvec, route)
        y = _dev(q, c.X)
        c.check(y, "after recreate to %d" % n)
        assert _same_bits(q.execute_batch(c.X, fill=np.nan), y)
    other = DB.KINDS[(DB.KINDS.index(t) + 1) % 3]
    o = DB.case(other, 257, DB.SINGLE_ROWS, tag="single")
    r = np.array([LQ.dotprod_run(other, o.h, x) for x in o.X], o.X.dtype)
    o.check_bound(r)
    assert _same_bits(q.execute_batch(c.X, fill=np.nan), y)
    assert _same_bits(np.array([LQ.dotprod_run(other, o.h, x) for x in o.X], o.X.dtype), r)
