"""Every channelizer kernel against an error bound local to each output frame
(tests/pfb_bound.py), however the caller cuts the stream (`-m gpu`).

The parity tests compare a whole run with one number, max|err| / max|y|, on
input at one level, so a quiet frame is checked only against the loudest
frame's level: a stale LDS buffer or ring row, a warm-up row too few, the
taps of the other block parity or a history one block off would all pass as
long as they hit quiet frames.  Here the streams are quiet (1e-5 of full
scale, or exactly zero) with full-level stretches on the seams of each
kernel's workgroup runs, and every output is held to

  (1) the bound derived from the inputs its own frame sees (exactly zero
      where those are all zero), and every output finite;
  (2) r_gpu <= 4 r_oracle, r the worst ratio err / bound over the case and
      r_oracle the oracle's on the same case, computed here: both are float32
      evaluations of the same sums in another order, which moves the error's
      spread by well under 2, and the maximum over 10^4 - 10^5 outputs of
      either fluctuates by less than another factor of 2.

One row per kernel the dispatch reaches (pfb_bound.ROWS names them), both
envelopes, each
  (a) in one call (host pointers),
  (b) in ragged calls that start on both block parities, one of them quiet
      and right after a loud stretch, which it sees only through the carried
      history or state,
  (c) through execute_block_dev on device pointers;
rows of mode `few' run (a) and (c) in calls of 16 blocks, and the row at a
pointer that is 8 but not 16 bytes aligned runs on device pointers only.
The float64 model and the oracle's output of a case are computed once and
shared.  Every call asserts, immediately before it is made, the route the
launch will take (liquidmi.firpfbch2_route / firpfbch_route, the launch's own
decision) with the call's real alignment and block parity.

test_long_runs runs every run-walking kernel family at runs of at least three
times the minimum, and the short extra run of k_pfb2_an256 / k_pfb2_an2048,
under a limit of 3 workgroups; test_chunk_seams runs the chunking analyzers
across four chunks of 64 blocks.  Both hold the outputs to (1) and (2) and to
bit equality with the unlimited, unchunked launch.
"""
import numpy as np
import pytest

import liquidmi as LQ
import pfb_bound as PB

pytestmark = pytest.mark.gpu

MARGIN = 4.0
# rows held to (1) only: {row id: why the kernel's arithmetic is sound} (DESIGN.md has the measured ratios)
BOUND_ONLY = {}


CASES = [(r, name, way) for r in PB.ROWS for name in PB.ENVELOPES for way, _, _ in PB.ways(r)]


def _make(c):
    r = c.r
    typ = LQ.LIQUID_ANALYZER if r.an else LQ.LIQUID_SYNTHESIZER
    if r.kind == "pfb2":
        return LQ.FirPfbch2(typ, r.M, r.q, h=c.h)
    return LQ.FirPfbch(typ, r.M, p=r.q, h=c.h, t=r.t)


def _query(r, n, parity, x16, y16, host):
    typ = LQ.LIQUID_ANALYZER if r.an else LQ.LIQUID_SYNTHESIZER
    if r.kind == "pfb2":
        return LQ.firpfbch2_route(typ, r.M, r.q, n, parity, x16, y16, host)
    return LQ.firpfbch_route(r.t, typ, r.M, r.q, n, x16, y16, host)


def _expect(r, a, n, x16, y16, host, chunk=0):
    """The launch's decision for the call about to be made (n blocks from
    block a of the stream): the route the row names for a call of that
    length, cut into the chunks the knob asks for."""
    got = _query(r, n, a & 1, x16, y16, host)
    assert got.route == PB.piece_route(r, n, host), (PB.row_id(r), a, n, got)
    assert got.chunks == (-(-n // chunk) if chunk and got.route in CHUNKING else 1), (PB.row_id(r), a, n, got)
    return got


CHUNKING = ("pfb2_an1024", "pfb2_an1024_unpaired", "pfb2_an256", "pfb2_an512", "pfb2_an2048", "pfb2_an4096",
            "pfb2_an_small", "pfb2_poly+fft", "pfb_an1024", "pfb_an1024_unpaired")


def _run_host(c, at, chunk=0):
    """One execute_block per piece (the staging buffers are 16-byte aligned)."""
    g = _make(c)
    out = []
    for a, n in PB.pieces(c.r, at):
        _expect(c.r, a, n, True, True, True, chunk)
        out.append(g.execute_block(c.x[a * PB.nin(c.r):(a + n) * PB.nin(c.r)]))
    return np.concatenate(out)


def _run_dev(c, at, shift=0, chunk=0):
    """One execute_block_dev per piece; the input `shift' bytes into its buffer."""
    g = _make(c)
    ni, no = PB.nin(c.r) * 8, PB.nout(c.r) * 8
    bx = LQ.DeviceBuffer(c.x.nbytes + 16)
    by = LQ.DeviceBuffer(c.nb * no)
    LQ.lib().liquid_mi355x_memcpy_h2d(bx.p + shift, LQ.ptr(c.x), c.x.nbytes)
    for a, n in PB.pieces(c.r, at):
        px, py = bx.p + shift + a * ni, by.p + a * no
        _expect(c.r, a, n, px % 16 == 0, py % 16 == 0, False, chunk)
        g.execute_block_dev(px, n, py)
    g.synchronize()
    return by.to_array(np.complex64, c.nb * PB.nout(c.r))


def _run(c, way, chunk=0):
    at, host = {w: (at, host) for w, at, host in PB.ways(c.r)}[way]
    if host:
        return _run_host(c, at, chunk)
    return _run_dev(c, at, 8 if c.r.mode == "unaligned" else 0, chunk)


def _hold(c, y, what):
    rep = c.check(y, what)                                     # (1)
    ro = c.oracle()[1]["worst"]
    print("pfb_bound ratios | %s | %s | %s | r_oracle %.4g | r_gpu %.4g" % (PB.row_id(c.r), c.name, what, ro,
                                                                            rep["worst"]))
    if PB.row_id(c.r) not in BOUND_ONLY:
        assert rep["worst"] <= MARGIN * ro, (                  # (2)
            "%s %s %s: worst error %.4g of the bound at output %d, the oracle's %.4g" % (
                PB.row_id(c.r), c.name, what, rep["worst"], rep["index"], ro))


@pytest.mark.parametrize("r,name,way", CASES, ids=lambda v: PB.row_id(v) if isinstance(v, PB.Row) else v)
def test_channelizer_frame_bound(r, name, way):
    assert LQ.get_max_workgroups() == 0 and LQ.get_channelizer_chunk() == 0
    c = PB.case(r, name)
    _hold(c, _run(c, way), way)


# ------------------------------------------------------------------ long runs
# Every run-walking kernel at a run of at least three times its minimum: a
# limit of 3 workgroups (liquid_mi355x_set_max_workgroups) lengthens the runs
# of a stream short enough for a test.  S comes from the query, so the bursts
# sit on the seams of the long runs.
LIMIT = 3
LONG_BASE = [PB.PFB2_AN[10], PB.PFB2_AN[11],                  # an1024, m = 2 and 4
             PB.PFB2_AN[8], PB.PFB2_AN[9], PB.PFB2_AN[18], PB.PFB2_AN[19],   # an256, an512, an2048, an4096
             PB.PFB2_AN[6], PB.PFB2_AN[7],                    # an_small, M = 64 (4 sets to a workgroup) and 128 (2)
             PB.PFB2_AN[15],                                  # poly, M = 1024, m = 3
             PB.PFB2_SYN[5], PB.PFB2_SYN[2], PB.PFB2_SYN[3], PB.PFB2_SYN[6],   # syn1024, syn_fused (256, 512), syn4096
             PB.PFB_AN[3], PB.PFB_AN[4], PB.PFB_AN[2], PB.PFB_AN[1], PB.PFB_AN[5],   # an1024 (p = 4, 8), an_fused, an_small, an4096
             PB.PFB_SYN[3], PB.PFB_SYN[2], PB.PFB_SYN[1], PB.PFB_SYN[5],   # syn1024, syn_fused, syn_small, syn4096
             PB.PFB_CCCF[1], PB.PFB_CCCF[5]]                  # complex taps: an_fused, syn4096


def _sets(r):
    """Column sets to a workgroup (the small kernels), else 1."""
    return 256 // r.M if r.route.endswith(("_small", "_small_c")) else 1


def _limit(r):
    """The limit that leaves LIMIT runs: k_pfb2_poly covers M > 256 in column
    slices of 256, each run of rows a workgroup per slice, and its target
    counts them all."""
    return LIMIT * max(1, r.M // 256) if r.route == "pfb2_poly+fft" else LIMIT


def _long_rows():
    """(row, workgroups) under the limit: the shortest stream of exactly
    LIMIT runs (or column sets) each at least three times the minimum run,
    and for an256 / an2048 also the shortest that takes the short extra run
    (LIMIT runs of the minimum and a few rows)."""
    out = []
    try:
        for r in LONG_BASE:
            LQ.set_max_workgroups(_limit(r))
            want = -(-_limit(r) // _sets(r))
            for nb in range(3 * LIMIT * r.S - 8, 3 * LIMIT * r.S + 200):
                got = _query(r, nb, 0, True, True, False)
                if got.workgroups == want and got.run >= 3 * r.S and -(-nb // got.run) == LIMIT:
                    break
            else:
                raise AssertionError("no stream of %d long runs for %s" % (LIMIT, PB.row_id(r)))
            assert got.route == r.route
            out.append((r._replace(S=got.run, nb=nb), want))
            if r.route in ("pfb2_an256", "pfb2_an2048"):
                nb = 2 * (LIMIT * 32 + 5) - 3                 # 3 x 32 + 5 rows
                got = _query(r, nb, 0, True, True, False)
                assert got.run == r.S and got.workgroups == LIMIT + 1, got
                out.append((r._replace(nb=nb), LIMIT + 1))
    finally:
        LQ.set_max_workgroups(0)
    return out


LONG = _long_rows()
# rows whose output under the limit need not equal the unlimited one bit for
# bit: {row id: where the arithmetic depends on the run's start}
RUN_DEPENDENT = {}


@pytest.mark.parametrize("name", PB.ENVELOPES)
@pytest.mark.parametrize("r,wg", LONG, ids=lambda v: PB.row_id(v) if isinstance(v, PB.Row) else "wg%d" % v)
def test_long_runs(r, wg, name):
    c = PB.case(r, name)
    assert LQ.get_max_workgroups() == 0
    free = _query(r, c.nb, 0, True, True, False)
    y0 = _run_dev(c, [])
    try:
        LQ.set_max_workgroups(_limit(r))
        got = _query(r, c.nb, 0, True, True, False)
        assert (got.route, got.run, got.workgroups) == (r.route, r.S, wg), got
        assert got.run >= free.run and (got.run >= 3 * free.run or wg == LIMIT + 1)
        assert -(-c.nb // got.run) == (LIMIT if got.run > free.run else LIMIT + 1)
        y = _run_dev(c, [])
        yh = _run_host(c, [])
    finally:
        LQ.set_max_workgroups(0)
    _hold(c, y, "limit %d, run %d, device" % (_limit(r), got.run))
    _hold(c, yh, "limit %d, run %d, one-call" % (_limit(r), got.run))
    _hold(c, y0, "no limit, run %d" % free.run)
    assert np.array_equal(y.view(np.uint32), yh.view(np.uint32))
    if PB.row_id(r) not in RUN_DEPENDENT:
        d = np.flatnonzero(y.view(np.uint64) != y0.view(np.uint64))
        assert len(d) == 0, "%s %s: %d outputs differ from the unlimited launch's, the first at %d (block %d)" % (
            PB.row_id(r), name, len(d), d[0], d[0] // PB.nout(r))


# ------------------------------------------------------------------ chunk seams
# The three launches that cut a long call into chunks, at the smallest chunk
# the knob allows (64 blocks), so the rows' streams span four chunks.  S = 64
# puts the loud stretches on the seams: one ends with the last block before
# the first seam, one begins a block after it, one straddles the second.
CHUNK = 64
CHUNK_ROWS = [PB.PFB2_AN[11],                                 # k_pfb2_an1024 at m = 4 (lqk_firpfbch2_analyzer_fast)
              PB.PFB2_AN[8],                                  # M = 256 fused (lqk_firpfbch2_analyzer)
              PB.PFB2_AN[16]._replace(S=CHUNK),               # M = 256, m = 8: polyphase pass + transform per chunk
              PB.PFB_AN[3]._replace(S=CHUNK)]                 # k_pfb_an1024 at p = 4 (lqk_firpfbch_analyzer_fast)


@pytest.mark.parametrize("name", PB.ENVELOPES)
@pytest.mark.parametrize("r", CHUNK_ROWS, ids=PB.row_id)
def test_chunk_seams(r, name):
    c = PB.case(r, name)
    assert r.S == CHUNK and c.nb > 3 * CHUNK and LQ.get_channelizer_chunk() == 0
    s = PB.stretches(r.S, PB.window_blocks(r), c.nb, True)
    assert s["before"][1] == CHUNK and s["after"][0] == CHUNK + 1 and s["straddle"][0] < 2 * CHUNK < s["straddle"][1]
    # ragged: a call from block 1 (odd; its seams at 65, where a loud stretch
    # begins, and 129, inside the straddling one) and one from block 140 (even)
    at = [1, 140]
    assert [(a & 1, n > CHUNK) for a, n in PB.pieces(r, at)[1:]] == [(1, True), (0, True)]
    runs = {"one-call": lambda k: _run_host(c, [], k), "ragged": lambda k: _run_host(c, at, k),
            "device": lambda k: _run_dev(c, [], 0, k), "device-ragged": lambda k: _run_dev(c, at, 0, k)}
    y0 = {w: f(0) for w, f in runs.items()}
    try:
        LQ.set_channelizer_chunk(CHUNK)
        assert _query(r, c.nb, 0, True, True, False).chunks == -(-c.nb // CHUNK) >= 3
        y = {w: f(CHUNK) for w, f in runs.items()}
    finally:
        LQ.set_channelizer_chunk(0)
    for w in runs:
        _hold(c, y[w], "chunks of %d, %s" % (CHUNK, w))
        d = np.flatnonzero(y[w].view(np.uint64) != y0[w].view(np.uint64))
        assert len(d) == 0, "%s %s %s: %d outputs differ from the unchunked call's, the first in block %d" % (
            PB.row_id(r), name, w, len(d), d[0] // PB.nout(r))


# one row per object: firpfbch2 analyzer and synthesizer, firpfbch crcf and cccf both ways
RESET_ROWS = [PB.PFB2_AN[11], PB.PFB2_SYN[5], PB.PFB_AN[3], PB.PFB_SYN[3], PB.PFB_CCCF[1], PB.PFB_CCCF[4]]


@pytest.mark.parametrize("r", RESET_ROWS, ids=PB.row_id)
def test_reset_leaves_silence(r):
    """A loud stretch, reset(), then input that is exactly zero: the output
    is exactly zero.  Then an odd number of blocks, reset(), and the whole
    stream, which must come out as from a new object (the block parity is
    part of the state)."""
    c = PB.case(r, "gaps")
    ni, no = PB.nin(r), PB.nout(r)
    wl = PB.window_blocks(r)
    lo, hi = PB.stretches(r.S, wl, c.nb, r.an)["window"]
    assert np.min(np.abs(c.x[lo * ni:hi * ni])) > 0
    g = _make(c)
    g.execute_block(c.x[:hi * ni])
    g.reset()
    nz = r.S + 2 * wl + 1
    y = g.execute_block(np.zeros(nz * ni, np.complex64))
    PB.check("%s after reset" % PB.row_id(r), y, np.zeros(nz * no, np.complex128), np.zeros(nz * no))
    g.execute_block(c.x[:3 * ni])
    g.reset()
    _hold(c, g.execute_block(c.x), "after reset")
