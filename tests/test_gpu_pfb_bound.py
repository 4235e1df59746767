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
shared.
"""
import numpy as np
import pytest

import liquidmi as LQ
import pfb_bound as PB

pytestmark = pytest.mark.gpu

MARGIN = 4.0
# rows held to (1) only: {row id: why the kernel's arithmetic is sound} (DESIGN.md has the measured ratios)
BOUND_ONLY = {}


def _ways(r):
    return ("device", "device-ragged") if r.mode == "unaligned" else ("one-call", "ragged", "device")


CASES = [(r, name, way) for r in PB.ROWS for name in PB.ENVELOPES for way in _ways(r)]


def _make(c):
    r = c.r
    typ = LQ.LIQUID_ANALYZER if r.an else LQ.LIQUID_SYNTHESIZER
    if r.kind == "pfb2":
        return LQ.FirPfbch2(typ, r.M, r.q, h=c.h)
    return LQ.FirPfbch(typ, r.M, p=r.q, h=c.h, t=r.t)


def _run_host(c, at):
    g = _make(c)
    return np.concatenate([g.execute_block(p) for p in np.split(c.x, [b * PB.nin(c.r) for b in at])])


def _run_dev(c, at, shift=0):
    """One execute_block_dev per piece; the input `shift' bytes into its buffer."""
    g = _make(c)
    ni, no = PB.nin(c.r) * 8, PB.nout(c.r) * 8
    bx = LQ.DeviceBuffer(c.x.nbytes + 16)
    by = LQ.DeviceBuffer(c.nb * no)
    LQ.lib().liquid_mi355x_memcpy_h2d(bx.p + shift, LQ.ptr(c.x), c.x.nbytes)
    edges = [0] + list(at) + [c.nb]
    for a, b in zip(edges[:-1], edges[1:]):
        g.execute_block_dev(bx.p + shift + a * ni, b - a, by.p + a * no)
    g.synchronize()
    return by.to_array(np.complex64, c.nb * PB.nout(c.r))


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
    c = PB.case(r, name)
    few = PB.few_cuts(r) if r.mode == "few" else []
    shift = 8 if r.mode == "unaligned" else 0
    if way == "one-call":
        y = _run_host(c, few)
    elif way == "ragged":
        y = _run_host(c, PB.cuts(r))
    elif way == "device":
        y = _run_dev(c, few, shift)
    else:
        y = _run_dev(c, PB.cuts(r), shift)
    _hold(c, y, way)


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
