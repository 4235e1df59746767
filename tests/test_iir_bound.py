"""The recursive filters' per-output bound (tests/iir_bound.py) on the CPU: the
serial float32 model meets it on every filter and stream, the scale's float64
model is iirfilt_model.run64, the zero rule and the floor work, and the
checker is pinned by four value-only mutations of y64 -- each a way the
block-parallel kernels (csrc/k_iirfilt.hip) could combine states wrongly.
Where the suite's normwise criterion (iirfilt_model.criterion) has a stream
that reaches the mutated code, the mutation is shown to pass it there, which
documents the hole; each must fail the new check on the named row.

No GPU.
"""
import functools

import numpy as np
import pytest

from scipy.signal import lfilter

import iir_bound as IB
import iirfilt_model as IM

TILE, SCAN, NS = IB.TILE, IB.SCAN, IB.NS
MUTATIONS = []     # (mutation, row, old criterion, new check) as the tests fill it


def record(mutation, row, old, new):
    MUTATIONS.append((mutation, row, old, new))
    print("mutation %-44s %-28s old criterion: %-6s new check: %s" % (mutation, row, old, new))


# ------------------------------------------------------------------ the model meets the bound
@pytest.mark.parametrize("fname,kind,ms", IB.ROWS, ids=["%s_%s" % r[:2] for r in IB.ROWS])
def test_run32_meets_the_bound(fname, kind, ms):
    assert ms == max(1, 1 << (IB.nsec(fname) - 1).bit_length())
    for e in IB.envelopes(fname):
        x, y64, A, U = IB.case(fname, kind, e)
        ok, r, w = IB.verdict(IB.model32(fname, kind, e), x, y64, A, U)
        floor = float(np.mean(IB.TINY * U > IB.EPS * A))
        print("iir_bound %-9s %s MS=%d %-6s run32 r %.3f at %5d, floor the larger term on %2.0f %%"
              % (fname, kind, ms, e, r, w, 100 * floor))
        assert ok and r <= 1.0       # within the bound with K = 1 too: room to spare
    print("iir_bound %-9s %s r_ref %.3f" % (fname, kind, IB.r_ref(fname, kind)))
    assert 0.0 < IB.r_ref(fname, kind) <= 1.0


@pytest.mark.parametrize("fname,kind,ms", IB.ROWS, ids=["%s_%s" % r[:2] for r in IB.ROWS])
def test_scale_model_is_run64(fname, kind, ms):
    e = IB.envelopes(fname)[1]
    x, y64, _, _ = IB.case(fname, kind, e)
    form, b, a = IB.coefs(fname, kind)
    ref = IM.run64(kind, form, b, a, x)
    assert np.max(np.abs(y64 - ref)) <= 1e-9 * np.max(np.abs(ref))


def test_streams():
    lv = IB.level(NS, "gaps")
    assert np.all(lv[TILE - 50:TILE + 1] == 1) and lv[TILE + 1] == 0 and lv[TILE - 51] == 0
    assert np.all(lv[2 * TILE - 1:2 * TILE + 60] == 1) and np.all(lv[NS - 5:] == 1) and lv[NS - 6] == 0
    assert lv[IB.CUT - 1] == 1 and lv[IB.CUT] == 0
    for s in (TILE + 17 * IB.RUN, TILE + 64 * IB.RUN):
        assert lv[s - 2] == 0 and lv[s - 1] == 1 and lv[s] == 1 and lv[s + 1] == 0
    assert np.all(lv[1300:TILE - 50] == 0)
    # a longer stream begins with the short one, so r_ref's streams are the call patterns' streams
    assert np.array_equal(IB.stream("crcf", NS + 64, "burst", 5)[:NS], IB.stream("crcf", NS, "burst", 5))
    # the accumulator's streams: no float32 partial sum of them is exact for long
    for e in IB.envelopes("accum"):
        x = IB.case("accum", "rrrf", e)[0]
        s64 = np.cumsum(x.astype(np.float64))
        assert np.mean(s64[100:].astype(np.float32) != s64[100:]) > 0.9


def test_eligibility_and_ladder_weight():
    """every filter is device-eligible by the rule of host/iirfilt.c (the accumulator's pole sits on
    the circle: |a1| <= 1 + a2 holds with equality), and at every ladder level that a stream of the
    suite reaches (a scan of step 2^l lanes' worth, l = 0..6 within a tile, 8..14 across tiles, 16
    and 17 across the long stream's three chunks) one of the slow filters has 0.02 <= |G| <= 1"""
    for fname in IB.FILTERS:
        for b0, b1, b2, a1, a2 in IB.sections(fname):
            if np.iscomplexobj(np.array([a1])):
                assert np.max(np.abs(np.roots([1, a1, a2]))) <= 1 + 1e-12
            else:
                assert abs(a2) <= 1 and abs(a1) <= 1 + a2
    poles = [abs(IB.sections(f)[0][3]) for f in ("leak12", "leak20", "accum")] + [abs(s[3]) for s in IB.sections("slow8")]
    for lv in list(range(0, 7)) + list(range(8, 15)) + [16, 17]:
        g = [p ** (IB.RUN * 2.0 ** lv) for p in poles]
        assert any(0.02 <= v < 1.0 for v in g), lv      # and not the accumulator's 1 alone


# ------------------------------------------------------------------ zeros and the floor
def test_zero_rule_and_floor():
    fname, kind = "butter4", "rrrf"
    # all zeros in: all zeros out, and nothing else
    z = np.zeros(300, np.float32)
    y64, A, U = IB.scale(fname, z)
    assert np.all(A == 0) and np.all(U >= 1)
    assert IB.verdict(z, z, y64, A, U)[0] and IB.verdict(-z, z, y64, A, U)[0]
    bad = z.copy()
    bad[7] = 2.0 ** -149
    assert not IB.verdict(bad, z, y64, A, U)[0]
    # zeros ahead of the stream: exactly 0 until the first input, the floor's allowance after it
    x = np.concatenate([np.zeros(100, np.float32), IB.case(fname, kind, "gaps")[0][:900]])
    y64, A, U = IB.scale(fname, x)
    first = IB.first_input(x)
    assert first >= 100 and np.all(A[:first] == 0) and A[first] > 0
    good = y64.astype(np.float32)
    assert IB.verdict(good, x, y64, A, U)[0]
    bad = good.copy()
    bad[first - 1] = 2.0 ** -149
    assert not IB.verdict(bad, x, y64, A, U)[0]
    # a non-finite output fails whatever the bound
    bad = good.copy()
    bad[500] = np.inf
    assert not IB.verdict(bad, x, y64, A, U)[0]
    # the floor: deep in a gap the bound is a few times 2^-126; a flush to zero and a denormal pass
    x, y64, A, U = IB.case(fname, kind, "gaps")
    n = TILE - 100
    assert IB.EPS * A[n] < IB.TINY * U[n] < 2.0 ** -120
    y = y64.astype(np.float32)
    assert y[n] == 0 and IB.verdict(y, x, y64, A, U)[0]
    y[n] = 2.0 ** -140
    assert IB.verdict(y, x, y64, A, U)[0]
    assert mutation_d()


def test_truncated_convolution():
    """|g| cut where its tail is below 2^-24 of the floor: against the uncut convolution"""
    b0, b1, b2, a1, a2 = IB.sections("ellip8")[3]
    rng = np.random.default_rng(1)
    r = rng.uniform(0, 1, 20000) * (rng.uniform(0, 1, 20000) < 0.01)
    L = IB._absg_len(a1, a2, 1.0)
    assert 1000 < L < 20000
    imp = np.zeros(len(r))
    imp[0] = 1.0
    full = np.convolve(r, np.abs(lfilter([1.0], [1.0, a1, a2], imp)))[:len(r)]
    got = IB._absg_conv(a1, a2, r)
    # (the two sums round their float64 terms in different orders)
    assert np.all(np.abs(full - got) <= 2.0 ** -24 * IB.TINY + 1e-13 * full)
    assert np.all(got[r.cumsum() == 0] == 0)      # exact zeros stay exact
    # a long stream: |g| beyond J through its majorant, never below the exact scale and, at a steady
    # level, above it by next to nothing
    n = IB.LONG + 5000
    r = np.concatenate([np.zeros(100), rng.uniform(0.5, 1, n - 100)])
    J = IB._absg_head(a1, a2)
    assert J < IB._absg_len(a1, a2, 1.0) / 2
    imp = np.zeros(n)
    imp[0] = 1.0
    full = np.convolve(r, np.abs(lfilter([1.0], [1.0, a1, a2], imp)))[:n]
    got = IB._absg_conv(a1, a2, r)
    assert np.all(got >= full * (1 - 1e-13)) and np.all(got <= full * (1 + 1e-11)) and np.all(got[:100] == 0)


# ------------------------------------------------------------------ mutations of y64
def old_criterion(y, y64, spans=(slice(None),)):
    """iirfilt_model.criterion against a float32 result without any error (e_ref = 0): the
    strictest form the suite's criterion can take on a stream"""
    return all(IM.criterion("mutation", y, y64, y64, s)[2] for s in spans)


def drop_older(first):
    """span i >= first starts from the span before it alone"""
    return lambda i, true, z: true if i < first else z[i - 1]


@functools.lru_cache(maxsize=None)
def mutation_d():
    """1e-30 is written into one output of a gap"""
    x, y64, A, U = IB.case("butter4", "rrrf", "gaps")
    n = TILE - 100
    y = y64.astype(np.float32)
    y[n] = 1e-30
    ok, r, w = IB.verdict(y, x, y64, A, U)
    assert not ok and w == n
    record("(d) 1e-30 written into a gap", "butter4 rrrf gaps", "-", "FAIL at %d" % w)
    return True


@functools.lru_cache(maxsize=None)
def mutation_a():
    """every tile from the third on starts from z[t-1] alone"""
    start = drop_older(2)
    # the suite's stream that reaches the cross-chunk scans: the 0.99 DC blocker at SCAN TILE + 1
    n = SCAN * TILE + 1
    x = IM.noise_input("rrrf", n, 77)
    edges = list(range(0, n, TILE)) + [n]
    y64 = IB.run64_seg("dc01", x)[0]
    mut = IB.run64_spans("dc01", x, edges, start)
    old = old_criterion(mut, y64, (slice(None), slice(n - TILE, n)))
    assert old and np.max(np.abs(mut - y64)) < 1e-15
    record("(a) tile t >= 2 starts from z[t-1] alone", "dc01 rrrf SCAN TILE + 1", "passes", "-")
    for fname, kind in (("leak12", "rrrf"), ("slow8", "cccf")):
        x, y64, A, U = IB.case(fname, kind, "burst")
        edges = list(range(0, NS, TILE)) + [NS]
        assert np.array_equal(IB.run64_spans(fname, x, edges, lambda i, true, z: true), IB.run64_seg(fname, x)[0])
        mut = IB.run64_spans(fname, x, edges, start)
        assert np.array_equal(mut[:2 * TILE], IB.run64_seg(fname, x)[0][:2 * TILE])
        ok, r, w = IB.verdict(mut, x, y64, A, U)
        assert not ok and w >= 2 * TILE
        record("(a) tile t >= 2 starts from z[t-1] alone", "%s %s burst" % (fname, kind), "-", "FAIL r %.3g at %d" % (r, w))
    return True


@functools.lru_cache(maxsize=None)
def mutation_b():
    """chunk c >= 1 starts from chunk c-1's total alone"""
    ch = SCAN * TILE
    # two chunks from zero state (the suite's test_two_scan_levels): the mutation is the correct result
    n = ch + 1
    x = IM.noise_input("rrrf", n, 77)
    whole = IB.run64_seg("leak20", x)[0]
    mut = IB.run64_spans("leak20", x, [0, ch, n], drop_older(1))
    assert np.array_equal(mut, whole)
    record("(b) chunk c >= 1 starts from chunk c-1's total", "two chunks, zero state", "equal", "equal")
    # the long stream after its loud first call: three chunks, a state to carry
    x, y64, A, U = IB.long_case("leak20", "rrrf")
    edges = [0, IB.FIRST, IB.FIRST + ch, IB.FIRST + 2 * ch, len(x)]
    mut = IB.run64_spans("leak20", x, edges, drop_older(2))
    assert np.array_equal(mut[:IB.FIRST + ch], IB.run64_seg("leak20", x)[0][:IB.FIRST + ch])
    ok, r, w = IB.verdict(mut, x, y64, A, U, slice(IB.FIRST, None))
    assert not ok and w >= IB.FIRST + ch
    record("(b) chunk c >= 1 starts from chunk c-1's total", "leak20 rrrf long after 777", "-", "FAIL r %.3g at %d" % (r, w))
    return True


@functools.lru_cache(maxsize=None)
def mutation_c():
    """2^-24 of the loudest tile's end state is added to the start state of a later, quiet span"""
    def polluted(fname, x, y64, loud_end, at):
        """y64 with 2^-24 of the state before sample loud_end added to the state before sample at"""
        extra = [(2.0 ** -24 * v1, 2.0 ** -24 * v2) for v1, v2 in IB.df2_state(fname, x, loud_end)]
        mut = y64.copy()
        mut[at:] += IB.zero_input(fname, extra, len(x) - at)
        return mut
    # the suite's burst stream (test_burst): 1e-4 around a loud middle third, judged in thirds; the
    # loudest tile is tile 1 and tile 3 starts quiet
    for idx, (fname, kind) in enumerate((("dc01", "crcf"), ("butter4", "rrrf"))):
        lv = np.full(NS, 1e-4)
        lv[NS // 3:2 * NS // 3] = 1.0
        x = IM.noise_input(kind, NS, 9000 + idx, lv)
        form, b, a = IB.coefs(fname, kind)
        y32, _ = IM.run32(kind, form, b, a, x)
        y64 = IM.run64(kind, form, b, a, x)
        mut = polluted(fname, x, y64, 2 * TILE, 3 * TILE)
        assert np.max(np.abs(mut[3 * TILE:] - y64[3 * TILE:])) > 0
        spans = (slice(None), slice(0, NS // 3), slice(NS // 3, 2 * NS // 3), slice(2 * NS // 3, NS))
        assert all(IM.criterion("(c) %s" % fname, mut, y32, y64, s)[2] for s in spans)
        record("(c) 2^-24 of a loud state into a quiet start", "%s %s old burst stream" % (fname, kind), "passes", "-")
        # the new rows: tile 0 ends loud; wave 3 of tile 2 starts 1295 samples after the last run.
        # On the DC blocker's burst row the floor of 1e-5 keeps the bound at 100 (the sum of |g|)
        # times the local level there, and 2^-24 of this stream's state at TILE, |v| = 0.6, through
        # 1 - 0.99 stays inside 4 r_ref (printed): its gaps row is the one that shows it.
        at = 2 * TILE + 3 * 64 * IB.RUN
        for envelope in ("burst", "gaps"):
            x, y64, A, U = IB.case(fname, kind, envelope)
            mut = polluted(fname, x, y64, TILE, at)
            ok, r, w = IB.verdict(mut, x, y64, A, U)
            rr = IB.r_ref(fname, kind)
            fails = not ok or r > IB.MARGIN * rr
            print("(c) %s %s %s: within the bound %s, r %.3g against %g x r_ref %.3g"
                  % (fname, kind, envelope, ok, r, IB.MARGIN, rr))
            if (fname, envelope) != ("dc01", "burst"):
                assert fails and w >= at
            record("(c) 2^-24 of a loud state into a quiet start", "%s %s %s" % (fname, kind, envelope), "-",
                   "%s r %.3g at %d" % ("pass" if not fails else "FAIL (bound)" if not ok else "FAIL (4 r_ref)", r, w))
    return True


def test_mutation_a_tiles_drop_everything_older():
    assert mutation_a()


def test_mutation_b_chunks_drop_everything_older():
    assert mutation_b()


def test_mutation_c_a_quiet_span_starts_polluted():
    assert mutation_c()


def test_mutation_table():
    """the four mutations, each with the old criterion's outcome where the suite has a stream that
    reaches it and the new check's on the named row"""
    assert mutation_a() and mutation_b() and mutation_c() and mutation_d()
    for m in MUTATIONS:
        print("%-48s %-30s %-8s %s" % m)
    for tag in "abcd":
        assert any(m[0].startswith("(%s)" % tag) and m[3].startswith("FAIL") for m in MUTATIONS), tag
