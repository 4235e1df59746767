"""detector_cccf's block calls on the GPU against tests/detector_model.py:
every row within the per-output bound (and within 4 x the float32 serial
model's own worst ratio), exactly zero where the window's energy is zero;
detections at the float64 state machine's indices with estimates within their
propagated bounds, however the stream is cut into calls and tiles, whatever the
device list's capacity; bit-identical results across host pointers, device
pointers, streams, resets and alignments.

TILE, MAX_LEN and MAX_CORRELATORS come from the library; N = 3 TILE + 5 unless
stated.  Models are computed once per stream and shared.
"""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import detector_model as DM
import liquidmi as LQ

pytestmark = pytest.mark.gpu

TILE = LQ.Detector.TILE
MAX_LEN = LQ.Detector.MAX_LEN
MAX_M = LQ.Detector.MAX_CORRELATORS
N = 3 * TILE + 5
SEAMS = (TILE, 2 * TILE, 3 * TILE)
FIX = DM.load_fixture()
BY_NAME = {c["name"]: c for c in FIX["cases"]}
IDS = [c[0] for c in DM.CASES]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dphi_max_for(n, m):
    """a dphi_max that gives m correlators"""
    return 0.0 if m <= 2 else (m - 0.5) * float(DM.step_of(n))


def call_sizes(total, sizes):
    out, k = [], 0
    sizes = list(sizes)
    while k < total:
        c = min(sizes.pop(0) if sizes else total - k, total - k)
        out.append(c)
        k += c
    return out


def run_host(q, x, sizes=(), max_det=64):
    """the stream through correlate_block; -> [(index in the stream, tau, dphi, gamma)]"""
    out, k = [], 0
    for c in call_sizes(len(x), sizes):
        cnt, idx, tau, dphi, gam = q.correlate_block(x[k:k + c], max_det=max_det)
        assert len(idx) == min(cnt, max_det) and np.all(idx < c), "indices are relative to their own call"
        out += [(k + int(i), t, p, g) for i, t, p, g in zip(idx, tau, dphi, gam)]
        k += c
    return out


def run_dev(q, x, sizes=(), rows=True, max_det=64, off_x=0, off_r=0):
    """the stream through correlate_block_dev; off_x / off_r: samples / floats
    by which the device input / rows are moved off their allocation's start.
    -> detections, rows (N x m) or None"""
    m, n = q.num_correlators, len(x)
    dx = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(off_x, np.complex64), x]))
    dr = LQ.DeviceBuffer((n * m + off_r) * 4) if rows else None
    out, k = [], 0
    for c in call_sizes(n, sizes):
        cnt, idx, tau, dphi, gam = q.correlate_block_dev(dx.p + (off_x + k) * 8, c,
                                                         dr.p + (off_r + k * m) * 4 if rows else 0, max_det=max_det)
        assert len(idx) == min(cnt, max_det) and np.all(idx < c), "indices are relative to their own call"
        out += [(k + int(i), t, p, g) for i, t, p, g in zip(idx, tau, dphi, gam)]
        k += c
    r = dr.to_array(np.float32, n * m + off_r)[off_r:].reshape(n, m) if rows else None
    return out, r


def est_bits(dets):
    return [(d[0],) + tuple(np.float32(v).tobytes() for v in d[1:]) for d in dets]


class Model:
    """a stream with its float64 rows, bound and detections; the margin asserted"""

    def __init__(self, label, s, thr, dphi_max, x, margin=True):
        self.label, self.s, self.thr, self.dphi_max, self.x = label, s, thr, dphi_max, x
        self.bank = DM.Bank(s, dphi_max)
        self.r64, self.E64, self.bound = DM.rows64(self.bank, x)
        if margin:
            self.dets = DM.check_margin(label, self.bank, thr, self.r64, self.bound, self.E64)
        else:
            self.dets = None
        x.setflags(write=False)

    def detector(self):
        q = LQ.Detector(self.s, self.thr, self.dphi_max)
        assert q.num_correlators == self.bank.m
        return q

    def check(self, what, got):
        return DM.check_detections(self.label + " " + what, got, self.bank, self.r64, self.E64, self.bound, self.thr,
                                   self.dets)

    def check_rows(self, what, r, serial=None):
        return DM.check_rows(self.label + " " + what, r, self.r64, self.E64, self.bound, serial)


# ------------------------------------------------------------------ 1 fixtures
@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_fixture_case(case):
    """every recorded case through correlate_block: the reference's indices,
    estimates within the bound; the ten autotest lengths also by the autotest's
    own acceptance"""
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    name, n, thr, dphi_max, carrier = case[:5]
    q = LQ.Detector(s, thr, dphi_max)
    assert q.device_eligible and q.num_correlators == BY_NAME[name]["m"]
    got = run_host(q, x)
    assert [g[0] for g in got] == [d[0] for d in BY_NAME[name]["detections"]]
    DM.check_detections("fixture " + name, got, bank, r64, E64, bound, thr, dets64)
    if n in DM.AUTOTEST_N and name.startswith("n"):
        (i, tau, dphi, gamma), = got
        assert abs(dphi - carrier) < 0.01
        assert abs(i + tau - (case[6][0] + n)) < 0.2
        assert abs(20 * np.log10(gamma)) < 2.0   # the preamble's amplitude is 1


# ------------------------------------------------------------------ 2 rows
@functools.lru_cache(maxsize=None)
def rows_model(n, m, env):
    s = DM.sequence(n)
    x = DM.envelope_stream(env, N, 4100 + n + (env == "gaps"), SEAMS, n)
    return Model("rows n=%d m=%d %s" % (n, m, env), s, 0.5, dphi_max_for(n, m), x, margin=False)


@pytest.mark.parametrize("env", ["burst", "gaps"])
@pytest.mark.parametrize("m", [2, 3, 13, MAX_M])   # 13: a bank walked in two uneven halves (7 + 6)
@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 83, 335])
def test_rows(n, m, env):
    M = rows_model(n, m, env)
    assert M.bank.m == m
    q = M.detector()
    assert q.device_eligible
    _, r = run_dev(q, M.x, max_det=0)
    serial = DM.report(DM.serial32(M.bank, M.x)[0], M.r64, M.E64, M.bound)["worst"]
    M.check_rows("kernel", r, serial)
    if env == "gaps":
        zero = M.E64 == 0
        assert zero.sum() >= n and np.all(r[zero] == 0)


# ------------------------------------------------------------------ 3 seams
def seam_stream(delta, seed):
    """n = 64, three correlators, the carrier on the middle one; five preambles
    at the positions below"""
    n = 64
    s = DM.sequence(n)
    ends = [TILE + delta,                 # the peak next to a tile seam and to a call boundary of TILE, TILE, ..
            TILE + 9 + 3 * n + delta,     # well inside a tile (the call boundary of 1, 7, TILE + 1 is at TILE + 9)
            2 * TILE + delta]
    # a stale pair across the last seam: the second preamble ends on the first sample after the first one's timer
    p0 = 3 * TILE - n - n // 4 - 1 + delta
    pos = [e - n + 1 for e in ends] + [p0, p0 + n // 4 + 2]
    return s, DM.stream(s, N, pos, 5000 + 17 * seed + (delta + 8), dphi=0.0)


@functools.lru_cache(maxsize=None)
def seam_model(delta):
    """the first seed whose stream meets the decision margin"""
    for seed in range(1, 12):
        s, x = seam_stream(delta, seed)
        bank = DM.Bank(s, 0.08)
        r64, E64, bound = DM.rows64(bank, x)
        if DM.margins(bank, 0.5, r64, bound, E64)[0] >= 1:
            M = Model("seam %+d seed %d" % (delta, seed), s, 0.5, 0.08, x)
            assert M.bank.m == 3 and len(M.dets) >= 5
            return M
    raise AssertionError("no seed meets the margin")


PATTERNS = {"1,7,TILE+1,rest": (1, 7, TILE + 1), "TILE": (TILE,) * 4, "one": ()}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("delta", [-3, -2, -1, 0, 1, 2])
def test_seams(delta, pattern):
    """the trigger, the peak and the terminating sample on either side of a
    tile seam and of a call boundary; a timer that spans a call boundary
    (delta <= -1: the detection before TILE starts one that ends after it);
    the stale row across a timer gap next to the last seam"""
    M = seam_model(delta)
    got, _ = run_dev(M.detector(), M.x, PATTERNS[pattern], rows=False)
    M.check(pattern, got)
    assert any(d["idetect"] == 1 for d in M.dets), "the middle of the bank"
    stale = [d for d in M.dets if d["src"][0] is not None and d["src"][1] - d["src"][0] > 1]
    assert stale, "a detection that reads its oldest row across a timer gap"


def test_seam_at_call_boundary_of_the_first_pattern():
    """peaks next to sample TILE + 9, where the third call of 1, 7, TILE + 1 ends"""
    n = 64
    s = DM.sequence(n)
    for delta in (-1, 0, 1):
        for seed in range(1, 12):
            x = DM.stream(s, N, [TILE + 9 + delta - n + 1], 5300 + seed, dphi=0.0)
            bank = DM.Bank(s, 0.08)
            r64, E64, bound = DM.rows64(bank, x)
            if DM.margins(bank, 0.5, r64, bound, E64)[0] >= 1:
                break
        M = Model("call seam %+d" % delta, s, 0.5, 0.08, x)
        got, _ = run_dev(M.detector(), M.x, PATTERNS["1,7,TILE+1,rest"], rows=False)
        M.check("1,7,TILE+1,rest", got)
        assert [g[0] for g in got] == [TILE + 9 + delta + 1]


# ------------------------------------------------------------------ 4 the marked list
@functools.lru_cache(maxsize=None)
def repeated_model():
    """the sequence back to back: a detection every period, more than a third
    of the samples marked"""
    n = 12
    s = DM.sequence(n)
    x = DM.noise(N, 901, 0.05).astype(np.complex128)
    x += np.tile(s.astype(np.complex128), N // n + 1)[:N] * np.exp(0.01j * np.arange(N))
    x = x.astype(np.complex64)
    DM.assert_not_quiet(x)
    M = Model("repeated", s, 0.45, 0.0, x)
    assert len(M.dets) >= N // n - 2
    assert DM.marked(M.r64, M.thr).sum() > TILE
    return M


def test_marked_list_and_its_capacity():
    M = repeated_model()
    big = len(M.dets) + 8
    got, r = run_dev(M.detector(), M.x, max_det=big)
    M.check("default list", got)
    try:
        LQ.set_detector_list_capacity(1)   # the least the library takes: one tile's worth; the call runs in pieces
        got2, r2 = run_dev(M.detector(), M.x, max_det=big)
        got3 = run_host(M.detector(), M.x, (TILE + 100,), max_det=big)
    finally:
        LQ.set_detector_list_capacity(0)
    assert est_bits(got2) == est_bits(got) and est_bits(got3) == est_bits(got) and same_bits(r, r2)


# ------------------------------------------------------------------ 5 max_det
def test_max_det():
    M = repeated_model()
    full = run_host(M.detector(), M.x, max_det=len(M.dets) + 8)
    cnt, idx, tau, dphi, gam = M.detector().correlate_block(M.x, max_det=3, guard=2)
    assert cnt == len(M.dets) == len(full)
    assert list(idx[:3]) == [d[0] for d in full[:3]] and same_bits(tau[:3], [d[1] for d in full[:3]])
    assert np.all(idx[3:] == np.iinfo(np.uint32).max)
    for a in (tau, dphi, gam):
        assert np.all(a[3:] == np.float32(-77.0))
    # no outputs at all
    q = M.detector()
    n = LQ.lib().detector_cccf_correlate_block(q.q, LQ.ptr(M.x), len(M.x), None, None, None, None, 0)
    assert n == len(M.dets)


# ------------------------------------------------------------------ 6 mixed calls
def test_mixed_calls_and_reset():
    """a block call, 70 correlate calls, a block call: the model's detections;
    after reset the same bits again"""
    M = seam_model(-2)
    a = TILE - 40   # the per-sample stretch covers the peak next to the first seam

    def run(q):
        out = run_host(q, M.x[:a])
        for t in range(a, a + 70):
            e = q.correlate(M.x[t])
            if e:
                out.append((t,) + e)
        return out + [(a + 70 + i, t, p, g) for i, t, p, g in run_host(q, M.x[a + 70:])]

    q = M.detector()
    first = run(q)
    M.check("block, 70 samples, block", first)
    assert any(a <= d[0] < a + 70 for d in first)
    q.reset()
    assert est_bits(run(q)) == est_bits(first)


# ------------------------------------------------------------------ 7 same bits
@functools.lru_cache(maxsize=None)
def caller_stream():
    """a HIP stream of the test's own, from the runtime the library runs on"""
    LQ.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    hip = ctypes.CDLL(paths[0])
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    return s.value


def test_same_bits():
    M = seam_model(0)
    sizes = (1, 7, TILE + 1)
    dev, r = run_dev(M.detector(), M.x, sizes)
    M.check("device pointers", dev)
    M.check_rows("device pointers", r)
    # host pointers, the same call sizes
    assert est_bits(run_host(M.detector(), M.x, sizes)) == est_bits(dev)
    # a caller's stream
    q = M.detector()
    q.set_stream(caller_stream())
    dev2, r2 = run_dev(q, M.x, sizes)
    q.destroy()
    assert est_bits(dev2) == est_bits(dev) and same_bits(r2, r)
    # a reset object
    q = M.detector()
    run_dev(q, M.x[:TILE + 77], rows=False)
    q.reset()
    dev3, r3 = run_dev(q, M.x, sizes)
    assert est_bits(dev3) == est_bits(dev) and same_bits(r3, r)
    # input one sample, rows one float off 16-byte alignment; other call sizes (rows do not depend on the cut)
    dev4, r4 = run_dev(M.detector(), M.x, sizes, off_x=1, off_r=1)
    dev5, r5 = run_dev(M.detector(), M.x, (TILE,) * 3)
    assert est_bits(dev4) == est_bits(dev) and same_bits(r4, r)
    assert est_bits(dev5) == est_bits(dev) and same_bits(r5, r)


# ------------------------------------------------------------------ 8 the eligibility edge
@pytest.mark.parametrize("n", [MAX_LEN, MAX_LEN + 1])
def test_eligibility_edge(n):
    """the longest sequence the kernel takes and the first one the host loop
    takes: both meet the bound, on a stream of TILE + 5 samples"""
    s = DM.sequence(n)
    x = DM.envelope_stream("burst", TILE + 5, 77 + n, (TILE,), n)
    M = Model("edge n=%d" % n, s, 0.5, 0.0, x, margin=False)
    q = M.detector()
    assert q.device_eligible == (n <= MAX_LEN)
    _, r = run_dev(q, M.x, max_det=0)
    M.check_rows("kernel" if n <= MAX_LEN else "host loop", r)


def test_wide_bank_runs_in_the_host_loop():
    n = 64
    s = DM.sequence(n)
    x = DM.envelope_stream("burst", 300, 78, (150,), n)
    M = Model("wide bank", s, 0.5, dphi_max_for(n, MAX_M + 1), x, margin=False)
    q = M.detector()
    assert q.num_correlators == MAX_M + 1 and not q.device_eligible
    _, r = run_dev(q, M.x, max_det=0)
    M.check_rows("host loop", r)


# ------------------------------------------------------------------ 9 arguments
@pytest.mark.parametrize("args,msg", [("0, 0.5", "sequence length cannot be zero"),
                                      ("8, 0.0", "threshold must be greater than zero")])
def test_bad_arguments_exit(args, msg):
    code = ("import sys; sys.path.insert(0, %r); import numpy as np; import liquidmi as LQ; "
            "s = np.ones(8, np.complex64); n, thr = %s; LQ.lib().detector_cccf_create(LQ.ptr(s), n, thr, 0.0); "
            "print('survived')" % (os.path.dirname(os.path.abspath(LQ.__file__)), args))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert "error: detector_cccf_create(), " + msg in r.stderr and "survived" not in r.stdout
