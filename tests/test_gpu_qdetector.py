"""qdetector_cccf on the GPU against the float64 model (tests/qdetector_model.py):
routes, window records to the bound B and to 4x the serial model's own ratio,
offsets that wrap at both ends of S, the recorded reference cases through the
host call, the device call and per sample, and bit identity across call cuts,
pointer kinds, chunk seams, max_det, reset and streams.  Shapes are the
smallest that reach each seam: a few dozen windows at the most."""
import ctypes
import functools

import numpy as np
import pytest

import liquidmi as LQ
import qdetector_model as QM

pytestmark = pytest.mark.gpu
FIXTURE = QM.load_fixture()


def as_tuples(rec):
    return [(float(r["peak"]), int(r["index"]), int(r["offset"]), float(r["energy"])) for r in rec]


def got_detections(r):
    return [(int(r["idx"][k]), {n: float(r[n][k]) for n in QM.EST}) for k in range(len(r["idx"]))]


def same(a, b):
    """two block-call results, bit for bit"""
    assert a["count"] == b["count"] and a["num_records"] == b["num_records"]
    for k in ("idx",) + QM.EST:
        assert np.array_equal(a[k].view(np.uint32 if a[k].dtype == np.float32 else np.uint64),
                              b[k].view(np.uint32 if b[k].dtype == np.float32 else np.uint64)), k
    for k in ("records", "frames"):
        if k in a and k in b:
            assert a[k].tobytes() == b[k].tobytes(), k


def run_cut(q, x, cuts, dev=False, max_det=4, shift=0):
    """the stream through calls that end at `cuts`; one merged result.  dev:
    device pointers, the input `shift` samples off its allocation's start"""
    nfft = q.nfft
    out = {"count": 0, "num_records": 0, "idx": [], "records": [], "frames": [], **{n: [] for n in QM.EST}}
    if dev:
        dx = LQ.DeviceBuffer.from_array(np.concatenate([np.zeros(shift, np.complex64), x]))
        nr_max = 1 + (len(x) + nfft) // (nfft // 2)
        dr, df = LQ.DeviceBuffer(nr_max * 16), LQ.DeviceBuffer(max_det * nfft * 8)
    start = 0
    for end in list(cuts) + [len(x)]:
        if end <= start:
            continue
        n = end - start
        if dev:
            r = q.execute_block_dev(dx.p + 8 * (shift + start), n, max_det, df.p, dr.p)
            r["records"] = dr.to_array(QM_REC, max(r["num_records"], 1))[:r["num_records"]]
            r["frames"] = df.to_array(np.complex64, max_det * nfft).reshape(max_det, nfft)[:len(r["idx"])]
        else:
            r = q.execute_block(x[start:end], max_det, frames=True)
        out["count"] += r["count"]
        out["num_records"] += r["num_records"]
        out["idx"] += [int(v) + start for v in r["idx"]]
        for k in QM.EST:
            out[k] += list(r[k])
        out["records"].append(r["records"])
        out["frames"].append(r["frames"])
        start = end
    out["idx"] = np.array(out["idx"], np.uint64)
    for k in QM.EST:
        out[k] = np.array(out[k], np.float32)
    out["records"] = np.concatenate(out["records"])
    out["frames"] = np.concatenate(out["frames"])
    return out


QM_REC = LQ.QDETECTOR_RECORD


def test_routes():
    for nfft in (512, 1024):
        for nw in (1, 8, 1 << 20):
            assert LQ.qdetector_route(nfft, QM.range_of(0.3, nfft), nw) == "fused"
        assert LQ.qdetector_route(nfft, 0, 1) == "fused"
    for nfft in (2, 8, 16, 64, 256, 2048, 8192):      # no separate trivial kernel: the composed path from 2 up
        for nw in (1, 8, 4096):
            assert LQ.qdetector_route(nfft, QM.range_of(0.3, nfft), nw) == "composed"
    try:
        LQ.set_qdetector_route("composed")           # the measurements' override is visible to the query
        assert LQ.qdetector_route(512) == LQ.qdetector_route(1024) == "composed"
    finally:
        LQ.set_qdetector_route(None)
    assert LQ.qdetector_route(512) == "fused"


@functools.lru_cache(maxsize=None)
def record_case(s_len, dphi_max, nwin=10):
    """bursts on the floor, one all-zero window ahead of them; model records and the serial ratio"""
    s = QM.chips(s_len, 300 + s_len)
    T = QM.Template(s)
    n, h = T.nfft, T.nfft // 2
    N = nwin * h
    x = QM.burst_stream(s, N, (4 * h + h // 3,), 400 + s_len, bin_=0).astype(np.complex64)
    x[h:h + n] = 0                       # the window at ext position 2h
    rng = QM.range_of(dphi_max, n)
    # 64 lags of floor noise against 32 chips reach 0.5 now and then: the short templates take a higher threshold
    thr = 0.8 if n <= 128 else QM.THRESHOLD
    wins, dets = QM.walk64(T, x, rng, thr)
    QM.check_margin("records %d" % s_len, T, wins, dets, thr)
    assert any(w[1][3] == 0.0 for w in wins) and len(dets) == 1, (len(wins), len(dets))
    w32, _ = QM.serial32(T, x, rng, thr)
    serial_worst = max(QM.record_ratio(T, a[1], b[1]) for a, b in zip(w32, wins) if b[1][3] > 0)
    return T, x, rng, wins, dets, serial_worst, thr


# s_len = nfft/2 exactly, and just above a power of two (the smallest s_len / nfft, the largest B)
@pytest.mark.parametrize("s_len", (32, 33, 128, 129, 256, 257, 512, 513, 1025, 2049))
@pytest.mark.parametrize("want_range", (0, 1, None))
def test_records(s_len, want_range):
    check_records_on_gpu(s_len, want_range)


@pytest.mark.parametrize("s_len", (129, 256, 257, 512))
def test_records_composed_path_at_fused_sizes(s_len):
    try:
        LQ.set_qdetector_route("composed")
        check_records_on_gpu(s_len, None)
    finally:
        LQ.set_qdetector_route(None)


@pytest.mark.parametrize("s_len", (1, 3, 8))
def test_small_sizes(s_len):
    """nfft 2, 8, 16 (the composed path's smallest transforms): records against the model; the
    threshold is one no peak reaches (a peak is at most sqrt(nfft / s_len) < 2), so the grid never moves"""
    s = QM.chips(s_len, 50 + s_len)
    T = QM.Template(s)
    n = T.nfft
    rng = QM.range_of(0.5, n)
    assert n == (2, 8, 16)[(1, 3, 8).index(s_len)] and rng == (0, 0, 1)[(1, 3, 8).index(s_len)]
    x = QM.burst_stream(s, 24 * n, (5 * n + 1, 14 * n + n // 2), 60 + s_len)
    x[2 * n:3 * n] = 0
    wins, dets = QM.walk64(T, x, rng, 2.0)
    assert len(wins) == 2 * 24 and not dets and any(w[1][3] == 0.0 for w in wins)
    q = LQ.QDetector(s)
    q.set_range(0.5)
    q.set_threshold(2.0)
    r = q.execute_block(x)
    assert r["count"] == 0
    QM.check_records("nfft %d" % n, T, as_tuples(r["records"]), wins, thr=2.0)
    q2 = LQ.QDetector(s)
    q2.set_range(0.5)
    q2.set_threshold(2.0)
    cut = run_cut(q2, x, range(1, len(x)), dev=True)
    assert cut["records"].tobytes() == r["records"].tobytes()


def check_records_on_gpu(s_len, want_range):
    nfft = QM.nfft_of(s_len)
    dphi_max = 0.3 if want_range is None else 2 * np.pi * (want_range + 0.5) / nfft
    T, x, rng, wins, dets, serial_worst, thr = record_case(s_len, float(dphi_max), 8 if nfft == 8192 else 10)
    assert rng == (QM.range_of(0.3, nfft) if want_range is None else want_range)
    q = LQ.QDetector(T.s)
    q.set_range(dphi_max)
    q.set_threshold(thr)
    assert q.range == rng
    r = q.execute_block(x, frames=True)
    worst = QM.check_records("nfft %d" % nfft, T, as_tuples(r["records"]), wins, thr=thr)
    print("nfft %d s_len %d range %d: worst %.4g of B, serial %.4g" % (nfft, s_len, rng, worst, serial_worst))
    assert worst <= 4 * serial_worst, "%.4g of B, the serial model stays within %.4g" % (worst, serial_worst)
    QM.check_detections("nfft %d" % nfft, got_detections(r), dets)
    a = dets[0][0] - nfft + 1                  # the frame's position in x
    assert np.array_equal(r["frames"][0], x[a:a + nfft])


@pytest.mark.parametrize("s_len,dphi_max", ((100, 0.2), (300, 0.05)))
def test_offsets_wrap(s_len, dphi_max):
    s = QM.chips(s_len, 77)
    T = QM.Template(s)
    n = T.nfft
    rng = QM.range_of(dphi_max, n)
    assert rng == 8
    x = (QM.burst_stream(s, 12 * n, (2 * n + 17,), 5, bin_=-rng).astype(np.complex128)
         + QM.burst_stream(s, 12 * n, (7 * n + 5,), 6, bin_=rng, nfft=n)).astype(np.complex64)
    wins, dets = QM.walk64(T, x, rng)
    QM.check_margin("wrap", T, wins, dets)
    assert [w[1][2] for w in wins if QM.detects(T, w[1], QM.THRESHOLD)] == [-rng, rng]
    q = LQ.QDetector(s)
    q.set_range(dphi_max)
    r = q.execute_block(x)
    QM.check_records("wrap", T, as_tuples(r["records"]), wins)
    QM.check_detections("wrap", got_detections(r), dets)


@pytest.mark.parametrize("name", QM.CASE_NAMES)
def test_fixture_cases(name):
    T, x, rng, wins, dets = QM.case_model(name)
    kind, a, _, dmax = QM.case_inputs(name)
    ref = FIXTURE[name]["detections"]
    auto = {"tau": QM.TAU, "gamma": 1.0, "dphi": 0.0, "phi": QM.PHI} if kind == "linear" else None

    def make():
        q = LQ.QDetector(a, linear=("arkaiser", QM.K, QM.M, QM.BETA) if kind == "linear" else None)
        if dmax is not None:
            q.set_range(dmax)
        assert (q.s_len, q.nfft, q.range) == (T.s_len, T.nfft, rng)
        return q
    q = make()
    if kind == "linear":     # the template the library built, against the model's
        assert np.max(np.abs(q.sequence() - T.s)) <= 8 * QM.EPS * np.max(np.abs(T.s))
    rb = q.execute_block(x, frames=True)
    QM.check_records(name, T, as_tuples(rb["records"]), wins)
    QM.check_detections(name, got_detections(rb), dets, autotest=auto)
    assert [d[0] for d in ref] == [int(v) for v in rb["idx"]]
    rd = run_cut(make(), x, (), dev=True)
    same(rb, rd)
    q = make()
    got = []
    for i, v in enumerate(x):
        fr = q.execute(v)
        if fr is not None:
            got.append((i, dict(zip(QM.EST, q.estimates())), fr))
    assert [g[0] for g in got] == [int(v) for v in rb["idx"]]
    for k, g in enumerate(got):
        assert [np.float32(g[1][n]).tobytes() for n in QM.EST] == [rb[n][k].tobytes() for n in QM.EST]
        assert np.array_equal(g[2], rb["frames"][k])


@functools.lru_cache(maxsize=None)
def two_frames(s_len):
    s = QM.chips(s_len, 21)
    T = QM.Template(s)
    n = T.nfft
    x = QM.burst_stream(s, 10 * n, (2 * n + 37, 6 * n + 11), 9, bin_=1)
    rng = QM.range_of(0.3, n)
    wins, dets = QM.walk64(T, x, rng)
    QM.check_margin("two frames", T, wins, dets)
    assert len(dets) == 2
    return s, T, x, dets


@pytest.mark.parametrize("s_len", (100, 200, 300))   # composed (nfft 256), fused (nfft 512 and 1024)
def test_call_cuts(s_len):
    s, T, x, dets = two_frames(s_len)
    n, h = T.nfft, T.nfft // 2
    whole = run_cut(LQ.QDetector(s), x, ())
    QM.check_detections("whole", got_detections(whole), dets)
    inside = dets[0][0] - 3                            # a call that ends inside the align stage
    patterns = [range(1, len(x)), range(h - 1, len(x), h - 1), range(h + 1, len(x), h + 1), (inside,),
                (inside, inside + 1, dets[1][0])]
    for cuts in patterns:
        same(whole, run_cut(LQ.QDetector(s), x, cuts))
        same(whole, run_cut(LQ.QDetector(s), x, cuts, dev=True))
        same(whole, run_cut(LQ.QDetector(s), x, cuts, dev=True, shift=1))    # 8 bytes off the allocation's start
    same(whole, run_cut(LQ.QDetector(s), x, (), dev=True))
    # per-sample and block calls mixed on one object
    q = LQ.QDetector(s)
    k0 = dets[0][0] - n // 3
    for v in x[:k0]:
        assert q.execute(v) is None
    r = q.execute_block(x[k0:], frames=True)
    assert [int(v) + k0 for v in r["idx"]] == [int(v) for v in whole["idx"]]
    assert r["frames"].tobytes() == whole["frames"].tobytes()
    assert all(r[k].tobytes() == whole[k].tobytes() for k in QM.EST)


@pytest.mark.parametrize("s_len", (100, 200, 300))
def test_chunk_seams(s_len):
    s, T, x, dets = two_frames(s_len)
    assert LQ.qdetector_chunk(T.nfft) > 2 * len(x) // T.nfft     # the default takes the stream in one launch
    whole = run_cut(LQ.QDetector(s), x, ())
    try:
        for chunk in (1, 2, 3, 5, 7):   # every window is in turn the last of a chunk and the first of the next
            LQ.set_qdetector_chunk(chunk)
            assert LQ.qdetector_chunk(T.nfft) == chunk
            same(whole, run_cut(LQ.QDetector(s), x, ()))
            same(whole, run_cut(LQ.QDetector(s), x, (dets[0][0] - 3,), dev=True))
    finally:
        LQ.set_qdetector_chunk(0)


def test_max_det_smaller_than_frames():
    s, T, x, dets = two_frames(100)
    whole = run_cut(LQ.QDetector(s), x, ())
    q = LQ.QDetector(s)
    cut = dets[1][0] + 1 + T.nfft
    r = q.execute_block(x[:cut], max_det=1, frames=True)
    assert r["count"] == 2 and len(r["idx"]) == 1 and int(r["idx"][0]) == dets[0][0]
    assert r["frames"].tobytes() == whole["frames"][:1].tobytes()
    assert q.estimates() == tuple(whole[k][1] for k in QM.EST)      # the object holds the last frame's
    r2 = q.execute_block(x[cut:])
    assert r2["count"] == 0
    nrec = r["num_records"]
    assert r2["records"].tobytes() == whole["records"][nrec:].tobytes()


def caller_stream():
    """a HIP stream of the test's own, from the runtime the library runs on"""
    LQ.lib()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda p: "/torch/" in p)
    hip = ctypes.CDLL(paths[0])
    s = ctypes.c_void_p()
    assert hip.hipStreamCreate(ctypes.byref(s)) == 0
    return s.value


def test_lifecycle():
    s, T, x, dets = two_frames(100)
    whole = run_cut(LQ.QDetector(s), x, ())
    q = LQ.QDetector(s)
    assert (q.threshold, q.range) == (0.5, QM.range_of(0.3, T.nfft))
    q.set_threshold(3.0)                       # out of range: ignored
    q.set_range(0.6)
    assert (q.threshold, q.range) == (0.5, QM.range_of(0.3, T.nfft))
    # a threshold no peak reaches hides the first frame; set back, the second is found
    q.set_threshold(2.0)
    mid = dets[0][0] + 1 + T.nfft
    r1 = q.execute_block(x[:mid])
    assert r1["count"] == 0
    q.set_threshold(0.5)
    q.set_range(0.0)                           # takes effect on the next window: offsets all 0
    r2 = q.execute_block(x[mid:])
    assert r2["num_records"] > 4 and not r2["records"]["offset"].any()
    q.set_range(0.3)
    q.reset()
    same(whole, run_cut(q, x, ()))             # the state after create
    q2 = LQ.QDetector(s)
    q2.set_stream(caller_stream())
    same(whole, run_cut(q2, x, (dets[0][0] - 3,)))
    q2.synchronize()
