"""The qdetector model (tests/qdetector_model.py) against the reference's
recorded behaviour (tests/golden/qdetector.json) and against itself, on the CPU:

  * the float32 serial restatement of the reference's loop meets the bound B
    on every window of every case, and detects where the float64 machine does;
  * the reference's recorded frames sit at the float64 machine's indices with
    estimates inside the propagated bounds, and the ten linear cases meet the
    autotest's own tolerances (0.05, 0.05, 0.01, 0.1 around tau = -0.3,
    gamma = 1, dphi = 0, phi = 0.5);
  * the cases are what they claim: a carrier on bin +3, a grid that restarts,
    a peak refused at index >= nfft - s_len and caught by the next window;
  * mutations pin the checker: a lag off by one, an offset off by one, a peak
    moved by 3 B and a grid restarted at the wrong sample are each rejected.
"""
import numpy as np
import pytest

import qdetector_model as QM

AUTOTEST = {"tau": QM.TAU, "gamma": 1.0, "dphi": 0.0, "phi": QM.PHI}
FIXTURE = QM.load_fixture()
_SERIAL = {}


def serial(name):
    if name not in _SERIAL:
        T, x, rng, _, _ = QM.case_model(name)
        _SERIAL[name] = QM.serial32(T, x, rng)
    return _SERIAL[name]


@pytest.mark.parametrize("name", QM.CASE_NAMES)
def test_serial_model_meets_bound(name):
    T, x, rng, wins, dets = QM.case_model(name)
    w32, d32 = serial(name)
    assert [p for p, _ in w32] == [p for p, _ in wins]
    worst = QM.check_records("serial " + name, T, [r for _, r in w32], wins)
    print("%s: serial worst %.4g of B" % (name, worst))
    QM.check_detections("serial " + name, d32, dets)


@pytest.mark.parametrize("name", QM.CASE_NAMES)
def test_reference_detections(name):
    T, x, rng, wins, dets = QM.case_model(name)
    fx = FIXTURE[name]
    assert (fx["s_len"], fx["nfft"]) == (T.s_len, T.nfft)
    QM.check_detections("reference " + name, fx["detections"], dets,
                        autotest=AUTOTEST if name.startswith("linear") else None)


def test_cases_are_what_they_claim():
    T, x, rng, wins, dets = QM.case_model("bin3")
    assert rng > 3 and [w[1][2] for w in wins if QM.detects(T, w[1], QM.THRESHOLD)] == [3]
    T, x, rng, wins, dets = QM.case_model("two_frames")
    assert len(dets) == 2
    h = T.nfft // 2
    first = dets[0][0] + h + 1 - T.nfft          # the first frame's position
    after = [p for p, _ in wins if p > first]
    assert after[0] == first + h and (first % h) != 0, "the grid restarts half a buffer into the frame"
    T, x, rng, wins, dets = QM.case_model("straddle")
    hits = [(p, r) for p, r in wins if r[0] > QM.THRESHOLD]
    assert len(hits) == 2 and hits[0][1][1] >= T.nfft - T.s_len and QM.detects(T, hits[1][1], QM.THRESHOLD)
    assert hits[1][0] == hits[0][0] + h and len(dets) == 1


def test_margin_refuses_a_close_call():
    T, x, rng, wins, dets = QM.case_model("straddle")
    peak = max(r[0] for _, r in wins)
    with pytest.raises(AssertionError):
        QM.check_margin("thr at the peak", T, wins, dets, thr=peak - T.bound(peak))


def test_mutations_are_rejected():
    T, x, rng, wins, dets = QM.case_model("two_frames")
    good = [r[:4] for _, r in wins]
    QM.check_records("unchanged", T, good, wins)
    k = next(i for i, (_, r) in enumerate(wins) if QM.detects(T, r, QM.THRESHOLD))

    def mutated(f):
        rec = list(good)
        rec[k] = f(rec[k])
        return rec
    for label, f in (("lag", lambda r: (r[0], r[1] + 1, r[2], r[3])),
                     ("offset", lambda r: (r[0], r[1], r[2] + 1, r[3])),
                     ("peak", lambda r: (r[0] + 3 * T.bound(r[0]), r[1], r[2], r[3]))):
        with pytest.raises(AssertionError):
            QM.check_records(label, T, mutated(f), wins)
    # a grid restarted one sample late: other windows, and the second frame is reported elsewhere or not at all
    wins2, dets2 = QM.walk64(T, x, rng, grid_shift=1)
    with pytest.raises(AssertionError):
        QM.check_records("grid", T, [r[:4] for _, r in wins2], wins)
    got = [(d[0], d[1]) for d in dets]
    QM.check_detections("unchanged", got, dets)
    with pytest.raises(AssertionError):
        QM.check_detections("index", [(got[0][0] + 1, got[0][1])] + got[1:], dets)
