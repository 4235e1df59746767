"""detector_cccf without a GPU: the model's state machine reproduces the
reference's recorded detections, the library's templates, correlator count and
per-sample path agree with the model, unmarked rows decide nothing, and three
mutations of the state machine each fail a named check (the checker is
pinned)."""
import ctypes
import re

import numpy as np
import pytest

import detector_model as DM
import liquidmi as LQ

FIX = DM.load_fixture()
CASES = FIX["cases"]
BY_NAME = {c["name"]: c for c in CASES}
IDS = [c[0] for c in DM.CASES]


def lib_correlate(q, x, base=0):
    out = []
    for t, v in enumerate(x):
        e = q.correlate(v)
        if e:
            out.append((base + t,) + e)
    return out


def test_fixture_covers_the_cases():
    assert [c["name"] for c in CASES] == IDS
    for c, d in zip(CASES, DM.CASES):
        assert (c["n"], c["N"], tuple(c["positions"]), c["seed"]) == (d[1], d[5], d[6], DM.SEEDS[d[0]])
        assert np.float32(c["threshold"]) == np.float32(d[2]) and np.float32(c["dphi_max"]) == np.float32(d[3])
        assert c["N"] <= 4 * c["n"] + 200
    assert [c["n"] for c in CASES[:10]] == list(DM.AUTOTEST_N)
    assert len(BY_NAME["missed"]["detections"]) == 1 and len(BY_NAME["stale"]["detections"]) == 2
    assert all(len(c["detections"]) == 1 for c in CASES[:10])


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_model_reproduces_the_reference(case):
    """the state machine over the reference-form rows (float32 serial sums,
    the running energy replayed): the recorded indices exactly, the recorded
    estimates within the propagated bound of the float64 ones; the float64
    form agrees on the indices (the margin condition, asserted by case_model)"""
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    rec = BY_NAME[case[0]]
    assert rec["m"] == bank.m
    rref, Eref = DM.serial32(bank, x, energy="running")
    got = DM.StateMachine(bank, case[2], np.float32).run(rref, Eref)
    assert [d["index"] for d in got] == [d[0] for d in rec["detections"]] == [d["index"] for d in dets64]
    DM.check_detections("reference " + case[0], rec["detections"], bank, r64, E64, bound, case[2], dets64)
    DM.check_detections("reference form " + case[0], [(d["index"], d["tau"], d["dphi"], d["gamma"]) for d in got],
                        bank, r64, E64, bound, case[2], dets64)


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_detections_sit_at_the_preamble_end(case):
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    ends = [p + case[1] for p in case[6]]
    want = ends if case[0] != "missed" else ends[:1]
    assert [d["index"] for d in dets64] == want
    if case[0] == "stale":   # the second detection reads its oldest row across the timer gap
        s0, s1, s2 = dets64[1]["src"]
        assert s0 == dets64[0]["index"] and s1 == s0 + case[1] // 4 + 1 and s2 == s1 + 1


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_serial_form_meets_the_bound(case):
    bank, s, x, r64, E64, bound, _ = DM.case_model(case)
    r32, _ = DM.serial32(bank, x)
    DM.check_rows("serial32 " + case[0], r32, r64, E64, bound)


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_unmarked_rows_decide_nothing(case):
    """with every row the kernel would not record replaced by NaN, for several
    call patterns, the detections are the same, estimates included"""
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    N = len(x)
    for calls in (None, [1, 7, 51, N - 59], [N // 3, N - N // 3], [64] * (N // 64) + [N % 64] * (N % 64 > 0)):
        mk = DM.marked(r64, case[2], calls)
        got = DM.StateMachine(bank, case[2]).run(r64, E64, poison=~mk)
        assert [(d["index"], d["tau"], d["dphi"]) for d in got] == [(d["index"], d["tau"], d["dphi"]) for d in dets64]
        assert mk.sum() < N


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_library_templates_and_count(case):
    """the library's templates against the float64 formula: within 2 ulp of
    |s[i]| per component"""
    bank, s = DM.case_model(case)[:2]
    q = LQ.Detector(s, case[2], case[3])
    assert q.num_correlators == bank.m
    p = q.templates().astype(np.complex128)
    tol = 2 * 2.0 ** -23 * np.abs(s.astype(np.complex128))[None, :]
    assert np.all(np.abs(p.real - bank.P.real) <= tol) and np.all(np.abs(p.imag - bank.P.imag) <= tol)


def test_num_correlators_rule():
    n = 100
    step = DM.step_of(n)
    s = DM.sequence(n)
    for dphi_max, want in ((0.0, 2), (1e-6, 2), (float(step), 2), (2 * float(step), 2), (3 * float(step), 3),
                           (float(np.nextafter(np.float32(3) * step, np.float32(1))), 4), (-3 * float(step), 3),
                           (-0.2, DM.num_correlators(n, 0.2)), (0.2, 8)):
        q = LQ.Detector(s, 0.5, dphi_max)
        assert q.num_correlators == want == DM.num_correlators(n, dphi_max), dphi_max


@pytest.mark.parametrize("case", DM.CASES, ids=IDS)
def test_library_correlate_reproduces_the_fixture(case):
    """the per-sample path, which runs on the host: indices exactly, estimates
    within the bound, and the recorded estimates of the reference alike"""
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    q = LQ.Detector(s, case[2], case[3])
    got = lib_correlate(q, x)
    assert [g[0] for g in got] == [d[0] for d in BY_NAME[case[0]]["detections"]]
    DM.check_detections("correlate " + case[0], got, bank, r64, E64, bound, case[2], dets64)
    # reset: the same bits again
    q.reset()
    again = lib_correlate(q, x)
    assert [tuple(np.float32(v).tobytes() for v in g[1:]) for g in again] == \
        [tuple(np.float32(v).tobytes() for v in g[1:]) for g in got]


def test_host_loop_block_calls_equal_the_per_sample_path():
    """a bank of 17 correlators is wider than the kernel takes, so its block
    calls run in the library's host loop and need no GPU: the stream through
    correlate_block split 1, 7, rest, and through correlate sample by sample,
    gives the model's detections with the same bits; indices are relative to
    their call"""
    n = 64
    s = DM.sequence(n)
    x = DM.stream(s, 700, [200, 200 + n // 4 + 2], 5, dphi=0.01)
    dphi_max = 16.5 * float(DM.step_of(n))
    bank = DM.Bank(s, dphi_max)
    r64, E64, bound = DM.rows64(bank, x)
    dets = DM.check_margin("host loop", bank, 0.5, r64, bound, E64)
    q = LQ.Detector(s, 0.5, dphi_max)
    assert q.num_correlators == 17 and not q.device_eligible
    a = lib_correlate(LQ.Detector(s, 0.5, dphi_max), x)
    b, base = [], 0
    for part in (x[:1], x[1:8], x[8:]):
        cnt, idx, tau, dphi, gam = q.correlate_block(part)
        assert cnt == len(idx) and np.all(idx < len(part))
        b += [(base + int(i), t, p, g) for i, t, p, g in zip(idx, tau, dphi, gam)]
        base += len(part)
    DM.check_detections("host loop 1, 7, rest", b, bank, r64, E64, bound, 0.5, dets)
    assert len(a) == len(dets) >= 1 and a == b


def test_zero_energy_rows_are_zero():
    """a stream with a stretch of exact zeros longer than the window: the
    per-sample path stays finite and still finds the preamble after it"""
    n = 64
    s = DM.sequence(n)
    pre = s * np.exp(0.01j * np.arange(n))   # off the middle of the two-correlator bank
    x = np.concatenate([DM.noise(100, 3), np.zeros(2 * n, np.complex64), pre, DM.noise(40, 4)]).astype(np.complex64)
    got = lib_correlate(LQ.Detector(s, 0.5, 0.02), x)
    assert [g[0] for g in got] == [100 + 2 * n + n] and all(np.isfinite(g[1:]).all() for g in got)


def test_header_and_library_export_the_interface():
    names = [n for n in LQ.header_functions() if re.match(r"detector_cccf_", n)]
    want = ["create", "destroy", "print", "reset", "correlate", "correlate_block", "correlate_block_dev",
            "get_num_correlators", "get_templates", "device_eligible", "set_stream", "synchronize"]
    assert sorted(names) == sorted("detector_cccf_" + w for w in want)
    L = ctypes.CDLL(LQ.LIB_PATH)
    consts = ["liquid_mi355x_detector_tile", "liquid_mi355x_detector_max_len", "liquid_mi355x_detector_max_correlators"]
    for nm in names + consts + ["liquid_mi355x_detector_set_list_capacity"]:
        assert hasattr(L, nm), nm
        assert nm in LQ.header_functions()
    assert LQ.Detector.TILE >= 64 and LQ.Detector.MAX_LEN >= 2048 and LQ.Detector.MAX_CORRELATORS >= 16


# ------------------------------------------------------------------ mutations that pin the checker
def _mutated(case, mutate):
    bank, s, x, r64, E64, bound, dets64 = DM.case_model(case)
    got = DM.StateMachine(bank, case[2], mutate=mutate).run(r64, E64)
    return [(d["index"], d["tau"], d["dphi"], d["gamma"]) for d in got], (bank, r64, E64, bound, case[2], dets64)


def test_mutation_timer_one_longer_fails_the_index_check():
    """n/4 + 1: the peak of the second preamble of "stale" falls inside the
    timer and the detection moves"""
    got, args = _mutated(DM.case_by_name("stale"), "timer+1")
    with pytest.raises(AssertionError, match="detections at"):
        DM.check_detections("timer+1", got, *args)


def test_mutation_rows_shift_during_the_timer_fails_the_estimate_check():
    """the second detection of "stale" then reads rxy0 from the sample before
    the peak instead of across the gap: tau_hat moves by far more than its bound"""
    got, args = _mutated(DM.case_by_name("stale"), "shift_in_timer")
    with pytest.raises(AssertionError, match="tau_hat"):
        DM.check_detections("shift_in_timer", got, *args)
    # and the unmutated machine passes the same check
    ok, args = _mutated(DM.case_by_name("stale"), None)
    DM.check_detections("unmutated", ok, *args)


def test_mutation_ge_in_findmax_fails_the_index_check():
    """>= for >: on two rows equal bit for bit FINDMAX goes on instead of
    reporting.  The library's per-sample path stands with > on that stream."""
    s, thr, dphi_max, x = DM.plateau_case()
    bank = DM.Bank(s, dphi_max)
    r64, E64, bound = DM.rows64(bank, x)
    want = DM.StateMachine(bank, thr).run(r64, E64)
    got = DM.StateMachine(bank, thr, mutate="ge").run(r64, E64)
    assert len(want) >= 1
    with pytest.raises(AssertionError, match="detections at"):
        DM.check_detections("ge", [(d["index"], d["tau"], d["dphi"], d["gamma"]) for d in got], bank, r64, E64, bound,
                            thr, want)
    lib = lib_correlate(LQ.Detector(s, thr, dphi_max), x)
    assert [g[0] for g in lib] == [d["index"] for d in want]
