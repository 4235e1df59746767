"""qdetector_cccf's walk (host/qdetector_walk.c) on its own, on the CPU:
tests/plan/qdetector_walk_test.c and the module are compiled here without HIP,
with the address and undefined-behaviour sanitizers, and run as a child
process.  That the two link with nothing but libc and libm shows the walk
needs no GPU.  The program is fed the window records and align scalars of the
Python model (tests/qdetector_model.py) and compares the windows consumed, the
detections, their indices, the estimates and the carried state with the model
across every cut of the stream into calls: one call, calls of 1, of nfft/2 - 1,
nfft/2 and nfft/2 + 1 samples, and a call that ends inside each align stage,
with 1, 3 and 5 windows per launch chunk.  A made-up scenario holds a hit at
index == 0 (the window is the frame) next to an ordinary one."""
import os
import subprocess

import numpy as np

import qdetector_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "liquid-dsp_amd", "host")


def _b(v):
    return str(int(np.array([v], np.float32).view(np.uint32)[0]))


def _scenario(nfft, s_len, s2, rng, N, wins, dets):
    """wins: [(pos, (peak, index, offset, energy))]; dets: [(pos, idx, i0, a[3], v[3], metric)]"""
    out = ["%d %d %s %s %d %d %d" % (nfft, s_len, _b(s2), _b(QM.THRESHOLD), rng, N, len(wins))]
    for pos, r in wins:
        out.append("%d %s %d %d %s" % (pos, _b(r[0]), r[1], r[2], _b(r[3])))
    out.append(str(len(dets)))
    for pos, idx, i0, a, v, metric in dets:
        a32, v32 = np.asarray(a, np.float32).astype(np.float64), np.asarray(v, np.float32).astype(np.float64)
        tau, gamma = QM.fit_tau_gamma(a32, nfft, float(np.float32(s2)))
        dphi = QM.fit_dphi(i0, v32, nfft)
        m = np.complex64(metric)
        est = (tau, gamma, dphi, np.angle(m))
        rxy = " ".join("%s %s" % (_b(x), _b(0.0)) for x in a)
        vv = " ".join("%s %s" % (_b(x), _b(0.0)) for x in v)
        out.append("%d %d %d %s %s %s %s %s" % (pos, idx, i0, rxy, vv, _b(m.real), _b(m.imag),
                                                 " ".join(_b(e) for e in est)))
    return out


def _from_model(name):
    T, x, rng, wins, dets = QM.case_model(name)
    h = T.nfft // 2
    dd = []
    for idx, est, _, al in dets:
        metric = np.sum(al["vt"] * np.exp(-1j * est["dphi"] * np.arange(T.s_len)))
        dd.append((idx + h + 1 - T.nfft, idx, al["i0"], al["a"], al["v"], metric))
    return _scenario(T.nfft, T.s_len, T.s2, rng, len(x), [(p, r[:4]) for p, r in wins], dd)


def _made_up():
    """nfft 16, s_len 4, 64 samples: a hit at index 0 in the window at 8 (frame
    at 8, complete with the window: idx 15, grid restarts at 16), one at index 3
    in the window at 32 (frame at 35, idx 42, grid restarts at 43)"""
    no, e = (0.1, 5, 0, 1.0), 1.0
    wins = [(0, no), (8, (0.9, 0, 1, e)), (16, no), (24, no), (32, (0.8, 3, -1, e)), (43, no), (51, no)]
    dets = [(8, 15, 1, (3.0, 5.0, 4.0), (2.0, 6.0, 3.0), 1 + 1j),
            (35, 42, 15, (2.0, 7.0, 2.5), (1.0, 4.0, 3.5), -1 + 0.5j)]
    return _scenario(16, 4, 4.0, 1, 64, wins, dets)


def test_walk_module_against_model(tmp_path):
    exe = str(tmp_path / "qdetector_walk_test")
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "liquid-dsp_amd", "csrc"),
                    "-I" + HOST, "-D__HIP_PLATFORM_AMD__", "-o", exe,
                    os.path.join(ROOT, "tests", "plan", "qdetector_walk_test.c"),
                    os.path.join(HOST, "qdetector_walk.c"), "-lm"], check=True)
    scen = [_made_up()] + [_from_model(n) for n in ("two_frames", "straddle", "bin3", "linear_n64")]
    path = tmp_path / "scenarios.txt"
    path.write_text("%d\n%s\n" % (len(scen), "\n".join("\n".join(s) for s in scen)))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("walk ok")
