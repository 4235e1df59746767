"""Throughput of the widened rows (SURVEY §8 a3-a11 variants and §8f), device
resident, against the HBM roofline (dev tool; the headline is bench.py).

One JSON object per workload: kernel time per call from HIP events on the
objects' stream (20 warm-up + 30 timed calls), samples/s and algorithmic
GB/s (bytes stated per workload) as a fraction of the 8 TB/s spec.
    python tools/bench_widened.py > gpurun_out/widened.json
    python tools/bench_widened.py --halfband      (the resamp2 / firhilbf / msresamp rows alone)
    python tools/bench_widened.py --iir           (the iirfilt, iirdecim and iirinterp rows alone)
    python tools/bench_widened.py --autocorr      (the autocorr rows alone)
    python tools/bench_widened.py --detector      (the detector_cccf rows alone)
    python tools/bench_widened.py --qdetector     (the qdetector_cccf rows alone)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "liquid-dsp_amd"))
import liquidmi as LQ  # noqa: E402

PEAK = 8000.0
STREAM = torch.cuda.Stream()
S = STREAM.cuda_stream


def timed(fn, it=30, w=20, floor_ms=150.0):
    """w warm-up calls, then more until floor_ms of wall time (clock ramp, as
    bench.py), then `it` timed calls"""
    import time
    t0 = time.perf_counter()
    for _ in range(w):
        fn()
    torch.cuda.synchronize()
    while (time.perf_counter() - t0) * 1e3 < floor_ms:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(STREAM)
    for _ in range(it):
        fn()
    e1.record(STREAM)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


def cbuf(n, seed=1):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand(2 * n, generator=g, device="cuda") - 0.5


def rbuf(n, seed=1):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.rand(n, generator=g, device="cuda") - 0.5


def report(name, ms, units, unit_name, nbytes, note):
    gbps = nbytes / (ms * 1e-3) / 1e9
    print(json.dumps({"workload": name, "ms": round(ms, 4), "value": units / (ms * 1e-3) / 1e6,
                      "unit": "M %s/s" % unit_name, "achieved_GBps": round(gbps, 1),
                      "frac_of_8TBps": round(gbps / PEAK, 3), "bytes": note}))
    sys.stdout.flush()


def halfband_rows(L):
    """resamp2 decim / interp (m = 12), the firhilbf rows next to them (same
    structure, less arithmetic per byte), msresamp r = 0.3 / 3.3"""
    n = 1 << 26
    x = cbuf(n)
    y = torch.empty(2 * 4 * n, device="cuda")
    r2 = LQ.Resamp2(12, 0.0, 60.0)
    r2.set_stream(S)
    ms = timed(lambda: L.resamp2_crcf_execute_block_dev(r2.q, LQ.RESAMP2_DECIM, x.data_ptr(), n // 2,
                                                         y.data_ptr(), None))
    report("resamp2_crcf decim m=12", ms, n, "input samples", 8 * n + 4 * n, "8 B/input + 8 B/output")
    ms = timed(lambda: L.resamp2_crcf_execute_block_dev(r2.q, LQ.RESAMP2_INTERP, x.data_ptr(), n,
                                                         y.data_ptr(), None))
    report("resamp2_crcf interp m=12", ms, n, "input samples", 8 * n + 16 * n, "8 B/input + 16 B/output")
    # firhilbf: 2^26 real inputs -> 2^25 complex outputs; 2^25 complex inputs -> 2^26 real outputs
    fh = LQ.FirHilb(12, 60.0)
    fh.set_stream(S)
    nc = n // 2
    ms = timed(lambda: fh.decim_block_dev(x.data_ptr(), nc, y.data_ptr()))
    report("firhilbf decim m=12", ms, n, "input samples", 16 * nc, "8 B in + 8 B out per output")
    ms = timed(lambda: fh.interp_block_dev(x.data_ptr(), nc, y.data_ptr()))
    report("firhilbf interp m=12", ms, nc, "input samples", 16 * nc, "8 B in + 8 B out per input")
    fh.destroy()
    for rate in (0.3, 3.3):
        ms_ = LQ.MsResamp(rate, 60.0)
        ms_.set_stream(S)
        nin = n if rate < 1 else n // 4
        nout = ms_.num_output(nin)
        ms = timed(lambda: ms_.execute_block_dev(x.data_ptr(), nin, y.data_ptr()))
        report("msresamp_crcf r=%g" % rate, ms, nin, "input samples", 8 * nin + 8 * nout,
               "8 B/input + 8 B/output")
        ms_.destroy()


def iir_rows(L):
    """iirfilt_crcf, 2^26 samples in place in device memory: the DC blocker (one
    section) and a 4-section cascade (Butterworth order 8, fc 0.1, the sections
    from scipy).  16 B/sample algorithmic; the kernels move 24 (the tile pass
    reads x, the apply pass reads it again and writes y).  Then the device path
    against the library's host loop at 2^20 samples, host pointers, wall clock."""
    import time

    import numpy as np
    from scipy.signal import butter
    n = 1 << 26
    x = cbuf(n)
    sos = butter(8, 0.2, output="sos").astype(np.float32)
    filters = (("iirfilt_crcf dc_blocker alpha=0.01", lambda: LQ.IirFilt.dc_blocker("crcf", 0.01)),
               ("iirfilt_crcf 4 sections (butter 8, fc 0.1)", lambda: LQ.IirFilt.sos("crcf", sos[:, :3], sos[:, 3:])))
    for name, mk in filters:
        q = mk()
        assert q.device_eligible
        q.set_stream(S)
        ms = timed(lambda: q.execute_block_dev(x.data_ptr(), n, x.data_ptr()))
        report(name, ms, n, "samples", 16 * n, "16 B/sample algorithmic (24 B/sample moved)")
        q.destroy()
    iir_rate_rows(x, n)
    del x
    nh = 1 << 20
    xh = (np.random.default_rng(1).uniform(-0.5, 0.5, 2 * nh).astype(np.float32)).view(np.complex64)
    # the host loop runs the objects that are not device-eligible: the same forms with one pole
    # moved to radius 1 + 1e-7 (same arithmetic per sample; grows by 1.1 over 2^20 samples)
    out = sos.copy()
    out[3, 5] = np.float32(1.0000002)
    hosts = (lambda: LQ.IirFilt("crcf", [1.0, -1.0], [1.0, -1.0000002]),
             lambda: LQ.IirFilt.sos("crcf", out[:, :3], out[:, 3:]))
    for (name, mk), mkh in zip(filters, hosts):
        res = {}
        for key, make, want in (("device_ms", mk, True), ("host_loop_ms", mkh, False)):
            q = make()
            assert q.device_eligible == want
            q.execute_block(xh)
            t0 = time.perf_counter()
            for _ in range(3):
                q.execute_block(xh)
            res[key] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
            q.destroy()
        print(json.dumps(dict({"workload": name + ", 2^20 samples, host pointers, wall clock"}, **res)))
        sys.stdout.flush()


def iir_rate_rows(x, n):
    """iirdecim_crcf / iirinterp_crcf at n full-rate samples in device memory, M = 2, 4, 16, a
    one-section filter (the DC blocker's size) and Butterworth 8 (create_default: 4 sections), each
    measured fused (the object) and composed as it could be before these objects existed:
    IirFilt.execute_block_dev plus a torch strided copy (decimator) or a zero-stuff (interpolator).
    Bytes per full-rate sample by count: fused decimator 16 + 8/M, fused interpolator 8 + 16/M,
    composed decimator 32 + 8/M, composed interpolator 32 + 16/M."""
    full = torch.empty(2 * n, device="cuda")
    y = torch.empty(2 * n, device="cuda")
    one_b, one_a = [1.0, -1.0], [1.0, -0.99]
    for M in (2, 4, 16):
        m = n // M
        for fname, rate, plain in (
                ("1 section", lambda c: c("crcf", M, one_b, one_a), lambda: LQ.IirFilt("crcf", one_b, one_a)),
                ("butter 8 (4 sections)", lambda c: c.default("crcf", M, 8),
                 lambda: LQ.IirFilt.lowpass("crcf", 8, 0.5 / M))):
            d, i, f = rate(LQ.IirDecim), rate(LQ.IirInterp), plain()
            for q in (d, i, f):
                assert q.device_eligible
                q.set_stream(S)
            ms = timed(lambda: d.execute_block_dev(x.data_ptr(), m, y.data_ptr()))
            report("iirdecim_crcf M=%d %s, fused" % (M, fname), ms, n, "input samples", 16 * n + 8 * m,
                   "16 + 8/M B per input sample")

            def composed_decim():
                f.execute_block_dev(x.data_ptr(), n, full.data_ptr())
                with torch.cuda.stream(STREAM):
                    y.view(-1, 2)[:m].copy_(full.view(-1, 2)[::M])
            ms = timed(composed_decim)
            report("iirdecim_crcf M=%d %s, composed (iirfilt + strided copy)" % (M, fname), ms, n, "input samples",
                   32 * n + 8 * m, "32 + 8/M B per input sample")
            ms = timed(lambda: i.execute_block_dev(x.data_ptr(), m, y.data_ptr()))
            report("iirinterp_crcf M=%d %s, fused" % (M, fname), ms, n, "output samples", 8 * n + 16 * m,
                   "8 + 16/M B per output sample")

            def composed_interp():
                with torch.cuda.stream(STREAM):
                    full.zero_()
                    full.view(-1, 2)[::M] = x.view(-1, 2)[:m]
                f.execute_block_dev(full.data_ptr(), n, y.data_ptr())
            ms = timed(composed_interp)
            report("iirinterp_crcf M=%d %s, composed (zero-stuff + iirfilt)" % (M, fname), ms, n, "output samples",
                   32 * n + 16 * m, "32 + 16/M B per output sample")
            for q in (d, i, f):
                q.destroy()
    del full, y


def autocorr_rows(L):
    """autocorr_cccf, 2^26 samples in device memory, (W, d) = (64, 32), (1024, 1024), (4096, 1), without
    and with the e2 output: 16 B/sample (8 in, 8 out), 20 with e2.  Beside each shape the same result
    composed from what the library had before the object: a torch product x[d:] conj(x[:-d]) and a
    FirFilt("crcf", ones(W)) over it (24 B/sample for the product, 16 for the filter).  Last, the time of the
    W = 4096 row over the W = 64 row next to the growth the design predicts, the ratio of their halo
    ratios (TILE + W - 1) / TILE."""
    import numpy as np
    n = 1 << 26
    x = cbuf(n)
    y = torch.empty(2 * n, device="cuda")
    e2 = torch.empty(n, device="cuda")
    prod = torch.empty(2 * n, device="cuda")
    xc, pc = torch.view_as_complex(x.view(-1, 2)), torch.view_as_complex(prod.view(-1, 2))
    tile = LQ.AutoCorr.TILE
    ms_of = {}
    for W, d in ((64, 32), (1024, 1024), (4096, 1)):
        q = LQ.AutoCorr("cccf", W, d)
        assert q.device_eligible
        q.set_stream(S)
        for with_e2 in (False, True):
            ms = timed(lambda: q.execute_block_dev(x.data_ptr(), n, y.data_ptr(), e2.data_ptr() if with_e2 else 0))
            report("autocorr_cccf W=%d d=%d%s" % (W, d, " + e2" if with_e2 else ""), ms, n, "samples",
                   (20 if with_e2 else 16) * n, "20 B/sample" if with_e2 else "16 B/sample")
            ms_of[(W, with_e2)] = ms
        q.destroy()
        f = LQ.FirFilt("crcf", np.ones(W, np.float32))
        f.set_stream(S)

        def composed():
            with torch.cuda.stream(STREAM):
                torch.mul(xc[d:], xc[:n - d].conj(), out=pc[:n - d])
            f.execute_block_dev(prod.data_ptr(), n - d, y.data_ptr())
        ms = timed(composed, it=5, w=2)
        report("autocorr_cccf W=%d d=%d, composed (torch product + firfilt_crcf of ones)" % (W, d), ms, n, "samples",
               40 * n, "24 B/sample product + 16 B/sample filter")
        f.destroy()
    halo = lambda W: (tile + W - 1) / tile  # noqa: E731
    print(json.dumps({"workload": "autocorr_cccf W=4096 over W=64", "time_ratio": round(ms_of[(4096, False)] / ms_of[(64, False)], 3),
                      "time_ratio_with_e2": round(ms_of[(4096, True)] / ms_of[(64, True)], 3),
                      "halo_ratio_W4096": round(halo(4096), 3), "halo_ratio_W64": round(halo(64), 3),
                      "predicted_growth": round(halo(4096) / halo(64), 3)}))
    sys.stdout.flush()


def detector_rows(L):
    """detector_cccf, 2^24 samples of noise in device memory (nothing crosses the threshold: the decision
    pass sees the call's first and last sample and one word of flags per tile), (n, m) = (64, 2), (256, 4), (1341, 11) and (512, 16: a bank the
    kernel walks in two halves), without and with the rows in drxy.  A call returns its detections in host memory, so the time of a call (events around
    synchronous calls) holds the kernel, the copy of the marked list and the host pass; the kernel alone is
    timed through lqk_detector, and the difference is the decision pass's share.  8 m n flops per sample
    against the 157.3 TFLOP/s float32 vector peak.  Beside each shape the same rows composed from what the
    library had before the object: m firfilt_cccf with the reversed templates, autocorr_cccf's e2 for the
    energy, and a torch normalise and row maximum.  Every side is timed three times in turn with the same
    counts (3 warm-up calls, 10 timed); "ms" is the median, "runs_ms" all three."""
    import ctypes as C

    import numpy as np
    n = 1 << 24
    peak = 157.3e12
    x = cbuf(n)
    xc = torch.view_as_complex(x.view(-1, 2))
    rng = np.random.default_rng(3)
    for ln, m in ((64, 2), (256, 4), (1341, 11), (512, 16)):
        s = (rng.integers(0, 2, ln) * 2.0 - 1.0).astype(np.complex64)
        dphi_max = 0.0 if m == 2 else (m - 0.5) * 0.8 * np.pi / ln
        q = LQ.Detector(s, 0.6, dphi_max)
        assert q.device_eligible and q.num_correlators == m
        q.set_stream(S)
        drxy = torch.empty(n * m, device="cuda")
        cnt = [0]

        def call(rows):
            cnt[0] = q.correlate_block_dev(x.data_ptr(), n, drxy.data_ptr() if rows else 0, max_det=4)[0]
        # the kernel alone
        P = q.templates()
        pad = (ln + 3) & ~3
        pt = np.zeros((pad, m), np.complex64)
        pt[:ln] = P.T
        dpt = torch.view_as_real(torch.from_numpy(pt).cuda()).contiguous()
        hist = torch.zeros(2 * 2 * ln, device="cuda")
        cap = 1 << 17
        nt = (n + LQ.Detector.TILE - 1) // LQ.Detector.TILE
        lst = torch.zeros(4 + nt + cap * (2 + m), dtype=torch.int32, device="cuda")
        edge = torch.zeros(2 * nt * (2 + m), dtype=torch.int32, device="cuda")
        fn = L.lqk_detector
        fn.restype = None
        fn.argtypes = [C.c_uint, C.c_uint, C.c_float] + [C.c_void_p] * 3 + [C.c_ulonglong, C.c_void_p, C.c_void_p,
                                                                           C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]

        def kernel(rows):
            fn(ln, m, 0.6, dpt.data_ptr(), hist.data_ptr(), x.data_ptr(), n, drxy.data_ptr() if rows else None,
               lst.data_ptr(), cap, edge.data_ptr(), hist.data_ptr() + 8 * ln, S)
        # the composition: m firfilt_cccf + autocorr e2 + torch
        filts = []
        for k in range(m):
            f = LQ.FirFilt("cccf", np.ascontiguousarray(P[k][::-1]))
            f.set_stream(S)
            filts.append(f)
        ac = LQ.AutoCorr("cccf", ln, 0)
        ac.set_stream(S)
        y = torch.empty(m, 2 * n, device="cuda")
        rxx = torch.empty(2 * n, device="cuda")
        e2 = torch.empty(n, device="cuda")
        rmax = torch.empty(n, device="cuda")
        yc = torch.view_as_complex(y.view(m, n, 2))

        def composed():
            for k, f in enumerate(filts):
                f.execute_block_dev(x.data_ptr(), n, y[k].data_ptr())
            ac.execute_block_dev(x.data_ptr(), n, rxx.data_ptr(), e2.data_ptr())
            with torch.cuda.stream(STREAM):
                r = yc.abs() / torch.sqrt(e2 * float(ln))[None, :]
                torch.amax(r, dim=0, out=rmax)
        # three rounds over all five, the same warm-up and iteration counts for each; the median counts
        sides = (("call", lambda: call(False)), ("call + drxy", lambda: call(True)), ("kernel", lambda: kernel(False)),
                 ("kernel + drxy", lambda: kernel(True)), ("composed", composed))
        runs = {k: [] for k, _ in sides}
        for _ in range(3):
            for k, f in sides:
                runs[k].append(timed(f, it=10, w=3))
        med = {k: sorted(v)[1] for k, v in runs.items()}
        for k, _ in sides:
            row = {"workload": "detector_cccf n=%d m=%d, %s" % (ln, m, k), "ms": round(med[k], 4),
                   "runs_ms": [round(v, 4) for v in runs[k]]}
            if k != "composed":
                row["frac_of_fp32_vector_peak"] = round(8.0 * m * ln * n / (med[k] * 1e-3) / peak, 3)
            if k.startswith("call"):
                row["decision_pass_share_of_call"] = round(max(1.0 - med[k.replace("call", "kernel")] / med[k], 0.0), 4)
                row["over_composed"] = round(med[k] / med["composed"], 4)
                row["detections"] = cnt[0]
            print(json.dumps(row))
        sys.stdout.flush()
        q.destroy()
        for f in filts:
            f.destroy()
        ac.destroy()
        del y, yc, drxy, rxx, e2, rmax


def qdetector_rows(L):
    """qdetector_cccf, 2^24 samples of noise in device memory (no window detects), (s_len, range) = (156, 24),
    (284, 48), (540, 97), (2710, 391): nfft 512, 1024, 2048, 8192.  A call returns after its last chunk's records
    are on the host (events around synchronous calls).  Beside each shape what a user could do without the
    object: windows gathered with torch (unfold), fft_execute_batch_dev forward, torch for the shifted
    products, fft_execute_batch_dev backward, torch for abs and max, in pieces of 2^25 values
    ("plan API + torch"); and at the sizes with a fused kernel the library's own composed path
    (liquid_mi355x_qdetector_set_route) beside it.  Flops: (1 + offsets) transforms of 5 nfft log2 nfft and
    9 nfft per offset for the product and the magnitude, per window, against the 157.3 TFLOP/s float32 vector
    peak.  Every side is timed three times in turn (1 warm-up call, 3 timed); "ms" is the median."""
    import numpy as np
    n = 1 << 24
    peak = 157.3e12
    x = cbuf(n)
    xc = torch.view_as_complex(x.view(-1, 2))
    rng = np.random.default_rng(5)
    for s_len, r in ((156, 24), (284, 48), (540, 97), (2710, 391)):
        s = ((rng.integers(0, 2, s_len) * 2.0 - 1.0) + 1j * (rng.integers(0, 2, s_len) * 2.0 - 1.0)).astype(np.complex64)
        q = LQ.QDetector(s)
        nfft = q.nfft
        q.set_range((r + 0.5) * 2 * np.pi / nfft)
        assert q.range == r
        q.set_stream(S)
        route = LQ.qdetector_route(nfft)
        noff, h = 2 * r + 1, nfft // 2
        nwin = (n - nfft) // h + 1
        Sf = torch.fft.fft(torch.cat([torch.from_numpy(s).cuda(), torch.zeros(nfft - s_len, dtype=torch.complex64, device="cuda")]))
        idx = (torch.arange(nfft, device="cuda")[None, :] - torch.arange(-r, r + 1, device="cuda")[:, None]) % nfft
        Sc = torch.conj(Sf)[idx]                              # noff x nfft
        piece = max(1, (1 << 25) // (noff * nfft))
        fwd, bwd = L.fft_create_plan(nfft, None, None, +1, 0), L.fft_create_plan(nfft, None, None, -1, 0)
        L.fft_set_stream(fwd, S)
        L.fft_set_stream(bwd, S)
        W = torch.empty(piece, nfft, dtype=torch.complex64, device="cuda")
        X = torch.empty_like(W)
        P = torch.empty(piece, noff, nfft, dtype=torch.complex64, device="cuda")
        R = torch.empty_like(P)
        cnt = [0]

        def call(composed):
            LQ.set_qdetector_route("composed" if composed else None)
            try:
                cnt[0] = q.execute_block_dev(x.data_ptr(), n, max_det=4)["count"]
            finally:
                LQ.set_qdetector_route(None)

        def by_plan_api():
            with torch.cuda.stream(STREAM):
                win = xc.unfold(0, nfft, h)
                best = []
                for w0 in range(0, win.shape[0], piece):
                    k = min(piece, win.shape[0] - w0)
                    W[:k].copy_(win[w0:w0 + k])
                    L.fft_execute_batch_dev(fwd, W.data_ptr(), X.data_ptr(), k)
                    torch.mul(X[:k, None, :], Sc[None], out=P[:k])
                    L.fft_execute_batch_dev(bwd, P.data_ptr(), R.data_ptr(), k * noff)
                    best.append(torch.max(R[:k].abs().reshape(k, -1), dim=1))
                return best
        sides = [("call", lambda: call(False)), ("plan API + torch", by_plan_api)]
        if route != "composed":
            sides.insert(1, ("call, composed path", lambda: call(True)))
        runs = {k: [] for k, _ in sides}
        for _ in range(3):
            for k, f in sides:
                runs[k].append(timed(f, it=3, w=1, floor_ms=0.0))
        med = {k: sorted(v)[1] for k, v in runs.items()}
        flops = nwin * ((1 + noff) * 5.0 * nfft * np.log2(nfft) + noff * 9.0 * nfft)
        for k, _ in sides:
            row = {"workload": "qdetector_cccf s_len=%d range=%d nfft=%d (%s), %s" % (s_len, r, nfft, route, k),
                   "ms": round(med[k], 3), "runs_ms": [round(v, 3) for v in runs[k]]}
            if k != "plan API + torch":
                row["frac_of_fp32_vector_peak"] = round(flops / (med[k] * 1e-3) / peak, 4)
                row["over_plan_api"] = round(med[k] / med["plan API + torch"], 4)
                row["detections"] = cnt[0]
            print(json.dumps(row))
        sys.stdout.flush()
        q.destroy()
        L.fft_destroy_plan(fwd)
        L.fft_destroy_plan(bwd)
        del Sc, idx, W, X, P, R


def main():
    L = LQ.lib()
    if "--qdetector" in sys.argv[1:]:
        qdetector_rows(L)
        return
    if "--detector" in sys.argv[1:]:
        detector_rows(L)
        return
    if "--autocorr" in sys.argv[1:]:
        autocorr_rows(L)
        return
    if "--iir" in sys.argv[1:]:
        iir_rows(L)
        return
    if "--halfband" in sys.argv[1:]:   # only the half-band rows (resamp2, firhilbf, msresamp)
        halfband_rows(L)
        return
    # firfilt rrrf / cccf, h = 64
    n = 1 << 27
    for t, esz in (("rrrf", 4), ("cccf", 8)):
        x = rbuf(n) if t == "rrrf" else cbuf(n)
        y = torch.empty_like(x)
        h = torch.rand(64 * (2 if t == "cccf" else 1)).numpy() - 0.5
        h = h.view("complex64") if t == "cccf" else h.astype("float32")
        q = LQ.FirFilt(t, h)
        q.set_stream(S)
        fn = getattr(L, "firfilt_%s_execute_block_dev" % t)
        ms = timed(lambda: fn(q.q, x.data_ptr(), n, y.data_ptr()))
        report("firfilt_%s h=64" % t, ms, n, "samples", 2 * esz * n, "%d B/sample" % (2 * esz))
        q.destroy()
    # firfilt crcf at other lengths (h <= 32 and h > 64: the VALU kernel)
    n = 1 << 27
    x = cbuf(n)
    y = torch.empty_like(x)
    for hl in (16, 32, 48, 128, 256):
        h = (torch.rand(hl) - 0.5).numpy().astype("float32")
        q = LQ.FirFilt("crcf", h)
        q.set_stream(S)
        ms = timed(lambda: L.firfilt_crcf_execute_block_dev(q.q, x.data_ptr(), n, y.data_ptr()))
        report("firfilt_crcf h=%d" % hl, ms, n, "samples", 16 * n, "16 B/sample")
        q.destroy()
    del x, y
    # firdecim / firinterp crcf M = 8, m = 8 (Kaiser, 2Mm taps)
    n = 1 << 27
    x = cbuf(n)
    y = torch.empty(2 * n, device="cuda")
    d = LQ.FirDecim(8, m=8, As=60.0)
    d.set_stream(S)
    ms = timed(lambda: L.firdecim_crcf_execute_block_dev(d.q, x.data_ptr(), n // 8, y.data_ptr()))
    report("firdecim_crcf M=8 m=8", ms, n, "input samples", 8 * n + n, "8 B/input + 8 B/output")
    xi = cbuf(n // 8)
    it = LQ.FirInterp(8, m=8, As=60.0)
    it.set_stream(S)
    ms = timed(lambda: L.firinterp_crcf_execute_block_dev(it.q, xi.data_ptr(), n // 8, y.data_ptr()))
    report("firinterp_crcf M=8 m=8", ms, n, "output samples", 8 * n + n, "8 B/output + 8 B/input")
    # firpfbch2 analyzer at other channel counts (M = 1024 is the bench's
    # fused fast path; the others take the generic polyphase + transform kernels)
    n = 1 << 27
    x = cbuf(n)
    y = torch.empty(4 * n, device="cuda")
    for M in (64, 128, 256, 512, 1024, 2048, 4096):
        a2 = LQ.FirPfbch2(LQ.LIQUID_ANALYZER, M, 4, 60.0)
        a2.set_stream(S)
        nb = n // (M // 2)
        ms = timed(lambda: L.firpfbch2_crcf_execute_block_dev(a2.q, x.data_ptr(), nb, y.data_ptr()))
        report("firpfbch2_crcf analyzer M=%d m=4" % M, ms, n, "input samples", 24 * n,
               "8 B/input + 16 B/output (2 per input)")
        a2.destroy()
    del x, y
    # firpfbch2 synthesizer, firpfbch analyzer / synthesizer, M = 1024
    M, nb = 1024, 1 << 17
    X = cbuf(nb * M)
    Y = torch.empty(2 * nb * M, device="cuda")
    q2 = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, M, 4, 60.0)
    q2.set_stream(S)
    ms = timed(lambda: L.firpfbch2_crcf_execute_block_dev(q2.q, X.data_ptr(), nb, Y.data_ptr()))
    report("firpfbch2_crcf synthesizer M=1024 m=4", ms, nb * M // 2, "output samples", 12 * nb * M,
           "8 B/channel sample in + 8 B/output (M/2 per block)")
    for typ, nm in ((LQ.LIQUID_ANALYZER, "analyzer"), (LQ.LIQUID_SYNTHESIZER, "synthesizer")):
        for Mc in (64, 256, 1024, 4096):
            nbc = nb * M // Mc
            p = LQ.FirPfbch(typ, Mc, m=4, As=60.0)
            p.set_stream(S)
            ms = timed(lambda: L.firpfbch_crcf_execute_block_dev(p.q, X.data_ptr(), nbc, Y.data_ptr()))
            report("firpfbch_crcf %s M=%d m=4" % (nm, Mc), ms, nbc * Mc, "samples", 16 * nbc * Mc, "16 B/sample")
            p.destroy()
    for Mc in (256, 4096):
        nbc = nb * M // Mc
        q2 = LQ.FirPfbch2(LQ.LIQUID_SYNTHESIZER, Mc, 4, 60.0)
        q2.set_stream(S)
        ms = timed(lambda: L.firpfbch2_crcf_execute_block_dev(q2.q, X.data_ptr(), nbc, Y.data_ptr()))
        report("firpfbch2_crcf synthesizer M=%d m=4" % Mc, ms, nbc * Mc // 2, "output samples", 12 * nbc * Mc,
               "8 B/channel sample in + 8 B/output (M/2 per block)")
        q2.destroy()
    # resamp timing plans (host/resamp.c): wall clock per call including the
    # host's plan work -- a periodic rate (plan built once, then cached), a
    # rate whose float32 timing has no period <= 2^25 inputs (a direct plan of
    # the call's inputs built serially on the host per call), and a
    # symsync-style loop that steers the rate before every 4096-input call
    import time
    n = 1 << 24
    x = cbuf(n)
    y = torch.empty(2 * 2 * n, device="cuda")
    # (float32 timing periods at npfb = 64: r = 1.037 1 011 163 inputs,
    # r = 0.9999999 8 388 609; every rate tried has a period below 2^24)
    for name, rate in (("r=1.037", 1.037), ("r=0.9999999", 0.9999999)):
        rs = LQ.Resamp(rate, 7, 0.4, 60.0, 64)
        rs.set_stream(S)
        t0 = time.perf_counter()
        rs.execute_block_dev(x.data_ptr(), n, y.data_ptr())   # first call: period search + plan build
        rs.synchronize()
        print(json.dumps({"workload": "resamp_crcf %s m=7, first 2^24-input call (host period search + plan)" % name,
                          "ms": round((time.perf_counter() - t0) * 1e3, 2)}))
        t0 = time.perf_counter()
        for _ in range(4):
            rs.execute_block_dev(x.data_ptr(), n, y.data_ptr())
        rs.synchronize()
        dt = (time.perf_counter() - t0) / 4
        print(json.dumps({"workload": "resamp_crcf %s m=7, later 2^24-input calls (plan cached), wall clock" % name,
                          "ms": round(dt * 1e3, 3), "value": n / dt / 1e6, "unit": "M input samples/s"}))
        rs.destroy()
    rs = LQ.Resamp(1.037, 7, 0.4, 60.0, 64)
    rs.set_stream(S)
    nc, calls = 4096, 200
    t0 = time.perf_counter()
    for i in range(calls):
        rs.set_rate(1.037 + (1e-6 if i & 1 else -1e-6))   # (adjust_rate clips the rate to 0.5, resamp.c:222-239)
        rs.execute_block_dev(x.data_ptr(), nc, y.data_ptr())
    rs.synchronize()
    dt = (time.perf_counter() - t0) / calls
    print(json.dumps({"workload": "resamp_crcf set_rate before every 4096-input call (direct plan per call)",
                      "ms": round(dt * 1e3, 4), "value": nc / dt / 1e6, "unit": "M input samples/s"}))
    rs.destroy()
    del x, y
    # resamp away from config 5: r = 0.3 (k_resamp4's 1/4 < r <= 1/2 class since
    # r05zj), r = 3.7 and 60 (its r > 2 class since r05ze / r05zi);
    # device-resident calls on a cached periodic plan, kernel time from HIP events
    for rate, nin in ((0.3, 1 << 24), (3.7, 1 << 22), (60.0, 1 << 18)):
        rs = LQ.Resamp(rate, 7, 0.4, 60.0, 64)
        rs.set_stream(S)
        x = cbuf(nin)
        nout = rs.num_output(nin)
        y = torch.empty(2 * (nout + 64), device="cuda")
        ms = timed(lambda: rs.execute_block_dev(x.data_ptr(), nin, y.data_ptr()))
        kern = "k_resamp4" if rate > 0.25 else "k_resamp3"
        report("resamp_crcf r=%g m=7 (%s)" % (rate, kern), ms, nout,
               "output samples", 8 * nin + 8 * nout, "8 B/input + 8 B/output")
        rs.destroy()
    del x, y
    halfband_rows(L)
    iir_rows(L)
    autocorr_rows(L)
    # FFT API batches
    for N in (256, 512, 1024, 2048, 4096, 8192, 16384, 65536, 12345):
        B = (1 << 26) // N
        Z = cbuf(B * N)
        pl = L.fft_create_plan(N, None, None, 1, 0)
        L.fft_set_stream(pl, S)
        ms = timed(lambda: L.fft_execute_batch_dev(pl, Z.data_ptr(), Z.data_ptr(), B))
        report("fft n=%d batch %d" % (N, B), ms, B * N, "points", 16 * B * N, "16 B/point (one pass)")
        L.fft_destroy_plan(pl)
    # spgram estimate, nfft = 1024 (window 512, transforms every 256 samples)
    n = 1 << 26
    x = cbuf(n)
    psd = torch.empty(1024, device="cuda")
    sg = LQ.Spgram(1024, default=True)
    L.spgramcf_set_stream(sg.q, S)
    ms = timed(lambda: L.spgramcf_estimate_psd_dev(sg.q, x.data_ptr(), n, psd.data_ptr()), it=5, w=2)
    report("spgramcf estimate_psd nfft=1024", ms, n, "input samples", 8 * n, "8 B/input (transform batch "
           "staged through HBM: +32 B/input)")


if __name__ == "__main__":
    main()
