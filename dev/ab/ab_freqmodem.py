"""freqmod / freqdem block calls, the numbers DESIGN.md records (dev tool, needs the GPU):
  1. 2^24 samples in device memory: freqmod, freqdem with M = 1 and M = 1024, each
     against a device copy that moves the same 12 bytes per sample;
  2. the same work as a torch composition: cumsum of rounded products and a table
     gather (torch.round rounds halves to even: a timing, not the same function),
     and angle(x[M:] * conj(x[:-M]));
  3. freqmod's traffic: the sums launch reads m once more, 16 bytes per sample
     requested against the 12 the function needs.
Device times are device events over 30 calls after warm-up (tools/bench_widened.timed).
--profile: 40 freqmod calls and nothing else, for a kernel trace that gives the
stage split (rocprofv3 --kernel-trace --stats -- python dev/ab/ab_freqmodem.py --profile)."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import bench_widened as W  # noqa: E402

LQ = W.LQ
n = 1 << 24
kf = 0.04
m = W.rbuf(n)
x = W.cbuf(n)
s = torch.empty(2 * n, device="cuda")
y = torch.empty(n, device="cuda")

mod = LQ.FreqMod(kf)
mod.set_stream(W.S)
run_mod = lambda: mod.modulate_block_dev(m.data_ptr(), n, s.data_ptr())   # noqa: E731

if "--profile" in sys.argv:
    with torch.cuda.stream(W.STREAM):
        for _ in range(40):
            run_mod()
    torch.cuda.synchronize()
    sys.exit(0)

a, b = torch.empty(6 * n // 4, device="cuda"), torch.empty(6 * n // 4, device="cuda")
torch.cuda.synchronize()
with torch.cuda.stream(W.STREAM):
    copy_ms = W.timed(lambda: b.copy_(a))
    print("device copy, %d MB read + %d MB written: %.4f ms, %.0f GB/s" % (6 * n >> 20, 6 * n >> 20, copy_ms,
                                                                          12 * n / copy_ms / 1e6))
    ms = W.timed(run_mod)
    print("freqmod: %.4f ms, %.0f GB/s of the 12 bytes per sample it needs (%.0f GB/s of the 16 it requests), "
          "%.2f x the copy" % (ms, 12 * n / ms / 1e6, 16 * n / ms / 1e6, ms / copy_ms))
    for M in (1, 1024):
        dem = LQ.FreqDem(kf, M)
        dem.set_stream(W.S)
        ms = W.timed(lambda: dem.demodulate_block_dev(x.data_ptr(), n, y.data_ptr()))
        print("freqdem M = %4d: %.4f ms, %.0f GB/s, %.2f x the copy" % (M, ms, 12 * n / ms / 1e6, ms / copy_ms))
        dem.set_stream(None)

    table = torch.view_as_complex(torch.randn(1024, 2, device="cuda"))
    ref = kf * 65536.0

    def torch_mod():
        ph = torch.cumsum(torch.round(m * ref).to(torch.int32), 0, dtype=torch.int32)
        return table[((ph + 32) >> 6) & 1023]
    ms = W.timed(torch_mod)
    print("torch cumsum + gather: %.4f ms" % ms)
    xc = torch.view_as_complex(x.view(n, 2))
    dref = 1.0 / (2 * math.pi * kf)
    for M in (1, 1024):
        ms = W.timed(lambda: torch.angle(xc[M:] * torch.conj(xc[:-M])) * dref)
        print("torch angle(x[M:] conj(x[:-M])), M = %4d: %.4f ms" % (M, ms))
mod.set_stream(None)
