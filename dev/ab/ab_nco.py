"""nco_crcf block mixer, the numbers DESIGN.md records (dev tool, needs the GPU):
  1. 2^24 samples in device memory on a served periodic plan (d_theta = 0.1),
     both types, up and in place, against a device copy of the same 2 n 8 bytes;
  2. the same call on a first-pass direct plan, the host walk and the table
     upload included (a new phase before every call, so no plan is reused),
     host clock around call + synchronize;
  3. the periodic plan of d_theta = 0.3 from phase 0: build time on the host and
     table bytes.
Device times are device events over 30 calls after warm-up (tools/bench_widened.timed)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tools"))
import bench_widened as W  # noqa: E402

LQ = W.LQ
L = LQ.lib()
n = 1 << 24
x = W.cbuf(n)
y = torch.empty_like(x)
nbytes = 2 * n * 8

torch.cuda.synchronize()
with torch.cuda.stream(W.STREAM):
    ms = W.timed(lambda: y.copy_(x))
print("device copy of %d MB read + %d MB written: %.4f ms, %.0f GB/s"
      % (n * 8 >> 20, n * 8 >> 20, ms, nbytes / ms / 1e6))
copy_ms = ms

with torch.cuda.stream(W.STREAM):
    for typ, name in ((LQ.LIQUID_NCO, "nco"), (LQ.LIQUID_VCO, "vco")):
        q = LQ.NCO(typ, plan="periodic")
        q.set_stream(W.S)
        q.set_frequency(0.1)
        for fn, what in ((lambda: q.mix_block_up_dev(x.data_ptr(), y.data_ptr(), n), "up"),
                         (lambda: q.mix_block_down_dev(y.data_ptr(), y.data_ptr(), n), "down in place")):
            ms = W.timed(fn)
            print("%s periodic plan %-13s: %.4f ms, %.0f GB/s, %.2f x the copy" % (name, what, ms, nbytes / ms / 1e6,
                                                                               ms / copy_ms))
        q = LQ.NCO(typ, plan="direct")
        q.set_stream(W.S)
        q.set_frequency(0.1)
        ts = []
        for k in range(12):
            q.set_phase(1e-3 * k)           # off the orbit: the next call walks a new direct plan
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            q.mix_block_up_dev(x.data_ptr(), y.data_ptr(), n)
            t1 = time.perf_counter()
            q.synchronize()
            ts.append(((time.perf_counter() - t0) * 1e3, (t1 - t0) * 1e3))
        ts = sorted(ts[2:])
        print("%s direct plan, first pass: median %.3f ms per call (host walk + upload + launch %.3f ms), min %.3f"
              % (name, ts[len(ts) // 2][0], ts[len(ts) // 2][1], ts[0][0]))

for rep in range(3):
    t0 = time.perf_counter()
    r = LQ.nco_walk(LQ.LIQUID_NCO, 0.0, 0.3, 0, True)
    dt = (time.perf_counter() - t0) * 1e3
    pre, per = r[2], r[3]
    ck = LQ.NCO.CHECKPOINT
    print("periodic plan d_theta = 0.3: pre-period %d, period %d, built in %.1f ms, table %d bytes"
          % (pre, per, dt, 4 * ((pre + per + ck - 1) // ck)))
