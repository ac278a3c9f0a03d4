import os as _os, sys as _sys
_r = _os.path.dirname(_os.path.abspath(__file__))
while not _os.path.exists(_os.path.join(_r, "_gfbe_import.py")):
    _r = _os.path.dirname(_r)
_sys.path[:0] = [_r, _os.path.join(_r, "tests")]   # (measurement scripts: the package root and the test helpers they share)
"""Timing of gfbe_line_refine (onlyLineOpt + removeLineOutlier on the device): one window and batches of 256 / 1024 / 4096 windows of
150 eligible lines with 5-11 observations each (NUM_ITERATIONS = 8), and the numpy checker (tests/line_np.py) for scale.
  call   the whole call on its stream, hipEvents around it: packing, copies both ways, the kernel (median of 5)
  kernel the longest time one window spent in the kernel (gfbe_summary.ms_solve, device wall clock)
  host   the call's wall clock on the host (median of 5)"""
import time

import numpy as np
import torch

from _gfbe_import import gf
import line_np as ln

abi, synth_line = gf.abi, gf.synth_line


def main():
    be = gf.Backend(0)
    stream = torch.cuda.Stream(device=0)
    be.set_stream(stream.cuda_stream)
    base = [synth_line.line_window(seed=900 + k, n_ok=150, n_short=0, n_late=0, n_untri=0, n_behind=0, n_long=0, n_outlier=0)
            for k in range(32)]
    holders = [abi.LineWindowHolder(w) for w in base]
    print("lines per window %d, observations per window %.0f (mean)" % (holders[0].n, np.mean([len(h.obs) for h in holders])))
    for nw in (1, 256, 1024, 4096):
        hs = [holders[k % len(holders)] for k in range(nw)]
        be.line_refine(hs)          # warm-up (module load, first allocation)
        calls, hosts, kern = [], [], 0.0
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            out = be.line_refine(hs)
            hosts.append(time.perf_counter() - t0)
            e1.record(stream)
            e1.synchronize()
            calls.append(e0.elapsed_time(e1))
            kern = max(o["perf"]["ms_solve"] for o in out)
        call, host = sorted(calls)[2], sorted(hosts)[2] * 1e3
        print("%5d windows: call %8.3f ms (%7.2f us / window), kernel %7.3f ms, host %8.3f ms, iterations %d" %
              (nw, call, 1e3 * call / nw, kern, host, out[0]["summary"]["iterations"]))
    t0 = time.perf_counter()
    for w in base[:4]:
        ln.refine(w)
    print("numpy checker: %.1f ms / window" % ((time.perf_counter() - t0) / 4 * 1e3))


if __name__ == "__main__":
    main()
