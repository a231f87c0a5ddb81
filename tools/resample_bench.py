"""Times the polyphase resampler (ainp_resample_poly) at the two shapes it was
built for, against the host loop it replaces:

  train48   16 kHz -> 48 kHz, float64, 9 clips x 5 s  (models/AudioReg/train.m:72,203)
  irmas     44.1 kHz -> 16 kHz, float32, 64 clips x 7 s  (irmas/IRMAS_gaps.m, load_audio)

For each: the kernel's time per call, its traffic floor (input + output bytes,
each moved once; the coefficient table is not counted) over that time as a
rate and as a share of the MI355X's 8 TB/s HBM peak, and the wall time of
scipy.signal.resample_poly over the same clips one by one on the host (what
utils.load_audio does), with the largest difference between the two results.

Method: the kernel is warmed up, then timed with device events around
`--iters` back-to-back calls of torch.ops.ainp.resample_poly on preallocated
outputs, `--reps` times; the median is reported with the min-max spread.  The
calls rotate through enough input / output sets that the timed window's
footprint exceeds the 256 MiB Infinity Cache, so the rate is an HBM rate.  The
host loop is timed `--host-reps` times with a wall clock; "not measured" when
scipy is not installed.  Prints one table row and one JSON line per case.

Usage: python tools/resample_bench.py [--iters 200] [--reps 9] [--host-reps 3]
"""
import argparse
import json
import os
import statistics
import sys
import time
from math import gcd

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "ml-audio-inpainting_amd"))
from ainp import ops  # noqa: E402,F401  (registers torch.ops.ainp)
from ainp import resample as rs  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s (MI355X HBM3E)
L3_BYTES = 256 << 20
# (name, native rate, target rate, dtype, clips, seconds)
CASES = [
    ("train48", 16000, 48000, "float64", 9, 5.0),
    ("irmas", 44100, 16000, "float32", 64, 7.0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="substring of the case name")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resample_bench needs a GPU: timings taken anywhere else say nothing")
    dev = torch.device("cuda")
    for name, sr, target, dtype, clips, secs in CASES:
        if a.only and a.only not in name:
            continue
        g = gcd(sr, target)
        up, down = target // g, sr // g
        n_in = int(sr * secs)
        n_out = rs.out_len(n_in, up, down)
        tdt = torch.float64 if dtype == "float64" else torch.float32
        esize = np.dtype(dtype).itemsize
        floor = clips * (n_in + n_out) * esize
        n_sets = max(1, min(64, -(-2 * L3_BYTES // floor)))
        rng = np.random.default_rng(0)
        host = rng.standard_normal((clips, n_in)).astype(dtype)
        X = [torch.from_numpy(host).to(dev) for _ in range(n_sets)]
        Y = [torch.empty(clips, n_out, device=dev, dtype=tdt) for _ in range(n_sets)]
        n_dev = torch.full((clips,), n_in, dtype=torch.int32, device=dev)
        p = rs.plan(up, down, dtype)
        table = rs.device_table(up, down, dtype, dev)

        def call(i):
            torch.ops.ainp.resample_poly(X[i], table, n_dev, up, down, Y[i])

        for i in range(max(n_sets, 3)):            # warm-up: every set
            call(i % n_sets)
        torch.cuda.synchronize()
        runs = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.iters):
                call(i % n_sets)
            e1.record()
            torch.cuda.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / a.iters)
        med, lo, hi = statistics.median(runs), min(runs), max(runs)
        rate = floor / (med * 1e-6)

        # the whole public path once, host to host (copies and allocation included)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y_dev = ops.resample_poly(torch.from_numpy(host).to(dev), up, down).cpu().numpy()
        e2e_ms = (time.perf_counter() - t0) * 1e3

        host_ms, diff = None, None
        try:
            from scipy.signal import resample_poly
        except ImportError:
            resample_poly = None
        if resample_poly is not None:
            walls = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                want = [resample_poly(host[r], up, down) for r in range(clips)]
                walls.append((time.perf_counter() - t0) * 1e3)
            host_ms = statistics.median(walls)
            diff = float(max(np.max(np.abs(y_dev[r] - want[r])) for r in range(clips)))

        host_txt = f"{host_ms:9.1f} ms" if host_ms is not None else "not measured"
        print(f"{name:8s} {sr} -> {target} ({up}/{down}) {dtype} {clips} x {secs:g} s  "
              f"{rs.ROUTE_NAMES[p.route]} tile {p.tile} lds {p.lds_bytes}\n"
              f"  kernel {med:9.2f} us [{lo:8.2f} .. {hi:8.2f}]  {rate / 1e9:8.1f} GB/s over "
              f"in + out ({100 * rate / HBM_PEAK:5.1f} % of HBM peak)\n"
              f"  host to host through ops.resample_poly, one call: {e2e_ms:9.1f} ms\n"
              f"  scipy.signal.resample_poly loop on the host: {host_txt}", flush=True)
        print(json.dumps(dict(
            case=name, sr=sr, target=target, up=up, down=down, dtype=dtype, clips=clips,
            n_in=n_in, n_out=n_out, route=rs.ROUTE_NAMES[p.route], tile=p.tile,
            lds_bytes=p.lds_bytes, tpp=p.tpp, floor_bytes=floor, sets=n_sets, iters=a.iters,
            reps=a.reps, kernel_us=round(med, 3), kernel_us_min=round(lo, 3),
            kernel_us_max=round(hi, 3), GBps=round(rate / 1e9, 1),
            hbm_frac=round(rate / HBM_PEAK, 4), e2e_ms=round(e2e_ms, 3),
            scipy_loop_ms=None if host_ms is None else round(host_ms, 3),
            max_abs_diff_vs_scipy=diff)), flush=True)
        del X, Y


if __name__ == "__main__":
    main()
