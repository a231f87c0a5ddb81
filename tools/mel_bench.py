"""Times the mel kernels (ainp_mel_fwd, ainp_mel_inverse) against their torch
compositions on the same device:

  forward   torch.matmul(basis, X.abs() ** p, out=O)              vs torch.ops.ainp.mel_fwd
  inverse   torch.matmul(P, M, out=O).clamp_min_(0).sqrt_()       vs torch.ops.ainp.mel_inverse

at the reference's default shape (n_fft 2048, hop 512, 128 mels, 32 clips of
5 s at 16 kHz: X [32, 1025, 157]) and at the small shapes of
tests/test_gpu_mel.py.  Both kernels are bandwidth-bound, so each time is also
given as bytes/s over the kernel's traffic floor

  forward   sizeof(complex) F T + sizeof(real) n_mels T     per signal
  inverse   4 (n_mels T + F T) per signal + 4 F n_mels

and as a share of the MI355X's 8 TB/s HBM peak.  Method: every variant is
warmed up, then timed with device events around `--iters` back-to-back calls,
`--reps` times, the two variants alternating; the median is reported with the
min-max spread.  Calls rotate through enough input / output sets that the
timed window's footprint exceeds the 256 MiB Infinity Cache (the default shape
alone would sit in it), so the rate is an HBM rate; torch's intermediate
|X|^p comes from its caching allocator.  --graph replays the same
calls from a captured HIP graph instead, which takes the host's launch cost
out of the small shapes.  Prints one table row and one JSON line per case.

Usage: python tools/mel_bench.py [--iters 200] [--reps 9] [--graph] [--power 2.0]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "ml-audio-inpainting_amd"))
from ainp import mel, ops  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s (MI355X HBM3E)
L3_BYTES = 256 << 20
SR = 16000
# (name, n_fft, n_mels, batch, T, fmin, fmax)
CASES = [
    ("default 32x5s", 2048, 128, 32, 157, 0.0, None),
    ("2048/128 1s", 2048, 128, 1, 32, 0.0, None),
    ("128/20 T65", 128, 20, 1, 65, 300.0, 3400.0),
    ("64/8 B3 T70", 64, 8, 3, 70, 0.0, None),
    ("64/40 T1", 64, 40, 1, 1, 0.0, None),
]


def time_pair(fns, n_sets, iters, reps, graph):
    """Median / min / max microseconds per call of each fn(i) (i = set index),
    the fns alternating rep by rep."""
    runs = {k: [] for k in fns}
    launch = {}
    for k, fn in fns.items():
        def body(fn=fn):
            for i in range(iters):
                fn(i % n_sets)
        for i in range(max(n_sets, 3)):          # warm-up: every set, every shape
            fn(i % n_sets)
        torch.cuda.synchronize()
        if graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            g.replay()
            torch.cuda.synchronize()
            launch[k] = g.replay
        else:
            launch[k] = body
    for _ in range(reps):
        for k in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch[k]()
            e1.record()
            torch.cuda.synchronize()
            runs[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in runs.items()}


def report(kind, name, floor, res, extra):
    for k, (med, lo, hi) in res.items():
        rate = floor / (med * 1e-6)
        print(f"{kind:8s} {name:14s} {k:6s} {med:9.2f} us [{lo:8.2f} .. {hi:8.2f}]  "
              f"{rate / 1e9:9.1f} GB/s over the floor ({100 * rate / HBM_PEAK:5.1f} % of HBM peak)",
              flush=True)
    out = dict(kind=kind, case=name, floor_bytes=floor, **extra)
    for k, (med, lo, hi) in res.items():
        out[f"{k}_us"] = round(med, 3)
        out[f"{k}_us_min"] = round(lo, 3)
        out[f"{k}_us_max"] = round(hi, 3)
        out[f"{k}_GBps"] = round(floor / (med * 1e-6) / 1e9, 1)
        out[f"{k}_hbm_frac"] = round(floor / (med * 1e-6) / HBM_PEAK, 4)
    out["speedup_vs_torch"] = round(res["torch"][0] / res["ainp"][0], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--power", type=float, default=2.0)
    ap.add_argument("--only", default=None, help="substring of the case name")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mel_bench needs a GPU: timings taken anywhere else say nothing")
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    warnings.simplefilter("ignore")            # the empty-band warning of the 64/40 case
    for name, n_fft, n_mels, B, T, fmin, fmax in CASES:
        if a.only and a.only not in name:
            continue
        F = n_fft // 2 + 1
        cfg = (SR, n_fft, n_mels, fmin, fmax)
        bands = mel.device_bands(*cfg, dev)
        basis = torch.from_numpy(mel.mel_filterbank(*cfg).copy()).to(dev)
        P = mel.device_pinv(*cfg, dev)
        shape = dict(n_fft=n_fft, n_mels=n_mels, batch=B, T=T, graph=a.graph, iters=a.iters)

        # ---- forward
        floor = B * (8 * F * T + 4 * n_mels * T)
        n_sets = max(1, min(64, -(-2 * L3_BYTES // floor)))
        X = [torch.view_as_complex(torch.randn(B, F, T, 2, device=dev, generator=gen))
             for _ in range(n_sets)]
        O = [torch.empty(B, n_mels, T, device=dev) for _ in range(n_sets)]
        Ot = [torch.empty(B, n_mels, T, device=dev) for _ in range(n_sets)]

        def fwd_ainp(i):
            torch.ops.ainp.mel_fwd(X[i], bands.lo, bands.off, bands.weights, a.power, O[i])

        def fwd_torch(i):
            torch.matmul(basis, X[i].abs() ** a.power, out=Ot[i])

        fwd_ainp(0)
        fwd_torch(0)
        err = ((O[0] - Ot[0]).abs().max() / Ot[0].abs().max()).item()
        res = time_pair({"ainp": fwd_ainp, "torch": fwd_torch}, n_sets, a.iters, a.reps, a.graph)
        report("mel_fwd", name, floor, res, dict(shape, power=a.power, sets=n_sets,
                                                 max_diff_vs_torch=err))
        del X, O, Ot

        # ---- inverse (sqrt of the clamped product, the default path)
        floor = B * 4 * (n_mels * T + F * T) + 4 * F * n_mels
        n_sets = max(1, min(64, -(-2 * L3_BYTES // floor)))
        M = [torch.rand(B, n_mels, T, device=dev, generator=gen) for _ in range(n_sets)]
        flags = ops.MEL_SQRT | ops.MEL_CLAMP
        O = [torch.empty(B, F, T, device=dev) for _ in range(n_sets)]
        Ot = [torch.empty(B, F, T, device=dev) for _ in range(n_sets)]

        def inv_ainp(i):
            torch.ops.ainp.mel_inverse(P, M[i], flags, O[i])

        def inv_torch(i):          # in place: the composition's cheapest form
            torch.matmul(P, M[i], out=Ot[i]).clamp_min_(0).sqrt_()

        inv_ainp(0)
        inv_torch(0)
        err = ((O[0] - Ot[0]).abs().max() / Ot[0].abs().max()).item()
        res = time_pair({"ainp": inv_ainp, "torch": inv_torch}, n_sets, a.iters, a.reps, a.graph)
        report("mel_inv", name, floor, res, dict(shape, sets=n_sets, max_diff_vs_torch=err))
        del M, O, Ot


if __name__ == "__main__":
    main()
