"""Times STOI / ESTOI on the GPU (ainp_stoi) at the two shapes it was built
for -- the scoring loop of models/AudioReg/train.m:183-213 over 9 clips of 5 s
at 16 kHz:

  curve   9 clean rows, 900 restored (9 clips x 5 rows x 20 iterations)
  final   9 clean rows, 9 restored (one result per clip)

one call     what ainp.stoi.stoi does once the rows are on the device: one
             ops.resample_poly launch to 10 kHz (float64) and one ops.stoi call
             (four launches: keep, bands, score, finish), tables uploaded and
             workspace allocated inside the timed window.
kernels      torch.ops.ainp.stoi alone on the 10 kHz rows, buffers preallocated.
composed     the same steps from existing operators on the device, float64,
             clean row by clean row because the kept frames differ: unfold,
             norm / log10 / nonzero for the silent frames, two shifted adds for
             the overlap-add, unfold, torch.fft.rfft, a [15, 257] band matrix
             product, unfold into segments and the normalisations as tensor
             expressions.  It starts from the same 10 kHz rows as `kernels`.
oracle       the float64 numpy loop of tests/stoi_ref.py on the host over
             `--oracle-pairs` pairs; for more restored rows than that the
             figure given is per pair times the rows, marked as extrapolated.

Method: each device path is warmed up, then timed with device events around
`--iters` back-to-back calls, `--reps` times; the median is reported with the
min-max spread.  The largest difference between the paths' scores is printed.
For the bands launch the least time the hardware could take is printed from
the shapes (bytes over the measured HBM copy rate, float64 operations over the
vector peak); its kernel time comes from a kernel trace taken in a run of its
own (--trace-only runs the kernels path a few times and nothing else).
Prints one table and one JSON line per case.

Usage: python tools/stoi_bench.py [--iters 5] [--reps 5] [--only curve] [--extended]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-audio-inpainting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ainp import ops  # noqa: E402
from ainp import stoi as st  # noqa: E402

SR, SECONDS, CLIPS = 16000, 5.0, 9
CASES = [("curve", 100), ("final", 1)]      # restored rows per clip
HBM_BYTES_PER_S = 6.29e12     # measured float4 copy rate of an MI355X
FP64_FLOPS = 78.6e12          # vector float64 peak (data sheet)


def timed(call, iters, reps):
    call()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            call()
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / iters)
    return statistics.median(runs), min(runs), max(runs)


def signals(k, dev):
    """9 clean clips and k restored per clip at 16 kHz: harmonic stacks under a
    slow envelope with a pause, restored = clean + noise growing with the row."""
    gen = torch.Generator(device=dev).manual_seed(0)
    S = int(SR * SECONDS)
    t = torch.arange(S, device=dev, dtype=torch.float64) / SR
    clean = torch.zeros(CLIPS, S, device=dev, dtype=torch.float64)
    for c in range(CLIPS):
        f0 = 110.0 + 9.0 * c
        for h in range(1, 20):
            clean[c] += torch.sin(2 * np.pi * h * f0 * t + 0.7 * h * (c + 1)) / h ** 0.7
        clean[c] *= 0.1 * (0.55 + 0.45 * torch.sin(2 * np.pi * (2.0 + 0.3 * c) * t))
        clean[c, int((1.0 + 0.2 * c) * SR):int((1.4 + 0.2 * c) * SR)] *= 1e-4     # a pause
    clean += 1e-3 * torch.randn(CLIPS, S, device=dev, generator=gen, dtype=torch.float64)
    noise = torch.randn(CLIPS * k, S, device=dev, generator=gen, dtype=torch.float64)
    level = 0.002 * (1 + torch.arange(CLIPS * k, device=dev, dtype=torch.float64) % k)
    restored = clean.repeat_interleave(k, 0) + level[:, None] * noise
    return clean, restored


def composed(x, y, k, extended):
    """x [C, L], y [C k, L] at 10 kHz (row r of y belongs to clean row r // k) ->
    scores [C k], from torch operators alone."""
    dev = x.device
    i = torch.arange(st.NF, device=dev, dtype=torch.float64)
    w = 0.5 * (1.0 - torch.cos(2.0 * np.pi * (i + 1) / (st.NF + 1)))
    B = torch.zeros(st.J, st.NFFT // 2 + 1, device=dev, dtype=torch.float64)
    for j in range(st.J):
        B[j, st.BAND[j]:st.BAND[j + 1]] = 1.0
    e = 20.0 * torch.log10((x.unfold(-1, st.NF, st.HOP) * w).norm(dim=-1) + st.EPS)
    keep = e > e.max(dim=1, keepdim=True).values - st.DYN
    clip = 1.0 + 10.0 ** (-st.BETA / 20.0)
    out = []
    for c in range(x.shape[0]):
        idx = keep[c].nonzero().squeeze(1)
        T = idx.numel()
        if T < st.N:
            out.append(torch.full((k,), st.SENTINEL, device=dev, dtype=torch.float64))
            continue
        rows = torch.cat((x[c:c + 1], y[c * k:(c + 1) * k]))
        fr = rows.unfold(-1, st.NF, st.HOP)[:, idx] * w                 # [1 + k, T, 256]
        s = torch.zeros(1 + k, (T + 1) * st.HOP, device=dev, dtype=torch.float64)
        s[:, :T * st.HOP] += fr[:, :, :st.HOP].reshape(1 + k, -1)
        s[:, st.HOP:] += fr[:, :, st.HOP:].reshape(1 + k, -1)
        spec = torch.fft.rfft(s.unfold(-1, st.NF, st.HOP) * w, n=st.NFFT)
        env = torch.sqrt((spec.real ** 2 + spec.imag ** 2) @ B.T).transpose(1, 2)   # [1 + k, J, T]
        seg = env.unfold(-1, st.N, 1)                                    # [1 + k, J, M, N]
        X, Y = seg[:1], seg[1:]

        def rows_n(a):
            a = a - a.mean(dim=-1, keepdim=True)
            return a / (a.norm(dim=-1, keepdim=True) + st.EPS)

        def cols_n(a):
            a = a - a.mean(dim=1, keepdim=True)
            return a / (a.norm(dim=1, keepdim=True) + st.EPS)

        if extended:
            d = (cols_n(rows_n(X)) * cols_n(rows_n(Y))).sum(dim=(1, 3)) / st.N
        else:
            alpha = X.norm(dim=-1, keepdim=True) / (Y.norm(dim=-1, keepdim=True) + st.EPS)
            d = (rows_n(X) * rows_n(torch.minimum(alpha * Y, clip * X))).sum(dim=(1, 3)) / st.J
        out.append(d.mean(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="substring of the case name")
    ap.add_argument("--extended", action="store_true", help="ESTOI instead of STOI")
    ap.add_argument("--oracle-pairs", type=int, default=9)
    ap.add_argument("--trace-only", action="store_true",
                    help="run the kernels path a few times and exit (for a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stoi_bench needs a GPU: timings taken anywhere else say nothing")
    import stoi_ref
    dev = torch.device("cuda")
    for name, k in CASES:
        if a.only and a.only not in name:
            continue
        clean, restored = signals(k, dev)
        C, R, S = CLIPS, CLIPS * k, clean.shape[1]
        rows16 = torch.cat((clean, restored))
        clean_row = [c for c in range(C) for _ in range(k)]
        n16 = [S] * C
        res = {}

        def one_call():
            res["one"] = st._score(rows16, n16, clean_row, C, SR, a.extended)[0]

        rows10 = ops.resample_poly(rows16, 5, 8)
        L = rows10.shape[1]
        x10, y10 = rows10[:C], rows10[C:]
        plan = st.plan(C, R, L)
        n32 = torch.full((C,), L, dtype=torch.int32)
        row32 = torch.tensor(clean_row, dtype=torch.int32)
        tables = torch.cat((n32, row32)).to(dev)
        ws = torch.empty(plan.bytes // 8 + 1, device=dev, dtype=torch.float64)
        score = torch.empty(R, device=dev, dtype=torch.float64)
        frames = torch.zeros(C, device=dev, dtype=torch.int32)

        def kernels():
            torch.ops.ainp.stoi(x10, y10, n32, row32, tables, a.extended, ws, score, frames)

        if a.trace_only:
            for _ in range(5):
                kernels()
            torch.cuda.synchronize()
            continue

        def comp():
            res["comp"] = composed(x10, y10, k, a.extended)

        one = timed(one_call, a.iters, a.reps)
        ker = timed(kernels, a.iters, a.reps)
        cmp_ = timed(comp, max(1, a.iters // 2), a.reps)
        diff_paths = float((res["one"] - score).abs().max())
        diff_comp = float((res["comp"] - score).abs().max())

        xh, yh, sh = x10.cpu().numpy(), y10.cpu().numpy(), score.cpu().numpy()
        pairs = [r * (R // min(R, a.oracle_pairs)) for r in range(min(R, a.oracle_pairs))]
        t0 = time.perf_counter()
        want = [stoi_ref.score(xh[clean_row[r]], yh[r], a.extended)[0] for r in pairs]
        per_pair = (time.perf_counter() - t0) / len(pairs)
        diff_oracle = max(abs(w - sh[r]) for w, r in zip(want, pairs))
        oracle_ms = 1e3 * per_pair * R

        T = frames.cpu().numpy()
        kept = int(T.sum() + sum(int(T[c]) for c in clean_row))
        bands_bytes = 8 * (C + R) * L + 8 * st.J * kept
        bands_flops = kept * (5 * 256 * 8 + 10 * 256 + 6 * 256 + 2 * 257)
        least_bytes_us = 1e6 * bands_bytes / HBM_BYTES_PER_S
        least_flops_us = 1e6 * bands_flops / FP64_FLOPS
        what = "ESTOI" if a.extended else "STOI"
        print(f"{name:6s} {what}: {C} clean x {R} restored rows of {SECONDS:g} s at {SR} Hz "
              f"({L} samples at 10 kHz, kept frames per clean row {T.tolist()})\n"
              f"  one call   {one[0]:9.3f} ms [{one[1]:9.3f} .. {one[2]:9.3f}]\n"
              f"  kernels    {ker[0]:9.3f} ms [{ker[1]:9.3f} .. {ker[2]:9.3f}]\n"
              f"  composed   {cmp_[0]:9.3f} ms [{cmp_[1]:9.3f} .. {cmp_[2]:9.3f}]"
              f"  composed / kernels: {cmp_[0] / ker[0]:.2f}\n"
              f"  oracle     {oracle_ms:9.1f} ms on the host ({1e3 * per_pair:.1f} ms a pair over "
              f"{len(pairs)} pairs{', extrapolated' if len(pairs) < R else ''})\n"
              f"  largest score difference: one call vs kernels {diff_paths:.1e}, composed vs "
              f"kernels {diff_comp:.1e}, oracle vs kernels {diff_oracle:.1e}\n"
              f"  bands launch: {bands_bytes / 1e6:.1f} MB, {bands_flops / 1e9:.2f} GFLOP float64; "
              f"least time {least_bytes_us:.1f} us by bytes, {least_flops_us:.1f} us by operations",
              flush=True)
        print(json.dumps(dict(
            case=name, measure=what, clean=C, restored=R, samples_10k=L, kept=T.tolist(),
            iters=a.iters, reps=a.reps, one_call_ms=round(one[0], 4),
            one_call_ms_min=round(one[1], 4), one_call_ms_max=round(one[2], 4),
            kernels_ms=round(ker[0], 4), kernels_ms_min=round(ker[1], 4),
            kernels_ms_max=round(ker[2], 4), composed_ms=round(cmp_[0], 4),
            composed_ms_min=round(cmp_[1], 4), composed_ms_max=round(cmp_[2], 4),
            oracle_ms=round(oracle_ms, 1), oracle_pairs=len(pairs),
            oracle_extrapolated=len(pairs) < R, diff_one_vs_kernels=diff_paths,
            diff_composed_vs_kernels=diff_comp, diff_oracle_vs_kernels=diff_oracle,
            bands_bytes=bands_bytes, bands_flops=bands_flops,
            bands_least_us_bytes=round(least_bytes_us, 2),
            bands_least_us_flops=round(least_flops_us, 2))), flush=True)
        del clean, restored, rows16, rows10, ws


if __name__ == "__main__":
    main()
