"""Times ainp_janssen_ex (csrc/janssen.hip) and, with --algorithm
extrapolation, ainp_ar_extrapolate (csrc/ar_extrapolate.hip) at the reference's
configuration
(models/AudioReg/train.m: w = 4096 samples of context either side of an 80 ms
gap at 16 kHz, h = 1280, 20 iterations) for AR orders p in {256, 512, 1024,
3072} and batches of 1, 9, 64 and 256 segments, next to a float64 CPU run of
the same algorithm (FFT autocorrelation, scipy.linalg.solve_toeplitz for the
AR fit and for the gap -- the fast Toeplitz variant, not the tests' dense
reference; --method arburg: Burg's estimator in numpy whole-vector operations;
--algorithm extrapolation: the fit of either kind per side, scipy.signal's
lfiltic + lfilter for the recursion) on `--threads` worker processes, one single-threaded segment each
(solve_toeplitz holds the GIL, so threads of one process would run in turn).
The workers are started, timed and joined before this process touches the GPU
and import nothing of torch; `cpu x1` is one worker alone, `cpu xT` the wall
time of T concurrent segments / T.

Method: device events around one launch, `--reps` launches after one warm-up,
median with the min-max spread; every launch starts from a fresh copy of the
input batch (copied outside the timed window).  Reported per case: time per
launch, per segment (launch / batch) and per segment-iteration of one
workgroup (launch / maxit: segments run side by side, one per workgroup).

Dependent-chain model.  One iteration is p + h strictly dependent recursion
steps (one barrier each) plus the lag and right-hand-side sums, about
N (p + 1) + p^2 / 2 + h min(2p, N - h) multiply-adds spread over the
workgroup.  --fit times batch 1 over p x h in {640, 1280} and fits
  t_iter = c_step (p + h) + c_mac MACs
by least squares; it prints both constants, each case's share of the chain
and the residuals.  Prints one table row and one JSON line per case.

--burg-steps times one Janssen iteration with the Burg estimator and a 16-sample
gap (so the p Burg steps dominate) at n = 9472 and n = 16384 and prints the
time per Burg step and its slope between successive orders.

--algorithm janssen_hann | janssen_rect | janssen_tukey times the window-wise
rows (ainp.janssen.janssen_windowed's three launches: the gather
ainp_janssen_windows, ainp_janssen_ex over the windows, the overlap-add
ainp_janssen_ola) at w = 4096 and the shift --a (1024) for batches of gaps,
each launch between its own pair of device events, the same median of --reps
after one warm-up, next to the gap-wise launch of the same batch.  The tables
of the gather and the overlap-add are on the device before the timed window;
the Janssen launch goes through ops.janssen as the gap-wise one does.  It
prints how many windows (rows) the batch makes and how many rounds of 256
workgroups (one per CU) that is.  --history also writes every iteration.  No
CPU run.  --any-mask plans the same batch with plan_windows_mask (the fixed grid
of the whole signal, 5 rows a gap, no per-gap support): the same three launches
over the other plan's tables.

Usage: python tools/janssen_bench.py [--reps 5] [--threads 16] [--no-cpu] [--fit]
           [--method lpc|arburg]
           [--algorithm janssen|extrapolation|janssen_hann|janssen_rect|janssen_tukey]
           [--a 1024] [--history] [--any-mask] [--orders 256,512] [--batches 1,256]
           [--burg-steps]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-audio-inpainting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from janssen_ref import harmonic_signal as signal  # noqa: E402  (the parity tests' signal)

# torch and ainp.ops are imported where the GPU is used, so that the CPU
# workers (which re-import this module) stay free of them
W, H, MAXIT = 4096, 1280, 20
ORDERS = (256, 512, 1024, 3072)
BATCHES = (1, 9, 64, 256)


def cpu_fit(x, p, method):
    """[1, a_1 .. a_p]: FFT autocorrelation + Toeplitz solve, or Burg."""
    if method == "arburg":
        from ar_ref import arburg
        return arburg(x, p)
    from scipy.linalg import solve_toeplitz
    nfft = 1 << int(np.ceil(np.log2(2 * len(x) - 1)))
    r = np.fft.irfft(np.abs(np.fft.rfft(x, nfft)) ** 2, nfft)[:p + 1]
    return np.concatenate(([1.0], solve_toeplitz(r[:p], -r[1:p + 1])))


def cpu_janssen(x, s, h, p, maxit, method="lpc"):
    """The same algorithm in float64 numpy / scipy, Toeplitz solves throughout."""
    from scipy.linalg import solve_toeplitz
    from scipy.signal import fftconvolve
    sol = x.copy()
    sol[s:s + h] = 0.0
    obs = sol.copy()
    for _ in range(maxit):
        a = cpu_fit(sol, p, method)
        b = np.correlate(a, a, "full")[p:]
        col = np.zeros(h)
        col[:min(h, p + 1)] = b[:h]
        rhs = fftconvolve(obs, np.concatenate((b[:0:-1], b)), "same")[s:s + h]
        sol[s:s + h] = solve_toeplitz(col, -rhs)
    return sol


def cpu_extrapolate(x, s, h, p, w, method="lpc"):
    """arinpaint.m: per side mean, fit, filtic + filter, then the cross-fade."""
    from scipy.signal import lfilter, lfiltic
    sol = x.copy()
    sides = []
    for c in (x[max(0, s - w):s], x[s + h:min(len(x), s + h + w)][::-1]):
        mean = c.mean()
        y = c - mean
        a = cpu_fit(y, p, method)
        zi = lfiltic([1.0], a, y[::-1][:p])
        sides.append(lfilter([1.0], a, np.zeros(h), zi=zi)[0] + mean)
    wts = np.cos(np.linspace(0.0, np.pi / 2, h)) ** 2
    sol[s:s + h] = wts * sides[0] + (1.0 - wts) * sides[1][::-1]
    return sol


def time_gpu(batch, n, s, h, p, maxit, reps, method="lpc", algorithm="janssen"):
    import torch
    from ainp import ops
    x0 = torch.from_numpy(np.stack([signal(n, 100 + i) for i in range(min(batch, 16))]))
    x0 = x0.repeat((batch + x0.shape[0] - 1) // x0.shape[0], 1)[:batch].cuda().contiguous()
    tabs = ([n] * batch, [s] * batch, [h] * batch)
    ts = []
    for r in range(reps + 1):
        sol = x0.clone()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if algorithm == "janssen":
            iters, _ = ops.janssen(sol, *tabs, p, maxit, method=method)
        else:
            status = ops.ar_extrapolate(sol, *tabs, p, W, method=method)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1))          # ms
    if algorithm == "janssen":
        assert int(iters.min()) == maxit, "a segment stopped early"
    else:
        assert int(status.min()) == 1, "a segment was not filled from both sides"
    return statistics.median(ts), min(ts), max(ts), sol[0].cpu().numpy()


def time_windowed(batch, n, s, h, p, maxit, reps, method, wtype, a, history, any_mask=False):
    """One gap [s, s + h) in each of `batch` signals -> {launch: (median, min,
    max) ms} for the three launches, the number of rows, iterations done."""
    import torch
    from ainp import janssen as jn, ops
    T = torch.ops.ainp
    sigs = [signal(n, 100 + i % 16) for i in range(batch)]
    mask = np.ones(n, bool)
    mask[s:s + h] = False
    for x in sigs:
        x[s:s + h] = 0.0
    plan = (jn.plan_windows_mask if any_mask else jn.plan_windows)([mask] * batch, p, W, a,
                                                                   (wtype,))
    assert np.all(plan.gap_len >= 1)                # one run a row: all through ops.janssen
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    buf0 = up(np.concatenate(sigs))
    tabs = plan.tables()._replace(miss_idx=np.zeros(1, np.int32))
    miss, so, rt, *ola_tabs = (up(t) for t in tabs)
    gana, gsyn = up(plan.gana), up(plan.gsyn)
    rows = len(plan)
    ts = {"gather": [], "janssen": [], "ola": []}
    for r in range(reps + 1):
        buf = buf0.clone()
        sol = torch.empty(rows, W, device="cuda", dtype=torch.float64)
        out = torch.full((batch, maxit, h), float("nan"), device="cuda",
                         dtype=torch.float64) if history else None
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        T.janssen_windows(buf, miss, so, rt, a, gana, sol)
        ev[1].record()
        iters, rhist = ops.janssen(sol, [W] * rows, plan.gap_start, plan.gap_len, p, maxit,
                                   return_history=history, method=method)
        ev[2].record()
        T.janssen_ola(sol, rhist, rt, *ola_tabs, h, a, gana, gsyn, buf, out)
        ev[3].record()
        torch.cuda.synchronize()
        if r:
            for k, name in enumerate(ts):
                ts[name].append(ev[k].elapsed_time(ev[k + 1]))
    assert bool(torch.isfinite(buf).all())
    return ({k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}, rows,
            (int(iters.min()), int(iters.max())))


def windowed_table(args, n):
    import torch
    wtype = args.algorithm[len("janssen_"):]
    print(f"{torch.cuda.get_device_name(0)}; {args.algorithm} {args.method}, w = {W}, "
          f"a = {args.a}, n = {n}, h = {H}, maxit = {MAXIT}, history = {args.history}, "
          f"any mask = {args.any_mask}",
          flush=True)
    for p in args.orders:
        for batch in args.batches:
            t, rows, iters = time_windowed(batch, n, W, H, p, MAXIT, args.reps, args.method,
                                           wtype, args.a, args.history, args.any_mask)
            gap, glo, ghi, _ = time_gpu(batch, n, W, H, p, MAXIT, args.reps, args.method)
            rounds = -(-rows // 256)
            row = dict(algorithm=args.algorithm, any_mask=args.any_mask, method=args.method, p=p,
                       a=args.a, gaps=batch,
                       rows=rows, workgroup_rounds=rounds, iters_min=iters[0],
                       iters_max=iters[1], history=args.history,
                       gap_wise_launch_ms=round(gap, 3), gap_wise_launch_ms_min=round(glo, 3),
                       gap_wise_launch_ms_max=round(ghi, 3))
            for k, (med, lo, hi) in t.items():
                row.update({f"{k}_ms": round(med, 4), f"{k}_ms_min": round(lo, 4),
                            f"{k}_ms_max": round(hi, 4)})
            print(f"p {p:5d} gaps {batch:4d} rows {rows:5d} ({rounds} round{'s' * (rounds > 1)})  "
                  + "  ".join(f"{k} {med:9.4f} ms [{lo:9.4f} .. {hi:9.4f}]"
                              for k, (med, lo, hi) in t.items())
                  + f"  gap-wise {gap:9.3f} ms [{glo:9.3f} .. {ghi:9.3f}]  iters {iters}",
                  flush=True)
            print(json.dumps(row), flush=True)


def _cpu_job(args):
    n, seed, s, h, p, maxit, method, algorithm = args
    if algorithm == "janssen":
        return cpu_janssen(signal(n, seed), s, h, p, maxit, method)
    return cpu_extrapolate(signal(n, seed), s, h, p, W, method)


def time_cpu(pool, workers, n, s, h, p, maxit, method, algorithm):
    """ms per segment with `workers` segments in flight (wall / workers)."""
    jobs = [(n, 100 + i, s, h, p, maxit, method, algorithm) for i in range(workers)]
    t0 = time.perf_counter()
    outs = pool.map(_cpu_job, jobs, chunksize=1)
    return (time.perf_counter() - t0) * 1e3 / workers, outs[0]


def cpu_table(n, threads, orders, method, algorithm):
    """{p: (ms alone, ms per segment at `threads` in flight, solution)}; runs
    and ends its worker processes before the caller opens the GPU."""
    import multiprocessing as mp
    out = {}
    with mp.get_context("spawn").Pool(threads) as pool:
        pool.map(_cpu_job, [(n, 100 + i, W, H, 64, 1, method, algorithm)
                            for i in range(4 * threads)],
                 chunksize=1)                       # every worker up: imports, FFT plans
        for p in orders:
            one, _ = time_cpu(pool, 1, n, W, H, p, MAXIT, method, algorithm)
            per, sol = time_cpu(pool, threads, n, W, H, p, MAXIT, method, algorithm)
            out[p] = (one, per, sol)
            print(f"cpu p {p:5d}  x1 {one:9.2f} ms/segment  x{threads} {per:9.2f} ms/segment "
                  f"({one / per:.1f} segments at a time)", flush=True)
        pool.close()
        pool.join()
    return out


def macs(n, p, h):
    return n * (p + 1) + p * p / 2 + h * min(2 * p, n - h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--fit", action="store_true")
    ap.add_argument("--method", choices=("lpc", "arburg"), default="lpc")
    ap.add_argument("--algorithm", default="janssen",
                    choices=("janssen", "extrapolation", "janssen_hann", "janssen_rect",
                             "janssen_tukey"))
    ap.add_argument("--a", type=int, default=1024)
    ap.add_argument("--history", action="store_true")
    ap.add_argument("--any-mask", action="store_true")
    ap.add_argument("--orders", type=lambda v: tuple(int(t) for t in v.split(",")), default=ORDERS)
    ap.add_argument("--batches", type=lambda v: tuple(int(t) for t in v.split(",")),
                    default=BATCHES)
    ap.add_argument("--burg-steps", action="store_true")
    args = ap.parse_args()
    n = 2 * W + H
    method, algorithm = args.method, args.algorithm
    if algorithm.startswith("janssen_"):
        return windowed_table(args, n)
    cpu = {} if args.no_cpu else cpu_table(n, args.threads, args.orders, method, algorithm)
    import torch
    print(f"{torch.cuda.get_device_name(0)}; {algorithm} {method}, n = {n}, h = {H}, "
          f"maxit = {MAXIT}", flush=True)
    for p in args.orders:
        cpu_one, cpu_ms, cpu_sol = cpu.get(p, (None, None, None))
        for batch in args.batches:
            med, lo, hi, gsol = time_gpu(batch, n, W, H, p, MAXIT, args.reps, method, algorithm)
            row = dict(algorithm=algorithm, method=method, p=p, batch=batch,
                       launch_ms=round(med, 3), launch_ms_min=round(lo, 3),
                       launch_ms_max=round(hi, 3), per_segment_ms=round(med / batch, 4),
                       per_iteration_us=round(med * 1e3 / MAXIT, 2))
            line = (f"p {p:5d} batch {batch:4d}  launch {med:9.3f} ms [{lo:9.3f} .. {hi:9.3f}]  "
                    f"{med / batch:9.4f} ms/segment  {med * 1e3 / MAXIT:9.2f} us/iteration")
            if cpu_ms is not None:
                row.update(cpu_ms_per_segment=round(cpu_ms, 2), cpu_workers=args.threads,
                           cpu_ms_one_worker=round(cpu_one, 2),
                           speedup_vs_cpu=round(cpu_ms / (med / batch), 2))
                line += f"  cpu {cpu_ms:9.2f} ms/segment  x{cpu_ms / (med / batch):.2f}"
                if batch == 1:
                    g = slice(W, W + H)
                    row["cpu_gpu_rel_diff"] = float(np.max(np.abs(cpu_sol[g] - gsol[g]))
                                                    / np.max(np.abs(gsol[g])))
            print(line, flush=True)
            print(json.dumps(row), flush=True)
    if args.burg_steps:
        for nn in (n, 16384):
            prev = None
            for p in ORDERS:
                med, lo, hi, _ = time_gpu(1, nn, nn // 2, 16, p, 1, args.reps, "arburg")
                slope = None if prev is None else (med - prev[1]) * 1e6 / (p - prev[0])
                print(f"burg steps n {nn:5d} p {p:5d}  iteration {med * 1e3:9.1f} us "
                      f"[{lo * 1e3:9.1f} .. {hi * 1e3:9.1f}]  {med * 1e6 / p:7.1f} ns/step"
                      + ("" if slope is None else f"  slope {slope:7.1f} ns/step"), flush=True)
                print(json.dumps(dict(burg_steps=True, n=nn, p=p, iteration_us=round(med * 1e3, 1),
                                      ns_per_step=round(med * 1e6 / p, 1),
                                      slope_ns_per_step=None if slope is None
                                      else round(slope, 1))), flush=True)
                prev = (p, med)
    if args.fit:
        cases = [(p, h) for p in ORDERS for h in (640, 1280)]
        t = np.array([time_gpu(1, n, W, h, p, MAXIT, args.reps)[0] * 1e3 / MAXIT
                      for p, h in cases])                              # us per iteration
        M = np.array([[p + h, macs(n, p, h)] for p, h in cases], dtype=np.float64)
        (c_step, c_mac), *_ = np.linalg.lstsq(M, t, rcond=None)
        print(f"fit: c_step = {c_step * 1e3:.1f} ns per recursion step, "
              f"c_mac = {c_mac * 1e6:.2f} ps per multiply-add "
              f"({1 / (c_mac * 1e3):.1f} multiply-adds per ns per workgroup)", flush=True)
        for (p, h), ti, row in zip(cases, t, M):
            fit = c_step * row[0] + c_mac * row[1]
            print(f"  p {p:5d} h {h:5d}  measured {ti:9.2f} us/iteration  model {fit:9.2f}  "
                  f"chain share {100 * c_step * row[0] / fit:5.1f} %", flush=True)
        print(json.dumps(dict(fit=True, c_step_ns=round(c_step * 1e3, 2),
                              c_mac_ps=round(c_mac * 1e6, 3),
                              cases=[dict(p=p, h=h, us_per_iteration=round(float(ti), 2))
                                     for (p, h), ti in zip(cases, t)])), flush=True)


if __name__ == "__main__":
    main()
