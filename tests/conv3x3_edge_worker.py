"""The integer cases of tests/conv3x3_ref.py on the GPU, shared by
tests/test_gpu_conv3x3_edges.py (in-process, the default environment) and run
as a script by it in a fresh child process for the routes that only an
environment switch reaches (csrc/conv_route.h conv_env() is read once):

  AINP_CONV_EXACT=1 python conv3x3_edge_worker.py <out.json> <planes> <cin>x<cout>:<prec> ...

planes: "edge" (EDGE_PLANES + the persistent-walk shape), "child" (CHILD_PLANES
+ the walk) or "short" (CHILD_PLANES only).  Writes the JSON list of failures
and exits 0 if and only if it is empty.  Integer cases need no tolerance: the
verdict is equality with the float64 reference, element by element, of every
launch in conv3x3_ref.calls().
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ml-audio-inpainting_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import conv3x3_ref as R  # noqa: E402

DEV = "cuda"
NAN = float("nan")
MAX_FAILURES = 40


def _first_bad(got, ref):
    """'' if got equals ref everywhere, else the first wrong index and values."""
    got = got.double()
    if got.shape == ref.shape and torch.equal(got, ref):
        return ""
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    bad = ~(got == ref)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return f"{int(bad.sum())} wrong of {ref.numel()}, first at {idx}: got {float(got[idx])} " \
           f"ref {float(ref[idx])}"


def _put(t, flag):
    """An NCHW tensor as an entry point takes it with its layout flag set or
    not: the shape the flag announces, the memory order of R.lay_of."""
    N, C, H, W = t.shape
    m = R.to_lay(t, R.lay_of(flag, C))
    return m.reshape(N, H, W, C) if flag else m


def _get(buf, flag, C):
    """The NCHW view of an output written under a layout flag (see _put)."""
    if flag and C <= 2:
        N, H, W, _ = buf.shape
        return buf.reshape(N, C, H, W)
    return R.from_lay(buf, "cl" if flag else "nchw")


class _Shape:
    """One (pair, shape, thin) on the device: the operands in both layouts and
    both storage types, built once.  The layout flags act on tensors of more
    than two channels (include/ainp.h): the 1-2-channel side of the small
    pairs stays planar whatever the flag says."""

    def __init__(self, cin, cout, N, H, W, thin):
        c = R.int_case(cin, cout, N, H, W, thin)
        self.c, self.key = c, (cin, cout, N, H, W, thin)
        self.dims = (N, cin, cout, H, W)
        d = lambda t: t.to(DEV)  # noqa: E731
        self.w, self.bias, self.scale, self.shift = d(c["w"]), d(c["bias"]), d(c["scale"]), d(c["shift"])
        self.x, self.dy = {}, {}
        for cl in (False, True):
            for s16 in (False, True):
                dt = torch.bfloat16 if s16 else torch.float32
                self.x[cl, s16] = d(_put(c["x"], cl)).to(dt)
                self.dy[cl, s16] = d(_put(c["dy"], cl)).to(dt)
        if cin in (16, 32, 64):   # the BatchNorm the fused data gradient feeds: any finite values
            g = torch.Generator().manual_seed(cin + H)
            self.bn_y = d(torch.randint(-3, 4, (N, H, W, cin), generator=g).float())
            self.bn = [d(torch.rand(cin, generator=g) + 0.5), d(torch.randn(cin, generator=g) * 0.3),
                       d(torch.cat([torch.randn(cin, generator=g) * 0.1,
                                    torch.rand(cin, generator=g) + 0.5]))]

    def refs(self, pro):
        return R.int_refs(*self.key, pro)


def _must_serve(ops, op, flags, dims):
    """The host-only queries promise that this call is served."""
    N, cin, cout, H, W = dims
    if flags & R.YCFNT:
        return ops.dgrad_cfnt_ok(N, cin, cout, H, W)
    ok = True
    if flags & (R.XCL | R.YCL | R.GCL):
        ok = ok and ops.cl_ok(N, cin, cout, H, W)
    if flags & R.DY16:
        ok = ok and ops.dy16_ok(N, cin, cout, H, W)
    if flags & (R.X16 | R.Y16):
        ok = ok and ops.io16_ok(N, cin, cout, H, W)
    if op == "bnr":
        ok = ok and (cin, cout) in R.MODEL_PAIRS
    return ok


def _launch(ops, s, op, flags, pro):
    """One launch into NaN-filled outputs -> dict of NCHW results on the CPU."""
    T, lib = torch.ops.ainp, ops._lib.lib
    N, cin, cout, H, W = s.dims
    sc, sh = (s.scale, s.shift) if pro else (None, None)
    nan = lambda shape, dt=torch.float32: torch.full(shape, NAN, device=DEV, dtype=dt)  # noqa: E731
    if op == "fwd":
        x = s.x[bool(flags & R.XCL), bool(flags & R.X16)]
        ycl = bool(flags & R.YCL)
        rows = lib.ainp_conv3x3_fwd_stat_rows_ex(N, cin, cout, H, W, flags)
        outs = []
        for _ in range(2):   # the second call: the same bits
            y = nan((N, H, W, cout) if ycl else (N, cout, H, W),
                    torch.bfloat16 if flags & R.Y16 else torch.float32)
            stats = nan((rows, 2 * cout), torch.float64)
            T.conv3x3_fwd(x, s.w, s.bias, sc, sh, y, stats, flags)
            outs.append((y, stats))
        same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        y, stats = outs[0]
        return dict(y=_get(y.float().cpu(), ycl, cout), stats=stats.cpu(),
                    same=same or bool(torch.isnan(stats).any()) or bool(torch.isnan(y).any()))
    if op in ("dgrad", "bnr"):
        dy = s.dy[bool(flags & R.XCL), bool(flags & R.DY16)]
        lay = "cfnt" if flags & R.YCFNT else "cl" if flags & R.YCL else "nchw"
        dx = nan({"cfnt": (cin, H, N, W), "cl": (N, H, W, cin), "nchw": (N, cin, H, W)}[lay])
        back = (lambda t: R.from_lay(t, lay)) if lay == "cfnt" else \
            (lambda t: _get(t, lay == "cl", cin))
        if op == "dgrad":
            T.conv3x3_dgrad(dy, s.w, dx, flags)
        else:
            y16 = bool(flags & R.DY16)
            ws = torch.empty(lib.ainp_conv3x3_dgrad_bnr_workspace(N, cin, cout, H, W), device=DEV,
                             dtype=torch.uint8)
            sums = nan((2 * cin,), torch.float64)
            T.conv3x3_dgrad_bnr(dy, s.w, dx, flags, s.bn_y.bfloat16() if y16 else s.bn_y, *s.bn,
                                ws, sums, R.BN_Y16 if y16 else 0)
            if not bool(torch.isfinite(sums).all()):
                return dict(dx=back(dx.cpu()), bad_sums=True)
        return dict(dx=back(dx.cpu()))
    x = s.x[bool(flags & R.XCL), bool(flags & R.X16)]
    dy = s.dy[bool(flags & R.GCL), bool(flags & R.DY16)]
    dw, db = nan((cout, cin, 3, 3)), nan((cout,))
    ws = torch.empty(lib.ainp_conv3x3_wgrad_workspace(N, cin, cout, H, W), device=DEV,
                     dtype=torch.uint8)
    T.conv3x3_wgrad(x, sc, sh, dy, dw, db, ws, flags)
    return dict(dw=dw.cpu(), db=db.cpu())


def _check(op, out, ref, cout):
    """-> list of what is wrong with one launch's results."""
    bad = []
    if op == "fwd":
        b = _first_bad(out["y"], ref["y"])
        if b:
            bad.append("y " + b)
        st = out["stats"]
        if bool(torch.isnan(st).any()):
            bad.append(f"stats: {int(torch.isnan(st).sum())} NaN left of {st.numel()}")
        else:
            tot = st.sum(0)
            for name, got, want, mag in (("sum y", tot[:cout], ref["sums"][:cout], ref["sabs"]),
                                         ("sum y^2", tot[cout:], ref["sums"][cout:],
                                          ref["sums"][cout:])):
                err = (got - want).abs()
                if bool((err > 1e-6 * mag).any()):
                    c = int((err - 1e-6 * mag).argmax())
                    bad.append(f"stats {name}[{c}] {float(got[c])} ref {float(want[c])}")
        if not out["same"]:
            bad.append("second call differs")
    elif op in ("dgrad", "bnr"):
        b = _first_bad(out["dx"], ref["dx"])
        if b:
            bad.append("dx " + b)
        if out.get("bad_sums"):
            bad.append("sums not finite")
    else:
        for k in ("dw", "db"):
            b = _first_bad(out[k], ref[k])
            if b:
                bad.append(f"{k} " + b)
    return bad


def flag_names(flags):
    names = [n for n in ("BF16", "DY16", "X16", "Y16", "XCL", "YCL", "GCL", "YCFNT")
             if flags & getattr(R, n)]
    return "|".join(names) or "0"


def run_int(ops, cin, cout, prec, shp, only=None, tally=None):
    """Every launch of R.calls(cin, cout, prec, shp) (only: of these entry
    points) against the float64 reference -> list of failure messages.
    tally: a dict counting launches served / refused."""
    texts = [t for t in R.refusal_texts().values() if t]
    fails, cur = [], None
    for op, N, H, W, flags, pro in R.calls(cin, cout, prec, shp):
        if only and op not in only:
            continue
        if len(fails) >= MAX_FAILURES:
            fails.append("... (more)")
            break
        tag = f"({cin},{cout}) {prec} {op} N={N} {H}x{W} {flag_names(flags)} pro={int(pro)}"
        thin = prec == "st16"
        if cur is None or cur.key != (cin, cout, N, H, W, thin):
            cur = _Shape(cin, cout, N, H, W, thin)
        try:
            out = _launch(ops, cur, op, flags, pro)
        except RuntimeError as e:
            msg = str(e)
            if "HIP error" in msg or "illegal memory" in msg:
                raise
            if _must_serve(ops, op, flags, cur.dims):
                fails.append(f"{tag}: refused though the queries accept it: {msg[:160]}")
            elif not any(t in msg for t in texts):
                fails.append(f"{tag}: refused with an unknown message: {msg[:160]}")
            if tally is not None:
                tally["refused"] = tally.get("refused", 0) + 1
            continue
        if tally is not None:
            tally["served"] = tally.get("served", 0) + 1
        for b in _check(op, out, cur.refs(pro), cout):
            fails.append(f"{tag}: {b}")
    return fails


def plane_set(name):
    if name == "edge":
        return R.shapes()
    if name == "child":
        return R.shapes(R.CHILD_PLANES)
    return R.shapes(R.CHILD_PLANES, walk=False)


def main(argv):
    out, planes = argv[1], argv[2]
    from ainp import ops
    fails, tally = [], {}
    for spec in argv[3:]:
        pair, prec = spec.split(":")
        cin, cout = (int(v) for v in pair.split("x"))
        fails += run_int(ops, cin, cout, prec, plane_set(planes), tally=tally)
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(fails, f)
    print(f"conv3x3_edge_worker: {tally} {len(fails)} failures")
    return 0 if not fails else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
