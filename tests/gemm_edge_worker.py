"""The cases of tests/gemm_ref.py on the GPU, shared by
tests/test_gpu_gemm_edges.py (in-process, the default environment) and run as a
script by it in a fresh child process for the routes that only an environment
switch reaches (csrc/gemm_route.h gemm_env() is read once):

  AINP_X6R_APF=0 python gemm_edge_worker.py <out.json> <spec> ...

spec: "f32:x6", "f32:exact", "f32:bf16", "bf16nt", "bf16multi", "x6nt",
"x6multi" or "copy" (gemm_ref.int_cases), or "cancel:<spec>" / "real:<spec>" for
the cancellation / real cases of a split-bf16 route (within_floor).  Writes the JSON list of failures and
exits 0 if and only if it is empty.

Every operand and every output is a view into a larger NaN-filled buffer
(gemm_ref.guarded: its ld above the extent, a guard row before and after, a
guard slab after the last split-K slab).  A read past an operand's edge turns
an output into NaN; after the call every output element outside the views must
still be NaN and every one inside finite.  Integer cases need no tolerance:
the verdict is equality with the float64 reference, element by element.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "ml-audio-inpainting_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import gemm_ref as R  # noqa: E402

DEV = "cuda"
MAX_FAILURES = 40


def first_bad(got, ref):
    """'' if got equals ref everywhere, else the first wrong index and values."""
    got = got.double()
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if torch.equal(got, ref):
        return ""
    bad = ~(got == ref)
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return f"{int(bad.sum())} wrong of {ref.numel()}, first at {idx}: got {float(got[idx])} " \
           f"ref {float(ref[idx])}"


class Out:
    """An output: NaN everywhere, or the initial C inside the view."""

    def __init__(self, shape, strides, init=None, dtype=torch.float32):
        t = torch.full(shape, R.NAN, dtype=dtype) if init is None else init
        self.buf, self.view = R.guarded(t, strides, device=DEV)

    def check(self, tag):
        """-> (the view on the CPU, what is wrong with the guards)."""
        m = R.inside_mask(self.buf, self.view)
        bad = []
        left = int((~torch.isnan(self.buf[~m])).sum())
        if left:
            first = int((~torch.isnan(self.buf) & ~m).nonzero()[0])
            bad.append(f"{tag}: {left} elements written outside the output, first at buffer offset "
                       f"{first - self.view.storage_offset()} from its start")
        inside = self.view.cpu()
        nf = int((~torch.isfinite(inside)).sum())
        if nf:
            idx = tuple(int(i) for i in (~torch.isfinite(inside)).nonzero()[0])
            bad.append(f"{tag}: {nf} elements not finite of {inside.numel()}, first at {idx}")
        return inside, bad


def _in(t, strides=None, off=0, dtype=None):
    t = t if dtype is None else t.to(dtype)
    return R.guarded(t, strides, off, device=DEV)[1]


def _vec(t):
    """A bias vector (contiguous) inside NaN guards."""
    return None if t is None else _in(t)


# ------------------------------------------------------------------ ainp_gemm_f32_ex
def launch_f32(ops, c, d, flags):
    """-> (list of C [M, N] on the CPU, guard failures)."""
    T, lib = torch.ops.ainp, ops._lib.lib
    M, N, K, nptr, ns = c["M"], c["N"], c["K"], c["nptr"], c["nstrided"]
    sam, sak, lda, sbk, sbn, ldb, scm, scn, ldc = R.f32_strides(c)
    ra = K if c["ta"] else M          # rows of the stored operand
    rb = N if c["tb"] else K
    rc, cc = (N, M) if c["c_col"] else (M, N)
    sA, sB, sC = ra * lda + c["sa_extra"], rb * ldb + c["sb_extra"], rc * ldc + 8
    nC = ns if c["ksplit"] == 0 else 1
    As, Bs, outs, b1, b2 = [], [], [], [], []
    for p in range(nptr):
        last = p == nptr - 1
        offa = c["off_a"] if (last or not c["off_last"]) else 0
        offb = c["off_b"] if (last or not c["off_last"]) else 0
        a = torch.stack([d["A"][p + s * nptr].T if c["ta"] else d["A"][p + s * nptr] for s in range(ns)])
        b = torch.stack([d["B"][p + s * nptr].T if c["tb"] else d["B"][p + s * nptr] for s in range(ns)])
        if c["share_a"] and p:
            As.append(As[0])
        else:
            As.append(_in(a, (max(sA, 1), lda, 1), offa))
        Bs.append(_in(b, (max(sB, 1), ldb, 1), offb))
        init = None
        if c["beta"] != 0 and (c["ksplit"] != 1 or p == 0):
            ci = [d["C0"][p + s * nptr] if c["ksplit"] == 0 else d["C0"][p] for s in range(nC)]
            init = torch.stack([t.T if c["c_col"] else t for t in ci])
        outs.append(Out((nC, rc, cc), (sC, ldc, 1), init))
        b1.append(_vec(d["b1"][p]) if c["bias"] & 1 else None)
        b2.append(_vec(d["b2"][p]) if c["bias"] & 2 else None)
    need = int(lib.ainp_gemm_f32_workspace(M, N, K, nptr, ns, c["ksplit"]))
    ws = None
    if need and c["ws"] != "none":
        ws = torch.empty(need - (1 if c["ws"] == "short" else 0), device=DEV, dtype=torch.uint8)
    T.gemm(M, N, K, c["alpha"], As, sam, sak, sA, Bs, sbk, sbn, sB, c["beta"],
           [o.view for o in outs], scm, scn, sC, b1 if c["bias"] & 1 else [],
           b2 if c["bias"] & 2 else [], ns, c["ksplit"], flags, ws)
    res, bad = [], []
    written = {0: range(nptr), 1: range(1), 2: range(nptr)}[c["ksplit"]]
    for p, o in enumerate(outs):
        if p not in written:       # K-concatenation into C[0]: the other C pointers stay untouched
            left = int((~torch.isnan(o.buf)).sum())
            if left:
                bad.append(f"C[{p}]: {left} elements written though ksplit == 1 sums into C[0]")
            continue
        inside, b = o.check(f"C[{p}]")
        bad += b
        res.append([t.T if c["c_col"] else t for t in inside])
    # reference order: ksplit 0 by batch b = p + s nptr; 1: C[0]; 2: by pointer batch
    if c["ksplit"] == 0:
        flat = [res[p][s] for s in range(ns) for p in range(nptr)]
    else:
        flat = [r[0] for r in res]
    return flat, bad


# ------------------------------------------------------------------ the nt entries
def _rows(t, pad, km, dtype, ld=None):
    """Logical [R, K] as the entry takes it: [R][ld] k-contiguous or k-major [K][ld]."""
    t = t.T if km else t
    ld = t.shape[1] + pad if ld is None else ld
    return _in(t, (ld, 1), dtype=dtype)


def _bias(d):
    return [_vec(t) for t in d["bias"]]


def _slabs(p, rows):
    """Split-K slabs [nsplit, rows, N] with ldc above N and a gap between slabs."""
    ldc = p["N"] + p["pad_c"]
    return Out((p["nsplit"], rows, p["N"]), ((rows + 2) * ldc, ldc, 1))


def _c_arg(o, S):
    return o.view if S > 1 else o.view[0]


def launch_nt(ops, c, ds):
    """-> (one [nsplit, M, N] per problem on the CPU, guard failures)."""
    T, e = torch.ops.ainp, c["entry"]
    b16 = torch.bfloat16 if R.IS_BF16[e] else None
    outs, args = [], []
    for p, d in zip(c["probs"], ds):
        M, N, K, S = p["M"], p["N"], p["K"], p["nsplit"]
        if e in ("bf16nt", "bf16multi"):
            A = _rows(d["A"], p["pad_a"], p["akm"], b16)
            B = _rows(d["B"], p["pad_b"], p["bkm"], b16)
            o = _slabs(p, M)
            outs.append([o])
            args.append((A, B, o, p, d))
        elif e == "x6nt":
            ldb = K + p["pad_b"]
            A = _rows(d["A"], p["pad_a"], False, None)
            b1 = _rows(d["B"][:p["bsplit"]], 0, False, None, ldb)
            b2 = _rows(d["B"][p["bsplit"]:], 0, False, None, ldb) if p["bsplit"] < N else b1[:0]
            o = _slabs(p, M)
            outs.append([o])
            args.append((A, b1, b2, o, p, d))
        else:
            ak, bk, bn, cm = p["a_ksplit"], p["b_ksplit"], p["b_nsplit"], p["c_msplit"]
            a_parts = [d["A"][:, :ak], d["A"][:, ak:]] if ak else [d["A"], None]
            if bk:
                b_parts = [d["B"][:, :bk], d["B"][:, bk:]]
            elif bn:
                b_parts = [d["B"][:bn], d["B"][bn:]]
            else:
                b_parts = [d["B"], None]

            def ld_of(parts, km, pad):
                return max((t.shape[0] if km else t.shape[1]) for t in parts if t is not None) + pad
            lda, ldb = ld_of(a_parts, p["akm"], p["pad_a"]), ld_of(b_parts, p["bkm"], p["pad_b"])
            Av = [None if t is None else _rows(t, 0, p["akm"], None, lda) for t in a_parts]
            Bv = [None if t is None else _rows(t, 0, p["bkm"], None, ldb) for t in b_parts]
            m1 = cm if cm else M
            ldc = N + p["pad_c"]
            stride = (max(m1, M - m1) + 2) * ldc
            o1 = Out((S, m1, N), (stride, ldc, 1))
            o2 = Out((S, M - m1, N), (stride, ldc, 1)) if cm else None
            outs.append([o1, o2])

            def flat2d(o):   # the slabs as one 2-D strided view: what torch_ops' extent check takes
                v = o.view
                return v.as_strided(((S - 1) * (stride // ldc) + v.shape[1], N), (ldc, 1),
                                    v.storage_offset())
            args.append(ops.x6_problem(Av[0], Bv[0], flat2d(o1), M, N, K, lda, ldb, ldc, A2=Av[1],
                                       a_ksplit=ak, a_kmajor=p["akm"], B2=Bv[1], b_nsplit=bn,
                                       b_ksplit=bk, b_kmajor=p["bkm"],
                                       C2=flat2d(o2) if cm else None, c_msplit=cm, bias=_bias(d),
                                       bias_nsplit=p["bias_nsplit"], nsplit=S, kc=p["kc"],
                                       strideC=stride))
    if e == "bf16nt":
        A, B, o, p, d = args[0]
        T.gemm_bf16nt(A, B, _c_arg(o, p["nsplit"]), p["K"], *_bias(d), p["bias_nsplit"], p["nsplit"],
                      p["kc"])
    elif e == "bf16multi":
        ops.gemm_bf16nt_multi([(A, B, _c_arg(o, p["nsplit"]), p["K"], p["nsplit"], p["kc"], p["akm"],
                                p["bkm"]) for A, B, o, p, d in args])
    elif e == "x6nt":
        A, b1, b2, o, p, d = args[0]
        T.gemm_x6nt_256(A, b1, b2, _c_arg(o, p["nsplit"]), *_bias(d), p["bias_nsplit"], p["nsplit"],
                        p["kc"])
    else:
        ops.gemm_x6_multi(args)
    res, bad = [], []
    for q, os_ in enumerate(outs):
        parts = []
        for i, o in enumerate(os_):
            if o is not None:
                inside, b = o.check(f"problem {q} C{'2' if i else ''}")
                bad += b
                parts.append(inside)
        res.append(torch.cat(parts, 1))
    return res, bad


# ------------------------------------------------------------------ cast / transpose
SENTINEL16 = 0x7FFF     # the cast's guard: a NaN pattern (NaN guards would hide among NaN data)


def launch_copy(ops, c):
    """-> failures: bits compared with torch's .bfloat16() / the transpose."""
    T = torch.ops.ainp
    Rr, Cc = c["R"], c["C"]
    x = R.copy_data(Rr, Cc)
    xv = _in(x, (Cc + c["pad_in"], 1))
    bad = []
    if c["entry"] == "transpose":
        o = Out((Cc, Rr), (Rr + c["pad_t"], 1))
        T.transpose_f32(xv, o.view)
        m = R.inside_mask(o.buf, o.view)
        if int((~torch.isnan(o.buf[~m])).sum()):
            bad.append("outT: written outside the output")
        if not torch.equal(o.view.cpu().view(torch.int32), x.T.contiguous().view(torch.int32)):
            bad.append("outT: bits differ from the transpose")
        return bad
    want = x.bfloat16()
    nan = torch.isnan(x)
    pairs = []
    for on, shape, pad, ref, rnan in ((c["out"], (Rr, Cc), c["pad_out"], want, nan),
                                      (c["outT"], (Cc, Rr), c["pad_t"], want.T, nan.T)):
        if on:
            buf, view = R.guarded(torch.full(shape, SENTINEL16, dtype=torch.int16),
                                  (shape[1] + pad, 1), device=DEV, fill=SENTINEL16)
            pairs.append((buf, view, ref, rnan))
        else:
            pairs.append(None)
    T.cast_bf16_t(xv, *(None if p is None else p[1].view(torch.bfloat16) for p in pairs))
    for name, p in zip(("out", "outT"), pairs):
        if p is None:
            continue
        buf, view, ref, rnan = p
        m = R.inside_mask(buf, view)
        if int((buf[~m] != SENTINEL16).sum()):
            bad.append(f"{name}: written outside the output")
        got = view.cpu()
        gf = got.view(torch.bfloat16)
        if not bool(torch.isnan(gf[rnan]).all()):
            bad.append(f"{name}: a NaN did not stay NaN")
        diff = (got != ref.contiguous().view(torch.int16)) & ~rnan
        if bool(diff.any()):
            idx = tuple(int(i) for i in diff.nonzero()[0])
            src = idx if name == "out" else idx[::-1]
            bad.append(f"{name}: {int(diff.sum())} elements differ from .bfloat16(), first at {idx}: "
                       f"x bits {int(x.view(torch.int32)[src]) & 0xFFFFFFFF:#010x} got "
                       f"{int(got[idx]) & 0xFFFF:#06x}")
    return bad


# ------------------------------------------------------------------ running cases
def launch(ops, c, flags, real=False):
    """-> (outputs, references in float64, in float32 or None, failures)."""
    if c["entry"] == "f32":
        d = R.f32_data(c, real)
        got, bad = launch_f32(ops, c, d, flags)
        return got, R.f32_ref_of(c, flags, real), (R.f32_ref_of(c, flags, real, True) if real else None), bad
    ds = [R.nt_data(c, q, real) for q in range(len(c["probs"]))]
    got, bad = launch_nt(ops, c, ds)
    n = range(len(ds))
    return (got, [R.nt_ref_of(c, q, real) for q in n],
            [R.nt_ref_of(c, q, real, True) for q in n] if real else None, bad)


def tag_of(c, flags):
    prec = {0: "", R.EXACT_F32: ":exact", R.BF16: ":bf16"}[flags] if c["entry"] == "f32" else ""
    return f"{c['entry']}{prec}/{c['name']}"


def refusal(c):
    return c.get("refused") if c["entry"] != "f32" else None


def is_gpu_error(msg):
    """A failed launch or a HIP error, not a refusal (AINP_EINVAL = -1, a TORCH_CHECK)."""
    return "HIP error" in msg or "illegal memory" in msg or "hipError" in msg or "failed (-2)" in msg


def run_int(ops, cases, tally=None):
    """Every (case, flags) against the float64 reference -> failure messages."""
    lib = ops._lib.lib
    fails = []
    for c, flags in cases:
        if len(fails) >= MAX_FAILURES:
            fails.append("... (more)")
            break
        tag = tag_of(c, flags)
        if c["entry"] in ("cast", "transpose"):
            fails += [f"{tag}: {b}" for b in launch_copy(ops, c)]
            continue
        if c["entry"] == "f32":      # the workspace query says what the case table says
            need = int(lib.ainp_gemm_f32_workspace(c["M"], c["N"], c["K"], c["nptr"], c["nstrided"],
                                                   c["ksplit"]))
            if (need > 0) != c["sk"]:
                fails.append(f"{tag}: the workspace query gives {need} bytes, the table says "
                             f"stream-K is {c['sk']}")
        if c.get("tile") is not None:
            p = c["probs"][0]
            tile = ops.gemm_bf16nt_tile(p["M"], p["N"], p["K"], p["nsplit"])
            want = c["tile"]
            if not ops.GEMM16_256:
                want = 0
            elif want == 2 and ops.gemm_bf16nt_tile(512, 512, 64) == 1:     # AINP_G256_BK64=0
                want = 1
            if tile != want:
                fails.append(f"{tag}: ainp_gemm_bf16nt_tile names tile {tile}, the table {want}")
        try:
            got, ref, _, bad = launch(ops, c, flags)
            if c.get("sk"):          # a second call gives the same bits
                again = launch(ops, c, flags)[0]
                if not all(torch.equal(a, b) for a, b in zip(got, again)):
                    bad.append("the second call differs")
        except RuntimeError as e:
            msg = str(e)
            if is_gpu_error(msg):
                raise
            if refusal(c) is None:
                fails.append(f"{tag}: refused: {msg[:200]}")
            elif refusal(c) not in msg:
                fails.append(f"{tag}: refused with another message than '{refusal(c)}': {msg[:200]}")
            if tally is not None:
                tally["refused"] = tally.get("refused", 0) + 1
            continue
        if tally is not None:
            tally["served"] = tally.get("served", 0) + 1
        if refusal(c) is not None:
            fails.append(f"{tag}: served though the header's contract refuses it")
            continue
        fails += [f"{tag}: {b}" for b in bad]
        for i, (g, r) in enumerate(zip(got, ref)):
            b = first_bad(g, r)
            if b:
                fails.append(f"{tag}: output {i}: {b}")
    return fails


# split-bf16 / bf16 routes that need the analytic bound instead of the floor rule
# (none: DESIGN.md, "Edge-shape tests", has the measured figures)
ANALYTIC = set()


def _abs_bound(c, flags):
    """(K + 8) 2^-24 (|alpha| sum |a||b| + |bias| + |beta C|) per element: the
    first-order bound of any fp32 summation of the rounded operands."""
    u = 2.0 ** -24
    if c["entry"] == "f32":
        d = R.f32_data(c, not c["name"].startswith("cancel-"))
        dd = {k: [t.abs() for t in v] for k, v in d.items()}
        ab = dict(c, alpha=abs(c["alpha"]), beta=abs(c["beta"]))
        kk = c["K"] * (c["nptr"] * c["nstrided"] if c["ksplit"] == 1 else
                       c["nstrided"] if c["ksplit"] == 2 else 1)
        return [(kk + 8) * u * t for t in R.f32_ref(ab, dd, flags)]
    out = []
    for q, p in enumerate(c["probs"]):
        d = R.nt_data(c, q, True)
        dd = dict(A=d["A"].abs(), B=d["B"].abs(), bias=[None if t is None else t.abs() for t in d["bias"]])
        out.append((p["kc"] + 8) * u * R.nt_ref(p, dd, R.IS_BF16[c["entry"]]))
    return out


def run_real(ops, cases, worst=None):
    """within_floor on every output of every (case, flags); prints what it
    measured, with the share of the analytic bound the worst element uses.
    -> failure messages; worst: route -> the largest shares."""
    fails = []
    for c, flags in cases:
        tag = tag_of(c, flags)
        got, ref64, ref32, bad = launch(ops, c, flags, real=True)
        fails += [f"{tag}: {b}" for b in bad]
        key = tag.split("/")[0]
        for i, (g, r64, r32, bnd) in enumerate(zip(got, ref64, ref32, _abs_bound(c, flags))):
            dev, floor, ok = R.within_floor(g, r64, r32)
            scale = float(r64.abs().max())
            allowed = 4.0 * floor + 4e-7 * scale
            share = dev / allowed if allowed > 0 else 0.0
            ashare = float(((g.double() - r64).abs() / bnd.clamp_min(1e-300)).max())
            print(f"{tag} output {i}: dev {dev:.3e} floor {floor:.3e} max|ref| {scale:.3e} "
                  f"share {share:.2f} analytic share {ashare:.2f}")
            if worst is not None:
                w = worst.setdefault(key, [0.0, 0.0])
                w[0], w[1] = max(w[0], share), max(w[1], ashare)
            if not (ok or (key in ANALYTIC and ashare <= 1.0)):
                fails.append(f"{tag}: output {i}: deviation {dev:.3e} above 4 x {floor:.3e} + 4e-7 x "
                             f"{scale:.3e} ({share:.2f} of the allowance)")
    return fails


def real_cases(spec):
    """"real:<spec>" / "cancel:<spec>" of gemm_ref.SPECS -> [(case, flags)]."""
    kind, spec = spec.split(":", 1)
    if spec.startswith("f32:"):
        prec = spec[4:]
        table = R.REAL_F32 if kind == "real" else (R.CANCEL_F32 if prec == "x6" else [])
        return [(c, R.FLAGS[prec]) for c in table if c["only"] in (None, prec)]
    return [(c, 0) for c in (R.REAL_NT if kind == "real" else R.CANCEL_NT).get(spec, [])]


def main(argv):
    out = argv[1]
    from ainp import ops
    fails, tally = [], {}
    for spec in argv[2:]:
        if spec.startswith(("real:", "cancel:")):
            fails += run_real(ops, real_cases(spec))
        else:
            fails += run_int(ops, R.int_cases(spec), tally=tally)
    torch.cuda.synchronize()
    with open(out, "w") as f:
        json.dump(fails, f)
    print(f"gemm_edge_worker: {tally} {len(fails)} failures")
    return 0 if not fails else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
