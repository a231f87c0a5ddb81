"""tests/gemm_ref.py without a GPU: the references of the GEMM family's ABI
against plain torch.matmul compositions, the conditions under which the integer
cases are exact in every summation order, the memory layouts
tests/gemm_edge_worker.py builds against an index-by-index reading of
include/ainp.h, the power of the cancellation cases on an emulation of the
split-bf16 loop, the refusals of the launchers (their checks run before any
launch, so the library answers without a device) and the kernel every case
reaches under every switch.
"""
import ctypes
import re
import subprocess

import pytest
import torch

import gemm_edge_worker as W
import gemm_ref as R

TWO23 = 2.0 ** 23


def _all_f32():
    return R.F32_CASES + R.SK_CASES


def _all_nt():
    return [c for e in R.NT_CASES for c in R.NT_CASES[e]]


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("name", ["nptr2x3", "ksplit1", "ksplit2", "ep-a2.0-b0.5-bias3", "K0-batched"])
def test_f32_reference_against_matmul_compositions(name):
    """ksplit 1 / 2 are K-concatenations: one matmul of the operands laid side
    by side; ksplit 0 is torch.bmm; bias and beta C by broadcasting."""
    c = next(x for x in R.F32_CASES if x["name"] == name)
    d = R.f32_data(c)
    nptr, ns = c["nptr"], c["nstrided"]
    ref = R.f32_ref(c, d, 0)
    A = [t.double() for t in d["A"]]
    B = [t.double() for t in d["B"]]
    if c["ksplit"] == 0:
        prod = list(torch.bmm(torch.stack(A), torch.stack(B)))
        owner = [b % nptr for b in range(nptr * ns)]
    elif c["ksplit"] == 1:
        prod = [torch.cat(A, 1) @ torch.cat(B, 0)]
        owner = [0]
    else:
        prod = [torch.cat(A[p::nptr], 1) @ torch.cat(B[p::nptr], 0) for p in range(nptr)]
        owner = list(range(nptr))
    assert len(ref) == len(prod)
    for i, (r, t) in enumerate(zip(ref, prod)):
        want = c["alpha"] * t + c["beta"] * d["C0"][i].double()
        if c["bias"] & 1:
            want = want + d["b1"][owner[i]].double()[None, :]
        if c["bias"] & 2:
            want = want + d["b2"][owner[i]].double()[None, :]
        assert torch.equal(r, want), (name, i)
    # the bf16 flag rounds every operand element, and only the operands
    dr = R.f32_data(c, real=True)
    r16 = R.f32_ref(c, dr, R.BF16)
    dq = dict(dr, A=[t.bfloat16().float() for t in dr["A"]], B=[t.bfloat16().float() for t in dr["B"]])
    assert all(torch.equal(a, b) for a, b in zip(r16, R.f32_ref(c, dq, 0)))
    assert not torch.equal(r16[0], R.f32_ref(c, dr, 0)[0]) or c["K"] == 0


def _served_nt():
    return [c for c in _all_nt() if not c["refused"]]


def test_nt_reference_against_matmul_compositions():
    for c in _served_nt():
        for q, p in enumerate(c["probs"]):
            d = R.nt_data(c, q)
            r = R.nt_ref(p, d, False)
            assert r.shape == (p["nsplit"], p["M"], p["N"])
            full = d["A"].double() @ d["B"].double().T
            bias = torch.zeros(p["N"], dtype=torch.float64)
            for n in range(p["N"]):
                lo = n < p["bias_nsplit"]
                for t in (d["bias"][0:2] if lo else d["bias"][2:4]):
                    if t is not None:
                        bias[n] += float(t[n if lo else n - p["bias_nsplit"]])
            assert torch.equal(r.sum(0), full + bias), (c["name"], q)       # integers: any order
            assert torch.equal(r[0] - bias, (d["A"][:, :p["kc"]].double() @ d["B"][:, :p["kc"]].double().T))
            for t, n in zip(d["bias"], (p["bias_nsplit"],) * 2 + (p["N"] - p["bias_nsplit"],) * 2):
                assert t is None or t.numel() == n
            # the table asks for what its mask says wherever the segment is not empty
            given = sum(bit for bit, t in zip((R.A1, R.A2, R.B1, R.B2), d["bias"]) if t is not None)
            empty = (R.A1 | R.A2 if p["bias_nsplit"] == 0 else 0) | \
                    (R.B1 | R.B2 if p["bias_nsplit"] == p["N"] else 0)
            assert given == p["bias"] & ~empty


# ------------------------------------------------------------------ integer data
def _is_int(t):
    return bool((t == t.round()).all())


def _bf16_exact(t):
    return torch.equal(t.bfloat16().float(), t)


def test_integer_cases_are_exact():
    """For every case of the tables: operands, biases and the initial C are
    integers, the operands exact in bf16, alpha and beta from {1, -1, 2, 0.5, 0},
    and sum |a||b| + |bias| + |beta C| (times |alpha|) below 2^24 -- below 2^23
    where a factor 0.5 makes half-integers -- so every product and every partial
    sum in any order and any of the three loops is exact in fp32; the float32
    torch evaluation already equals the float64 one."""
    for c in _all_f32():
        d = R.f32_data(c)
        assert c["alpha"] in (1.0, -1.0, 2.0, 0.5, 0.0) and c["beta"] in (1.0, -1.0, 2.0, 0.5, 0.0)
        for k in ("A", "B", "C0", "b1", "b2"):
            assert all(_is_int(t) for t in d[k]), (c["name"], k)
        assert all(_bf16_exact(t) and float(t.abs().max() if t.numel() else 0) <= 3
                   for k in ("A", "B") for t in d[k]), c["name"]
        bound = R.f32_bound(c, d)
        assert bound < (TWO23 if 0.5 in (c["alpha"], c["beta"]) else R.TWO24), (c["name"], bound)
        r64 = R.f32_ref_of(c, 0)
        r32 = R.f32_ref(c, d, 0, torch.float32)
        assert all(t.dtype == torch.float32 and torch.equal(t.double(), r) for t, r in zip(r32, r64)), \
            c["name"]
        if c["K"] <= 512:       # the flags change nothing on this data
            for flags in (R.EXACT_F32, R.BF16):
                assert all(torch.equal(a, b) for a, b in zip(R.f32_ref(c, d, flags), r64)), c["name"]
    for c in _served_nt():
        for q, p in enumerate(c["probs"]):
            d = R.nt_data(c, q)
            assert _is_int(d["A"]) and _is_int(d["B"]) and _bf16_exact(d["A"]) and _bf16_exact(d["B"])
            assert float(d["A"].abs().max()) <= 3 and float(d["B"].abs().max()) <= 3
            assert all(t is None or _is_int(t) for t in d["bias"])
            assert R.nt_bound(p, d) < R.TWO24, c["name"]
            assert torch.equal(R.nt_ref(p, d, True, torch.float32).double(), R.nt_ref(p, d, False))


def test_special_values_of_the_cast():
    """The patterns are what the comments say: exact ties both ways, a tie and
    the largest finite fp32 that round to inf, subnormals; every row and column
    residue of the 64 x 64 tile sees them."""
    bits = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in R.SPECIAL_BITS],
                        dtype=torch.int32)
    x = bits.view(torch.float32)
    y = x.bfloat16().view(torch.int16).int() & 0xFFFF
    want = {0x3F808000: 0x3F80, 0x3F818000: 0x3F82, 0xBF808000: 0xBF80, 0xBF818000: 0xBF82,
            0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80, 0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,
            0x7F7F8000: 0x7F80, 0x00000001: 0x0000, 0x80000001: 0x8000, 0x00400000: 0x0040,
            0x007FFFFF: 0x0080, 0x00008000: 0x0000, 0x00018000: 0x0002, 0x80000000: 0x8000}
    for b, yy in zip(R.SPECIAL_BITS, y.tolist()):
        if b in want:
            assert yy == want[b], hex(b)
    assert int(torch.isnan(x).sum()) == 2 and bool(torch.isnan(x.bfloat16()[torch.isnan(x)]).all())
    d = R.copy_data(130, 130).view(torch.int32)
    pos = (d == bits[0]).nonzero()
    assert len({int(r) % 64 for r, _ in pos}) > 8 and len({int(c) % 64 for _, c in pos}) > 8


# ------------------------------------------------------------------ layouts
class _FakeT:
    """torch.ops.ainp's GEMM family read off include/ainp.h index by index, on
    the CPU: every element through its documented address in the storage the
    view points into (torch checks the bounds), never through the view's shape."""

    @staticmethod
    def _at(t, shape, strides, extra=0):
        return torch.as_strided(t, shape, strides, t.storage_offset() + extra)

    def gemm(self, M, N, K, alpha, A, sam, sak, sA, B, sbk, sbn, sB, beta, C, scm, scn, sC, b1, b2,
             ns, ksplit, flags, ws):
        nptr = len(A)
        nb = nptr * ns
        acc = {}
        for b in range(nb):
            p, s = b % nptr, b // nptr
            a = self._at(A[p], (M, K), (sam, sak), s * sA).double()
            bb = self._at(B[p], (K, N), (sbk, sbn), s * sB).double()
            dst = (p, s) if ksplit == 0 else ((0, 0) if ksplit == 1 else (p, 0))
            acc[dst] = acc.get(dst, 0) + a @ bb
        for (p, s), t in acc.items():
            out = self._at(C[p], (M, N), (scm, scn), s * sC)
            r = alpha * t
            if b1:
                r = r + b1[p].double()
            if b2:
                r = r + b2[p].double()
            if beta != 0:
                r = r + beta * out.double()
            out.copy_(r)

    def _nt(self, a, b, C, ldc, strideC, bias, bias_nsplit, M, N, K, S, kc):
        for s in range(S):
            k0, k1 = (0, K) if S == 1 else (s * kc, min(K, (s + 1) * kc))
            r = a[:, k0:k1].double() @ b[:, k0:k1].double().T
            if s == 0:
                r = r + R.bias_vec(bias, bias_nsplit, N)
            self._at(C, (M, N), (ldc, 1), s * strideC).copy_(r)

    def gemm_bf16nt(self, A, B, C, K, a1, a2, b1, b2, bias_nsplit, S, kc):
        M, N = A.shape[0], B.shape[0]
        self._nt(self._at(A, (M, K), (A.stride(0), 1)), self._at(B, (N, K), (B.stride(0), 1)), C,
                 C.stride(-2), C.stride(0) if C.dim() == 3 else 0, (a1, a2, b1, b2), bias_nsplit,
                 M, N, K, S, kc)

    def gemm_x6nt_256(self, A, B1, B2, C, a1, a2, b1, b2, bias_nsplit, S, kc):
        M, K, N1 = A.shape[0], A.shape[1], B1.shape[0]
        N = N1 + B2.shape[0]
        b = torch.cat([self._at(B1, (N1, K), (B1.stride(0), 1)),
                       self._at(B2, (N - N1, K), (B1.stride(0), 1))])
        self._nt(self._at(A, (M, K), (A.stride(0), 1)), b, C, C.stride(-2),
                 C.stride(0) if C.dim() == 3 else 0, (a1, a2, b1, b2), bias_nsplit, M, N, K, S, kc)

    def transpose_f32(self, x, outT):
        outT.copy_(x.T)

    def cast_bf16_t(self, x, out, outT):
        if out is not None:
            out.copy_(x.bfloat16())
        if outT is not None:
            outT.copy_(x.bfloat16().T)


class _FakeOps:
    def __init__(self):
        from ainp import _lib, ops
        self._lib, self.x6_problem = _lib, ops.x6_problem
        self.gemm_bf16nt_tile, self.GEMM16_256 = ops.gemm_bf16nt_tile, ops.GEMM16_256
        self.T = _FakeT()

    def gemm_bf16nt_multi(self, problems):
        for A, B, C, K, S, kc, akm, bkm in problems:
            M, N = C.shape[-2], C.shape[-1]
            a = self.T._at(A, (M, K), (1, A.stride(0)) if akm else (A.stride(0), 1))
            b = self.T._at(B, (N, K), (1, B.stride(0)) if bkm else (B.stride(0), 1))
            self.T._nt(a, b, C, C.stride(-2), C.stride(0) if C.dim() == 3 else 0, (None,) * 4, 0,
                       M, N, K, S, kc)

    def gemm_x6_multi(self, problems):
        at = self.T._at
        for pr in problems:
            A, A2, B, B2, *bias = pr["ins"]
            C, C2 = pr["outs"]
            (ak, akm, bn, bk, bkm, cm, bias_ns, M, N, K, S, kc, strideC, lda, ldb, ldc) = pr["ints"]
            sa, sb = ((1, lda) if akm else (lda, 1)), ((1, ldb) if bkm else (ldb, 1))
            a = at(A, (M, ak if A2 is not None else K), sa)
            if A2 is not None:
                a = torch.cat([a, at(A2, (M, K - ak), sa)], 1)
            if B2 is not None and bk > 0:
                b = torch.cat([at(B, (N, bk), sb), at(B2, (N, K - bk), sb)], 1)
            elif B2 is not None:
                b = torch.cat([at(B, (bn, K), sb), at(B2, (N - bn, K), sb)], 0)
            else:
                b = at(B, (N, K), sb)
            m1 = cm if C2 is not None else M
            for s in range(S):
                k0, k1 = (0, K) if S == 1 else (s * kc, min(K, (s + 1) * kc))
                r = a[:, k0:k1].double() @ b[:, k0:k1].double().T
                if s == 0:
                    r = r + R.bias_vec(bias, bias_ns, N)
                at(C, (m1, N), (ldc, 1), s * strideC).copy_(r[:m1])
                if C2 is not None:
                    at(C2, (M - m1, N), (ldc, 1), s * strideC).copy_(r[m1:])


@pytest.fixture()
def fake(monkeypatch):
    ops = _FakeOps()
    monkeypatch.setattr(W, "DEV", "cpu")
    monkeypatch.setattr(torch.ops, "ainp", ops.T, raising=False)
    return ops


CPU_SPECS = ["f32:x6", "f32:exact", "bf16nt", "bf16multi", "x6nt", "x6multi", "copy"]
SK_ON_CPU = ("sk-order1-col", "sk-2ptr-shareA", "sk-not-full")


@pytest.mark.parametrize("spec", CPU_SPECS)
def test_worker_layouts_follow_the_header(fake, spec):
    """Every case of the tables, laid out by the worker and evaluated by the
    index-by-index reading of the header, equals the reference: the strides,
    offsets, splits and slabs the GPU tests pass are the ones the header means,
    and none reaches outside its buffer.  (Of the exact loop's cases only the
    stream-K layouts that differ from the small cases are repeated.)"""
    cases = [(c, f) for c, f in R.int_cases(spec)
             if W.refusal(c) is None and (c["name"] in SK_ON_CPU if spec == "f32:exact" else True)]
    assert cases
    fails = W.run_int(fake, [(dict(c, sk=False) if c["entry"] == "f32" else c, f) for c, f in cases])
    fails = [f for f in fails if "workspace query" not in f]
    assert not fails, "\n".join(fails[:20])


def test_worker_sees_a_write_outside_and_a_read_outside(fake, monkeypatch):
    """The guards work: a launch that writes one element past a row, or reads one
    past an operand's row, is reported."""
    c = next(x for x in R.NT_CASES["bf16nt"] if x["name"] == "M129")
    real = fake.T.gemm_bf16nt

    def writes_past(A, B, C, K, *rest):
        real(A, B, C, K, *rest)
        torch.as_strided(C, (1,), (1,), C.storage_offset() + C.shape[-1]).fill_(1.0)

    def reads_past(A, B, C, K, *rest):
        wide = torch.as_strided(A, (A.shape[0], K + 8), (A.stride(0), 1), A.storage_offset())
        real(wide, torch.nn.functional.pad(B[:, :K], (0, 8), value=1.0), C, K + 8, *rest)
    monkeypatch.setattr(fake.T, "gemm_bf16nt", writes_past)
    fails = W.run_int(fake, [(c, 0)])
    assert len(fails) == 1 and "written outside" in fails[0]
    monkeypatch.setattr(fake.T, "gemm_bf16nt", reads_past)
    fails = W.run_int(fake, [(c, 0)])
    assert any("not finite" in f for f in fails)


# ------------------------------------------------------------------ the six cross terms
def split3(x):
    """x = x0 + x1 + x2, each piece the bf16 nearest to what is left (gemm.hip)."""
    x0 = x.bfloat16().float()
    x1 = (x - x0).bfloat16().float()
    x2 = (x - x0 - x1).bfloat16().float()
    return x0, x1, x2


TERMS = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]     # smallest first


def emulate_x6(A, B, drop=None):
    """The loop documented at the top of csrc/gemm.hip on logical A [M, K],
    B [N, K]: per 16-k step the six cross terms, smallest first, each one
    product of 16 k added into the fp32 accumulator."""
    a, b = split3(A), split3(B)
    acc = torch.zeros(A.shape[0], B.shape[0])
    for k0 in range(0, A.shape[1], 16):
        for t in TERMS:
            if t != drop:
                acc = acc + a[t[0]][:, k0:k0 + 16] @ b[t[1]][:, k0:k0 + 16].T
    return acc


def _real_ab():
    c = next(x for x in R.REAL_NT["x6nt"] if x["name"] == "real-ragged")
    d = R.nt_data(c, 0, real=True)
    return d["A"], d["B"]


def test_cancellation_cases_see_every_cross_term():
    """The full emulation passes within_floor on every cancellation case and on
    the real data; with any one of the six terms removed it fails the case that
    term carries -- "a": a1 b0, a2 b0; "b": a0 b1, a0 b2; "ab": a1 b1 -- and it
    fails by a factor of at least 10 over what the rule allows.  a0 b0 sums to
    zero in all three by construction (that is what lets the small terms show),
    so its removal is the real data's to catch."""
    seen = {"a": [(1, 0), (2, 0)], "b": [(0, 1), (0, 2)], "ab": [(1, 1)], "real": [(0, 0)]}
    pieces = {}
    for kind in R.CANCEL_KINDS + ("real",):
        A, B = _real_ab() if kind == "real" else R.cancel_data(kind)
        r64 = A.double() @ B.double().T
        r32 = A @ B.T
        dev, floor, ok = R.within_floor(emulate_x6(A, B), r64, r32)
        allowed = 4.0 * floor + 4e-7 * float(r64.abs().max())
        print(f"{kind}: full emulation dev {dev:.3e} floor {floor:.3e} share {dev / allowed:.3f}")
        assert ok, kind
        for t in TERMS:
            d2, _, ok2 = R.within_floor(emulate_x6(A, B, drop=t), r64, r32)
            print(f"{kind}: without a{t[0]} b{t[1]}: {d2 / allowed:.1f} x the allowance")
            if t in seen[kind]:
                assert not ok2 and d2 > 10 * allowed, (kind, t)
        if kind != "real":
            a, b = split3(A), split3(B)
            pieces[kind] = [float(t.abs().max()) for t in a + b]
            # the premise: x0 is the integer part and a0 b0 cancels exactly
            assert _is_int(a[0]) and _is_int(b[0]) and float((a[0].double() @ b[0].double().T).abs().max()) == 0
            assert torch.equal((a[0].double() + a[1].double() + a[2].double()).float(), A)
    # pieces: a0 a1 a2 b0 b1 b2
    assert pieces["a"][4] == 0 and pieces["a"][5] == 0 and pieces["a"][1] > 0 and pieces["a"][2] > 0
    assert pieces["b"][1] == 0 and pieces["b"][2] == 0 and pieces["b"][4] > 0 and pieces["b"][5] > 0
    assert pieces["ab"][1] > 0 and pieces["ab"][2] == 0 and pieces["ab"][4] > 0 and pieces["ab"][5] == 0
    assert {t for v in seen.values() for t in v} == set(TERMS)


def test_reverted_guards_fail_named_cases(fake, monkeypatch):
    """What the issue asks to try once, on the CPU reading of the contract: a
    loader without its K-tail predicate (reads one k past K), the bias split
    compared with <= instead of <, beta C read when beta == 0.  Each fails a
    named case of the tables."""
    real_nt = fake.T._nt

    def k_tail(a, b, C, ldc, strideC, bias, ns, M, N, K, S, kc):
        a2 = torch.as_strided(a, (M, K + 1), a.stride(), a.storage_offset())
        b2 = torch.as_strided(b, (N, K + 1), b.stride(), b.storage_offset()) if b.stride(1) == 1 else \
            torch.cat([b, torch.ones(N, 1)], 1)
        real_nt(a2, b2, C, ldc, strideC, bias, ns, M, N, K + 1, S, kc + 1 if S == 1 else kc)
    monkeypatch.setattr(fake.T, "_nt", k_tail)
    c = next(x for x in R.NT_CASES["bf16nt"] if x["name"] == "K56")
    assert any("not finite" in f for f in W.run_int(fake, [(c, 0)]))
    monkeypatch.setattr(fake.T, "_nt", real_nt)

    def bias_le(bias, nsplit, N, dtype=torch.float64):     # n <= bias_nsplit takes the first segment
        v = torch.zeros(N, dtype=dtype)
        a1, a2, b1, b2 = bias
        for n in range(N):
            lo = n <= nsplit
            for t in ((a1, a2) if lo else (b1, b2)):
                if t is not None:
                    i = n if lo else n - nsplit
                    v[n] += float(t[i]) if i < t.numel() else float("nan")
        return v
    true_bias = R.bias_vec
    c = next(x for x in R.NT_CASES["bf16nt"] if x["name"] == "bias-ns127")
    ref = R.nt_ref_of(c, 0)                # the reference keeps the true rule
    monkeypatch.setattr(R, "bias_vec", bias_le)
    fails = W.run_int(fake, [(c, 0)])
    monkeypatch.setattr(R, "bias_vec", true_bias)
    assert torch.equal(ref, R.nt_ref_of(c, 0))
    assert fails and "(0, 0, 127)" in fails[0], fails[:2]

    real_gemm = fake.T.gemm

    def reads_c(M, N, K, alpha, A, sam, sak, sA, B, sbk, sbn, sB, beta, *rest):
        real_gemm(M, N, K, alpha, A, sam, sak, sA, B, sbk, sbn, sB, 1e-30 if beta == 0 else beta, *rest)
    monkeypatch.setattr(fake.T, "gemm", reads_c)
    c = next(x for x in R.F32_CASES if x["name"] == "M129")
    assert any("not finite" in f for f in W.run_int(fake, [(dict(c, sk=False), 0)]))


# ------------------------------------------------------------------ refusals
class _Bf16Problem(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int64), ("B", ctypes.c_void_p),
                ("ldb", ctypes.c_int64), ("C", ctypes.c_void_p), ("ldc", ctypes.c_int64),
                ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64),
                ("nsplit", ctypes.c_int), ("kc", ctypes.c_int64), ("strideC", ctypes.c_int64),
                ("a_kmajor", ctypes.c_int), ("b_kmajor", ctypes.c_int)]


class _X6Problem(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("A2", ctypes.c_void_p), ("lda", ctypes.c_int64),
                ("a_ksplit", ctypes.c_int64), ("a_kmajor", ctypes.c_int),
                ("B", ctypes.c_void_p), ("B2", ctypes.c_void_p), ("ldb", ctypes.c_int64),
                ("b_nsplit", ctypes.c_int64), ("b_ksplit", ctypes.c_int64), ("b_kmajor", ctypes.c_int),
                ("C", ctypes.c_void_p), ("C2", ctypes.c_void_p), ("ldc", ctypes.c_int64),
                ("c_msplit", ctypes.c_int64),
                ("bias_a1", ctypes.c_void_p), ("bias_a2", ctypes.c_void_p),
                ("bias_b1", ctypes.c_void_p), ("bias_b2", ctypes.c_void_p),
                ("bias_nsplit", ctypes.c_int64), ("M", ctypes.c_int64), ("N", ctypes.c_int64),
                ("K", ctypes.c_int64), ("nsplit", ctypes.c_int), ("kc", ctypes.c_int64),
                ("strideC", ctypes.c_int64)]


PTR = 1 << 20        # never dereferenced: every call below is refused before a launch


def _refused(lib, rc, text):
    msg = lib.ainp_last_error().decode()
    assert rc == -1 and text in msg, (rc, msg)


def test_launcher_refusals_on_the_host():
    """The refused cases of the tables and of the issue, against the launchers'
    own checks: AINP_EINVAL with a message, before anything is launched."""
    from ainp import _lib
    lib = _lib.lib
    PP = ctypes.c_void_p * 9
    ptrs = PP(*([PTR] * 9))

    def f32(nptr=1, flags=0, ksplit=0, sam=40, sak=1):
        return lib.ainp_gemm_f32_ex(129, 127, 36, 1.0, ptrs, sam, sak, 0, ptrs, 131, 1, 0, 0.0, ptrs,
                                    130, 1, 0, None, None, nptr, 1, ksplit, flags, None, 0, None)
    _refused(lib, f32(nptr=9), "bad argument")
    _refused(lib, f32(flags=R.EXACT_F32 | R.BF16), "exclusive")
    _refused(lib, f32(flags=4), "unknown flags")
    _refused(lib, f32(ksplit=3), "ksplit")
    _refused(lib, f32(sam=40, sak=2), "unit stride")
    for c in _all_nt():
        if not c["refused"] or len(c["probs"]) > 3:
            continue
        p = c["probs"][0]
        M, N, K, S, kc = p["M"], p["N"], p["K"], p["nsplit"], p["kc"]
        big = 1 << 40
        if c["entry"] == "bf16nt":
            rc = lib.ainp_gemm_bf16nt(M, N, K, PTR, K + 8, PTR, K + 8, PTR, N, None, None, None, None, 0,
                                      S, kc, big, None)
        elif c["entry"] == "x6nt":
            rc = lib.ainp_gemm_x6nt_256(M, N, K, PTR, K, PTR, PTR, K, 256, PTR, N, None, None, None,
                                        None, 0, S, kc, big, None)
        elif c["entry"] == "bf16multi":
            pr = _Bf16Problem(PTR, K + 8, PTR, K + 8, PTR, N, M, N, K, S, kc, big, 0, 0)
            rc = lib.ainp_gemm_bf16nt_multi(ctypes.byref(pr), 1, None)
        else:
            pr = _X6Problem(PTR, PTR if p["a_ksplit"] else None, max(K, M) + 4, p["a_ksplit"],
                            int(p["akm"]), PTR, None, K + 4, 0, 0, 0, PTR, None, N, 0, None, None, None,
                            None, 0, M, N, K, S, kc, big)
            rc = lib.ainp_gemm_x6_multi(ctypes.byref(pr), 1, None)
        _refused(lib, rc, c["refused"])
    pr4 = (_Bf16Problem * 4)()
    _refused(lib, lib.ainp_gemm_bf16nt_multi(pr4, 4, None), "1..3 problems")
    x4 = (_X6Problem * 4)()
    _refused(lib, lib.ainp_gemm_x6_multi(x4, 4, None), "1..3 problems")
    # a k-major A2 takes the same M rows of lda floats as A: lda < M is refused
    pr = _X6Problem(PTR, PTR, 256, 16, 1, PTR, None, 52, 0, 0, 0, PTR, None, 300, 0, None, None, None,
                    None, 0, 260, 300, 48, 1, 48, 0)
    _refused(lib, lib.ainp_gemm_x6_multi(ctypes.byref(pr), 1, None), "bad problem")
    # split-K with C2: a slab stride that holds C's 256 rows but not C2's 512 would
    # let C2's slabs overlap
    pr = _X6Problem(PTR, None, 36, 0, 0, PTR, None, 36, 0, 0, 0, PTR, PTR, 300, 256, None, None, None,
                    None, 0, 768, 300, 32, 2, 16, 256 * 300)
    _refused(lib, lib.ainp_gemm_x6_multi(ctypes.byref(pr), 1, None), "slab stride")


# ------------------------------------------------------------------ routes
@pytest.fixture(scope="module")
def route_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route") / "gemm_route_names"
    src = R.os.path.join(R.ROOT, "tests", "gemm_route_names.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), src], check=True)

    def run(lines):
        text = "".join(" ".join(str(int(v)) for v in ln) + "\n" for ln in lines)
        out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True)
        rows = [ln.split() for ln in out.stdout.splitlines()]
        assert len(rows) == len(lines)
        return [(int(r[0]), r[1], int(r[2])) for r in rows]
    return run


def test_streamk_eligibility_is_the_documented_one():
    from ainp import _lib
    q = _lib.lib.ainp_gemm_f32_workspace
    for c in _all_f32() + R.REAL_F32 + R.CANCEL_F32:
        need = int(q(c["M"], c["N"], c["K"], c["nptr"], c["nstrided"], c["ksplit"]))
        nb = c["nptr"] * c["nstrided"]
        assert (need > 0) == c["sk"] == R.f32_streamk(c["M"], c["N"], c["K"], nb, c["ksplit"]), c["name"]
    sk = [c for c in R.SK_CASES if c["sk"]]
    tiles = lambda c: (R.cdiv(c["M"], 128), R.cdiv(c["N"], 128))  # noqa: E731
    assert {tiles(c)[1] <= tiles(c)[0] for c in sk} == {True, False}        # both tile orders
    assert {c["ws"] for c in sk} == {"given", "none", "short"}
    assert any(c["nptr"] == 2 and c["share_a"] for c in sk) and any(c["c_col"] and c["bias"] for c in sk)
    assert all(c["K"] % 32 and c["M"] % 128 and c["N"] % 128 for c in sk)
    # one step outside each rule
    assert q(2043, 1533, 2047, 1, 1, 0) == 0 and q(2043, 1533, 2048, 1, 1, 0) > 0
    assert q(2043, 1533 - 128, 2100, 1, 1, 0) == 0                          # 176 tiles
    assert q(2043, 1533, 2100, 1, 1, 1) == 0 and q(2043, 1533, 2100, 1, 2, 2) == 0


def test_vector_load_preconditions_break_one_at_a_time():
    """vec*-all takes 16-byte loads of both operands; every other vec* case loses
    them for exactly the operand its name says, by exactly one precondition."""
    by = {c["name"]: c for c in R.F32_CASES}
    for t in ("vec0", "vec1"):
        assert R.f32_vec(by[f"{t}-all"]) == (True, True)
        a_only = ["lda", "offA", "strideA", "lastA"] + (["extK"] if t == "vec0" else ["extM"])
        b_only = ["ldb", "offB", "strideB", "lastB"] + (["extN"] if t == "vec0" else ["extK"])
        for n in a_only:
            assert R.f32_vec(by[f"{t}-{n}"]) == (False, True), (t, n)
        for n in b_only:
            assert R.f32_vec(by[f"{t}-{n}"]) == (True, False), (t, n)
        for n in ("extM", "extN", "extK"):
            c = by[f"{t}-{n}"]
            _, _, lda, _, _, ldb, _, _, _ = R.f32_strides(c)
            assert lda % 4 == 0 and ldb % 4 == 0
        for n in ("lda", "ldb"):
            c = by[f"{t}-{n}"]
            assert c["M"] % 4 == 0 and c["N"] % 4 == 0 and c["K"] % 4 == 0
    # the launcher's own expression is the documented one
    src = open(R.os.path.join(R.CSRC, "gemm.hip")).read()
    assert "bool avec = (lda % 4 == 0) && ((akc ? K : M) % 4 == 0) && (strideA % 4 == 0);" in src
    assert "bool bvec = (ldb % 4 == 0) && ((bkc ? K : N) % 4 == 0) && (strideB % 4 == 0);" in src
    assert "avec = avec && aligned16(A[i]);" in src and "bvec = bvec && aligned16(B[i]);" in src


def test_case_tables_reach_every_kernel(route_host):
    """Every kernel of the family, the two copy kernels and both sides of every
    switch are reached by an integer case that is served; each case's route is
    asserted, so a routing change cannot silently empty a route's coverage."""
    reached = {}

    def tiles_for(env, cases):
        lines = [(R.env_bits(env), p["M"], p["N"], p["K"], p["nsplit"], p["kc"], 64)
                 for p in (c["probs"][0] for c in cases)]
        return dict(zip([c["name"] for c in cases], route_host(lines)))

    settings = [None] + list(R.CHILD_SETTINGS)
    for setting in settings:
        env = R.env_of(setting)
        specs = R.SPECS if setting is None else [s for s in R.CHILD_SETTINGS[setting][3] if ":" not in s
                                                 or s.startswith("f32:")]
        b16 = [c for c in R.NT_CASES["bf16nt"]]
        tiles = tiles_for(env, b16)
        for spec in specs:
            for c, flags in R.int_cases(spec):
                if W.refusal(c):
                    if c["entry"] == "bf16nt":
                        assert tiles[c["name"]][2] == 0, c["name"]          # splitk_covers refuses
                    continue
                if c["entry"] == "bf16nt":
                    assert tiles[c["name"]][2] == 1, c["name"]
                names = R.route(c, flags, env, lambda *a, n=c["name"]: tiles[n][0])
                if c["entry"] == "bf16nt":
                    assert names[0] == tiles[c["name"]][1], c["name"]
                    if c["tile"] is not None:
                        want = c["tile"] if env["gemm16_256"] else 0
                        want = 1 if (want == 2 and not env["g256_bk64"]) else want
                        assert tiles[c["name"]][0] == want, (setting, c["name"])
                    elif setting is None:
                        assert tiles[c["name"]][0] == 0, c["name"]
                for n in names:
                    reached.setdefault((setting, n), []).append(W.tag_of(c, flags))
    default = {n for s, n in reached if s is None}
    # the default environment reaches all but what the switches are for
    assert default == set(R.KERNELS + ["order:m-first", "order:n-first"]) - {
        "gemm_f32_kernel<B16K64>", "gemm_x6nt_256_kernel", "gemm_x6r_kernel<noapf>"}
    assert len(R.KERNELS) == 17          # 13 GEMM kernels (two of them in two depths) + 2 copies
    per = {s: {n for t, n in reached if t == s} for s in R.CHILD_SETTINGS}
    assert per["b16_kt64"] == {"gemm_f32_kernel<B16K64>"}
    assert per["g256_bk64_0"] == {"gemm_bf16nt_kernel", "gemm_bf16nt_256_kernel",
                                  "gemm_bf16nt_256_multi_kernel<b32>"}
    assert per["gemm16_256_0"] == {"gemm_bf16nt_kernel"}
    assert per["x6_splitpass_0"] == {"gemm_x6nt_256_kernel"}
    assert per["x6r_mfast_0"] == {"gemm_x6r_kernel<apf>", "order:n-first"}
    assert per["x6r_apf_0"] == {"gemm_x6r_kernel<noapf>", "order:m-first", "order:n-first"}
    # named cases on named routes
    for tag, name in (("f32:exact/sk-order0", "gemm_f32_streamk"),
                      ("f32:exact/sk-order0-nows", "gemm_f32_kernel<F32>"),
                      ("f32:exact/sk-order0-short", "gemm_f32_kernel<F32>"),
                      ("bf16nt/tall-b64-s3", "gemm_bf16nt_256b_kernel"),
                      ("bf16nt/tall-b32-s3", "gemm_bf16nt_256_kernel"),
                      ("bf16nt/split-not-tall", "gemm_bf16nt_kernel"),
                      ("bf16multi/three-b64", "gemm_bf16nt_256_multi_kernel<b64>"),
                      ("bf16multi/tiny-beside-large-mixedK", "gemm_bf16nt_256_multi_kernel<b32>"),
                      ("bf16multi/split-partial", "gemm_bf16nt_256_multi_kernel<b32>"),
                      ("x6multi/order-2x8", "order:m-first"), ("x6multi/order-3x8", "order:n-first"),
                      ("x6multi/order-2x7", "order:n-first"), ("x6multi/order-8x8", "order:m-first")):
        assert tag in reached[None, name], (tag, name)
    order = {t for t in reached[None, "order:m-first"]}
    assert {"x6multi/order-2x8", "x6multi/order-4x9", "x6multi/order-8x8"} <= order
    # the restated dispatch is the launchers': the lines it restates are there
    g = open(R.os.path.join(R.CSRC, "gemm.hip")).read()
    g16 = open(R.os.path.join(R.CSRC, "gemm16.hip")).read()
    x6r = open(R.os.path.join(R.CSRC, "gemm_x6r.hip")).read()
    assert "if (pm == PM_B16 && gemm_env().b16_kt64)" in g
    assert "const bool sk = !use_x6 && g.P && workspace &&" in g
    assert re.search(r"if \(K < 64 \* BK \|\| tiles < SK_SLOTS / 4\) return g;", g)
    assert "if (tiles * 10 >= waves * SK_SLOTS * 9) return g;" in g and "SK_SLOTS = 768" in g
    assert "job.bk64 = gemm_env().g256_bk64 ? 1 : 0;" in g16
    assert "if (job.p[q].K % g256::b64::BK || job.p[q].kc % g256::b64::BK) job.bk64 = 0;" in g16
    assert "if (gemm_env().x6_splitpass)" in g16
    assert "d.mfast = (gemm_env().x6r_mfast && (d.tiles_m == 2 || d.tiles_m == 4 || d.tiles_m == 8) &&" in x6r
    assert "d.tiles_n >= 8) ? 1 : 0;" in x6r and "if (gemm_env().x6r_apf)" in x6r
    # the real and cancellation cases sit on the routes their names say
    env = R.env_of()
    tiles = tiles_for(env, R.REAL_NT["bf16nt"])
    for c in R.REAL_NT["bf16nt"]:
        if c["tile"] is not None:
            assert tiles[c["name"]][0] == c["tile"], c["name"]
    assert R.route(R.REAL_NT["bf16multi"][0], 0, env)[0].endswith("<b64>")
    assert R.route(R.REAL_NT["bf16multi"][1], 0, env)[0].endswith("<b32>")
    assert R.route(R.REAL_F32[2], R.EXACT_F32, env) == ["gemm_f32_streamk", "gemm_streamk_fixup"]
