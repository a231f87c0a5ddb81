"""Plain torch restatement of the GEMM family's ABI (include/ainp.h:
ainp_gemm_f32_ex, ainp_gemm_bf16nt, ainp_gemm_bf16nt_multi, ainp_gemm_x6nt_256,
ainp_gemm_x6_multi, ainp_cast_bf16_t, ainp_transpose_f32 over csrc/gemm.hip,
csrc/gemm16.hip, csrc/gemm_x6r.hip and csrc/gemm_route.h), for the tests only,
written from the header's text and in whatever dtype it is asked for: float64
for the reference proper, float32 for the rounding floor the GPU tests measure
against it (gan_glue_ref.within_floor).

  f32_ref:  C = alpha op(A) op(B) + beta C + bias1 + bias2 over pointer x strided
            batches, ksplit 0 / 1 / 2, flags 0 / EXACT_F32 / BF16
  nt_ref:   C[s] = A[:, chunk s] B[:, chunk s]^T (+ the two-segment bias in slab 0),
            the contract of the four "nt" entries on logical A [M, K], B [N, K];
            where B1 / B2, A2, C2 and k-major operands lie in memory is the
            launcher's business (tests/gemm_edge_worker.py builds them)

The same module holds the case tables, the input builders, the guarded buffer
layout and the kernel every case reaches (a restatement of the launchers'
dispatch; tests/test_cpu_gemm_ref.py pins it to the sources and to the host
queries), so tests/test_cpu_gemm_ref.py (no GPU) and
tests/test_gpu_gemm_edges.py / tests/gemm_edge_worker.py walk one table.  The
builders are cached: a case is built once and shared, and nobody writes into
what they return.
"""
import functools
import os
import zlib

import torch

from gan_glue_ref import within_floor  # noqa: F401  (the GPU tests' element-wise rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-audio-inpainting_amd", "csrc")

EXACT_F32, BF16 = 1, 2          # include/ainp.h AINP_GEMM_*
FLAGS = {"x6": 0, "exact": EXACT_F32, "bf16": BF16}
TWO24 = 2.0 ** 24
NAN = float("nan")
A1, A2, B1, B2 = 1, 2, 4, 8     # bias mask of the nt entries: which of the four vectors is given


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


# ------------------------------------------------------------------ references
def f32_ref(c, d, flags, dtype=torch.float64):
    """ainp_gemm_f32_ex on the logical operands of f32_data -> list of C [M, N]:
    one per batch (ksplit 0), C[0] alone (1), one per pointer batch (2).  Batch
    b = pointer entry b % nptr, strided slab b // nptr."""
    cast = (lambda t: t.bfloat16().to(dtype)) if flags & BF16 else (lambda t: t.to(dtype))
    nptr, ns = c["nptr"], c["nstrided"]
    prod = [cast(a) @ cast(b) for a, b in zip(d["A"], d["B"])]
    if c["ksplit"] == 0:
        acc = prod
    elif c["ksplit"] == 1:
        acc = [sum(prod[1:], prod[0])]
    else:
        acc = [sum((prod[p + s * nptr] for s in range(1, ns)), prod[p]) for p in range(nptr)]
    out = []
    for i, t in enumerate(acc):
        p = i % nptr
        r = c["alpha"] * t
        if c["bias"] & 1:
            r = r + d["b1"][p].to(dtype)
        if c["bias"] & 2:
            r = r + d["b2"][p].to(dtype)
        if c["beta"] != 0:
            r = r + c["beta"] * d["C0"][i].to(dtype)
        out.append(r)
    return out


def f32_bound(c, d):
    """max over the outputs of |alpha| sum |a||b| + |bias1| + |bias2| + |beta C|."""
    ab = dict(c, alpha=abs(c["alpha"]), beta=abs(c["beta"]))
    dd = {k: [t.abs() for t in v] for k, v in d.items()}
    return max(float(t.max()) for t in f32_ref(ab, dd, 0))


def bias_vec(bias, nsplit, N, dtype=torch.float64):
    """(a1 + a2)[n] for n < nsplit, (b1 + b2)[n - nsplit] after; None = 0."""
    v = torch.zeros(N, dtype=dtype)
    a1, a2, b1, b2 = bias
    for t in (a1, a2):
        if t is not None:
            v[:nsplit] += t.to(dtype)
    for t in (b1, b2):
        if t is not None:
            v[nsplit:] += t.to(dtype)
    return v


def nt_ref(p, d, bf16, dtype=torch.float64):
    """sum_k A[m][k] B[n][k] + bias(n) -> slabs [nsplit, M, N]: split s sums k in
    [s kc, min(K, (s + 1) kc)), the bias in slab 0 only."""
    cast = (lambda t: t.bfloat16().to(dtype)) if bf16 else (lambda t: t.to(dtype))
    a, b = cast(d["A"]), cast(d["B"])
    K, S = p["K"], p["nsplit"]
    out = []
    for s in range(S):
        k0, k1 = (0, K) if S == 1 else (s * p["kc"], min(K, (s + 1) * p["kc"]))
        t = a[:, k0:k1] @ b[:, k0:k1].T
        if s == 0:
            t = t + bias_vec(d["bias"], p["bias_nsplit"], p["N"], dtype)
        out.append(t)
    return torch.stack(out)


def nt_bound(p, d):
    dd = dict(A=d["A"].abs(), B=d["B"].abs(), bias=[None if t is None else t.abs() for t in d["bias"]])
    return float(nt_ref(dict(p, nsplit=1), dd, False).max())


# ------------------------------------------------------------------ guarded buffers
def guarded(t, strides=None, off=0, device="cpu", fill=NAN):
    """t in the memory layout an entry point is given: a view with element
    `strides` (default: contiguous) into a larger buffer filled with `fill`,
    with a guard of at least the largest stride (one row, one slab) before and
    after it, a multiple of 8 elements so the view keeps the buffer's 16-byte
    alignment unless `off` elements shift it.  -> (buffer, view)."""
    shape = tuple(t.shape)
    if strides is None:
        strides = tuple(torch.empty(shape).stride())
    strides = tuple(int(s) for s in strides)
    span = 1 + sum((n - 1) * s for n, s in zip(shape, strides)) if t.numel() else 0
    G = -(-max(strides + (64,)) // 8) * 8
    buf = torch.full((G + off + span + G,), fill, dtype=t.dtype, device=device)
    view = buf.as_strided(shape, strides, G + off)
    view.copy_(t)
    return buf, view


def inside_mask(buf, view):
    """Which elements of buf the view covers."""
    m = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    m.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
    return m


# ------------------------------------------------------------------ ainp_gemm_f32_ex
def f32_case(name, M=129, N=127, K=36, **kw):
    """ta / tb: op(A) is stored m-contiguous ([K][lda]) / op(B) k-contiguous
    ([N][ldb]); c_col: C column-major.  pad_a / pad_b: ld beyond the contiguous extent
    rounded up to 4 (so ld % 4 == 0 whatever the extent, unless the pad breaks it); off_*: the
    base pointer shifted by that many floats (off_last: of the last pointer batch
    only); sa_extra / sb_extra: strideA / strideB beyond rows * ld; bias: bit 0
    bias1, bit 1 bias2; ws: the stream-K workspace "given", "none" or "short"."""
    c = dict(entry="f32", name=name, M=M, N=N, K=K, ta=False, tb=False, c_col=False, nptr=1,
             nstrided=1, ksplit=0, alpha=1.0, beta=0.0, bias=0, pad_a=4, pad_b=4, pad_c=3, off_a=0,
             off_b=0, off_last=False, sa_extra=8, sb_extra=8, share_a=False, ws="given", sk=False,
             only=None)
    c.update(kw)
    return c


AB = [(1.0, 0.0), (-1.0, 1.0), (2.0, 0.5), (0.5, -1.0), (0.0, 2.0)]
EDGE_MN = (1, 127, 128, 129, 257)
EDGE_K = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100)


def _f32_cases():
    cs = []
    # one dimension across its edges, the others ragged; K = 36: 16-byte rows, no whole K-tile
    cs += [f32_case(f"M{v}", M=v) for v in EDGE_MN]
    cs += [f32_case(f"N{v}", N=v, tb=True) for v in EDGE_MN]
    cs += [f32_case(f"K{v}", K=v, tb=True) for v in EDGE_K]
    cs += [f32_case("K0-beta-bias", K=0, alpha=2.0, beta=0.5, bias=3),
           f32_case("K0-batched", K=0, nptr=2, nstrided=3, beta=-1.0, bias=1)]
    # the XCD / group-of-8 remap: a short last group, grids that are no multiple of 8
    cs += [f32_case(f"tiles{tm}x{tn}", M=128 * tm - 7, N=128 * tn - 3, K=16, tb=True)
           for tn in (8, 9, 17) for tm in (1, 3)]
    # the four operand layouts, C row- and column-major (with the full epilogue)
    cs += [f32_case(f"lay-{int(ta)}{int(tb)}-{'col' if cc else 'row'}", ta=ta, tb=tb, c_col=cc,
                    alpha=2.0 if cc else 1.0, beta=0.5 if cc else 0.0, bias=3 if cc else 0, K=33)
           for ta in (False, True) for tb in (False, True) for cc in (False, True)]
    # each vector-load precondition broken on its own: every extent of the base
    # shape is a multiple of 4, in (ta, tb) = (0, 0) [A k-, B n-contiguous] and (1, 1)
    for ta in (False, True):
        base = dict(M=132, N=124, K=36, ta=ta, tb=ta)
        tag = f"vec{int(ta)}"
        cs += [f32_case(f"{tag}-all", **base),
               f32_case(f"{tag}-extK", **dict(base, K=34)), f32_case(f"{tag}-extM", **dict(base, M=130)),
               f32_case(f"{tag}-extN", **dict(base, N=126)),
               f32_case(f"{tag}-lda", pad_a=5, **base), f32_case(f"{tag}-ldb", pad_b=5, **base),
               f32_case(f"{tag}-offA", off_a=1, **base), f32_case(f"{tag}-offB", off_b=1, **base),
               f32_case(f"{tag}-strideA", nstrided=3, sa_extra=10, **base),
               f32_case(f"{tag}-strideB", nstrided=3, sb_extra=10, **base),
               f32_case(f"{tag}-lastA", nptr=3, off_a=1, off_last=True, **base),
               f32_case(f"{tag}-lastB", nptr=3, off_b=1, off_last=True, **base)]
    # batches
    cs += [f32_case("nptr2", nptr=2, bias=1), f32_case("nptr8", nptr=8, bias=2),
           f32_case("nstrided3", nstrided=3, bias=3), f32_case("nptr2x3", nptr=2, nstrided=3, bias=3)]
    # K-concatenation: K = 40 leaves a partial last tile at every K-tile depth (16, 32, 64)
    cs += [f32_case("ksplit1", K=40, nptr=2, nstrided=3, ksplit=1, bias=3, alpha=2.0, beta=0.5),
           f32_case("ksplit2", K=40, nptr=2, nstrided=3, ksplit=2, bias=3, alpha=-1.0, beta=1.0),
           f32_case("ksplit1-K17", K=17, nptr=3, ksplit=1, ta=True),
           f32_case("ksplit2-K100", K=100, nptr=2, nstrided=2, ksplit=2, tb=True)]
    # the epilogue: alpha, beta (beta == 0 reads no C: it is NaN), the two biases
    cs += [f32_case(f"ep-a{a}-b{b}-bias{bi}", alpha=a, beta=b, bias=bi)
           for a, b in AB for bi in range(4)]
    return cs


def _sk_cases():
    """Stream-K (exact loop): the smallest eligible grids, ragged, K % 32 != 0."""
    big = dict(K=2100, tb=True, sk=True, only="exact")
    cs = [f32_case("sk-order0", M=16 * 128 - 5, N=12 * 128 - 3, **big),
          f32_case("sk-order0-nows", M=16 * 128 - 5, N=12 * 128 - 3, ws="none", **big),
          f32_case("sk-order0-short", M=16 * 128 - 5, N=12 * 128 - 3, ws="short", **big),
          f32_case("sk-order1-col", M=12 * 128 - 3, N=16 * 128 - 5, c_col=True, alpha=2.0, beta=0.5,
                   bias=3, **big),
          f32_case("sk-2ptr-shareA", M=10 * 128 - 5, N=10 * 128 - 1, nptr=2, share_a=True, bias=1,
                   alpha=-1.0, beta=1.0, **big),
          # not stream-K: K one short of 2048; a last wave 90 % full (696 one-element tiles)
          f32_case("sk-not-K2047", M=16 * 128 - 5, N=12 * 128 - 3, K=2047, tb=True, only="exact"),
          f32_case("sk-not-full", M=1, N=1, K=2048, nptr=8, nstrided=87, tb=True, only="exact")]
    return cs


F32_CASES = _f32_cases()
SK_CASES = _sk_cases()


def _f32_key(c):
    return (c["name"], c["M"], c["N"], c["K"], c["nptr"], c["nstrided"], c["ksplit"], c["share_a"])


@functools.lru_cache(maxsize=None)
def _f32_data(key, real):
    name, M, N, K, nptr, ns, ksplit, share = key
    g = _gen(name.replace("-nows", "").replace("-short", ""))
    nb = nptr * ns
    if real:     # activations of O(1) against weights of O(0.05), as in the model
        mk_a = lambda: torch.tanh(torch.randn(M, K, generator=g))  # noqa: E731
        mk_b = lambda: torch.randn(K, N, generator=g) * 0.05  # noqa: E731
        mk_c = lambda: torch.randn(M, N, generator=g)  # noqa: E731
        mk_v = lambda: torch.randn(N, generator=g) * 0.1  # noqa: E731
    else:
        mk_a, mk_b = (lambda: ints(g, (M, K))), (lambda: ints(g, (K, N)))
        mk_c, mk_v = (lambda: ints(g, (M, N), -50, 50)), (lambda: ints(g, (N,), -50, 50))
    A = [mk_a() for _ in range(nb)]
    if share:
        A = [A[0]] * nb
    nC = nb if ksplit == 0 else (1 if ksplit == 1 else nptr)
    return dict(A=A, B=[mk_b() for _ in range(nb)], C0=[mk_c() for _ in range(nC)],
                b1=[mk_v() for _ in range(nptr)], b2=[mk_v() for _ in range(nptr)])


def f32_data(c, real=False):
    if c["name"].startswith("cancel-"):
        A, B = cancel_data(c["name"][7:])
        z = torch.zeros(c["N"])
        return dict(A=[A], B=[B.T.contiguous()], C0=[torch.zeros(c["M"], c["N"])], b1=[z], b2=[z])
    return _f32_data(_f32_key(c), real)


@functools.lru_cache(maxsize=None)
def _f32_ref_cached(key, flags, real, f32, frozen):
    c = dict(frozen)
    return f32_ref(c, _f32_data(key, real), flags, torch.float32 if f32 else torch.float64)


def f32_ref_of(c, flags, real=False, f32=False):
    """The cached reference of a table case (bf16 rounding is the identity on the
    integer data, so the three flags share one evaluation)."""
    if c["name"].startswith("cancel-"):
        return f32_ref(c, f32_data(c), 0, torch.float32 if f32 else torch.float64)
    frozen = tuple((k, c[k]) for k in ("nptr", "nstrided", "ksplit", "alpha", "beta", "bias"))
    return _f32_ref_cached(_f32_key(c), flags if real else 0, real, f32, frozen)


def f32_strides(c):
    """sam, sak, lda, sbk, sbn, ldb, scm, scn, ldc of a case."""
    up4 = lambda n: -(-n // 4) * 4  # noqa: E731
    lda = up4(c["M"] if c["ta"] else c["K"]) + c["pad_a"]
    ldb = up4(c["K"] if c["tb"] else c["N"]) + c["pad_b"]
    ldc = (c["M"] if c["c_col"] else c["N"]) + c["pad_c"]
    sam, sak = (1, lda) if c["ta"] else (lda, 1)
    sbk, sbn = (1, ldb) if c["tb"] else (ldb, 1)
    scm, scn = (1, ldc) if c["c_col"] else (ldc, 1)
    return sam, sak, lda, sbk, sbn, ldb, scm, scn, ldc


def f32_vec(c):
    """(avec, bvec): whether ainp_gemm_f32_ex may take 16-byte loads of A / B --
    its documented precondition, restated (16-byte rows, extent % 4 == 0, batch
    stride % 4 == 0, every base pointer aligned)."""
    _, _, lda, _, _, ldb, _, _, _ = f32_strides(c)
    ea, eb = (c["M"] if c["ta"] else c["K"]), (c["K"] if c["tb"] else c["N"])
    ra, rb = (c["K"] if c["ta"] else c["M"]), (c["N"] if c["tb"] else c["K"])
    av = lda % 4 == 0 and ea % 4 == 0 and (ra * lda + c["sa_extra"]) % 4 == 0 and c["off_a"] % 4 == 0
    bv = ldb % 4 == 0 and eb % 4 == 0 and (rb * ldb + c["sb_extra"]) % 4 == 0 and c["off_b"] % 4 == 0
    return av, bv


# ------------------------------------------------------------------ the nt entries
def nt(M, N, K, **kw):
    """One problem of an nt entry.  bias: mask of A1 | A2 | B1 | B2; bsplit
    (x6nt): rows of B1; a_ksplit / b_ksplit / b_nsplit / c_msplit (x6multi): 0 =
    no A2 / B2 / C2; akm / bkm: the operand k-major."""
    p = dict(M=M, N=N, K=K, pad_a=8, pad_b=16, pad_c=5, bias=0, bias_nsplit=0, nsplit=1, kc=0,
             bsplit=None, a_ksplit=0, b_ksplit=0, b_nsplit=0, c_msplit=0, akm=False, bkm=False)
    p.update(kw)
    if p["nsplit"] == 1:
        p["kc"] = K
    if p["bsplit"] is None:
        p["bsplit"] = N
    return p


def case(entry, name, *probs, **kw):
    return dict(entry=entry, name=name, probs=list(probs), tile=kw.get("tile"), refused=kw.get("refused"))


ALLB = A1 | A2 | B1 | B2


def _bf16nt_cases():
    cs = [case("bf16nt", f"M{v}", nt(v, 127, 72)) for v in EDGE_MN]
    cs += [case("bf16nt", f"N{v}", nt(129, v, 72)) for v in EDGE_MN]
    cs += [case("bf16nt", f"K{v}", nt(129, 127, v)) for v in (8, 56, 64, 72, 136)]
    cs += [case("bf16nt", f"bias-ns{v}", nt(129, 257, 72, bias=ALLB, bias_nsplit=v))
           for v in (0, 1, 127, 128, 256, 257)]
    cs += [case("bf16nt", f"bias-mask{m}", nt(129, 257, 72, bias=m, bias_nsplit=128))
           for m in (ALLB & ~A1, ALLB & ~A2, ALLB & ~B1, ALLB & ~B2, A1, B2)]
    cs += [case("bf16nt", "split-partial", nt(129, 127, 136, nsplit=3, kc=64, bias=ALLB, bias_nsplit=1)),
           case("bf16nt", "split-per-tile", nt(257, 129, 192, nsplit=3, kc=64, bias=A1 | B1,
                                               bias_nsplit=128)),
           case("bf16nt", "split-2of3", nt(129, 127, 136, nsplit=2, kc=64), refused="split-K"),
           case("bf16nt", "split-kc32", nt(129, 127, 136, nsplit=5, kc=32), refused="split-K")]
    return cs


def _g256_cases():
    """Routed to the 256 x 256 tiles only for M, N >= 512: tile 1 the 32-deep
    ring (K % 64 != 0), tile 2 the 64-deep one."""
    cs = []
    for K, tile in ((96, 1), (128, 2)):
        cs += [case("bf16nt", f"g256-M{v}-K{K}", nt(v, 767, K, bias=ALLB, bias_nsplit=256), tile=tile)
               for v in (512, 513, 767, 769)]
        cs += [case("bf16nt", f"g256-N{v}-K{K}", nt(513, v, K, bias=A1 | B2, bias_nsplit=512), tile=tile)
               for v in (512, 513, 769)]
    cs += [case("bf16nt", f"g256-K{K}", nt(513, 767, K), tile=1) for K in (32, 160)]
    cs += [case("bf16nt", f"g256-K{K}", nt(513, 767, K), tile=2) for K in (64, 192)]
    # the tall split route (M >= 8 N) on both tiles; chunks of 64 (g16's granule)
    cs += [case("bf16nt", "tall-b64-s3", nt(4096, 512, 192, nsplit=3, kc=64, bias=ALLB, bias_nsplit=256),
                tile=2),
           case("bf16nt", "tall-b64-s2", nt(4097, 512, 192, nsplit=2, kc=128), tile=2),
           case("bf16nt", "tall-b32-s3", nt(4096, 512, 160, nsplit=3, kc=64, bias=A2 | B1, bias_nsplit=511),
                tile=1),
           case("bf16nt", "tall-b32-s2", nt(4099, 513, 160, nsplit=2, kc=128), tile=0),   # M < 8 N
           case("bf16nt", "split-not-tall", nt(769, 513, 192, nsplit=3, kc=64), tile=0)]
    return cs


def _bf16multi_cases():
    e = "bf16multi"
    cs = [case(e, "one-6items", nt(300, 520, 64)),
          case(e, "one-8items", nt(512, 1024, 128)),
          case(e, "tiny-beside-large-mixedK", nt(512, 1024, 128), nt(8, 16, 32)),
          case(e, "three-b64", nt(257, 255, 64), nt(40, 24, 128, akm=True),
               nt(264, 520, 192, nsplit=3, kc=64)),
          case(e, "three-mixedK", nt(257, 255, 96), nt(1, 1, 64), nt(264, 520, 192, nsplit=2, kc=128)),
          case(e, "split-partial", nt(264, 520, 160, nsplit=3, kc=64)),
          case(e, "split-b64", nt(300, 257, 192, nsplit=2, kc=128)),
          case(e, "split-2of3", nt(264, 520, 160, nsplit=2, kc=64), refused="bad problem"),
          case(e, "four", *[nt(8, 8, 32)] * 4, refused="1..3 problems")]
    for K in (96, 128):
        cs += [case(e, f"akm-K{K}", nt(264, 520, K, akm=True)),
               case(e, f"bkm-K{K}", nt(264, 520, K, bkm=True)),
               case(e, f"abkm-K{K}", nt(264, 520, K, akm=True, bkm=True)),
               case(e, f"abkm-split-K{K}", nt(264, 520, 2 * K, akm=True, bkm=True, nsplit=2, kc=K))]
    return cs


X6_M, X6_K = (1, 255, 256, 257), (16, 48, 272)


def _x6_edges(e):
    """The edges the two x6 entries share (one problem each)."""
    cs = [case(e, f"M{v}", nt(v, 300, 48, pad_a=4, pad_b=8, bsplit=256, b_nsplit=256)) for v in X6_M]
    cs += [case(e, f"N{n}-bs{bs}", nt(257, n, 48, pad_a=4, pad_b=8, bsplit=bs, b_nsplit=bs % n))
           for n, bs in ((256, 256), (300, 256), (300, 300), (513, 256), (513, 512), (513, 513))]
    cs += [case(e, f"K{v}", nt(257, 300, v, pad_a=4, pad_b=8, bsplit=256, b_nsplit=256)) for v in X6_K]
    cs += [case(e, f"bias-ns{v}", nt(257, 300, 48, pad_a=4, pad_b=8, bias=ALLB, bias_nsplit=v))
           for v in (0, 1, 255, 256, 299, 300)]
    cs += [case(e, f"bias-mask{m}", nt(257, 300, 48, pad_a=4, pad_b=8, bias=m, bias_nsplit=256))
           for m in (ALLB & ~A1, ALLB & ~B2, A2, B1)]
    cs += [case(e, "split-partial", nt(257, 300, 272, pad_a=4, pad_b=8, nsplit=3, kc=96, bias=ALLB,
                                       bias_nsplit=256, bsplit=256, b_nsplit=256)),
           case(e, "split-2of3", nt(257, 300, 272, pad_a=4, pad_b=8, nsplit=2, kc=96),
                refused="split-K" if e == "x6nt" else "bad problem")]
    return cs


def _x6multi_cases():
    e = "x6multi"
    q = dict(pad_a=4, pad_b=8)
    cs = _x6_edges(e)
    cs += [case(e, "A2", nt(257, 300, 48, a_ksplit=16, **q)),
           case(e, "B2-k", nt(257, 300, 48, b_ksplit=32, **q)),
           case(e, "B2-n-one-tile", nt(257, 512, 48, b_nsplit=256, **q)),
           case(e, "C2", nt(300, 300, 48, c_msplit=256, **q)),
           case(e, "C2-one-tile", nt(512, 300, 48, c_msplit=256, **q)),
           case(e, "akm", nt(260, 300, 48, akm=True, **q)),
           case(e, "bkm", nt(257, 300, 48, bkm=True, **q)),
           case(e, "abkm", nt(260, 300, 48, akm=True, bkm=True, **q)),
           case(e, "akm-M-not-4", nt(257, 300, 48, akm=True, **q), refused="bad problem"),
           case(e, "A2-split", nt(257, 300, 96, a_ksplit=64, nsplit=3, kc=32, **q)),
           case(e, "A2-split-straddle", nt(257, 300, 96, a_ksplit=48, nsplit=3, kc=32, **q),
                refused="bad problem"),
           case(e, "A2-akm-B2-bkm", nt(260, 300, 64, a_ksplit=32, akm=True, b_ksplit=16, bkm=True, **q)),
           case(e, "B2-n-bkm", nt(257, 516, 48, b_nsplit=256, bkm=True, **q)),
           # the model's combinations: ops.lstm_l0_bwd_x6 (dW with C2 from k-major
           # operands beside dX with B2 along k), ops.proj_bwd_x6 (both k-major / B
           # k-major, split-K), ops.gemm_x6r_nt (B2 along n, bias, split-K)
           case(e, "l0-bwd-pair", nt(512, 68, 272, akm=True, bkm=True, c_msplit=256, **q),
                nt(271, 68, 512, b_ksplit=256, bkm=True, **q)),
           case(e, "proj-bwd-pair", nt(272, 132, 80, akm=True, bkm=True, nsplit=2, kc=48, **q),
                nt(80, 132, 272, bkm=True, nsplit=3, kc=96, **q)),
           case(e, "x6r-nt", nt(257, 513, 272, b_nsplit=256, bias=ALLB, bias_nsplit=256, nsplit=3, kc=96,
                                **q)),
           case(e, "three", nt(257, 300, 48, **q), nt(4, 4, 16, akm=True, bkm=True, **q),
                nt(300, 257, 272, nsplit=2, kc=144, c_msplit=256, **q)),
           case(e, "four", *[nt(4, 4, 16, **q)] * 4, refused="1..3 problems")]
    # the m-first order on both sides of its condition (tiles_m in {2, 4, 8} and tiles_n >= 8)
    cs += [case(e, f"order-{tm}x{tn}", nt(256 * tm - 3, 256 * tn - 4, 16, **q))
           for tm, tn in ((2, 8), (4, 9), (8, 8), (3, 8), (2, 7))]
    return cs


NT_CASES = dict(bf16nt=_bf16nt_cases() + _g256_cases(), bf16multi=_bf16multi_cases(),
                x6nt=_x6_edges("x6nt"), x6multi=_x6multi_cases())
IS_BF16 = dict(bf16nt=True, bf16multi=True, x6nt=False, x6multi=False)


@functools.lru_cache(maxsize=None)
def _nt_data(name, q, M, N, K, bias, bias_nsplit, real):
    g = _gen(f"{name}#{q}")
    if real:
        A = torch.tanh(torch.randn(M, K, generator=g))
        B = torch.randn(N, K, generator=g) * 0.05
        mk = lambda n: torch.randn(n, generator=g) * 0.1  # noqa: E731
    else:
        A, B = ints(g, (M, K)), ints(g, (N, K))
        mk = lambda n: ints(g, (n,), -50, 50)  # noqa: E731
    sizes = (bias_nsplit, bias_nsplit, N - bias_nsplit, N - bias_nsplit)
    vs = [mk(n) if bias & bit and n > 0 else None for bit, n in zip((A1, A2, B1, B2), sizes)]
    return dict(A=A, B=B, bias=vs)


def nt_data(c, q, real=False):
    p = c["probs"][q]
    if c["name"].startswith("cancel-"):
        A, B = cancel_data(c["name"][7:])
        return dict(A=A, B=B, bias=[None] * 4)
    return _nt_data(f"{c['entry']}/{c['name']}", q, p["M"], p["N"], p["K"], p["bias"],
                    p["bias_nsplit"], real)


@functools.lru_cache(maxsize=None)
def _nt_ref_cached(entry, name, q, real, f32):
    c = next(x for x in NT_CASES[entry] + REAL_NT.get(entry, []) + CANCEL_NT.get(entry, [])
             if x["name"] == name)
    return nt_ref(c["probs"][q], nt_data(c, q, real), IS_BF16[entry] and real,
                  torch.float32 if f32 else torch.float64)


def nt_ref_of(c, q, real=False, f32=False):
    return _nt_ref_cached(c["entry"], c["name"], q, real, f32)


# ------------------------------------------------------------------ cast / transpose
EDGE_RC = (1, 63, 64, 65, 130)
# fp32 bit patterns: ties to even both ways, +-0, +-inf, NaN, the largest finite
# fp32 (rounds to inf), a tie that rounds to inf, subnormals
SPECIAL_BITS = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000000,
                0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F7FFFFF, 0xFF7FFFFF,
                0x7F7F8000, 0x00000001, 0x80000001, 0x00400000, 0x007FFFFF, 0x00008000, 0x00018000]


def copy_case(entry, R, C, out=True, outT=True):
    return dict(entry=entry, name=f"{R}x{C}-{int(out)}{int(outT)}", R=R, C=C, out=out, outT=outT,
                pad_in=3, pad_out=5, pad_t=7)


COPY_CASES = ([copy_case(e, r, 65) for e in ("cast", "transpose") for r in EDGE_RC] +
              [copy_case(e, 63, v) for e in ("cast", "transpose") for v in EDGE_RC] +
              [copy_case("cast", 130, 130, out=o, outT=t) for o, t in ((True, False), (False, True))] +
              [copy_case("cast", 1, 1), copy_case("transpose", 1, 1), copy_case("transpose", 130, 130)])


@functools.lru_cache(maxsize=None)
def copy_data(R, C):
    """fp32 [R, C]: randn with every special pattern at a stride coprime to the
    tile, so each lands in rows and columns of every residue."""
    g = _gen(f"copy{R}x{C}")
    x = torch.randn(R * C, generator=g)
    bits = x.view(torch.int32)
    sp = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in SPECIAL_BITS], dtype=torch.int32)
    idx = torch.arange(0, R * C, 3)
    bits[idx] = sp[torch.arange(idx.numel()) % sp.numel()]
    return x.view(R, C)


# ------------------------------------------------------------------ real and cancellation cases
# for each route one unragged shape and the most ragged one of its integer table
REAL_F32 = [f32_case("real-unragged", M=256, N=128, K=64, tb=True, bias=3, alpha=1.0, beta=0.0),
            f32_case("real-ragged", M=257, N=129, K=100, nptr=2, nstrided=3, ksplit=2, bias=3,
                     alpha=2.0, beta=0.5, off_a=1),
            f32_case("real-sk", M=16 * 128 - 5, N=12 * 128 - 3, K=2100, tb=True, sk=True, only="exact",
                     bias=1)]
REAL_NT = dict(
    bf16nt=[case("bf16nt", "real-unragged", nt(256, 128, 64, bias=ALLB, bias_nsplit=64)),
            case("bf16nt", "real-ragged", nt(257, 129, 136, nsplit=3, kc=64, bias=ALLB, bias_nsplit=127)),
            case("bf16nt", "real-g256", nt(769, 513, 160, bias=ALLB, bias_nsplit=256), tile=1),
            case("bf16nt", "real-g256b", nt(769, 513, 192, bias=ALLB, bias_nsplit=256), tile=2)],
    bf16multi=[case("bf16multi", "real-b64", nt(512, 256, 128)),
               case("bf16multi", "real-ragged", nt(264, 520, 160, akm=True, bkm=True, nsplit=3, kc=64),
                    nt(257, 255, 96))],
    x6nt=[case("x6nt", "real-unragged", nt(256, 512, 64, pad_a=4, pad_b=8, bsplit=256, bias=ALLB,
                                           bias_nsplit=256)),
          case("x6nt", "real-ragged", nt(257, 513, 272, pad_a=4, pad_b=8, bsplit=256, bias=ALLB,
                                         bias_nsplit=255, nsplit=3, kc=96))],
    x6multi=[case("x6multi", "real-unragged", nt(256, 512, 64, pad_a=4, pad_b=8, b_nsplit=256, bias=ALLB,
                                                bias_nsplit=256)),
             case("x6multi", "real-ragged", nt(260, 516, 272, pad_a=4, pad_b=8, akm=True, bkm=True,
                                               c_msplit=256, nsplit=3, kc=96, bias=ALLB, bias_nsplit=255),
                  nt(257, 300, 96, pad_a=4, pad_b=8, a_ksplit=64, b_ksplit=32))])

# Cancellation data for the split-bf16 loop (x = x0 + x1 + x2, six cross terms):
#   "a":  A = c_m + d, c_m a per-row integer (= a0), d = (0.5 .. 0.95) 2^-8 c_m (a1,
#         a2: as large as a0 = c_m allows, so a2 b0 stands 2^7 above fp32 rounding);
#         B integer with sum_k B[n][k] = 0 (= b0; b1 = b2 = 0).  The a0 b0 terms
#         cancel and C is carried by a1 b0 and a2 b0.
#   "b":  the roles swapped: C carried by a0 b1 and a0 b2.
#   "ab": A = c_m + d, B = z + e with z zero-sum integers and d, e of three bits
#         (second pieces only): C holds sum d e = a1 b1 at 2^-16 of |a||b| beside
#         a1 b0 and a0 b1.
# a0 b0 itself sums to zero here by construction, so no cancellation data can see
# it dropped; the plain real data does, by orders of magnitude
# (test_cpu_gemm_ref.py::test_cancellation_cases_see_every_cross_term).
CANCEL_KINDS = ("a", "b", "ab")
CANCEL_SHAPE = (257, 300, 272)


@functools.lru_cache(maxsize=None)
def cancel_data(kind, M=CANCEL_SHAPE[0], N=CANCEL_SHAPE[1], K=CANCEL_SHAPE[2]):
    """-> logical A [M, K], B [N, K] (float32, every value exact in fp32)."""
    g = _gen(f"cancel-{kind}")

    def sign(shape):
        return torch.randint(0, 2, shape, generator=g).float() * 2 - 1

    def pow2(shape):
        return 2.0 ** torch.randint(0, 3, shape, generator=g).float()          # 1, 2, 4

    def small(mag, full):
        """0 < d < 2^-8 |x| (half a bf16 ulp above a power of two x: x0 stays x):
        a full fp32 mantissa (second and third pieces) or three bits."""
        if full:
            u = 0.5 + 0.45 * torch.rand(mag.shape, generator=g)
        else:
            u = torch.randint(5, 8, mag.shape, generator=g).float() / 8
        return u * mag * 2.0 ** -8

    def row_const(R, full):
        c = pow2((R, 1)).expand(R, K).contiguous()
        return c + small(c, full)

    def zero_sum(R, eps):
        """Integer rows of +-{1, 2, 4} in adjacent pairs (z, -z): every partial sum
        of c z stays below 4 c in k order.  eps: plus a three-bit second piece."""
        h = sign((R, K // 2)) * pow2((R, K // 2))
        z = torch.stack([h, -h], 2).reshape(R, K)
        return z + z.sign() * small(z.abs(), False) if eps else z      # away from zero: b0 stays z
    if kind == "a":
        return row_const(M, True), zero_sum(N, False)
    if kind == "b":
        return zero_sum(M, False), row_const(N, True)
    return row_const(M, False), zero_sum(N, True)


CANCEL_F32 = [f32_case(f"cancel-{k}", *CANCEL_SHAPE, tb=True) for k in CANCEL_KINDS]
CANCEL_NT = dict(
    x6nt=[case("x6nt", f"cancel-{k}", nt(*CANCEL_SHAPE, pad_a=4, pad_b=8, bsplit=256)) for k in CANCEL_KINDS],
    x6multi=[case("x6multi", f"cancel-{k}", nt(*CANCEL_SHAPE, pad_a=4, pad_b=8, b_nsplit=256))
             for k in CANCEL_KINDS])


# ------------------------------------------------------------------ process-wide switches
# name -> (variable, value, GemmEnv field it clears or sets, the entries whose
# integer cases the child runs)
CHILD_SETTINGS = {
    "b16_kt64": ("AINP_GEMM_B16_KT", "64", "b16_kt64", ["f32:bf16"]),
    "g256_bk64_0": ("AINP_G256_BK64", "0", "g256_bk64", ["bf16nt", "bf16multi"]),
    "gemm16_256_0": ("AINP_GEMM16_256", "0", "gemm16_256", ["bf16nt"]),
    "x6_splitpass_0": ("AINP_X6_SPLITPASS", "0", "x6_splitpass", ["x6nt", "cancel:x6nt"]),
    "x6r_mfast_0": ("AINP_X6R_MFAST", "0", "x6r_mfast", ["x6multi"]),
    "x6r_apf_0": ("AINP_X6R_APF", "0", "x6r_apf", ["x6multi", "cancel:x6multi"]),
}
ENV_DEFAULT = dict(b16_kt64=False, g256_bk64=True, gemm16_256=True, x6_splitpass=True, x6r_mfast=True,
                   x6r_apf=True)
ENV_FIELDS = list(ENV_DEFAULT)            # bit i of the host program's `bits` = field i differs


def env_of(setting=None):
    env = dict(ENV_DEFAULT)
    if setting is not None:
        f = CHILD_SETTINGS[setting][2]
        env[f] = not env[f]
    return env


def env_bits(env):
    return sum(1 << i for i, f in enumerate(ENV_FIELDS) if env[f] != ENV_DEFAULT[f])


def cdiv(a, b):
    return -(-a // b)


def f32_streamk(M, N, K, nb, ksplit):
    """The stream-K eligibility the header documents for ainp_gemm_f32_workspace
    (exact loop): no K-concatenation, K >= 2048, at least 192 tiles x batches, a
    last wave of the 768 resident slots less than 90 % full."""
    tiles = cdiv(M, 128) * cdiv(N, 128) * nb
    return ksplit == 0 and K >= 2048 and tiles >= 192 and tiles * 10 < cdiv(tiles, 768) * 768 * 9


def route(c, flags, env, tile_of=None):
    """The kernels a served case launches -- the launchers' dispatch restated
    (gemm.hip ainp_gemm_f32_ex, gemm16.hip, gemm_x6r.hip; the bf16nt tile comes
    from csrc/gemm_route.h through tile_of(M, N, K, nsplit, kc))."""
    e = c["entry"]
    if e == "f32":
        if flags & BF16:
            return ["gemm_f32_kernel<B16K64>" if env["b16_kt64"] else "gemm_f32_kernel<B16>"]
        if flags & EXACT_F32:
            if c["ws"] == "given" and f32_streamk(c["M"], c["N"], c["K"], c["nptr"] * c["nstrided"],
                                                  c["ksplit"]):
                return ["gemm_f32_streamk", "gemm_streamk_fixup"]
            return ["gemm_f32_kernel<F32>"]
        return ["gemm_f32_kernel<X6>"]
    if e == "bf16nt":
        p = c["probs"][0]
        return [("gemm_bf16nt_kernel", "gemm_bf16nt_256_kernel", "gemm_bf16nt_256b_kernel")[
            tile_of(p["M"], p["N"], p["K"], p["nsplit"], p["kc"])]]
    if e == "bf16multi":
        b64 = env["g256_bk64"] and all(p["K"] % 64 == 0 and p["kc"] % 64 == 0 for p in c["probs"])
        return ["gemm_bf16nt_256_multi_kernel<b64>" if b64 else "gemm_bf16nt_256_multi_kernel<b32>"]
    if e == "x6nt":
        return ["gemm_x6nt_256s_kernel" if env["x6_splitpass"] else "gemm_x6nt_256_kernel"]
    if e == "x6multi":
        names = ["gemm_x6r_kernel<apf>" if env["x6r_apf"] else "gemm_x6r_kernel<noapf>"]
        for p in c["probs"]:
            tm, tn = cdiv(p["M"], 256), cdiv(p["N"], 256)
            names.append("order:m-first" if env["x6r_mfast"] and tm in (2, 4, 8) and tn >= 8
                         else "order:n-first")
        return names
    return [{"cast": "cast_bf16_t_kernel", "transpose": "transpose_f32_kernel"}[e]]


KERNELS = ["gemm_f32_kernel<F32>", "gemm_f32_kernel<X6>", "gemm_f32_kernel<B16>",
           "gemm_f32_kernel<B16K64>", "gemm_f32_streamk", "gemm_streamk_fixup", "gemm_bf16nt_kernel",
           "gemm_bf16nt_256_kernel", "gemm_bf16nt_256b_kernel", "gemm_bf16nt_256_multi_kernel<b64>",
           "gemm_bf16nt_256_multi_kernel<b32>", "gemm_x6nt_256_kernel", "gemm_x6nt_256s_kernel",
           "gemm_x6r_kernel<apf>", "gemm_x6r_kernel<noapf>", "cast_bf16_t_kernel",
           "transpose_f32_kernel"]


def int_cases(spec):
    """"f32:x6" / "f32:exact" / "f32:bf16" / an nt entry / "copy" -> [(case, flags)]."""
    if spec.startswith("f32:"):
        prec = spec[4:]
        return [(c, FLAGS[prec]) for c in F32_CASES + SK_CASES if c["only"] in (None, prec)]
    if spec == "copy":
        return [(c, 0) for c in COPY_CASES]
    return [(c, 0) for c in NT_CASES[spec]]


SPECS = ["f32:x6", "f32:exact", "f32:bf16", "bf16nt", "bf16multi", "x6nt", "x6multi", "copy"]
