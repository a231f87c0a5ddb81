"""sha256 of what the GEMM family's public entries of ainp.ops write, one small
case per entry and per route, on the GPU.

    python tests/golden/gen_gemm_outputs.py     # writes gemm_outputs.json

The fixture was written by the library as it stood before the split-K rule
and the 256 x 256 tile route moved into csrc/gemm_route.h and ops.split_k;
tests/test_gpu_gemm_route.py asserts that the same cases still give the same
bytes.  None of these kernels uses atomics: every case runs twice and the
fixture is not written if the two runs differ.  Inputs come from a seeded CPU
generator; M and N are ragged against the 128- and 256-wide tiles.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "ml-audio-inpainting_amd")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_outputs.json")

# the tile ainp_gemm_bf16nt must take (the library's route query, in
# tests/test_gpu_gemm_route.py): name -> (M, N, K, nsplit as launched, tile)
G16, G256, G256B = "g16", "g256", "g256_bk64"
BF16NT = {
    "bf16nt_g16_bias": (200, 136, 72, 1, 1, G16),
    "bf16nt_g16_split": (200, 136, 400, 3, 3, G16),          # kc 192
    "bf16nt_g16_split_fallback": (200, 136, 200, 3, 1, G16),  # kc 128 gives 2 chunks: unsplit
    "bf16nt_g256_k96": (520, 512, 96, 1, 1, G256),
    "bf16nt_g256_k128": (520, 512, 128, 1, 1, G256B),
    "bf16nt_g256_tall_split": (4104, 512, 384, 3, 3, G256B),  # M >= 8N, kc 128
}
# planner answers the cases below rely on (tests/golden/gemm_plans.json)
PLAN_SPLITK = {(64, 65, 2112, 16): 11, (64, 65, 2112, 512): 33}    # ops._splitk_bf16
PLAN_G256 = {"256,40,288": 9}                                     # ops.g256_splits, one problem


def _bf(t):
    import torch
    return t.to(torch.bfloat16).cuda()


def _nan(*shape):
    import torch
    return torch.full(shape, float("nan"), device="cuda")


def _bias(g, n):
    import torch
    return tuple(torch.randn(n, generator=g).cuda() for _ in range(4))


def c_bf16nt(ops, g, name):
    import torch
    M, N, K, S, _, _ = BF16NT[name]
    A = _bf(torch.randn(M, K, generator=g))
    B = _bf(torch.randn(N, K + 8, generator=g))[:, :K]           # ld > K
    nb = N // 2
    bias = tuple(torch.randn(n, generator=g).cuda() for n in (nb, nb, N - nb, N - nb))
    out = _nan(M, N)
    ops.gemm_bf16nt(A, B, K=K, out=out, bias=bias, bias_nsplit=nb, nsplit=S)
    return {"c": out}


def c_x6_proj(ops, g, entry, K, S):
    import torch
    M, H4 = 264, 256
    A = torch.relu(torch.randn(M, K, generator=g)).cuda()
    wf = (torch.randn(H4, K, generator=g) * 0.02).cuda()
    wr = (torch.randn(H4, K, generator=g) * 0.02).cuda()
    out = _nan(M, 2 * H4)
    getattr(ops, entry)(A, wf, wr, out, bias=_bias(g, H4), bias_nsplit=H4, nsplit=S)
    return {"c": out}


def c_l0_bwd_x6(ops, g):
    import torch
    NT, H, I = 272, 64, 20
    dg = (torch.randn(NT, 8 * H, generator=g) * 1e-2).cuda()
    x = torch.relu(torch.randn(NT, I, generator=g)).cuda()
    wf = (torch.randn(4 * H, I, generator=g) * 0.05).cuda()
    wr = (torch.randn(4 * H, I, generator=g) * 0.05).cuda()
    dx, dwf, dwr = _nan(NT, I), _nan(4 * H, I), _nan(4 * H, I)
    ops.lstm_l0_bwd_x6(dg, wf, wr, x, dx, dwf, dwr)
    return {"dx": dx, "dwf": dwf, "dwr": dwr}


def c_proj_bwd_x6(ops, g, joint):
    import torch
    NT, NO, K = 272, 48, 36
    gp = (torch.randn(NO, NT, generator=g) * 1e-2).cuda()
    h = torch.tanh(torch.randn(NT, K, generator=g)).cuda()
    w = (torch.randn(NO, K, generator=g) * 0.05).cuda()
    dh, dw = _nan(NT, K), _nan(NO, K)
    if joint:
        ops.proj_bwd_x6(gp, h, w, dh=dh, dw=dw)
    else:
        ops.proj_bwd_x6(gp, h, w, dh=dh)
        ops.proj_bwd_x6(gp, h, w, dw=dw)
    return {"dh": dh, "dw": dw}


def c_l0_bwd_bf16(ops, g, km):
    import torch
    NT, H, I = 288, 32, 40
    dg16 = _bf(torch.randn(NT, 8 * H, generator=g) * 1e-3)
    x16 = _bf(torch.randn(NT, I, generator=g))
    wT16 = _bf(torch.randn(I, 8 * H, generator=g) * 0.01)
    dx, gcat = _nan(NT, I), _nan(8 * H, I)
    ops.lstm_l0_bwd_bf16(dg16, None if km else dg16.T.contiguous(), wT16,
                         x16 if km else x16.T.contiguous(), dx, gcat, km=km)
    return {"dx": dx, "gcat": gcat}


def c_wgrad_bf16_km(ops, g):
    import torch
    NT, rows, I = 288, 256, 40                  # PLAN_G256: split 9
    dg16 = _bf(torch.randn(NT, 2 * rows, generator=g) * 1e-3)
    x16 = _bf(torch.randn(NT, I, generator=g))
    out = _nan(rows, I)
    ops.wgrad_bf16_km(dg16[:, rows:], x16, NT, out)
    return {"dw": out}


def c_bf16nt_splitk(ops, g, max_split):
    import torch
    M, N, K = 64, 65, 2112                      # PLAN_SPLITK: split 11 / 33
    A = _bf(torch.randn(M, K, generator=g) * 1e-2)
    B = _bf(torch.randn(N, K, generator=g))
    return {"c": ops.gemm_bf16nt_splitk(A, B, K, max_split=max_split)}


def c_tn_splitk(ops, g, bf16):
    import torch
    NT, H = 272, 64
    dg = (torch.randn(NT, 8 * H, generator=g) * 1e-2).cuda()
    hp = torch.tanh(torch.randn(NT, 2 * H, generator=g)).cuda()
    c0, c1 = ops.gemm_tn_splitk(dg, 8 * H, hp, 2 * H, NT, 4 * H, H, offsets_b=(0, H), bf16=bf16)
    return {"c0": c0, "c1": c1}


def c_wgrad16_nhwc(ops, g):
    import torch
    N, Cin, Cout, HW, k, s, p = 2, 8, 64, 16, 4, 2, 1
    ldA = N * 8 * 8                              # N * Ho * Wo = 128, a multiple of 64
    gA = _bf(torch.randn(Cout, ldA, generator=g))
    x16 = _bf(torch.randn(N, HW, HW, Cin, generator=g))
    return {"g": ops.wgrad16_nhwc(gA, x16, k, s, p, max_split=512)}


def c_batched_splitk(ops, g):
    import torch
    b, c, hw = 2, 24, 1024
    x = torch.randn(b, c, hw, generator=g).cuda()
    out = _nan(b, c, c)
    ops.gemm_batched_splitk(c, c, hw, [x[i] for i in range(b)], hw, 1, [x[i] for i in range(b)],
                            1, hw, out, alpha=1.0 / (c * hw), per_batch_out=True)
    return {"c": out}


CASES = {name: (lambda ops, g, name=name: c_bf16nt(ops, g, name)) for name in BF16NT}
for _e in ("gemm_x6nt_256", "gemm_x6r_nt"):
    for _s in (1, 3):
        CASES[f"{_e}_k112_s{_s}"] = lambda ops, g, e=_e, s=_s: c_x6_proj(ops, g, e, 112, s)
CASES.update({
    "gemm_x6r_nt_k32_s3_fallback": lambda ops, g: c_x6_proj(ops, g, "gemm_x6r_nt", 32, 3),
    "lstm_l0_bwd_x6": c_l0_bwd_x6,
    "proj_bwd_x6_joint": lambda ops, g: c_proj_bwd_x6(ops, g, True),
    "proj_bwd_x6_two_calls": lambda ops, g: c_proj_bwd_x6(ops, g, False),
    "lstm_l0_bwd_bf16": lambda ops, g: c_l0_bwd_bf16(ops, g, False),
    "lstm_l0_bwd_bf16_km": lambda ops, g: c_l0_bwd_bf16(ops, g, True),
    "wgrad_bf16_km": c_wgrad_bf16_km,
    "gemm_bf16nt_splitk_max16": lambda ops, g: c_bf16nt_splitk(ops, g, 16),
    "gemm_bf16nt_splitk_max512": lambda ops, g: c_bf16nt_splitk(ops, g, 512),
    "gemm_tn_splitk_fp32": lambda ops, g: c_tn_splitk(ops, g, False),
    "gemm_tn_splitk_bf16": lambda ops, g: c_tn_splitk(ops, g, True),
    "wgrad16_nhwc": c_wgrad16_nhwc,
    "gemm_batched_splitk": c_batched_splitk,
})


def run_case(name):
    """{output name: sha256} of one case."""
    import torch
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ainp import ops
    g = torch.Generator().manual_seed(2000 + sum(map(ord, name)))
    outs = CASES[name](ops, g)
    torch.cuda.synchronize()
    return {k: hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()
            for k, t in outs.items()}


def main():
    doc = {}
    for name in CASES:
        a, b = run_case(name), run_case(name)
        if a != b:
            raise SystemExit(f"{name}: two runs differ ({a} / {b}); fixture not written")
        doc[name] = a
        print(name, {k: v[:12] for k, v in a.items()}, flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, len(doc), "cases")


if __name__ == "__main__":
    main()
