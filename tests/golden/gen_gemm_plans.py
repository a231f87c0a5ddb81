"""What the GEMM family's pure planning functions answer (no GPU, no launch):
ops.b16_proj_split, ops._splitk_bf16 (max_split 16 and 512), ops.x6r_splits
and ops.g256_splits (one and two problems), ops._chunks_for.

    python tests/golden/gen_gemm_plans.py     # writes gemm_plans.json

The fixture was written by the package as it stood before the split-K rule,
the makespan planner and the 256 x 256 tile route each got one definition
(csrc/gemm_route.h, ops.split_k); tests/test_cpu_gemm_route.py asserts that
the same questions still get the same answers.  Default environment.

The grid: the model's shapes (layer 0 at M = N*T = 10688, N = 8H = 1024,
K = I = 16448; the upper layers' I = 256; the output projection; the
discriminator's weight gradients at the 5 s clip, batch 8) and small, ragged
ones (K % 64 != 0, K < 64, M or N just below 512, M = 8N - 1 and 8N).
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = os.path.join(ROOT, "ml-audio-inpainting_amd")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_plans.json")

NT, G8, I0, I1 = 10688, 1024, 16448, 256      # N*T, 8H, layer-0 / upper-layer input width
NO = 514                                      # the output projection's C*F
# (Cout, Cin*k*k + 1, ldA) of the discriminator layers with a GEMM weight gradient
D_WGRAD = [(64, 17, 320512), (128, 1025, 79872), (256, 2049, 19968), (512, 4097, 19136)]

MS = (200, 511, 512, 520, 4095, 4096, 4104, 8191, 8192, NT, 40000)
NS = (136, 511, 512, G8)
KS = (8, 40, 64, 72, 96, 128, 200, I1, 384, 400, I0)

SPLITK_SHAPES = D_WGRAD + [(G8, I0, NT), (128, I0, NT), (G8, I1, NT), (512, 520, 1024),
                           (64, 65, 2112), (2, 17, 56), (40, 40, 72), (128, 129, 200),
                           (300, 200, 4000), (64, 129, 128), (64, 33, 128000)]
ONE = [(NT, I1, NO), (NO, I1, NT), (16896, 256, 4112), (4112, 256, 16896), (G8, I0, NT),
       (128, I0, NT), (272, 36, 48), (48, 36, 272), (288, 40, 256), (256, 40, 288), (264, 512, 112),
       (512, 20, 272), (300, 520, 96), (1000, 776, 2112), (64, 64, 16), (64, 64, 32),
       (100, 100, 40), (512, 512, 1056), (256, 256, 4000)]
TWO = [((NT, I1, NO), (NO, I1, NT)), ((256, 40, 288), (288, 40, 256)),
       ((512, 20, 272), (272, 20, 512)), ((264, 512, 112), (512, 264, 1056)),
       ((1024, 520, 2112), (2048, 520, 1024))]
G256_C2_PAIR = ((G8, I0, NT), (NT, I0, G8))     # ops.lstm_l0_bwd_bf16 in the C3-shape step
CHUNKS = [(NT, t) for t in (1, 2, 4, 16, 130, 258, 512, 1000)] + \
    [(k, t) for k in (1, 63, 64, 272, 288, 1000, 1024, 4099, 16896) for t in (1, 3, 8, 64)]


def key(*a):
    return ",".join(str(int(v)) for v in a)


def skey(shapes):
    return ";".join(key(*s) for s in shapes)


def table(ops):
    """The whole table as plain JSON types (lists, not tuples)."""
    doc = {"b16_proj_split": {}, "_splitk_bf16": {}, "x6r_splits": {}, "g256_splits": {},
           "_chunks_for": {}}
    for M, N, K in itertools.product(MS, NS, KS):
        doc["b16_proj_split"][key(M, N, K)] = int(ops.b16_proj_split(M, N, K))
    for (M, N, K), ms in itertools.product(SPLITK_SHAPES, (16, 512)):
        doc["_splitk_bf16"][key(M, N, K, ms)] = int(ops._splitk_bf16(M, N, K, max_split=ms))
    for name, fn in (("x6r_splits", ops.x6r_splits), ("g256_splits", ops.g256_splits)):
        for sh in [(s,) for s in ONE] + TWO + ([G256_C2_PAIR] if name == "g256_splits" else []):
            doc[name][skey(sh)] = [[int(S), int(kc)] for S, kc in fn(tuple(sh))]
    for K, tiles in CHUNKS:
        doc["_chunks_for"][key(K, tiles)] = int(ops._chunks_for(K, tiles))
    return doc


def main():
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from ainp import ops
    doc = table(ops)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, {k: len(v) for k, v in doc.items()})


if __name__ == "__main__":
    main()
