"""Host-side tests of SPAIN over the whole signal with a unitary basis: the
test-only reference tests/spain_learned_ref.py, the padding, grouping, defaults
and refusals of ainp.spain_learned, the argument checks of ainp_spain_learned,
and the exports.  No GPU.

The hard threshold is discontinuous (test_cpu_spain.py says why that matters):
test_parity_inputs_are_well_conditioned asserts, on the reference alone, that no
input of the GPU parity tests comes near a tie or near epsilon, and
test_parity_bound_sits_between_roundoff_and_float32 that 1e-9 * max|clean gap|
lies between what two float64 formulations differ by and what float32 input
moves.  DESIGN §14.2 records the figures both print.
"""
import ctypes
import inspect
import os

import numpy as np
import pytest

import spain_learned_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAC = os.path.join(ROOT, "tests", "golden", "flac")
BOUND = 1e-9          # the project's parity bound, relative to max|clean gap|


def _runs():
    """Every (tag, reference dict) the GPU parity tests compare with."""
    for name in R.PARITY:
        for alg in R.ALGS:
            for wb in (False, True):
                yield f"{name} {alg} {'U' if wb else 'I'}", R.case_reference(name, alg, wb)
    for alg in R.ALGS:
        for wb in (False, True):
            yield (f"schedule {alg} {'U' if wb else 'I'}",
                   R.case_reference(R.SCHEDULE[0], alg, wb, extra=R.SCHEDULE[1]))
        yield f"largest {alg}", R.big_reference(alg)
        tie = R.tie_reference(alg)
        # the first pass of the tie run is the pure tie it is there for
        yield f"tie {alg}", dict(tie, stats=tie["stats"][1:])


# ---------------------------------------------------------- the reference
def test_parity_inputs_are_well_conditioned():
    """At every evaluated pass of every GPU parity run the k-th and the (k+1)-th
    ranked magnitude of every column are at least 1e-8 apart (relative; two exact
    zeros are exempt) and the objective is at least 1e-6 (relative) from epsilon.
    Measured: smallest margin 3.6e-7 (aspain, w64 with s 2, r 3, U), among the
    default schedules 1.07e-6 (aspain, w128, U); smallest distance 1.07e-3
    (sspain, w128, U)."""
    worst_m, worst_d = np.inf, np.inf
    for tag, ref in _runs():
        margin, dist = R.conditions(ref["stats"], R.EPSILON if "tie" not in tag else R.TIE["epsilon"])
        print(f"{tag}: passes {ref['iters']}, margin {margin:.2e}, distance to epsilon {dist:.2e}")
        assert margin >= 1e-8, tag
        assert dist >= 1e-6, tag
        worst_m, worst_d = min(worst_m, margin), min(worst_d, dist)
    print(f"smallest margin {worst_m:.2e}, smallest distance {worst_d:.2e}")


def test_parity_bound_sits_between_roundoff_and_float32():
    """1e-9 * max|clean gap| lies at least 10 x above what the two formulations
    differ by and, wherever float32 input keeps the pass count, at least 10 x
    below what it moves.  Measured over the parity cases: formulations at most
    5.7e-15, float32 at least 5.3e-8 (both relative to max|clean gap|)."""
    two, f32 = 0.0, np.inf
    for name in R.PARITY:
        scale = R.gap_scale(name)
        for alg in R.ALGS:
            for wb in (False, True):
                one = R.case_reference(name, alg, wb)
                other = R.case_reference(name, alg, wb, 2)
                single = R.case_reference(name, alg, wb, 1, True)
                assert other["iters"] == one["iters"]
                d2 = np.abs(one["out"] - other["out"]).max() / scale
                d_obj = np.nanmax(np.abs(one["obj"] - other["obj"]) / one["obj"])
                assert 10 * d2 <= BOUND and 10 * d_obj <= BOUND, (name, alg, wb, d2, d_obj)
                two = max(two, d2)
                if single["iters"] == one["iters"]:
                    d32 = np.abs(one["out"] - single["out"]).max() / scale
                    assert d32 >= 10 * BOUND, (name, alg, wb, d32)
                    f32 = min(f32, d32)
                    print(f"{name} {alg} {'U' if wb else 'I'}: formulations {d2:.2e}, "
                          f"float32 input {d32:.2e}")
                else:
                    print(f"{name} {alg} {'U' if wb else 'I'}: formulations {d2:.2e}, float32 "
                          f"input changes the pass count ({single['iters']} for {one['iters']})")
    print(f"formulations at most {two:.2e}, float32 at least {f32:.2e}, bound {BOUND:.0e}")
    for alg in R.ALGS:                       # the largest transform, objectives and gap
        one, other = R.big_reference(alg), R.big_reference(alg, 2)
        d_obj = np.nanmax(np.abs(one["obj"] - other["obj"]) / one["obj"])
        assert 10 * d_obj <= BOUND and np.abs(one["out"] - other["out"]).max() * 10 <= BOUND


def test_evaluation_clip_is_well_conditioned():
    """The same two conditions for the clip, gap and settings of the GPU test of
    run_spain_learned_evaluation.  Measured: smallest margin 2.2e-6."""
    import utils
    E = R.EVAL
    audio, sr = utils.load_audio(os.path.join(FLAC, E["clip"]))
    audio = audio.astype(np.float64)
    obs = np.ones(len(audio), bool)
    obs[int(2.0 * sr):int(2.0 * sr) + int(0.08 * sr)] = False
    for U in (None, R.basis(E["M"] // 2 + 1, E["level"])):
        for alg in R.ALGS:
            ref = R.padded_reference(audio, obs, U, alg, E["w"], E["a"], E["M"], maxit=E["maxit"])
            margin, dist = R.conditions(ref["stats"], R.EPSILON)
            print(f"{E['clip']} {alg} {'I' if U is None else 'U'}: margin {margin:.2e}, "
                  f"distance to epsilon {dist:.2e}")
            assert margin >= 1e-8 and dist >= 1e-6


@pytest.mark.parametrize("w,a,M", [(8, 2, 8), (16, 4, 32), (64, 16, 128), (128, 32, 256),
                                   (16, 8, 16)])
def test_transforms_reconstruct(w, a, M):
    """idgt(dgt(x, g), gd) = x and idgt(dgt(x, gd), g) = x, both formulations."""
    g, gd = R.windows(w, a, M)
    x = np.random.default_rng(5).standard_normal(3 * M)
    for full in (False, True):
        for wa, ws in ((g, gd), (gd, g)):
            err = np.abs(R.idgt(R.dgt(x, wa, a, M, full), ws, a, M, len(x), full) - x).max()
            assert err <= 4e-15, (full, err)
    assert R.dgt(x, g, a, M).shape == (M // 2 + 1, len(x) // a)


def test_basis_is_unitary():
    for K, level in ((5, 0.02), (17, 0.02), (65, 0.02), (129, 0.05), (1025, 0.02)):
        U = R.basis(K, level)
        assert U.shape == (K, K)
        assert np.abs(U @ U.conj().T - np.eye(K)).max() <= 1e-13
        assert np.abs(U - np.eye(K)).max() > 1e-3          # and not the identity


@pytest.mark.parametrize("alg", R.ALGS)
def test_diagonal_basis_selects_and_returns_what_identity_does(alg):
    """A diagonal unitary U only turns phases: the same magnitudes, so the same
    selections, objectives and result as U = I."""
    clean, obs, _, w, a, M = R.case_input("w64")
    K = M // 2 + 1
    D = np.diag(np.exp(2j * np.pi * np.random.default_rng(11).uniform(0, 1, K)))
    z = R.dgt(clean, R.windows(w, a, M)[0], a, M)
    for k in (1, 7, 40):
        assert np.array_equal(R.hard_threshold(D @ z, k)[0] != 0, R.hard_threshold(z, k)[0] != 0)
    plain = R.spain_learned(clean, obs, None, alg, w, a, M, epsilon=R.EPSILON)
    turned = R.spain_learned(clean, obs, D, alg, w, a, M, epsilon=R.EPSILON)
    assert turned["iters"] == plain["iters"]
    assert np.nanmax(np.abs(turned["obj"] - plain["obj"]) / plain["obj"]) <= BOUND
    assert np.abs(turned["out"] - plain["out"]).max() <= BOUND * R.gap_scale("w64")


def test_the_other_tie_rule_changes_the_objectives():
    """The unit impulse of the GPU tie test: the first H_1 is a pure tie in the
    impulse's frame and in no other, and keeping the higher row instead moves the
    objectives of the passes after it by far more than the parity bound."""
    x, obs = R.tie_input()
    T = R.TIE
    z = R.dgt(x, R.windows(T["w"], T["a"], T["M"])[0], T["a"], T["M"])
    col = np.abs(z[:, T["at"] // T["a"]])
    assert np.all(col == col[0]) and col[0] > 0
    rest = np.delete(z, T["at"] // T["a"], axis=1)              # no other column is near a tie
    assert R.hard_threshold(rest, 1)[1] >= 1e-8
    for alg in R.ALGS:
        low, high = R.tie_reference(alg), R.tie_reference(alg, "high")
        assert low["stats"][0][0] == 0.0                      # the pure tie
        moved = np.nanmax(np.abs(low["obj"] - high["obj"]) / low["obj"])
        print(f"{alg}: the other tie rule moves the objectives by {moved:.2e}")
        assert moved >= 1e-6


# ------------------------------------------------------- planner, host layer
def test_padding_and_grouping():
    from ainp.spain_learned import L_MAX, padded_length, plan_groups
    assert padded_length(1, 32) == 32 and padded_length(32, 32) == 32
    assert padded_length(33, 32) == 64 and padded_length(0, 8) == 8
    assert padded_length(81920, 2048) == 81920 and padded_length(80000, 2048) == 81920
    assert padded_length(L_MAX, 2048) == L_MAX
    with pytest.raises(ValueError, match="frames"):
        padded_length(L_MAX + 1, 2048)
    groups = plan_groups([700, 768, 100, 769, 641], 128)
    assert groups == {768: [0, 1, 4], 128: [2], 896: [3]}
    assert list(groups) == [768, 128, 896]                 # order of first appearance
    assert plan_groups([], 128) == {}


def test_defaults():
    from ainp.spain_learned import check_args, default_maxit, spain_learned_inpaint
    assert check_args() == (1024, 256, 2048, 1025)
    assert check_args(64, 16) == (64, 16, 128, 65)
    assert check_args(64, 16, M=64) == (64, 16, 64, 33)
    assert check_args(64, 16, s=2, r=3) == (64, 16, 128, 98)
    assert check_args(64, 16, maxit=7)[3] == 7
    assert default_maxit(128, 2, 3) == R.default_maxit(128, 2, 3) == 98
    sig = inspect.signature(spain_learned_inpaint)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("mask", None), ("basis", None), ("algorithm", "aspain"), ("w", 1024), ("a", 256),
        ("M", None), ("s", 1), ("r", 1), ("epsilon", 0.1), ("maxit", None),
        ("return_history", False), ("device", "cuda")]


def test_refusals():
    from ainp.spain_learned import check_basis, spain_learned_inpaint
    x = np.zeros(768)
    m = R.mask(768, ((300, 320),))
    U = R.basis(65, 0.02)
    bad = [dict(algorithm="pspain"), dict(w=48, a=16), dict(w=4, a=2), dict(w=64, a=16, M=32),
           dict(w=64, a=16, M=96), dict(w=2048, a=512, M=4096), dict(w=64, a=24), dict(w=64, a=64),
           dict(w=64, a=0), dict(w=64, a=16, s=0), dict(w=64, a=16, r=0),
           dict(w=64, a=16, epsilon=-1.0), dict(w=64, a=16, epsilon=float("nan")),
           dict(w=64, a=16, maxit=0), dict(w=64, a=16, maxit=65537),
           dict(w=64, a=16, basis=U[:64, :64]), dict(w=64, a=16, basis=U[:, :64]),
           dict(w=64, a=16, basis=np.ones(65)), dict(w=64, a=16, basis=U * (1 + 2e-10)),
           dict(w=64, a=16, basis=np.zeros((65, 65)))]
    for kw in bad:
        with pytest.raises(ValueError):
            spain_learned_inpaint(x, m, **kw)
    with pytest.raises(ValueError, match="unitary"):
        check_basis(U + 1e-9, 128)
    with pytest.raises(ValueError, match=r"\[K, K\]"):
        check_basis(U, 256)
    assert np.array_equal(check_basis(U, 128), U)
    with pytest.raises(ValueError):
        spain_learned_inpaint(x, m[:-1], w=64, a=16)


def test_exports(tmp_path):
    import models.AudioReg as AR
    from ainp import _lib, ops
    from ainp.spain_learned import spain_learned_inpaint
    from models import model_eval
    assert AR.spain_learned_inpaint is spain_learned_inpaint
    assert "spain_learned_inpaint" in AR.__all__ and "spain_inpaint" in AR.__all__
    assert callable(ops.spain_learned)
    assert {"ainp_spain_learned", "ainp_spain_learned_workspace"} <= set(_lib.EXPORTED)
    ev = inspect.signature(model_eval.run_spain_learned_evaluation).parameters
    assert list(ev) == ["input_dir", "output_dir", "basis", "algorithm", "w", "a", "solver"]
    assert (ev["basis"].default, ev["algorithm"].default, ev["w"].default, ev["a"].default) == \
        (None, "aspain", 1024, 256)
    assert model_eval.SPAIN_ALGORITHMS == ("aspain", "sspain")
    with pytest.raises(ValueError):
        model_eval.run_spain_learned_evaluation(str(tmp_path), str(tmp_path / "o"),
                                                algorithm="ASPAIN-MOD")


def test_ops_spain_learned_refuses_cpu_tensors():
    import torch
    from ainp import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.spain_learned(torch.zeros(2, 128, dtype=torch.float64),
                          torch.ones(2, 128, dtype=torch.uint8), w=16, a=4)


# ---------------------------------------------------------------- the C ABI
ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def test_spain_learned_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["x", "observed", "L", "n_signals", "w", "a", "M", "basis", "algorithm", "s", "r",
             "epsilon", "maxit", "iters", "obj_history", "workspace", "ws_bytes", "stream"]
    good = dict(x=ONE, observed=ONE, L=768, n_signals=2, w=64, a=16, M=128, basis=None, algorithm=0,
                s=1, r=1, epsilon=0.1, maxit=65, iters=ONE, obj_history=None, workspace=ONE,
                ws_bytes=1 << 30, stream=None)
    einval = [(dict(x=None), b"bad argument"), (dict(observed=None), b"bad argument"),
              (dict(iters=None), b"bad argument"), (dict(n_signals=-1), b"bad argument"),
              (dict(algorithm=2), b"AINP_SPAIN_A"), (dict(algorithm=-1), b"AINP_SPAIN_A"),
              (dict(M=96), b"M a power of two"), (dict(M=4, w=4, a=2, L=64), b"8 <= M <= 2048"),
              (dict(M=4096, L=8192), b"8 <= M <= 2048"),
              (dict(w=48), b"w a power of two"), (dict(w=4, a=2), b"8 <= w <= M"),
              (dict(w=256, a=64), b"8 <= w <= M"),
              (dict(a=24), b"a divides w"), (dict(a=64), b"w / a >= 2"), (dict(a=0), b"a divides w"),
              (dict(L=700), b"multiple of M"), (dict(L=0), b"multiple of M"),
              (dict(L=64), b"multiple of M"), (dict(L=(1 << 22) + 128), b"2^22 / a frames"),
              (dict(s=0), b"s >= 1"), (dict(r=0), b"r >= 1"),
              (dict(epsilon=-1e-9), b"epsilon >= 0"), (dict(epsilon=float("nan")), b"epsilon >= 0"),
              (dict(maxit=0), b"1 <= maxit <= 65536"), (dict(maxit=65537), b"1 <= maxit <= 65536"),
              (dict(ws_bytes=8), b"workspace"), (dict(workspace=None), b"workspace"),
              (dict(workspace=ctypes.c_void_p(24)), b"workspace")]

    def call(**kw):
        a = dict(good, **kw)
        return _lib.lib.ainp_spain_learned(*(a[k] for k in order))

    for kw, rule in einval:
        assert call(**kw) == -1, kw                               # AINP_EINVAL
        msg = _lib.lib.ainp_last_error()
        assert b"ainp_spain_learned" in msg and rule in msg, (kw, msg)
    assert call(n_signals=0) == 0        # an empty batch is a no-op, still no launch


def test_spain_learned_workspace_is_a_host_call():
    from ainp import _lib
    f = _lib.lib.ainp_spain_learned_workspace
    K, N, L = 65, 48, 768
    plain = f(L, 1, 64, 16, 128, 0, 0)
    # A: two windows, x, three K x N spectra less one without a basis, frames, parts, state
    assert plain >= 8 * (2 * 64 + L + N * 64 + N) + 16 * 2 * K * N
    assert f(L, 1, 64, 16, 128, 1, 0) - plain == 16 * K * N
    assert f(L, 1, 64, 16, 128, 0, 1) > plain                    # S: u and xe as well
    assert f(L, 2, 64, 16, 128, 0, 0) > plain
    for bad in ((700, 1, 64, 16, 128, 0, 0), (L, 1, 64, 16, 96, 0, 0), (L, 0, 64, 16, 128, 0, 0),
                (L, 1, 64, 16, 128, 0, 2)):
        assert f(*bad) == 0
