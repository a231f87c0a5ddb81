"""CPU tests of the basis learning: the properties of the
test-only reference tests/basis_learn_ref.py, the conditions on the inputs that
the GPU parity cases of test_gpu_basis_learn.py rest on, the derivation of their
bound, the frame selection and range checks of ainp.basis_learn, and the
argument checks of ainp_basis_learn / ainp_spain_dgt (no launch).

Measured here (float64, the cases of basis_learn_ref.CASES):
  two float64 formulations (row sums in a permuted order, expm by eigh instead
  of the Taylor action): U moves by at most 2.5e-13 (max abs), P, D and the
  sparsities by at most 1.6e-15 (relative);
  float32-rounded X: U moves by at least 1.0e-10, P, D and the sparsities by at
  least 3.1e-12 (relative).
BOUND_U = 5e-12 and BOUND_OBJ = 1e-13 lie 10 x above the first and 10 x below
the second for every case.
"""
import ctypes
import inspect

import numpy as np
import pytest

import basis_learn_ref as R

BOUND_U = 5e-12
BOUND_OBJ = 1e-13


def _moved(a, b):
    """-> (counts and flags equal, max |dU|, largest relative change of P, D and
    the sparsities) between two runs."""
    ta, tb = a["trace"], b["trace"]
    fin = np.isfinite(ta[:, 0])
    same = (np.array_equal(np.isfinite(tb[:, 0]), fin) and np.array_equal(ta[fin, 1], tb[fin, 1])
            and np.array_equal(ta[fin, 5], tb[fin, 5]))
    obj = max(np.max(np.abs(ta[fin, c] - tb[fin, c]) / np.abs(ta[fin, c])) for c in (2, 3, 4))
    for key in ("sparsity_init", "sparsity_final"):
        obj = max(obj, abs(a[key] - b[key]) / a[key])
    return same, float(np.abs(a["U"] - b["U"]).max()), float(obj)


# ------------------------------------------------------------ the restatement
def test_adjoint_identity():
    """Re <lam, B v> = <B^H lam, v> for B (d, e) = j 2 pi tridiag(d, e) Y."""
    rng = np.random.default_rng(0)
    for K, Mt in ((5, 1), (17, 24), (33, 70)):
        Y = rng.standard_normal((K, Mt)) + 1j * rng.standard_normal((K, Mt))
        lam = rng.standard_normal((K, Mt)) + 1j * rng.standard_normal((K, Mt))
        d = rng.standard_normal(K)
        e = rng.standard_normal(K - 1) + 1j * rng.standard_normal(K - 1)
        lhs = (np.conj(lam) * (1j * R.TWO_PI * R.band(d, e, Y))).real.sum()
        g_d, g_e = R.adjoint(lam, Y)
        rhs = (g_d * d).sum() + (np.conj(g_e) * e).real.sum()
        scale = np.abs(lam).sum() * np.abs(Y).max() * R.TWO_PI * 3
        assert abs(lhs - rhs) <= 1e-14 * scale, (K, Mt, lhs, rhs)
        assert np.allclose(R.band(d, e, Y), R.dense(d, e) @ Y, rtol=0, atol=1e-13 * np.abs(Y).max())


@pytest.mark.parametrize("name", list(R.CASES))
def test_weak_duality_margins_and_result(name):
    """D <= P at every check; the run is clear of gap_tol and of a tie in every
    accept / reject decision; U is unitary; the sparsity falls and is |U X|_1."""
    res, X = R.case_reference(name), R.case_input(name)
    for cs in res["checks"]:
        for it, P, D in cs:
            assert D <= P * (1 + 1e-14), (name, it, P, D)
    gap_margin, tie_margin = R.margins(res, R.GAP_TOL)
    print(f"{name}: |gap - gap_tol| / gap_tol >= {gap_margin:.2e}, decisions clear by {tie_margin:.2e}")
    assert gap_margin >= 1e-6 and tie_margin >= 1e-10
    U = res["U"]
    assert np.abs(U @ U.conj().T - np.eye(len(U))).max() <= 1e-10
    assert res["sparsity_final"] < res["sparsity_init"]
    assert res["sparsity_init"] == np.abs(X).sum(axis=1).sum()
    assert abs(res["sparsity_final"] - np.abs(U @ X).sum()) <= 1e-13 * res["sparsity_final"]
    tr = res["trace"]
    fin = np.isfinite(tr[:, 0])
    assert fin.sum() == len(res["checks"]) and np.all(np.isnan(tr[~fin]))
    if name in R.CONVERGES:
        kw = dict(max_iters=20000, check=100)
        kw.update(R.CASES[name][1])
        assert np.all(tr[fin, 1] < kw["max_iters"])
        assert np.all((tr[fin, 2] - tr[fin, 3]) <= R.GAP_TOL * tr[fin, 2])


def test_zero_row_and_column_take_step_zero():
    X = R.case_input("zero_row_col")
    tau_d, tau_e, sigma = R.steps(X)
    K, Mt = X.shape
    assert tau_d[K // 2] == 0.0 and np.all(sigma[:, Mt // 3] == 0.0)
    assert np.all(np.isfinite(tau_d)) and np.all(np.isfinite(tau_e)) and np.all(np.isfinite(sigma))
    res = R.case_reference("zero_row_col")
    assert np.all(np.isfinite(res["U"])) and np.all(np.isfinite(res["trace"][:4]))


def test_tiny_level_ends_on_the_bound():
    X = R.case_input("tiny_level")
    s = R.solve(X, 1e-4, R.GAP_TOL)
    assert np.allclose(np.abs(s["e"]), 1e-4, rtol=1e-12, atol=0)


def test_reject_case_halves_twice():
    tr = R.case_reference("reject")["trace"]
    assert tr[:, 5].tolist() == [1.0] * 10 + [0.0, 0.0, 1.0, 1.0]
    assert tr[:, 0].tolist() == [0.05] * 11 + [0.025, 0.0125, 0.0125]
    assert tr[10, 4] > tr[9, 4] and tr[11, 4] > tr[9, 4] and tr[12, 4] < tr[9, 4]


def test_preconditioning_is_needed():
    X = R.case_input("k17_m24")
    kw = dict(gap_tol=R.GAP_TOL, max_iters=3000, check=100)
    assert R.solve(X, 0.05, **kw)["iters"] < 3000
    s = R.solve(X, 0.05, scalar_step=True, **kw)
    assert s["iters"] == 3000 and s["P"] - s["D"] > 10 * R.GAP_TOL * s["P"]


def test_taylor_action_is_expm():
    rng = np.random.default_rng(2)
    for K, level in ((17, 0.25), (65, 0.02), (33, 1e-4)):
        d = rng.uniform(-level, level, K)
        e = level * np.exp(2j * np.pi * rng.uniform(size=K - 1))
        T = rng.standard_normal((K, 9)) + 1j * rng.standard_normal((K, 9))
        got, want = R.taylor_action(d, e, T, level), R.expm_eigh(d, e) @ T
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (K, level)
    assert [R.taylor_terms(v) for v in (0.25, 0.02, 1e-4)] == [37, 15, 6]


@pytest.mark.parametrize("name", list(R.CASES))
def test_parity_bound_lies_between_round_off_and_float32(name):
    a = R.case_reference(name)
    same2, u2, o2 = _moved(a, R.case_reference(name, 2))
    same32, u32, o32 = _moved(a, R.case_reference(name, 1, True))
    print(f"{name}: formulations U {u2:.2e} obj {o2:.2e}; float32 X U {u32:.2e} obj {o32:.2e}")
    assert same2 and same32
    assert 10 * u2 <= BOUND_U <= u32 / 10
    assert 10 * o2 <= BOUND_OBJ <= o32 / 10


# ------------------------------------------------------------- training frames
def test_training_frame_selection():
    from ainp.basis_learn import training_frame_indices
    import spain_learned_ref as S
    w, a, M, Ls = 16, 4, 32, 150                       # pads to 160: N = 40 frames
    obs = S.mask(Ls, ((70, 78),))
    frames = training_frame_indices(obs, Ls, w, a, M)
    assert np.array_equal(frames, R.training_frames(S.signal(Ls), obs, w, a, M)[1])
    # frame n holds samples [4 n - 8, 4 n + 8)
    assert frames[0] == 2 and 1 not in frames           # frame 1 wraps around the start
    assert 15 in frames and 16 not in frames            # frame 15 ends before 70; 16 holds it
    assert 21 not in frames and 22 in frames            # frame 21 starts at 76 < 78; 22 at 80
    assert frames[-1] == 35                             # frame 35 ends at 148 <= 150; 36 holds padding
    one_before = S.mask(Ls, ((72, 78),))                # frame 16 = [56, 72) ends one sample before
    assert 16 in training_frame_indices(one_before, Ls, w, a, M)
    assert 16 not in training_frame_indices(S.mask(Ls, ((71, 78),)), Ls, w, a, M)
    near = training_frame_indices(obs, Ls, w, a, M, context=2)
    assert np.array_equal(near, [14, 15, 22, 23])       # frames 16 .. 21 touch the gap
    assert np.array_equal(near, R.training_frames(S.signal(Ls), obs, w, a, M, context=2)[1])
    assert training_frame_indices(obs, Ls, w, a, M, context=0).size == 0
    # a gap at the start: the last frames wrap onto it, which is not near in time
    w2, a2, M2, L2, gaps2 = S.CASES["w16_wraps"][:5]
    for Ls2 in (L2, L2 - 10):
        got = training_frame_indices(S.mask(Ls2, gaps2), Ls2, w2, a2, M2, context=2)
        assert np.array_equal(got, [5, 6])
        assert np.array_equal(got, R.training_frames(S.signal(Ls2), S.mask(Ls2, gaps2), w2, a2, M2, 2)[1])
    with pytest.raises(ValueError):
        training_frame_indices(obs, Ls, w, a, M, context=-1)


# ------------------------------------------------------- host layer, C ABI
def test_check_args_and_exports():
    import models.AudioReg as AR
    from ainp import _lib, ops
    from ainp import basis_learn as BL
    assert BL.check_args(17, 24) == (0.02, 0.02 / 16, 20, 1e-5, 20000, 100)
    sig = inspect.signature(BL.learn_basis)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("level_init", 0.02), ("epsilon", None), ("cnt_max", 20), ("gap_tol", 1e-5),
        ("max_iters", 20000), ("check", 100), ("return_trace", False), ("device", "cuda")]
    bad = [dict(K=16), dict(K=4), dict(K=2049), dict(Mt=0), dict(K=1025, Mt=(1 << 26) // 1025 + 1),
           dict(level_init=0.0), dict(level_init=0.26), dict(level_init=float("nan")),
           dict(epsilon=0.0), dict(epsilon=-1.0), dict(cnt_max=0), dict(cnt_max=65),
           dict(gap_tol=-1e-9), dict(gap_tol=float("nan")), dict(check=0),
           dict(check=200, max_iters=100), dict(max_iters=(1 << 20) + 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            BL.check_args(**dict(dict(K=17, Mt=24), **kw))
    for name in ("learn_basis", "spain_learn_basis", "spain_training_frames"):
        assert getattr(AR, name) is getattr(BL, name) and name in AR.__all__
    assert callable(ops.basis_learn) and callable(ops.spain_dgt)
    assert {"ainp_basis_learn", "ainp_basis_learn_workspace", "ainp_spain_dgt",
            "ainp_spain_dgt_workspace"} <= set(_lib.EXPORTED)
    with pytest.raises(ValueError, match="learn"):
        AR.spain_learned_inpaint(np.zeros(768), np.ones(768, bool), basis="learned", w=64, a=16)


def test_ops_refuse_cpu_tensors():
    import torch
    from ainp import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.basis_learn(torch.zeros(5, 3, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.spain_dgt(torch.zeros(1, 128, dtype=torch.float64), w=16, a=4)


ONE = ctypes.c_void_p(16)            # a non-null stand-in, never dereferenced


def test_basis_learn_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["X", "K", "M_tr", "level_init", "epsilon", "cnt_max", "gap_tol", "max_iters", "check",
             "U", "sparsity", "trace", "workspace", "ws_bytes", "stream"]
    good = dict(X=ONE, K=17, M_tr=24, level_init=0.02, epsilon=0.001, cnt_max=20, gap_tol=1e-5,
                max_iters=20000, check=100, U=ONE, sparsity=ONE, trace=ONE, workspace=ONE,
                ws_bytes=1 << 40, stream=None)
    einval = [(dict(X=None), b"bad argument"), (dict(U=None), b"bad argument"),
              (dict(sparsity=None), b"bad argument"), (dict(trace=None), b"bad argument"),
              (dict(K=16), b"K = M / 2 + 1"), (dict(K=4), b"8 <= M <= 2048"),
              (dict(K=2049), b"8 <= M <= 2048"), (dict(K=0), b"K = M / 2 + 1"),
              (dict(M_tr=0), b"M_tr >= 1"), (dict(K=1025, M_tr=(1 << 26) // 1025 + 1), b"2^26"),
              (dict(epsilon=0.0), b"epsilon > 0"), (dict(epsilon=float("nan")), b"epsilon > 0"),
              (dict(level_init=0.0), b"0 < level_init <= 0.25"),
              (dict(level_init=0.2500001), b"0 < level_init <= 0.25"),
              (dict(cnt_max=0), b"1 <= cnt_max <= 64"), (dict(cnt_max=65), b"1 <= cnt_max <= 64"),
              (dict(gap_tol=-1e-12), b"gap_tol >= 0"), (dict(gap_tol=float("nan")), b"gap_tol >= 0"),
              (dict(check=0), b"1 <= check <= max_iters"),
              (dict(check=101, max_iters=100), b"1 <= check <= max_iters"),
              (dict(max_iters=(1 << 20) + 1), b"max_iters <= 2^20"),
              (dict(ws_bytes=8), b"workspace"), (dict(workspace=None), b"workspace"),
              (dict(workspace=ctypes.c_void_p(24)), b"workspace")]
    for kw, rule in einval:
        a = dict(good, **kw)
        assert _lib.lib.ainp_basis_learn(*(a[k] for k in order)) == -1, kw       # AINP_EINVAL
        msg = _lib.lib.ainp_last_error()
        assert b"ainp_basis_learn" in msg and rule in msg, (kw, msg)
    f = _lib.lib.ainp_basis_learn_workspace
    K, Mt = 17, 24
    # Y, its copy and lambda, sigma, two Taylor buffers of K x max(K, Mt), the old U, the rows
    assert f(K, Mt) >= 16 * 3 * K * Mt + 8 * K * Mt + 16 * 2 * K * Mt + 16 * K * K
    assert f(K, 2 * Mt) > f(K, Mt) and f(16, Mt) == 0 and f(K, 0) == 0


def test_spain_dgt_bad_arguments_fail_without_launching():
    from ainp import _lib
    order = ["x", "L", "n_signals", "w", "a", "M", "coef", "workspace", "ws_bytes", "stream"]
    good = dict(x=ONE, L=768, n_signals=1, w=64, a=16, M=128, coef=ONE, workspace=ONE,
                ws_bytes=1 << 30, stream=None)
    einval = [(dict(x=None), b"bad argument"), (dict(coef=None), b"bad argument"),
              (dict(n_signals=-1), b"bad argument"), (dict(M=96), b"M a power of two"),
              (dict(w=48), b"w a power of two"), (dict(a=24), b"a divides w"),
              (dict(L=700), b"multiple of M"), (dict(ws_bytes=8), b"workspace"),
              (dict(workspace=None), b"workspace")]
    for kw, rule in einval:
        a = dict(good, **kw)
        assert _lib.lib.ainp_spain_dgt(*(a[k] for k in order)) == -1, kw
        msg = _lib.lib.ainp_last_error()
        assert msg.startswith(b"ainp_spain_dgt:") and rule in msg, (kw, msg)
    a = dict(good, n_signals=0)
    assert _lib.lib.ainp_spain_dgt(*(a[k] for k in order)) == 0
    f = _lib.lib.ainp_spain_dgt_workspace
    assert f(1, 64) >= 2 * 64 * 8 + 4 and f(2, 64) > f(1, 64) and f(0, 64) == 0
