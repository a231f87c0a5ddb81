"""Host side of learning SPAIN's sparsity-enhancing unitary basis
(models/AudioReg/references/basisopt/basis_opt_new.m), restated without CVX:
DESIGN §14.4.

The training columns are the Gabor coefficients of a signal's reliable frames
(the dgt of ainp.spain_learned, computed on the GPU by ainp_spain_dgt); the
basis is learned from them by ainp_basis_learn (csrc/basis_learn.hip, float64):
every convex subproblem of the reference's loop is solved by a preconditioned
primal-dual iteration to a relative duality gap, the update expm(j 2 pi A) is a
Taylor action, and the accept / reject / halve loop is the reference's.
"""
from __future__ import annotations

import numpy as np

from .gaps import _normalise
from .spain_learned import M_MAX, M_MIN, check_args as _frame_args, padded_length

ELEMS_MAX = 1 << 26                  # csrc/basis_learn.hip BL_ELEMS: K M_tr
MAX_ITERS_MAX = 1 << 20              # BL_MAXIT
CNT_MAX = 64                         # BL_CNT
LEVEL_MAX = 0.25
TRACE_COLUMNS = ("level", "iterations", "P", "D", "sparsity", "kept")


def check_args(K, Mt, level_init=0.02, epsilon=None, cnt_max=20, gap_tol=1e-5, max_iters=20000,
               check=100):
    """ainp_basis_learn's range -> (level_init, epsilon, cnt_max, gap_tol,
    max_iters, check) with epsilon None = level_init / 16 filled in."""
    K, Mt = int(K), int(Mt)
    M = 2 * (K - 1)
    if not (M_MIN <= M <= M_MAX and M & (M - 1) == 0):
        raise ValueError(f"K must be M / 2 + 1 for a power of two M in [{M_MIN}, {M_MAX}], "
                         f"got K = {K}")
    if Mt < 1:
        raise ValueError("at least one training column is needed")
    if K * Mt > ELEMS_MAX:
        raise ValueError(f"K M_tr must not exceed 2^26, got {K} x {Mt}")
    level_init = float(level_init)
    if not 0.0 < level_init <= LEVEL_MAX:
        raise ValueError(f"level_init must be in (0, {LEVEL_MAX}], got {level_init}")
    epsilon = level_init / 16 if epsilon is None else float(epsilon)
    if not epsilon > 0.0:
        raise ValueError("epsilon must be positive")
    if not 1 <= int(cnt_max) <= CNT_MAX:
        raise ValueError(f"cnt_max must be in [1, {CNT_MAX}], got {cnt_max}")
    if not float(gap_tol) >= 0.0:
        raise ValueError("gap_tol must not be negative")
    if not 1 <= int(check) <= int(max_iters) <= MAX_ITERS_MAX:
        raise ValueError(f"1 <= check <= max_iters <= {MAX_ITERS_MAX} is required, got check = "
                         f"{check}, max_iters = {max_iters}")
    return level_init, epsilon, int(cnt_max), float(gap_tol), int(max_iters), int(check)


def _planes(Z):
    """complex128 array -> float64 [..., 2] (re, im), a copy."""
    Z = np.array(Z, dtype=np.complex128, order="C")
    return Z.view(np.float64).reshape(Z.shape + (2,))


def learn_basis(X, level_init=0.02, epsilon=None, cnt_max=20, gap_tol=1e-5, max_iters=20000,
                check=100, return_trace=False, device="cuda"):
    """The unitary U (complex128 numpy [K, K]) that makes U X sparse, for the
    training spectra X [K, M_tr] (array or tensor), by the reference's
    basis_opt_new(X, level_init, epsilon) on the GPU.  level_init: the first
    bound on the entries of the Hermitian tridiagonal generator; it is halved
    after an update that does not lower |U X|_1, until it is <= epsilon (None:
    level_init / 16) or cnt_max subproblems are solved.  gap_tol, max_iters,
    check: a subproblem stops at the first multiple of `check` iterations with
    a relative duality gap <= gap_tol, or at max_iters.  return_trace: also a
    dict(sparsity_init, sparsity_final, trace [cnt_max, 6]: TRACE_COLUMNS per
    solve, NaN past the last)."""
    import torch
    from . import ops
    if hasattr(X, "detach"):
        X = X.detach().cpu().numpy()
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"X must be [K, M_tr], got {X.shape}")
    if not np.all(np.isfinite(_planes(X))):
        raise ValueError("X must be finite")
    args = check_args(X.shape[0], X.shape[1], level_init, epsilon, cnt_max, gap_tol, max_iters, check)
    U, sparsity, trace = ops.basis_learn(torch.from_numpy(_planes(X)).to(device), *args)
    U = np.ascontiguousarray(U.cpu().numpy()).view(np.complex128)[..., 0]
    if not return_trace:
        return U
    sparsity = sparsity.cpu().numpy()
    return U, {"sparsity_init": float(sparsity[0]), "sparsity_final": float(sparsity[1]),
               "trace": trace.cpu().numpy()}


def training_frame_indices(observed, Ls, w, a, M, context=None):
    """The frames of a signal of Ls samples (padded to a multiple of M) whose w
    samples n a - w/2 + i are all inside the signal, none of them wrapped around
    or padding, and all observed; context c: only those within c frames of a
    frame that holds a missing sample (in time: the wrap does not count)."""
    observed = np.asarray(observed, bool)
    N = padded_length(Ls, M) // a
    bad = np.concatenate([[0], np.cumsum(~observed)])            # missing samples before t
    n = np.arange(N)
    t0 = n * a - w // 2
    inside = (t0 >= 0) & (t0 + w <= Ls)
    lo, hi = np.clip(t0, 0, Ls), np.clip(t0 + w, 0, Ls)
    holes = bad[hi] - bad[lo]
    good = inside & (holes == 0)
    if context is not None:
        if int(context) < 0:
            raise ValueError("context must not be negative")
        touch = np.flatnonzero(holes > 0)
        near = np.zeros(N, bool)
        for f in touch:
            near[max(0, f - int(context)):f + int(context) + 1] = True
        good &= near
    return np.flatnonzero(good)


def spain_training_frames(signal, mask, w, a, M, context=None, device="cuda"):
    """The training spectra X (complex128 numpy [K, n]) of one signal: the
    columns of dgt(x, g) (ainp.spain_learned's frame: periodic Hann window of w
    samples every a samples, M channels) over its reliable frames, see
    training_frame_indices.  mask None: NaN marks the missing samples.
    ValueError if no frame qualifies."""
    import torch
    from . import ops
    w, a, M, _ = _frame_args(w, a, M)
    sigs, masks, _ = _normalise(signal, mask)
    if len(sigs) != 1:
        raise ValueError("spain_training_frames takes one signal")
    x, obs = sigs[0], masks[0]
    frames = training_frame_indices(obs, len(x), w, a, M, context)
    if frames.size == 0:
        raise ValueError(f"no frame of {w} samples is fully observed"
                         + ("" if context is None else f" within {context} frames of a gap"))
    xp = np.zeros((1, padded_length(len(x), M)))
    xp[0, :len(x)] = np.where(obs, x, 0.0)
    coef = ops.spain_dgt(torch.from_numpy(xp).to(device), w, a, M)[0].cpu().numpy()
    coef = np.ascontiguousarray(coef[frames]).view(np.complex128)[..., 0]        # [n, K]
    return np.ascontiguousarray(coef.T)


def spain_learn_basis(signal, mask, w, a, M, context=None, device="cuda", **learn):
    """learn_basis on a signal's own reliable frames: spain_training_frames(signal,
    mask, w, a, M, context), then learn_basis(X, **learn)."""
    X = spain_training_frames(signal, mask, w, a, M, context, device=device)
    return learn_basis(X, device=device, **learn)
