"""Host side of SPAIN as its paper states it, with an optional learned basis
(models/AudioReg/references/basisopt: a_spain_learned.m, s_spain_learned.m,
hard_thresholding_dgtreal.m), restated without LTFAT: DESIGN §14.2.

One ADMM loop runs over the whole signal with a Gabor frame (periodic Hann
window of w samples every a samples, M channels) and one stopping rule; the
coefficients of every frame are rotated by a unitary basis before the hard
threshold.  Without a basis this is the global, non-segmented SPAIN row.  The
basis is an input, or basis="learn": basis_opt_new.m on the signal's own
reliable frames (ainp.basis_learn).  (The reference's OMP
coefficient update exists only in the segment-wise sspain.m:
ainp.spain.spain_inpaint(f_update="OMP"))

Signals are padded with observed zeros to a multiple of M and grouped by padded
length; each group is one ainp_spain_learned launch sequence
(csrc/spain_learned.hip, float64).
"""
from __future__ import annotations

import numpy as np

from .gaps import _cdiv, _normalise, restack
from .spain import algorithm_id

M_MIN, M_MAX, W_MIN = 8, 2048, 8     # csrc/spain_learned.hip SL_MMIN, SL_MMAX, SL_WMIN
L_MAX = 1 << 22                      # SL_LMAX: at most L_MAX / a frames a signal
MAXIT_MAX = 65536                    # SL_MAXIT
UNITARY_TOL = 1e-10


def default_maxit(M, s=1, r=1):
    """ceil(K r / s) with K = M / 2 + 1: the pass at which k reaches K."""
    return _cdiv((M // 2 + 1) * int(r), int(s))


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def check_args(w=1024, a=256, M=None, s=1, r=1, epsilon=0.1, maxit=None):
    """The solver's range (ainp_spain_learned's) -> (w, a, M, maxit) with the
    defaults M = 2 w and maxit = ceil(K r / s) filled in."""
    w, a = int(w), int(a)
    M = 2 * w if M is None else int(M)
    if not (_pow2(M) and M_MIN <= M <= M_MAX):
        raise ValueError(f"M must be a power of two in [{M_MIN}, {M_MAX}], got M = {M}")
    if not (_pow2(w) and W_MIN <= w <= M):
        raise ValueError(f"w must be a power of two in [{W_MIN}, M = {M}], got w = {w}")
    if a < 1 or w % a or w // a < 2:
        raise ValueError(f"a must divide w with w / a >= 2, got w = {w}, a = {a}")
    if int(s) < 1 or int(r) < 1:
        raise ValueError("s and r must be at least 1")
    if not float(epsilon) >= 0.0:
        raise ValueError("epsilon must not be negative")
    if maxit is None:
        maxit = default_maxit(M, s, r)
    if not 1 <= int(maxit) <= MAXIT_MAX:
        raise ValueError(f"maxit must be in [1, {MAXIT_MAX}], got {maxit}")
    return w, a, M, int(maxit)


def padded_length(Ls, M):
    """The next multiple of M (dgtlength: a | w | M), at least M."""
    L = max(1, _cdiv(int(Ls), M)) * M
    if L > L_MAX:
        raise ValueError(f"a signal of {Ls} samples pads to {L}, above the {L_MAX} the kernel takes "
                         f"({L_MAX} / a frames)")
    return L


def plan_groups(lengths, M):
    """{padded length: [indices of the signals that have it]}, in order of
    first appearance; every group is one launch sequence."""
    groups = {}
    for i, Ls in enumerate(lengths):
        groups.setdefault(padded_length(Ls, M), []).append(i)
    return groups


def check_basis(basis, M):
    """basis (array or tensor) -> complex128 [K, K], K = M / 2 + 1; ValueError
    for another shape or max|U U^H - I| > 1e-10."""
    if hasattr(basis, "detach"):
        basis = basis.detach().cpu().numpy()
    U = np.ascontiguousarray(basis, dtype=np.complex128)
    K = M // 2 + 1
    if U.shape != (K, K):
        raise ValueError(f"basis must be [K, K] with K = M / 2 + 1 = {K}, got {U.shape}")
    if not np.all(np.isfinite(U.view(np.float64))):
        raise ValueError("basis must be finite")
    dev = float(np.abs(U @ U.conj().T - np.eye(K)).max())
    if dev > UNITARY_TOL:
        raise ValueError(f"basis must be unitary: max|U U^H - I| = {dev:.3g} > {UNITARY_TOL}")
    return U


def spain_learned_inpaint(signal, mask=None, basis=None, algorithm="aspain", w=1024, a=256, M=None,
                          s=1, r=1, epsilon=0.1, maxit=None, return_history=False, device="cuda"):
    """Fill the missing samples of `signal` by A-SPAIN or S-SPAIN over the whole
    signal on the GPU (the reference's a_spain_learned.m / s_spain_learned.m):
    Gabor frame of the periodic Hann window of w samples, hop a, M channels (None:
    2 w); basis: a unitary complex [K, K] array or tensor, K = M / 2 + 1, applied
    to every frame's coefficients before the threshold (None: the identity, the
    global SPAIN row).  basis="learn": one basis per signal, learned from the
    signal's own reliable frames by ainp.basis_learn.spain_learn_basis with its
    defaults; a dict instead of "learn" holds keyword arguments for it (context,
    level_init, epsilon, cnt_max, gap_tol, max_iters, check).  Each such signal
    is its own launch sequence.

    Input layouts, mask / NaN conventions and the return layout are
    spain_inpaint's; only missing samples are written, and there is no limit on
    the number or the length of the gaps.  A signal is padded with observed
    zeros to the next multiple of M.  s, r: k starts at s and grows by s every r
    passes; epsilon: the objective that ends a signal's loop; maxit None:
    ceil(K r / s).  return_history: also one dict per signal (signal, iters,
    objective [maxit]: the objective of every pass, NaN after the last).  A
    signal with nothing missing comes back unchanged with iters = 0.
    """
    import torch
    from . import ops
    algorithm_id(algorithm)
    w, a, M, maxit = check_args(w, a, M, s, r, epsilon, maxit)
    learn = {} if isinstance(basis, str) and basis == "learn" else basis
    learn = dict(learn) if isinstance(learn, dict) else None
    if isinstance(basis, str) and learn is None:
        raise ValueError(f'basis must be None, a unitary matrix, "learn" or a dict, got {basis!r}')
    U = None if basis is None or learn is not None else check_basis(basis, M)
    sigs, masks, kind = _normalise(signal, mask)
    res = [x.copy() for x in sigs]
    iters = [0] * len(sigs)
    objs = [np.full(maxit, np.nan) for _ in sigs]
    todo = [i for i, m in enumerate(masks) if not m.all()]
    to_device = lambda V: torch.from_numpy(V.view(np.float64).reshape(V.shape + (2,))).to(device)
    if learn is None:
        groups = plan_groups([len(sigs[i]) for i in todo], M)
        Ud = to_device(U) if U is not None and groups else None
        runs = [(L, [todo[j] for j in members], Ud) for L, members in groups.items()]
    else:
        from .basis_learn import spain_learn_basis
        runs = []
        for i in todo:
            Ui = check_basis(spain_learn_basis(sigs[i], masks[i], w, a, M, device=device, **learn), M)
            runs.append((padded_length(len(sigs[i]), M), [i], to_device(Ui)))
    for L, idx, Ud in runs:
        x = np.zeros((len(idx), L))
        obs = np.ones((len(idx), L), np.uint8)
        for row, i in enumerate(idx):
            x[row, :len(sigs[i])] = sigs[i]
            obs[row, :len(sigs[i])] = masks[i]
        xd = torch.from_numpy(x).to(device)
        it, hist = ops.spain_learned(xd, torch.from_numpy(obs).to(device), basis=Ud,
                                     algorithm=algorithm, w=w, a=a, M=M, s=s, r=r, epsilon=epsilon,
                                     maxit=maxit, return_history=return_history)
        out, it = xd.cpu().numpy(), it.cpu().numpy()
        hist = hist.cpu().numpy() if hist is not None else None
        for row, i in enumerate(idx):
            res[i] = out[row, :len(sigs[i])].copy()
            iters[i] = int(it[row])
            if hist is not None:
                objs[i] = hist[row].copy()
    out = restack(res, kind)
    if not return_history:
        return out
    return out, [{"signal": i, "iters": iters[i], "objective": objs[i]} for i in range(len(sigs))]
