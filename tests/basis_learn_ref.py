"""Float64 NumPy reference of the basis learning of the reference project's
references/basisopt/basis_opt_new.m, written from the algorithm as DESIGN §14.4
restates it: the convex subproblem solved by a diagonally preconditioned
primal-dual iteration to a duality gap, the basis update as a Taylor action,
the outer accept / reject / halve loop.  Test-only.

It shares no structure with csrc/basis_learn.hip: whole-array operations, and
numpy.linalg.eigh for an independent expm.  formulation 2 computes the same
thing another way (row sums in a permuted order, expm by eigh instead of the
Taylor action) to measure what float64 round-off moves.
"""
import functools

import numpy as np

TWO_PI = 2.0 * np.pi


# ------------------------------------------------------------ the band operator
def band(d, e, T):
    """tridiag(d, e) T: d real [K] on the diagonal, e complex [K-1] above it,
    conj(e) below it."""
    R = d[:, None] * T
    R[:-1] += e[:, None] * T[1:]
    R[1:] += np.conj(e)[:, None] * T[:-1]
    return R


def dense(d, e):
    return np.diag(d).astype(complex) + np.diag(e, 1) + np.diag(np.conj(e), -1)


def residual(d, e, Y):
    """r = (I + j 2 pi A) Y."""
    return Y + 1j * TWO_PI * band(d, e, Y)


def _rowsum(a, perm):
    """Sum over the training index, in the given column order."""
    return a.sum(axis=1) if perm is None else np.add.reduce(a[:, perm], axis=1)


def adjoint(lam, Y, perm=None):
    """B^H lam for B (d, e) = j 2 pi tridiag(d, e) Y, as (g_d real [K], g_e
    complex [K-1]) with <g, v> = sum g_d d + Re sum conj(g_e) e."""
    g_d = TWO_PI * _rowsum((lam * np.conj(Y)).imag, perm)
    g_e = (-1j * TWO_PI * _rowsum(lam[:-1] * np.conj(Y[1:]), perm)
           + 1j * TWO_PI * _rowsum(np.conj(lam[1:]) * Y[:-1], perm))
    return g_d, g_e


def _inv(x):
    """1 / (2 pi x), 0 where x is 0: that variable or term has no effect."""
    out = np.zeros_like(x)
    np.divide(1.0, TWO_PI * x, out=out, where=x > 0)
    return out


def steps(Y, perm=None):
    """-> (tau_d [K], tau_e [K-1], sigma [K, M_tr]) of Pock & Chambolle 2011
    (alpha = 1) for the operator B."""
    absY = np.abs(Y)
    rho = _rowsum(absY, perm)
    col = absY.copy()
    col[:-1] += absY[1:]
    col[1:] += absY[:-1]
    return _inv(rho), _inv(rho[:-1] + rho[1:]), _inv(col)


def solve(Y, level, gap_tol=1e-5, max_iters=20000, check=100, perm=None, scalar_step=False):
    """The subproblem min sum |r(d, e)| s.t. |d_i| <= level, |e_i| <= level ->
    dict(d, e, iters, P, D, checks [(iteration, P, D)]).  Starts from zero."""
    K, Mt = Y.shape
    tau_d, tau_e, sigma = steps(Y, perm)
    if scalar_step:           # one step size for all: what the preconditioning buys
        nrm = 1.0 / max(tau_d[tau_d > 0].min(), 1e-300)
        tau_d, tau_e, sigma = (np.where(t > 0, 1.0 / nrm, 0.0) for t in (tau_d, tau_e, sigma))
    d, e = np.zeros(K), np.zeros(K - 1, complex)
    db, eb = d.copy(), e.copy()
    lam = np.zeros((K, Mt), complex)
    checks, it, P, D = [], 0, np.nan, np.nan
    while it < max_iters:
        it += 1
        lam = lam + sigma * residual(db, eb, Y)
        lam = lam / np.maximum(1.0, np.abs(lam))
        g_d, g_e = adjoint(lam, Y, perm)
        dn = np.clip(d - tau_d * g_d, -level, level)
        en = e - tau_e * g_e
        en = en * (level / np.maximum(level, np.abs(en)))
        db, eb = 2 * dn - d, 2 * en - e
        d, e = dn, en
        if it % check == 0 or it == max_iters:
            P = float(_rowsum(np.abs(residual(d, e, Y)), perm).sum())
            D = float(_rowsum((np.conj(lam) * Y).real, perm).sum()
                      - level * (np.abs(g_d).sum() + np.abs(g_e).sum()))
            checks.append((it, P, D))
            if P - D <= gap_tol * P:
                break
    return {"d": d, "e": e, "iters": it, "P": P, "D": D, "checks": checks}


# ------------------------------------------------------------- the basis update
def taylor_terms(level):
    """The smallest n with (6 pi level)^n / n! < 1e-18 (|A| <= 3 level)."""
    n, term = 0, 1.0
    while term >= 1e-18:
        n += 1
        term *= 6.0 * np.pi * level / n
    return n


def taylor_action(d, e, T, level):
    """expm(j 2 pi A) T as sum_n (j 2 pi A)^n / n! T, band passes only."""
    acc, term = T.copy(), T
    for n in range(1, taylor_terms(level) + 1):
        term = (1j * TWO_PI / n) * band(d, e, term)
        acc = acc + term
    return acc


def expm_eigh(d, e):
    lam, V = np.linalg.eigh(dense(d, e))
    return (V * np.exp(1j * TWO_PI * lam)) @ V.conj().T


# --------------------------------------------------------------- the outer loop
def learn(X, level_init=0.02, epsilon=None, cnt_max=20, gap_tol=1e-5, max_iters=20000, check=100,
          formulation=1):
    """basis_opt_new.m:43-74 -> dict(U, sparsity_init, sparsity_final, trace
    [cnt_max, 6] (level, iterations, P, D, sparsity after the update, kept; NaN
    past the last solve), checks [per solve [(iteration, P, D)]], decisions
    [(sparsity, sparsity_old)] of every finite accept / reject test)."""
    X = np.asarray(X, complex)
    K = X.shape[0]
    epsilon = level_init / 16 if epsilon is None else epsilon
    perm = np.random.default_rng(5).permutation(X.shape[1]) if formulation == 2 else None
    Aopt, Y = np.eye(K, dtype=complex), X.copy()
    sparsity_old, sparsity = np.inf, float(_rowsum(np.abs(X), perm).sum())
    sparsity_init, level, cnt = sparsity, level_init, 1
    trace = np.full((cnt_max, 6), np.nan)
    checks, decisions = [], []
    Aold, Yold, save = Aopt, Y, np.inf
    while level > epsilon:
        while True:
            if np.isfinite(sparsity_old):
                decisions.append((sparsity, sparsity_old))
            if not sparsity < sparsity_old:
                if cnt >= 2:
                    trace[cnt - 2, 5] = 0.0
                break
            s = solve(Y, level, gap_tol, max_iters, check, perm)
            save, sparsity_old, Aold, Yold = sparsity_old, sparsity, Aopt, Y
            if formulation == 2:
                E = expm_eigh(s["d"], s["e"])
                Aopt, Y = E @ Aopt, E @ Y
            else:
                Aopt = taylor_action(s["d"], s["e"], Aopt, level)
                Y = taylor_action(s["d"], s["e"], Y, level)
            sparsity = float(_rowsum(np.abs(Y), perm).sum())
            trace[cnt - 1] = (level, s["iters"], s["P"], s["D"], sparsity, 1.0)
            checks.append(s["checks"])
            cnt += 1
            if cnt > cnt_max:
                break
        if cnt > cnt_max:
            break
        level = level / 2
        Aopt, Y, sparsity, sparsity_old = Aold, Yold, sparsity_old, save     # undo the update
    return {"U": Aopt, "sparsity_init": sparsity_init,
            "sparsity_final": float(_rowsum(np.abs(Aopt @ X), perm).sum()), "trace": trace,
            "checks": checks, "decisions": decisions}


def margins(res, gap_tol):
    """-> (smallest |gap - gap_tol| / gap_tol over every gap check, smallest
    |sparsity - sparsity_old| / sparsity_old over every decision) of a run."""
    gaps = [abs((P - D) / P - gap_tol) / gap_tol for cs in res["checks"] for _, P, D in cs
            if P > 0] if gap_tol > 0 else []
    dec = [abs(s - o) / o for s, o in res["decisions"]]
    return (min(gaps) if gaps else np.inf), (min(dec) if dec else np.inf)


# ------------------------------------------------------------------ the inputs
def training(K, Mt, seed=11, noise=1e-3):
    """Columns: rfft of Hann-windowed sums of four sinusoids plus noise."""
    rng = np.random.default_rng(seed)
    M = 2 * (K - 1)
    n = np.arange(M)
    g = 0.5 - 0.5 * np.cos(TWO_PI * n / M)
    cols = []
    for _ in range(Mt):
        f = rng.uniform(0.02, 0.45, 4)
        a = rng.uniform(0.2, 1.0, 4)
        p = rng.uniform(0, TWO_PI, 4)
        x = sum(ai * np.sin(TWO_PI * fi * n + pi) for ai, fi, pi in zip(a, f, p))
        cols.append(np.fft.rfft(g * (x + noise * rng.standard_normal(M))))
    return np.stack(cols, axis=1)


def zeroed(K, Mt):
    X = training(K, Mt).copy()
    X[K // 2] = 0.0
    X[:, Mt // 3] = 0.0
    return X


# name: (X factory, learn() arguments)
CASES = {
    "k5_m1": (lambda: training(5, 1), dict(level_init=0.05, cnt_max=4)),
    "k5_m3": (lambda: training(5, 3), dict(level_init=0.05, cnt_max=4)),
    "k17_m24": (lambda: training(17, 24), dict(level_init=0.05, cnt_max=6)),
    "k65_m67": (lambda: training(65, 67), dict(level_init=0.02, cnt_max=3, max_iters=4000)),
    "k33_m300": (lambda: training(33, 300), dict(level_init=0.02, cnt_max=3, max_iters=4000)),
    "zero_row_col": (lambda: zeroed(17, 24), dict(level_init=0.05, cnt_max=4)),
    "tiny_level": (lambda: training(17, 24), dict(level_init=1e-4, cnt_max=3)),
    "level_quarter": (lambda: training(17, 24), dict(level_init=0.25, cnt_max=4)),
    # too few iterations to solve the subproblem: the 11th update ends up worse and is
    # undone, so is the 12th at half the level; the 13th, at a quarter, is kept
    "reject": (lambda: training(17, 24), dict(level_init=0.05, cnt_max=14, max_iters=50, check=50)),
    "largest": (lambda: training(1025, 40), dict(level_init=0.02, cnt_max=1, max_iters=200)),
}
CONVERGES = ("k5_m1", "k5_m3", "k17_m24", "zero_row_col", "tiny_level", "level_quarter")
GAP_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def case_input(name):
    X = CASES[name][0]()
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def case_reference(name, formulation=1, float32=False):
    X = case_input(name)
    if float32:
        X = X.astype(np.complex64).astype(np.complex128)
    return learn(X, gap_tol=GAP_TOL, formulation=formulation, **CASES[name][1])


# ------------------------------------------------------------- training frames
def training_frames(x, observed, w, a, M, context=None):
    """-> (X [K, n] = the dgt columns (periodic Hann, 'timeinv') of the frames
    whose w samples are all inside the signal and observed, frame indices);
    context c: only those within c frames of one that holds a missing sample
    (in time: the circular wrap does not count)."""
    import spain_learned_ref as S
    Ls = len(x)
    L = max(1, -(-Ls // M)) * M
    xp, ok = np.zeros(L), np.zeros(L, bool)
    xp[:Ls] = np.where(observed, x, 0.0)
    ok[:Ls] = observed
    N = L // a
    t = np.arange(N)[:, None] * a - w // 2 + np.arange(w)[None, :]       # [N, w], not wrapped
    inside = (t[:, 0] >= 0) & (t[:, -1] < Ls)
    good = inside & ok[t % L].all(axis=1)
    if context is not None:
        missing = np.zeros(L, bool)
        missing[:Ls] = ~np.asarray(observed, bool)
        real = (t >= 0) & (t < Ls)                     # a wrapped sample is not near in time
        touch = np.flatnonzero((missing[t % L] & real).any(axis=1))
        near = np.zeros(N, bool)
        for n in touch:
            near[max(0, n - context):n + context + 1] = True
        good &= near
    frames = np.flatnonzero(good)
    g, _ = S.windows(w, a, M)
    return S.dgt(xp, g, a, M)[:, frames], frames
