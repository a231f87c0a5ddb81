"""GPU tests of S-SPAIN with the OMP coefficient update (csrc/spain_omp.hip
between the gather and the overlap-add of csrc/janssen_windows.hip, through
ainp.spain.spain_inpaint(f_update="omp")) against the float64 NumPy restatement
in tests/spain_omp_ref.py.

Bound of the parity cases: 1e-9 * max|clean gap| on the gap and 1e-9 relative
on the objectives, as tests/test_gpu_spain.py; passes and atoms per pass equal
the reference's in every window, observed samples are bit-equal.  OMP's
decisions are discrete, so that holds only where none is a near-tie;
test_cpu_spain_omp.py asserts that on the reference alone for every case used
here, and that two float64 solvers agree well inside the bound while float32
input misses it.  Every test prints its measured figure; DESIGN §14.3 records
them.  Measured on an MI355X: parity gap <= 1.2e-14 and objectives <= 3.1e-12
over all cases, the largest transform's objectives 2.8e-15, the exact tie's
1.2e-15.
"""
import numpy as np
import pytest
import torch

import janssen_ref as R
import spain_omp_ref as O
import spain_ref as S

pytestmark = pytest.mark.gpu


def _check(out, info, x, mask, s0, e0, ref, tag, gap=True):
    obj, robj = info["objective"], ref["obj"]
    assert obj.shape == robj.shape, (obj.shape, robj.shape)
    fin = np.isfinite(robj)
    assert np.array_equal(np.isfinite(obj), fin) and np.all(np.isnan(obj[~fin]))
    d_obj = np.max(np.abs(obj[fin] - robj[fin]) / robj[fin])
    scale = np.max(np.abs(x[s0:e0]))
    d = np.max(np.abs(out[s0:e0] - ref["out"][s0:e0])) / scale
    print(f"{tag}: gap {d:.3e}, objective {d_obj:.3e}, passes {info['iters']}, most atoms "
          f"{int(info['atoms'].max())}")
    assert info["iters"] == ref["iters"]
    assert info["atoms"].dtype == np.int32 and np.array_equal(info["atoms"], ref["atoms"])
    assert d_obj <= 1e-9
    if gap:
        assert d <= 1e-9
    assert out.dtype == np.float64 and np.array_equal(out[mask], x[mask])


@pytest.mark.parametrize("case,eps,errdb,kw", O.PARITY, ids=O.PARITY_IDS)
def test_parity(case, eps, errdb, kw):
    from ainp.spain import spain_inpaint
    w, a, s0, e0, n = case
    x, mask = S.case_signal(case), S.case_mask(case)
    out, info = spain_inpaint(x, mask, algorithm="sspain", w=w, a=a, epsilon=eps, f_update="omp",
                              omp_errdb=errdb, return_history=True, **kw)
    assert len(info) == 1 and (info[0]["signal"], info[0]["start"], info[0]["end"]) == (0, s0, e0)
    _check(out, info[0], x, mask, s0, e0, O.case_reference(case, eps, errdb, kw),
           f"{case} {eps} {errdb} {kw}")


def test_largest_transform():
    """w 4096, red 2: M 8192, the whole LDS budget, 12 passes of up to 12 atoms.
    What it checks are the 60 objectives and atom counts.  It does not check the
    gap: in 12 passes at this size the smallest objective is the first, so the
    recorded iterate is the gapped block itself on both sides.  Nor does it reach
    the cap of 512 unknowns (test_cap_...), or the least squares beyond 24."""
    from ainp.spain import spain_inpaint
    B = S.BIG
    x, mask = S.big_signal()
    out, info = spain_inpaint(x, mask, algorithm="sspain", w=B["w"], a=B["a"], red=B["red"],
                              maxit=O.BIG_MAXIT, f_update="OMP", return_history=True)
    _check(out, info[0], x, mask, B["s0"], B["e0"], O.big_reference(), "largest", gap=False)


def test_more_unknowns_than_lanes():
    """w 512 runs 256 lanes; 130 atoms a pass are 260 real unknowns, so every
    loop over the unknowns takes a second round."""
    from ainp import ops
    row, obs, g0, h = O.wide_row()
    ref = O.wide_reference()
    kw = {k: v for k, v in O.WIDE.items() if k != "w"}
    sol = torch.from_numpy(row[None].copy()).cuda()
    iters, hist, na = ops.spain_omp(sol, [g0], [h], return_history=True, **kw)
    got, hist, na = sol.cpu().numpy()[0], hist.cpu().numpy()[0], na.cpu().numpy()[0]
    d = np.max(np.abs(got - ref["rec"])) / np.max(np.abs(row))
    d_obj = np.max(np.abs(hist - ref["obj"]) / np.array(ref["obj"]))
    print(f"wide row: row {d:.3e}, objectives {d_obj:.3e}, atoms {na.tolist()}")
    assert iters.tolist() == [2] and na.tolist() == ref["atoms"] == [130, 130]
    assert d <= 1e-9 and d_obj <= 1e-9 and np.array_equal(got[obs], row[obs])
    assert np.any(got[~obs] != 0.0)


def test_an_exact_tie_takes_dc():
    """A unit impulse has a flat spectrum and OMP ranks plain magnitudes: the
    first selection is an exact tie over all M/2 + 1 bins and takes m = 0."""
    from ainp import ops
    row, obs, g0, h = S.tie_row(64)
    for red in (1, 2):
        rec, objs, atoms = O.sspain_omp(row, obs, red=red, epsilon=1e-3, maxit=4)
        assert O.omp(row, 64 * red, 1)[1] == [0]
        # DC alone fits the block's mean; m = 1, which H_1 takes, leaves another objective
        dc = np.linalg.norm(row - row.mean())
        C = O.atom_columns(1, 64, 64 * red)
        alt = np.linalg.norm(row - C @ np.linalg.lstsq(C, row, rcond=None)[0])
        assert abs(alt - dc) > 1e-6 and abs(objs[0] - dc) <= 1e-12
        sol = torch.from_numpy(np.stack([row, row])).cuda()
        iters, hist, na = ops.spain_omp(sol, [g0, g0], [h, h], red=red, epsilon=1e-3, maxit=4,
                                        return_history=True)
        got, hist, na = sol.cpu().numpy(), hist.cpu().numpy(), na.cpu().numpy()
        d_obj = np.max(np.abs(hist[0] - objs) / np.array(objs))
        d = np.max(np.abs(got[0] - rec))
        print(f"red {red}: objectives {d_obj:.3e}, row {d:.3e}, atoms {na[0].tolist()}")
        assert iters.tolist() == [4, 4] and na[0].tolist() == atoms and d_obj <= 1e-9
        assert d <= 1e-9
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0][obs], row[obs])
        # the first pass has one atom, DC: A* z-bar is the constant mean(row)
        assert abs(hist[0, 0] - np.linalg.norm(row - row.mean())) <= 1e-12


def test_all_missing_windows_stay_zero():
    """The 90-sample gap under w = 64 (spain_ref.CASES[3]): windows without an
    observed sample have no row, and the samples they alone cover stay zero."""
    from ainp.spain import spain_inpaint
    case = S.CASES[3]
    w, a, s0, e0, n = case
    x, mask = S.case_signal(case), S.case_mask(case)
    out, info = spain_inpaint(x, mask, algorithm="sspain", w=w, a=a, f_update="omp",
                              return_history=True)
    ref = O.case_reference(case)
    zeros = np.flatnonzero(ref["out"][s0:e0] == 0.0)
    assert len(zeros) > 0 and np.all(out[s0:e0][zeros] == 0.0)
    assert np.count_nonzero(out[s0:e0]) == e0 - s0 - len(zeros)
    print(f"{len(zeros)} samples under all-missing windows alone stay zero")


def test_an_all_zero_row_returns_at_once():
    from ainp import ops
    sol = torch.zeros(3, 128, dtype=torch.float64).cuda()
    sol[1] = torch.from_numpy(S.case_signal(S.CASES[1])[500:628])
    iters, hist, na = ops.spain_omp(sol, [10, 31, 100], [5, 24, 28], maxit=6, epsilon=0.0,
                                    return_history=True)
    hist, na = hist.cpu().numpy(), na.cpu().numpy()
    assert iters.tolist() == [1, 6, 1]
    for row in (0, 2):
        assert hist[row, 0] == 0.0 and np.all(np.isnan(hist[row, 1:]))
        assert na[row].tolist() == [0, -1, -1, -1, -1, -1]
        assert not sol[row].any()
    assert na[1].tolist() == [1, 2, 3, 4, 5, 6] and np.all(np.isfinite(hist[1]))


def test_batch_is_the_separate_calls_and_repeats():
    from ainp.spain import spain_inpaint
    w, a = 128, 32
    sigs = [R.sinusoid_mix(n, noise=1e-3, seed=i) for i, n in enumerate((1500, 1201, 1800))]
    gaps = [((300, 340), (1000, 1001)), ((531, 555), (900, 1000)), ((40, 70), (1700, 1760))]
    masks = []
    for x, gs in zip(sigs, gaps):
        m = np.ones(len(x), bool)
        for s0, e0 in gs:
            m[s0:e0] = False
        masks.append(m)
    kw = dict(algorithm="sspain", w=w, a=a, f_update="omp", return_history=True)
    outs, info = spain_inpaint(sigs, masks, **kw)
    again, info2 = spain_inpaint(sigs, masks, **kw)
    assert [(g["signal"], g["start"], g["end"]) for g in info] == [
        (i, s0, e0) for i, gs in enumerate(gaps) for s0, e0 in gs]
    rows = 0
    for i, (x, m) in enumerate(zip(sigs, masks)):
        assert np.array_equal(outs[i], again[i])
        alone, hist = spain_inpaint(x, m, **kw)
        assert np.array_equal(outs[i], alone), i
        assert np.array_equal(outs[i][m], x[m])
        for g, h in zip([g for g in info if g["signal"] == i], hist):
            assert g["iters"] == h["iters"] and len(g["iters"]) > 0
            assert np.array_equal(g["objective"], h["objective"], equal_nan=True)
            assert np.array_equal(g["atoms"], h["atoms"])
            rows += len(g["iters"])
    for g, g2 in zip(info, info2):
        assert np.array_equal(g["objective"], g2["objective"], equal_nan=True)
        assert np.array_equal(g["atoms"], g2["atoms"])
    plain = spain_inpaint(sigs, masks, algorithm="sspain", w=w, a=a, f_update="OMP")
    assert all(np.array_equal(p, o) for p, o in zip(plain, outs))
    print(f"{rows} windows of 3 signals in one launch give the bits of separate calls")


def test_h_is_what_it_was():
    """f_update "H" is ainp_spain's S-SPAIN and A-SPAIN, bit for bit, and its
    history has no atoms."""
    from ainp import ops
    from ainp.spain import plan_spain_windows, spain_inpaint
    case = S.CASES[1]
    w, a, s0, e0, n = case
    x, mask = S.case_signal(case), S.case_mask(case)
    plan = plan_spain_windows([mask], w, a)
    for alg in S.ALGS:
        out, info = spain_inpaint(x, mask, algorithm=alg, w=w, a=a, f_update="h",
                                  return_history=True)
        old, old_info = spain_inpaint(x, mask, algorithm=alg, w=w, a=a, return_history=True)
        assert np.array_equal(out, old) and "atoms" not in info[0]
        assert np.array_equal(info[0]["objective"], old_info[0]["objective"], equal_nan=True)
        # and the launch below it: the rows of the plan through ops.spain
        dbuf = torch.from_numpy(x.copy()).cuda()
        tabs = plan.tables()
        sol = ops.janssen_windows(dbuf, torch.from_numpy(tabs.missing).cuda(), tabs, plan.w,
                                  plan.a, plan.gana)
        iters, hist = ops.spain(sol, plan.gap_start, plan.gap_len, algorithm=alg,
                                return_history=True)
        assert iters.cpu().tolist() == info[0]["iters"]
        assert np.array_equal(hist.cpu().numpy(), info[0]["objective"], equal_nan=True)
        ref = S.case_reference(case, alg)
        assert info[0]["iters"] == ref["iters"]
        assert np.max(np.abs(out[s0:e0] - ref["out"][s0:e0])) <= 1e-9 * np.max(np.abs(x[s0:e0]))


def test_cap_is_refused_before_any_launch():
    from ainp import ops
    from ainp.spain import spain_inpaint
    x, mask = S.big_signal()
    with pytest.raises(ValueError, match="512 real unknowns"):
        spain_inpaint(x, mask, algorithm="sspain", w=4096, a=1024, f_update="omp", maxit=257)
    sol = torch.zeros(2, 1024, dtype=torch.float64).cuda()
    with pytest.raises(ValueError, match="512 real unknowns"):
        ops.spain_omp(sol, [3, 4], [5, 6], maxit=300)
    # below Python the library refuses it too, naming the rule
    with pytest.raises(RuntimeError, match="512 real unknowns"):
        torch.ops.ainp.spain_omp(sol, torch.tensor([3, 4], dtype=torch.int32).cuda(),
                                 torch.tensor([5, 6], dtype=torch.int32).cuda(), 2, 1, 1, 0.1,
                                 300, -40.0, torch.zeros(2, dtype=torch.int32).cuda(), None, None,
                                 torch.empty(2 * 512 * 513 * 4, dtype=torch.uint8).cuda())
    assert not sol.any()
