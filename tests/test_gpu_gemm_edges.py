"""Element-wise tests of every GEMM route (csrc/gemm.hip, csrc/gemm16.hip,
csrc/gemm_x6r.hip behind csrc/gemm_route.h) and of the two copy kernels against
the float64 reference of tests/gemm_ref.py, at the shapes where each tiling
changes, in every layout the entry points take.  test_cpu_gemm_ref.py pins the
reference to torch.matmul, proves the conditions of the integer data, checks
the worker's memory layouts against the header and which kernel every case
reaches.

Integer cases (gemm_edge_worker.run_int): every output torch.equal to the
float64 result.  Operands and outputs are views into larger NaN-filled buffers
with ld above the extent, a guard row before and after and a guard slab after
the last split-K slab: nothing outside the output is written, everything inside
is finite (beta == 0 starts from NaN), a read past an operand shows as NaN.  A
call the header refuses must be refused with its message; the stream-K cases
are what ainp_gemm_f32_workspace says they are and give the same bits twice;
the 256 x 256 cases sit on the tile ainp_gemm_bf16nt_tile names.

Real and cancellation cases: gan_glue_ref.within_floor on every output (the
largest deviation from float64 at most 4 x that of the float32 torch evaluation
of the same reference plus 4e-7 of the reference's largest magnitude); for the
bf16 routes both references take the bf16-rounded operands.  Each check prints
what it measured; DESIGN.md ("Edge-shape tests") keeps the largest.

The routes that gemm_env() selects once per process run their integer cases in
a fresh child each (gemm_edge_worker.py as a script), one after the other.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import gemm_edge_worker as Wk
import gemm_ref as R

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_edge_worker.py")
# a clean child takes 2.2-2.8 s on the MI355X, Python's and torch's start-up
# included; 5 x the slowest is 14 s, and 60 s is the least a child gets
CHILD_TIMEOUT = 60


@pytest.fixture(scope="module")
def ops():
    from ainp import ops as _ops
    return _ops


def _guarded(fn, *args, **kw):
    """A HIP error ends the session: nothing more runs on that GPU."""
    try:
        return fn(*args, **kw)
    except RuntimeError as e:
        pytest.exit(f"GPU error, the session ends here: {str(e)[:300]}", returncode=3)


def _report(fails):
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails)


@pytest.mark.parametrize("spec", R.SPECS)
def test_integer_cases_every_element(ops, spec):
    tally = {}
    cases = R.int_cases(spec)
    fails = _guarded(Wk.run_int, ops, cases, tally=tally)
    print(f"{spec}: {len(cases)} cases {tally}")
    refused = sum(1 for c, _ in cases if Wk.refusal(c))
    assert spec == "copy" or (tally.get("refused", 0) == refused and
                              tally.get("served", 0) == len(cases) - refused) or fails
    _report(fails)


REAL = ["f32:x6", "f32:exact", "f32:bf16", "bf16nt", "bf16multi", "x6nt", "x6multi"]


@pytest.mark.parametrize("spec", REAL)
def test_real_cases_within_floor(ops, spec):
    worst = {}
    cases = Wk.real_cases("real:" + spec)
    assert len(cases) >= 2
    fails = _guarded(Wk.run_real, ops, cases, worst)
    for k, v in worst.items():
        print(f"WORST real {k}: share {v[0]:.2f} analytic share {v[1]:.2f}")
    _report(fails)


@pytest.mark.parametrize("spec", ["f32:x6", "x6nt", "x6multi"])
def test_cancellation_cases_within_floor(ops, spec):
    """The six cross terms of the split-bf16 loop, one carried by each of the
    three data sets (test_cpu_gemm_ref.py shows which, and by how much a loop
    without it misses the rule)."""
    worst = {}
    cases = Wk.real_cases("cancel:" + spec)
    assert len(cases) == len(R.CANCEL_KINDS)
    fails = _guarded(Wk.run_real, ops, cases, worst)
    for k, v in worst.items():
        print(f"WORST cancel {k}: share {v[0]:.2f} analytic share {v[1]:.2f}")
    _report(fails)


# ------------------------------------------------------------------ child processes
_ended_badly = []


@pytest.mark.parametrize("name", list(R.CHILD_SETTINGS))
def test_env_switched_routes_in_a_fresh_process(name, tmp_path):
    """One child per setting, one after the other; the inherited environment
    plus the one variable.  A child that ends by signal, abort or time limit
    fails, and no later child is started on that GPU."""
    if _ended_badly:
        pytest.fail(f"an earlier child ended badly ({_ended_badly[0]}): nothing more is started "
                    "on a GPU that has just faulted")
    var, val, _, specs = R.CHILD_SETTINGS[name]
    out = tmp_path / "failures.json"
    t0 = time.time()
    try:
        proc = subprocess.run([sys.executable, WORKER, str(out), *specs],
                              env=dict(os.environ, **{var: val}), timeout=CHILD_TIMEOUT,
                              capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _ended_badly.append(f"{var}={val}: time limit of {CHILD_TIMEOUT} s")
        pytest.fail(_ended_badly[0])
    print(f"{var}={val}: {time.time() - t0:.1f} s; {proc.stdout.strip().splitlines()[-1:]}")
    if proc.returncode not in (0, 1) or not out.exists():
        _ended_badly.append(f"{var}={val}: exit status {proc.returncode}")
        pytest.fail(_ended_badly[0] + "\n" + proc.stderr[-2000:])
    fails = json.loads(out.read_text())
    assert isinstance(fails, list) and (proc.returncode == 0) == (not fails)
    _report(fails)
