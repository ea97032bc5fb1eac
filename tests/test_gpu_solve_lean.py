"""The lean solve path (CFDH_SOLVE_LEAN, default on) against the general one (CFDH_SOLVE_LEAN=0) on one GPU: the Krylov product that
reuses the preconditioner's coupling product, the one-read-back prologue and epilogue of a linear solve, the merged read-backs of
the Newton iteration, and the re-launch after a re-orthogonalisation under launch-ahead.

Meshes: the DFG channel at m = 6 (tests/golden/dfg_m6.npz), the lid cavity at nx = 16 (289 nodes, 867 unknowns: an odd vector
length, singular pressure) and at nx = 128 (16 641 nodes, above the 16 384-row threshold of the SELL and graph-replay paths).

Bounds: the product is compared row by row within the fp64 summation bound (3 nnz_row + 3) eps sum |a_ij| |z_j| (both kernels sum
the row's 3 nnz_row products in some order, then add at most three partial results); whole steps at the tight tolerances within
twice the 1e-9 the tight-step parity test (tests/test_gpu_parity.py) allows between the GPU and the oracle."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from util import lid_case, load_golden, make_ctx

pytestmark = pytest.mark.gpu

TIGHT = dict(snes_rtol=1e-12, snes_stol=0.0, ksp_rtol=1e-10)
PARITY = 1e-9  # tests/test_gpu_parity.py: converged tight step, GPU against the oracle
EPS = np.finfo(np.float64).eps

CASES = {
    "dfg6": lambda: load_golden("dfg_m6")[0],
    "lid16": lambda: lid_case(16),
    "lid128": lambda: lid_case(128),
}


class _env:
    """Environment variables for the contexts created (and the solves run) inside the block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ctx(case, opts):
    ctx = make_ctx(case)
    o = ctx.default_options()
    for k, v in opts.items():
        setattr(o, k, v)
    ctx.set_options(o)
    nv = case.nv
    ctx.set_state(u_prev=np.zeros(2 * nv), p_prev=np.zeros(nv), u=np.zeros(2 * nv), p=np.zeros(nv))
    return ctx


COUNTERS = {"host_sync": 15, "cycles": 84, "projections": 86, "iter_sync": 87, "guess_used": 70, "discarded": 73}
GRAM = {"rank": 88, "k": 89}  # of the last projected guess of a step


def _step(ctx, rec):
    before = {k: ctx.info(i) for k, i in COUNTERS.items()}
    st = ctx.solve_step()
    assert st.reason > 0
    for k, i in COUNTERS.items():
        rec.setdefault(k, []).append(ctx.info(i) - before[k])
    for k, i in GRAM.items():
        rec.setdefault(k, []).append(ctx.info(i))
    rec.setdefault("newton", []).append(int(st.newton_its))
    rec.setdefault("krylov", []).append(int(st.krylov_its))
    rec.setdefault("ksp_its", []).append([int(v) for v in ctx.newton_history()["ksp_its"]])


def run_steps(case, nsteps, opts, repeat=0, keep=False):
    """nsteps time steps from rest, then `repeat` more solves of the last step from the identical state (same previous step, same
    initial iterate): the corrections they keep duplicate the ones the ring holds already."""
    ctx = _ctx(case, opts)
    rec = {}
    nv = case.nv
    start = (np.zeros(2 * nv), np.zeros(nv))
    for s in range(nsteps):
        _step(ctx, rec)
        if s + 1 < nsteps or repeat == 0:
            ctx.advance()
            start = ctx.get_solution()
    for _ in range(repeat):
        ctx.set_state(u=start[0], p=start[1])
        _step(ctx, rec)
    rec["x"] = np.concatenate(ctx.get_solution())
    rec["info70"], rec["info71"], rec["info72"] = ctx.info(70), ctx.info(71), ctx.info(72)
    rec["discarded"] = ctx.info(73)
    rec["lean"] = ctx.info(85)
    if keep:
        rec["ctx"] = ctx
    else:
        ctx.close()
    return rec


@functools.lru_cache(maxsize=None)
def _run(key, lean, tight, nsteps=3, repeat=0, check=False, fresh=0):  # fresh: a run of its own behind the cache
    with _env(CFDH_SOLVE_LEAN=1 if lean else 0, CFDH_GUESS_CHECK="1" if check else None):
        r = run_steps(CASES[key](), nsteps, dict(TIGHT) if tight else {}, repeat=repeat)
    assert r["lean"] == (1 if lean else 0)
    return r


def _operator(key, lean):
    """(J, z, w, J z by cfdh_spmv, singular flag) after one time step on the given path, for a random r."""
    with _env(CFDH_SOLVE_LEAN=1 if lean else 0):
        case = CASES[key]()
        ctx = _ctx(case, {})
        assert ctx.solve_step().reason > 0
        r = np.random.default_rng(7).standard_normal(3 * case.nv)
        z, w = ctx.apply_operator(r)
        ref = ctx.spmv(z)
        J = ctx.get_csr()
        sing = ctx.info(76)
        ctx.close()
    return J, z, w, ref, sing


@pytest.mark.parametrize("key", ["dfg6", "lid128"])
def test_product_with_the_kept_coupling(key):
    J, z, w, ref, sing = _operator(key, True)
    assert sing == (1 if key.startswith("lid") else 0)
    if not sing:
        bound = (3 * J.getnnz(axis=1) + 3) * EPS * (abs(J) @ np.abs(z))
        err = np.abs(w - ref)
        print("%s: max |w - J z| / bound = %.3f, max |w - J z| = %.3e, rows that differ %d of %d"
              % (key, (err / np.maximum(bound, 1e-300)).max(), err.max(), int((err > 0).sum()), err.size))
        assert (err <= bound).all()
    else:
        assert np.array_equal(w, ref)
    J0, z0, w0, ref0, _ = _operator(key, False)
    assert np.array_equal(w0, ref0)  # the general path: the plain product, bit for bit


@pytest.mark.parametrize("key", ["lid16", "lid128"])
def test_singular_case_uses_the_plain_product(key):
    for lean in (True, False):
        J, z, w, ref, sing = _operator(key, lean)
        assert sing == 1
        assert np.array_equal(w, ref)


@pytest.mark.parametrize("key", ["dfg6", "lid16", "lid128"])
def test_prologue(key):
    a, b = _run(key, True, False, 3, 2, True), _run(key, False, False, 3, 2, True)  # the check hook fails the step when it trips
    print("%s: solves from a projected guess per step lean %s general %s; info 71 lean %d general %d"
          % (key, a["guess_used"], b["guess_used"], a["info71"], b["info71"]))
    assert a["info70"] == b["info70"] and a["info70"] > 0
    # info 71 is the mean |r0| / |b| (a relative quantity) as an integer count of 1e-6, its resolution: one unit
    assert abs(a["info71"] - b["info71"]) <= 1
    # the step repeated from the identical state: the ring gains near-duplicates (measured: the solves stop at rtol 1e-5, so the Gram
    # system keeps full rank, 4 of 4, and the guess is used on both paths) -- the same outcome and the same rank for every solve
    assert a["guess_used"] == b["guess_used"] and a["projections"] == b["projections"]
    assert a["newton"] == b["newton"]
    print("%s: rank / size of the last Gram system per step lean %s general %s" % (key, list(zip(a["rank"], a["k"])), list(zip(b["rank"], b["k"]))))
    assert a["rank"] == b["rank"] and a["k"] == b["k"]


@pytest.mark.parametrize("key", ["dfg6", "lid16", "lid128"])
def test_whole_steps_tight(key):
    a, b = _run(key, True, True), _run(key, False, True)
    d = np.linalg.norm(a["x"] - b["x"]) / np.linalg.norm(b["x"])
    print("%s: |x_lean - x_general| / |x| = %.3e, Newton %s / %s, Krylov %s / %s" % (key, d, a["newton"], b["newton"], a["krylov"], b["krylov"]))
    assert a["newton"] == b["newton"]
    assert d <= 2 * PARITY


@pytest.mark.parametrize("key", ["dfg6", "lid128"])
def test_krylov_iterations_at_default_tolerances(key):
    b, b2 = _run(key, False, False), _run(key, False, False, fresh=1)
    assert b["ksp_its"] == b2["ksp_its"], "the general path is not stable over these steps"
    a = _run(key, True, False)
    print("%s: Krylov iterations per solve lean %s general %s" % (key, a["ksp_its"], b["ksp_its"]))
    assert a["newton"] == b["newton"]
    assert a["ksp_its"] == b["ksp_its"]
    assert a["info72"] == 0 and b["info72"] == 0


@pytest.mark.parametrize("key", ["dfg6", "lid16", "lid128"])
def test_read_back_counts(key):
    a, b = _run(key, True, False), _run(key, False, False)
    for s in range(3):
        # per solve outside its iterations: one read-back when a guess is projected (|b| comes from the Newton iteration), one per
        # cycle for the true residual; one per Newton iteration (line search); one per step (|F| and the null-space test)
        want = a["iter_sync"][s] + a["projections"][s] + a["cycles"][s] + a["newton"][s] + 1
        print("%s step %d: read-backs lean %d (formula %d) general %d" % (key, s, a["host_sync"][s], want, b["host_sync"][s]))
        assert a["host_sync"][s] == want
        assert a["host_sync"][s] < b["host_sync"][s]


@pytest.mark.parametrize("key", ["dfg6", "lid128"])
def test_refine_under_launch_ahead(key, tmp_path):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_solve_lean_worker.py")
    res = {}
    for lag in (9, 0):
        out = str(tmp_path / ("lag%d.npz" % lag))
        env = dict(os.environ, CFDH_GS_ETA2="0.5", CFDH_KSP_LAG=str(lag), CFDH_SOLVE_LEAN="1")
        subprocess.run([sys.executable, worker, key, "3", "1e-5", out], check=True, env=env, timeout=120)
        res[lag] = np.load(out)
    d = np.linalg.norm(res[9]["x"] - res[0]["x"]) / np.linalg.norm(res[0]["x"])
    print("%s: Krylov per step lag 9 %s lag 0 %s, discarded %d, |dx| / |x| = %.3e"
          % (key, res[9]["krylov"], res[0]["krylov"], int(res[9]["discarded"]), d))
    assert np.array_equal(res[9]["krylov"], res[0]["krylov"]) and np.array_equal(res[9]["newton"], res[0]["newton"])
    assert d <= 2 * PARITY
    assert int(res[9]["discarded"]) > 0


@pytest.mark.parametrize("key", ["dfg6", "lid16", "lid128"])
def test_bitwise_reproducible(key):
    a, b = _run(key, True, False, 2), _run(key, True, False, 2, fresh=1)
    assert a is not b and np.array_equal(a["x"], b["x"])
