"""The host-side checks of tests/fgmres_ref.py on the CPU: the float64 twin of the FGMRES cycle satisfies the six invariants, the
orthogonality constants the GPU test uses are re-measured against the recorded table, and a trace with one of four driver
mistakes fails the matching invariant although the restarted solve still converges (no GPU)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import fgmres_ref as R

SEED = 20261020
NG = 20          # grid: NG x NG unknowns
COLUMNS = 40


def convection_diffusion(ng, peclet, swirl, rng):
    """Upwinded convection-diffusion on the unit square, Dirichlet boundary eliminated: non-symmetric, diagonally dominant;
    wind (1, 0.5) + swirl x rotation about the centre, with a random 10 % variation of the diffusion coefficient per row."""
    h = 1.0 / (ng + 1)
    idx = np.arange(ng * ng).reshape(ng, ng)
    rows, cols, vals = [], [], []
    for i in range(ng):
        for j in range(ng):
            x, y = (i + 1) * h, (j + 1) * h
            wx, wy = 1.0 - swirl * (y - 0.5), 0.5 + swirl * (x - 0.5)
            d = (1.0 + 0.1 * rng.uniform(-1, 1)) / peclet
            diag = 4 * d / h ** 2 + (abs(wx) + abs(wy)) / h
            rows.append(idx[i, j]); cols.append(idx[i, j]); vals.append(diag)
            for di, dj, w in ((1, 0, wx), (-1, 0, -wx), (0, 1, wy), (0, -1, -wy)):
                ii, jj = i + di, j + dj
                if 0 <= ii < ng and 0 <= jj < ng:
                    rows.append(idx[i, j]); cols.append(idx[ii, jj]); vals.append(-d / h ** 2 - max(-w, 0.0) / h)
    return sp.csr_matrix((vals, (rows, cols)), shape=(ng * ng, ng * ng))


def preconditioner(A, kind):
    if kind == "jacobi":
        dinv = 1.0 / A.diagonal()
        return lambda v: dinv * v
    ilu = spla.spilu(A.tocsc(), drop_tol=1e-2, fill_factor=2.0, permc_spec="NATURAL", diag_pivot_thresh=0.0)
    return lambda v: ilu.solve(v)


OPERATORS = [(10.0, 0.0), (50.0, 2.0), (200.0, 0.0), (200.0, 6.0)]   # (Peclet number, swirl)
ORTH_CASES = [(op, pc, order) for op in range(4) for pc in ("jacobi", "ilu") for order in ("natural", "permuted")]


def problem(op):
    rng = np.random.default_rng(SEED + op)
    A = convection_diffusion(NG, *OPERATORS[op], rng)
    b = 3.0 * rng.standard_normal(A.shape[0])
    return A, b, rng


def kappa64(A, tr, cols):
    """2-norm condition number of [r_start, A z_0 .. A z_{cols-1}] with unit columns"""
    K = np.column_stack([tr["beta"] * tr["V"][0], (A @ tr["Z"][:cols].T)])
    K = K / np.linalg.norm(K, axis=0)
    s = np.linalg.svd(K, compute_uv=False)
    return s[0] / s[-1]


def measure(fp32):
    unit = R.U32 if fp32 else R.EPS
    worst, least, used = 0.0, np.inf, 0
    for op, pc, order in ORTH_CASES:
        A, b, rng = problem(op)
        perm = rng.permutation(len(b)) if order == "permuted" else None
        tr = R.twin_cycle(A, preconditioner(A, pc), b, np.zeros(len(b)), COLUMNS, fp32=fp32, perm=perm)
        for cols in range(3, COLUMNS + 1):
            uk2 = unit * kappa64(A, tr, cols) ** 2
            if uk2 >= 0.1:
                break
            q = R.eps_v(tr["V"][:cols + 1]) / uk2
            worst, least, used = max(worst, q), min(least, q), used + 1
    return worst, least, used


@pytest.mark.parametrize("key", ["fp64", "fp32"])
def test_orthogonality_table_is_current(key):
    worst, least, used = measure(key == "fp32")
    print("%s: eV / (unit kappa^2) between %.3g and %.3g over %d prefixes; recorded %.3g" % (key, least, worst, used, R.ORTH_TABLE[key]))
    assert used >= 50
    # recorded = the maximum rounded up to two digits: a stale table shows as a measurement above it or well below it
    assert 0.8 * R.ORTH_TABLE[key] <= worst <= R.ORTH_TABLE[key]


@pytest.mark.parametrize("refine,fp32", [(None, False), ("all", False), ("dgks", False), (None, True)])
@pytest.mark.parametrize("op,pc", [(1, "jacobi"), (3, "ilu")])
def test_twin_satisfies_the_invariants(op, pc, refine, fp32):
    A, b, rng = problem(op)
    k = 12
    tr = R.twin_cycle(A, preconditioner(A, pc), b, 0.01 * rng.standard_normal(len(b)), k, refine=refine, fp32=fp32)
    S = R.System(A)
    R.check_cycle(S, b, tr, refined=refine is not None, label="twin op %d %s %s fp32=%d" % (op, pc, refine, fp32))
    if refine == "all":
        assert tr["second_pass"].all()


# the driver mistakes, the cycle they are made in, and the invariant that has to see each
MISTAKES = [("stale_h", 0, "I1"), ("hnorm", 0, "I1"), ("zshift", 0, "I4"), ("v0", 1, "I2")]


@pytest.mark.parametrize("bug,cycle,sees", MISTAKES)
def test_checks_see_what_the_converged_answer_hides(bug, cycle, sees):
    A, b, rng = problem(1)
    pre = preconditioner(A, "jacobi")
    S = R.System(A)
    m, rtol = 10, 1e-8
    kw = dict(refine="all" if bug == "hnorm" else None)
    x_ok, betas_ok, traces_ok = R.twin_solve(A, pre, b, m, rtol, **kw)
    x_bad, betas_bad, traces_bad = R.twin_solve(A, pre, b, m, rtol, bug=bug, bug_cycle=cycle, **kw)
    bn = np.linalg.norm(b)
    # end to end nothing shows: both solves converge to the tolerance, and the answers agree to what the tolerance allows
    assert betas_ok[-1] <= rtol * bn and betas_bad[-1] <= rtol * bn
    assert len(traces_ok) >= 3
    smin = np.linalg.svd(A.toarray(), compute_uv=False)[-1]
    assert np.linalg.norm(x_bad - x_ok) <= 2 * rtol * bn / smin
    print("%s: cycles %d against %d" % (bug, len(traces_bad), len(traces_ok)))

    def ratios(tr):
        r2 = R.i2_start(S, b, tr)
        r5 = R.i5_optimal(S, b, tr)
        return {"I1": R.i1_arnoldi(S, tr), "I2": max(r2), "I3": R.i3_lsq(tr), "I4": R.i4_update(tr), "I5": np.inf if r5 is None else max(r5)}

    good, bad = ratios(traces_ok[cycle]), ratios(traces_bad[cycle])
    print("   clean %s\n   %s %s" % (good, bug, bad))
    assert all(v <= 1.0 for v in good.values())
    assert bad[sees] > 10.0        # far outside the bound, not a near miss
    if bug in ("stale_h", "hnorm", "zshift", "v0"):
        assert bad["I5"] > 1.0     # and the iterate is not the minimiser (or the basis is no basis): I5 has nothing good to say
