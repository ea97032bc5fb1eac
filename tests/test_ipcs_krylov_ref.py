"""The extended-precision recurrences of tests/ipcs_krylov_ref.py, checked on the CPU before the GPU tests lean on them: at
float64 they are the solvers of tests/ipcs_twin.py, they converge to direct solutions, the flexible variant with a symmetric
preconditioner is plain PCG -- and the rounding-spread table of tests/test_gpu_ipcs_krylov.py is what they produce."""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

import ipcs_krylov_ref as R
import ipcs_twin as T
import test_gpu_ipcs_krylov as G

U = 2.0 ** -53
_mats = {}


def mats(name):
    if name not in _mats:
        _mats[name] = G.twin_matrices(name)
    return _mats[name]


def problem(which, name, extra=0):
    A = mats(name)[which]
    d = 2 if name.startswith("sq") else 3
    shape = (A.shape[0],) if which == 1 else (A.shape[0], d)
    b, x0 = G.data(which, name, shape, singular=name.startswith("sq"), extra=extra)
    return A, b, x0


@pytest.mark.parametrize("name", ["sq8", "cube4"])
@pytest.mark.parametrize("which", [0, 2])
def test_float64_trajectories_are_the_twin_solvers(which, name):
    """Same iteration count at rtol = 1e-8 and the same final iterate.  The two codes differ in the order of the sums inside a
    matrix row only (scipy's product against reduceat), a few ulp per iteration: the iterates are held to 4 u per iteration."""
    A, b, x0 = problem(which, name)
    xt, its = (T.bicgstab_jacobi if which == 0 else T.cg_jacobi)(A, b, x0, 1e-8)
    tr = R.DRIVERS[which](A, b, x0, its + 2, dtype=np.float64)
    tol = 1e-8 * np.sqrt(np.sum(b * b))
    mine = next(k for k, s in enumerate(tr) if np.sqrt(s["rn2"]) <= tol)
    gap = R.rel(tr[its]["x"], xt)
    print("ipcs krylov ref vs twin, %s %s: its %d / %d, final iterate %.2e" % (G.NAMES[which], name, mine, its, gap))
    assert mine == its and 3 <= its <= 100
    assert gap <= 4 * U * its


@pytest.mark.parametrize("name", ["sq8", "cube4"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_trajectories_converge_to_direct_solutions(which, name):
    A, b, x0 = problem(which, name)
    if which == 1:   # Jacobi stands in for the V-cycle; the singular 2-D problem is compared without its constant
        tr = R.fpcg(A, b, x0, 150, pre=1.0 / A.diagonal())
    else:
        tr = R.DRIVERS[which](A, b, x0, 80)
    # no stopping test in the recurrences: the iterate of the smallest recurrence residual (later ones drift on rounding noise)
    x = np.asarray(min(tr, key=lambda s: s["rn2"])["x"], dtype=np.float64)
    if which == 1 and name == "sq8":
        import scipy.sparse as sp
        one = np.ones((A.shape[0], 1))
        xs = spl.splu(sp.bmat([[A, one], [one.T, None]]).tocsc()).solve(np.append(b, 0.0))[:-1]
        x, xs = x - x.mean(), xs - xs.mean()
    else:
        xs = spl.splu(A.tocsc()).solve(b)
    assert np.abs(x - xs).max() <= 1e-11 * np.abs(xs).max()


@pytest.mark.parametrize("name", ["sq8", "cube4"])
def test_flexible_pcg_with_a_symmetric_preconditioner_is_pcg(name):
    """With an exactly symmetric `pre`, -alpha (q . z) / rz = (r_new . z_new) / rz: same iterates; the flexible variant holds after
    iteration k the beta and rz that plain PCG held after k - 1."""
    A, b, x0 = problem(2, name)
    w = 1.0 / A.diagonal()
    a, f = R.pcg(A, b, x0, 10, pre=w), R.fpcg(A, b, x0, 10, pre=w)
    for k in range(1, 11):   # two extended-precision runs: they agree below what a float64 comparison can resolve (u / 2)
        assert R.rel(f[k]["x"], a[k]["x"]) <= U / 2 and R.rel(f[k]["alpha"], a[k]["alpha"]) <= U / 2
        assert R.rel(f[k]["beta"], a[k - 1]["beta"]) <= U / 2 and R.rel(f[k]["rz"], a[k - 1]["rz"]) <= U / 2
        assert R.rel(f[k]["p"], a[k - 1]["p"]) <= U / 2


def test_omega_is_zero_when_t_vanishes():
    """x0 such that s = r - alpha v vanishes after the first half step (a 1 x 1 system): t . t = 0 gives omega = 0, not NaN."""
    import scipy.sparse as sp
    tr = R.bicgstab(sp.csr_matrix(np.array([[2.0]])), np.array([1.0]), np.array([0.0]), 1)
    assert tr[1]["omega"] == 0 and float(tr[1]["x"][0]) == 0.5 and tr[1]["rn2"] == 0


def measure_spreads():
    """The rows of drivers 0 and 2 of test_gpu_ipcs_krylov.SPREAD (python -c "import test_ipcs_krylov_ref as t; t.measure_spreads()")."""
    out = {}
    for (which, name) in G.SPREAD:
        if which != 1:
            A, b, x0 = problem(which, name)
            out[(which, name)] = R.spread(which, A, b, x0, G.KMAX[name])
            print('    (%d, "%s"): (%.1e, %.1e),' % (which, name, *out[(which, name)]))
    return out


@pytest.mark.parametrize("key", [k for k in G.SPREAD if k[0] != 1], ids=lambda k: "%s-%s" % (G.NAMES[k[0]], k[1]))
def test_spread_table_is_what_the_reference_produces(key):
    which, name = key
    A, b, x0 = problem(which, name)
    got = R.spread(which, A, b, x0, G.KMAX[name])
    print("ipcs krylov spread %s %s: measured (%.2e, %.2e), table (%.2e, %.2e)" % (G.NAMES[which], name, *got, *G.SPREAD[key]))
    for g, t in zip(got, G.SPREAD[key]):
        assert t / 2 <= g <= 2 * t, (key, got, G.SPREAD[key])
        assert t < G.SPREAD_CAP


@pytest.mark.parametrize("which", [0, 2])
def test_seeds_give_three_convergence_targets(which):
    found = []
    for name, extra in G.MIDBATCH[which]:
        A, b, x0 = problem(which, name, extra)
        tr = R.DRIVERS[which](A, b, x0, 8)
        bn = np.linalg.norm(b)
        found += [(name, extra, k) for k, tol in G.midbatch_targets(tr) if tol / bn < 1]
    print("ipcs krylov mid-batch targets on the CPU, %s: %s" % (G.NAMES[which], found))
    assert len(found) >= 3 and any(k % 4 for _, _, k in found)
