"""The reference of tests/test_gpu_scalar_krylov.py, checked on the CPU before the GPU tests lean on it: the reference is
ipcs_krylov_ref.bicgstab with 1-D vectors and the Jacobi weights fl64(1 / diag); at float64 it is scalar_twin.bicgstab_jacobi, the
rounding-spread table and the KMAX per case are what it produces on the twin's matrices, the mid-batch data have convergence
targets, the twin treats exact convergence as the device does, and the data of the edge tests are what those tests say."""
import numpy as np
import pytest
import scipy.sparse as sp

import ipcs_krylov_ref as R
import scalar_twin as T
import scalar_util as U
import test_gpu_scalar_krylov as G

_mats = {}


def mat(key):
    if key not in _mats:
        _mats[key] = G.twin_matrix(key)
    return _mats[key]


def problem(key, extra=0):
    A = mat(key)
    b, x0 = G.data(key, A.shape[0], extra)
    return A, b, x0


@pytest.mark.parametrize("key", G.SMALL, ids=lambda k: "%s-%d" % k)
def test_float64_trajectory_is_the_twin_solver(key):
    """Same iteration count at rtol = 1e-8 on the eight systems and the same final iterate.  The two codes differ in the order of the
    sums inside a matrix row only (scipy's product against reduceat), a few ulp per iteration: the iterates are held to 4 u per
    iteration."""
    A, b, x0 = problem(key)
    xt, its = T.bicgstab_jacobi(A, b, x0, 1e-8)
    tr = R.bicgstab(A, b, x0, its + 2, dtype=np.float64)
    tol = 1e-8 * np.sqrt(np.sum(b * b))
    mine = next(k for k, s in enumerate(tr) if np.sqrt(s["rn2"]) <= tol)
    gap = R.rel(tr[its]["x"], xt)
    print("scalar krylov ref vs twin %s: its %d / %d, final iterate %.2e" % (key, mine, its, gap))
    assert mine == its and 3 <= its <= 100
    assert gap <= 4 * G.UNIT * its


def measure():
    """The rows of KMAX and SPREAD (python -c "import test_scalar_krylov_ref as t; t.measure()")."""
    for key in G.SMALL + G.TINY + G.LARGE:
        A, b, x0 = problem(key)
        kmax, row = 0, None
        for k in range(1, G.KLIM[key[0]] + 1):
            got = R.spread(0, A, b, x0, k)
            if got[1] > G.SPREAD_CAP:
                break
            kmax, row = k, got
        print('    ("%s", %d): KMAX %d  SPREAD (%.1e, %.1e),' % (key[0], key[1], kmax, *row))


@pytest.mark.parametrize("key", list(G.SPREAD), ids=lambda k: "%s-%d" % k)
def test_spread_table_is_what_the_reference_produces(key):
    """The table within a factor 2, below the cap; KMAX is the largest k up to KLIM at which the scalar spread stays below the cap,
    and at least 6 on the small systems, so that every trajectory crosses a batch of 4 launches."""
    A, b, x0 = problem(key)
    k = G.KMAX[key]
    got = R.spread(0, A, b, x0, k)
    print("scalar krylov spread %s: KMAX %d, measured (%.2e, %.2e), table (%.2e, %.2e)" % (key, k, *got, *G.SPREAD[key]))
    for g, t in zip(got, G.SPREAD[key]):
        assert t / 2 <= g <= 2 * t, (key, got, G.SPREAD[key])
        assert t <= G.SPREAD_CAP
    assert 1 <= k <= G.KLIM[key[0]]
    if key in G.SMALL:
        assert k >= 6
    if k < G.KLIM[key[0]]:
        assert R.spread(0, A, b, x0, k + 1)[1] > G.SPREAD_CAP


@pytest.mark.parametrize("key", G.SMALL, ids=lambda k: "%s-%d" % k)
def test_seeds_give_convergence_targets(key):
    A, b, x0 = problem(key, G.MIDBATCH_EXTRA[key])
    tg = G.targets(R.bicgstab(A, b, x0, 8))
    print("scalar krylov mid-batch targets on the CPU %s: %s" % (key, [k for k, _ in tg]))
    assert tg and any(k % 4 for k, _ in tg)


def test_twin_takes_exact_convergence_as_convergence():
    """A = I: the first half step lands on the solution (s = 0, omega = 0, beta = 0 * inf): one iteration, x = b, no NaN; and a
    breakdown above the tolerance (rh . v = 0 in iteration 2) ends the twin's solve where it is instead of looping."""
    rng = np.random.default_rng(51)
    x0, b = rng.integers(-4, 5, size=80).astype(np.float64), rng.integers(-4, 5, size=80).astype(np.float64)
    with np.errstate(all="ignore"):
        x, its = T.bicgstab_jacobi(sp.identity(80, format="csr"), b, x0, 1e-8)
    assert its == 1 and np.array_equal(x, b)
    tr = R.bicgstab(sp.identity(80, format="csr"), b, x0, 1, dtype=np.float64)
    assert tr[1]["omega"] == 0 and tr[1]["rn2"] == 0 and not np.isfinite(tr[1]["beta"])
    A = mat(("rectangle", 1))
    _, fl = G.setup("rectangle")
    b = np.zeros(A.shape[0])
    b[fl["nodes"]] = np.arange(len(fl["nodes"])) % 4 + 1.0
    with np.errstate(all="ignore"):
        x, its = T.bicgstab_jacobi(A, b, np.zeros_like(b), 1e-8)
    tr = R.bicgstab(A, b, np.zeros_like(b), 1, dtype=np.float64)
    assert tr[1]["alpha"] == 1.0 and tr[1]["rho"] == 0.0 and tr[1]["beta"] == 0.0 and tr[1]["rn2"] > 0
    assert its == 2 and not np.isfinite(x).all()   # the twin has no frozen iterate: iteration 2 spreads the NaN


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_one_free_vertex_cases_exist(name):
    found = G.one_free_vertex(name)
    assert found is not None
    ip, v, nodes, vals = found
    print("scalar one free vertex on the CPU %s: params %d, vertex %d" % (name, ip, v))
    assert len(nodes) == G.setup(name)[0].num_vertices - 1 and v not in nodes
