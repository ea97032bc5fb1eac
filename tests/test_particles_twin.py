"""The NumPy twin of the particle step (particles_twin.py) against closed forms, on the CPU.  P1 interpolates an affine field
exactly, so uniform translation, rigid rotation, simple shear and a field that is linear in time have solutions the explicit
midpoint scheme reproduces to rounding on any mesh (particles_util.py holds the cases; test_gpu_particles.py puts the device
through the same ones).  Also here: the tables of the twin, the decisions margin, and the seeds of the random-field comparison,
chosen so that the twin takes no decision closer than 1e-9."""
import numpy as np
import pytest

import particles_twin as T
import particles_util as U


@pytest.mark.parametrize("name", ["square", "stenosis", "cube", "bifurcation"])
def test_tables(name):
    m = U.mesh(name)
    tw = U.twin(m)
    nb, n1 = tw.nb, m.d + 1
    e, f = np.nonzero(nb >= 0)
    back = nb[nb[e, f]]                                   # the neighbour lists e on exactly one of its facets
    assert ((back == e[:, None]).sum(axis=1) == 1).all()
    ext = np.sort(-1 - nb[nb < 0])
    assert np.array_equal(ext, np.arange(len(m.facet_cells)))
    # lambda of the twin's table at the vertices of every cell is the identity
    X = m.x[m.cells]
    g = tw.aff[:, :m.d * m.d].reshape(-1, m.d, m.d)
    lam = np.einsum("cai,cbi->cba", g, X - tw.aff[:, None, m.d * m.d:])  # [cell, vertex b, a - 1]
    assert np.abs(lam - np.eye(n1)[None, :, 1:]).max() <= 1e-12
    # seeds of the helper lie in their cells, with the margin the helper promises
    x0, c0 = U.random_seeds(m, 200, 5)
    assert tw.min_lambda(c0, x0).min() >= 0.02 / n1 - 1e-12


@pytest.mark.parametrize("name", ["square", "cube"])
def test_uniform_translation(name):
    case = U.case_translation(name, 257)
    case["check"](U.result_of_twin(case))


@pytest.mark.parametrize("name", ["square", "cube"])
def test_rigid_rotation(name):
    case = U.case_rotation(name, 65)
    case["check"](U.result_of_twin(case))


@pytest.mark.parametrize("name", ["square", "cube"])
def test_simple_shear(name):
    case = U.case_shear(name, 257)
    case["check"](U.result_of_twin(case))


def test_simple_shear_in_the_stenosed_channel():
    """The same identities on a mesh that is no box: exits through the walls of the narrowing included."""
    m = U.mesh("stenosis")
    gam, dt, nsteps = 40.0, 0.01, 6
    f = U.affine_field(m, np.array([[0.0, gam], [0.0, 0.0]]), np.zeros(2))
    x0, c0 = U.random_seeds(m, 257, 6)
    tw, st = U.twin_run(m, x0, c0, f, f, dt, 2, nsteps)
    age = st["age"]
    assert (st["status"] != 0).any() and (st["status"] == 0).any()
    assert np.abs(st["x"][:, 0] - (x0[:, 0] + gam * x0[:, 1] * age)).max() <= U.TOL * m.size
    assert np.abs(st["exposure"] - U.MU * gam * age).max() <= U.TOL * U.MU * gam * nsteps * dt


@pytest.mark.parametrize("nsub", [1, 2, 5])
@pytest.mark.parametrize("name", ["square", "cube"])
def test_linear_in_time(name, nsub):
    case = U.case_linear_in_time(name, 65, nsub)
    case["check"](U.result_of_twin(case))


@pytest.mark.parametrize("name", ["stenosis", "bifurcation"])
def test_random_field_seeds_keep_clear_of_ties(name):
    """The comparison of the device with the twin may leave out particles whose twin margin is below 1e-9, at most 1 % of them:
    the seeds are chosen so that the twin alone leaves out none, moves about 3 cells per substep and sees every outcome."""
    tc = U.twin_case(name)
    st, m = tc["state"], tc["m"]
    close = st["margin"] < U.MARGIN
    print("%s: %d of %d particles with a margin below 1e-9, smallest %.2e; active %d, exited %d" % (
        name, close.sum(), len(close), st["margin"].min(), (st["status"] == 0).sum(), (st["status"] > 0).sum()))
    assert close.sum() == 0
    # (the bifurcation is some 30 cells long: at 3 cells per substep nobody is left inside after 10 substeps)
    assert (st["status"] > 0).any() and ((st["status"] == 0).any() or name == "bifurcation") and not (st["status"] < 0).any()
    assert len(np.unique(st["status"])) >= 3  # more than one way out
    assert tc["twin"].min_lambda(st["cell"], st["x"]).min() >= -1e-9
    assert not np.array_equal(tc["u_prev"], tc["u_sol"])
    wall = np.unique(m.cells[m.facet_cells])
    assert np.abs(tc["u_prev"][wall]).min() > 0  # not zero on the walls
    h = U.TWIN_DT / U.TWIN_NSUB
    moved = st["path"] / (st["age"] / h) / U.cell_size(m)
    assert 2.0 <= np.median(moved) <= 4.5  # about three cells per substep


def test_walk_cap():
    cc = U.cap_case()
    st = cc["state"]
    lost = st["status"] == -1
    # the others leave through the outlet (marker 3) or run into the wall of the narrowing (marker 4) before the cap
    assert lost.any() and np.isin(st["status"][~lost], (1 + 3, 1 + 4)).all() and (st["status"] == 1 + 3).any()
    assert np.array_equal(st["x"][lost], cc["x0"][lost]) and np.array_equal(st["cell"][lost], cc["c0"][lost])  # frozen at the substep's start
    assert (st["path"][lost] == 0).all() and (st["t_end"][lost] == 0.0).all()
    assert np.median(cc["x0"][lost, 0]) < cc["x0"][st["status"] == 1 + 3, 0].min() + 0.5  # the ones that started furthest from the outlet


def test_a_walk_of_exactly_the_cap_is_allowed():
    """64 crossings end the walk inside a cell, the 65th loses the particle."""
    m = U.mesh("stenosis")
    tw = U.twin(m)
    x0, c0 = U.random_seeds(m, 40, 8, keep=lambda c: c[:, 0] < 1.0)
    L = m.x[:, 0].max()
    counts = set()
    for x, c in zip(x0, c0):
        for frac in np.linspace(0.5, 0.99, 25):
            y = [x[0] + frac * (L - x[0]), x[1]]
            crossings = 0
            r = tw.walk(x.tolist(), y, int(c))[0]
            # count by walking again with the cap lifted
            cap, T.MAX_CROSSINGS = T.MAX_CROSSINGS, 10 ** 6
            try:
                cc = int(c)
                while True:
                    ly = tw.lam(cc, y)
                    if not any(v < -T.TOL_INSIDE for v in ly):
                        break
                    lx = tw.lam(cc, x.tolist())
                    ts = [(lx[f] / (lx[f] - ly[f]), f) for f in range(3) if ly[f] < -T.TOL_INSIDE]
                    nbr = tw._nb[cc][min(ts)[1]]
                    if nbr < 0:
                        crossings = -1
                        break
                    cc, crossings = nbr, crossings + 1
            finally:
                T.MAX_CROSSINGS = cap
            if crossings < 0:
                continue
            counts.add(crossings)
            assert (r == T.LOST) == (crossings > T.MAX_CROSSINGS)
    assert any(c > T.MAX_CROSSINGS for c in counts) and any(0 < c <= T.MAX_CROSSINGS for c in counts)
