"""The point sampler on the device (cfdh_sample_*, csrc/cfdh_sample.hip): location against connectivity and against the brute-force
twin (sample_twin.py), sampling of affine fields against their closed form and of random fields against the twin, the series, the
means, repeatability, every refusal and state error, the untouched flow step, and the scenario / command-line routes.

Point counts 1, 63, 64, 65, 257 and 1000 (wave and workgroup edges); meshes of 1 to 6288 cells; grids of 625 to about 3500 nodes, most
of them outside the domain.  Every comparison prints its error next to its bound before it asserts."""
import os

import numpy as np
import pytest

import sample_twin as T
import sample_util as U
from cfd_hemodynamic_amd import _lib
from util import dfg_case, make_ctx

pytestmark = pytest.mark.gpu

INFO = (_lib.INFO_SAMPLE_POINTS, _lib.INFO_SAMPLE_LOCATED, _lib.INFO_SAMPLE_LAUNCHES, _lib.INFO_SAMPLE_SERIES_ROWS)
_CTX = {}


def set_state(ctx, m, u, p):
    u, p = np.ascontiguousarray(u).ravel(), np.ascontiguousarray(p).ravel()
    ctx.set_state(u_prev=u, p_prev=p, u=u, p=p)


def context(m, state=None):
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    ctx.set_params(0.01, 1.06e-3, 3.5e-3)
    if state is not None:
        set_state(ctx, m, *state)
    return ctx


def shared(name):
    """One context per mesh for the tests that only set points, a state, and read."""
    if name not in _CTX:
        _CTX[name] = context(U.mesh(name))
    return _CTX[name]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()


def infos(ctx):
    return tuple(ctx.info(w) for w in INFO)


def check_location(m, ctx, pts, want, what):
    """The device's location of `pts` against the expected cells, the twin's rows and the two identities."""
    ctx.sample_set_points(pts)
    cell, lam, x = ctx.sample_location()
    assert cell.dtype == np.int32 and lam.shape == (len(pts), m.d + 1) and np.array_equal(x, pts)
    assert np.array_equal(cell, want), "%s: %d cells differ" % (what, (cell != want).sum())
    assert ctx.info(_lib.INFO_SAMPLE_POINTS) == len(pts) and ctx.info(_lib.INFO_SAMPLE_LOCATED) == (want >= 0).sum()
    assert U.worst(what + " lambda", lam, T.lambda_in(m.x, m.cells, pts, want), U.TOL_LAMBDA)
    inside = want >= 0
    assert (lam[~inside] == 0.0).all()
    if inside.any():
        assert U.worst(what + " sum", lam[inside].sum(axis=1), 1.0, U.TOL_EXACT)
        assert U.worst(what + " lam.X", np.einsum("na,nai->ni", lam[inside], m.x[m.cells[cell[inside]]]), pts[inside], U.TOL_EXACT * m.size)
    return cell, lam


# --------------------------------------------------------------------------------------------------------------------- location
@pytest.mark.parametrize("n", U.COUNTS)
@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_seeds_in_known_cells(name, n):
    m = U.mesh(name)
    pts, want = U.seeds(m, n)
    check_location(m, shared(name), pts, want, "seeds")


@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_vertices_and_facet_midpoints(name):
    """One answer on a vertex (valence up to 24 on the cube) and on a face: the lowest-indexed cell, taken from `cells`."""
    m = U.mesh(name)
    vp, ve = U.vertex_points(m)
    cell, lam = check_location(m, shared(name), vp, ve, "vertices")
    assert (np.sort(lam, axis=1)[:, -1] == 1.0).all() and (np.sort(lam, axis=1)[:, :-1] == 0.0).all()  # the unit row of a vertex
    assert np.array_equal(m.cells[cell, lam.argmax(axis=1)], np.arange(m.nv))
    fp, fe = U.facet_points(m)
    if len(fp):
        check_location(m, shared(name), fp, fe, "facets")


@pytest.mark.parametrize("name", U.MESHES)
def test_points_outside(name):
    """Beyond the bounding box on each side, and inside the box but outside the domain: -1."""
    m = U.mesh(name)
    pts = U.outside_box(m)
    if name in ("stenosis", "bifurcation"):
        pts = np.vstack([pts, U.outside_domain(name)])
        assert len(pts) >= 100
    check_location(m, shared(name), pts, np.full(len(pts), -1, dtype=np.int32), "outside")


@pytest.mark.parametrize("name", U.MESHES)
def test_grid_against_the_twin(name):
    """A grid with a margin on every side: cell by cell equal to the twin on the coordinates the device made, but for the nodes
    where some cell has min lambda in (-10 tol, -tol / 10) (at most 1 %: test_sample_twin.py)."""
    m = U.mesh(name)
    ctx = shared(name)
    origin, spacing, dims = U.margin_grid(m, U.GRID_N[name])
    ctx.sample_set_grid(origin, spacing, dims)
    cell, lam, x = ctx.sample_location()
    n = int(dims.prod())
    assert len(cell) == n == ctx.info(_lib.INFO_SAMPLE_POINTS) and ctx.info(_lib.INFO_SAMPLE_LOCATED) == (cell >= 0).sum()
    ref = U.grid_points(m, origin, spacing, dims)
    assert U.worst("grid nodes", x, ref, 4e-16 * np.abs(ref).max())  # index * spacing + origin, rounded once or twice
    tc, tl, amb, count = U.cached(("twin grid on device x", name, x.tobytes()), lambda: T.locate(m.x, m.cells, x, U.TOL))
    keep = ~amb
    print("%s: %d nodes, %d located, %d ties, %d left out" % (name, n, (cell >= 0).sum(), (count > 1).sum(), amb.sum()))
    assert amb.mean() <= U.MAX_AMBIGUOUS and np.array_equal(cell[keep], tc[keep])
    assert (cell >= 0).sum() >= (484 if name == "square" else 500) and (cell < 0).sum() > 0.1 * n
    assert U.worst("grid lambda", lam[keep], tl[keep], U.TOL_LAMBDA)
    u, p, exact = U.affine_state(m)
    set_state(ctx, m, u, p)
    rows = ctx.sample_now()
    inside = cell >= 0
    assert (rows[~inside] == 0.0).all()
    assert U.worst("grid affine", rows[inside], exact(x[inside]), U.TOL_EXACT * np.abs(exact(x[inside])).max())


@pytest.mark.parametrize("name", ["square", "cube", "bifurcation"])
def test_permuted_numbering(name):
    """The caller's cells in another order and with other local vertex orders (half of them change orientation): the expectation is
    permuted with them, the rows follow the caller's local order."""
    m, q = U.mesh(name), U.permuted(name)
    ctx = context(q)
    pts, old = U.seeds(m, 257)
    check_location(q, ctx, pts, q.new_of_old[old], "seeds, permuted")
    check_location(q, ctx, *U.vertex_points(q), "vertices, permuted")
    check_location(q, ctx, *U.facet_points(q), "facets, permuted")
    # ... and they are the same places: the lowest new index among the cells that hold the point in the old numbering
    fp = U.facet_points(m)[0][::5]
    holders = T.containing(m.x, m.cells, fp, U.TOL)
    check_location(q, ctx, fp, np.array([q.new_of_old[h].min() for h in holders], dtype=np.int32), "old facets, permuted")
    u, p, exact = U.affine_state(m)
    set_state(ctx, q, u, p)
    assert U.worst("affine, permuted", ctx.sample_now(), exact(fp), U.TOL_EXACT * np.abs(exact(fp)).max())
    ctx.close()


def _all_bytes(ctx, m, name):
    out = b""
    pts = np.vstack([U.seeds(m, 257)[0], m.x, U.facet_points(m)[0], U.outside_box(m)])
    ctx.sample_set_points(pts)
    out += b"".join(a.tobytes() for a in ctx.sample_location()) + ctx.sample_now().tobytes()
    ctx.sample_set_grid(*U.margin_grid(m, U.GRID_N[name]))
    out += b"".join(a.tobytes() for a in ctx.sample_location()) + ctx.sample_now().tobytes()
    ctx.sample_mean_reset()
    ctx.sample_mean_accumulate(0.4)
    ctx.sample_mean_accumulate(0.6)
    return out + b"".join(ctx.sample_mean_get(w).tobytes() for w in range(4))


@pytest.mark.parametrize("name", ["stenosis", "bifurcation"])
def test_same_bytes(name):
    """Two calls of every entry point on one state, and a second context on the same mesh."""
    m = U.mesh(name)
    state = U.random_state(name)
    a = context(m, state)
    first, second = _all_bytes(a, m, name), _all_bytes(a, m, name)
    b = context(m, state)
    third = _all_bytes(b, m, name)
    a.close()
    b.close()
    assert first == second == third


# --------------------------------------------------------------------------------------------------------------------- sampling
def mixed_points(name):
    m = U.mesh(name)
    return np.vstack([U.seeds(m, 1000)[0], m.x[::3], U.facet_points(m)[0][::7], U.outside_box(m)])


@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_affine_fields_are_exact(name):
    """u = A x + b, p = c . x + e: every located point equals the closed form, whichever of the tied cells was chosen; unlocated
    points are exactly 0."""
    m = U.mesh(name)
    ctx = shared(name)
    pts = mixed_points(name)
    u, p, exact = U.affine_state(m)
    set_state(ctx, m, u, p)
    ctx.sample_set_points(pts)
    cell = ctx.sample_location()[0]
    rows = ctx.sample_now()
    inside = cell >= 0
    assert rows.shape == (len(pts), m.d + 1) and inside.sum() == len(pts) - len(U.outside_box(m))
    assert (rows[~inside] == 0.0).all() and not np.signbit(rows[~inside]).any()
    assert U.worst("affine", rows[inside], exact(pts[inside]), U.TOL_EXACT * np.abs(exact(pts[inside])).max())


@pytest.mark.parametrize("name", ["cube", "stenosis", "bifurcation"])
def test_random_fields_match_the_twin(name):
    m = U.mesh(name)
    ctx = shared(name)
    pts = mixed_points(name)
    u, p = U.random_state(name)
    set_state(ctx, m, u, p)
    ctx.sample_set_points(pts)
    cell, lam, _ = ctx.sample_location()
    tc, tl = U.cached(("twin mixed", name), lambda: T.locate(m.x, m.cells, pts, U.TOL)[:2])
    assert np.array_equal(cell, tc)
    want = T.rows(m, tc, tl, u, p)
    rows = ctx.sample_now()
    assert U.worst("velocity", rows[:, :-1], want[:, :-1], U.TOL_TWIN * np.abs(u).max())
    assert U.worst("pressure", rows[:, -1], want[:, -1], U.TOL_TWIN * np.abs(p).max())


def test_series():
    """Capacity 3: the fourth record is refused and names cfdh_sample_series_get; get returns 3 blocks and their times and empties
    the buffer, which then takes 3 more; every block equals sample_now of the same state bit for bit."""
    name = "stenosis"
    m = U.mesh(name)
    ctx = context(m)
    pts = mixed_points(name)[::2]
    ctx.sample_set_points(pts)
    states = [U.random_state(name, k) for k in range(6)]
    launches = ctx.info(_lib.INFO_SAMPLE_LAUNCHES)
    ctx.sample_series_enable(3)
    now = []
    for round_ in range(2):
        times = [0.1 * (3 * round_ + k) + 0.05 for k in range(3)]
        for k in range(3):
            set_state(ctx, m, *states[3 * round_ + k])
            ctx.sample_record(times[k])
            assert ctx.info(_lib.INFO_SAMPLE_SERIES_ROWS) == k + 1
            now.append(ctx.sample_now())
        with pytest.raises(_lib.CfdhError, match="cfdh_sample_series_get"):
            ctx.sample_record(9.0)
        assert ctx.info(_lib.INFO_SAMPLE_SERIES_ROWS) == 3
        t, blocks = ctx.sample_series_get()
        assert t.tolist() == times and blocks.shape == (3, len(pts), m.d + 1)
        for k in range(3):
            assert blocks[k].tobytes() == now[3 * round_ + k].tobytes()
        assert ctx.info(_lib.INFO_SAMPLE_SERIES_ROWS) == 0
    assert np.abs(blocks).max() > 0 and ctx.info(_lib.INFO_SAMPLE_LAUNCHES) == launches + 12
    t, blocks = ctx.sample_series_get()  # nothing waiting
    assert len(t) == 0 and blocks.shape == (0, len(pts), m.d + 1)
    ctx.sample_set_points(pts[:5])  # a new set drops the series
    with pytest.raises(_lib.CfdhError):
        ctx.sample_record(0.0)
    ctx.close()


def test_series_capacity_is_bounded():
    """rows * n * (d + 1) * 8 bytes must not wrap: a buffer above 2^40 bytes is CFDH_E_ARG, and the context stays usable."""
    m = U.mesh("square")
    u, p, exact = U.affine_state(m)
    ctx = context(m, (u, p))
    pts = U.seeds(m, 1000)[0]
    ctx.sample_set_points(pts)
    for rows in (2 ** 31 - 1, 2 ** 26, 2 ** 40 // (1000 * 24) + 1):  # the first wraps 64 bits, all are above 2^40 bytes
        with pytest.raises(ValueError, match="2\\^40"):
            ctx.sample_series_enable(rows)
    with pytest.raises(ValueError):
        ctx.sample_series_enable(2 ** 31)
    with pytest.raises(_lib.CfdhError):  # nothing was allocated
        ctx.sample_record(0.0)
    ctx.sample_series_enable(2)
    ctx.sample_record(0.5)
    t, blocks = ctx.sample_series_get()
    assert t.tolist() == [0.5] and U.worst("after the refusals", blocks[0], exact(pts), U.TOL_EXACT * np.abs(exact(pts)).max())
    ctx.close()


@pytest.mark.parametrize("name", ["stenosis", "cube"])
def test_means(name):
    m = U.mesh(name)
    pts = mixed_points(name)
    (ua, pa), (ub, pb) = U.random_state(name, 1), U.random_state(name, 2)
    wa, wb = 0.3, 0.7
    ctx = context(m, (ua, pa))
    ctx.sample_set_points(pts)
    tc, tl = U.cached(("twin mixed", name), lambda: T.locate(m.x, m.cells, pts, U.TOL)[:2])
    with pytest.raises(_lib.CfdhError):  # before a reset: CFDH_E_STATE
        ctx.sample_mean_accumulate(wa)
    with pytest.raises(_lib.CfdhError):
        ctx.sample_mean_get(_lib.SAMPLE_TOTALS)
    ctx.sample_mean_reset()
    assert ctx.sample_mean_get(_lib.SAMPLE_TOTALS).tolist() == [0.0, 0.0]
    with pytest.raises(_lib.CfdhError):  # W == 0: CFDH_E_STATE
        ctx.sample_mean_get(_lib.SAMPLE_MEAN_U)
    for bad in (0.0, -1.0, np.nan, np.inf):  # CFDH_E_ARG, nothing accumulated
        with pytest.raises(ValueError):
            ctx.sample_mean_accumulate(bad)
    for bad in (4, -1):
        with pytest.raises(ValueError):
            ctx.sample_mean_get(bad)
    launches = ctx.info(_lib.INFO_SAMPLE_LAUNCHES)
    ctx.sample_mean_accumulate(wa)
    set_state(ctx, m, ub, pb)
    ctx.sample_mean_accumulate(wb)
    assert ctx.info(_lib.INFO_SAMPLE_LAUNCHES) == launches + 2
    assert ctx.sample_mean_get(_lib.SAMPLE_TOTALS).tolist() == [1.0, 2.0]
    ra, rb = T.rows(m, tc, tl, ua, pa), T.rows(m, tc, tl, ub, pb)
    W = wa + wb
    mean = (wa * ra + wb * rb) / W
    k = np.maximum(0.0, 0.5 * ((wa * (ra[:, :-1] ** 2).sum(axis=1) + wb * (rb[:, :-1] ** 2).sum(axis=1)) / W - (mean[:, :-1] ** 2).sum(axis=1)))
    umax, pmax = max(np.abs(ua).max(), np.abs(ub).max()), max(np.abs(pa).max(), np.abs(pb).max())
    got_u, got_p, got_k = (ctx.sample_mean_get(w) for w in range(3))
    assert got_u.shape == (len(pts), m.d) and got_p.shape == got_k.shape == (len(pts),)
    assert U.worst("mean velocity", got_u, mean[:, :-1], U.TOL_MEAN * umax)
    assert U.worst("mean pressure", got_p, mean[:, -1], U.TOL_MEAN * pmax)
    assert U.worst("k'", got_k, k, U.TOL_MEAN * umax * umax) and k.max() > 0.01 * umax * umax
    assert (got_u[tc < 0] == 0.0).all() and (got_k[tc < 0] == 0.0).all()
    ctx.sample_mean_reset()  # a second reset zeroes everything
    assert ctx.sample_mean_get(_lib.SAMPLE_TOTALS).tolist() == [0.0, 0.0]
    with pytest.raises(_lib.CfdhError):
        ctx.sample_mean_get(_lib.SAMPLE_FLUCTUATION)
    ctx.sample_mean_accumulate(1.0)
    assert U.worst("mean of one state", ctx.sample_mean_get(_lib.SAMPLE_MEAN_U), ctx.sample_now()[:, :-1], 1e-15 * umax)
    assert (ctx.sample_mean_get(_lib.SAMPLE_FLUCTUATION) <= 1e-15 * umax * umax).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------- states and refusals
def test_states_arguments_and_info():
    m = U.mesh("square")
    ctx = context(m)
    assert infos(ctx) == (0, 0, 0, 0)
    cell, lam, x = ctx.sample_location()  # no set: empty
    assert len(cell) == 0 and lam.shape == (0, 3) and x.shape == (0, 2)
    for fn, a in ((ctx.sample_now, ()), (ctx.sample_series_enable, (3,)), (ctx.sample_record, (0.0,)), (ctx.sample_series_get, ()),
                  (ctx.sample_mean_reset, ())):  # no set: CFDH_E_STATE
        with pytest.raises(_lib.CfdhError):
            fn(*a)
    good = U.seeds(m, 65)[0]
    for bad_x in (np.array([[0.5, np.nan]]), np.array([[np.inf, 0.5]])):
        with pytest.raises(ValueError):
            ctx.sample_set_points(bad_x)
    for tol in (-1e-12, 1.1e-3, np.nan, np.inf):
        with pytest.raises(ValueError):
            ctx.sample_set_points(good, tol)
        with pytest.raises(ValueError):
            ctx.sample_set_grid((0, 0, 0), (0.1, 0.1, 1), (3, 3, 1), tol)
    o, h, d = (0.0, 0.0, 0.0), (0.1, 0.1, 1.0), (4, 4, 1)
    bad_grids = [((np.nan, 0, 0), h, d), ((0, np.inf, 0), h, d), (o, (0.1, np.nan, 1), d), (o, (0.0, 0.1, 1), d), (o, (0.1, -0.1, 1), d),
                 (o, h, (0, 4, 1)), (o, h, (4, -1, 1)), (o, h, (4, 4, 2)), (o, h, (4, 4, 0)), (o, h, (2 ** 16, 2 ** 15, 1)), (o, h, (2 ** 40, 1, 1))]
    for g in bad_grids:
        with pytest.raises(ValueError):
            ctx.sample_set_grid(*g)
    assert infos(ctx) == (0, 0, 0, 0)  # nothing happened so far
    ctx.sample_set_points(good)
    assert infos(ctx) == (65, 65, 0, 0)
    with pytest.raises(_lib.CfdhError):  # no state yet: CFDH_E_STATE
        ctx.sample_now()
    ctx.sample_series_enable(2)
    with pytest.raises(_lib.CfdhError):
        ctx.sample_record(0.0)
    ctx.sample_mean_reset()
    with pytest.raises(_lib.CfdhError):
        ctx.sample_mean_accumulate(0.5)
    with pytest.raises(ValueError):
        ctx.sample_series_enable(-1)
    assert infos(ctx) == (65, 65, 0, 0)
    u, p, exact = U.affine_state(m)
    set_state(ctx, m, u, p)
    ctx.sample_now()
    ctx.sample_record(0.1)
    ctx.sample_mean_accumulate(0.5)
    assert infos(ctx) == (65, 65, 3, 1)
    assert ctx.info(_lib.INFO_SAMPLE_LOCATE_NS) > 0 and ctx.info(_lib.INFO_SAMPLE_KERNEL_NS) > 0
    assert ctx.info(_lib.INFO_SAMPLE_BIN_TOTAL) <= 16 * m.nc and ctx.info(_lib.INFO_SAMPLE_BIN_LONGEST) >= 1
    ctx.sample_set_grid((0.05, 0.05, 0.0), (0.4, 0.4, 1.0), (4, 3, 1))  # replaces the set: the series and the means are dropped
    assert infos(ctx) == (12, 9, 3, 0)  # the column at x = 1.25 lies outside the unit square
    with pytest.raises(_lib.CfdhError):
        ctx.sample_record(0.2)
    with pytest.raises(_lib.CfdhError):
        ctx.sample_mean_get(_lib.SAMPLE_TOTALS)
    x = ctx.sample_location()[2]
    assert np.allclose(x[5], [0.45, 0.45], rtol=0, atol=1e-16) and np.array_equal(x[:4, 1], np.full(4, 0.05))
    assert np.array_equal(ctx.sample_location()[0] >= 0, np.tile([True, True, True, False], 3))
    ctx.sample_set_points(np.zeros((0, 2)))  # n = 0 removes the set
    assert infos(ctx) == (0, 0, 3, 0)
    with pytest.raises(_lib.CfdhError):
        ctx.sample_now()
    ctx.sample_set_points(good[:7], 0.0)  # tol = 0 is allowed
    assert infos(ctx) == (7, 7, 3, 0)
    assert U.worst("after everything", ctx.sample_now(), exact(good[:7]), U.TOL_EXACT * np.abs(exact(good)).max())
    ctx.close()


def _refused(ctx):
    calls = [(ctx.sample_set_points, np.zeros((1, ctx.dim))), (ctx.sample_set_grid, (0, 0, 0), (1, 1, 1), (2, 2, 1)), (ctx.sample_location,),
             (ctx.sample_now,), (ctx.sample_series_enable, 3), (ctx.sample_record, 0.1), (ctx.sample_series_get,), (ctx.sample_mean_reset,),
             (ctx.sample_mean_accumulate, 0.1), (ctx.sample_mean_get, _lib.SAMPLE_TOTALS)]
    for fn, *a in calls:
        with pytest.raises(ValueError) as e:
            fn(*a)
        assert len(str(e.value)) > 20  # a reason
    assert infos(ctx) == (0, 0, 0, 0)


def test_unsupported_contexts_refuse():
    """Generic-element contexts, pressure-correction contexts and parts of a partitioned run: CFDH_E_ARG with a reason from every
    entry point, the context unchanged; a valid context on the same mesh works."""
    from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
    from gen_util import node_mesh
    case = dfg_case(4)
    m = case.mesh
    pts = np.asarray(m.x, dtype=float)[::5, :2]

    def works():
        ok = make_ctx(case)
        z = np.zeros(case.nv)
        ok.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.ones(2 * case.nv), p=z + 2.0)
        ok.sample_set_points(pts)
        assert infos(ok) == (len(pts), len(pts), 0, 0) and np.array_equal(ok.sample_now(), np.tile([1.0, 1.0, 2.0], (len(pts), 1)))
        ok.close()

    gen = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker, etype=3)
    _refused(gen)
    gen.close()
    works()
    p2 = node_mesh("P2", 3, 0.1)
    nvert = int(p2.cells[:, :3].max()) + 1
    ip = _lib.IpcsContext(p2.x, p2.cells, nvert, p2.facet_cells, p2.facet_local, p2.facet_marker)
    _refused(ip)
    ip.close()
    works()
    lp = LocalPart(m, partition_vertices_rcb(m.x, 2), 0)
    part = _lib.Context(lp.x, lp.cells, lp.facet_cells, lp.facet_local, lp.facet_marker, nv_owned=lp.nvo)
    _refused(part)
    part.close()
    works()


def _every_call(ctx, pts, k):
    if k == 0:
        ctx.sample_set_points(pts)
    elif k == 1:
        ctx.sample_series_get()
        ctx.sample_set_grid((0.0, 0.0, 0.0), (0.05, 0.05, 1.0), (45, 10, 1))
    if k < 2:
        ctx.sample_series_enable(2)
        ctx.sample_mean_reset()
    ctx.sample_location()
    ctx.sample_now()
    ctx.sample_record(0.01 * k)
    ctx.sample_mean_accumulate(0.01)
    for w in range(4):
        ctx.sample_mean_get(w)


def test_flow_step_is_untouched():
    """u and p of three steps, bit for bit, with every sampler call made between the steps and without; a context that never calls
    the sampler reports 0 for cfdh_info 111 - 114."""
    case = dfg_case(6)
    pts = np.asarray(case.mesh.x, dtype=float)[::3, :2] * 0.999 + 1e-4
    out = []
    for on in (False, True):
        ctx = make_ctx(case)
        z = np.zeros(case.nv)
        ctx.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.zeros(2 * case.nv), p=z)
        for k in range(3):
            ctx.solve_step()
            if on:
                _every_call(ctx, pts, k)
            u, p = ctx.get_solution()
            out.append((u.copy(), p.copy()))
            ctx.advance()
        if on:
            assert infos(ctx) == (450, ctx.info(_lib.INFO_SAMPLE_LOCATED), 9, 2) and 0 < ctx.info(_lib.INFO_SAMPLE_LOCATED) < 450
            assert np.abs(ctx.sample_now()).max() > 0
        else:
            assert infos(ctx) == (0, 0, 0, 0)
        ctx.close()
    for k in range(3):
        assert out[k][0].tobytes() == out[3 + k][0].tobytes() and out[k][1].tobytes() == out[3 + k][1].tobytes()
        assert np.abs(out[k][0]).max() > 0


# -------------------------------------------------------------------------------------------------------------------- scenario
def _stenosis():
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    sc = StenosisSimulation("stabilized_schur", 0.01, 0.06, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True)
    sc.early_stop_tolerance = 0
    sc.setup()
    return sc


def test_scenario_probes(tmp_path):
    """probes.npz holds one row per recorded step (every second of 6; the buffer of 2 records is drained on the way and at the end); a probe
    on a Dirichlet inlet vertex returns the inlet value exactly; a probe outside reads zeros."""
    from cfd_hemodynamic_amd import sampling
    out = str(tmp_path / "run")
    sc = _stenosis()
    x = np.asarray(sc.mesh.x, dtype=float)[:, :2]
    inlet = np.flatnonzero(x[:, 0] == x[:, 0].min())
    v = inlet[np.argsort(x[inlet, 1])[len(inlet) // 2]]  # a vertex in the middle of the inlet
    pts = np.vstack([x[v], sampling.line([1.0, 0.5 * x[:, 1].max()], [11.0, 0.5 * x[:, 1].max()], 6), [[-1.0, 0.0]]])
    sc.solve(output_folder=out, max_steps=6, write_every=0, probes={"points": pts, "every": 2, "rows": 2})
    P = sc.probes
    assert P["u"].shape == (3, 8, 2) and P["p"].shape == (3, 8) and np.allclose(P["t"], [0.02, 0.04, 0.06])
    assert P["cell"][0] >= 0 and (P["cell"][1:7] >= 0).all() and P["cell"][7] == -1 and np.array_equal(P["x"], pts)
    nodal = np.asarray(sc.solver.u_sol.x.array).reshape(-1, 2)
    assert P["u"][-1, 0].tobytes() == nodal[v].tobytes() and abs(nodal[v, 0]) > 0  # the Dirichlet value, bit for bit
    assert (P["u"][:, 7] == 0).all() and (P["p"][:, 7] == 0).all() and np.linalg.norm(P["u"][:, 1:7], axis=2).min() > 0
    assert P["p"][-1, 0].tobytes() == np.asarray(sc.solver.p_sol.x.array)[v].tobytes()
    z = np.load(os.path.join(out, "probes.npz"))
    assert sorted(z.files) == ["cell", "p", "t", "u", "x"] and np.array_equal(z["u"], P["u"]) and np.array_equal(z["t"], P["t"])
    assert sc.solver.ctx.info(_lib.INFO_SAMPLE_SERIES_ROWS) == 0 and sc.solver.ctx.info(_lib.INFO_SAMPLE_LAUNCHES) == 3
    with pytest.raises(ValueError):
        sc.solve(max_steps=1, probes={"points": pts}, sample_grid={"spacing": 0.5})  # one sample set


def test_scenario_grid(tmp_path):
    from cfd_hemodynamic_amd import sampling
    out = str(tmp_path / "run")
    sc = _stenosis()
    sc.solve(output_folder=out, max_steps=4, write_every=0, sample_grid={"spacing": 0.25, "pad": 0.1, "every": 2, "window": (0.01, 0.04)})
    G = sc.sample_grid
    n = int(G["dims"].prod())
    ctx = sc.solver.ctx
    assert ctx.info(_lib.INFO_SAMPLE_POINTS) == n and G["located"] == ctx.info(_lib.INFO_SAMPLE_LOCATED) and 0 < G["located"] < n
    assert sorted(os.listdir(os.path.join(out, "grid"))) == ["grid_000000.vti", "grid_000001.vti"]
    z = sampling.read_vti(os.path.join(out, "grid", "grid_000001.vti"))
    assert np.array_equal(z["dims"], G["dims"]) and np.array_equal(z["origin"], G["origin"]) and np.array_equal(z["spacing"], G["spacing"])
    assert int(z["located"].sum()) == ctx.info(_lib.INFO_SAMPLE_LOCATED) and np.array_equal(z["located"] > 0, G["cell"] >= 0)
    u, p = sc.solver.sample_now()  # the state of the last step is still there
    assert np.array_equal(z["velocity"][:, :2], u) and np.array_equal(z["pressure"], p) and np.abs(u).max() > 0
    assert (z["velocity"][z["located"] == 0] == 0).all()
    W = G["window"]
    assert W["steps"] == 3 and abs(W["W"] - 0.03) <= 1e-15  # the steps that end in (0.01, 0.04]
    mean = sampling.read_vti(os.path.join(out, "grid_mean.vti"))
    assert np.array_equal(mean["mean_velocity"][:, :2], W["mean_velocity"]) and np.array_equal(mean["mean_pressure"], W["mean_pressure"])
    assert np.array_equal(mean["fluctuation"], W["fluctuation"]) and (W["fluctuation"] >= 0).all() and int(mean["located"].sum()) == G["located"]


def test_cli_flags_reach_solve(monkeypatch, tmp_path):
    from cfd_hemodynamic_amd.__main__ import main
    from cfd_hemodynamic_amd.scenario import Scenario
    seen = {}

    def solve(self, output_folder, *a, **kw):  # the stenosis scenario writes its own files into the folder afterwards
        os.makedirs(output_folder, exist_ok=True)
        seen.update(kw)
        return output_folder

    monkeypatch.setattr(Scenario, "solve", solve)
    base = ["simulate", "--simulation", "stenosis", "--solver", "stabilized_schur", "--T", "0.02", "--dt", "0.01", "--output_dir", str(tmp_path),
            "--quiet", "True", "--ny", "6", "--L", "12.0", "--x_sten", "5.0"]
    assert main(base + ["--probes", "1.0,0.5;2.0,0.25", "--probe_line", "0,1;4,1;3", "--sample_every", "2"]) == 0
    assert seen["probes"] == {"points": [[1.0, 0.5], [2.0, 0.25], [0.0, 1.0], [2.0, 1.0], [4.0, 1.0]], "every": 2} and "sample_grid" not in seen
    seen.clear()
    assert main(base + ["--sample_grid_spacing", "0.5", "--sample_every", "3", "--sample_window_from", "0.01"]) == 0
    assert seen["sample_grid"] == {"spacing": 0.5, "every": 3, "window": (0.01, 0.02)} and "probes" not in seen
    seen.clear()
    assert main(base) == 0
    assert "probes" not in seen and "sample_grid" not in seen
    # one sample set per run, and no flag without the set it belongs to: refused before the scenario is built
    for bad in (["--probes", "1.0,0.5", "--sample_grid_spacing", "0.5"], ["--probe_line", "0,1;4,1;3", "--sample_grid_spacing", "0.5"],
                ["--sample_window_from", "0.01"], ["--probes", "1.0,0.5", "--sample_window_to", "0.02"], ["--sample_every", "2"]):
        with pytest.raises(SystemExit):
            main(base + bad)
    assert not seen
