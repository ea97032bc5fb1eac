"""The cut-plane sections on the device (cfdh_section_*, csrc/cfdh_section.hip): affine fields against their closed form, random
fields against the brute-force twin (section_twin.py), the boundary flux against cfdh_functional, the cut lists, orientation, sizes,
repeatability, the series, the means, every refusal and state error, the untouched flow step, and the scenario / command-line
routes.

Meshes of 128 to 6288 cells; sections of 0, 2, 12 ... 1344 entries (below a wave, above one and above five workgroups); 1 to 256
sections.  Every comparison prints its error next to its bound before it asserts."""
import os

import numpy as np
import pytest

import section_twin as T
import section_util as U
from cfd_hemodynamic_amd import _lib
from util import dfg_case, make_ctx

pytestmark = pytest.mark.gpu

INFO = (_lib.INFO_SECTION_COUNT, _lib.INFO_SECTION_ENTRIES, _lib.INFO_SECTION_LONGEST, _lib.INFO_SECTION_LAUNCHES, _lib.INFO_SECTION_SERIES_ROWS)
_CTX = {}


def set_state(ctx, u, p):
    u, p = np.ascontiguousarray(u).ravel(), np.ascontiguousarray(p).ravel()
    ctx.set_state(u_prev=u, p_prev=p, u=u, p=p)


def context(m, state=None, params=True):
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    if params:
        ctx.set_params(0.01, U.RHO, 3.5e-3)
    if state is not None:
        set_state(ctx, *state)
    return ctx


def shared(name):
    """One context per mesh for the tests that only set sections, a state, and read."""
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


def set_cases(ctx, cs):
    ctx.section_set(*U.arrays(cs))


# ----------------------------------------------------------------------------------------------------------------- the integrals
@pytest.mark.parametrize("name", ["cube", "square"])
def test_affine_fields_against_the_closed_form(name):
    """u = M x + b, p = c . x + e: all ten slots on the planes of the issue against the integral over the analytically known
    polygon, at 1e-12 of the magnitude; the areas; ten +0.0 where nothing is cut."""
    m, ctx = U.mesh(name), shared(name)
    u, p, ufun, pfun = U.affine_state(m)
    set_state(ctx, u, p)
    keys = list(U.cases(name))
    set_cases(ctx, [U.cases(name)[k] for k in keys])
    rows = ctx.section_now()
    assert rows.shape == (len(keys), 10)
    for k, key in enumerate(keys):
        c = U.cases(name)[key]
        if c["area"] == 0.0:
            assert rows[k].tobytes() == np.zeros(10).tobytes(), key
            continue
        want = T.polygon_rows(c["polygon"], ufun, pfun, c["normal"], U.RHO)
        assert abs(want[0] - c["area"]) <= 1e-15
        assert U.worst(name + " " + key, rows[k], want, U.TOL_EXACT * U.row_scale(c["area"], u, p))
        if m.d == 2:
            assert rows[k, 9].tobytes() == np.zeros(1).tobytes()


@pytest.mark.parametrize("name", U.MESHES)
def test_random_fields_match_the_twin(name):
    """Random vertex fields against the twin (closed-form moments; the kernel integrates by quadrature) at 1e-11 of the scale."""
    m, ctx = U.mesh(name), shared(name)
    u, p = U.random_state(name)
    set_state(ctx, u, p)
    keys = list(U.cases(name))
    set_cases(ctx, [U.cases(name)[k] for k in keys])
    rows = ctx.section_now()
    for k, key in enumerate(keys):
        sec = U.twin_cuts(name)[key]
        want = T.rows(sec, m.cells, u, p, U.RHO)
        assert U.worst(name + " " + key, rows[k], want, U.TOL_TWIN * U.row_scale(max(want[0], 1e-300), u, p))
    if name == "bifurcation":  # the two balls select one daughter each (straddling == 0: test_section_twin.py)
        both, left, right = (rows[keys.index(k)] for k in ("both", "left", "right"))
        assert U.worst("left + right = both", left + right, both, U.TOL_EXACT * U.row_scale(both, u, p))
        strad = ctx.section_get_cut()[3]
        assert strad[keys.index("left")] == 0 and strad[keys.index("right")] == 0 and strad[keys.index("bad_ball")] > 0


@pytest.mark.parametrize("name", ["cube", "square"])
def test_boundary_flux_equals_the_functional(name):
    """A section on the boundary x = 1 with n = +x (marker 11 alone): slot 1 is cfdh_functional(7, 11); with n = -x it sees nothing."""
    m, ctx = U.mesh(name), shared(name)
    u, p = U.random_state(name)
    set_state(ctx, u, p)
    c = U.cases(name)["x1_outward"]
    set_cases(ctx, [c, U.case(c["origin"], -c["normal"])])
    rows = ctx.section_now()
    flux = ctx.functional(7, 11)
    assert abs(flux) > 1e-3
    assert U.worst(name + " flux", rows[0, 1], flux, U.TOL_EXACT * U.row_scale(1.0, u, p)[1])
    assert rows[1].tobytes() == np.zeros(10).tobytes()


@pytest.mark.parametrize("name", U.MESHES)
def test_cut_lists_equal_the_twin(name):
    m, ctx = U.mesh(name), shared(name)
    keys = list(U.cases(name))
    set_cases(ctx, [U.cases(name)[k] for k in keys])
    ptr, cell, meas, strad = ctx.section_get_cut()
    assert ptr.dtype == np.int64 and cell.dtype == np.int32 and ptr[0] == 0 and len(cell) == ptr[-1] == ctx.info(_lib.INFO_SECTION_ENTRIES)
    assert ctx.info(_lib.INFO_SECTION_LONGEST) == np.diff(ptr).max() and ctx.info(_lib.INFO_SECTION_COUNT) == len(keys)
    for k, key in enumerate(keys):
        sec = U.twin_cuts(name)[key]
        assert np.array_equal(cell[ptr[k]:ptr[k + 1]], sec.cells), key
        assert strad[k] == sec.straddling
        assert U.worst(key + " measures", meas[ptr[k]:ptr[k + 1]], sec.measure, U.TOL_EXACT * max(sec.measure.sum(), 1e-300))


@pytest.mark.parametrize("name", ["cube", "stenosis", "bifurcation"])
def test_opposite_normals(name):
    """Planes through no vertex: slots 1, 5, 6 change sign, 0, 2, 3, 4 stay, at 1e-13 (the tie rule is one-sided: not bitwise)."""
    m, ctx = U.mesh(name), shared(name)
    u, p = U.random_state(name)
    set_state(ctx, u, p)
    keys = {"cube": ("x037", "y061_down"), "stenosis": ("proximal", "oblique"), "bifurcation": ("both", "left_oblique")}[name]
    cs = [U.cases(name)[k] for k in keys]
    for c in cs:
        assert np.abs(T.signed_distance(m.x, c["origin"], T.unit(c["normal"]))).min() > 1e-6 * m.size
    set_cases(ctx, cs + [dict(c, normal=-c["normal"]) for c in cs])
    rows = ctx.section_now()
    for k in range(len(cs)):
        a, b = rows[k], rows[len(cs) + k]
        sign = np.array([1, -1, 1, 1, 1, -1, -1, 1, 1, 1.0])
        assert abs(a[1]) > 0 and U.worst(keys[k] + " flipped", b, sign * a, U.TOL_FLIP * U.row_scale(a, u, p))


# ------------------------------------------------------------------------------------------------------------------------- sizes
def test_section_counts_and_list_lengths():
    """K = 1, 2, 17, 256 (257 is refused); a section below a wave (40 entries), above a workgroup (312) and above five (1344), an
    empty one among full ones; the row of a section does not depend on the other sections of the set."""
    m, ctx = U.mesh("bifurcation"), shared("bifurcation")
    u, p = U.random_state("bifurcation")
    set_state(ctx, u, p)
    cs = U.cases("bifurcation")
    set_cases(ctx, [cs["bad_ball"], cs["both"], U.case([0.0, -1.0, 0.0], [0, 1, 0]), cs["lengthwise"]])
    ptr = ctx.section_get_cut()[0]
    assert list(np.diff(ptr)) == [40, 312, 0, 1344]
    assert infos(ctx)[:3] == (4, 1696, 1344)
    four = ctx.section_now()
    assert four[2].tobytes() == np.zeros(10).tobytes() and (four[[0, 1, 3], 0] > 0).all()
    want = T.rows(U.twin_cuts("bifurcation")["lengthwise"], m.cells, u, p, U.RHO)
    assert U.worst("lengthwise", four[3], want, U.TOL_TWIN * U.row_scale(want, u, p))
    rng = np.random.default_rng(9)
    ys = rng.uniform(0.002, 0.029, 256)
    launches = ctx.info(_lib.INFO_SECTION_LAUNCHES)
    single = {}
    for K in (1, 2, 17, 256):
        o = np.stack([np.zeros(K), ys[:K], np.zeros(K)], axis=1)
        ctx.section_set(o, np.tile([0.0, 1.0, 0.0], (K, 1)))
        rows = ctx.section_now()
        launches += 1
        assert rows.shape == (K, 10) and (rows[:, 0] > 0).all()
        assert infos(ctx) == (K, int(ctx.section_get_cut()[0][-1]), int(np.diff(ctx.section_get_cut()[0]).max()), launches, 0)
        single[K] = rows
        assert rows[0].tobytes() == single[1][0].tobytes()
        if K > 2:
            assert rows[:2].tobytes() == single[2].tobytes()
    k = 200
    sec = T.cut(m.x, m.cells, [0.0, ys[k], 0.0], [0, 1, 0])
    want = T.rows(sec, m.cells, u, p, U.RHO)
    assert U.worst("section 200 of 256", single[256][k], want, U.TOL_TWIN * U.row_scale(want, u, p))
    with pytest.raises(ValueError, match="256"):
        ctx.section_set(np.zeros((257, 3)), np.tile([0.0, 1.0, 0.0], (257, 1)))
    assert infos(ctx)[0] == 256  # a refused call leaves the set in place
    with pytest.raises(ValueError, match="2\\^40"):  # 256 sections x 10 doubles x 2^31 - 1 blocks
        ctx.section_series_enable(2 ** 31 - 1)


def test_same_bytes():
    """Two calls, a second context, and the sections in another order (row k follows its section)."""
    name = "bifurcation"
    m, ctx = U.mesh(name), shared(name)
    u, p = U.random_state(name)
    set_state(ctx, u, p)
    keys = list(U.cases(name))
    cs = [U.cases(name)[k] for k in keys]
    set_cases(ctx, cs)
    a, b = ctx.section_now(), ctx.section_now()
    assert a.tobytes() == b.tobytes() and np.abs(a).max() > 0
    other = context(m, (u, p))
    set_cases(other, cs)
    assert other.section_now().tobytes() == a.tobytes()
    order = np.random.default_rng(2).permutation(len(cs))
    set_cases(other, [cs[j] for j in order])
    assert other.section_now().tobytes() == a[order].tobytes()
    other.close()


# ------------------------------------------------------------------------------------------------------------- series and means
def test_series():
    """Capacity 3: the fourth record is refused and names cfdh_section_series_get; three blocks and times come back, three more
    are taken; every block equals section_now bit for bit."""
    name = "stenosis"
    m = U.mesh(name)
    ctx = context(m)
    set_cases(ctx, list(U.cases(name).values()))
    ctx.section_series_enable(3)
    states = [U.random_state(name, s) for s in range(6)]
    for rnd in range(2):
        want = []
        for k in range(3):
            set_state(ctx, *states[3 * rnd + k])
            ctx.section_record(0.1 * (3 * rnd + k))
            want.append(ctx.section_now())
        assert ctx.info(_lib.INFO_SECTION_SERIES_ROWS) == 3
        with pytest.raises(_lib.CfdhError, match="cfdh_section_series_get"):
            ctx.section_record(9.9)
        t, out = ctx.section_series_get()
        assert ctx.info(_lib.INFO_SECTION_SERIES_ROWS) == 0
        assert np.array_equal(t, 0.1 * (3 * rnd + np.arange(3))) and out.shape == (3, len(U.cases(name)), 10)
        assert out.tobytes() == np.stack(want).tobytes() and np.abs(out[0] - out[1]).max() > 0
    t, out = ctx.section_series_get()
    assert len(t) == 0 and out.shape[0] == 0
    ctx.close()


def test_means():
    """Two states with the weights 0.3 and 0.7 against NumPy on the rows of section_now, {W, count} = {1, 2}; then a reset."""
    name = "cube"
    m = U.mesh(name)
    ctx = context(m)
    set_cases(ctx, list(U.cases(name).values()))
    ctx.section_mean_reset()
    assert ctx.section_mean_get() == (None, 0.0, 0)
    rows = []
    for s, w in ((1, 0.3), (2, 0.7)):
        set_state(ctx, *U.random_state(name, s))
        ctx.section_mean_accumulate(w)
        rows.append(ctx.section_now())
    mean, W, count = ctx.section_mean_get()
    assert (W, count) == (1.0, 2)
    want = 0.3 * rows[0] + 0.7 * rows[1]
    scale = np.maximum(np.abs(rows[0]), np.abs(rows[1])).max(axis=0)
    assert U.worst("means", mean, want, U.TOL_MEAN * np.maximum(scale, 1e-300)) and np.abs(mean).max() > 0
    ctx.section_mean_reset()
    assert ctx.section_mean_get() == (None, 0.0, 0)
    ctx.section_mean_accumulate(0.25)
    mean, W, count = ctx.section_mean_get()
    assert (W, count) == (0.25, 1) and U.worst("one state", mean, rows[1], U.TOL_MEAN * np.maximum(scale, 1e-300))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------ error cases
def test_states_arguments_and_info():
    m = U.mesh("square")
    ctx = context(m, params=False)
    good = [U.SQUARE["x037"], U.SQUARE["diag11"], U.SQUARE["outside"]]
    o, n, r = U.arrays(good)
    assert infos(ctx) == (0, 0, 0, 0, 0) and ctx.info(_lib.INFO_SECTION_KERNEL_NS) == 0
    ptr, cell, meas, strad = ctx.section_get_cut()  # no set: empty
    assert list(ptr) == [0] and len(cell) == len(meas) == len(strad) == 0
    for fn, a in ((ctx.section_now, ()), (ctx.section_series_enable, (3,)), (ctx.section_record, (0.0,)), (ctx.section_series_get, ()),
                  (ctx.section_mean_reset, ()), (ctx.section_mean_accumulate, (0.5,)), (ctx.section_mean_get, ())):  # no set: CFDH_E_STATE
        with pytest.raises(_lib.CfdhError):
            fn(*a)
    for j in range(2):  # CFDH_E_ARG: non-finite entries, a zero normal
        for v in (np.nan, np.inf):
            for which in range(3):
                bad = [o.copy(), n.copy(), r.copy()]
                if which < 2:
                    bad[which][1, j] = v
                else:
                    bad[2][j] = v
                with pytest.raises(ValueError, match="not finite"):
                    ctx.section_set(*bad)
    zero = n.copy()
    zero[2] = 0.0
    with pytest.raises(ValueError, match="normal of section 2 is zero"):
        ctx.section_set(o, zero, r)
    with pytest.raises(ValueError):
        ctx.section_set(o, n[:2])
    assert infos(ctx) == (0, 0, 0, 0, 0)  # nothing happened so far
    ctx.section_set(o, n)  # radius == NULL: unbounded
    assert infos(ctx) == (3, 46, 30, 0, 0)
    ctx.section_series_enable(2)
    ctx.section_mean_reset()
    calls = ((ctx.section_now, ()), (ctx.section_record, (0.0,)), (ctx.section_mean_accumulate, (0.5,)))
    for fn, a in calls:  # no parameters, no state
        with pytest.raises(_lib.CfdhError, match="cfdh_set_params"):
            fn(*a)
    u, p = U.affine_state(m)[:2]
    set_state(ctx, u, p)
    for fn, a in calls:  # a state, but no parameters
        with pytest.raises(_lib.CfdhError, match="cfdh_set_params"):
            fn(*a)
    ctx.close()
    ctx = context(m)
    ctx.section_set(o, n, r)
    ctx.section_series_enable(2)
    ctx.section_mean_reset()
    calls = ((ctx.section_now, ()), (ctx.section_record, (0.0,)), (ctx.section_mean_accumulate, (0.5,)))
    for fn, a in calls:  # parameters, but no state
        with pytest.raises(_lib.CfdhError, match="state"):
            fn(*a)
    for w in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="weight"):
            ctx.section_mean_accumulate(w)
    with pytest.raises(ValueError):
        ctx.section_series_enable(-1)
    assert infos(ctx) == (3, 46, 30, 0, 0)
    set_state(ctx, u, p)
    first = ctx.section_now()
    ctx.section_record(0.1)
    ctx.section_mean_accumulate(0.5)
    assert infos(ctx) == (3, 46, 30, 3, 1) and ctx.info(_lib.INFO_SECTION_KERNEL_NS) > 0
    with pytest.raises(ValueError):  # a refused set leaves everything in place
        ctx.section_set(o, zero, r)
    assert infos(ctx) == (3, 46, 30, 3, 1)
    ctx.section_set(o[:2], n[:2], r[:2])  # a new set drops the series and the means
    assert infos(ctx) == (2, 46, 30, 3, 0)
    with pytest.raises(_lib.CfdhError, match="cfdh_section_series_enable"):
        ctx.section_record(0.2)
    with pytest.raises(_lib.CfdhError, match="cfdh_section_mean_reset"):
        ctx.section_mean_get()
    assert ctx.section_now().tobytes() == first[:2].tobytes()
    ctx.section_series_enable(1)
    ctx.section_series_enable(0)  # frees the buffer
    with pytest.raises(_lib.CfdhError, match="cfdh_section_series_enable"):
        ctx.section_series_get()
    ctx.section_set(np.zeros((0, 2)), np.zeros((0, 2)))  # K = 0 removes the set
    assert infos(ctx) == (0, 0, 0, 4, 0)
    with pytest.raises(_lib.CfdhError, match="cfdh_section_set"):
        ctx.section_now()
    ctx.section_set(o, n, r)
    assert ctx.section_now().tobytes() == first.tobytes()
    ctx.close()


def _refused(ctx):
    d = ctx.dim
    calls = [(ctx.section_set, np.zeros((1, d)), np.ones((1, d))), (ctx.section_get_cut,), (ctx.section_now,), (ctx.section_series_enable, 3),
             (ctx.section_record, 0.1), (ctx.section_series_get,), (ctx.section_mean_reset,), (ctx.section_mean_accumulate, 0.1),
             (ctx.section_mean_get,)]
    for fn, *a in calls:
        with pytest.raises(ValueError) as e:
            fn(*a)
        assert len(str(e.value)) > 20  # a reason
    assert infos(ctx) == (0, 0, 0, 0, 0)


def test_unsupported_contexts_refuse():
    """Generic-element contexts, pressure-correction contexts and parts of a partitioned run: CFDH_E_ARG with a reason from every
    entry point, the context unchanged; a valid context on the same mesh works."""
    from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
    from gen_util import node_mesh
    case = dfg_case(4)
    m = case.mesh

    def works():
        ok = make_ctx(case)
        z = np.zeros(case.nv)
        ok.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.tile([1.0, 0.5], case.nv), p=z + 2.0)
        ok.section_set([[1.0, 0.2]], [[1.0, 0.0]])
        row = ok.section_now()[0]
        assert infos(ok)[:2] == (1, len(ok.section_get_cut()[1])) and infos(ok)[1] > 0
        assert np.allclose(row, 0.41 * np.array([1.0, 1.0, 2.0, 1.0, 1.25, 2.0, 0.5 * case.rho * 1.25, 1.0, 0.5, 0.0]), rtol=1e-12, atol=0)
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


def _every_call(ctx, k):
    if k < 2:
        ctx.section_set([[0.5 + 0.4 * k, 0.2], [1.5, 0.2]], [[1.0, 0.0], [1.0, 0.3]], [0.0, 0.15] if k else None)
        ctx.section_series_enable(2)
        ctx.section_mean_reset()
    ctx.section_get_cut()
    ctx.section_now()
    ctx.section_record(0.01 * k)
    ctx.section_mean_accumulate(0.01)
    ctx.section_mean_get()
    if k == 2:
        ctx.section_series_get()


def test_flow_step_is_untouched():
    """u and p of three steps, bit for bit, with every section call made between the steps and without; a context that never sets
    sections reports 0 for cfdh_info 120 - 125."""
    case = dfg_case(6)
    out = []
    for on in (False, True):
        ctx = make_ctx(case)
        z = np.zeros(case.nv)
        ctx.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.zeros(2 * case.nv), p=z)
        for k in range(3):
            ctx.solve_step()
            if on:
                _every_call(ctx, k)
            u, p = ctx.get_solution()
            out.append((u.copy(), p.copy()))
            ctx.advance()
        if on:
            assert infos(ctx)[0] == 2 and infos(ctx)[3:] == (9, 0) and abs(ctx.section_now()[0, 1]) > 0
        else:
            assert infos(ctx) == (0, 0, 0, 0, 0) and ctx.info(_lib.INFO_SECTION_KERNEL_NS) == 0
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


def test_scenario_sections(tmp_path):
    """sections.npz and sections.txt exist and hold one row per recorded step (the buffer of 2 records is drained on the way and
    at the end).  The station on the inlet looks along the outward normal -x -- with +x the tie rule gives it nothing -- so its Q
    is cfdh_functional(7, inlet) and the inflow is -Q = -cfdh_functional(7, inlet), per step.  The mean pressure distal to the
    throat is at most the proximal one (pressure ratio <= 1).  Sections go with probes."""
    from cfd_hemodynamic_amd import sections as S
    out = str(tmp_path / "run")
    sc = _stenosis()
    x = np.asarray(sc.mesh.x, dtype=float)[:, :2]
    mid = 0.5 * x[:, 1].max()
    planes = [S.plane([0.0, mid], [-1.0, 0.0])] + S.stations([[2.0, mid], [9.0, mid]], 2) + [S.plane([5.0, mid], [1.0, 0.0])]
    flux = []
    sc.solve(output_folder=out, max_steps=5, write_every=0, sections={"planes": planes, "every": 1, "rows": 2, "window": (0.01, 0.04)},
             probes={"points": [[1.0, mid]]}, afterStepCallback=lambda t: flux.append(sc.solver.functional(7, 2)))
    R = sc.sections
    assert R["rows"].shape == (5, 4, 10) and np.allclose(R["t"], 0.01 * np.arange(1, 6)) and (R["straddling"] == 0).all()
    assert sc.probes["u"].shape == (5, 1, 2)
    flux = np.array(flux)
    assert (flux < 0).all()
    scale = np.abs(flux).max()
    assert U.worst("inlet station", R["rows"][:, 0, 1], flux, U.TOL_EXACT * scale)
    assert U.worst("inflow", -R["rows"][:, 0, 1], -flux, U.TOL_EXACT * scale)
    d = S.derive(R["rows"], reference=1)
    print("Q", R["rows"][-1, :, 1], "pressure ratio", d["pressure_ratio"][-1])
    assert d["pressure_ratio"][-1, 1] == 1.0 and d["pressure_ratio"][-1, 2] <= 1.0
    assert (d["area"][:, 3] < d["area"][:, 1]).all() and (d["flow"][-1, 1:] > 0).all()
    assert R["window_steps"] == 3 and abs(R["window_W"] - 0.03) <= 1e-15
    assert U.worst("window", R["window_mean"], R["rows"][1:4].mean(axis=0), 1e-12 * np.abs(R["rows"]).max(axis=(0, 1)))
    z = np.load(os.path.join(out, "sections.npz"))
    assert sorted(z.files) == sorted(["t", "origin", "normal", "radius", "rows", "straddling", "window_mean", "window_W", "window_steps"])
    assert np.array_equal(z["rows"], R["rows"]) and np.array_equal(z["origin"], [p["origin"] for p in planes])
    text = open(os.path.join(out, "sections.txt")).read()
    assert text.count("# section") == 4 and len(text.splitlines()) == 4 * 8
    ctx = sc.solver.ctx
    assert ctx.info(_lib.INFO_SECTION_SERIES_ROWS) == 0 and ctx.info(_lib.INFO_SECTION_LAUNCHES) == 5 + 3 and ctx.info(_lib.INFO_SECTION_COUNT) == 4
    assert sc.solver.section_now().tobytes() == R["rows"][-1].tobytes()  # the sections stay on the solver
    with pytest.raises(ValueError):
        sc.solve(max_steps=1, sections={"planes": []})


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
    assert main(base + ["--sections", "2,1.5;1,0 | 9,1.5;1,0;0.5", "--sections_every", "2", "--sections_window_from", "0.01", "--probes", "1.0,0.5"]) == 0
    sec = seen["sections"]
    assert sec["every"] == 2 and sec["window"] == (0.01, 0.02) and len(sec["planes"]) == 2 and "probes" in seen
    assert np.array_equal(sec["planes"][1]["origin"], [9.0, 1.5]) and sec["planes"][1]["radius"] == 0.5 and sec["planes"][0]["radius"] == 0.0
    seen.clear()
    assert main(base) == 0 and "sections" not in seen
    for bad in (["--sections_every", "2"], ["--sections_window_to", "0.02"], ["--sections", "1,2"], ["--sections", "1,2;0,0"]):
        with pytest.raises(SystemExit):
            main(base + bad)
    assert not seen
