"""Lagrangian particle tracking on the device (cfdh_particles_*, csrc/cfdh_particles.hip): the closed forms of
test_particles_twin.py (uniform translation, rigid rotation, simple shear, a field linear in time), random fields against the NumPy
twin (particles_twin.py) on the stenosed channel and the bifurcation, the walk cap, repeatability, the untouched flow step,
refusals, and the scenario / command-line routes.

Particle counts 1, 63, 64, 65, 257 and 1000 (wave and workgroup edges) in a capacity of 1024; the 1000 are seeded in two calls."""
import os

import numpy as np
import pytest

import particles_util as U
from cfd_hemodynamic_amd import _lib
from util import dfg_case, make_ctx, stenosis_case

pytestmark = pytest.mark.gpu

RHO = 1.06e-3
FIELDS = (_lib.PARTICLE_X, _lib.PARTICLE_CELL, _lib.PARTICLE_STATUS, _lib.PARTICLE_AGE, _lib.PARTICLE_PATH, _lib.PARTICLE_EXPOSURE,
          _lib.PARTICLE_T_END)


def context(m, u_prev, u_sol, dt, mu=U.MU):
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    ctx.set_params(dt, RHO, mu)
    z = np.zeros(m.nv)
    ctx.set_state(u_prev=np.ascontiguousarray(u_prev).ravel(), p_prev=z, u=np.ascontiguousarray(u_sol).ravel(), p=z)
    return ctx


def seed(ctx, x0, c0, t_birth=0.0):
    """1000 particles go in by two calls, every other count by one."""
    if len(x0) == 1000:
        ctx.particles_seed(x0[:600], c0[:600], t_birth)
        ctx.particles_seed(x0[600:], c0[600:], t_birth)
    else:
        ctx.particles_seed(x0, c0, t_birth)


def fields(ctx):
    x, cell, status, age, path, expo, t_end = (ctx.particles_get(w) for w in FIELDS)
    return dict(x=x, cell=cell, status=status, age=age, path=path, exposure=expo, t_end=t_end)


def device_run(m, x0, c0, u_prev, u_sol, dt, nsub, nsteps, ctx=None):
    own = ctx is None
    if own:
        ctx = context(m, u_prev, u_sol, dt)
        ctx.particles_enable(U.CAPACITY, nsub)
    seed(ctx, x0, c0)
    total = 0
    for k in range(nsteps):
        st = ctx.particles_step(k * dt)
        assert st.active + st.exited + st.lost == len(x0) and st.stepped >= st.active
        total += st.stepped
    res = fields(ctx)
    assert (res["status"] == 0).sum() == st.active and (res["status"] > 0).sum() == st.exited and (res["status"] < 0).sum() == st.lost
    if own:
        assert ctx.info(_lib.INFO_PARTICLES_ENABLED) == 1 and ctx.info(_lib.INFO_PARTICLE_STEPS) == nsteps
        assert ctx.info(_lib.INFO_PARTICLE_LAUNCHES) == nsteps
        ctx.close()
    return res


def run_case(case):
    res = device_run(case["m"], case["x0"], case["c0"], case["u_prev"], case["u_sol"], case["dt"], case["nsub"], case["nsteps"])
    case["check"](res)
    tw = U.twin(case["m"])
    assert tw.min_lambda(res["cell"], res["x"]).min() >= -1e-9  # the cell holds the position
    return res


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("n", U.COUNTS)
@pytest.mark.parametrize("name", ["square", "cube"])
def test_uniform_translation(name, n):
    run_case(U.case_translation(name, n))


@pytest.mark.parametrize("n", [65, 1000])
@pytest.mark.parametrize("name", ["square", "cube"])
def test_rigid_rotation(name, n):
    run_case(U.case_rotation(name, n))


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("name", ["square", "cube"])
def test_simple_shear(name, n):
    run_case(U.case_shear(name, n))


@pytest.mark.parametrize("nsub", [1, 2, 5])
@pytest.mark.parametrize("name", ["square", "cube"])
def test_linear_in_time(name, nsub):
    run_case(U.case_linear_in_time(name, 65, nsub))


# ------------------------------------------------------------------------------------------------------------ against the twin
@pytest.mark.parametrize("name", ["stenosis", "bifurcation"])
def test_random_fields_match_the_twin(name):
    """Two different random P1 fields, about 3 cells per substep, 5 steps of 2 substeps: positions, path, exposure and t_end to
    1e-11 of their scale, the status equal on every particle; only particles whose twin margin is below 1e-9 may be left out of
    the status and t_end comparison, at most 1 % of them."""
    tc = U.twin_case(name)
    m, tw, ref = tc["m"], tc["twin"], tc["state"]
    res = device_run(m, tc["x0"], tc["c0"], tc["u_prev"], tc["u_sol"], U.TWIN_DT, U.TWIN_NSUB, U.TWIN_STEPS)
    keep = ref["margin"] >= U.MARGIN
    assert (~keep).sum() <= 0.01 * len(keep)
    T = U.TWIN_STEPS * U.TWIN_DT
    scale_x, scale_path = m.size, max(ref["path"].max(), m.size)
    scale_expo = ref["exposure"].max()
    err = dict(x=np.abs(res["x"] - ref["x"])[keep].max() / scale_x, path=np.abs(res["path"] - ref["path"])[keep].max() / scale_path,
               exposure=np.abs(res["exposure"] - ref["exposure"])[keep].max() / scale_expo)
    out = keep & (ref["status"] != 0)
    err["t_end"] = np.abs(res["t_end"] - ref["t_end"])[out].max(initial=0.0) / T
    print("%s: relative differences to the twin %s; %d particles left out" % (name, {k: "%.2e" % v for k, v in err.items()}, (~keep).sum()))
    assert np.array_equal(res["status"][keep], ref["status"][keep])
    assert np.isnan(res["t_end"][keep & (ref["status"] == 0)]).all()
    assert tw.min_lambda(res["cell"], res["x"]).min() >= -1e-9
    assert max(err.values()) <= 1e-11


def test_walk_cap_matches_the_twin():
    cc = U.cap_case()
    ref = cc["state"]
    res = device_run(cc["m"], cc["x0"], cc["c0"], cc["u_prev"], cc["u_sol"], cc["dt"], cc["nsub"], 1)
    assert np.array_equal(res["status"], ref["status"]) and (res["status"] == -1).any()
    lost = res["status"] == -1
    assert np.array_equal(res["x"][lost], cc["x0"][lost]) and np.array_equal(res["cell"][lost], cc["c0"][lost])  # frozen at the substep's start
    assert (res["path"][lost] == 0).all() and (res["exposure"][lost] == 0).all() and (res["t_end"][lost] == 0.0).all()
    assert np.abs(res["x"] - ref["x"]).max() <= 1e-11 * cc["m"].size
    assert np.abs(res["t_end"] - ref["t_end"])[~lost].max() <= 1e-11 * cc["dt"]


# -------------------------------------------------------------------------------------------------- repeatability and isolation
def _bytes(res):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in ("x", "cell", "status", "age", "path", "exposure", "t_end"))


@pytest.mark.parametrize("name", ["stenosis", "bifurcation"])
def test_same_bytes(name):
    tc = U.twin_case(name)
    m = tc["m"]
    a = device_run(m, tc["x0"], tc["c0"], tc["u_prev"], tc["u_sol"], U.TWIN_DT, U.TWIN_NSUB, 2)
    b = device_run(m, tc["x0"], tc["c0"], tc["u_prev"], tc["u_sol"], U.TWIN_DT, U.TWIN_NSUB, 2)
    assert _bytes(a) == _bytes(b)  # two contexts
    # two steps from the same state in one context: clear, seed again, step again
    ctx = context(m, tc["u_prev"], tc["u_sol"], U.TWIN_DT)
    ctx.particles_enable(U.CAPACITY, U.TWIN_NSUB)
    c = device_run(m, tc["x0"], tc["c0"], tc["u_prev"], tc["u_sol"], U.TWIN_DT, U.TWIN_NSUB, 2, ctx=ctx)
    ctx.particles_clear()
    assert ctx.particles_count() == 0
    d = device_run(m, tc["x0"], tc["c0"], tc["u_prev"], tc["u_sol"], U.TWIN_DT, U.TWIN_NSUB, 2, ctx=ctx)
    assert _bytes(c) == _bytes(d) == _bytes(a)
    ctx.close()


def test_flow_step_is_untouched():
    """u and p of cfdh_solve_step, bit for bit, with and without particles enabled and stepped; a context that never enables them
    launches nothing for them."""
    case = stenosis_case(6)
    m = U.mesh("stenosis")
    x0, c0 = U.random_seeds(m, 257, 31)
    out = []
    for with_particles in (False, True):
        ctx = make_ctx(case)
        z = np.zeros(case.nv)
        ctx.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.zeros(2 * case.nv), p=z)
        if with_particles:
            ctx.particles_enable(U.CAPACITY, 2)
            ctx.particles_seed(x0, c0)
        for k in range(2):
            ctx.solve_step()
            if with_particles:
                st = ctx.particles_step(k * case.dt)
                assert st.stepped > 0
            u, p = ctx.get_solution()
            out.append((u.copy(), p.copy()))
            ctx.advance()
        if with_particles:
            assert ctx.info(_lib.INFO_PARTICLE_LAUNCHES) == 2 and ctx.particles_get(_lib.PARTICLE_PATH).max() > 0
        else:
            assert ctx.info(_lib.INFO_PARTICLE_LAUNCHES) == 0 and ctx.info(_lib.INFO_PARTICLES_ENABLED) == 0 and ctx.info(_lib.INFO_PARTICLE_STEPS) == 0
        ctx.close()
    for k in range(2):
        assert out[k][0].tobytes() == out[2 + k][0].tobytes() and out[k][1].tobytes() == out[2 + k][1].tobytes()


def test_markers_are_read_at_the_exit():
    """cfdh_set_facet_markers after the tables were built: the status carries the new marker."""
    case = U.case_translation("square", 257)
    m = case["m"]
    ctx = context(m, case["u_prev"], case["u_sol"], case["dt"])
    ctx.particles_enable(U.CAPACITY, case["nsub"])
    ctx.set_facet_markers(m.facet_marker + 100)
    res = device_run(m, case["x0"], case["c0"], case["u_prev"], case["u_sol"], case["dt"], case["nsub"], case["nsteps"], ctx=ctx)
    ctx.close()
    ref = U.result_of_twin(case)
    assert np.array_equal(res["status"], np.where(ref["status"] > 0, ref["status"] + 100, ref["status"])) and (res["status"] > 100).any()


# -------------------------------------------------------------------------------------------------------------------- refusals
def _refused(exc, fn, *a):
    with pytest.raises(exc):
        fn(*a)


def test_refusals():
    m = U.mesh("square")
    f = U.affine_field(m, np.zeros((2, 2)), np.array([0.3, 0.1]))
    x0, c0 = U.random_seeds(m, 65, 41)
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    state_error = _lib.CfdhError
    # before cfdh_particles_enable: CFDH_E_STATE from every other call
    _refused(state_error, ctx.particles_seed, x0, c0)
    _refused(state_error, ctx.particles_clear)
    _refused(state_error, ctx.particles_step, 0.0)
    _refused(state_error, ctx.particles_get, _lib.PARTICLE_X)
    # bad arguments of enable: CFDH_E_ARG, nothing enabled
    _refused(ValueError, ctx.particles_enable, U.CAPACITY, 0)
    _refused(ValueError, ctx.particles_enable, 0, 2)
    assert ctx.info(_lib.INFO_PARTICLES_ENABLED) == 0
    ctx.particles_enable(U.CAPACITY, 2)
    _refused(ValueError, ctx.particles_enable, U.CAPACITY + 1, 2)  # a later call may change nsub only
    ctx.particles_enable(U.CAPACITY, 3)
    # a step with no state: CFDH_E_STATE
    ctx.particles_seed(x0, c0)
    _refused(state_error, ctx.particles_step, 0.0)
    ctx.set_params(0.05, RHO, U.MU)
    _refused(state_error, ctx.particles_step, 0.0)
    z = np.zeros(m.nv)
    ctx.set_state(u_prev=f.ravel(), p_prev=z, u=f.ravel(), p=z)
    assert ctx.particles_step(0.0).stepped == 65
    # seeds: outside the cell, a cell out of range, non-finite input, over capacity -- nothing is appended
    wrong = np.roll(c0, 1)
    assert (wrong != c0).any()
    _refused(ValueError, ctx.particles_seed, x0, wrong)
    _refused(ValueError, ctx.particles_seed, x0, np.full(65, m.nc, dtype=np.int32))
    bad = x0.copy()
    bad[7, 1] = np.nan
    _refused(ValueError, ctx.particles_seed, bad, c0)
    _refused(ValueError, ctx.particles_seed, x0, c0, np.inf)
    big_x, big_c = U.random_seeds(m, U.CAPACITY - 65 + 1, 42)
    _refused(ValueError, ctx.particles_seed, big_x, big_c)
    assert ctx.particles_count() == 65
    ctx.particles_seed(big_x[:-1], big_c[:-1])  # exactly the capacity fits
    assert ctx.particles_count() == U.CAPACITY
    _refused(ValueError, ctx.particles_seed, x0[:1], c0[:1])
    _refused(ValueError, ctx.particles_step, np.nan)
    _refused(ValueError, ctx.particles_get, 7)
    _refused(ValueError, ctx.particles_get, -1)
    st = ctx.particles_step(0.05)  # the context is usable after every refusal
    assert st.active + st.exited + st.lost == U.CAPACITY
    ctx.close()


def test_unsupported_contexts_refuse():
    """Generic-element contexts, pressure-correction contexts and parts of a partitioned run: CFDH_E_ARG, the context unchanged."""
    from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
    from gen_util import node_mesh
    case = dfg_case(4)
    m = case.mesh
    gen = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker, etype=3)
    _refused(ValueError, gen.particles_enable, 16, 2)
    assert gen.info(_lib.INFO_PARTICLES_ENABLED) == 0
    _refused(_lib.CfdhError, gen.particles_step, 0.0)
    gen.close()
    p2 = node_mesh("P2", 3, 0.1)
    nvert = int(p2.cells[:, :3].max()) + 1
    ip = _lib.IpcsContext(p2.x, p2.cells, nvert, p2.facet_cells, p2.facet_local, p2.facet_marker)
    _refused(ValueError, ip.particles_enable, 16, 2)
    _refused(_lib.CfdhError, ip.particles_get, _lib.PARTICLE_X)
    ip.close()
    lp = LocalPart(m, partition_vertices_rcb(m.x, 2), 0)
    part = _lib.Context(lp.x, lp.cells, lp.facet_cells, lp.facet_local, lp.facet_marker, nv_owned=lp.nvo)
    _refused(ValueError, part.particles_enable, 16, 2)
    assert part.info(_lib.INFO_PARTICLES_ENABLED) == 0
    part.close()
    ok = make_ctx(case)  # a valid call succeeds on the same mesh
    ok.particles_enable(16, 2)
    assert ok.info(_lib.INFO_PARTICLES_ENABLED) == 1
    ok.close()


# -------------------------------------------------------------------------------------------------------------------- scenario
def test_scenario_stenosis(tmp_path):
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    out = str(tmp_path / "run")
    sc = StenosisSimulation("stabilized_schur", 0.01, 0.03, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True)
    sc.early_stop_tolerance = 0
    sc.setup()
    sc.solve(output_folder=out, max_steps=3, particles={"n": 200, "every": 1})
    P = sc.particles
    T = 3 * sc.dt
    assert P["seeded"] == 600 and len(P["status"]) == 600
    assert sum(P["counts"].values()) == 600
    assert (P["age"] >= 0).all() and (P["age"] <= T * (1 + 1e-12)).all() and (P["path"] > 0).any()
    z = np.load(os.path.join(out, "particles.npz"))
    assert np.array_equal(z["status"], P["status"]) and np.array_equal(z["x"], P["x"]) and np.array_equal(z["age"], P["age"])
    assert sum(int(z["count_%d" % s]) for s in np.unique(P["status"])) == 600
    for s in np.unique(P["status"][P["status"] > 0]):
        assert np.array_equal(z["ages_%d" % s], P["age"][P["status"] == s])
    clouds = [f for f in os.listdir(os.path.join(out, "particles")) if f.endswith(".vtu")]
    assert len(clouds) == 3


def test_cli_flags_reach_solve(monkeypatch, tmp_path):
    from cfd_hemodynamic_amd.__main__ import main
    from cfd_hemodynamic_amd.scenario import Scenario
    seen = {}

    def solve(self, output_folder, *a, **kw):  # the stenosis scenario writes its own files into the folder afterwards
        os.makedirs(output_folder, exist_ok=True)
        seen.update(kw)
        return output_folder

    monkeypatch.setattr(Scenario, "solve", solve)
    argv = ["simulate", "--simulation", "stenosis", "--solver", "stabilized_schur", "--T", "0.02", "--dt", "0.01", "--output_dir", str(tmp_path),
            "--quiet", "True", "--ny", "6", "--L", "12.0", "--x_sten", "5.0", "--particles", "50", "--particles_every", "2", "--particles_nsub", "3"]
    assert main(argv) == 0
    assert seen["particles"] == {"n": 50, "every": 2, "nsub": 3}
