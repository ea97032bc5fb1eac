"""Volumetric flow diagnostics on the device (cfdh_flow_*, csrc/cfdh_flow.hip): the closed forms of test_flow_twin.py on affine
fields (G_v = A at every vertex of any mesh), non-affine fields against the NumPy twin (flow_twin.py) on the cube, the stenosed
channel and the bifurcation, the window averages, repeatability, the untouched flow step, refusals, and the scenario /
command-line routes.

Meshes: 81 and 125 vertices (one full slice of 64 and a partly filled one), 343 and 1681 vertices (several workgroups), one triangle
and one tetrahedron (a single partly filled slice).  Every comparison prints its error next to its bound before it asserts."""
import os

import numpy as np
import pytest

import flow_twin as T
import flow_util as U
from cfd_hemodynamic_amd import _lib
from util import dfg_case, make_ctx

pytestmark = pytest.mark.gpu

INFO = (_lib.INFO_FLOW_BUFFERS, _lib.INFO_FLOW_CELL_PASSES, _lib.INFO_FLOW_STATS_COUNT)
STATS = ("mean_velocity", "fluctuation", "mean_dissipation", "mean_shear_rate", "peak_shear_rate")  # _lib.FLOW_MEAN_U ..
_CTX = {}


def set_u(ctx, m, u):
    z = np.zeros(m.nv)
    u = np.ascontiguousarray(u).ravel()
    ctx.set_state(u_prev=u, p_prev=z, u=u, p=z)


def context(m, u=None, mu=U.MU):
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    ctx.set_params(0.01, U.RHO, mu)
    if u is not None:
        set_u(ctx, m, u)
    return ctx


def shared(name):
    """One context per mesh for the tests that only set a state and read fields."""
    if name not in _CTX:
        _CTX[name] = context(U.mesh(name))
    return _CTX[name]


@pytest.fixture(scope="module", autouse=True)
def _close_shared_contexts():
    yield
    for ctx in _CTX.values():
        ctx.close()
    _CTX.clear()


def names(m):
    return ("gradient",) + (U.FIELDS_3D if m.d == 3 else U.FIELDS_2D)


def device_result(ctx, m):
    res = {k: ctx.flow_field(_lib.FLOW_FIELDS[k]) for k in names(m)}
    res["integrals"] = ctx.flow_integrals()
    return res


def infos(ctx):
    return tuple(ctx.info(w) for w in INFO)


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("mesh_name,case_name", U.affine_cases())
def test_closed_forms(mesh_name, case_name):
    """Rigid rotation, simple shear, pure strain, uniform dilatation, a full non-symmetric A with b, and the helical field in 3-D:
    every vertex field and the stated integrals to 1e-12 of their natural scale."""
    case = U.affine_case(mesh_name, case_name)
    m = case["m"]
    ctx = shared(mesh_name)
    set_u(ctx, m, case["u"])
    res = device_result(ctx, m)
    assert res["gradient"].shape == (m.nv, m.d, m.d) and res["vorticity"].shape == ((m.nv,) if m.d == 2 else (m.nv, 3))
    assert U.check_affine(case, res)


# ------------------------------------------------------------------------------------------------------------ against the twin
@pytest.mark.parametrize("name", ["cube", "stenosis", "bifurcation"])
def test_random_fields_match_the_twin(name):
    """G_v, every vertex field and all 8 integrals to 1e-11 of their scale; LNH to 1e-9 absolute where |u||omega| is at least 1e-6
    of its maximum (at most 1 % of the vertices may fall below: a condition of the test)."""
    case = U.twin_case(name)
    m = case["m"]
    ctx = shared(name)
    set_u(ctx, m, case["u"])
    assert U.check_twin(case, device_result(ctx, m))


def test_lnh_is_zero_where_the_velocity_is():
    m = U.mesh("cube")
    u = U.random_field("cube").copy()
    at = np.array([0, 63, 64, 124])
    u[at] = 0.0
    ctx = shared("cube")
    set_u(ctx, m, u)
    lnh = ctx.flow_field(_lib.FLOW_LNH)
    hel = ctx.flow_field(_lib.FLOW_HELICITY)
    assert (lnh[at] == 0.0).all() and (hel[at] == 0.0).all() and not np.signbit(lnh[at]).any()
    rest = np.setdiff1d(np.arange(m.nv), at)
    assert (np.abs(lnh[rest]) > 0).all() and (np.abs(lnh) <= 1.0 + 1e-15).all()
    # ... and where the vorticity is: a uniform velocity
    set_u(ctx, m, np.tile([0.3, -0.2, 0.9], (m.nv, 1)))
    assert (ctx.flow_field(_lib.FLOW_LNH) == 0.0).all()


# ------------------------------------------------------------------------------------------------------------- window averages
@pytest.mark.parametrize("name", ["stenosis", "cube"])
def test_window_averages(name):
    m = U.mesh(name)
    ua, ub = U.window_fields(name)
    wa, wb = 0.3, 0.7
    ctx = context(m, ua)
    assert infos(ctx) == (0, 0, 0)
    with pytest.raises(_lib.CfdhError):  # before a reset: CFDH_E_STATE
        ctx.flow_stats_accumulate(wa)
    with pytest.raises(_lib.CfdhError):
        ctx.flow_stats_get(_lib.FLOW_MEAN_U)
    with pytest.raises(_lib.CfdhError):
        ctx.flow_stats_get(_lib.FLOW_TOTALS)
    assert infos(ctx) == (0, 0, 0)
    ctx.flow_stats_reset()
    assert infos(ctx) == (1, 0, 0)
    assert ctx.flow_stats_get(_lib.FLOW_TOTALS).tolist() == [0.0, 0.0]
    with pytest.raises(_lib.CfdhError):  # W == 0: CFDH_E_STATE
        ctx.flow_stats_get(_lib.FLOW_MEAN_SHEAR_RATE)
    for bad in (0.0, -1.0, np.nan, np.inf):  # CFDH_E_ARG, nothing accumulated
        with pytest.raises(ValueError):
            ctx.flow_stats_accumulate(bad)
    with pytest.raises(ValueError):
        ctx.flow_stats_get(6)
    with pytest.raises(ValueError):
        ctx.flow_stats_get(-1)
    assert infos(ctx) == (1, 0, 0)
    ctx.flow_stats_accumulate(wa)
    assert infos(ctx) == (1, 1, 1)
    set_u(ctx, m, ub)
    ctx.flow_stats_accumulate(wb)
    assert infos(ctx) == (1, 2, 2)
    got = {k: ctx.flow_stats_get(w) for w, k in enumerate(STATS)}
    assert ctx.flow_stats_get(_lib.FLOW_TOTALS).tolist() == [1.0, 2.0]
    # pointwise in the nodal values: a handful of roundings
    umax = max(np.abs(ua).max(), np.abs(ub).max())
    mean = (wa * ua + wb * ub) / (wa + wb)
    k = np.maximum(0.0, 0.5 * ((wa * (ua * ua).sum(axis=1) + wb * (ub * ub).sum(axis=1)) / (wa + wb) - (mean * mean).sum(axis=1)))
    assert got["mean_velocity"].shape == (m.nv, m.d)
    assert U._worst("mean velocity", got["mean_velocity"], mean, 1e-13 * umax)
    assert U._worst("k'", got["fluctuation"], k, 1e-13 * umax * umax) and k.max() > 0.01 * umax * umax
    # through the recovery: against the twin
    win = T.Window(m.x, m.cells, U.MU)
    win.accumulate(ua, wa)
    win.accumulate(ub, wb)
    ref = win.get()
    g = max(np.sqrt((T.fields(m.x, m.cells, f, U.MU)["gradient"] ** 2).sum(axis=(1, 2))).max() for f in (ua, ub))
    assert U._worst("mean phi", got["mean_dissipation"], ref["mean_dissipation"], U.TOL_TWIN * U.MU * g * g)
    assert U._worst("mean gamma", got["mean_shear_rate"], ref["mean_shear_rate"], U.TOL_TWIN * g)
    assert U._worst("peak gamma", got["peak_shear_rate"], ref["peak_shear_rate"], U.TOL_TWIN * g)
    assert (got["peak_shear_rate"] >= got["mean_shear_rate"] * (1 - 1e-14)).all()
    # a second reset zeroes everything
    ctx.flow_stats_reset()
    assert infos(ctx) == (1, 2, 0) and ctx.flow_stats_get(_lib.FLOW_TOTALS).tolist() == [0.0, 0.0]
    with pytest.raises(_lib.CfdhError):
        ctx.flow_stats_get(_lib.FLOW_PEAK_SHEAR_RATE)
    ctx.flow_stats_accumulate(1.0)
    again = {k: ctx.flow_stats_get(w) for w, k in enumerate(STATS)}
    assert np.array_equal(again["mean_velocity"], ub) and (again["fluctuation"] <= 1e-15 * umax * umax).all()
    assert U._worst("peak after reset", again["peak_shear_rate"], T.fields(m.x, m.cells, ub, U.MU)["shear_rate"], U.TOL_TWIN * g)
    ctx.close()


# -------------------------------------------------------------------------------------------------- repeatability and isolation
def _all_bytes(ctx, m):
    res = device_result(ctx, m)
    out = b"".join(np.ascontiguousarray(res[k]).tobytes() for k in names(m) + ("integrals",))
    ctx.flow_stats_reset()
    ctx.flow_stats_accumulate(0.4)
    ctx.flow_stats_accumulate(0.6)
    return out + b"".join(ctx.flow_stats_get(w).tobytes() for w in range(6))


@pytest.mark.parametrize("name", ["stenosis", "bifurcation"])
def test_same_bytes(name):
    """Two calls of every entry point on one state, and a second context on the same mesh."""
    case = U.twin_case(name)
    m = case["m"]
    a = context(m, case["u"])
    first, second = _all_bytes(a, m), _all_bytes(a, m)
    b = context(m, case["u"])
    third = _all_bytes(b, m)
    a.close()
    b.close()
    assert first == second == third


def _every_call(ctx, dim):
    for w in range(5 if dim == 2 else 7):
        ctx.flow_field(w)
    ctx.flow_integrals()
    ctx.flow_stats_accumulate(0.01)
    for w in range(6):
        ctx.flow_stats_get(w)


def test_flow_step_is_untouched():
    """u and p of three steps, bit for bit, with every diagnostics call made between the steps and without; a context that never
    calls the feature reports 0 for cfdh_info 106 - 108."""
    case = dfg_case(6)
    out = []
    for on in (False, True):
        ctx = make_ctx(case)
        z = np.zeros(case.nv)
        ctx.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.zeros(2 * case.nv), p=z)
        if on:
            ctx.flow_stats_reset()
        for k in range(3):
            ctx.solve_step()
            if on:
                _every_call(ctx, 2)
            u, p = ctx.get_solution()
            out.append((u.copy(), p.copy()))
            ctx.advance()
        if on:
            assert infos(ctx) == (1, 3 * 6, 3) and ctx.flow_stats_get(_lib.FLOW_PEAK_SHEAR_RATE).max() > 0
        else:
            assert infos(ctx) == (0, 0, 0)
        ctx.close()
    for k in range(3):
        assert out[k][0].tobytes() == out[3 + k][0].tobytes() and out[k][1].tobytes() == out[3 + k][1].tobytes()
        assert np.abs(out[k][0]).max() > 0


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    m = U.mesh("square")
    ctx = context(m)
    n_before = infos(ctx)
    with pytest.raises(_lib.CfdhError):  # no state yet: CFDH_E_STATE
        ctx.flow_field(_lib.FLOW_VORTICITY)
    with pytest.raises(_lib.CfdhError):
        ctx.flow_integrals()
    set_u(ctx, m, U.random_field("cube")[:m.nv, :2])
    for which in (_lib.FLOW_HELICITY, _lib.FLOW_LNH, 7, -1, 100):  # helicity and LNH in 2-D, unknown fields: CFDH_E_ARG
        with pytest.raises(ValueError):
            ctx.flow_field(which)
    assert infos(ctx) == n_before == (0, 0, 0)
    assert ctx.flow_field(_lib.FLOW_VORTICITY).shape == (m.nv,)  # usable after every refusal
    assert infos(ctx) == (1, 1, 0)
    ctx.close()
    no_params = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    set_u(no_params, m, np.ones((m.nv, 2)))
    with pytest.raises(_lib.CfdhError):  # the dissipation needs mu
        no_params.flow_field(_lib.FLOW_DISSIPATION)
    assert (no_params.flow_field(_lib.FLOW_SHEAR_RATE) <= 1e-14).all()
    no_params.close()


def _refused(ctx):
    calls = [(ctx.flow_field, _lib.FLOW_VORTICITY), (ctx.flow_integrals,), (ctx.flow_stats_reset,), (ctx.flow_stats_accumulate, 0.1),
             (ctx.flow_stats_get, _lib.FLOW_TOTALS)]
    for fn, *a in calls:
        with pytest.raises(ValueError) as e:
            fn(*a)
        assert len(str(e.value)) > 20  # a reason
    assert infos(ctx) == (0, 0, 0)


def test_unsupported_contexts_refuse():
    """Generic-element contexts, pressure-correction contexts and parts of a partitioned run: CFDH_E_ARG with a reason from every
    entry point, the context unchanged; a valid context on the same mesh works."""
    from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
    from gen_util import node_mesh
    case = dfg_case(4)
    m = case.mesh
    gen = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker, etype=3)
    _refused(gen)
    gen.close()
    p2 = node_mesh("P2", 3, 0.1)
    nvert = int(p2.cells[:, :3].max()) + 1
    ip = _lib.IpcsContext(p2.x, p2.cells, nvert, p2.facet_cells, p2.facet_local, p2.facet_marker)
    _refused(ip)
    ip.close()
    lp = LocalPart(m, partition_vertices_rcb(m.x, 2), 0)
    part = _lib.Context(lp.x, lp.cells, lp.facet_cells, lp.facet_local, lp.facet_marker, nv_owned=lp.nvo)
    _refused(part)
    part.close()
    ok = make_ctx(case)
    z = np.zeros(case.nv)
    ok.set_state(u_prev=np.zeros(2 * case.nv), p_prev=z, u=np.ones(2 * case.nv), p=z)
    assert ok.flow_integrals()[0] > 0 and infos(ok) == (0, 0, 0)  # the integrals need no buffer
    ok.flow_stats_reset()
    assert infos(ok) == (1, 0, 0)
    ok.close()


# -------------------------------------------------------------------------------------------------------------------- scenario
def test_scenario_stenosis(tmp_path):
    from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
    out = str(tmp_path / "run")
    sc = StenosisSimulation("stabilized_schur", 0.01, 0.04, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True)
    sc.early_stop_tolerance = 0
    sc.setup()
    sc.solve(output_folder=out, max_steps=4, flow_diagnostics={"fields": ("vorticity", "shear_rate"), "window": (0.01, 0.04)})
    F = sc.flow_diagnostics
    assert F["integrals"].shape == (4, 8) and np.allclose(F["times"], 0.01 * np.arange(1, 5))
    area = float(sc.mesh.cell_areas().sum())
    assert abs(F["integrals"][:, 0] - area).max() <= 1e-12 * area
    assert (F["integrals"][:, 1] > 0).all() and (F["integrals"][:, 3] > 0).all() and (F["integrals"][:, 4] == 0).all()
    W = F["window"]
    assert W["steps"] == 3 and abs(W["W"] - 0.03) <= 1e-15  # the steps that end in (0.01, 0.04]
    assert abs(W["energy_loss"] - 0.01 * F["integrals"][1:, 3].sum()) <= 1e-12 * W["energy_loss"]
    assert W["mean_velocity"].shape == (sc.mesh.num_vertices, 2) and (W["peak_shear_rate"] >= W["mean_shear_rate"] * (1 - 1e-14)).all()
    z = np.load(os.path.join(out, "flow_diagnostics.npz"))
    assert np.array_equal(z["integrals"], F["integrals"]) and np.array_equal(z["window_mean_shear_rate"], W["mean_shear_rate"])
    txt = open(os.path.join(out, "flow_diagnostics.txt")).read()
    assert "energy loss" in txt and len([ln for ln in txt.splitlines() if not ln.startswith("#")]) == 4
    for k in ("vorticity", "shear_rate"):
        assert any(f.startswith(k) for f in os.listdir(out)), os.listdir(out)
    # the last frame of the series holds the field of the last step
    assert np.abs(sc.solver.flow_field("shear_rate")).max() > 0
    with pytest.raises(ValueError):
        sc.solve(max_steps=1, flow_diagnostics={"fields": ("lnh",)})  # 3-D only


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
            "--quiet", "True", "--ny", "6", "--L", "12.0", "--x_sten", "5.0", "--flow_fields", "vorticity,q_criterion", "--flow_window_from", "0.01"]
    assert main(argv) == 0
    assert seen["flow_diagnostics"] == {"fields": ("vorticity", "q_criterion"), "window": (0.01, 0.02)}
    seen.clear()
    assert main(argv[:-4]) == 0
    assert "flow_diagnostics" not in seen
