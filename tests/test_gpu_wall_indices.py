"""GPU tests of the wall shear stress on the P2/P1 context and of the cycle-averaged wall shear indices (csrc/cfdh_wallstats.hip,
cfdh_wall_stats_*, the plugin methods and `Scenario.solve(..., wall_indices=...)`): the device field against a quadrature twin
(tests/wss_p2_twin.py) and against the Newton context, the accumulated sums and derived indices against
wall_indices.indices_from_sums, the special values of reversing / unidirectional flow, error codes, and the window of the time loop.

The accumulation count is cfdh_info(ctx, 90) on every context kind; a pressure-correction context answers 84 as well (on the
Newton contexts 84 has long been the FGMRES cycle counter, tests/test_gpu_solve_lean.py)."""
import ctypes
import os

import numpy as np
import pytest

import wss_p2_twin
from gen3_util import node_mesh3
from gen_util import node_mesh

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
from cfd_hemodynamic_amd.wall_indices import FIELDS, indices_from_sums

pytestmark = pytest.mark.gpu
COUNT = _lib.INFO_WALL_STATS_COUNT
WEIGHTS = [0.3, 0.7, 0.1, 0.4, 0.5]


def _ipcs_mesh(dim):
    m = create_unit_square(3) if dim == 2 else create_unit_cube(2)
    return m, (NodeMesh(m) if dim == 2 else NodeMesh3D(m))


def _ipcs_ctx(m, nm, mu):
    """Built as tests/test_gpu_ipcs.py builds its contexts."""
    ctx = _lib.IpcsContext(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, np.zeros(len(nm.facet_cells), dtype=np.int32))
    ctx.set_params(0.01, 1.0, mu, f=np.zeros(m.x.shape[1]))
    return ctx


@pytest.mark.parametrize("dim", [2, 3], ids=["2d", "3d"])
def test_ipcs_wss_matches_the_twin(dim):
    m, nm = _ipcs_mesh(dim)
    rng = np.random.default_rng(7)
    u = rng.standard_normal(nm.x.shape)
    mu = 0.7
    ctx = _ipcs_ctx(m, nm, mu)
    ctx.set_state(u=u.ravel(), p=np.zeros(m.num_vertices))
    w1 = ctx.wall_shear_stress()
    w2 = ctx.wall_shear_stress()
    ctx.close()
    tw = wss_p2_twin.wall_shear_stress(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, u, mu)
    err = np.abs(w1.reshape(-1, dim) - tw).max() / np.abs(tw).max()
    print("ipcs wss gdim %d (%d vertices, %d facets): max |device - twin| / max |twin| = %.3e" % (dim, m.num_vertices, len(nm.facet_cells), err))
    assert err <= 1e-12
    assert w1.tobytes() == w2.tobytes()
    off_wall = np.setdiff1d(np.arange(m.num_vertices), np.unique(m.facet_vertices))
    if dim == 2:
        assert len(off_wall) > 0
    assert not w1.reshape(-1, dim)[off_wall].any()
    assert np.abs(tw).max() > 0


def test_ipcs_wss_of_a_quadratic_shear():
    """u = (y^2, 0), mu = 1: T = -(grad u + grad u^T) n gives (-2, 0) on y = 1 and 0 on y = 0."""
    m = create_unit_square(4)
    nm = NodeMesh(m)
    u = np.stack([nm.x[:, 1] ** 2, np.zeros(len(nm.x))], axis=1)
    ctx = _ipcs_ctx(m, nm, 1.0)
    ctx.set_state(u=u.ravel(), p=np.zeros(m.num_vertices))
    w = ctx.wall_shear_stress().reshape(-1, 2)
    ctx.close()
    inner = (m.x[:, 0] > 1e-9) & (m.x[:, 0] < 1.0 - 1e-9)
    top, bottom = inner & np.isclose(m.x[:, 1], 1.0), inner & np.isclose(m.x[:, 1], 0.0)
    assert top.sum() == 3 and bottom.sum() == 3
    assert np.abs(w[top] - np.array([-2.0, 0.0])).max() <= 1e-13
    assert np.abs(w[bottom]).max() <= 1e-13


def test_ipcs_wss_of_a_p1_field_equals_the_newton_context():
    m = create_unit_square(4)
    nm = NodeMesh(m)
    rng = np.random.default_rng(7)
    uv = rng.standard_normal((m.num_vertices, 2))
    u = np.vstack([uv, 0.5 * (uv[nm.edges[:, 0]] + uv[nm.edges[:, 1]])])
    mu = 0.7
    ctx = _ipcs_ctx(m, nm, mu)
    ctx.set_state(u=u.ravel(), p=np.zeros(m.num_vertices))
    wi = ctx.wall_shear_stress()
    ctx.close()
    c1 = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    c1.set_params(0.01, 1.0, mu, f=(0.0, 0.0))
    c1.set_state(u_prev=uv.ravel(), p_prev=np.zeros(m.num_vertices), u=uv.ravel(), p=np.zeros(m.num_vertices))
    wn = c1.wall_shear_stress()
    c1.close()
    assert np.abs(wn).max() > 0
    assert np.abs(wi - wn).max() <= 1e-13 * np.abs(wn).max()


def _stats_ctx(kind):
    """(context, gdim, vertices of the wall-shear field, velocity nodes, pressure nodes)."""
    if kind in ("ipcs2d", "ipcs3d"):
        m, nm = _ipcs_mesh(2 if kind == "ipcs2d" else 3)
        return _ipcs_ctx(m, nm, 0.7), m.x.shape[1], m.num_vertices, len(nm.x), m.num_vertices
    if kind == "p1tri":
        m, et = create_unit_square(4), 0
    elif kind == "p1tet":
        m, et = create_unit_cube(3), 0
    elif kind == "q1hex":
        m, et = node_mesh3("Q1"), 2
    else:
        m, et = node_mesh("P2"), 1
    ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, np.zeros(len(m.facet_cells), dtype=np.int32), etype=et)
    d = m.x.shape[1]
    ctx.set_params(0.01, 1.0, 0.7, f=np.zeros(d))
    return ctx, d, m.num_vertices, m.num_vertices, m.num_vertices


def _wall_mask(kind):
    """The vertices of the wall-shear field of _stats_ctx(kind) that lie on an exterior facet, from the mesh alone."""
    from post_twin import PostTwin
    if kind in ("ipcs2d", "ipcs3d"):
        m, _ = _ipcs_mesh(2 if kind == "ipcs2d" else 3)
        mask = np.zeros(m.num_vertices, dtype=bool)
        mask[np.unique(m.facet_vertices)] = True
        return mask
    m = {"p1tri": lambda: create_unit_square(4), "p1tet": lambda: create_unit_cube(3), "q1hex": lambda: node_mesh3("Q1"), "p2tri": lambda: node_mesh("P2")}[kind]()
    return PostTwin(m.x, m.cells, m.facet_cells, m.facet_local).wall_nodes()


def _set_state(ctx, u, p):
    if isinstance(ctx, _lib.IpcsContext):
        ctx.set_state(u=u.ravel(), p=p)
    else:
        ctx.set_state(u_prev=u.ravel(), p_prev=p, u=u.ravel(), p=p)


def _wss(ctx, d):
    return ctx.wall_shear_stress().reshape(-1, d)


@pytest.mark.parametrize("kind", ["p1tri", "p1tet", "q1hex", "p2tri", "ipcs2d", "ipcs3d"])
def test_sums_and_indices_match_numpy(kind):
    ctx, d, nv, nu, npr = _stats_ctx(kind)
    rng = np.random.default_rng(7)
    S, A, M, W = np.zeros((nv, d)), np.zeros(nv), np.zeros(nv), 0.0
    ctx.wall_stats_reset()
    for w in WEIGHTS:
        _set_state(ctx, rng.standard_normal((nu, d)), rng.standard_normal(npr))
        tau = _wss(ctx, d)
        assert tau.shape == (nv, d)
        mag = np.sqrt((tau * tau).sum(axis=1))
        S += w * tau
        A += w * mag
        M = np.maximum(M, mag)
        W += w
        ctx.wall_stats_accumulate(w)
    ref = indices_from_sums(S, A, M, W)
    dev = {k: ctx.wall_stats_get(i) for i, k in enumerate(FIELDS)}
    totals = ctx.wall_stats_get(_lib.WALL_TOTALS)
    wall = A > 0
    assert wall.any() and np.isfinite(ref["rrt"]).all()
    # "zero away from the boundary": the accumulated field marks exactly the vertices on an exterior facet, and every index is 0 elsewhere
    # (an interior vertex that received rounding noise would have A > 0, an OSI formed from noise and an RRT of order 1e16)
    geo = _wall_mask(kind)
    assert geo.shape == wall.shape and np.array_equal(wall, geo), "A > 0 on %d vertices off the wall" % int((wall & ~geo).sum())
    assert (~geo).any()
    for k in ("tawss", "osi", "rrt", "wss_peak"):
        assert np.array_equal(dev[k][~geo], np.zeros(int((~geo).sum()))), k
    assert np.array_equal(dev["wss_mean"][~geo], np.zeros((int((~geo).sum()), d)))
    errs = {k: np.abs(dev[k] - ref[k]).max() / np.abs(ref[k]).max() for k in ("tawss", "wss_mean", "wss_peak")}
    errs["osi"] = np.abs(dev["osi"] - ref["osi"]).max()
    errs["rrt"] = (np.abs(dev["rrt"] - ref["rrt"])[wall] / ref["rrt"][wall]).max()
    print("wall indices %s (%d vertices, %d on the wall): min A / max A on the wall %.3f, OSI in [%.3f, %.3f], errors %s"
          % (kind, nv, wall.sum(), A[wall].min() / A.max(), ref["osi"][wall].min(), ref["osi"][wall].max(),
             {k: "%.2e" % v for k, v in errs.items()}))
    for k in ("tawss", "wss_mean", "wss_peak"):
        assert dev[k].shape == ref[k].shape and errs[k] <= 1e-13, (k, errs[k])
    assert errs["osi"] <= 1e-12          # absolute, on every vertex
    assert errs["rrt"] <= 1e-11          # relative, on every wall vertex
    assert not dev["rrt"][~wall].any() and not dev["osi"][~wall].any()
    assert abs(totals[0] - 2.0) <= 1e-15 and totals[1] == 5.0
    assert ctx.info(COUNT) == 5
    if kind.startswith("ipcs"):
        assert ctx.info(84) == 5
    ctx.wall_stats_reset()
    assert ctx.info(COUNT) == 0
    if kind.startswith("ipcs"):
        assert ctx.info(84) == 0
    ctx.close()


def test_reversing_and_unidirectional_flow():
    ctx, d, nv, nu, npr = _stats_ctx("p1tri")
    rng = np.random.default_rng(7)
    s, p = rng.standard_normal((nu, d)), rng.standard_normal(npr)
    _set_state(ctx, s, p)
    wall = np.sqrt((_wss(ctx, d) ** 2).sum(axis=1)) > 0
    assert wall.any() and (~wall).any()
    ctx.wall_stats_reset()
    for sign in (1.0, -1.0):
        _set_state(ctx, sign * s, p)
        ctx.wall_stats_accumulate(0.5)
    osi, rrt = ctx.wall_stats_get(_lib.WALL_OSI), ctx.wall_stats_get(_lib.WALL_RRT)
    assert (osi[wall] == 0.5).all() and np.isposinf(rrt[wall]).all()
    assert (rrt[~wall] == 0.0).all() and (osi[~wall] == 0.0).all()
    ctx.wall_stats_reset()
    S, W = np.zeros((nv, d)), 0.0
    for k, w in ((1.0, 0.25), (2.0, 0.5), (0.5, 0.25)):
        _set_state(ctx, k * s, p)
        S += w * _wss(ctx, d)
        W += w
        ctx.wall_stats_accumulate(w)
    osi, rrt = ctx.wall_stats_get(_lib.WALL_OSI), ctx.wall_stats_get(_lib.WALL_RRT)
    assert (osi >= 0.0).all() and osi.max() <= 1e-15
    sn = np.sqrt((S * S).sum(axis=1))
    assert np.abs(rrt[wall] * sn[wall] / W - 1.0).max() <= 1e-14
    assert (rrt[~wall] == 0.0).all()
    ctx.close()


@pytest.mark.parametrize("kind", ["p1tri", "ipcs2d"])
def test_error_codes(kind):
    ctx, d, nv, nu, npr = _stats_ctx(kind)
    L, h = ctx.L, ctx.h
    n = ctypes.c_int64()
    rng = np.random.default_rng(7)
    _set_state(ctx, rng.standard_normal((nu, d)), rng.standard_normal(npr))
    assert L.cfdh_wall_stats_get(h, 0, ctypes.byref(n), None) == -3
    assert L.cfdh_wall_stats_get(h, 5, ctypes.byref(n), None) == -3
    assert L.cfdh_wall_stats_accumulate(h, 0.5) == -3
    assert L.cfdh_wall_stats_reset(h) == 0
    assert L.cfdh_wall_stats_get(h, 0, ctypes.byref(n), None) == -3      # nothing accumulated: W == 0
    assert L.cfdh_wall_stats_get(h, 5, ctypes.byref(n), None) == 0 and n.value == 2
    for w in (0.0, -1.0, float("nan"), float("inf")):
        assert L.cfdh_wall_stats_accumulate(h, w) == -1
    assert ctx.info(COUNT) == 0
    assert L.cfdh_wall_stats_get(h, 9, ctypes.byref(n), None) == -1
    assert L.cfdh_wall_stats_get(h, -1, ctypes.byref(n), None) == -1
    assert L.cfdh_wall_stats_accumulate(h, 0.5) == 0
    assert L.cfdh_wall_stats_get(h, 0, ctypes.byref(n), None) == 0 and n.value == nv
    assert L.cfdh_wall_stats_get(h, 3, ctypes.byref(n), None) == 0 and n.value == nv * d
    assert L.cfdh_wall_shear_stress(h, None) == 0
    with pytest.raises(ValueError):
        ctx.wall_stats_accumulate(-1.0)
    ctx.close()


def _scenario(name, **kw):
    if name == "stabilized_schur":
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        sc = StenosisSimulation("stabilized_schur", 0.01, 0.06, ny=6, L=12.0, x_sten=5.0, v_max=100.0, quiet=True, **kw)   # no inlet flow without v_max
    else:
        from cfd_hemodynamic_amd.scenarios.taylor_green import TaylorGreenSimulation
        sc = TaylorGreenSimulation("ipcs_bdf2", 0.01, 0.06, nx=8, quiet=True, **kw)
    sc.early_stop_tolerance = 0
    return sc


CLI = {"stabilized_schur": ["--simulation", "stenosis", "--solver", "stabilized_schur", "--ny", "6", "--L", "12.0", "--x_sten", "5.0", "--v_max", "100.0"],
       "ipcs_bdf2": ["--simulation", "taylor_green", "--solver", "ipcs_bdf2", "--nx", "8"]}
FILES = ("wall_indices.npz", "wall_indices.vtu", "wall_indices.txt")


@pytest.mark.parametrize("name", ["stabilized_schur", "ipcs_bdf2"])
@pytest.mark.filterwarnings("ignore::RuntimeWarning")   # taylor_green imposes a non-zero pressure value (the ipcs plugin warns once)
def test_scenario_window(name, tmp_path):
    from cfd_hemodynamic_amd.__main__ import main
    from cfd_hemodynamic_amd.io import read_vtu
    sc = _scenario(name)
    sc.setup()
    rec = []
    out = str(tmp_path / "on")
    sc.solve(out, afterStepCallback=lambda t: rec.append((t, np.array(sc.solver.shear_stress.x.array, copy=True))), wall_indices=(0.02, 0.05))
    assert sc.num_steps == 6 and len(rec) == 6
    wi = sc.wall_indices
    assert wi["steps"] == 3 and abs(wi["W"] - 0.03) <= 1e-15
    assert sc.solver.ctx.info(COUNT) == 3
    d = sc.mesh.geometry.dim
    taus = [w.reshape(-1, d) for _, w in rec[2:5]]   # the steps that end at 0.03, 0.04, 0.05
    assert [round(t, 6) for t, _ in rec[2:5]] == [0.03, 0.04, 0.05]
    S = sum(0.01 * w for w in taus)
    A = sum(0.01 * np.sqrt((w * w).sum(axis=1)) for w in taus)
    assert A.max() > 0
    assert np.abs(wi["tawss"] - A / 0.03).max() <= 1e-12 * (A / 0.03).max()
    assert np.abs(wi["wss_mean"] - S / 0.03).max() <= 1e-12 * np.abs(S / 0.03).max()
    for f in FILES:
        assert os.path.exists(os.path.join(out, f)), f
    z = np.load(os.path.join(out, "wall_indices.npz"))
    for k in FIELDS:
        assert np.array_equal(z[k], wi[k]), k
    assert float(z["W"]) == wi["W"] and int(z["steps"]) == 3
    assert z["x"].shape == (len(wi["tawss"]), d) and z["cells"].shape[1] == d + 1
    v = read_vtu(os.path.join(out, "wall_indices.vtu"))
    assert np.array_equal(v["tawss"].ravel(), wi["tawss"]) and np.array_equal(v["osi"].ravel(), wi["osi"])
    text = open(os.path.join(out, "wall_indices.txt")).read()
    assert "steps: 3" in text and "TAWSS max" in text and "OSI max" in text and "RRT max" in text
    # off: no file, no accumulation, nothing allocated
    sc2 = _scenario(name)
    sc2.setup()
    out2 = str(tmp_path / "off")
    sc2.solve(out2)
    assert sc2.wall_indices is None and sc2.solver.ctx.info(COUNT) == 0
    for f in FILES:
        assert not os.path.exists(os.path.join(out2, f)), f
    n = ctypes.c_int64()
    assert sc2.solver.ctx.L.cfdh_wall_stats_get(sc2.solver.ctx.h, 5, ctypes.byref(n), None) == -3   # never reset: no accumulators
    # command line
    assert main(["simulate", "--T", "0.06", "--dt", "0.01", "--name", "run", "--output_dir", str(tmp_path / "cli"), "--quiet", "True",
                 "--wall_indices_from", "0.02", "--wall_indices_to", "0.05"] + CLI[name]) == 0
    zc = np.load(str(tmp_path / "cli" / CLI[name][1] / "run" / "wall_indices.npz"))
    assert float(zc["W"]) == wi["W"] and int(zc["steps"]) == 3
