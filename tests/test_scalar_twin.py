"""The passive-scalar twin (scalar_twin.py) against its definition, on the CPU: closed-form element matrices against a high-order
quadrature of the same integrands, conservation properties, the steady uniform-flow age c = x / U, and the host work-list builder
of the device assembly (csrc/cfdh_scalar_host.hpp) in a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

import numpy as np
import pytest

import scalar_twin as T
import scalar_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")


def duffy_rule(d, n=6):
    """Barycentric points [nq, d + 1] and weights (summing to 1) on the simplex: tensor Gauss-Legendre collapsed by the Duffy
    map; exact for polynomials of degree 2 n - 1 - (d - 1) at least."""
    t, w = np.polynomial.legendre.leggauss(n)
    t, w = 0.5 * (t + 1.0), 0.5 * w
    if d == 2:
        r, s = np.meshgrid(t, t, indexing="ij")
        wr, ws = np.meshgrid(w, w, indexing="ij")
        l1, l2 = r, s * (1 - r)
        wt = wr * ws * (1 - r) * 2.0
        lam = np.stack([1 - l1 - l2, l1, l2], axis=-1)
    else:
        r, s, q = np.meshgrid(t, t, t, indexing="ij")
        wr, ws, wq = np.meshgrid(w, w, w, indexing="ij")
        l1, l2, l3 = r, s * (1 - r), q * (1 - r) * (1 - s)
        wt = wr * ws * wq * (1 - r) ** 2 * (1 - s) * 6.0
        lam = np.stack([1 - l1 - l2 - l3, l1, l2, l3], axis=-1)
    return lam.reshape(-1, d + 1), wt.ravel()


@pytest.mark.parametrize("name", ["rectangle", "box"])
@pytest.mark.parametrize("theta,D,s", U.PARAMS)
def test_element_matrices_equal_quadrature(name, theta, D, s):
    mesh = U.MESHES[name]()
    d = mesh.x.shape[1]
    fl = U.fields(mesh)
    E = T.element_matrices(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], U.DT, D, s, theta)
    lam, wt = duffy_rule(d)
    assert abs(wt.sum() - 1.0) < 1e-14
    # the definitions, restated: wbar, tau_c, p_a
    g, vol, h = T.geometry(mesh.x, mesh.cells)
    assert np.allclose(vol, mesh.cell_areas() if d == 2 else mesh.cell_volumes(), rtol=1e-14) and np.allclose(h, mesh.h(), rtol=1e-15)
    wv = (theta * fl["u_sol"] + (1 - theta) * fl["u_prev"])[mesh.cells]
    wbar = wv.sum(axis=1) / (d + 1)
    tau = ((2 / U.DT) ** 2 + (2 * np.sqrt((wbar ** 2).sum(axis=1)) / h) ** 2 + (4 * D / h ** 2) ** 2) ** -0.5
    p = tau[:, None] * np.einsum("ci,cai->ca", wbar, g)
    wq = np.einsum("qc,kci->kqi", lam, wv)                       # w(x_q) per cell k
    ref = dict(
        M=vol[:, None, None] * np.einsum("q,qa,qb->ab", wt, lam, lam)[None],
        C=vol[:, None, None] * np.einsum("q,qa,kqi,kbi->kab", wt, lam, wq, g),
        K=D * vol[:, None, None] * np.einsum("kai,kbi->kab", g, g) * wt.sum(),
        Ms=vol[:, None, None] * np.einsum("ka,q,qb->kab", p, wt, lam),
        Cs=vol[:, None, None] * np.einsum("ka,ki,kbi->kab", p, wbar, g) * wt.sum(),
        b=s * vol[:, None] * (np.einsum("q,qa->a", wt, lam)[None] + p * wt.sum()),
    )
    for k, r in ref.items():
        assert np.abs(E[k] - r).max() <= 1e-13, (k, np.abs(E[k] - r).max())
    # the set-up the GPU tests rely on: wbar is exactly zero in one cell and nowhere else
    z = np.all(E["wbar"] == 0.0, axis=1)
    assert z[fl["zero_cell"]] and z.sum() == 1


@pytest.mark.parametrize("name", ["rectangle", "box"])
@pytest.mark.parametrize("theta,D", [(0.5, 0.0), (1.0, 2e-2)])
def test_constant_field_stays_constant(name, theta, D):
    mesh = U.MESHES[name]()
    fl = U.fields(mesh)
    E = T.element_matrices(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], U.DT, D, 0.0, theta)
    for k in ("C", "K", "Cs"):
        scale = np.abs(E[k]).sum(axis=2).max()
        assert np.abs(E[k].sum(axis=2)).max() <= 1e-14 * max(scale, 1.0), k
    c0 = np.full(mesh.num_vertices, 1.75)
    c1 = T.step(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], c0, U.DT, D, 0.0, theta)
    assert np.abs(c1 - 1.75).max() <= 1e-12


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_uniform_flow_age_reaches_x_over_U(name):
    """Uniform flow (U, 0[, 0]), inlet c = 0, s = 1, D = 0, theta_c = 1: the steady state is c = x / U, to 1e-12 L / U."""
    mesh = U.MESHES[name]()
    d = mesh.x.shape[1]
    Uf = 2.0
    u = np.zeros((mesh.num_vertices, d))
    u[:, 0] = Uf
    inlet = np.unique(mesh.facet_vertices[mesh.facet_marker == U.INLET])
    c = np.zeros(mesh.num_vertices)
    dt = 0.5
    for it in range(400):
        cn = T.step(mesh.x, mesh.cells, u, u, c, dt, 0.0, 1.0, 1.0, inlet, 0.0)
        delta = np.abs(cn - c).max()
        c = cn
        if delta <= 1e-15:
            break
    err = np.abs(c - mesh.x[:, 0] / Uf).max()
    print("uniform-flow age, %s: %d steps, max error %.3e" % (name, it + 1, err))
    assert err <= 1e-12 * mesh.L / Uf


def test_numpy_bicgstab_solves_the_step():
    mesh = U.rectangle()
    fl = U.fields(mesh)
    A, b = T.assemble(mesh.x, mesh.cells, fl["u_sol"], fl["u_prev"], fl["c0"], U.DT, 2e-2, 1.0, 0.5, fl["nodes"], fl["vals"])
    x0 = fl["c0"].copy()
    x0[fl["nodes"]] = fl["vals"]
    x, its = T.bicgstab_jacobi(A, b, x0, 1e-12)
    assert 0 < its < 200 and np.linalg.norm(b - A @ x) <= 1e-12 * np.linalg.norm(b)
    assert np.array_equal((A[fl["nodes"]] != 0).sum(axis=1).A1, np.ones(len(fl["nodes"]))) and np.array_equal(b[fl["nodes"]], fl["vals"])


def test_functionals_of_known_fields():
    for name in ("rectangle", "box"):
        mesh = U.MESHES[name]()
        d = mesh.x.shape[1]
        vol = (mesh.cell_areas() if d == 2 else mesh.cell_volumes()).sum()
        c = 2.0 + 3.0 * mesh.x[:, 0]
        assert abs(T.integral(mesh.x, mesh.cells, c) - vol * (2.0 + 1.5 * mesh.L)) <= 1e-13 * vol * 10
        u = np.zeros((mesh.num_vertices, d))
        u[:, 0] = 1.0 + mesh.x[:, 1]
        area = vol / mesh.L                                   # of the outlet cross-section
        H = mesh.x[:, 1].max()
        want = (2.0 + 3.0 * mesh.L) * area * (1.0 + 0.5 * H)  # c constant on the outlet, mean of u_x there
        got = T.flux(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, U.OUTLET, u, c)
        assert abs(got - want) <= 1e-13 * abs(want)
        assert abs(T.flux(mesh.x, mesh.cells, mesh.facet_cells, mesh.facet_local, mesh.facet_marker, U.INLET, u, c) + 2.0 * area * (1.0 + 0.5 * H)) <= 1e-13 * want


def test_bolus_window_is_half_open_on_accumulated_times():
    """Scenario.solve(transport=("bolus", t0, t1)): inlet c = 1 for the steps that end in (t0, t1], with t accumulated in floating
    point as the time loop does; the Dirichlet set is re-sent only when the value changes."""
    from types import SimpleNamespace

    from cfd_hemodynamic_amd.scenario import Scenario

    class Solver:
        sent = []

        def transport_set_dirichlet(self, nodes, value):
            self.sent.append(value)

        def transport_step(self):
            return SimpleNamespace(its=3)

        def transport_functional(self, kind, marker=0):
            return 0.25

        def transport_field(self, c=None):
            return np.zeros(2)
    fake = SimpleNamespace(solver=Solver(), dt=0.1)
    tr = {"window": (0.1, 0.3), "nodes": np.array([0], dtype=np.int32), "value": 0.0, "function": None, "integral": [], "times": [], "its": []}
    t, values = 0.0, []
    for _ in range(5):
        t += 0.1                      # 0.1, 0.2, 0.30000000000000004, 0.4, 0.5
        Scenario._transport_step(fake, tr, t, False)
        values.append(tr["value"])
    assert values == [0.0, 1.0, 1.0, 0.0, 0.0] and Solver.sent == [1.0, 0.0]
    assert tr["integral"] == [0.25] * 5 and tr["its"] == [3] * 5 and len(tr["times"]) == 5
    for bad in ("dye", ("bolus", 0.1), ("age", 1.0)):
        with pytest.raises(ValueError):
            Scenario._transport_setup(fake, bad, 0.0)
    assert Scenario._transport_setup(fake, None, 0.0) is None


# ---------------------------------------------------------------------------- the host work-list builder under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scalar_host_san") / "scalar_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "scalar_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_builder_under_sanitizers(sanitized, tmp_path, name):
    mesh = U.MESHES[name]()
    vptr, vcol = U.graph(mesh)
    rng = np.random.default_rng(0)
    for k in range(mesh.num_vertices):  # the builder must not rely on ascending columns
        vcol[vptr[k]:vptr[k + 1]] = rng.permutation(vcol[vptr[k]:vptr[k + 1]])
    path = str(tmp_path / "list.bin")
    with open(path, "wb") as f:
        f.write(np.array([mesh.x.shape[1], mesh.num_vertices, len(mesh.cells), len(vcol)], np.int32).tobytes())
        for a in (mesh.cells, vptr, vcol):
            f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    valence = np.bincount(mesh.cells.ravel(), minlength=mesh.num_vertices)
    nsl = (mesh.num_vertices + 63) // 64
    widest = max(valence[64 * s: 64 * s + 64].max() for s in range(nsl))
    assert r.stdout.split()[1:] == [str(mesh.num_vertices), str(mesh.cells.size), str(nsl), str(widest)]
    assert nsl == 2 and mesh.num_vertices % 64 != 0  # a full and a partial slice
