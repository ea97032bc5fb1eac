"""CPU tests of the twin of `ipcs_midpoint` (tests/ipcs_mid_twin.py): the discrete momentum equation against the weak form F1
evaluated pointwise as the reference writes it, the structure of the viscous operator, the Poiseuille fixed point of a whole step
(which the ds pair makes, and its absence breaks), and the plugin's host-side refusals."""
import functools

import numpy as np
import pytest

import ipcs_mid_twin as MT
import ipcs_twin as T
from util import dfg_case

from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D, create_box, create_rectangle
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_bifurcation, create_unit_cube


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(mesh, P2 node mesh, operators, midpoint operators), built once and left unchanged"""
    if name == "dfg":
        m = dfg_case(6).mesh
        nm = NodeMesh(m)
    else:
        m, _ = create_bifurcation(1.2e-3)
        nm = NodeMesh3D(m)
    op = T.Operators(nm.x, nm.cells, m.num_vertices)
    return m, nm, op, MT.MidOperators(op, nm.facet_cells, nm.facet_local)


def _weak_form_F1(tw, u, up, p, v):
    """F1(u; v) of the reference's src/solvers/ipcs_midpoint.py:60-67 with eps = sym(nabla_grad), sigma = 2 mu eps - p I
    (solverBase.py:176-182), nabla_grad(u)[i, j] = d_i u_j: tensors at the quadrature points, cells with the volume rule, exterior
    facets with their own.  Returns (value, sum of the absolute contributions)."""
    op, mo = tw.op, tw.mo
    rho, mu, dt = tw.rho, tw.mu, tw.dt
    val = lambda phi, f, cells: np.einsum("qa,cad->cqd", phi, f[cells])
    grad = lambda gphi, f, cells: np.einsum("cqai,caj->cqij", gphi, f[cells])      # [c, q, i, j] = d_i f_j
    sym = lambda G: 0.5 * (G + np.swapaxes(G, 2, 3))
    c2, c1 = op.c2, op.c1
    W = op.w[None, :] * op.adet[:, None]
    uq, upq, vq = val(op.phi, u, c2), val(op.phi, up, c2), val(op.phi, v, c2)
    Gup, Gv = grad(op.gphi, up, c2), grad(op.gphi, v, c2)
    Gum = grad(op.gphi, 0.5 * (u + up), c2)
    pq = np.einsum("qa,ca->cq", op.lam, p[c1])
    sigma = 2 * mu * sym(Gum) - pq[:, :, None, None] * np.eye(op.dim)[None, None]
    terms = [
        rho * np.einsum("cqd,cqd->cq", (uq - upq) / dt, vq),
        rho * np.einsum("cqi,cqij,cqj->cq", upq, Gup, vq, optimize=True),                          # dot(dot(u_prev, nabla_grad(u_prev)), v)
        np.einsum("cqij,cqij->cq", sigma, sym(Gv)),
        -tw.sf * np.einsum("d,cqd->cq", tw.f, vq),
    ]
    tot = sum(float((W * t).sum()) for t in terms)
    mag = sum(float(np.abs(W * t).sum()) for t in terms)
    for sel, lam, fw, phi, gphi, n, meas in mo.facets:
        Wf = fw[None, :] * meas[:, None]
        vf = val(phi, v, c2[sel])
        Gf = grad(gphi, 0.5 * (u + up), c2[sel])
        pf = np.einsum("qa,ca->cq", lam, p[c1[sel]])
        t5 = pf * np.einsum("cd,cqd->cq", n, vf)                                     # dot(p_prev n, v)
        t6 = -mu * np.einsum("cqij,cj,cqi->cq", Gf, n, vf, optimize=True)                           # -dot(mu nabla_grad(u_mid) n, v)
        for t in (t5, t6):
            tot += float((Wf * t).sum())
            mag += float(np.abs(Wf * t).sum())
    return tot, mag


@pytest.mark.parametrize("name", ["dfg", "bifurcation"])
@pytest.mark.parametrize("consistent", [True, False])
def test_discrete_momentum_equation_is_the_weak_form_of_the_reference(name, consistent):
    m, nm, op, mo = _mesh(name)
    d, nn, nv = m.x.shape[1], nm.num_vertices, m.num_vertices
    rng = np.random.default_rng(3)
    tw = MT.MidTwin(nm.x, nm.cells, nv, nm.facet_cells, nm.facet_local, 0.013, 1.06, 3.5e-3, f=(0.3, -0.7, 0.2)[:d], consistent=consistent,
                    ops=op, mops=mo)
    u, up, p = rng.standard_normal((nn, d)), rng.standard_normal((nn, d)), rng.standard_normal(nv)
    tw.u_prev, tw.p_prev = up.copy(), p.copy()
    _, b1, Af = tw.assemble1()
    res = (Af @ u.ravel()).reshape(nn, d) - b1
    worst = 0.0
    for _ in range(2):
        v = rng.standard_normal((nn, d))
        F, mag = _weak_form_F1(tw, u, up, p, v)
        worst = max(worst, abs(float((res * v).sum()) - F) / mag)
    print("ipcs_midpoint twin vs weak form, %s consistent=%s: %.2e of the absolute contributions" % (name, consistent, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("name", ["dfg", "bifurcation"])
def test_viscous_operator_structure(name):
    m, nm, op, mo = _mesh(name)
    d, nn, nv = m.x.shape[1], nm.num_vertices, m.num_vertices
    mu = 0.035
    tw = MT.MidTwin(nm.x, nm.cells, nv, nm.facet_cells, nm.facet_local, 0.01, 1.0, mu, ops=op, mops=mo)
    KE = (mo.KI + mo.E).tocsr()
    scale = abs(KE) @ np.ones(d * nn)
    x = nm.x
    rots = [(0, 1)] if d == 2 else [(0, 1), (0, 2), (1, 2)]
    for i, j in rots:       # rigid rotation in the (i, j) plane: eps = 0
        r = np.zeros((nn, d))
        r[:, i], r[:, j] = -x[:, j], x[:, i]
        assert np.abs(KE @ r.ravel()).max() <= 1e-12 * scale.max() * np.abs(x).max()
    assert abs(mo.E - mo.E.T).max() <= 1e-13 * abs(mo.E).max()
    V = tw.V()
    D = (V - V.T) + mu * (mo.S - mo.S.T)
    assert abs(D).max() <= 1e-13 * abs(V).max()
    assert abs(mo.S - mo.S.T).max() > 1e-3 * abs(mo.S).max()   # S is not symmetric


def _poiseuille(dim, ds):
    """Exact steady state u = (4 s (1 - s), 0[, 0]), p = 8 mu (1 - x) with s = y (2-D) or z (3-D); returns the relative errors of
    u_sol and p after one step with direct solves from the exact state."""
    mu, rho, dt = 0.035, 1.06, 0.02
    if dim == 2:
        m = create_unit_square(4, 4)
        nm = NodeMesh(m)
    else:
        m = create_unit_cube(2)
        nm = NodeMesh3D(m)
    x, s_ax = nm.x, dim - 1
    u = np.zeros((len(x), dim))
    u[:, 0] = 4 * x[:, s_ax] * (1 - x[:, s_ax])
    p = 8 * mu * (1 - m.x[:, 0])
    fx = x[nm.facet_vertices]
    on = lambda ax, v: np.isclose(fx[:, :, ax], v).all(axis=1)
    dir_f = on(0, 0.0) | on(s_ax, 0.0) | on(s_ax, 1.0)
    nodes = np.unique(nm.facet_vertices[dir_f].ravel())
    v_out = np.nonzero(np.isclose(m.x[:, 0], 1.0))[0]
    tw = MT.MidTwin(nm.x, nm.cells, m.num_vertices, nm.facet_cells, nm.facet_local, dt, rho, mu, bcu=[(nodes, u[nodes])],
                    bcp=[(v_out, np.zeros(len(v_out)))], ds=ds)
    tw.u_prev, tw.p_prev = u.copy(), p.copy()
    tw.step()
    return np.abs(tw.u_sol - u).max() / np.abs(u).max(), np.abs(tw.p - p).max() / np.abs(p).max()


@pytest.mark.parametrize("dim", [2, 3])
def test_poiseuille_is_a_fixed_point_of_a_whole_step_because_of_the_ds_pair(dim):
    eu, ep = _poiseuille(dim, True)
    eu0, ep0 = _poiseuille(dim, False)
    print("ipcs_midpoint Poiseuille fixed point, gdim %d: |u_sol - u| %.2e, |p_sol - p| %.2e; without S, Pn %.2e, %.2e" % (dim, eu, ep, eu0, ep0))
    assert eu <= 1e-11 and ep <= 1e-11
    # without the ds pair the outlet rows keep sigma n: the same test misses its bound by orders of magnitude
    assert max(eu0, ep0) >= 1e-11 * 1e4


def test_plugin_refusals_come_before_any_device_work(monkeypatch):
    from cfd_hemodynamic_amd import _lib
    from cfd_hemodynamic_amd.solvers import ipcs_midpoint

    def boom(*a, **k):
        raise AssertionError("device work before the refusal")

    monkeypatch.setattr(_lib, "IpcsContext", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    with pytest.raises(NotImplementedError, match="ipcs_midpoint.*quadrilateral"):
        ipcs_midpoint.Solver(create_rectangle((0, 0), (1, 1), (2, 2)), 0.1, 1.0, 1.0, [0, 0])
    with pytest.raises(NotImplementedError, match="ipcs_midpoint.*hexahedron"):
        ipcs_midpoint.Solver(create_box((0, 0, 0), (1, 1, 1), (2, 2, 2)), 0.1, 1.0, 1.0, [0, 0, 0])

    class Comm:
        size = 2

    with pytest.raises(NotImplementedError, match="ipcs_midpoint runs on one GPU"):
        ipcs_midpoint.Solver(create_unit_square(2, 2), 0.1, 1.0, 1.0, [0, 0], comm=Comm())
