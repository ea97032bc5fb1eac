"""tests/post_twin.py against the twins that already exist (1e-13 relative, the level at which the project compares its twins with each
other) and against closed forms that need no other code."""
import math

import numpy as np
import pytest

import wss_p2_twin
from gen3_util import node_mesh3, problem3
from gen_util import node_mesh, problem
from oracle import np_twin as T, np_twin_nd as TN
from post_twin import PostTwin, couette_case, deposit_weights, family


TOL = 1e-13
MU = 0.7


def _mesh(d, kind, n=None):
    return node_mesh(kind, n or 5, distort=0.05) if d == 2 else node_mesh3(kind, n or 2, distort=0.05)


def _state(m, seed=11):
    rng = np.random.default_rng(seed)
    nn, d = m.x.shape
    return rng.standard_normal((nn, d)), rng.standard_normal(nn)


def _twin(m):
    return PostTwin(m.x, m.cells, m.facet_cells, m.facet_local)


@pytest.mark.parametrize("d,nloc", [(2, 3), (2, 6), (2, 4), (3, 4), (3, 10), (3, 8)])
def test_bases_are_nodal_and_facet_nodes_are_the_librarys(d, nloc):
    F = family(d, nloc)
    phi, dphi = F.tabulate(F.nodes)
    assert np.array_equal(phi, np.eye(nloc))
    assert np.abs(dphi.sum(axis=1)).max() <= 1e-15          # partition of unity
    assert abs(F.cell_w.sum() - 1.0) <= 1e-15 and abs(F.facet_w.sum() - 1.0) <= 1e-15
    # the facet nodes found by coordinates are the facet_vertices of the project's node meshes
    kind = {3: "P1", 6: "P2", 4: "Q1" if d == 2 else "P1", 10: "P2", 8: "Q1"}[nloc]
    m = _mesh(d, kind)
    for k in range(m.num_facets):
        mine = sorted(np.asarray(m.cells)[m.facet_cells[k], list(F.facet_nodes[m.facet_local[k]])])
        assert mine == sorted(np.asarray(m.facet_vertices)[k].tolist())
    tw = _twin(m)
    assert np.array_equal(np.nonzero(tw.wall_nodes())[0], np.unique(m.facet_vertices))


def test_p1_triangles_against_np_twin_and_np_twin_nd():
    m = _mesh(2, "P1")
    u, p = _state(m)
    xv = np.concatenate([u.ravel(), p])
    tw = _twin(m)
    sel = np.arange(0, m.num_facets, 2)
    pb = T.Problem(m.x, m.cells, m.facet_cells, m.facet_local, T.Params(0.01, 1.0, MU, (0.0, 0.0)))
    fd, fl = pb.drag_lift(xv, sel, MU)
    (d_, l_) = tw.drag_lift(u, p, sel, MU)
    assert abs(d_.value - fd) <= TOL * d_.abs and abs(l_.value - fl) <= TOL * l_.abs
    nu_, np_ = pb.l2_norms(xv)
    a, b = tw.l2_norms(u, p)
    assert abs(a.value - nu_) <= TOL * nu_ and abs(b.value - np_) <= TOL * np_
    assert a.value == math.sqrt(a.abs) and b.value == math.sqrt(b.abs)


@pytest.mark.parametrize("d", [2, 3])
def test_p1_against_np_twin_nd(d):
    m = _mesh(d, "P1")
    u, p = _state(m)
    xv = np.concatenate([u.ravel(), p])
    tw = _twin(m)
    pb = TN.Problem(m.x, m.cells, m.facet_cells, m.facet_local, TN.Params(0.01, 1.0, MU, (0.0,) * d))
    w = pb.wall_shear_stress(xv, MU).reshape(-1, d)
    mine = tw.wall_shear_stress(u, MU)
    assert np.abs(mine - w).max() <= TOL * np.abs(w).max() > 0
    assert np.array_equal(tw.wall_shear_stress(u, MU, test="p1"), mine)
    assert not mine[~tw.wall_nodes()].any() and (~tw.wall_nodes()).any()
    sel = np.arange(1, m.num_facets, 3)
    q = tw.flux(u, sel)
    assert abs(q.value - pb.flux(xv, sel)) <= TOL * q.abs
    nu_, np_ = pb.l2_norms(xv)
    a, b = tw.l2_norms(u, p)
    assert abs(a.value - nu_) <= TOL * nu_ and abs(b.value - np_) <= TOL * np_


@pytest.mark.parametrize("d,kind", [(2, "P1"), (2, "P2"), (2, "Q1"), (3, "P1"), (3, "P2"), (3, "Q1")])
def test_l2_and_flux_against_the_generic_twins(d, kind):
    m = _mesh(d, kind)
    u, p = _state(m)
    xv = np.concatenate([u.ravel(), p])
    prm = T.Params(0.01, 1.0, MU, (0.0, 0.0)) if d == 2 else TN.Params(0.01, 1.0, MU, (0.0, 0.0, 0.0))
    pb = (problem if d == 2 else problem3)(kind, m, prm)
    tw = _twin(m)
    nu_, np_ = pb.l2_norms(xv)
    a, b = tw.l2_norms(u, p)
    assert abs(a.value - nu_) <= TOL * nu_ and abs(b.value - np_) <= TOL * np_
    for sel in (np.arange(m.num_facets), np.arange(0, m.num_facets, 3)):
        q = tw.flux(u, sel)
        assert abs(q.value - pb.flux(xv, sel)) <= TOL * q.abs


@pytest.mark.parametrize("d", [2, 3])
def test_p1_test_space_on_p2_cells_against_wss_p2_twin(d):
    m = _mesh(d, "P2")
    u, _ = _state(m)
    nvert = m.num_base_vertices
    ref = wss_p2_twin.wall_shear_stress(m.x, m.cells, nvert, m.facet_cells, m.facet_local, u, MU)
    mine = _twin(m).wall_shear_stress(u, MU, test="p1")
    assert not mine[nvert:].any()
    assert np.abs(mine[:nvert] - ref).max() <= TOL * np.abs(ref).max() > 0
    own = _twin(m).wall_shear_stress(u, MU)
    assert np.abs(own[nvert:]).max() > 0          # the P2 test space deposits on the edge nodes as well


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("d,kind", [(2, "P1"), (2, "P2"), (2, "Q1"), (3, "P1"), (3, "P2"), (3, "Q1")])
def test_flux_of_the_position_field_is_d_times_the_volume(d, kind):
    m = _mesh(d, kind)
    tw = _twin(m)
    vol = tw.l2_norms(np.zeros_like(m.x), np.ones(len(m.x)))[1].abs        # int 1^2
    exact = {(2, "Q1"): 0.8, (3, "Q1"): 0.48}.get((d, kind), 1.0)          # the shear keeps the volume
    assert abs(vol - exact) <= 1e-14
    q = tw.flux(m.x)
    assert abs(q.value - d * vol) <= TOL * q.abs


@pytest.mark.parametrize("d,kind", [(2, "P1"), (2, "P2"), (2, "Q1"), (3, "P2"), (3, "Q1")])
def test_couette_flow(d, kind):
    gamma = 1.7
    m, u, H, L = couette_case(d, kind, 3 if d == 2 else 2)
    tw = _twin(m)
    w = tw.wall_shear_stress(u, MU)
    mid = m.facet_midpoints()
    for y, sign in ((0.0, 1.0), (H, -1.0)):          # T = -mu (grad u + grad u^T) n: +mu gamma e_x on the lower plate, - on the upper
        plate = np.nonzero(np.isclose(mid[:, 1], y))[0]
        # summed over a plate's nodes the field is (number of plate facets) * Tt: the test functions sum to one on each facet
        nodes = np.unique(np.asarray(m.facet_vertices)[plate])
        side = np.nonzero(~np.isclose(mid[:, 1], 0.0) & ~np.isclose(mid[:, 1], H))[0]
        inner = np.setdiff1d(nodes, np.unique(np.asarray(m.facet_vertices)[side]))
        tot = w[inner].sum(axis=0)
        # side walls are parallel to the flow (x-normal walls carry shear too): only nodes off the side walls are summed, so count by weight
        wsum = sum(deposit_weights(tw, plate, inner))
        assert abs(tot[0] - sign * MU * gamma * wsum) <= 1e-12 * MU * gamma * wsum and np.abs(tot[1:]).max() <= 1e-13 * MU * gamma * wsum
        if d == 2:
            fd, fl = tw.drag_lift(u, np.zeros(len(m.x)), plate, MU)
            # n = -FacetNormal, t = (n_y, -n_x), u_t = t . u: d_n u_t = gamma on both plates, n_y = +1 on the lower and -1 on the upper one,
            # so F_D = int mu d_n u_t n_y ds = +- mu gamma L; no lift from the viscous part (n_x = 0)
            assert abs(fd.value - sign * MU * gamma * L) <= 1e-12 * fd.abs and abs(fl.value) <= 1e-13 * fd.abs


@pytest.mark.parametrize("d,kind", [(2, "P1"), (2, "P2"), (2, "Q1"), (3, "P1"), (3, "P2"), (3, "Q1")])
def test_rigid_rotation_has_no_wall_shear_stress(d, kind):
    m = _mesh(d, kind)
    u = np.zeros_like(m.x)
    u[:, 0], u[:, 1] = -m.x[:, 1], m.x[:, 0]
    w = _twin(m).wall_shear_stress(u, MU)
    assert np.abs(w).max() <= 1e-13


@pytest.mark.parametrize("d", [2, 3])
def test_a_quadratic_velocity_on_p2_is_integrated_exactly(d):
    m = _mesh(d, "P2", 3 if d == 2 else 1)
    x = m.x
    u = np.zeros_like(x)
    u[:, 0] = x[:, 1] ** 2
    tw = _twin(m)
    # ||u||^2 = int y^4 over the sheared unit square / cube: the shear x += g(y or z) keeps y (and z), so it is 1/5
    nu_, _ = tw.l2_norms(u, np.zeros(len(x)))
    assert abs(nu_.abs - 0.2) <= 1e-14
    # flux of (y^2, 0): its divergence is zero
    q = tw.flux(u)
    assert abs(q.value) <= TOL * q.abs and q.abs > 0.1
    # unsheared mesh, plate y = 1: T = -mu (grad u + grad u^T) n = (-2 mu y, 0) = (-2 mu, 0), deposited with weights that sum to one per facet
    m2, _, H, L = couette_case(d, "P2", 2)
    u2 = np.zeros_like(m2.x)
    u2[:, 0] = m2.x[:, 1] ** 2
    w = _twin(m2).wall_shear_stress(u2, 1.0)
    top = np.nonzero(np.isclose(m2.facet_midpoints()[:, 1], 1.0))[0]
    side = np.nonzero(~np.isclose(m2.facet_midpoints()[:, 1], 1.0))[0]
    inner = np.setdiff1d(np.unique(np.asarray(m2.facet_vertices)[top]), np.unique(np.asarray(m2.facet_vertices)[side]))
    wsum = sum(deposit_weights(_twin(m2), top, inner))
    assert len(inner) > 0 and abs(w[inner, 0].sum() + 2.0 * wsum) <= 1e-13 * 2.0 * wsum and np.abs(w[inner, 1:]).max() <= 1e-14
    assert math.isfinite(wsum)
