"""Every scalar the host reads from the device goes through csrc/cfdh_reduce.hip: partials, a final kernel into a named word of
red_out, the reduction over the ranks, a read through a handle ("Scalar reductions and read-backs").  These tests
look at what that layer must guarantee beyond the value of one call: a result does not depend on which read-backs ran before
it (no stale host-mapped word, no two users of one word), a read costs one counted synchronisation, and the words of the solver
(mean, lean residual norm) survive the plain reductions in between.

The smallest meshes that reach every branch of k_functional: closed-form triangles (kinds 0 .. 7) and tetrahedra, Q1 hexahedra
and P2 tetrahedra through the generic kernels (kinds 2 .. 7).  States are small dyadic numbers: every comparison is bitwise.
"""
import numpy as np
import pytest

import krylov_vec_ref as R
from cfd_hemodynamic_amd import _lib as L
from cfd_hemodynamic_amd.elements import NodeMesh3D, create_box
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube

pytestmark = pytest.mark.gpu

OUTLET = 7  # marker of the facets on the plane x = max


def _mesh(family):
    if family == "tri":
        return create_unit_square(4), 0        # 32 triangles
    if family == "tet":
        return create_unit_cube(2), 0          # 48 tetrahedra, 27 vertices
    if family == "hex":
        return create_box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 2, 2)), 2
    return NodeMesh3D(create_unit_cube(2)), 1  # P2 tetrahedra


FAMILIES = ["tri", "tet", "hex", "p2tet"]


def kinds_of(family):
    return list(range(8)) if family == "tri" else list(range(2, 8))  # drag and lift exist on closed-form triangles only


def make(family):
    m, etype = _mesh(family)
    x = np.asarray(m.x)
    d = x.shape[1]
    nv = len(x)
    fx = x[np.asarray(m.facet_vertices)][:, :, 0]
    marker = np.where(fx.min(axis=1) == x[:, 0].max(), OUTLET, 0).astype(np.int32)
    assert marker.any()
    ctx = L.Context(x, m.cells, m.facet_cells, m.facet_local, marker, etype=etype)
    ctx.set_params(0.0625, 1.0, 0.03125)
    i = np.arange(nv)
    u = np.stack([((5 * i + 3 * a) % 7 + (1 if a == 0 else -3)) / 8.0 for a in range(d)], axis=1)  # u_x > 0: flux through OUTLET
    un = np.stack([((3 * i + a) % 13 - 6) / 4.0 for a in range(d)], axis=1)
    ctx.set_state(u_prev=un.ravel(), p_prev=np.zeros(nv), u=u.ravel(), p=((7 * i) % 11 - 5) / 16.0)
    return ctx


def call(ctx, kind):
    return ctx.functional(kind, OUTLET if kind in (0, 1, 7) else 0)


def bits(v):
    return np.float64(v).tobytes()


@pytest.fixture(scope="module")
def fresh_values():
    """kind -> value on a context that has read nothing else back, per family"""
    out = {}
    for family in FAMILIES:
        out[family] = {}
        for kind in kinds_of(family):
            ctx = make(family)
            out[family][kind] = call(ctx, kind)
            ctx.close()
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_functionals_do_not_depend_on_the_calls_before_them(fresh_values, family):
    want = fresh_values[family]
    kinds = kinds_of(family)
    print(family, {k: want[k] for k in kinds})
    assert want[7] != 0.0                                            # a flux to get wrong
    assert len({want[4], want[5], want[6]}) == 3                     # the previous state differs from the current one
    assert want[2] > 0.0 and want[3] > 0.0
    ctx = make(family)
    for order in (kinds, kinds[::-1]):
        for k in order:
            assert bits(call(ctx, k)) == bits(want[k]), (order, k)
    for k in kinds:
        for other in kinds:
            if other != k:
                call(ctx, other)
                assert bits(call(ctx, k)) == bits(want[k]), (other, k)
    ctx.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_functional_costs_one_counted_synchronisation(family):
    ctx = make(family)
    for k in kinds_of(family):
        before = ctx.info(15)
        call(ctx, k)
        assert ctx.info(15) - before == 1, k
    ctx.close()


def test_solver_slots_survive_interleaved_reductions():
    """v_sub_mean (mean word), v_guess_combine + v_scale_inv_lean (lean word, host-mapped words of the prologue) and v_dot (result
    word 0, mirrored) one after the other in both orders: each equals its exact reference of krylov_vec_ref.py"""
    ctx = make("tri")
    n, k = 1027, 3
    ld = R.ld_of(n)
    rng = np.random.default_rng(11)
    x, y, z = R.exact_vector(rng, n), R.exact_vector(rng, n), R.exact_vector(rng, n)
    hd, yc = R.diagonal_gram(rng, k)
    Um, Wm = R.exact_block(rng, n, ld, k), R.exact_block(rng, n, ld, k)
    t, nrm = R.pow4_vector(rng, n)
    b = t + R.combine(Wm, yc, np.zeros(n, dtype=np.int64), 1)  # r = b - W y = t
    xg, r, s2 = R.guess(Um, Wm, yc, b)
    want_mean, S = R.sub_mean_exact(z)
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    same = lambda a, b: np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()

    def sub_mean():
        o = ctx.krylov_vec_op(L.KVOP_SUB_MEAN, n, ld, x=z)
        assert same(o["dev"], f64([S])) and same(o["out1"], want_mean)

    def guess_lean():
        o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, k, A=Um, B=Wm, coef=hd, x=b, flags=1)
        assert same(o["host"], f64([nrm, 1.0, k] + list(yc)))
        assert same(o["mirror"], f64([nrm * nrm, 1.0, k] + list(yc)))
        assert same(o["dev"], f64([nrm * nrm] + list(yc)))
        assert same(o["out1"], f64(xg)) and same(o["out2"], R.scaled(r, nrm))

    def dot():
        o = ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=x, y=y)
        assert same(o["host"], f64([R.dot(x, y)])) and same(o["dev"], o["host"]) and same(o["mirror"], o["host"])

    ops = [sub_mean, guess_lean, dot]
    for order in (ops, ops[::-1], ops):
        for op in order:
            op()
    ctx.close()
