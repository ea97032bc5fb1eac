"""The three Krylov drivers of the pressure-correction step (csrc/cfdh_ipcs_krylov.hip: ip_bicgstab, ip_cg<1, false>, ip_cg<D, true>),
iterate by iterate, through cfdh_ipcs_krylov_solve: the device's x_k and recurrence scalars after k = 1 .. 10 iterations against
the extended-precision recurrences of tests/ipcs_krylov_ref.py on the device's own matrices (get_operator), the reported
residual against the residual of the returned vector, convergence in the middle of a batch of launches, the edges of
ip_finish, and the second trip of the row loop.  DESIGN.md section 9, "The pressure-correction Krylov drivers, iterate by
iterate".

Not covered here, on purpose: the second trip of the row loop in the 3-D instantiation (it differs in the inner `d` loop only) and
in the pressure instantiation (it would need 66 049 vertices); the cap of the vector kernels' grid (more than 2 097 152 entries);
proof that a restart happened in the rtol = 1e-16 solves."""
import numpy as np
import pytest

import ipcs_krylov_ref as R
import ipcs_twin as T
from test_gpu_ipcs import _case, _ctx, _cube_markers

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd._lib import IP_ALPHA, IP_BAD, IP_BETA, IP_BN2, IP_DONE, IP_ITS, IP_OMEGA, IP_RHO, IP_RN2, IP_RZ, IP_TOL2
from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube

pytestmark = pytest.mark.gpu

CONVERGED, DIVERGED_ITS = 2, -3
NAMES = ("bicgstab", "fpcg", "cg")
SCAL_INDEX = dict(alpha=IP_ALPHA, omega=IP_OMEGA, beta=IP_BETA, rho=IP_RHO, rz=IP_RZ)
# smallest meshes of the list 16, 24, 32, ... whose pressure hierarchy has two levels (the set-up stops coarsening at 1000
# unknowns: 33^2 = 1089 and 17^3 = 4913 vertices); asserted where they are used
FPCG_MESH = {2: "sq32", 3: "cube16"}


def setup(name):
    """(m, nm, mk, par, bcu, bcp, u0).  sq8 / cube4: _case(2) / _case(3) of test_gpu_ipcs.py.  sqN: N x N unit square, no Dirichlet
    object (singular pressure problem), a Taylor-Green field as state; cubeN: N^3 unit cube, p = 0 on the outlet, from rest."""
    if name == "sq8":
        return _case(2)
    if name == "cube4":
        return _case(3)
    if name.startswith("sq"):
        n = int(name[2:])
        m = create_unit_square(n, n)
        nm = NodeMesh(m)
        k, x = 2 * np.pi, nm.x
        u0 = np.stack([-np.cos(k * x[:, 0]) * np.sin(k * x[:, 1]), np.sin(k * x[:, 0]) * np.cos(k * x[:, 1])], 1)
        return m, nm, np.zeros(len(nm.facet_cells), np.int32), dict(dt=0.02, rho=1.0, mu=1.0 / 50.0), [], [], u0
    n = int(name[4:])
    m = create_unit_cube(n)
    nm, mk = NodeMesh3D(m), _cube_markers(m)
    v_out = np.unique(m.facet_vertices[mk == 3].ravel()).astype(np.int32)
    return m, nm, mk, dict(dt=0.05, rho=1.0, mu=0.1), [], [(v_out, np.zeros(len(v_out)))], np.zeros((len(nm.x), 3))


def twin_matrices(name):
    """{0: A1, 1: L, 2: rho M} of the case from the NumPy twin (the CPU side of the spread table)."""
    m, nm, mk, par, bcu, bcp, u0 = setup(name)
    tw = T.Twin(nm.x, nm.cells, m.num_vertices, bcu=bcu, bcp=bcp, **par)
    tw.u_prev, tw.u_n1 = u0.copy(), u0.copy()
    return {0: tw.assemble1()[0], 1: tw.Lbc, 2: tw.rhoM}


SEEDS = {"sq8": 11, "cube4": 12, "sq1": 13, "sq32": 14, "cube16": 15, "sq128": 16}


def data(which, name, shape, singular=False, extra=0):
    """b and x0: standard normal draws with a fixed seed per (driver, case); a mean-free b on a singular pressure problem."""
    rng = np.random.default_rng(1000 * extra + 10 * SEEDS[name] + which)
    b, x0 = rng.standard_normal(shape), rng.standard_normal(shape)
    if which == 1 and singular:
        b -= b.mean()
    return b, x0


# Rounding spread of the float64 recurrence against the extended-precision one, (iterates, scalars), largest over k = 1 .. KMAX of the
# case: ipcs_krylov_ref.spread on the twin's matrices with the data above (tests/test_ipcs_krylov_ref.py asserts that the rows of
# drivers 0 and 2 are still what the reference gives, within a factor 2).  The rows of driver 1 cannot be measured without the
# device's V-cycle: they come from measure_fpcg_spreads() below, run on an MI355X.  The device is held to FACTOR x these.
KMAX = {"sq8": 10, "cube4": 10, "sq1": 3, "sq32": 10, "cube16": 10, "sq128": 3}
SPREAD = {
    (0, "sq8"): (4.1e-16, 4.5e-13), (2, "sq8"): (2.3e-16, 1.0e-15), (0, "cube4"): (3.6e-16, 4.2e-14), (2, "cube4"): (3.1e-16, 1.6e-15),
    (0, "sq1"): (5.2e-16, 3.3e-15), (2, "sq1"): (3.4e-16, 9.4e-16), (0, "sq128"): (3.0e-16, 1.8e-15), (2, "sq128"): (4.6e-16, 7.0e-16),
    (1, "sq32"): (8.2e-16, 6.2e-15), (1, "cube16"): (7.5e-15, 1.6e-14),
}
FACTOR = 50.0
SPREAD_CAP = 1e-12   # above this something other than rounding would be in a spread


def targets(tr):
    """Convergence targets (k*, tolerance) of a reference trajectory: k* in {1, 2, 3, 5, 6, 7} and the multiples of 4 (one is kept by
    the caller) at which |r_k*| is below every earlier |r_j| by a factor of at least 4; the tolerance is the geometric mean of |r_k*|
    and min_{j < k*} |r_j|, two binary orders of magnitude of room for the decision."""
    rn = [float(np.sqrt(s["rn2"])) for s in tr]
    out, have4 = [], False
    for k in (1, 2, 3, 4, 5, 6, 7, 8):
        if k >= len(rn):
            break
        lo = min(rn[:k])
        if not (rn[k] > 0 and 4.0 * rn[k] <= lo) or (k % 4 == 0 and have4):
            continue
        have4 |= k % 4 == 0
        out.append((k, float(np.sqrt(rn[k] * lo))))
    return out


# ---- contexts ----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name):
        self.name = name
        m, nm, mk, par, bcu, bcp, u0 = setup(name)
        self.dim, self.nn, self.nvert, self.singular = nm.x.shape[1], len(nm.x), m.num_vertices, not bcp
        self._make = lambda: self._new(m, nm, mk, par, bcu, bcp, u0)
        self.ctx = self._make()
        self.A = {}

    def _new(self, m, nm, mk, par, bcu, bcp, u0):
        ctx = _ctx(m, nm, mk, par["dt"], par["rho"], par["mu"], np.zeros(self.dim), bcu, bcp)
        z = np.zeros(m.num_vertices)
        ctx.set_state(u_prev=u0.ravel(), p_prev=z, u=u0.ravel(), p=z)
        ctx.set_previous2(u0.ravel())
        return ctx

    def fresh(self):
        return self._make()

    def mat(self, which):
        if which not in self.A:
            self.A[which] = self.ctx.get_operator(which)
        return self.A[which]

    def levels(self):
        self.mat(1)   # the hierarchy is built with the operators
        return self.ctx.info(6)

    def shape(self, which):
        return (self.nvert,) if which == 1 else (self.nn, self.dim)

    def data(self, which, extra=0):
        return data(which, self.name, self.shape(which), self.singular, extra)

    def pre(self, which):
        return self.ctx.apply_pressure_pc if which == 1 else None

    def reference(self, which, b, x0, nit, dtype=R.LD):
        return R.DRIVERS[which](self.mat(which), b, x0, nit, pre=self.pre(which), dtype=dtype)

    def solve(self, which, b, x0, rtol, atol, max_it, ctx=None):
        """The hook, and -- for every call of this file -- the reported residual against the residual of the returned vector:
        | rel_res |b| - |b - A x| | <= (nnz_row_max + 3) u | |A| |x| + |b| |_2; a converged solve is within its tolerance."""
        x, its, reason, rel_res, S = (ctx or self.ctx).krylov_solve(which, b, x0, rtol, atol, max_it)
        x = x.reshape(self.shape(which))
        bn = float(np.sqrt(np.sum(np.asarray(b, dtype=R.LD) ** 2)))
        true, bound = R.residual_check(self.mat(which), b, x)
        reported = rel_res * bn if bn > 0 else rel_res
        print("  %s %s: max_it %d rtol %.2e -> its %d reason %d; reported |r| %.6e, recomputed %.6e, gap / bound %.3f"
              % (NAMES[which], self.name, max_it, rtol, its, reason, reported, true, abs(reported - true) / max(bound, 1e-300)))
        assert np.isfinite(rel_res) and abs(reported - true) <= bound, (reported, true, bound)
        assert abs(np.sqrt(S[IP_RN2]) - true) <= bound and S[IP_ITS] == its
        if reason == CONVERGED:
            assert true <= max(rtol * bn, atol) + bound, (true, rtol * bn, atol)
            assert S[IP_DONE] == 1.0 and S[IP_BAD] == 0.0
        return x, its, reason, rel_res, S


_cases = {}


@pytest.fixture(scope="module")
def case():
    def get(name):
        if name not in _cases:
            _cases[name] = Case(name)
        return _cases[name]
    yield get
    for c in _cases.values():
        c.ctx.close()
    _cases.clear()


def measure_fpcg_spreads():
    """The rows of driver 1 in SPREAD: float64 against extended precision, both with the device's V-cycle as `pre`."""
    out = {}
    for dim, name in FPCG_MESH.items():
        c = Case(name)
        b, x0 = c.data(1)
        out[(1, name)] = R.spread(1, c.mat(1), b, x0, KMAX[name], pre=c.pre(1))
        c.ctx.close()
    return out


# ---- trajectories ------------------------------------------------------------------------------------------------------------
def _trajectory(c, which, kmax, bound):
    """k = 1 .. kmax capped solves against the reference: x_k, the scalars as the device holds them after iteration k (alpha_k,
    omega_k; beta: BiCGStab and CG the one iteration k computed for k + 1, flexible PCG the one that formed the direction of
    iteration k; rho = rh . r_k; rz = r_k . z_k for CG, r_{k-1} . z_{k-1} for flexible PCG) and |b|^2.  Returns the worst error / bound."""
    b, x0 = c.data(which)
    ref = c.reference(which, b, x0, kmax)
    bx, bs = FACTOR * bound[0], FACTOR * bound[1]
    bn2 = float(np.sum(np.asarray(b, dtype=R.LD) ** 2))
    worst = [0.0, 0.0]
    for k in range(1, kmax + 1):
        x, its, reason, _, S = c.solve(which, b, x0, 0.0, 0.0, k)
        assert its == k and reason == DIVERGED_ITS, (k, its, reason)
        ex = R.rel(x, ref[k]["x"])
        es = {s: R.rel(S[SCAL_INDEX[s]], ref[k][s]) for s in R.SCALARS[which]}
        print("  k %2d: x %.2e (bound %.2e) scalars %s (bound %.2e)" % (k, ex, bx, {s: "%.1e" % v for s, v in es.items()}, bs))
        worst = [max(worst[0], ex / bx), max([worst[1]] + [v / bs for v in es.values()])]
        assert ex <= bx, (k, ex, bx)
        for s, v in es.items():
            assert v <= bs, (k, s, v, bs, S[SCAL_INDEX[s]], float(ref[k][s]))
        assert abs(S[IP_BN2] - bn2) <= 4 * np.log2(b.size + 2) * 2.0 ** -53 * bn2 and S[IP_TOL2] == 0.0
    print("ipcs krylov trajectory %s %s: worst error / bound: x %.3f, scalars %.3f" % (NAMES[which], c.name, worst[0], worst[1]))
    return worst


def test_spread_table_is_rounding():
    assert all(0 < v < SPREAD_CAP for row in SPREAD.values() for v in row), SPREAD


@pytest.mark.parametrize("name", ["sq8", "cube4"])
@pytest.mark.parametrize("which", [0, 2])
def test_jacobi_driver_trajectories(case, which, name):
    c = case(name)
    _trajectory(c, which, KMAX[name], SPREAD[(which, name)])


@pytest.mark.parametrize("name", ["sq8", "cube4"])
def test_fpcg_on_a_one_level_hierarchy_is_one_direct_solve(case, name):
    """On the small meshes the hierarchy has one level, the cycle is a direct solve and the first iterate is the solution; what
    later iterations would do to a residual of rounding size is noise, so one iteration is compared: x_1, alpha_1 and rz against the
    reference with the device's cycle as `pre`, to the relative accuracy of the cycle's own fp32 coarse inverse (it enters the
    iterate only through alpha_1 p, which both sides take from the same call)."""
    c = case(name)
    assert c.levels() == 1
    b, x0 = c.data(1)
    ref = c.reference(1, b, x0, 1)
    x, its, reason, _, S = c.solve(1, b, x0, 0.0, 0.0, 1)
    assert its == 1 and reason == DIVERGED_ITS
    # r_0 is formed by the device in float64 and by the reference in extended precision: z_0 = V r_0 is the same vector up to the
    # cycle's Lipschitz constant times u |r_0|, and so are x_1, alpha_1 and rz
    lim = FACTOR * 1e-13
    assert R.rel(x, ref[1]["x"]) <= lim and R.rel(S[IP_ALPHA], ref[1]["alpha"]) <= lim and R.rel(S[IP_RZ], ref[1]["rz"]) <= lim
    assert S[IP_BETA] == 0.0


@pytest.mark.parametrize("dim", [2, 3])
def test_fpcg_trajectories_on_a_two_level_hierarchy(case, dim):
    c = case(FPCG_MESH[dim])
    assert c.levels() >= 2
    _trajectory(c, 1, KMAX[c.name], SPREAD[(1, c.name)])


def test_mesh_smaller_than_one_block(case):
    """create_unit_square(1, 1): 9 nodes, 4 vertices -- every kernel runs one partly filled block.  k = 1 .. 3 (the 9-node problem
    ends in exact arithmetic soon after); the pressure hierarchy has one level, so flexible PCG takes its one iteration."""
    c = case("sq1")
    assert (c.nn, c.nvert) == (9, 4) and c.levels() == 1
    for which in (0, 2):
        _trajectory(c, which, KMAX["sq1"], SPREAD[(which, "sq1")])
    b, x0 = c.data(1)
    ref = c.reference(1, b, x0, 1)
    x, its, reason, _, S = c.solve(1, b, x0, 0.0, 0.0, 1)
    assert its == 1 and reason == DIVERGED_ITS and R.rel(x, ref[1]["x"]) <= FACTOR * 1e-13


# ---- convergence in the middle of a batch --------------------------------------------------------------------------------------
# (case, extra seed) per driver; the Jacobi-CG residual on rho M falls by 2 - 3 per iteration on every mesh, so only the 9-node
# mesh, where it ends in at most 9 iterations, has drops of a factor 4 (tests/test_ipcs_krylov_ref.py checks the targets of drivers
# 0 and 2 on the CPU)
MIDBATCH = {0: [("sq8", 0), ("cube4", 0)], 1: [("sq32", 0), ("cube16", 0)], 2: [("sq1", 1), ("sq1", 2), ("sq8", 0)]}
MIN_RESOLVED = 1e-9   # a target whose |r_k*| is below this fraction of |r_0| is rounding noise of an ended recurrence: not used


def midbatch_targets(tr):
    r0 = float(np.sqrt(tr[0]["rn2"]))
    return [(k, tol) for k, tol in targets(tr) if float(np.sqrt(tr[k]["rn2"])) >= MIN_RESOLVED * r0]


def _direction(c, which):
    return c.ctx.get_intermediate(6 if which == 1 else 5)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_convergence_inside_a_batch_freezes_everything_behind_it(case, which):
    """The tolerance is put between |r_k*| and every earlier residual: the solve must stop at exactly k*, with the iterate, the
    recurrence scalars and the search direction bitwise those of the run capped at k* (Jacobi-CG, whose iteration ends by forming the
    next direction: the direction of the run capped at k* - 1) -- the launches behind the converged iteration changed nothing --
    and a later solve on the same context is bitwise the same solve on a fresh one."""
    used = []
    for name, extra in MIDBATCH[which]:
        c = case(name)
        b, x0 = c.data(which, extra)
        tr = c.reference(which, b, x0, 8)
        bn = float(np.linalg.norm(b))
        for k, tol in midbatch_targets(tr):
            rtol = tol / bn
            if not rtol < 1:
                continue
            xc, its, reason, _, Sc = c.solve(which, b, x0, 0.0, 0.0, k)
            assert its == k and reason == DIVERGED_ITS
            pc = _direction(c, which)
            if which == 2:
                if k > 1:
                    c.solve(which, b, x0, 0.0, 0.0, k - 1)
                    pc = _direction(c, which)
                else:
                    pc = None
            x, its, reason, _, S = c.solve(which, b, x0, rtol, 0.0, 100)
            assert its == k and reason == CONVERGED, (name, k, its, reason)
            assert x.tobytes() == xc.tobytes(), (name, k)
            assert S[IP_RN2] == Sc[IP_RN2] and S[IP_ITS] == k and S[IP_DONE] == 1.0 and S[IP_BAD] == 0.0 and Sc[IP_DONE] == 0.0
            for s in R.SCALARS[which]:
                assert S[SCAL_INDEX[s]] == Sc[SCAL_INDEX[s]], (name, k, s)
            p = _direction(c, which)
            if pc is not None:
                assert p.tobytes() == pc.tobytes(), (name, k, "the search direction moved after convergence")
            else:
                assert R.rel(p.reshape(x.shape), tr[0]["p"]) <= FACTOR * 1e-14
            used.append((name, extra, k))
        # nothing stale survives: the next solve on this context against the same solve on a fresh one
        b2, x2 = c.data(which, 7)
        xa = c.solve(which, b2, x2, 0.0, 0.0, 5)
        f = c.fresh()
        xb = c.solve(which, b2, x2, 0.0, 0.0, 5, ctx=f)
        f.close()
        assert xa[0].tobytes() == xb[0].tobytes()
        for w in [SCAL_INDEX[s] for s in R.SCALARS[which]] + [IP_TOL2, IP_BN2, IP_RN2, IP_DONE, IP_ITS, IP_BAD]:   # the words the driver writes
            assert xa[4][w] == xb[4][w], (name, w)
    print("ipcs krylov mid-batch targets %s: %s" % (NAMES[which], used))
    assert len(used) >= 3 and any(k % 4 for _, _, k in used), used


# ---- edges -------------------------------------------------------------------------------------------------------------------
def _splu_solution(c, which, b):
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    A = c.mat(which).tocsc()
    if which == 1 and c.singular:
        one = np.ones((c.nvert, 1))
        return spl.splu(sp.bmat([[A, one], [one.T, None]]).tocsc()).solve(np.append(b, 0.0))[:-1]
    return spl.splu(A).solve(b)


@pytest.mark.parametrize("name", ["sq8", "cube4"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_edges_of_the_convergence_test(case, which, name):
    c = case(name)
    b, x0 = c.data(which)
    xs = _splu_solution(c, which, b)
    # the solution as initial guess: no iteration, the guess comes back untouched
    x, its, reason, _, S = c.solve(which, b, xs, 1e-8, 0.0, 50)
    assert its == 0 and reason == CONVERGED and x.tobytes() == xs.reshape(x.shape).tobytes()
    # b = 0, x0 = 0, atol = 0: |r| = 0 <= 0 converges at once, and rel_res (the |b| = 0 branch of ip_finish) is finite
    z = np.zeros_like(b)
    x, its, reason, rel_res, S = c.solve(which, z, z, 1e-8, 0.0, 50)
    assert its == 0 and reason == CONVERGED and rel_res == 0.0 and not x.any() and S[IP_BN2] == 0.0
    # b = 0, x0 random, atol = 1e-6: the tolerance in force is atol and rel_res is the absolute residual
    x, its, reason, rel_res, S = c.solve(which, z, x0, 1e-8, 1e-6, 200)
    assert reason == CONVERGED and its > 0 and S[IP_TOL2] == 1e-6 * 1e-6 and S[IP_BN2] == 0.0
    assert rel_res <= 1e-6 and rel_res == np.sqrt(S[IP_RN2])


def test_identity_system_converges_in_its_first_half_step():
    """Every velocity node constrained: A1 = I, alpha = rho / rho = 1 and s = r - v = 0 exactly, so t = 0, omega = 0, r = 0 and
    beta = 0 * inf.  That is convergence at iteration 1 on the exact solution, not a breakdown (stage 3 of ip_scal_kernel looks at
    |r|^2 <= tol^2 before it looks at beta)."""
    m, nm, mk, par, _, bcp, u0 = setup("sq8")
    nn = len(nm.x)
    ctx = _ctx(m, nm, mk, par["dt"], par["rho"], par["mu"], np.zeros(2), [(np.arange(nn, dtype=np.int32), np.zeros((nn, 2)))], bcp)
    z = np.zeros(m.num_vertices)
    ctx.set_state(u_prev=u0.ravel(), p_prev=z, u=u0.ravel(), p=z)
    ctx.set_previous2(u0.ravel())
    A = ctx.get_operator(0)
    import scipy.sparse as sp
    assert abs(A - sp.identity(nn)).max() == 0.0
    rng = np.random.default_rng(51)
    x0, b = rng.integers(-4, 5, size=(nn, 2)).astype(np.float64), rng.integers(-4, 5, size=(nn, 2)).astype(np.float64)
    x, its, reason, rel_res, S = ctx.krylov_solve(0, b, x0, 1e-8, 0.0, 50)
    print("ipcs identity system: its %d reason %d rel_res %.2e bad %g alpha %g omega %g beta %g" % (its, reason, rel_res, S[IP_BAD], S[IP_ALPHA], S[IP_OMEGA], S[IP_BETA]))
    assert reason == CONVERGED and its == 1 and x.tobytes() == b.tobytes() and S[IP_BAD] == 0.0 and S[IP_DONE] == 1.0 and rel_res == 0.0
    assert S[IP_ALPHA] == 1.0 and S[IP_OMEGA] == 0.0
    ctx.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_unattainable_tolerance_keeps_the_invariants(case, which):
    """rtol = 1e-16, max_it = 200 on _case(2): the recurrence residual sinks below what the true residual can reach, so the outer
    loop re-verifies and restarts from the true residual.  Pinned: its <= 200, a reason of converged or DIVERGED_ITS, the residual
    identity (in `solve`) and x within 1e-11 of the direct solution.  This does NOT prove that a restart happened."""
    c = case("sq8")
    b, x0 = c.data(which)
    xs = _splu_solution(c, which, b).reshape(c.shape(which))
    x, its, reason, rel_res, S = c.solve(which, b, x0, 1e-16, 0.0, 200)
    assert its <= 200 and reason in (CONVERGED, DIVERGED_ITS), (its, reason)
    if which == 1 and c.singular:
        x, xs = x - x.mean(), xs - xs.mean()
    err = np.abs(x - xs).max() / np.abs(xs).max()
    print("ipcs krylov rtol 1e-16 %s: its %d reason %d rel_res %.2e, against splu %.2e" % (NAMES[which], its, reason, rel_res, err))
    assert err <= 1e-11


# ---- second trip of the row loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 2])
def test_second_trip_of_the_row_loop(case, which):
    """ip_spmv_kernel runs at most 2048 blocks of 32 rows: create_unit_square(128, 128) has 66 049 P2 nodes, so the rows from
    65 536 on are the second trip of block 0 .. 16.  (a) b with integers in [-4, 4] on those rows only, then on the last row only:
    |b|^2 is an exact integer and x_1 follows the reference; (b) random trajectories, k = 1 .. 3."""
    c = case("sq128")
    assert c.nn == 66049 and c.nn > 2048 * 32
    rng = np.random.default_rng(99)
    for first in (65536, c.nn - 1):
        b = np.zeros(c.shape(which))
        b[first:] = rng.integers(-4, 5, size=b[first:].shape)
        b[-1, 0] = 3.0
        x0 = np.zeros_like(b)
        ref = c.reference(which, b, x0, 1)
        x, its, reason, _, S = c.solve(which, b, x0, 0.0, 0.0, 1)
        assert its == 1 and S[IP_BN2] == float(np.sum(b * b)), (S[IP_BN2], np.sum(b * b))
        assert R.rel(x, ref[1]["x"]) <= FACTOR * SPREAD[(which, "sq128")][0]
    _trajectory(c, which, KMAX["sq128"], SPREAD[(which, "sq128")])


# ---- the hook itself ---------------------------------------------------------------------------------------------------------
def test_hook_leaves_the_time_state_alone(case):
    """A step after hook calls of all three drivers (capped, converged, with their own tolerances) is bitwise the step of a fresh
    context, and so is the step after it."""
    for name in ("sq8", "cube4"):
        c = case(name)
        used, fresh = c.fresh(), c.fresh()
        for ctx in (used, fresh):
            ctx.set_tolerances([1e-9, 1e-8, 1e-10], 1e-50, [300, 200, 100])
        for which in (0, 1, 2):
            b, x0 = c.data(which)
            c.solve(which, b, x0, 0.0, 0.0, 3, ctx=used)
            c.solve(which, b, x0, 1e-3, 0.0, 50, ctx=used)
        for _ in range(2):
            sa, sb = used.step(), fresh.step()
            assert list(sa.its) == list(sb.its) and list(sa.reason) == list(sb.reason) and list(sa.rel_res) == list(sb.rel_res)
            for k in range(5):
                assert used.get_intermediate(k).tobytes() == fresh.get_intermediate(k).tobytes(), (name, k)
            for a, b_ in zip(used.get_solution(), fresh.get_solution()):
                assert a.tobytes() == b_.tobytes()
            for a, b_ in zip(used.get_previous(), fresh.get_previous()):
                assert a.tobytes() == b_.tobytes()
            assert used.get_previous2().tobytes() == fresh.get_previous2().tobytes()
            used.advance()
            fresh.advance()
        used.close()
        fresh.close()


def test_bad_arguments_are_refused_before_anything_runs(case):
    import ctypes
    c = case("sq8")
    L, h = c.ctx.L, c.ctx.h
    b, x0 = c.data(2)
    x, S, st = np.empty(b.size), np.zeros(16), _lib.IpcsStats()
    dp = _lib._dp

    def call(which=2, b=b, x0=x0, rtol=1e-5, atol=0.0, max_it=5, x=x, st=st):
        return L.cfdh_ipcs_krylov_solve(h, which, None if b is None else dp(b), None if x0 is None else dp(x0), rtol, atol, max_it,
                                        None if x is None else dp(x), None if st is None else ctypes.byref(st), dp(S))

    for kw in (dict(which=-1), dict(which=3), dict(b=None), dict(x0=None), dict(x=None), dict(st=None), dict(max_it=0), dict(rtol=-1e-3),
               dict(rtol=1.0), dict(rtol=float("nan")), dict(atol=-1.0)):
        assert call(**kw) == -1, kw
    assert call() == 0
    assert L.cfdh_ipcs_krylov_solve(h, 2, dp(b), dp(x0), 1e-5, 0.0, 5, dp(x), ctypes.byref(st), None) == 0   # scalars may be NULL
    m = create_unit_square(3, 3)
    newton = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
    assert L.cfdh_ipcs_krylov_solve(newton.h, 2, dp(b), dp(x0), 1e-5, 0.0, 5, dp(x), ctypes.byref(st), dp(S)) == -3
    newton.close()
    assert L.cfdh_ipcs_krylov_solve(None, 2, dp(b), dp(x0), 1e-5, 0.0, 5, dp(x), ctypes.byref(st), dp(S)) == -1
