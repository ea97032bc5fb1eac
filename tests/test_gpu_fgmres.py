"""The FGMRES driver (cfdh_fgmres in csrc/cfdh_solver.cpp) cycle by cycle, through cfdh_fgmres_solve: what the device holds after a
cycle -- V, Z, the unrotated Hessenberg columns, y, the iterates -- against the six invariants of tests/fgmres_ref.py in
np.longdouble on J of cfdh_get_csr.  No twin of the preconditioner is needed: FGMRES assumes nothing about z_j = P^-1 v_j.
The driver corrects itself (true residual after every cycle), so a wrong Hessenberg column, a ring slot consumed late or a y
applied to the wrong columns costs iterations and never the answer; test_fgmres_ref.py shows that these checks see such mistakes.

Cases: lid cavity 16 (singular pressure, mean removal), DFG 8, a perturbed cube of tetrahedra, and the stenosed channel with a
weakened preconditioner (LONG) whose cycles at ksp_rtol 1e-7 are longer than twice the read-back ring.  The state is random
and violates the Dirichlet data; b is random with zero Dirichlet rows, mean-free in the pressure on the lid case."""
import functools
import os

import numpy as np
import pytest

import fgmres_ref as R
from util import dfg_case, lid_case, make_ctx, stenosis_case

pytestmark = pytest.mark.gpu

KRING = 12
# the long-cycle case: mesh, time step, size of the random state, and the weakening of the preconditioner; test_long_case_is_long
# asserts what makes it meaningful
# (measured at ksp_rtol 1e-7, right-hand side LONG_SEED: 40 iterations in one cycle, 1 discarded, 7 host synchronisations; with
# Cahouet-Chabard, pc_type 1, and the same smoothers 23 iterations and nothing discarded; at default options 18)
LONG = dict(ny=16, dt=0.01, scale=10.0, opts=dict(cheb_degree=1, cc_smooth_degree=1, pc_type=0))
LONG_SEED = 3
INFO_DISCARDED, INFO_ITER_SYNC, INFO_RANK, INFO_K, INFO_CYCLES, INFO_SINGULAR, INFO_LEAN = 73, 87, 88, 89, 84, 76, 85


class _env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class TetCase:
    """the perturbed unit cube of test_gpu_3d.py's smallest parity test, with its three Dirichlet sets"""

    def __init__(self):
        from cfd_hemodynamic_amd.mesh3d import Mesh3D, create_unit_cube
        n = 4
        m = create_unit_cube(n)
        rng = np.random.default_rng(3)
        interior = np.abs(m.x - 0.5).max(axis=1) < 0.49
        self.mesh = Mesh3D(m.cells, m.x + (0.12 / n) * rng.standard_normal(m.x.shape) * interior[:, None])
        x = self.mesh.x
        bnd = np.unique(self.mesh.facet_vertices)
        top, side, back = bnd[x[bnd, 2] > 0.99], bnd[x[bnd, 0] < 0.01], bnd[x[bnd, 1] > 0.99]
        self.bcs = [(0, side.astype(np.int32), rng.standard_normal((len(side), 3))),
                    (0, top.astype(np.int32), rng.standard_normal((len(top), 3))),
                    (1, back.astype(np.int32), rng.standard_normal(len(back)))]
        self.dt, self.rho, self.mu, self.f = 0.02, 1.3, 0.04, (0.2, -0.1, 0.3)
        self.nv = self.mesh.num_vertices


CASES = {"lid16": lambda: lid_case(16), "dfg8": lambda: dfg_case(8), "tet": TetCase, "long": lambda: stenosis_case(LONG["ny"], dt=LONG["dt"])}


class Problem:
    """A context at a random state with its Jacobian assembled, J in extended precision, and right-hand sides."""

    def __init__(self, key, opts=None, env=None):
        self.key, self.env = key, dict(env or {})
        case = CASES[key]()
        with _env(**self.env):
            ctx = make_ctx(case)
        self.ctx, self.nv, self.dim = ctx, case.nv, ctx.dim
        d, nv = self.dim, self.nv
        self.n = (d + 1) * nv
        self.opts = dict(LONG["opts"]) if key == "long" else {}
        self.opts.update(opts or {})
        self.set_options()
        if key == "lid16":
            # the constant-pressure null space is detected by the Newton step: one step from rest sets the flag (and builds the
            # preconditioner, which the hook then applies lagged); without the projected guess, so that its rings start empty here
            self.set_options(ksp_guess=0)
            ctx.set_state(u_prev=np.zeros(d * nv), p_prev=np.zeros(nv), u=np.zeros(d * nv), p=np.zeros(nv))
            assert ctx.solve_step().reason > 0
            self.set_options()
        rng = np.random.default_rng(11)
        scale = LONG["scale"] if key == "long" else 0.1
        ctx.set_state(u_prev=scale * rng.standard_normal(d * nv), p_prev=np.zeros(nv), u=scale * rng.standard_normal(d * nv),
                      p=0.1 * rng.standard_normal(nv))
        ctx.assemble(True)
        self.singular = ctx.info(INFO_SINGULAR) == 1
        assert self.singular == (key == "lid16")
        self.S = R.System(ctx.get_csr())
        fixed = np.zeros(self.n, dtype=bool)
        for field, nodes, _ in case.bcs:
            nodes = np.asarray(nodes)
            if field == 0:
                for i in range(d):
                    fixed[d * nodes + i] = True
            else:
                fixed[d * nv + nodes] = True
        self.fixed = fixed
        self.pslice = slice(d * nv, (d + 1) * nv)

    def set_options(self, **kw):
        o = self.ctx.default_options()
        for k, v in {**self.opts, **kw}.items():
            setattr(o, k, v)
        self.ctx.set_options(o)
        return o

    def rhs(self, seed):
        b = np.random.default_rng(1000 + seed).standard_normal(self.n)
        b[self.fixed] = 0.0
        if self.singular:
            b[self.pslice] -= b[self.pslice].mean()
        return b

    def solve(self, b, newton_index=-1, trace=True, **kw):
        if kw:
            self.set_options(**kw)
        before = {i: self.ctx.info(i) for i in (INFO_DISCARDED, INFO_ITER_SYNC, INFO_CYCLES)}
        x, its, reason, t = self.ctx.fgmres_solve(b, newton_index, trace=trace)
        if t is None:
            t = {}
        t.update(x=x, its=its, reason=reason, b=b)
        t["delta"] = {i: self.ctx.info(i) - v for i, v in before.items()}
        if kw:
            self.set_options()
        return t

    def close(self):
        self.ctx.close()


@functools.lru_cache(maxsize=None)
def problem(key, opts=(), env=()):
    return Problem(key, dict(opts), dict(env))


def cycle(t):
    """the last cycle of a traced solve in the form fgmres_ref checks"""
    k = t["k"]
    assert len(t["res"]) == t["its"]
    return dict(V=t["V"], Z=t["Z"], H=t["H"], y=t["y"], beta=t["beta"], x_start=t["x_start"], x=t["x"], res=t["res"][t["its"] - k:],
                second_pass=t["second_pass"], fp32_used=t["fp32_used"])


def true_residual(P, b, x):
    return float(R.norm(R.ld(b) - P.S.mul(x)))


def norm_allowance(P, b, x):
    """a device |b - J x| against the long-double one: the floor of the float64 residual (entry bound of I2 in norm) and the dot
    bound of the sum of squares"""
    return P.S.floor(b, x, 2.0) + R.KV.dot_bound(P.n, 1.0) * true_residual(P, b, x)


# ---- one cycle from a zero guess, every context -----------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["lid16", "dfg8", "tet", "long"])
def test_one_cycle_from_zero(key):
    P = problem(key)
    b = P.rhs(0)
    t = P.solve(b)
    print("%s: n = %d, its %d, reason %d, cycles %d" % (key, P.n, t["its"], t["reason"], t["cycles"]))
    assert t["reason"] == 2 and t["cycles"] == 1 and t["k"] == t["its"] >= 4
    assert not t["guess_used"] and not t["fp32_used"] and not t["x0"].any() and not t["x_start"].any()
    assert t["bn"] == pytest.approx(float(np.linalg.norm(b)), rel=1e-13) and t["tol"] == 1e-5 * t["bn"]
    assert t["res"][-1] <= t["tol"] < t["res"][-2]
    assert abs(t["cycle_est"][0] - t["res"][-1]) == 0.0 and t["cycle_beta"][0] == t["beta"] == t["bn"]
    R.check_cycle(P.S, b, cycle(t), refined=False, label=key)
    # the untraced call returns the same bytes
    u = P.solve(b, trace=False)
    assert np.array_equal(u["x"], t["x"]) and (u["its"], u["reason"]) == (t["its"], t["reason"])


# ---- the iteration cap ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["dfg8", "lid16"])
def test_iteration_cap(key):
    P = problem(key)
    b = P.rhs(1)
    full = P.solve(b)
    kstar = full["its"]
    assert full["reason"] == 2 and full["cycles"] == 1 and kstar >= 4
    prev = None
    for k in range(1, kstar + 1):
        t = P.solve(b, ksp_max_it=k)
        assert t["its"] == k and t["k"] == k and t["reason"] == (2 if k == kstar else -3), (k, t["its"], t["reason"])
        R.check_cycle(P.S, b, cycle(t), refined=False, label="%s cap %d" % (key, k))
        if prev is not None:
            assert np.array_equal(prev, t["res"][:k - 1])
        prev = t["res"]
    assert np.array_equal(prev, full["res"]) and np.array_equal(t["x"], full["x"])


# ---- launch-ahead against synchronous, long cycles --------------------------------------------------------------------------------
def _long(lag, eta2=None, **kw):
    env = {"CFDH_KSP_LAG": lag}
    if eta2 is not None:
        env["CFDH_GS_ETA2"] = eta2
    return problem("long", tuple(sorted({"ksp_rtol": 1e-7, **kw}.items())), tuple(sorted(env.items())))


def test_long_case_is_long():
    """what makes the long-cycle case meaningful: the ring wraps twice in ONE cycle, something ran ahead and was discarded, and the
    host processed in batches"""
    P = _long(9)
    b = P.rhs(LONG_SEED)
    t = P.solve(b)
    print("long: n = %d, its %d, cycles %d, discarded %d, host synchronisations %d" % (
        P.n, t["its"], t["cycles"], t["delta"][INFO_DISCARDED], t["delta"][INFO_ITER_SYNC]))
    assert t["reason"] == 2 and t["cycles"] == 1
    assert t["k"] >= 2 * KRING + 2
    assert t["delta"][INFO_DISCARDED] > 0
    assert t["delta"][INFO_ITER_SYNC] < t["its"]
    R.check_cycle(P.S, b, cycle(t), refined=False, label="long lag 9")
    # the same solve stopped after the ring has wrapped once: bitwise a prefix, and the basis is still a basis there (I5 says something)
    u = P.solve(b, ksp_max_it=KRING + 2)
    assert (u["its"], u["reason"]) == (KRING + 2, -3) and np.array_equal(u["res"], t["res"][:KRING + 2])
    assert np.array_equal(u["H"], t["H"][:KRING + 3, :KRING + 2])
    assert R.eps_v(u["V"]) < 0.1
    R.check_cycle(P.S, b, cycle(u), refined=False, label="long lag 9 capped")


def _same_bits(a, c):
    assert (a["its"], a["reason"], a["k"]) == (c["its"], c["reason"], c["k"])
    for name in ("x", "H", "res", "y"):
        assert np.array_equal(a[name], c[name]), name


def test_launch_ahead_is_bitwise_the_synchronous_solve():
    """Every iteration launches the same kernels on the same inputs whenever the host gets round to reading its slot."""
    runs = {}
    for lag in (0, 1, 9):
        P = _long(lag)
        runs[lag] = P.solve(P.rhs(LONG_SEED))
    assert runs[0]["delta"][INFO_ITER_SYNC] == runs[0]["its"] and runs[0]["delta"][INFO_DISCARDED] == 0
    _same_bits(runs[0], runs[1])
    _same_bits(runs[0], runs[9])


def test_second_pass_in_flight_relaunches():
    """CFDH_GS_ETA2 raised (to the lower third of the ratios |w'|^2 / |w|^2 this solve shows): some iterations take the second pass
    while later ones are in flight; those are launched again from the refined vector, so the solve stays bitwise the synchronous
    one."""
    P = _long(0)
    t = P.solve(P.rhs(LONG_SEED))
    ETA2_RAISED = float("%.3g" % np.quantile(t["nrm2"] / t["ww"], 0.35))
    print("ratios %s -> CFDH_GS_ETA2 = %g" % (np.round(t["nrm2"] / t["ww"], 4).tolist(), ETA2_RAISED))
    a, c = _long(0, ETA2_RAISED), _long(9, ETA2_RAISED)
    b = a.rhs(LONG_SEED)
    ta, tc = a.solve(b), c.solve(b)
    print("second pass per column, lag 0: %s\n                        lag 9: %s" % (ta["second_pass"].tolist(), tc["second_pass"].tolist()))
    assert (tc["second_pass"] == 2).any() and not (ta["second_pass"] == 2).any()
    assert np.array_equal(ta["second_pass"] > 0, tc["second_pass"] > 0)
    assert np.array_equal(ta["second_pass"] > 0, ~(ta["nrm2"] > ETA2_RAISED * ta["ww"]))
    _same_bits(ta, tc)
    R.check_cycle(c.S, b, cycle(tc), refined=False, label="long lag 9 eta2 %g" % ETA2_RAISED)


# ---- the tight path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["dfg8", "tet"])
def test_tight_path(key):
    P = problem(key)
    b = P.rhs(3)
    t = P.solve(b, ksp_rtol=1e-10)
    print("%s tight: its %d, cycles %d, reason %d, second passes %d" % (key, t["its"], t["cycles"], t["reason"], int((t["second_pass"] > 0).sum())))
    assert t["reason"] == 2 and t["its"] >= 8
    assert t["delta"][INFO_ITER_SYNC] >= t["its"] and t["delta"][INFO_DISCARDED] == 0      # synchronous
    assert np.array_equal(t["second_pass"] > 0, ~(t["nrm2"] > 0.5 * t["ww"]))             # DGKS criterion
    assert not (t["second_pass"] == 2).any()
    R.check_cycle(P.S, b, cycle(t), refined=True, label=key + " tight")


# ---- restart ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean", [1, 0])
def test_restart(lean):
    # (with the Cahouet-Chabard Schur approximation: the lean forms of prologue, epilogue and true residual exist for it)
    P = problem("long", (("pc_type", 1),), (("CFDH_SOLVE_LEAN", lean),))
    assert P.ctx.info(INFO_LEAN) == lean
    b = P.rhs(4)
    m = 7
    t = P.solve(b, ksp_restart=m)
    its, k, ncyc = t["its"], t["k"], t["cycles"]
    print("restart %d lean %d: its %d, cycles %d, last cycle %d" % (m, lean, its, ncyc, k))
    assert t["reason"] == 2 and ncyc >= 3 and ncyc == -(-its // m) and k == its - m * (ncyc - 1)
    R.check_cycle(P.S, b, cycle(t), refined=False, label="restart lean %d" % lean)
    # the iterate each cycle started from: the same solve capped there; its true residual on the host against the device's
    for c in range(ncyc):
        if c == 0:
            xc = np.zeros(P.n)
        else:
            u = P.solve(b, ksp_restart=m, ksp_max_it=m * c)
            assert (u["its"], u["reason"]) == (m * c, -3)
            assert np.array_equal(u["res"], t["res"][:m * c])
            xc = u["x"]
        ref = true_residual(P, b, xc)
        assert abs(t["cycle_beta"][c] - ref) <= norm_allowance(P, b, xc), (c, t["cycle_beta"][c], ref)
    assert np.array_equal(xc, t["x_start"])
    assert np.array_equal(t["cycle_est"], t["res"][[min(m * (c + 1), its) - 1 for c in range(ncyc)]])


# ---- the fp32 copy of the basis ---------------------------------------------------------------------------------------------------
def test_fp32_copy():
    P = problem("long", (), (("CFDH_KRYLOV_FP32", 2),))
    b = P.rhs(5)
    t = P.solve(b, ksp_rtol=1e-6)
    print("fp32 copy: its %d, cycles %d" % (t["its"], t["cycles"]))
    assert t["reason"] == 2 and t["fp32_used"] and t["k"] >= KRING
    R.check_cycle(P.S, b, cycle(t), refined=False, label="fp32 copy")
    u = P.solve(b, ksp_rtol=1e-7)
    assert u["reason"] == 2 and not u["fp32_used"]


# ---- the projected initial guess --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lean", [1, 0])
@pytest.mark.parametrize("key", ["dfg8", "lid16"])
def test_projected_guess(key, lean):
    P = problem(key, (), (("CFDH_SOLVE_LEAN", lean),))
    assert P.ctx.info(INFO_LEAN) == lean
    S = P.S
    sp_ = P.pslice if P.singular else None
    U = []
    for i in range(4):
        t = P.solve(P.rhs(10 + i), newton_index=0)
        assert t["reason"] == 2 and t["guess_used"] == (i > 0)
        U.append(t["x"])
    U = np.array(U)
    b5 = P.rhs(10) + 0.5 * P.rhs(12) + 1e-3 * P.rhs(20)   # mostly inside J span(U): the guess matters
    t = P.solve(b5, newton_index=0)
    assert t["reason"] == 2 and t["guess_used"] and P.ctx.info(INFO_RANK) == 4 == P.ctx.info(INFO_K)
    got, best, allow, xmag = R.guess_check(S, b5, U, t["x0"], sp_)
    print("%s lean %d: |b - J x0| = %.6e, minimum over the span %.6e, allowance %.2e; |b| = %.3e; its %d" % (key, lean, got, best, allow, t["bn"], t["its"]))
    assert best <= 0.05 * t["bn"]
    assert best - allow <= got <= best + allow
    if t["cycles"] == 1:
        assert np.array_equal(t["x0"], t["x_start"])
        r2, r2b = R.i2_start(S, b5, cycle(t), xmag)
        print("   I2 from the guess: %.3f, beta %.3f" % (r2, r2b))
        assert r2 <= 1.0 and r2b <= 1.0
        R.check_cycle(S, b5, cycle(t), refined=False, xmag=xmag, label="%s guess lean %d" % (key, lean))
    if P.singular:
        assert abs(t["x0"][P.pslice].mean()) <= 1e-14 * np.abs(t["x0"][P.pslice]).max()
    # the ring now holds the solutions of rhs 11, 12, 13 and b5.  Three times the last right-hand side starts below the tolerance.
    e = P.solve(3.0 * b5, newton_index=0)
    assert (e["its"], e["reason"], e["cycles"]) == (0, 2, 0) and e["guess_used"]
    assert np.array_equal(e["x"], e["x0"]) and e["beta"] == 0.0
    assert true_residual(P, 3.0 * b5, e["x0"]) <= e["tol"] + norm_allowance(P, 3.0 * b5, e["x0"])
    # rank drop, on the ring of Newton index 1: x, then a multiple of x (the solve of 2 b starts converged from y x), then b'
    b1 = P.rhs(30)
    a = P.solve(b1, newton_index=1)
    d = P.solve(2.0 * b1, newton_index=1)
    assert a["reason"] == 2 and not a["guess_used"] and (d["its"], d["reason"]) == (0, 2) and d["guess_used"]
    b2 = b1 + 0.1 * P.rhs(31)
    g = P.solve(b2, newton_index=1)
    assert (P.ctx.info(INFO_RANK), P.ctx.info(INFO_K)) == (1, 2) and g["guess_used"] and g["reason"] == 2
    got, best, allow, _ = R.guess_check(S, b2, a["x"][None, :], g["x0"], sp_)
    print("   rank 1 of 2: |b - J x0| = %.6e, minimum %.6e, allowance %.2e" % (got, best, allow))
    assert best - allow <= got <= best + allow and best <= 0.2 * g["bn"]
    # a Krylov workspace too small to hold the products of the kept vectors: no guess
    z = P.solve(b5, newton_index=0, ksp_restart=4, ksp_max_it=3)
    assert not z["guess_used"] and not z["x0"].any() and z["its"] == 3 and z["reason"] == -3


# ---- degenerate right-hand sides --------------------------------------------------------------------------------------------------
def test_degenerate_right_hand_sides():
    P = problem("dfg8")
    b = P.rhs(6)
    ref = P.solve(b)
    z = P.solve(np.zeros(P.n))
    assert (z["its"], z["reason"], z["cycles"]) == (0, 2, 0) and not z["x"].any() and z["bn"] == 0.0
    bad = b.copy()
    bad[np.flatnonzero(~P.fixed)[7]] = np.nan
    q = P.solve(bad)
    assert (q["its"], q["reason"], q["cycles"]) == (0, -9, 0)
    again = P.solve(b)
    _same_bits(ref, again)
    big = P.solve(b, ksp_atol=2.0 * float(np.linalg.norm(b)))
    assert (big["its"], big["reason"]) == (0, 2) and not big["x"].any()


# ---- the hook leaves the context alone --------------------------------------------------------------------------------------------
def test_hook_hygiene():
    from cfd_hemodynamic_amd import _lib
    case = dfg_case(8)
    nv = case.nv
    ctxs = [make_ctx(case) for _ in range(2)]
    for c in ctxs:
        c.set_state(u_prev=np.zeros(2 * nv), p_prev=np.zeros(nv), u=np.zeros(2 * nv), p=np.zeros(nv))
        assert c.solve_step().reason > 0
    a, ref = ctxs

    def snapshot(c):
        h = c.newton_history()
        return [np.concatenate(c.get_solution()), np.concatenate(c.get_residual())] + [h[k].copy() for k in sorted(h)]

    before = snapshot(a)
    counters = [a.info(i) for i in (15, INFO_CYCLES, INFO_ITER_SYNC)]
    b = np.random.default_rng(9).standard_normal(3 * nv)
    x = np.zeros(3 * nv)
    its, reason = _lib.C.c_int32(), _lib.C.c_int32()
    dp, L = _lib._dp, a.L
    for args in ((None, -1, dp(x)), (dp(b), -1, None), (dp(b), -2, dp(x)), (dp(b), 4, dp(x))):
        assert L.cfdh_fgmres_solve(a.h, args[0], args[1], args[2], _lib.C.byref(its), _lib.C.byref(reason), None) == -1
    assert L.cfdh_fgmres_solve(None, dp(b), -1, dp(x), _lib.C.byref(its), _lib.C.byref(reason), None) == -1
    small = _lib.FgmresTrace(m=3)
    assert L.cfdh_fgmres_solve(a.h, dp(b), -1, dp(x), _lib.C.byref(its), _lib.C.byref(reason), _lib.C.byref(small)) == -1
    assert [a.info(i) for i in (15, INFO_CYCLES, INFO_ITER_SYNC)] == counters      # nothing was launched or read back
    for got, want in zip(snapshot(a), before):
        assert np.array_equal(got, want)
    xs, its_, reason_, t = a.fgmres_solve(b, -1)
    assert reason_ == 2 and its_ > 0
    xu, itu, ru, _ = a.fgmres_solve(b, -1, trace=False)
    assert np.array_equal(xs, xu) and (its_, reason_) == (itu, ru)
    for got, want in zip(snapshot(a), before):
        assert np.array_equal(got, want)
    # the next steps are those of a context that never called the hook
    for _ in range(2):
        for c in ctxs:
            c.advance()
        sa, sr = a.solve_step(), ref.solve_step()
        assert (sa.newton_its, sa.krylov_its, sa.reason) == (sr.newton_its, sr.krylov_its, sr.reason)
        assert np.array_equal(np.concatenate(a.get_solution()), np.concatenate(ref.get_solution()))
    for c in ctxs:
        c.close()
