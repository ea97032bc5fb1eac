"""The staged P1 assembly (CFDH_ASM_STAGE, cfdh_kernels.hip) against the addressing and stores it replaces.

By default the kernel reads the per-block vertex and cell lists from a second copy at a fixed stride (padded with -1), whose
address needs no descriptor; CFDH_ASM_STAGE=0 is the kernel as it was, lists through blk_vptr / blk_cptr.
The arithmetic is the same in both -- same values in the same LDS slots, same code behind the barrier -- so the bound is not a
tolerance: F and every stored value of the matrix agree BYTE FOR BYTE, and a whole time step takes the same iterations to the
same bits.  The switch is read when a context is created, so one process holds a context of each kind.

Padded slots: a lane that read through a -1 would gather from outside the arrays, so both ends are exercised -- lists shorter
than the stride by more than 64 and lists that fill it to within 8, for vertices and for cells (test_padding_is_exercised
asserts it from the set-up tables, cfdh_info 98..101).  In the meshes' own numbering a workgroup runs out of lanes long before
its lists fill: on dfg_case(4 .. 48), lid_case(8, 40) and stenosis_case(12, 24) the longest vertex list is 104 and the longest
cell list 132 of 192.  The full lists come from dfg_case(12) with its vertices renumbered (renumbered_dfg12) and the library's
own Morton numbering switched off for these contexts (CFDH_NO_RENUMBER=1, read when a context is created): an independent
set of the vertex graph first -- rows that share no cell, so every row brings all its cells and the cell list fills first --
then the rest in random order, where every row brings itself and all its neighbours and the vertex list fills first."""
import contextlib
import os

import numpy as np
import pytest

from util import Case, dfg_case, lid_case, make_ctx, stenosis_backflow_case, stenosis_case

pytestmark = pytest.mark.gpu

MAX_BV = MAX_BC = 192  # CFDH_MAX_BV, CFDH_MAX_BC (cfdh_internal.hpp)
INFO_VL_MAX, INFO_VL_MIN, INFO_CL_MAX, INFO_CL_MIN, INFO_STAGE = 98, 99, 100, 101, 102
BDF2 = (1.0, 1.5, -2.0, 0.5)
STAGES = (0, 1, None)  # None: the default, which is 1

MESHES = {"dfg6": (dfg_case, 6), "dfg24": (dfg_case, 24), "lid8": (lid_case, 8), "stenosis12": (stenosis_case, 12),
          "backflow12": (stenosis_backflow_case, 12)}
_CASES = {}


def renumbered_dfg12():
    """dfg_case(12), vertices renumbered: a maximal independent set in the old order, then the others shuffled (fixed seed)"""
    case = dfg_case(12)
    m = case.mesh
    nv, cells = case.nv, np.asarray(m.cells)
    nbr = [set() for _ in range(nv)]
    for c in cells:
        for a in c:
            nbr[a].update(int(b) for b in c)
    taken, blocked = [], np.zeros(nv, bool)
    for v in range(nv):
        if not blocked[v]:
            taken.append(v)
            blocked[list(nbr[v])] = True
    rest = np.setdiff1d(np.arange(nv), taken)
    np.random.default_rng(2).shuffle(rest)
    old = np.concatenate([np.asarray(taken, dtype=np.int64), rest])  # old[new]
    new = np.empty(nv, np.int64)
    new[old] = np.arange(nv)

    class RawMesh:
        pass

    r = RawMesh()
    r.x, r.cells = np.ascontiguousarray(np.asarray(m.x)[old]), new[cells].astype(np.asarray(m.cells).dtype)
    r.facet_cells, r.facet_local, r.facet_marker = m.facet_cells, m.facet_local, m.facet_marker  # cell-based: unchanged
    r.num_vertices = nv
    bcs = [(f, new[np.asarray(n)].astype(np.int32), v) for f, n, v in case.bcs]
    out = Case(r, bcs, case.dt, case.rho, case.mu, case.f)
    out.keep_numbering = True
    return out


def case_of(name):
    if name not in _CASES:
        if name == "dfg12r":
            _CASES[name] = renumbered_dfg12()
        else:
            fn, arg = MESHES[name]
            _CASES[name] = fn(arg)
    return _CASES[name]


@contextlib.contextmanager
def environment(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def context(case, stage):
    """stage None: the default.  The renumbered mesh keeps its numbering (CFDH_NO_RENUMBER=1: no Morton order inside)."""
    with environment(CFDH_ASM_STAGE=stage, CFDH_NO_RENUMBER=1 if getattr(case, "keep_numbering", False) else None):
        ctx = make_ctx(case)
    assert ctx.info(INFO_STAGE) == (1 if stage is None else stage)
    return ctx


def _rand_state(nv, seed):
    rng = np.random.default_rng(seed)
    return 0.1 * rng.standard_normal(3 * nv), 0.1 * rng.standard_normal(2 * nv), 0.1 * rng.standard_normal(2 * nv)


def _assembled(case, stage, scheme):
    """(F, data) after assemble(True), F after assemble(False); random state that violates the Dirichlet data (lifting runs)"""
    nv = case.nv
    xv, un, un2 = _rand_state(nv, 11)
    ctx = context(case, stage)
    if scheme is not None:
        ctx.set_time_scheme(*scheme)
    ctx.set_state(u_prev=un, p_prev=np.zeros(nv), u=xv[: 2 * nv], p=xv[2 * nv:])
    if scheme is not None:
        ctx.set_previous2(un2)
    ctx.assemble(True)
    F1 = np.concatenate(ctx.get_residual())
    data = ctx.get_csr().data.copy()
    ctx.assemble(False)
    F2 = np.concatenate(ctx.get_residual())
    # the pass without the Jacobian must leave the stored matrix alone
    assert np.array_equal(ctx.get_csr().data, data)
    ctx.close()
    return F1, data, F2


# the BDF2 kernels (HIST2) on two meshes, the backflow kernels (BF, two waves per SIMD) on the stenosis with a do-nothing outlet
VARIANTS = [("dfg6", None), ("dfg24", None), ("lid8", None), ("stenosis12", None), ("dfg12r", None),
            ("dfg6", BDF2), ("dfg12r", BDF2), ("backflow12", None), ("backflow12", BDF2)]


@pytest.mark.parametrize("name,scheme", VARIANTS, ids=["%s%s" % (n, "-bdf2" if s else "") for n, s in VARIANTS])
def test_assembly_is_byte_identical(name, scheme):
    case = case_of(name)
    ref = _assembled(case, 0, scheme)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.abs(ref[1]).max() > 0
    for stage in (1, None):  # None: the default
        got = _assembled(case, stage, scheme)
        for what, a, b in zip(("F of assemble(True)", "matrix values", "F of assemble(False)"), ref, got):
            assert a.shape == b.shape and np.array_equal(a, b), "%s differs at stage %s" % (what, stage)


def test_contexts_of_each_kind_side_by_side():
    """The switch belongs to the context: live contexts of both kinds, assembled in turn, then once more in reverse order."""
    case = case_of("dfg24")
    nv = case.nv
    xv, un, _ = _rand_state(nv, 5)
    ctxs = [context(case, s) for s in STAGES]
    out = []
    for order in (ctxs, ctxs[::-1]):
        for ctx in order:
            ctx.set_state(u_prev=un, p_prev=np.zeros(nv), u=xv[: 2 * nv], p=xv[2 * nv:])
            ctx.assemble(True)
            out.append((np.concatenate(ctx.get_residual()), ctx.get_csr().data.copy()))
    for F, data in out[1:]:
        assert np.array_equal(F, out[0][0]) and np.array_equal(data, out[0][1])
    for ctx in ctxs:
        ctx.close()


def test_one_time_step_same_bits_same_counts():
    case = dfg_case(12)
    nv = case.nv
    res = {}
    for stage in (0, None):
        ctx = context(case, stage)
        o = ctx.default_options()
        o.snes_rtol, o.snes_stol, o.ksp_rtol = 1e-12, 0.0, 1e-10
        ctx.set_options(o)
        z2, z1 = np.zeros(2 * nv), np.zeros(nv)
        ctx.set_state(u_prev=z2, p_prev=z1, u=z2, p=z1)
        st = ctx.solve_step()
        assert st.reason > 0
        res[stage] = (st.newton_its, st.krylov_its, np.concatenate(ctx.get_solution()))
        ctx.close()
    assert res[0][0] == res[None][0] and res[0][1] == res[None][1], (res[0][:2], res[None][:2])
    assert np.abs(res[0][2]).max() > 0 and np.array_equal(res[0][2], res[None][2])


def test_padding_is_exercised():
    """Lists shorter than the stride by more than 64 and lists within 8 of it, for vertices and for cells, on one of the meshes
    of the byte-for-byte test."""
    ctx = context(case_of("dfg12r"), None)
    vmax, vmin, cmax, cmin = (ctx.info(k) for k in (INFO_VL_MAX, INFO_VL_MIN, INFO_CL_MAX, INFO_CL_MIN))
    nblk = ctx.info(7)
    ctx.close()
    print("renumbered dfg_case(12): %d blocks, vertex lists %d..%d, cell lists %d..%d" % (nblk, vmin, vmax, cmin, cmax))
    assert nblk > 1
    assert 0 < vmin < MAX_BV - 64 and MAX_BV - 8 <= vmax <= MAX_BV
    assert 0 < cmin < MAX_BC - 64 and MAX_BC - 8 <= cmax <= MAX_BC
