"""The head copies of the SELL-64 sweep operators (CsrDev::hcol ..., csrc/cfdh_amg_dev.hip: cfdh_amg_heads; fused_up_sell_head_kernel and
sell_cheb2_scale_kernel<true> in csrc/cfdh_amg_apply.hip) change where a sweep finds an entry, never which entries it adds or in which
order.  So the bound is derived, not measured: z = P^-1 r with CFDH_AMG_HEAD=1 equals z with CFDH_AMG_HEAD=0 BYTE FOR BYTE, for every
head width.

Only SELL-64 operators have heads (Sb, Sc of a finest level of 16384 rows or more, the Chebyshev matrix of H); heads of the CSR
operators were built, measured slower and removed.  The meshes that run a head kernel are therefore the smallest
whose finest level takes SELL-64: dfg_case(64) for fused_up_sell_head<.., false> and sell_cheb2_scale<true>, a cube of 27^3 vertices for
the chunked kernel fused_up_sell_head<double, true>; neither vertex count is a multiple of 64 (partial last slice).  Widths:
CFDH_AMG_HEAD_W = 1, 2, the widest a kernel preloads, and the width the rule picks.  The widths are read back (cfdh_get_amg_head) and
checked against the downloaded operators: every headed operator must, at one width at least, have slices with a tail and slices
without -- per operator, so that each kernel is shown to have seen both.

dfg_case(4), a lid case and the smallest cube of tetrahedra take CSR on every level: no head can exist there.  They stay as a guard
that the switch changes nothing where it has nothing to act on (and that no head is built).  For the same reason the whole step runs on
dfg_case(64), not on a smaller mesh.  The up-sweep on the first up0_rows rows only belongs to the overlapping velocity cycle of a
partitioned run: two ranks (tests/_gpu_amg_head_worker.py), which report their head widths and row counts."""
import contextlib
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest

from util import dfg_case, lid_case, make_ctx

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.mesh3d import create_unit_cube

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HA, HL, HH = _lib.AMG_HIER_A, _lib.AMG_HIER_P, _lib.AMG_HIER_H
OPS = (("Sb", _lib.AMG_OP_SB), ("Sc", _lib.AMG_OP_SC))


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


def _cube(n):
    m = create_unit_cube(n)
    bnd = np.nonzero((np.abs(m.x - 0.5).max(axis=1) > 0.5 - 1e-12))[0].astype(np.int32)
    out = bnd[np.isclose(m.x[bnd, 0], 1.0)]
    wall = np.setdiff1d(bnd, out).astype(np.int32)
    return m, [(0, wall, np.zeros((len(wall), 3))), (1, out, np.zeros(len(out)))]


_MESH = {}


def problem(name):
    """mesh, Dirichlet sets, dt, rho, mu, options"""
    if name not in _MESH:
        if name in ("dfg4", "dfg64"):
            k = dfg_case(4 if name == "dfg4" else 64)
            _MESH[name] = (k.mesh, k.bcs, k.dt, k.rho, k.mu, dict(amg_max_coarse=8) if name == "dfg4" else {})
        elif name == "lid":
            k = lid_case(13)     # 196 vertices
            _MESH[name] = (k.mesh, k.bcs, k.dt, k.rho, k.mu, dict(amg_max_coarse=8))
        elif name == "tet":
            m, bcs = _cube(3)
            _MESH[name] = (m, bcs, 0.01, 1.0, 1e-2, dict(amg_max_coarse=8))
        elif name == "tet26":
            m, bcs = _cube(26)    # 19683 vertices
            _MESH[name] = (m, bcs, 0.01, 1.0, 1e-2, dict(amg_max_coarse=500))
        else:
            raise KeyError(name)
    return _MESH[name]


def context(name, head, width=0):
    m, bcs, dt, rho, mu, opts = problem(name)
    with environment(CFDH_AMG_HEAD=head, CFDH_AMG_HEAD_W=width if width else None):
        markers = m.facet_marker if getattr(m, "facet_marker", None) is not None else np.zeros(len(m.facet_cells), np.int32)
        ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, markers)
        dim, nv = ctx.dim, ctx.nv
        ctx.set_params(dt, rho, mu, f=np.zeros(dim))
        for f, n, v in bcs:
            ctx.add_dirichlet(f, n, v)
        o = ctx.default_options()
        for key, val in opts.items():
            setattr(o, key, val)
        ctx.set_options(o)
        rng = np.random.default_rng(17)
        u, un = 0.3 * rng.standard_normal(dim * nv), 0.3 * rng.standard_normal(dim * nv)
        ctx.set_state(u_prev=un, p_prev=np.zeros(nv), u=u, p=rng.standard_normal(nv))
        ctx.assemble(True)
        ctx.apply_preconditioner(np.zeros((dim + 1) * nv))     # builds the hierarchies
    return ctx


def right_hand_sides(ctx):
    n = (ctx.dim + 1) * ctx.nv
    out = []
    for seed in (1, 2, 3):
        r = np.random.default_rng(seed).standard_normal(n)
        if ctx.info(76):
            r[ctx.dim * ctx.nv:] -= r[ctx.dim * ctx.nv:].mean()
        out.append(r)
    return out


def slice_widths(M):
    lens = np.diff(M.indptr)
    return np.array([lens[i:i + 64].max() for i in range(0, len(lens), 64)])


def heads(ctx):
    """{operator name: (head width, widths of its slices)} of every operator that has a head"""
    out = {}
    for hier, hn in ((HA, "hA"), (HL, "hL")):
        nlev = int(ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_SHAPE)[0])
        for level in range(nlev):
            for on, op in OPS:
                w = ctx.get_amg_head(hier, level, op)
                if w > 0:
                    out["%s.%d.%s" % (hn, level, on)] = (w, slice_widths(ctx.get_amg_operator(hier, level, op)))
    w = ctx.get_amg_head(HH, 0, _lib.AMG_OP_A)
    if w > 0:
        out["H"] = (w, slice_widths(ctx.get_amg_operator(HH, 0, _lib.AMG_OP_A)))
    return out


_BASE = {}


def baseline(name):
    """z for the seeded right-hand sides with the old addressing: computed once per mesh, never changed"""
    if name not in _BASE:
        ctx = context(name, 0)
        assert heads(ctx) == {}, "CFDH_AMG_HEAD=0 must build no head"
        _BASE[name] = [ctx.apply_preconditioner(r).tobytes() for r in right_hand_sides(ctx)]
        ctx.close()
    return _BASE[name]


def cap(op):
    """what a kernel preloads per row: 8 for the two right-hand sides of the velocity hierarchy, 10 otherwise"""
    return 8 if op.startswith("hA") else 10


def width_by_rule(sw, cap_):
    """head_width_by_rule (csrc/cfdh_amg_dev.hip) restated: the widest head whose padding stays within 1/8 of the entries and which
    7/8 of the slices fit into; 0: none"""
    best = 0
    for w in range(1, cap_ + 1):
        if 8 * int(np.maximum(w - sw, 0).sum()) <= int(sw.sum()) and 8 * int((sw > w).sum()) <= len(sw):
            best = w
    return best


# the SELL-64 operators of each mesh (they must have a head at every forced width); the widths, the widest forced one before the rule's
EXPECT = {
    "dfg64": dict(widths=(1, 2, 10, 0), sell=("hA.0.Sb", "hA.0.Sc", "hL.0.Sb", "hL.0.Sc", "H")),
    # tetrahedra: slices of 15 entries per row and more, the chunked kernel (for three right-hand sides too on this structured mesh)
    "tet26": dict(widths=(1, 2, 10, 0), sell=("hA.0.Sb", "hA.0.Sc", "hL.0.Sb", "hL.0.Sc", "H")),
}


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_preconditioner_with_heads_is_bytewise_the_one_without(name):
    ref = baseline(name)
    both = {}     # operator -> widths at which it had slices with a tail AND slices without
    widths_of = {}
    for width in EXPECT[name]["widths"]:
        ctx = context(name, 1, width)
        try:
            assert ctx.nv % 64 != 0 and ctx.nv >= 16384
            h = heads(ctx)
            if width:
                assert set(h) == set(EXPECT[name]["sell"]), "W=%d: heads %s" % (width, sorted(h))
                widths_of.update({op: sw for op, (_, sw) in h.items()})
            else:     # the rule's decision and width, operator by operator
                want = {op: width_by_rule(sw, cap(op)) for op, sw in widths_of.items()}
                print("%s: widths by the rule %s" % (name, want))
                assert {op: w for op, (w, _) in h.items()} == {op: w for op, w in want.items() if w > 0}
            for op, (w, sw) in sorted(h.items()):
                nt, nn = int((sw > w).sum()), int((sw <= w).sum())
                print("%s W=%d %s: head %d, slice widths %d..%d, %d slices with a tail, %d without" % (name, width, op, w, sw.min(), sw.max(), nt, nn))
                assert not width or w == min(width, cap(op))
                if nt > 0 and nn > 0:
                    both.setdefault(op, []).append(width)
            for r, zb in zip(right_hand_sides(ctx), ref):
                assert ctx.apply_preconditioner(r).tobytes() == zb, "W=%d" % width
        finally:
            ctx.close()
    missing = [op for op in EXPECT[name]["sell"] if op not in both]
    assert not missing, "no width gave %s both slices with a tail and slices without: the comparison proves less than it says" % missing


@pytest.mark.parametrize("name", ["dfg4", "lid", "tet"])
def test_switch_changes_nothing_where_every_level_takes_csr(name):
    ref = baseline(name)
    for width in (1, 0):
        ctx = context(name, 1, width)
        try:
            assert heads(ctx) == {}
            for r, zb in zip(right_hand_sides(ctx), ref):
                assert ctx.apply_preconditioner(r).tobytes() == zb
        finally:
            ctx.close()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _two_ranks(outdir, **extra_env):
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   CFDH_HOST_THREADS="2", **extra_env)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_amg_head_worker.py"), str(outdir)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    deadline = time.monotonic() + 200
    outs = []
    for r, p in enumerate(procs):
        try:
            outs.append(p.communicate(timeout=max(1.0, deadline - time.monotonic()))[0].decode())
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.exit("rank %d did not finish: nothing more is started on the GPU" % r, returncode=1)
    for r, p in enumerate(procs):
        if p.returncode != 0:
            msg = "rank %d failed (exit %d):\n%s" % (r, p.returncode, outs[r][-3000:])
            if p.returncode < 0 or p.returncode in (134, 139):
                pytest.exit(msg + "\nnothing more is started on the GPU", returncode=1)
            pytest.fail(msg)
    return [dict(np.load(os.path.join(outdir, "rank%d.npz" % r))) for r in range(2)]


def test_partitioned_up_sweep_on_the_owned_rows(tmp_path):
    """two ranks of dfg_case(64): the finest up-sweep of the overlapping velocity cycle keeps the first nvo of its nv rows"""
    res = {}
    for head in (0, 1):
        d = tmp_path / ("head%d" % head)
        d.mkdir()
        # width 8, the widest for two right-hand sides: Sc of this mesh has slices on both sides of it, and both operators get a head
        res[head] = _two_ranks(d, CFDH_AMG_HEAD=str(head), CFDH_AMG_HEAD_W="8")
    for a, b in zip(res[0], res[1]):
        assert int(a["head_sb"]) == 0 and int(a["head_sc"]) == 0
        assert int(b["head_sb"]) > 0 and int(b["head_sc"]) > 0, "the velocity hierarchy of a part has no head: nothing is compared"
        assert int(b["ras"]) == 1 and int(b["n0"]) == int(b["nv"]) and int(b["nvo"]) < int(b["nv"]), "up0_rows < n did not occur"
        for key in ("zu0", "zp0", "zu1", "zp1"):
            assert a[key].tobytes() == b[key].tobytes(), key


def test_a_whole_step_is_the_same_step():
    case = dfg_case(64)
    out = {}
    for head in (0, 1):
        with environment(CFDH_AMG_HEAD=head, CFDH_AMG_HEAD_W=None):
            ctx = make_ctx(case, device=0)
        z2, z1 = np.zeros(2 * case.nv), np.zeros(case.nv)
        ctx.set_state(u_prev=z2, p_prev=z1, u=z2, p=z1)
        st = ctx.solve_step()
        h = heads(ctx)
        # the Chebyshev solve of H and the pressure up-sweep (which takes the head kernel when Sb AND Sc have heads) go through heads
        assert ({"H", "hL.0.Sb", "hL.0.Sc"} <= set(h)) if head else h == {}, sorted(h)
        assert st.krylov_its > 0
        u, p = ctx.get_solution()
        out[head] = (st.krylov_its, st.newton_its, u.tobytes(), p.tobytes())
        ctx.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3]
