"""GPU tests of the preconditioner of a PARTITIONED run, operator by operator and stage by stage: the distributed finest pressure level
(k_dl0_down / k_dl0_up), the restricted-additive-Schwarz velocity cycle on owned + ghost vertices and the replicated pressure hierarchy.

Ranks are child processes sharing GPU 0 (tests/_gpu_part_pc_worker.py), as in tests/test_gpu_multirank.py.  Every rank writes what the
getters and cfdh_apply_preconditioner return; this process rebuilds the same partition (parallel.py is deterministic), loads the files
and compares on the CPU: operators bitwise where the library copies, within the fp64 summation bounds of amg_twin.check_operator where it
computes; actions against tests/part_pc_twin.py through amg_twin.gate -- the distance the float32 copies themselves cause, the fp64 floor
where nothing on the way is float32.  The all-reduced coarse right-hand side is summed in the transport's order, so nothing behind it is
compared bitwise with the twin.

P2 / Q1 parts (cfdh_create_elem_part, the element branch of cfdh_set_global_pressure_space) run the same tests on sheared node meshes
(GEN_RUNS), their level-0 operators against tests/cc_gen_twin.py, and their Jacobian and residual against the whole-mesh oracle.  A P2
part builds three hierarchy shapes (test_hierarchy_shapes_of_a_p2_part): the P1 step on the extended part mesh under restricted additive
Schwarz, aggregation of the owned node graph otherwise, aggregation of the global node graph in the replicated pressure hierarchy.

Not covered here: more than 3 ranks in this file, a real RCCL transport (the shared-memory stand-in carries two cases), PCD
(pc_type 2) on parts."""
import os
import socket
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp

import _gpu_part_pc_worker as W
import amg_twin as T
import cc_gen_twin as CG
import part_pc_twin as PT
from amg_checks import COARSE_FACTOR, HA, HH, _assert, _mat, check_h_level, check_hierarchy, fp64_copy, shape_of, twin_hierarchy

from cfd_hemodynamic_amd import _lib
from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HPG, HDL0 = _lib.AMG_HIER_PG, _lib.AMG_HIER_DL0
ALL6 = "2:2,1:2,0:2,2:3,1:3,0:3"

# name -> world, mesh, "schur_full:cc_smooth_degree" configurations, environment of the ranks
RUNS = {
    "dfg16w2": dict(world=2, case="dfg16", configs=ALL6),
    "dfg16w3": dict(world=3, case="dfg16", configs="2:2"),
    "ghostrhs": dict(world=2, case="dfg16", configs="2:2,1:2", env=dict(CFDH_DL0_GHOST_RHS="1", CFDH_RAS_GHOST_RHS="0")),
    "dfg64w2": dict(world=2, case="dfg64", configs="2:2"),
    "dfg64w3": dict(world=3, case="dfg64", configs="2:2"),
    "lid48w3": dict(world=3, case="lid48", configs="2:2,0:2", rccl=True, env=dict(PPC_STEP_FIRST="1")),
    "cube11w2": dict(world=2, case="cube11", configs="2:2,1:2"),
    "layers1": dict(world=2, case="dfg16", configs="2:2", layers=1, env=dict(CFDH_OVERLAP_LAYERS="1")),
    "hostasm": dict(world=3, case="dfg16", configs="2:2", env=dict(CFDH_PC_HOST_ASSEMBLY="1")),
    "sweeps": dict(world=2, case="dfg16", configs="2:2", env=dict(CFDH_DL0_COARSE_SWEEPS="1")),
    # amg_max_coarse at its largest, 4000, above the 2278 vertices of the mesh: the hierarchies have one level, so there is no level 1 to
    # distribute below and the whole pressure cycle runs replicated behind an all-reduce of the right-hand side
    "nodl0": dict(world=2, case="dfg16", configs="2:2,1:2", env=dict(PPC_MAX_COARSE="4000")),
    # ... and behind an all-gather of the owned slices where the communicator speaks the NCCL API
    "nodl0gather": dict(world=2, case="dfg16", configs="2:2", rccl=True, env=dict(PPC_MAX_COARSE="4000")),
    # P2 / Q1 parts on sheared node meshes of a few hundred nodes; amg_max_coarse small enough that the replicated hierarchy has two levels
    # at least, so that the distributed level exists
    "p2tri_w2": dict(world=2, case="p2tri", configs="2:2,1:2,0:2", env=dict(PPC_MAX_COARSE="100", PPC_BDF2="1")),
    "q1quad_w3": dict(world=3, case="q1quad", configs="2:2", rccl=True, env=dict(PPC_MAX_COARSE="16")),
    "p2tet_w2": dict(world=2, case="p2tet", configs="2:2,1:2", env=dict(PPC_MAX_COARSE="50")),
    "q1hex_w2": dict(world=2, case="q1hex", configs="2:2", env=dict(PPC_MAX_COARSE="8")),
}
GEN_RUNS = ["p2tri_w2", "q1quad_w3", "p2tet_w2", "q1hex_w2"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn(world, outdir, timeout=240, **extra_env):
    """One child per rank, all on GPU 0; each under its own communicate(timeout), killed on expiry; the first non-zero exit fails the
    test at once and takes the other ranks (blocked in a collective by then) with it."""
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2",
                   CFDH_HOST_THREADS="2", **extra_env)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "_gpu_part_pc_worker.py"), str(outdir)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    deadline = time.monotonic() + timeout
    pending = set(range(world))

    def stop():
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()

    while pending:
        for r in sorted(pending):
            try:
                o = procs[r].communicate(timeout=0.25)[0].decode()
            except subprocess.TimeoutExpired:
                if time.monotonic() > deadline:
                    stop()
                    pytest.exit("rank %d did not finish within %d s: nothing more is started on the GPU" % (r, timeout), returncode=1)
                continue
            pending.discard(r)
            rc = procs[r].returncode
            if rc != 0:
                stop()
                msg = "rank %d failed (exit %d):\n%s" % (r, rc, o[-3000:])
                if rc < 0 or rc in (134, 139):     # killed by a signal, abort, segmentation fault: the session ends here
                    pytest.exit(msg + "\nnothing more is started on the GPU", returncode=1)
                pytest.fail(msg)
    return [dict(np.load(os.path.join(outdir, "rank%d.npz" % r))) for r in range(world)]


class DumpCtx:
    """The two getters of _lib.Context answered from a rank's file; `pre`: the configuration whose velocity hierarchy and H are meant."""

    def __init__(self, d, pre=""):
        self.d, self.pre = d, pre

    def _key(self, k):
        if self.pre + k in self.d:
            return self.pre + k
        if k in self.d:
            return k
        raise _lib.CfdhError("not in the dump: " + self.pre + k)

    def get_amg_operator(self, hier, level, which, raw=False):
        if hier == HH:
            level = 0
        k = self._key("op_%d_%d_%d_rp" % (hier, level, which))[:-3]
        rp, col, val, shape = self.d[k + "_rp"], self.d[k + "_col"], self.d[k + "_val"], tuple(int(v) for v in self.d[k + "_shape"])
        return (rp, col, val, shape, len(col)) if raw else sp.csr_matrix((val, col, rp), shape=shape)

    def get_amg_vectors(self, hier, level, which):
        if hier == HH or which in (_lib.AMG_VEC_SHAPE, _lib.AMG_VEC_COARSE_INV, _lib.AMG_VEC_SPGEMM_ROWS):
            level = 0
        return self.d[self._key("vec_%d_%d_%d" % (hier, level, which))]


class Run:
    """One finished job: the global problem, the partition rebuilt here, the ranks' files."""

    def __init__(self, name, spec, outdir):
        self.name, self.spec = name, spec
        env = dict(spec.get("env", {}), PPC_CASE=spec["case"], PPC_CONFIGS=spec["configs"])
        if spec.get("rccl"):
            fake = os.path.join(HERE, "fake_rccl", "libfake_rccl.so")
            if not os.path.exists(fake):
                subprocess.check_call(["make", "-C", os.path.join(HERE, "fake_rccl"), "-s"])
            env.update(PPC_BACKEND="rccl", CFDH_RCCL_LIB=fake)
        self.d = _spawn(spec["world"], outdir, **env)
        self.world = spec["world"]
        self.case = W.make_case(spec["case"])
        m = self.case.mesh
        self.dim, self.nvg = m.geometry.dim, m.num_vertices
        # element: None for the P1 contexts, the kind of tests/cc_gen_twin.py for a node mesh of P2 / Q1 cells
        self.generic = spec["case"] in W.GENERIC
        self.kind = CG.kind_of(self.dim, np.asarray(m.cells).shape[1]) if self.generic else None
        self.etype = (1 if self.kind.startswith("P2") else 2) if self.generic else 0
        self.nq = W.GENERIC[spec["case"]][4] if self.generic else 1
        self.owner = partition_vertices_rcb(m.x, self.world)
        self.parts = [LocalPart(m, self.owner, r, layers=spec.get("layers", 2)) for r in range(self.world)]
        for p, d in zip(self.parts, self.d):
            assert (int(d["nvo"]), int(d["nv"])) == (p.nvo, p.nv), "the partition rebuilt here is not the ranks'"
        self.configs = [tuple(int(v) for v in c.split(":")) for c in spec["configs"].split(",")]
        self.pbc_g = np.zeros(self.nvg, dtype=np.uint8)
        for f, nodes, _ in self.case.bcs:
            if f == 1:
                self.pbc_g[nodes] = 1
        self.opt = _lib.Options()
        _lib.lib().cfdh_default_options(self.opt)
        if "PPC_MAX_COARSE" in env:
            self.opt.amg_max_coarse = int(env["PPC_MAX_COARSE"])
        self.dl0_on = int(self.d[0]["dl0_n1"]) > 0
        assert self.dl0_on or not self.generic, "the generic jobs are sized to have a distributed level"
        self._hLg = None
        self._ops = {}

    def cobj(self, r, k=0):
        """What amg_checks asks of a case: ctx, opt, theta, etype, name, singular, pg_singular."""
        p = self.parts[r]      # the mesh a P1 step of this rank's hierarchies interpolates on: the part's own node mesh, ghosts included
        return SimpleNamespace(ctx=DumpCtx(self.d[r], "c%d_" % k), opt=self.opt, theta=0.02 if self.dim == 3 else 0.07, etype=self.etype,
                               name="%s rank %d" % (self.name, r), singular=False, pg_singular=not self.pbc_g.any(), has_pbc=True,
                               dim=self.dim, mesh=SimpleNamespace(x=np.asarray(p.x)[:, : self.dim], cells=p.cells))

    def laplacian(self, x, cells, pbc):
        """(values, bound, terms) of the level-0 operator of a pressure hierarchy on the given mesh: the element's stiffness, Dirichlet rows."""
        x = np.asarray(x)[:, : self.dim]
        return CG.dirichlet_laplacian(self.kind, x, cells, pbc, self.nq) if self.generic else PT.dirichlet_laplacian(x, cells, pbc)

    def lumped_mass(self):
        """(M_l of the whole mesh, tolerance of a part's copy as a multiple of its largest entry): vol / (d + 1) per vertex and the
        16 eps of the one-rank test for P1, the HRZ mass and the derived bound of its scaling factor for the generic elements (the
        factor is one number for every mesh of affine cells of one element, tests/test_cc_gen_twin.py: the part's equals the global one)."""
        m = self.case.mesh
        x = np.asarray(m.x)[:, : self.dim]
        if not self.generic:
            return PT.lumped_mass(x, m.cells), [16 * T.EPS] * self.world
        return CG.lumped_mass(self.kind, x, m.cells), [CG.lumped_mass_tolerance(self.kind, p.cells) for p in self.parts]

    def dl0_shape(self, r):
        s = self.d[r]["vec_%d_0_%d" % (HDL0, _lib.AMG_VEC_DL0_SHAPE)]
        return dict(n1=int(s[0]), ghost_rhs=bool(s[1]), sell_pre=bool(s[2]), sell_post=bool(s[3]), sell_p=bool(s[4]), fused=bool(s[5]),
                    nvo=int(s[6]), nv=int(s[7]))

    def J(self, r):
        d = self.d[r]
        return sp.csr_matrix((d["J_val"], d["J_col"], d["J_rp"]), shape=tuple(int(v) for v in d["J_shape"]))

    def hLg(self):
        if self._hLg is None:
            self._hLg = twin_hierarchy(self.cobj(0), HPG)
        return self._hLg

    def dist_level(self, r):
        ctx = DumpCtx(self.d[r])
        s = self.dl0_shape(r)
        return PT.DistLevel(ctx.get_amg_operator(HDL0, 0, _lib.AMG_OP_A), ctx.get_amg_operator(HDL0, 0, _lib.AMG_OP_P),
                            ctx.get_amg_operator(HDL0, 0, _lib.AMG_OP_PT), ctx.get_amg_vectors(HDL0, 0, _lib.AMG_VEC_WDINV),
                            s["sell_pre"], s["sell_post"], s["sell_p"])

    def rank_ops(self, k):
        """The twin's operators of every rank for configuration k, from the device operators as they are."""
        if k in self._ops:
            return self._ops[k]
        ranks = []
        for r, p in enumerate(self.parts):
            c = self.cobj(r, k)
            R = PT.RankOps()
            R.part, R.dim = p, self.dim
            R.A01, R.A10, _ = PT.jacobian_blocks(self.J(r), self.dim, p.nvo, p.nv)
            R.ras = int(self.d[r]["c%d_ras" % k]) != 0
            R.hA = twin_hierarchy(c, HA)
            assert R.hA.levels[0].n == (p.nv if R.ras else p.nvo)
            Hm = c.ctx.get_amg_operator(HH, 0, _lib.AMG_OP_A)
            lam = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_LAMBDA)
            R.Hlev = T.Level(Hm, ratio=8.0, lm=lam[0] / 1.1)
            R.Hlev.lmax, R.Hlev.lmin = lam
            R.Hlev.w = T.jacobi_weights(R.Hlev.A, R.Hlev.dinv, lam[0], lam[1])
            R.fused_h = Hm.nnz <= 20 * Hm.shape[0] and Hm.shape[0] >= 16384
            R.alpha, R.beta = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_SCALARS)
            R.ml = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_ML)
            R.pbc = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_PBC).astype(np.uint8)
            R.dl0 = self.dist_level(r) if self.dl0_on else None
            ranks.append(R)
        self._ops[k] = ranks
        return ranks

    def gathered(self, k, tag):
        zu, zp = np.zeros((self.nvg, self.dim)), np.zeros(self.nvg)
        sfx = "" if not tag else "_" + tag
        for p, d in zip(self.parts, self.d):
            zu[p.l2g[: p.nvo]], zp[p.l2g[: p.nvo]] = d["c%d_zu%s" % (k, sfx)], d["c%d_zp%s" % (k, sfx)]
        return zu, zp

    def rhs(self, k):
        ru1, ru2, rp1 = W.global_vectors(self.case, self.dim, 100 + k)
        _, _, rp2 = W.global_vectors(self.case, self.dim, 200 + k)
        if self.singular(k):
            rp1, rp2 = rp1 - rp1.mean(), rp2 - rp2.mean()
        return ru1, rp1, ru2, rp2

    def singular(self, k):
        s = {int(d["c%d_singular" % k]) for d in self.d}
        assert len(s) == 1
        return s.pop() != 0


_RUNS = {}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    def get(name):
        if name not in _RUNS:
            try:
                _RUNS[name] = Run(name, RUNS[name], tmp_path_factory.mktemp(name))
            except BaseException as e:     # a job that failed is not started again by the next test that needs it
                _RUNS[name] = e
                raise
        if isinstance(_RUNS[name], BaseException):
            pytest.fail("the job %s failed in an earlier test: %s" % (name, str(_RUNS[name])[:300]))
        return _RUNS[name]
    return get


REPORT = []


def _note(line):
    REPORT.append(line)
    print("[part-pc] " + line)


def _same_csr(a, b):
    a, b = sp.csr_matrix(a), sp.csr_matrix(b)
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(a.data, b.data)


def _raw_of(d, key):
    return d[key + "_rp"], d[key + "_col"], d[key + "_val"], tuple(int(v) for v in d[key + "_shape"]), len(d[key + "_col"])


# ---------------------------------------------------------------------------------------------------------------- operators
OPS_RUNS = ["dfg16w2", "dfg16w3", "lid48w3", "cube11w2", "layers1", "hostasm"] + GEN_RUNS


@pytest.mark.parametrize("name", OPS_RUNS + ["dfg64w2"])
def test_replicated_hierarchy_is_the_same_on_every_rank_and_its_level0_is_the_global_laplacian(runs, name):
    run = runs(name)
    keys = sorted(k for k in run.d[0] if k.startswith(("op_%d_" % HPG, "vec_%d_" % HPG)))
    assert "op_%d_0_%d_val" % (HPG, _lib.AMG_OP_P) in keys and "vec_%d_0_%d" % (HPG, _lib.AMG_VEC_AGG) in keys, \
        "CFDH_AMG_KEEP=1 keeps P and the aggregates of the replicated hierarchy"
    for r in range(1, run.world):
        assert sorted(k for k in run.d[r] if k.startswith(("op_%d_" % HPG, "vec_%d_" % HPG))) == keys
        for k in keys:
            assert np.array_equal(run.d[0][k], run.d[r][k]), "%s differs between rank 0 and rank %d" % (k, r)
    m = run.case.mesh
    v = T.check_operator("%s hLg level 0" % name, _raw_of(run.d[0], "op_%d_0_%d" % (HPG, _lib.AMG_OP_A)), run.laplacian(m.x, m.cells, run.pbc_g))
    _note("%s: hLg level 0 against the global Laplacian: %.3g times the bound" % (name, v.ratio))
    _assert(v)


@pytest.mark.parametrize("name", OPS_RUNS + ["dfg64w2"])
def test_replicated_hierarchy_passes_the_one_rank_checks(runs, name):
    run = runs(name)
    report = []
    try:
        H = check_hierarchy(run.cobj(0), HPG, "hLg", report)
    finally:
        for ln in report:
            _note(ln)
    assert H.singular == (name == "lid48w3") and len(H.levels) >= (3 if name == "dfg64w2" else 2)


@pytest.mark.parametrize("name", OPS_RUNS + ["dfg64w2", "dfg64w3"])
def test_distributed_level_is_cut_out_of_the_replicated_level0(runs, name):
    """dl0.A / dl0.P / dl0.wdinv are copies of rows of level 0 by global id, dl0.PT the transposed owned rows of dl0.P with a fixed
    summation order; over the ranks every row of P is restricted exactly once."""
    run = runs(name)
    c0 = DumpCtx(run.d[0])
    A0, P0 = c0.get_amg_operator(HPG, 0, _lib.AMG_OP_A), c0.get_amg_operator(HPG, 0, _lib.AMG_OP_P)
    w0 = c0.get_amg_vectors(HPG, 0, _lib.AMG_VEC_WDINV)
    assert np.array_equal(c0.get_amg_vectors(HPG, 0, _lib.AMG_VEC_ORDER), np.arange(run.nvg)), "the global pressure space is not renumbered"
    tr, tc, tv = [], [], []
    for r, p in enumerate(run.parts):
        d = run.d[r]
        s = run.dl0_shape(r)
        assert (s["n1"], s["nvo"], s["nv"]) == (P0.shape[1], p.nvo, p.nv) and int(d["dl0_n1"]) == P0.shape[1]
        tw = PT.cut_dist_level(A0, P0, w0, p)
        for nm, which, ref in (("A", _lib.AMG_OP_A, tw.A), ("P", _lib.AMG_OP_P, tw.P)):
            raw = _raw_of(d, "op_%d_0_%d" % (HDL0, which))
            _assert(T.check_csr("%s rank %d dl0.%s" % (name, r, nm), raw[0], raw[1], raw[3], raw[4]))
            assert _same_csr(_mat(raw), ref), "%s rank %d: dl0.%s is not the rows of level 0" % (name, r, nm)
        assert np.array_equal(d["vec_%d_0_%d" % (HDL0, _lib.AMG_VEC_WDINV)], w0[p.l2g])
        # PT: coarse rows, owned columns in the caller's numbering, stored in the order they are summed in: ascending in the library's own
        rp, col, val, shape, nnz = _raw_of(d, "op_%d_0_%d" % (HDL0, _lib.AMG_OP_PT))
        assert shape == (P0.shape[1], p.nvo) and col.min() >= 0 and col.max() < p.nvo
        order = d["vec_%d_0_%d" % (HDL0, _lib.AMG_VEC_ORDER)].astype(np.int64)
        assert np.array_equal(np.sort(order[: p.nvo]), np.arange(p.nvo)) and np.array_equal(order[p.nvo:], np.arange(p.nvo, p.nv))
        inner = order[col]
        rows = np.repeat(np.arange(shape[0]), np.diff(rp))
        same = rows[1:] == rows[:-1]
        assert (inner[1:][same] > inner[:-1][same]).all(), "%s rank %d: dl0.PT is not summed in ascending owned order" % (name, r)
        PTm = sp.csr_matrix((val, col, rp), shape=shape)
        assert _same_csr(T.canonical(PTm), tw.PT), "%s rank %d: dl0.PT is not the transpose of the owned rows of dl0.P" % (name, r)
        tr.append(p.l2g[col]), tc.append(rows), tv.append(val)
    tr, tc, tv = np.concatenate(tr), np.concatenate(tc), np.concatenate(tv)
    assert len(tv) == P0.nnz, "%s: %d entries restricted over the ranks, P holds %d" % (name, len(tv), P0.nnz)
    total = sp.coo_matrix((tv, (tr, tc)), shape=P0.shape).tocsr()      # (explicit zeros of P stay)
    assert _same_csr(T.canonical(total), T.canonical(P0)), "%s: the restrictions of the ranks do not add up to P^T once per row" % name


def _global_proxy(run, k=0):
    """The proxy of the whole mesh assembled from the owned rows every rank holds (level 0 of its velocity hierarchy)."""
    gr, gc, gv = [], [], []
    for r, p in enumerate(run.parts):
        C = DumpCtx(run.d[r], "c%d_" % k).get_amg_operator(HA, 0, _lib.AMG_OP_A)[: p.nvo].tocoo()
        gr.append(p.l2g[C.row]), gc.append(p.l2g[C.col]), gv.append(C.data)
    return sp.coo_matrix((np.concatenate(gv), (np.concatenate(gr), np.concatenate(gc))), shape=(run.nvg, run.nvg)).tocsr()


def _check_single_level(c, hier, label):
    """A hierarchy whose level 0 is already the coarsest: the level quantities and the dense inverse, as check_hierarchy takes them."""
    ctx = c.ctx
    sh = shape_of(ctx, hier)
    assert sh["nl"] == 1 and sh["coarse_n"] == sh["lev"][0]["n"]
    A = _mat(ctx.get_amg_operator(hier, 0, _lib.AMG_OP_A, raw=True))
    lam = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_LAMBDA)
    L = T.Level(A, ratio=c.opt.amg_smooth_ratio, lm=lam[0] / 1.1)
    L.lmax, L.lmin = lam
    L.w = T.jacobi_weights(L.A, L.dinv, lam[0], lam[1])
    order = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_ORDER)
    _assert(T.check_lmax("%s %s" % (c.name, label), lam[0], lam[1], L, c.opt.amg_smooth_ratio, order))
    _assert(T.check_weights("%s %s" % (c.name, label), ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_DINV), ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_WDINV), L))
    n = sh["coarse_n"]
    X = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_COARSE_INV).reshape(n, n)
    sing = hier == HPG and c.pg_singular
    res = (T.coarse_residual(L.A, np.linalg.inv(T.coarse_matrix(L.A, sing)), sing), T.coarse_residual(L.A, X, sing))
    _note("%s %s: one level of %d rows; coarse inverse residual numpy %.3g device %.3g" % (c.name, label, n, res[0], res[1]))
    assert res[1] <= COARSE_FACTOR * res[0]


@pytest.mark.parametrize("name", OPS_RUNS + ["dfg64w2"])
def test_velocity_proxy_on_owned_and_ghost_rows(runs, name):
    run = runs(name)
    G = _global_proxy(run)
    for r, p in enumerate(run.parts):
        c = run.cobj(r)
        assert int(run.d[r]["c0_ras"]) == 1
        raw = c.ctx.get_amg_operator(HA, 0, _lib.AMG_OP_A, raw=True)
        _assert(T.check_csr("%s rank %d proxy" % (name, r), raw[0], raw[1], raw[3], raw[4]))
        A = _mat(raw)
        assert A.shape == (p.nv, p.nv)
        # owned rows: the one-rank formula on this rank's Jacobian
        tw = PT.proxy_rows(run.J(r), run.dim, p.nvo, p.nv)
        own = A[: p.nvo].tocsr()
        v = T.check_operator("%s rank %d proxy, owned rows" % (name, r), T.raw_csr(own), tw)
        _note("%s rank %d: owned rows of the proxy %.3g times the bound" % (name, r, v.ratio))
        _assert(v)
        # ghost rows: the owner's row restricted to this rank's columns; the whole matrix: the principal submatrix of the global proxy
        ref = T.canonical(G[p.l2g][:, p.l2g])
        gh = T.canonical(A[p.nvo:])
        assert _same_csr(gh, T.canonical(ref[p.nvo:])), "%s rank %d: a ghost row is not its owner's row on the local columns" % (name, r)
        assert _same_csr(T.canonical(A), ref), "%s rank %d: the extended proxy is not the principal submatrix of the global one" % (name, r)
        assert gh.nnz > p.ng, "ghost rows with neighbours"
    # the levels above, rank by rank
    for r in range(run.world):
        c = run.cobj(r)
        sh = shape_of(c.ctx, HA)
        if sh["nl"] == 1:
            _check_single_level(c, HA, "hA")     # a part of no more than amg_max_coarse local vertices: the dense inverse alone
            continue
        report = []
        try:
            check_hierarchy(c, HA, "hA", report)
        finally:
            for ln in report:
                _note(ln)
        if run.etype == 1:     # a P2 part: the P1 step of the extended part mesh, which check_hierarchy compared with the exact interpolation
            assert not sh["lev"][0]["agg"] and sh["lev"][0]["n"] == run.parts[r].nv
            continue
        agg = run.d[r]["c0_vec_%d_0_%d" % (HA, _lib.AMG_VEC_AGG)]
        assert len(agg) == run.parts[r].nv, "CFDH_AMG_KEEP=1 keeps the aggregates of the overlapping hierarchy"


@pytest.mark.parametrize("name", OPS_RUNS + ["dfg64w2"])
def test_h_lumped_mass_and_flags_of_a_part(runs, name):
    run = runs(name)
    ml_g, tols = run.lumped_mass()
    for r, p in enumerate(run.parts):
        c = run.cobj(r)
        pbc = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_PBC)
        assert np.array_equal(pbc, run.pbc_g[p.l2g[: p.nvo]].astype(np.float64))
        mld = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_ML)
        ref = ml_g[p.l2g[: p.nvo]]
        err = np.abs(mld - ref)[pbc == 0].max() / ml_g.max()
        _note("%s rank %d: lumped mass %.3g eps of the largest entry, allowed %.3g eps" % (name, r, err / T.EPS, tols[r] / T.EPS))
        assert (mld[pbc != 0] == 0.0).all() and err <= tols[r]
        alpha, beta = c.ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_CC_SCALARS)
        assert alpha == run.case.rho * 1.0 / (0.5 * run.case.dt) and beta == run.case.mu
        # H on the local operators with the ghost columns removed
        _, _, A11 = PT.jacobian_blocks(run.J(r), run.dim, p.nvo, p.nv)
        Lp, _, terms = run.laplacian(p.x, p.cells, np.zeros(p.nv))
        Lp = T.canonical(Lp[: p.nvo, : p.nvo])
        # generic elements (as in tests/test_gpu_amg.py): H from the device's own lumped mass where it is stored, and T = diag(A11) / diag(L)
        # carries the relative error of a sum of `terms` positive products on top of the 4 x 4 eps of the P1 contexts
        mlh, depth = (np.where(pbc == 0, mld, ref), 4 + (terms + 3) // 4) if run.generic else (ref, 4)
        Hm, Hb = T.h_operator(T.canonical(A11[:, : p.nvo]), Lp, mlh, pbc, alpha, beta)
        v = T.check_operator("%s rank %d H" % (name, r), c.ctx.get_amg_operator(HH, 0, _lib.AMG_OP_A, raw=True), (Hm, Hb, depth))
        _note("%s rank %d: H %.3g times the bound" % (name, r, v.ratio))
        _assert(v)
        check_h_level(c)


def test_sell_is_taken_from_16384_owned_rows_up(runs):
    """dfg_case(64): 34775 vertices.  Two parts own >= 16384 rows each: SELL in the three sweeps of the distributed level and fine / sell on
    level 0 of the overlapping hierarchy; three parts stay below: CSR."""
    two, three = runs("dfg64w2"), runs("dfg64w3")
    assert two.nvg == 34775
    for r, p in enumerate(two.parts):
        s = two.dl0_shape(r)
        assert p.nvo >= 16384 and s["sell_pre"] and s["sell_post"] and s["sell_p"], (r, p.nvo, s)
        lev0 = shape_of(two.cobj(r).ctx, HA)["lev"][0]
        assert lev0["n"] == p.nv and lev0["fine"] and lev0["sell"]
    for r, p in enumerate(three.parts):
        s = three.dl0_shape(r)
        assert p.nv < 16384 and not (s["sell_pre"] or s["sell_post"] or s["sell_p"]), (r, p.nv, s)
        lev0 = shape_of(three.cobj(r).ctx, HA)["lev"][0]
        assert not lev0["fine"] and not lev0["sell"]
    for name, run in (("dfg64w2", two), ("dfg64w3", three)):
        _note("%s: owned %s local %s; distributed level %s" % (name, [p.nvo for p in run.parts], [p.nv for p in run.parts],
                                                                 ["SELL" if run.dl0_shape(r)["sell_pre"] else "CSR" for r in range(run.world)]))


def test_branches_taken_by_the_small_cases(runs):
    for name in ("dfg16w2", "dfg16w3", "lid48w3", "cube11w2", "sweeps", "ghostrhs"):
        run = runs(name)
        for r in range(run.world):
            s = run.dl0_shape(r)
            assert not (s["sell_pre"] or s["sell_post"] or s["sell_p"])
            assert s["fused"] == (name != "sweeps") and s["ghost_rhs"] == (name == "ghostrhs")
    for name, gather in (("nodl0", False), ("nodl0gather", True)):
        no = runs(name)
        assert not no.dl0_on and all(shape_of(no.cobj(r).ctx, h)["nl"] == 1 for r in range(2) for h in (HA, HPG))
        # the right-hand side of the replicated cycle: all-reduced, or (NCCL API) the owned slices all-gathered, padded to the largest part
        assert all((int(d["allgather"]) == max(p.nvo for p in no.parts)) if gather else (int(d["allgather"]) == 0) for d in no.d), name
        assert all(int(d["rccl"]) == (1 if gather else 0) for d in no.d)
    lid = runs("lid48w3")
    assert all(str(d["backend"]) == "rccl" and int(d["rccl"]) == 1 for d in lid.d), "the in-stream all-reduce is the one under test"
    assert lid.singular(0) and not lid.pbc_g.any()


@pytest.mark.parametrize("name", ["p2tri_w2", "p2tet_w2"])
def test_hierarchy_shapes_of_a_p2_part(runs, name):
    """One P2 context builds three hierarchy shapes.  The P1 subspace of a part (gen_P1) has one row per LOCAL node, ghosts included, and the
    device build takes the p-multigrid step only where the level-0 operator has exactly those rows:
      hA, schur_full 2   owned + ghost rows (restricted additive Schwarz): the exact P1 interpolation of the extended part mesh, then aggregation
      hA, schur_full 1, 0   owned rows: aggregation of the owned node graph from level 0 on
      hLg   the nodes of the whole mesh: aggregation from level 0 on, so the distributed level's P is rows of a smoothed-aggregation prolongator
    (on one rank all of them take the P1 step, tests/test_gpu_amg.py)."""
    run = runs(name)
    assert run.etype == 1 and run.dl0_on
    if name == "p2tet_w2":
        # the overlap of rank 0 reaches every node of the mesh, so its local P1 subspace has as many rows as the GLOBAL operator: the
        # row count alone must not make hLg take the (locally numbered) P1 step on that rank -- the ranks then disagree on the coarse size
        # and the all-reduce of the coarse right-hand side aborts
        assert run.parts[0].nv == run.nvg > run.parts[1].nv
    for k, (sf, _) in enumerate(run.configs):
        for r, p in enumerate(run.parts):
            c = run.cobj(r, k)
            sh = shape_of(c.ctx, HA)
            lev0 = sh["lev"][0]
            assert int(run.d[r]["c%d_ras" % k]) == (1 if sf == 2 else 0)
            if sf == 2:
                nvert = len(np.unique(np.asarray(p.cells)[:, : run.dim + 1]))
                assert lev0["n"] == p.nv and not lev0["agg"] and sh["nl"] >= 2 and sh["lev"][1]["n"] == nvert, (name, k, r, sh["lev"])
            else:
                assert lev0["n"] == p.nvo and lev0["agg"] and sh["nl"] >= 2, (name, k, r, sh["lev"])
                report = []
                try:
                    check_hierarchy(c, HA, "hA (schur_full %d)" % sf, report)      # level 0 by the aggregation formulas
                finally:
                    for ln in report:
                        _note(ln)
            _note("%s rank %d schur_full %d: hA levels %s, level 0 %s" % (name, r, sf, [q["n"] for q in sh["lev"]],
                                                                          "aggregated" if lev0["agg"] else "P1 step"))
    sh = shape_of(run.cobj(0).ctx, HPG)
    nvert_g = len(np.unique(np.asarray(run.case.mesh.cells)[:, : run.dim + 1]))
    assert sh["lev"][0]["n"] == run.nvg and sh["lev"][0]["agg"] and sh["lev"][1]["n"] != nvert_g
    agg = run.d[0]["vec_%d_0_%d" % (HPG, _lib.AMG_VEC_AGG)]
    assert len(agg) == run.nvg and agg.max() + 1 == sh["lev"][1]["n"] == run.dl0_shape(0)["n1"]
    _note("%s: hLg levels %s, level 0 aggregated (%d vertices in the mesh)" % (name, [q["n"] for q in sh["lev"]], nvert_g))


def test_q1_parts_aggregate_everywhere(runs):
    for name in ("q1quad_w3", "q1hex_w2"):
        run = runs(name)
        assert run.etype == 2 and run.dl0_on
        for r, p in enumerate(run.parts):
            sh = shape_of(run.cobj(r).ctx, HA)
            assert sh["lev"][0]["n"] == p.nv and (sh["nl"] == 1 or sh["lev"][0]["agg"])
        sh = shape_of(run.cobj(0).ctx, HPG)
        assert sh["nl"] >= 2 and sh["lev"][0]["agg"]
    q = runs("q1quad_w3")
    assert all(str(d["backend"]) == "rccl" and int(d["rccl"]) == 1 for d in q.d), "the in-stream all-reduce carries the Q1 parts"


# ---------------------------------------------------------------------------------------------------------------- Jacobian and residual of a generic part
def _whole_mesh_assembly(run, bdf2):
    """Residual and Jacobian of the whole node mesh by the oracle (oracle/np_twin_gen.py, np_twin_gen3.py): the worker's global state and
    Dirichlet data."""
    import gen3_util
    import gen_util
    case, d, m = run.case, run.dim, run.case.mesh
    mod, make = (gen_util.G, gen_util.problem) if d == 2 else (gen3_util.G3, gen3_util.problem3)
    kw = dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5) if bdf2 else {}
    pb = make(run.kind[:2], m, mod.Params(case.dt, case.rho, case.mu, np.asarray(case.f, dtype=np.float64)[:d], **kw))
    for f, nodes, vals in case.bcs:
        (pb.add_bc_u if f == 0 else pb.add_bc_p)(nodes, vals)
    u, un, p = W.global_vectors(case, d, 17)
    un2, _, _ = W.global_vectors(case, d, 18)
    return pb.assemble(np.concatenate([0.3 * u.ravel(), p]), 0.3 * un, un2=0.3 * un2 if bdf2 else None)


@pytest.mark.parametrize("name,bdf2", [(n, False) for n in GEN_RUNS] + [("p2tri_w2", True)])
def test_jacobian_and_residual_of_a_generic_part(runs, monkeypatch, name, bdf2):
    """A wrong Jacobian on a part is invisible to the end-to-end runs (Newton converges on the residual alone, FGMRES with any nonsingular
    preconditioner): every rank's owned rows of cfdh_get_csr / cfdh_get_residual, mapped to global ids, against the whole-mesh oracle to the
    tolerance one rank is held to (tests/test_gpu_gen.py, tests/test_gpu_gen3.py: 1e-12 of the largest entry).  bdf2: BDF2 coefficients
    and a second history vector, whose ghost values the kernels read as well."""
    from oracle import np_twin_gen, np_twin_gen3, orcg, orcg3
    monkeypatch.setattr(np_twin_gen, "element_tensors", orcg.element_tensors)       # the oracle assembles with its C restatement, as in the
    monkeypatch.setattr(np_twin_gen3, "element_tensors", orcg3.element_tensors)     # one-rank tests
    run = runs(name)
    d, nvg = run.dim, run.nvg
    F, J = _whole_mesh_assembly(run, bdf2)
    tag = "2" if bdf2 else ""
    rows_seen = np.zeros((d + 1) * nvg, dtype=np.int64)
    gr, gc, gv = [], [], []
    Fg = np.zeros((d + 1) * nvg)
    for r, p in enumerate(run.parts):
        dd = run.d[r]
        Jr = sp.csr_matrix((dd["J%s_val" % tag], dd["J%s_col" % tag], dd["J%s_rp" % tag]), shape=tuple(int(v) for v in dd["J%s_shape" % tag]))
        assert Jr.shape == ((d + 1) * p.nvo, (d + 1) * p.nv)
        l2g = np.asarray(p.l2g, dtype=np.int64)
        rmap = np.concatenate([(d * l2g[: p.nvo, None] + np.arange(d)).ravel(), d * nvg + l2g[: p.nvo]])
        cmap = np.concatenate([(d * l2g[:, None] + np.arange(d)).ravel(), d * nvg + l2g])
        rows_seen[rmap] += 1
        C = Jr.tocoo()
        gr.append(rmap[C.row]), gc.append(cmap[C.col]), gv.append(C.data)
        ghost = np.concatenate([np.arange(d * p.nvo, d * p.nv), np.arange(d * p.nv + p.nvo, (d + 1) * p.nv)])
        assert abs(Jr[:, ghost]).sum() > 0, "rank %d: no ghost column in an owned row" % r
        Fg[rmap] = np.concatenate([dd["F%s_u" % tag].ravel(), dd["F%s_p" % tag]])
    assert (rows_seen == 1).all(), "every global row is owned by exactly one rank"
    Jg = sp.coo_matrix((np.concatenate(gv), (np.concatenate(gr), np.concatenate(gc))), shape=J.shape).tocsr()
    eF, eJ = np.abs(Fg - F).max() / np.abs(F).max(), abs(Jg - J).max() / abs(J).max()
    _note("%s%s: residual %.3g, Jacobian %.3g of the largest entry (allowed 1e-12)" % (name, " BDF2" if bdf2 else "", eF, eJ))
    assert eF <= 1e-12 and eJ <= 1e-12
    if bdf2:     # the variant is another matrix: the time-scheme coefficients reached the assembly
        F1, J1 = _whole_mesh_assembly(run, False)
        assert abs(J1 - J).max() > 1e-3 * abs(J).max()


# ---------------------------------------------------------------------------------------------------------------- actions
def _dev(H, b):
    return T.vcycle_composite(H, b, "device")


def _f64(H, b):
    return T.vcycle_composite(H, b, "fp64")


def _fp64_ranks(ranks):
    out = []
    for R in ranks:
        Q = PT.RankOps()
        Q.__dict__.update(R.__dict__)
        Q.hA = fp64_copy(R.hA)
        out.append(Q)
    return out


def _flags(run):
    env = run.spec.get("env", {})
    return dict(dl0_ghost_rhs=env.get("CFDH_DL0_GHOST_RHS") == "1", ras_ghost_rhs=env.get("CFDH_RAS_GHOST_RHS") != "0",
                coarse_fused=env.get("CFDH_DL0_COARSE_SWEEPS") != "1")


def _any_float32(run, k):
    """Does the whole action of configuration k pass through anything the device stores in float32?  The one-pass smoother on H, the
    SELL copies of the distributed level, the composite operators / the folded dense correction of the hierarchies as they are applied
    (the replicated one from level 1 on below a distributed level 0; a hierarchy of one level through its fp64 dense inverse)."""
    sf, _ = run.configs[k]
    ranks, hLg = run.rank_ops(k), run.hLg()

    def h32(H, l0=0):
        return len(H.levels) - l0 >= 2 and any(L.fine or L.sell or L.D is not None for L in H.levels[l0:])

    if any(R.fused_h and run.configs[k][1] == 2 for R in ranks) or any(h32(R.hA) for R in ranks):
        return True
    if run.dl0_on:
        return h32(hLg, 1) or any(R.dl0.sell_pre or R.dl0.sell_post or R.dl0.sell_p for R in ranks)
    return h32(hLg)


def _gate(run, k, tag, ru, rp, part, label):
    """One application of all ranks against the twin with device storage; part: "u", "p" or "all" of the gathered result."""
    sf, deg = run.configs[k]
    ranks, hLg = run.rank_ops(k), run.hLg()
    sing = run.singular(k)
    fl = _flags(run)
    zu, zp = run.gathered(k, tag)
    tr = PT.action(ranks, hLg, ru, rp, sf, deg, sing, _dev, "device", **fl)
    t64 = PT.action(_fp64_ranks(ranks), fp64_copy(hLg), ru, rp, sf, deg, sing, _f64, "fp64", **fl)
    cu, cp, kk = PT.action_bound(_fp64_ranks(ranks), fp64_copy(hLg), ru, rp, sf, deg)

    def pick(u, p):
        return u.ravel() if part == "u" else p if part == "p" else np.concatenate([u.ravel(), p])

    dist, d32, allowed, floor = T.gate(pick(zu, zp), pick(*tr), pick(*t64), (pick(cu, cp), kk))
    _note("%s %s (schur_full %d, degree %d): delta32 %.3g, device distance %.3g, allowed %.3g (fp64 floor %.3g), ratio %.3g"
          % (run.name, label, sf, deg, d32, dist, allowed, floor, dist / allowed if allowed > 0 else np.inf))
    if part == "all":     # the fp64 floor may stand in for 0.01 delta32 only where nothing on the way is float32
        assert d32 > 0.0 or not _any_float32(run, k), "float32 storage on the way and delta32 = 0: " + REPORT[-1]
    assert dist <= allowed, REPORT[-1]
    return (zu, zp), tr


ACTION_RUNS = ["dfg16w2", "dfg16w3", "ghostrhs", "dfg64w2", "dfg64w3", "lid48w3", "cube11w2", "layers1", "hostasm", "sweeps", "nodl0", "nodl0gather"] + GEN_RUNS


@pytest.mark.parametrize("name", ACTION_RUNS)
def test_velocity_cycle_alone(runs, name):
    """r_p = 0 with the upper factor: z_p = 0 and z_u is the owned part of one cycle of the rank's extended hierarchy on the global r_u
    (without the overlap residual's exchange: on r_u with zeros on the ghosts)."""
    run = runs(name)
    assert run.configs[0][0] == 2
    ru, rp, _, _ = run.rhs(0)
    (zu, zp), _ = _gate(run, 0, "vel", ru, 0.0 * rp, "u", "velocity cycle")
    assert not zp.any()
    fl = _flags(run)
    for R, p in zip(run.rank_ops(0), run.parts):
        b = ru[p.l2g].copy()
        if not fl["ras_ghost_rhs"]:
            b[p.nvo:] = 0.0
        assert T.rel_distance(zu[p.l2g[: p.nvo]], _dev(R.hA, b)[: p.nvo]) <= 1e-6     # it is that cycle which the gate compared


@pytest.mark.parametrize("name", ACTION_RUNS)
def test_pressure_branch_alone(runs, name):
    run = runs(name)
    ru, rp, _, _ = run.rhs(0)
    (zu, zp), (tu, tp) = _gate(run, 0, "pres", 0.0 * ru, rp, "p", "pressure branch")
    if name != "ghostrhs":
        return
    # With the right-hand side present on the ghosts the pressure cycle is the cycle of the whole mesh: stated without any partition
    # (the rank's H, whose ghost columns are dropped, is the only rank-local ingredient).
    ranks, hLg = run.rank_ops(0), run.hLg()
    zH = [T.chebyshev(R.Hlev, rp[p.l2g[: p.nvo]], 2) for R, p in zip(ranks, run.parts)]
    y = PT._gather(ranks, [R.ml * z for R, z in zip(ranks, zH)], run.nvg)
    zH_g = PT._gather(ranks, zH, run.nvg)
    al, be = ranks[0].alpha, ranks[0].beta
    ref = {s: np.where(run.pbc_g != 0, rp, al * PT.global_cycle_level0_sweeps(q, y, s) + be * zH_g)
           for s, q in (("device", hLg), ("fp64", fp64_copy(hLg)))}
    c, kk = PT.sweeps_bound(hLg, np.abs(y))
    dist, d32, allowed, floor = T.gate(zp, ref["device"], ref["fp64"], (al * c + be * np.abs(zH_g), kk))
    _note("%s pressure branch against the cycle of the whole mesh: delta32 %.3g, device distance %.3g, allowed %.3g" % (name, d32, dist, allowed))
    assert dist <= allowed, REPORT[-1]


@pytest.mark.parametrize("name,k", [(n, k) for n in ACTION_RUNS for k in range(len(RUNS[n]["configs"].split(",")))])
def test_whole_action_and_its_invariants(runs, name, k):
    run = runs(name)
    ru1, rp1, ru2, rp2 = run.rhs(k)
    (zu, zp), _ = _gate(run, k, "", ru1, rp1, "all", "whole action")
    # a second application replays the captured graphs: bitwise
    zu_a, zp_a = run.gathered(k, "again")
    assert np.array_equal(zu_a, zu) and np.array_equal(zp_a, zp)
    # every ghost value that is used came through a halo exchange: garbage on the ghosts of the caller's r changes nothing
    zu_g, zp_g = run.gathered(k, "garbage")
    assert np.array_equal(zu_g, zu) and np.array_equal(zp_g, zp)
    # linear in r
    zu2, zp2 = run.gathered(k, "2")
    zul, zpl = run.gathered(k, "lin")
    z, zl = np.concatenate([zu.ravel(), zp]), np.concatenate([zul.ravel(), zpl])
    z2 = np.concatenate([zu2.ravel(), zp2])
    assert T.rel_distance(zl, 0.7 * z - 1.3 * z2) <= 1e-10


def test_a_step_after_getter_calls_is_bitwise_the_step_without_them(tmp_path):
    a = _spawn(2, tmp_path, PPC_CASE="dfg16", PPC_MODE="step", PPC_GETTERS="1")
    b = _spawn(2, tmp_path, PPC_CASE="dfg16", PPC_MODE="step", PPC_GETTERS="0")
    for r in range(2):
        assert "op_%d_0_%d_val" % (HPG, _lib.AMG_OP_A) in a[r] and "op_%d_0_%d_val" % (HPG, _lib.AMG_OP_A) not in b[r]
        assert int(a[r]["krylov"]) == int(b[r]["krylov"]) > 0 and int(a[r]["newton"]) == int(b[r]["newton"])
        assert np.array_equal(a[r]["u"], b[r]["u"]) and np.array_equal(a[r]["p"], b[r]["p"])
