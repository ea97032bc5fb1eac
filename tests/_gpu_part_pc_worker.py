"""Worker of tests/test_gpu_part_pc.py: one rank of an N-process job whose ranks share GPU 0.  Builds its part through the ordinary solver
plug-in, sets a random state taken from global arrays (so that all ranks agree), assembles, builds the preconditioner with
CFDH_AMG_KEEP=1 and writes what cfdh_get_amg_operator / cfdh_get_amg_vectors / cfdh_apply_preconditioner return to one .npz per rank.
All comparisons happen in the parent, on the CPU.

Environment: PPC_CASE (dfg16, dfg64, lid48, cube11: the mesh; p2tri, q1quad, p2tet, q1hex: a sheared node mesh of a generic element, whose
part goes through cfdh_create_elem_part and cfdh_set_global_pressure_space's element branch), PPC_BACKEND (host | rccl), PPC_CONFIGS ("schur_full:degree,..." applied in
turn, each with its own dump of the velocity hierarchy and of H), PPC_MAX_COARSE (amg_max_coarse),
PPC_STEP_FIRST=1 (one time step before the random state: the singular-pressure flag is set by the Newton solver), PPC_MODE=step (one
time step from the start state after -- or, with PPC_GETTERS=0, without -- the getter calls; the solution is the output),
PPC_BDF2=1 (after everything else: the Jacobian and residual of the same state with BDF2 coefficients and a second history vector)."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cfd_hemodynamic_amd import _lib  # noqa: E402
from cfd_hemodynamic_amd.fem import DirichletBC, Function  # noqa: E402
from cfd_hemodynamic_amd.parallel import PartComm  # noqa: E402

HA, HH, HPG, HDL0 = _lib.AMG_HIER_A, _lib.AMG_HIER_H, _lib.AMG_HIER_PG, _lib.AMG_HIER_DL0
OPS5 = (_lib.AMG_OP_A, _lib.AMG_OP_P, _lib.AMG_OP_G, _lib.AMG_OP_SB, _lib.AMG_OP_SC)
LEVEL_VECS = (_lib.AMG_VEC_DINV, _lib.AMG_VEC_WDINV, _lib.AMG_VEC_AGG, _lib.AMG_VEC_D, _lib.AMG_VEC_LAMBDA, _lib.AMG_VEC_ORDER)


def make_case(name):
    """The global problem (mesh, Dirichlet data, parameters) by name; the parent calls this too."""
    from util import Case, dfg_case, lid_case
    if name.startswith("dfg"):
        return dfg_case(int(name[3:]))
    if name.startswith("lid"):
        return lid_case(int(name[3:]))
    if name.startswith("cube"):
        from cfd_hemodynamic_amd.mesh3d import create_unit_cube
        m = create_unit_cube(int(name[4:]))     # n cells per edge: (n + 1)^3 vertices
        bnd = np.nonzero((np.abs(m.x - 0.5).max(axis=1) > 0.5 - 1e-12))[0].astype(np.int32)
        out = bnd[np.isclose(m.x[bnd, 0], 1.0)]
        wall = np.setdiff1d(bnd, out).astype(np.int32)
        return Case(m, [(0, wall, np.zeros((len(wall), 3))), (1, out, np.zeros(len(out)))], 0.01, 1.0, 1e-2, f=(0.0, 0.0, 0.0))
    if name in GENERIC:
        return generic_case(name)
    raise KeyError(name)


# P2 / Q1 parts: node-mesh builder (gen_util / gen3_util), element, cells per edge, shear, quadrature points per cell of the library's element
# stiffness (the length of its sums, for the bounds of the parent).  The meshes of the generic cases of tests/test_gpu_amg.py.
GENERIC = {"p2tri": ("node_mesh", "P2", 12, 0.2, 49), "q1quad": ("node_mesh", "Q1", 16, 0.3, 49),
           "p2tet": ("node_mesh3", "P2", 4, 0.25, 171), "q1hex": ("node_mesh3", "Q1", 6, 0.3, 343)}


def generic_case(name):
    """Sheared node mesh of a generic element (a transposed or mis-indexed inverse cell Jacobian changes its matrices) with no-slip walls
    and a pressure-Dirichlet outlet (the face x = 1 before the shear), like `cube`.  case.mesh is the NODE mesh -- what is partitioned,
    what the global vectors live on; case.solver_mesh / case.degree are what the plug-in is given: the geometric mesh with _degree=2 for
    P2, the quadrilateral / hexahedral mesh itself for Q1."""
    from util import Case
    import gen3_util
    import gen_util
    mk, kind, n, distort, _ = GENERIC[name]
    mk = getattr(gen_util if mk == "node_mesh" else gen3_util, mk)
    m, flat = mk(kind, n, distort), mk(kind, n, 0.0)
    d = m.x.shape[1]
    bnd = np.unique(m.facet_vertices).astype(np.int32)
    out = bnd[np.isclose(flat.x[bnd, 0], flat.x[:, 0].max())]
    wall = np.setdiff1d(bnd, out).astype(np.int32)
    case = Case(m, [(0, wall, np.zeros((len(wall), d))), (1, out, np.zeros(len(out)))], 0.01, 1.0, 1e-2, f=(0.0,) * d)
    case.degree = 2 if kind == "P2" else 1
    case.solver_mesh = m.base if kind == "P2" else m
    if kind == "P2":
        m.base._p2_nodes = m     # the plug-in's function spaces live on this very node mesh
    return case


def global_vectors(case, dim, seed):
    """(u, u_prev, p) or right-hand sides (r_u [nv, dim], r_p [nv]) of the whole mesh from one seed."""
    rng = np.random.default_rng(seed)
    nv = case.mesh.num_vertices
    return rng.standard_normal((nv, dim)), rng.standard_normal((nv, dim)), rng.standard_normal(nv)


class _FixedBC:
    """What Solver.setup asks of a boundary condition: getBC(V) -> DirichletBC with the given values at the given vertex blocks."""

    def __init__(self, nodes, vals):
        self.nodes, self.vals = np.asarray(nodes, dtype=np.int32), np.asarray(vals, dtype=np.float64)

    def getBC(self, V):
        g = Function(V)
        g.vector_values()[self.nodes] = self.vals.reshape(len(self.nodes), -1)
        return DirichletBC(g, self.nodes)


def dump_hierarchy(ctx, hier, out, pre):
    """Every operator and vector of one hierarchy the getters hand out, under "<pre>op_<hier>_<level>_<which>_*" / "<pre>vec_<hier>_<level>_<which>"."""
    s = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_SHAPE)
    out[pre + "vec_%d_0_%d" % (hier, _lib.AMG_VEC_SHAPE)] = s
    for l in range(int(s[0])):
        for w in OPS5:
            try:
                rp, col, val, shape, nnz = ctx.get_amg_operator(hier, l, w, raw=True)
            except (_lib.CfdhError, ValueError):
                continue
            k = pre + "op_%d_%d_%d" % (hier, l, w)
            out[k + "_rp"], out[k + "_col"], out[k + "_val"], out[k + "_shape"] = rp, col, val, np.array(shape)
        for w in LEVEL_VECS:
            try:
                out[pre + "vec_%d_%d_%d" % (hier, l, w)] = ctx.get_amg_vectors(hier, l, w)
            except (_lib.CfdhError, ValueError):
                pass
    for w in (_lib.AMG_VEC_COARSE_INV, _lib.AMG_VEC_SPGEMM_ROWS):
        try:
            out[pre + "vec_%d_0_%d" % (hier, w)] = ctx.get_amg_vectors(hier, 0, w)
        except (_lib.CfdhError, ValueError):
            pass


def dump_config(ctx, out, pre):
    """What depends on the options: the velocity hierarchy (owned + ghost rows only with the upper factor), H, the scalars."""
    dump_hierarchy(ctx, HA, out, pre)
    dump_hierarchy(ctx, HH, out, pre)
    for w in (_lib.AMG_VEC_CC_SCALARS, _lib.AMG_VEC_CC_ML, _lib.AMG_VEC_CC_PBC):
        out[pre + "vec_%d_0_%d" % (HH, w)] = ctx.get_amg_vectors(HH, 0, w)
    out[pre + "ras"], out[pre + "singular"] = ctx.info(12), ctx.info(76)


def dump_replicated(ctx, out):
    dump_hierarchy(ctx, HPG, out, "")
    out["dl0_n1"] = ctx.info(11)
    if ctx.info(11) > 0:
        for w in (_lib.AMG_OP_A, _lib.AMG_OP_P, _lib.AMG_OP_PT):
            rp, col, val, shape, nnz = ctx.get_amg_operator(HDL0, 0, w, raw=True)
            k = "op_%d_0_%d" % (HDL0, w)
            out[k + "_rp"], out[k + "_col"], out[k + "_val"], out[k + "_shape"] = rp, col, val, np.array(shape)
        for w in (_lib.AMG_VEC_WDINV, _lib.AMG_VEC_ORDER, _lib.AMG_VEC_DL0_SHAPE):
            out["vec_%d_0_%d" % (HDL0, w)] = ctx.get_amg_vectors(HDL0, 0, w)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    outdir = sys.argv[1]
    os.environ["CFDH_AMG_KEEP"] = "1"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cfd_hemodynamic_amd.solvers.stabilized_schur import Solver
    case = make_case(os.environ.get("PPC_CASE", "dfg16"))
    mesh = case.mesh
    dim = mesh.geometry.dim
    comm = PartComm(rank, world, os.environ.get("PPC_BACKEND", "host"))
    configs = [tuple(int(v) for v in c.split(":")) for c in os.environ.get("PPC_CONFIGS", "2:2").split(",")]
    opts = dict(schur_full=configs[0][0], cc_smooth_degree=configs[0][1])
    if os.environ.get("PPC_MAX_COARSE"):
        opts["amg_max_coarse"] = int(os.environ["PPC_MAX_COARSE"])
    extra = dict(_degree=2) if getattr(case, "degree", 1) == 2 else {}
    solver = Solver(getattr(case, "solver_mesh", mesh), case.dt, case.rho, case.mu, list(case.f)[:dim], comm=comm, quiet=True, device=0, options=opts,
                    **extra)
    solver.setup([_FixedBC(n, v) for f, n, v in case.bcs if f == 0], [_FixedBC(n, v) for f, n, v in case.bcs if f == 1])
    ctx, part = solver.ctx, solver._part
    nv, nvo, l2g = part.nv, part.nvo, part.l2g
    out = dict(backend=str(comm.backend), nvo=nvo, nv=nv, rccl=ctx.info(10), allgather=ctx.info(9))

    def apply(ru_g, rp_g, ghosts=None):
        ru, rp = ru_g[l2g].copy(), rp_g[l2g].copy()
        if ghosts is not None:
            ru[nvo:], rp[nvo:] = ghosts, -ghosts
        z = ctx.apply_preconditioner(np.concatenate([ru.ravel(), rp]))
        return z[: dim * nv].reshape(nv, dim)[:nvo].copy(), z[dim * nv:][:nvo].copy()

    if os.environ.get("PPC_MODE") == "step":
        ctx.assemble(True)
        ctx.apply_preconditioner(np.zeros((dim + 1) * nv))
        if os.environ.get("PPC_GETTERS", "1") == "1":
            dump_replicated(ctx, out)
            dump_config(ctx, out, "c0_")
        st = ctx.solve_step()
        u, p = ctx.get_solution()
        out.update(u=u.reshape(nv, dim)[:nvo], p=p[:nvo], krylov=st.krylov_its, newton=st.newton_its)
    else:
        if os.environ.get("PPC_STEP_FIRST") == "1":
            ctx.solve_step()
        u, un, p = global_vectors(case, dim, 17)
        ctx.set_state(u_prev=0.3 * un[l2g], p_prev=np.zeros(nv), u=0.3 * u[l2g], p=p[l2g])
        ctx.assemble(True)
        # whatever preconditioner exists by now belongs to another Jacobian: a change of schur_full drops it, the first configuration builds anew
        o = solver.options
        o.schur_full = 1 if configs[0][0] != 1 else 2
        ctx.set_options(o)
        for k, (sf, deg) in enumerate(configs):
            pre = "c%d_" % k
            o.schur_full, o.cc_smooth_degree = sf, deg
            ctx.set_options(o)
            ctx.apply_preconditioner(np.zeros((dim + 1) * nv))
            if k == 0:
                J = ctx.get_csr()
                out["J_rp"], out["J_col"], out["J_val"], out["J_shape"] = J.indptr, J.indices, J.data, np.array(J.shape)
                Fu, Fp = ctx.get_residual()
                out["F_u"], out["F_p"] = Fu.reshape(nv, dim)[:nvo].copy(), Fp[:nvo].copy()
                dump_replicated(ctx, out)
            dump_config(ctx, out, pre)
            singular = ctx.info(76) != 0
            ru1, ru2, rp1 = global_vectors(case, dim, 100 + k)
            _, _, rp2 = global_vectors(case, dim, 200 + k)
            if singular:
                rp1, rp2 = rp1 - rp1.mean(), rp2 - rp2.mean()
            out[pre + "zu"], out[pre + "zp"] = apply(ru1, rp1)
            out[pre + "zu_again"], out[pre + "zp_again"] = apply(ru1, rp1)
            out[pre + "zu_garbage"], out[pre + "zp_garbage"] = apply(ru1, rp1, ghosts=1e30)
            out[pre + "zu_2"], out[pre + "zp_2"] = apply(ru2, rp2)
            out[pre + "zu_lin"], out[pre + "zp_lin"] = apply(0.7 * ru1 - 1.3 * ru2, 0.7 * rp1 - 1.3 * rp2)
            if k == 0:
                out[pre + "zu_vel"], out[pre + "zp_vel"] = apply(ru1, 0.0 * rp1)
                out[pre + "zu_pres"], out[pre + "zp_pres"] = apply(0.0 * ru1, rp1)
        if os.environ.get("PPC_BDF2") == "1":
            un2, _, _ = global_vectors(case, dim, 18)
            ctx.set_time_scheme(1.0, 1.5, -2.0, 0.5)
            ctx.set_previous2(0.3 * un2[l2g])
            ctx.assemble(True)
            J = ctx.get_csr()
            out["J2_rp"], out["J2_col"], out["J2_val"], out["J2_shape"] = J.indptr, J.indices, J.data, np.array(J.shape)
            Fu, Fp = ctx.get_residual()
            out["F2_u"], out["F2_p"] = Fu.reshape(nv, dim)[:nvo].copy(), Fp[:nvo].copy()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
