"""Worker of tests/test_gpu_amg_head.py: one rank of a two-process job whose ranks share GPU 0.  Builds its part of dfg_case(64)
through the ordinary solver plug-in (restricted additive Schwarz on owned + ghost vertices: the finest up-sweep of the velocity cycle
keeps the first nvo of its nv rows), applies the preconditioner to seeded right-hand sides and writes z, nvo, nv and the head widths
of the velocity hierarchy's finest level to one .npz per rank.  CFDH_AMG_HEAD / CFDH_AMG_HEAD_W come from the parent."""
import os
import sys

import numpy as np
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cfd_hemodynamic_amd import _lib  # noqa: E402
from cfd_hemodynamic_amd.parallel import PartComm  # noqa: E402
from _gpu_part_pc_worker import _FixedBC, global_vectors, make_case  # noqa: E402


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    outdir = sys.argv[1]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cfd_hemodynamic_amd.solvers.stabilized_schur import Solver
    case = make_case("dfg64")
    dim = case.mesh.geometry.dim
    comm = PartComm(rank, world, "host")
    solver = Solver(case.mesh, case.dt, case.rho, case.mu, list(case.f)[:dim], comm=comm, quiet=True, device=0, options=dict(schur_full=2, cc_smooth_degree=2))
    solver.setup([_FixedBC(n, v) for f, n, v in case.bcs if f == 0], [_FixedBC(n, v) for f, n, v in case.bcs if f == 1])
    ctx, part = solver.ctx, solver._part
    nv, nvo, l2g = part.nv, part.nvo, part.l2g
    u, un, p = global_vectors(case, dim, 17)
    ctx.set_state(u_prev=0.3 * un[l2g], p_prev=np.zeros(nv), u=0.3 * u[l2g], p=p[l2g])
    ctx.assemble(True)
    ctx.apply_preconditioner(np.zeros((dim + 1) * nv))     # builds
    out = dict(nvo=nvo, nv=nv, ras=ctx.info(12), n0=ctx.get_amg_vectors(_lib.AMG_HIER_A, 0, _lib.AMG_VEC_DINV).size,
               head_sb=ctx.get_amg_head(_lib.AMG_HIER_A, 0, _lib.AMG_OP_SB), head_sc=ctx.get_amg_head(_lib.AMG_HIER_A, 0, _lib.AMG_OP_SC))
    for k in range(2):
        ru, _, rp = global_vectors(case, dim, 100 + k)
        if ctx.info(76):
            rp = rp - rp.mean()
        z = ctx.apply_preconditioner(np.concatenate([ru[l2g].ravel(), rp[l2g]]))
        out["zu%d" % k], out["zp%d" % k] = z[: dim * nv].reshape(nv, dim)[:nvo].copy(), z[dim * nv:][:nvo].copy()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
