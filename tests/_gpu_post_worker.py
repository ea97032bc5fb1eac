"""Worker of the partitioned cases of tests/test_gpu_post.py: one rank of a two-process job whose ranks share GPU 0 and exchange through the
host backend.  For every case of POST_CASES it builds its part of the mesh directly through _lib.Context, sets the part's share of one
global random state (owned nodes and ghosts alike, so that all ranks agree), and writes the functionals and the owned rows of its wall
shear field to one .npz per rank.  All comparisons happen in the parent, on the CPU.

Cases: dfg16 (P1 triangles), cube<n> (P1 tetrahedra, n cells per edge), p2tri, q1quad, p2tet, q1hex (the sheared node meshes of
tests/_gpu_part_pc_worker.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MU = 0.7
M_A, M_B = 5, 7
KINDS = {2: (0, 1, 2, 3, 7, 8), 3: (2, 3, 7, 8)}      # functional kinds written, by gdim


def mesh_of(name):
    """(the mesh whose nodes are partitioned, etype for _lib.Context); the parent calls this too."""
    from _gpu_part_pc_worker import GENERIC, make_case
    m = make_case(name).mesh
    return m, (0 if name not in GENERIC else (1 if GENERIC[name][1] == "P2" else 2))


def markers_of(nfac):
    return np.array([M_A, M_B, 0], dtype=np.int32)[np.arange(nfac) % 3]


def state_of(nn, d, seed=23):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nn, d)), rng.standard_normal((nn, d)), rng.standard_normal(nn), rng.standard_normal(nn)


def main():
    import torch.distributed as dist
    from cfd_hemodynamic_amd import _lib
    from cfd_hemodynamic_amd.parallel import PartComm
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    outdir = sys.argv[1]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for name in os.environ["POST_CASES"].split(","):
        m, et = mesh_of(name)
        d, nn = m.x.shape[1], len(m.x)
        comm = PartComm(rank, world, "host")
        part = comm.make_part(m)
        mk = markers_of(m.num_facets)
        ctx = _lib.Context(part.x, part.cells, part.facet_cells, part.facet_local, mk[part.facet_ids], nv_owned=part.nvo, device=0, etype=et)
        comm.attach(ctx)
        ctx.set_params(0.01, 1.0, MU, f=np.zeros(d))
        u, un, p, pn = state_of(nn, d)
        l2g = part.l2g
        ctx.set_state(u_prev=un[l2g].ravel(), p_prev=pn[l2g], u=u[l2g].ravel(), p=p[l2g])
        for k in KINDS[d]:
            for marker in ((0,) if k in (2, 3) else (M_A, M_B)):
                out["%s_f_%d_%d" % (name, k, marker)] = ctx.functional(k, marker)
        out[name + "_wss"] = ctx.wall_shear_stress().reshape(part.nv, d)[: part.nvo].copy()
        out[name + "_owned"] = np.asarray(part.owned_global)
        dist.barrier()
        ctx.close()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
