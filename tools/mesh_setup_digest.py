#!/usr/bin/env python
"""sha256 digests of what the context builders produce, for comparing two builds of libcfdh.so byte for byte (the mesh set-up is
host code: numbering, graph and staging order decide the summation order of the assembly, h_Lval / h_Ml feed the preconditioner).

    python tools/mesh_setup_digest.py --out new.txt [--lib path/to/other/libcfdh.so]
    python tools/mesh_setup_digest.py --out old.txt --lib ../old-checkout/cfd_hemodynamic_amd/libcfdh.so && cmp old.txt new.txt

One small context of every family: closed-form P1 in 2-D / 3-D (also with CFDH_NO_RENUMBER=1), generic P1 / P2 / Q1 in 2-D / 3-D,
IPCS in 2-D / 3-D with either scheme (ipcs_bdf2; ipcs_midpoint with a pressure Dirichlet object and its block operators), and one
part of a 2-part split (two cell layers) of a closed-form mesh and of a P2 tetrahedral mesh.  Per context (IPCS: the operators):
Jacobian structure and values, residual, and -- whole meshes -- solution and iteration counts of two time steps; then the
functionals of kinds 2 to 7 (bit patterns) and cfdh_info 76.  The info counters 13 to 17 of every context go to stdout, not
into the file: they count collectives and read-backs, which two builds may do differently while computing the same numbers.

All of those meshes are far below the 16384 rows from which the AMG levels use SELL-64 / fp32 (cfdh_level_fine, cfdh_sweep_sell
in csrc/cfdh_internal.hpp).  The pc-* contexts are above it: z = apply_preconditioner(r) for one seeded r on dfg_case(64) with
pc_type 0, 1, 2 (fused cycle, SELL on level 0), the same with CFDH_NO_FUSED_AMG=1 (host-built hierarchy, sweep-by-sweep cycle
on SELL A and P) and with amg_smooth_degree 2 on top (Chebyshev cycle, the two-step SELL kernel of the Cahouet-Chabard
operator), and pc_type 1 on create_unit_cube(26) (19683 vertices, rows between 12 and 20 entries: the chunked SELL up-sweep in
the pressure hierarchy, CSR in the velocity hierarchy).  CFDH_NO_FUSED_AMG is read with getenv at every hierarchy build and
nowhere else, so it is set in this process around the context it is meant for."""
import argparse
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--lib", default=None, help="another build of libcfdh.so to load instead of the one in the tree")
    a = ap.parse_args()
    from cfd_hemodynamic_amd import _lib
    if a.lib:
        _lib._SO = os.path.abspath(a.lib)
    from cfd_hemodynamic_amd.elements import NodeMesh, NodeMesh3D
    from cfd_hemodynamic_amd.mesh3d import create_unit_cube
    from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
    from gen3_util import LIB_ETYPE3, node_mesh3
    from gen_util import LIB_ETYPE, node_mesh
    from util import dfg_case

    lines = []

    def put(case, item, *arrays):
        lines.append("%s %s %s" % (case, item, sha(*arrays)))

    def scalars(case, ctx):
        for kind in range(2, 8):
            try:
                lines.append("%s functional%d %s" % (case, kind, np.float64(ctx.functional(kind)).tobytes().hex()))
            except (RuntimeError, ValueError) as e:  # a kind the context family does not have
                lines.append("%s functional%d %s" % (case, kind, str(e).split("(")[0].strip()))
        lines.append("%s info76 %d" % (case, ctx.info(76)))
        print("%s counters 13-17: %s" % (case, " ".join(str(ctx.info(k)) for k in range(13, 18))))

    def part(m, rank):
        g = types.SimpleNamespace(x=m.x, cells=m.cells, num_vertices=len(m.x), num_cells=len(m.cells), facet_cells=m.facet_cells,
                                  facet_local=m.facet_local, facet_marker=np.zeros(len(m.facet_cells), np.int32))
        return LocalPart(g, partition_vertices_rcb(m.x, 2), rank, layers=2)

    def fgmres_context(case, m, etype, nvo=None, steps=2):
        d = m.x.shape[1]
        nv = len(m.x)
        rng = np.random.default_rng(17)
        ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, np.zeros(len(m.facet_cells), np.int32), nv_owned=nvo, etype=etype)
        ctx.set_params(0.02, 1.3, 0.04, f=(0.2, -0.1, 0.3)[:d])
        if nvo is None:  # a rotation on the whole boundary (no net flux), pressure free
            bnd = np.unique(np.asarray(m.facet_vertices)).astype(np.int32)
            vals = np.zeros((len(bnd), d))
            vals[:, 0], vals[:, 1] = 0.1 * m.x[bnd, 1], -0.1 * m.x[bnd, 0]
            ctx.add_dirichlet(0, bnd, vals)
        un, u, p = 0.05 * rng.standard_normal(d * nv), 0.05 * rng.standard_normal(d * nv), 0.05 * rng.standard_normal(nv)
        ctx.set_state(u_prev=un, p_prev=np.zeros(nv), u=u, p=p)
        ctx.assemble(True)
        J = ctx.get_csr()
        put(case, "csr-structure", J.indptr, J.indices)
        put(case, "csr-values", J.data)
        put(case, "residual", *ctx.get_residual())
        if nvo is None:  # a part needs its communicator to solve
            for k in range(steps):
                try:
                    st = ctx.solve_step()
                    lines.append("%s step%d newton %d krylov %d" % (case, k, st.newton_its, st.krylov_its))
                except RuntimeError as e:
                    lines.append("%s step%d %s" % (case, k, str(e).split("(")[0].strip()))
                put(case, "step%d-solution" % k, *ctx.get_solution())
                ctx.advance()
        scalars(case, ctx)
        ctx.close()

    def ipcs_context(case, m, nm, midpoint=False):
        d = m.x.shape[1]
        nn, nvert = len(nm.x), m.num_vertices
        rng = np.random.default_rng(19)
        ctx = _lib.IpcsContext(nm.x, nm.cells, nvert, nm.facet_cells, nm.facet_local, np.zeros(len(nm.facet_cells), np.int32))
        ctx.set_params(0.01, 1.06, 0.05, f=np.asarray((0.3, -0.7, 0.2)[:d]))
        bnd = np.unique(np.asarray(nm.facet_vertices)).astype(np.int32)
        vals = np.zeros((len(bnd), d))
        vals[:, 0], vals[:, 1] = 0.1 * nm.x[bnd, 1], -0.1 * nm.x[bnd, 0]
        ctx.add_dirichlet(0, bnd, vals)
        if midpoint:  # the block matrix, and a pressure value on the vertices of the side x = min: lifting formed on the device
            ctx.set_scheme(_lib.IPCS_MIDPOINT)
            side = np.nonzero(m.x[:, 0] == m.x[:, 0].min())[0].astype(np.int32)
            ctx.add_dirichlet(1, side, np.full(len(side), 0.02))
        u = 0.05 * rng.standard_normal(d * nn)
        ctx.set_state(u_prev=u, p_prev=np.zeros(nvert), u=u, p=np.zeros(nvert))
        ctx.set_previous2(u)
        for k in range(2):
            try:
                st = ctx.step()
                lines.append("%s step%d its %s" % (case, k, " ".join(str(int(i)) for i in st.its)))
            except RuntimeError as e:
                lines.append("%s step%d %s" % (case, k, str(e).split("(")[0].strip()))
            put(case, "step%d-solution" % k, *ctx.get_solution())
            if midpoint:  # the second step starts from the first one's fields: its lifting sees p_prev != 0
                ctx.advance()
        for which in range(2) if midpoint else ():
            A = ctx.get_block_operator(which)
            put(case, "block-operator%d" % which, A.indptr, A.indices, A.data)
        for which in range(1 if midpoint else 0, 3 + 2 * d):  # A1 of ipcs_midpoint is the block matrix above
            A = ctx.get_operator(which)
            put(case, "operator%d" % which, A.indptr, A.indices, A.data)
        scalars(case, ctx)
        ctx.close()

    def pc_context(case, m, bcs, dt, rho, mu, r, env=None, pcd=None, **opts):
        d, nv = m.x.shape[1], len(m.x)
        os.environ.update(env or {})
        ctx = _lib.Context(m.x, m.cells, m.facet_cells, m.facet_local, m.facet_marker)
        ctx.set_params(dt, rho, mu, f=np.zeros(d))
        for field, nodes, vals in bcs:
            ctx.add_dirichlet(field, nodes, vals)
        o = ctx.default_options()
        for key, val in opts.items():
            setattr(o, key, val)
        ctx.set_options(o)
        if pcd:
            ctx.set_schur_pcd(*pcd)
        rng = np.random.default_rng(17)
        u, un = 0.3 * rng.standard_normal(d * nv), 0.3 * rng.standard_normal(d * nv)
        ctx.set_state(u_prev=un, p_prev=np.zeros(nv), u=u, p=rng.standard_normal(nv))
        ctx.assemble(True)
        put(case, "csr-values", ctx.get_csr().data)
        put(case, "pc-apply", ctx.apply_preconditioner(r))  # builds the preconditioner first
        put(case, "pc-apply-again", ctx.apply_preconditioner(r))
        lines.append("%s info76 %d" % (case, ctx.info(76)))
        print("%s counters 13-17: %s" % (case, " ".join(str(ctx.info(k)) for k in range(13, 18))))
        ctx.close()
        for key in env or {}:
            os.environ.pop(key)

    tri, tet = dfg_case(6).mesh, create_unit_cube(4)
    for env in ("", "1"):
        os.environ["CFDH_NO_RENUMBER"] = env
        fgmres_context("closed-2d" + ("-norenumber" if env else ""), tri, 0)
        fgmres_context("closed-3d" + ("-norenumber" if env else ""), tet, 0)
    os.environ.pop("CFDH_NO_RENUMBER")
    for kind in ("P1", "P2", "Q1"):
        fgmres_context("gen-2d-" + kind, node_mesh(kind, 8, 0.05), LIB_ETYPE[kind])
        fgmres_context("gen-3d-" + kind, node_mesh3(kind, 3 if kind == "P2" else 4, 0.05), LIB_ETYPE3[kind])
    ipcs_context("ipcs-2d", tri, NodeMesh(tri))
    ipcs_context("ipcs-3d", tet, NodeMesh3D(tet))
    ipcs_context("ipcs-mid-2d", tri, NodeMesh(tri), midpoint=True)
    ipcs_context("ipcs-mid-3d", tet, NodeMesh3D(tet), midpoint=True)
    for case, m, etype in (("part-closed-2d", tri, 0), ("part-closed-3d", tet, 0), ("part-gen-3d-P2", node_mesh3("P2", 3, 0.05), 1)):
        lp = part(m, 1)
        pm = types.SimpleNamespace(x=lp.x, cells=lp.cells, facet_cells=lp.facet_cells, facet_local=lp.facet_local)
        fgmres_context(case, pm, etype, nvo=lp.nvo)
    # ---- above the SELL threshold: one preconditioner application per cycle kind
    k = dfg_case(64)
    assert k.mesh.num_vertices >= 16384
    r2 = np.random.default_rng(23).standard_normal(3 * k.mesh.num_vertices)
    sweeps = {"CFDH_NO_FUSED_AMG": "1"}
    pc_context("pc-2d-type0", k.mesh, k.bcs, k.dt, k.rho, k.mu, r2, pc_type=0)
    pc_context("pc-2d-type1", k.mesh, k.bcs, k.dt, k.rho, k.mu, r2, pc_type=1)
    pc_context("pc-2d-type2", k.mesh, k.bcs, k.dt, k.rho, k.mu, r2, pcd=(2, 3, 1), pc_type=2)
    pc_context("pc-2d-type1-sweeps", k.mesh, k.bcs, k.dt, k.rho, k.mu, r2, env=sweeps, pc_type=1)
    pc_context("pc-2d-type1-sweeps-cheb2", k.mesh, k.bcs, k.dt, k.rho, k.mu, r2, env=sweeps, pc_type=1, amg_smooth_degree=2)
    cube = create_unit_cube(26)
    bnd = np.nonzero(np.abs(cube.x - 0.5).max(axis=1) > 0.5 - 1e-12)[0].astype(np.int32)
    out = bnd[np.isclose(cube.x[bnd, 0], 1.0)]
    wall = np.setdiff1d(bnd, out).astype(np.int32)
    r3 = np.random.default_rng(29).standard_normal(4 * cube.num_vertices)
    pc_context("pc-3d-type1", cube, [(0, wall, np.zeros((len(wall), 3))), (1, out, np.zeros(len(out)))], 0.01, 1.0, 1e-2, r3, pc_type=1)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d lines -> %s" % (len(lines), a.out))


if __name__ == "__main__":
    main()
