"""The twin of the partitioned preconditioner action (tests/part_pc_twin.py) pinned without a GPU: operators from the C oracle on the
DFG mesh, partitioned by the package's own partitioner as tests/_gloo_worker.py does."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_twin as T
import part_pc_twin as PT
from util import dfg_case, make_oracle

from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
from oracle import orc

DIM = 2
_CACHE = {}


def _global():
    if "g" not in _CACHE:
        case = dfg_case(8)
        m, nv = case.mesh, case.mesh.num_vertices
        rng = np.random.default_rng(7)
        x, un = 0.1 * rng.standard_normal(3 * nv), 0.1 * rng.standard_normal(2 * nv)
        O = make_oracle(case)
        O.set_un(un)
        O.assemble(x)
        pbc = np.zeros(nv, dtype=np.uint8)
        for f, nodes, _ in case.bcs:
            if f == 1:
                pbc[nodes] = 1
        Ld = PT.dirichlet_laplacian(m.x[:, :DIM], m.cells, pbc)[0]
        hLg = T.build_hierarchy(Ld, 0.07, max_coarse=30, singular=not pbc.any())
        _CACHE["g"] = (case, x, un, O.csr(), pbc, hLg)
    return _CACHE["g"]


def _local_jacobian(case, part, x, un):
    nv = case.mesh.num_vertices
    OL = orc.Oracle(part.x, part.cells, part.facet_cells, part.facet_local, case.dt, case.rho, case.mu, case.f)
    for field, nodes, vals in case.bcs:
        loc = part.g2l[nodes]
        keep = loc >= 0
        (OL.add_bc_u if field == 0 else OL.add_bc_p)(loc[keep].astype(np.int32), vals[keep])
    l2g, nl = part.l2g, part.nv
    OL.set_un(un.reshape(-1, 2)[l2g].ravel())
    OL.assemble(np.concatenate([x[: 2 * nv].reshape(-1, 2)[l2g].ravel(), x[2 * nv:][l2g]]))
    own = np.arange(part.nvo)
    rows = np.concatenate([np.stack([2 * own, 2 * own + 1], 1).ravel(), 2 * nl + own])
    return sp.csr_matrix(OL.csr())[rows]          # [3 nvo x 3 nv]: the owned rows, complete


def _ranks(nparts, layers=2, schur_full=2, with_dl0=True):
    key = (nparts, layers, schur_full, with_dl0)
    if key in _CACHE:
        return _CACHE[key]
    case, x, un, Jg, pbc_g, hLg = _global()
    m = case.mesh
    owner = partition_vertices_rcb(m.x, nparts)
    parts = [LocalPart(m, owner, r, layers=layers) for r in range(nparts)]
    Jl = [_local_jacobian(case, p, x, un) for p in parts]
    owned_rows = [PT.proxy_rows(J, DIM, p.nvo, p.nv)[0] for J, p in zip(Jl, parts)]
    alpha, beta = 2.0 * case.rho / case.dt, case.mu
    ranks = []
    for r, (p, J) in enumerate(zip(parts, Jl)):
        R = PT.RankOps()
        R.part, R.dim = p, DIM
        R.A01, R.A10, A11 = PT.jacobian_blocks(J, DIM, p.nvo, p.nv)
        R.ras = schur_full == 2 and nparts > 1
        proxy = PT.extended_proxy(owned_rows, parts, r) if R.ras else T.canonical(owned_rows[r][:, : p.nvo])
        R.hA = T.build_hierarchy(proxy, 0.07, max_coarse=30)
        T.fold_dense(R.hA)
        R.hA.levels[0].fine = R.hA.levels[0].sell = True      # float32 storage on the finest level, as on a large mesh
        R.pbc = pbc_g[p.l2g[: p.nvo]]
        ml = PT.lumped_mass(p.x[:, :DIM], p.cells)[: p.nvo]
        R.ml = np.where(R.pbc == 0, ml, 0.0)
        Lp = T.canonical(PT.dirichlet_laplacian(p.x[:, :DIM], p.cells, np.zeros(p.nv))[0][: p.nvo, : p.nvo])
        Hm, _ = T.h_operator(T.canonical(A11[:, : p.nvo]), Lp, ml, R.pbc, alpha, beta)
        R.Hlev, R.fused_h, R.alpha, R.beta = T.Level(Hm, ratio=8.0), True, alpha, beta
        L0 = hLg.levels[0]
        R.dl0 = PT.cut_dist_level(L0.A, L0.P, L0.w, p) if with_dl0 and nparts > 1 else None
        ranks.append(R)
    _CACHE[key] = (ranks, parts, owner, owned_rows)
    return _CACHE[key]


def _dev(H, b):
    return T.vcycle_composite(H, b, "device")


@pytest.mark.parametrize("schur_full", [2, 1, 0])
@pytest.mark.parametrize("degree", [2, 3])
def test_one_part_without_ghosts_is_the_one_rank_action_bitwise(schur_full, degree):
    case, _, _, Jg, pbc_g, hLg = _global()
    nv = case.mesh.num_vertices
    ranks, parts, _, _ = _ranks(1, schur_full=schur_full)
    R = ranks[0]
    assert parts[0].ng == 0 and np.array_equal(parts[0].l2g, np.arange(nv)) and R.dl0 is None
    op = T.CCOperators()
    op.__dict__.update(dim=DIM, schur_full=schur_full, degree=degree, singular=True, fused_h=R.fused_h, alpha=R.alpha, beta=R.beta, pbc=R.pbc,
                       ml=R.ml, hL=hLg, hA=R.hA, Hlev=R.Hlev, A01=R.A01, A10=R.A10)
    r = np.random.default_rng(3).standard_normal(3 * nv)
    ref = T.cc_action(r, op, _dev, "device")
    zu, zp = PT.action(ranks, hLg, r[: 2 * nv].reshape(nv, 2), r[2 * nv:], schur_full, degree, True, _dev, "device")
    assert np.array_equal(zu.reshape(-1), ref[: 2 * nv]) and np.array_equal(zp, ref[2 * nv:])


@pytest.mark.parametrize("nparts", [2, 3, 5])
def test_distributed_cycle_with_ghost_rhs_is_the_global_sweep_cycle(nparts):
    """with the right-hand side present on the ghosts the distributed level does the SAME arithmetic as the replicated
    cycle -- Jacobi sweeps are row-local.  What differs is the order of the sums (local column numbering, the coarse right-hand side summed
    rank by rank): entrywise within gamma_(4 k) of the cycle applied to absolute values."""
    case, _, _, _, _, hLg = _global()
    ranks, parts, _, _ = _ranks(nparts)
    y_g = np.random.default_rng(11).standard_normal(case.mesh.num_vertices)
    ts, det = PT.dist_pressure_cycle(ranks, hLg, [y_g[p.l2g[: p.nvo]] for p in parts], True, fused=False)
    got = PT._gather(ranks, ts, len(y_g))
    ref = T.vcycle_sweeps(hLg, y_g)
    c, k = PT.sweeps_bound(hLg, np.abs(y_g))
    ratio = np.abs(got - ref) / (T.gamma(4 * k) * c)
    print("\n[part-twin] %d parts: distributed vs global sweep cycle, largest |diff| / bound %.3g (relative distance %.3g)"
          % (nparts, ratio.max(), T.rel_distance(got, ref)))
    assert ratio.max() <= 1.0
    # ... and through the composite operators on the replicated levels (k_dl0_up's default) it is the same linear map
    ts2, _ = PT.dist_pressure_cycle(ranks, hLg, [y_g[p.l2g[: p.nvo]] for p in parts], True, fused=True)
    c2, k2 = T.vcycle_bound(PT._sub_hierarchy(hLg, 1), np.abs(det["bc"]))
    assert T.rel_distance(PT._gather(ranks, ts2, len(y_g)), ref) <= T.gamma(4 * (k + k2)) * np.linalg.norm(c) / np.linalg.norm(ref)


@pytest.mark.parametrize("nparts", [2, 3, 5])
def test_ghost_zero_presmoothing_differs_at_the_part_boundaries_only(nparts):
    """Default (no exchange of the right-hand side's ghost layer): the pre-smoothed iterate is zero on the ghosts.  What that changes
    DIRECTLY is local: the residual behind the pre-sweep on the owned rows with a neighbour owned elsewhere, and -- for one and the same
    coarse correction -- the post-smoothed result on those rows.  (The cycle's result itself differs everywhere: the changed residual
    reaches every row through the coarse solve.)  The support is asserted, not a size."""
    case, _, _, _, _, hLg = _global()
    ranks, parts, owner, _ = _ranks(nparts)
    nvg = case.mesh.num_vertices
    y_g = np.random.default_rng(12).standard_normal(nvg)
    ys = [y_g[p.l2g[: p.nvo]] for p in parts]
    t1, d1 = PT.dist_pressure_cycle(ranks, hLg, ys, True, fused=False)
    t0, d0 = PT.dist_pressure_cycle(ranks, hLg, ys, False, fused=False)
    near = PT.interface_rows(hLg.levels[0].A, owner, 1)
    dr = PT._gather(ranks, d0["r"], nvg) != PT._gather(ranks, d1["r"], nvg)
    assert dr.any() and not (dr & ~near).any()
    assert all(np.array_equal(a[: p.nvo], b[: p.nvo]) for a, b, p in zip(d0["xa"], d1["xa"], parts))
    same_xc, _ = PT.dist_pressure_cycle(ranks, hLg, ys, False, fused=False, xc_override=d1["xc"])
    dt = PT._gather(ranks, same_xc, nvg) != PT._gather(ranks, t1, nvg)
    assert dt.any() and not (dt & ~near).any()
    assert not (dt & ~PT.interface_rows(hLg.levels[0].A, owner, 2)).any()
    full = PT._gather(ranks, t0, nvg) != PT._gather(ranks, t1, nvg)
    assert (full & ~PT.interface_rows(hLg.levels[0].A, owner, 2)).any(), "the coarse solve spreads the difference"


@pytest.mark.parametrize("nparts,layers", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_extended_proxy_is_the_principal_submatrix_of_the_global_proxy(nparts, layers):
    case, _, _, Jg, _, _ = _global()
    nv = case.mesh.num_vertices
    ranks, parts, _, owned_rows = _ranks(nparts, layers=layers)
    Pg = PT.proxy_rows(Jg, DIM, nv, nv)[0]
    # the exchange alone, on rows cut exactly out of the global proxy: bitwise
    cut = [T.canonical(Pg[p.l2g[: p.nvo]][:, p.l2g]) for p in parts]
    for r, p in enumerate(parts):
        assert p.ng > 0
        E = PT.extended_proxy(cut, parts, r)
        ref = T.canonical(Pg[p.l2g][:, p.l2g])
        assert np.array_equal(E.indptr, ref.indptr) and np.array_equal(E.indices, ref.indices) and np.array_equal(E.data, ref.data)
        # ... and on the rows every rank assembles from its own cells: the same pattern, values to the rounding of the cell sums
        # (1e-13 of the largest entry, the bound tests/_gloo_worker.py puts on the owned Jacobian rows)
        E = PT.extended_proxy(owned_rows, parts, r)
        assert np.array_equal(E.indptr, ref.indptr) and np.array_equal(E.indices, ref.indices)
        assert np.abs(E.data - ref.data).max() <= 1e-13 * np.abs(Jg).max()


@pytest.mark.parametrize("schur_full", [2, 1, 0])
def test_partitioned_action_statements(schur_full):
    """Properties the restatement must have whatever the operators: r_p = 0 with the upper factor gives z_p = 0 and one cycle of the
    extended hierarchy per rank; the ghost-layer switches matter; the lower factor returns y_u."""
    case, _, _, _, _, hLg = _global()
    nv = case.mesh.num_vertices
    ranks, parts, _, _ = _ranks(3, schur_full=schur_full)
    rng = np.random.default_rng(5)
    ru, rp = rng.standard_normal((nv, 2)), rng.standard_normal(nv)
    zu, zp = PT.action(ranks, hLg, ru, rp, schur_full, 2, False, _dev, "device")
    if schur_full == 2:
        zu0, zp0 = PT.action(ranks, hLg, ru, 0 * rp, 2, 2, False, _dev, "device")
        assert not zp0.any()
        for R, p in zip(ranks, parts):
            assert np.array_equal(zu0[p.l2g[: p.nvo]], _dev(R.hA, ru[p.l2g])[: p.nvo])
        zu1, _ = PT.action(ranks, hLg, ru, rp, 2, 2, False, _dev, "device", ras_ghost_rhs=False)
        assert not np.array_equal(zu1, zu)
    if schur_full == 0:
        for R, p in zip(ranks, parts):
            assert np.array_equal(zu[p.l2g[: p.nvo]], _dev(R.hA, ru[p.l2g[: p.nvo]]))
    _, zp1 = PT.action(ranks, hLg, ru, rp, schur_full, 2, False, _dev, "device", dl0_ghost_rhs=True)
    assert not np.array_equal(zp1, zp) and T.rel_distance(zp1, zp) < 0.5
    # the action is linear
    z2 = PT.action(ranks, hLg, 2.0 * ru, 2.0 * rp, schur_full, 2, False, _dev, "device")
    assert T.rel_distance(z2[0], 2.0 * zu) <= 1e-13 and T.rel_distance(z2[1], 2.0 * zp) <= 1e-13
