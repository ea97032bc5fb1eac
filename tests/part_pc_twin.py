"""NumPy / SciPy restatement (fp64, no GPU) of the Cahouet-Chabard action of a PARTITIONED run, rank by rank, on top of amg_twin.py --
written from pc_stage / pc_exchange (csrc/cfdh_solver.cpp), k_dl0_down / k_dl0_up (csrc/cfdh_amg_apply.hip) and build_global_pressure:

    pressure   t_p = r_p                                  (schur_full 1, 0: r_p - A10 y_u, y_u = rank-local cycle on r_u, halo of y_u)
               zH  = Chebyshev on the rank's H (ghost columns dropped),  y = M_l zH
               distributed level 0:  b = y on the owned rows, on the ghosts y of their owners (ghost_rhs) or 0
                                     xa = W b,  r = b - A xa on the owned rows,  b_c = sum over the ranks of PT r
                                     x_c = cycle of the replicated levels 1.. on b_c
                                     x1 = xa + P x_c on all local rows,  t = x1 + W (b - A x1) on the owned rows
               no distributed level: t = owned part of one cycle of the replicated hierarchy on the gathered y
               z_p = alpha t + beta zH  (t_p on the Dirichlet rows)
    velocity   schur_full 2: t_u = r_u - A01 z_p (ghost columns after the halo of z_p), t_u of the ghosts from their owners (or 0), one
               cycle of the rank's extended hierarchy on owned + ghost rows, owned part kept
               schur_full 1: the rank-local cycle on t_u;  schur_full 0: z_u = y_u
    singular   z_p minus its mean over ALL ranks

The exchanges are array indexing through `l2g`.  Vectors travel as global arrays: r_u [nvg, dim], r_p [nvg]; the result likewise, assembled
from the owned parts.  With one part and no distributed level the statements are those of amg_twin.cc_action in the same order (bitwise).

Storage: `storage = "device"` rounds what the device keeps in float32: the composite operators through amg_twin.vcycle_composite, the
one-pass smoother on H, and the SELL copies of the distributed level where the library took SELL (float32(a_ij w_j) in the pre-sweep)."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import amg_twin as T


class DistLevel:
    """This rank's share of level 0 of the replicated hierarchy: A [owned x local], P [local x n1], PT [n1 x owned], w [local]; sell_pre /
    sell_post / sell_p: the float32 SELL copies the three sweeps take."""

    def __init__(self, A, P, PT, w, sell_pre=False, sell_post=False, sell_p=False):
        self.A, self.P, self.PT, self.w = sp.csr_matrix(A), sp.csr_matrix(P), sp.csr_matrix(PT), np.asarray(w, dtype=np.float64)
        self.sell_pre, self.sell_post, self.sell_p = bool(sell_pre), bool(sell_post), bool(sell_p)


def cut_dist_level(A0, P0, w0, part, sell=(False, False, False)):
    """The distributed level cut out of level 0 of the replicated hierarchy by global id, as build_global_pressure does: rows l2g[:nvo] of
    A0 with the columns in local numbering, rows l2g of P0, PT the transpose of the owned rows of P."""
    l2g, nvo, nv = np.asarray(part.l2g, dtype=np.int64), part.nvo, part.nvo + part.ng
    g2l = -np.ones(A0.shape[0], dtype=np.int64)
    g2l[l2g] = np.arange(nv)
    Ar = sp.csr_matrix(A0)[l2g[:nvo]].tocoo()
    if (g2l[Ar.col] < 0).any():
        raise ValueError("a neighbour of an owned vertex is not local")
    A = T.canonical(sp.csr_matrix((Ar.data, (Ar.row, g2l[Ar.col])), shape=(nvo, nv)))
    P = T.canonical(sp.csr_matrix(P0)[l2g])
    PT = T.canonical(P[:nvo].T.tocsr())
    return DistLevel(A, P, PT, np.asarray(w0)[l2g], *sell)


class RankOps:
    """One rank: part (nvo, ng, l2g), dim, A01 [dim nvo x nv], A10 [nvo x dim nv] (local columns, ghosts included), hA (amg_twin.Hierarchy
    on nv rows when `ras`, on the nvo owned rows otherwise), ras, Hlev (amg_twin.Level on nvo rows), fused_h, ml, pbc [nvo], alpha, beta,
    dl0 (DistLevel or None)."""


def _sub_hierarchy(H, l0):
    S = T.Hierarchy()
    S.levels, S.X, S.singular = H.levels[l0:], H.X, H.singular
    return S


def coarse_cycle(hLg, bc, storage="fp64", fused=True):
    """The replicated levels 1.. of hLg on the all-reduced coarse right-hand side: composite operators (k_dl0_up's default) or sweep by sweep."""
    S = _sub_hierarchy(hLg, 1)
    return T.vcycle_composite(S, bc, storage) if fused else T.vcycle_sweeps(S, bc)


def dist_down(d, b, storage="fp64"):
    """k_dl0_down on one rank: b [local] -> (xa [local], r [owned])."""
    nvo = d.A.shape[0]
    AW = d.A @ T.diag(d.w)
    if storage == "device" and d.sell_pre:
        AW = T.f32(AW)
    return d.w * b, b[:nvo] - AW @ b


def dist_up(d, b, xa, xc, storage="fp64"):
    """k_dl0_up behind the coarse cycle on one rank: -> (x1 [local], t [owned])."""
    nvo = d.A.shape[0]
    dev = storage == "device"
    x1 = xa + (T.f32(d.P) if dev and d.sell_p else d.P) @ xc
    return x1, x1[:nvo] + d.w[:nvo] * (b[:nvo] - (T.f32(d.A) if dev and d.sell_post else d.A) @ x1)


def _gather(ranks, owned_vals, shape):
    out = np.zeros(shape)
    for R, v in zip(ranks, owned_vals):
        out[np.asarray(R.part.l2g[: R.part.nvo], dtype=np.int64)] = v
    return out


def dist_pressure_cycle(ranks, hLg, y_owned, ghost_rhs, storage="fp64", fused=True, xc_override=None):
    """The distributed pressure cycle on the owned right-hand sides y_owned[r]; returns (t_owned per rank, details).  details: b, xa, r per
    rank, the coarse right-hand side bc (summed in rank order) and x_c.  xc_override: a coarse correction to use in place of the cycle's own."""
    nvg = hLg.levels[0].n
    y_g = _gather(ranks, y_owned, nvg)
    bs, xas, rs = [], [], []
    bc = np.zeros(hLg.levels[1].n)
    for R, y in zip(ranks, y_owned):
        nvo, nv = R.part.nvo, R.part.nvo + R.part.ng
        b = np.zeros(nv)
        b[:nvo] = y
        if ghost_rhs:
            b[nvo:] = y_g[np.asarray(R.part.l2g[nvo:], dtype=np.int64)]
        xa, r = dist_down(R.dl0, b, storage)
        bc = bc + R.dl0.PT @ r
        bs.append(b), xas.append(xa), rs.append(r)
    xc = coarse_cycle(hLg, bc, storage, fused) if xc_override is None else xc_override
    ts = [dist_up(R.dl0, b, xa, xc, storage)[1] for R, b, xa in zip(ranks, bs, xas)]
    return ts, dict(b=bs, xa=xas, r=rs, bc=bc, xc=xc)


def action(ranks, hLg, ru_g, rp_g, schur_full, degree, singular, cycle, storage="fp64", dl0_ghost_rhs=False, ras_ghost_rhs=True, coarse_fused=True):
    """z = P^-1 r of a partitioned pc_type 1 context, all ranks at once.  ru_g [nvg, dim], rp_g [nvg]; cycle(H, b): one V-cycle of hierarchy H.
    Returns (zu_g [nvg, dim], zp_g [nvg]) assembled from the owned parts."""
    nvg, dim = len(rp_g), ranks[0].dim
    own = [np.asarray(R.part.l2g[: R.part.nvo], dtype=np.int64) for R in ranks]
    loc = [np.asarray(R.part.l2g, dtype=np.int64) for R in ranks]
    ru = [ru_g[o] for o in own]
    rp = [rp_g[o] for o in own]

    def VA(R, b):
        return cycle(R.hA, b)

    yu = None
    if schur_full == 2:
        tp = rp
    else:
        yu = [VA(R, b) for R, b in zip(ranks, ru)]
        yu_g = _gather(ranks, yu, (nvg, dim))
        tp = [p - R.A10 @ yu_g[l].reshape(-1) for R, p, l in zip(ranks, rp, loc)]
    zH = []
    for R, t in zip(ranks, tp):
        if degree == 2 and R.fused_h:
            zH.append(T.chebyshev2_weighted(R.Hlev, t, storage))
        else:
            zH.append(T.chebyshev(R.Hlev, t, degree))
    y = [R.ml * z for R, z in zip(ranks, zH)]
    if all(R.dl0 is not None for R in ranks):
        t, _ = dist_pressure_cycle(ranks, hLg, y, dl0_ghost_rhs, storage, coarse_fused)
    else:
        t_g = cycle(hLg, y[0] if len(ranks) == 1 and np.array_equal(own[0], np.arange(nvg)) else _gather(ranks, y, nvg))
        t = [t_g[o] for o in own]
    zp = [np.where((np.asarray(R.pbc).astype(np.int64) & 1) != 0, p, R.alpha * tt + R.beta * z) for R, p, tt, z in zip(ranks, tp, t, zH)]
    if schur_full:
        zp_g = _gather(ranks, zp, nvg)
        tu = [u - (R.A01 @ zp_g[l]).reshape(-1, dim) for R, u, l in zip(ranks, ru, loc)]
        if schur_full == 2 and any(R.ras for R in ranks):
            tu_g = _gather(ranks, tu, (nvg, dim))
            zu = []
            for R, u, l in zip(ranks, tu, loc):
                ext = tu_g[l]
                ext[: R.part.nvo] = u
                if not ras_ghost_rhs:
                    ext[R.part.nvo:] = 0.0
                zu.append(VA(R, ext)[: R.part.nvo])
        else:
            zu = [VA(R, u) for R, u in zip(ranks, tu)]
    else:
        zu = yu
    zp_g = _gather(ranks, zp, nvg) if len(ranks) > 1 or not np.array_equal(own[0], np.arange(nvg)) else zp[0]
    if singular:
        zp_g = zp_g - zp_g.mean()
    return _gather(ranks, zu, (nvg, dim)), zp_g


def sweeps_bound(H, b, l=0):
    """(c, k) of the sweep cycle as amg_twin.vcycle_bound gives them for the composite one: every operator by its absolute value, every
    difference by a sum; k the summed lengths of the longest rows a result passes through."""
    L = H.levels[l]
    w = np.abs(L.w)
    if l == len(H.levels) - 1:
        if H.X is not None:
            return np.abs(H.X) @ b, H.X.shape[0]
        xa = w * b
        return xa + w * (b + abs(L.A) @ xa), 2 * int(np.diff(L.A.indptr).max()) + 2
    A, P = abs(L.A), abs(sp.csr_matrix(L.P))
    xa = w * b
    xc, k = sweeps_bound(H, P.T @ (b + A @ xa), l + 1)
    x1 = xa + P @ xc
    return x1 + w * (b + A @ x1), k + 2 * int(np.diff(L.A.indptr).max()) + int(np.diff(P.indptr).max()) + int(np.diff(P.T.tocsr().indptr).max()) + 4


def interface_rows(A0, owner, rings=1):
    """Global rows within `rings` graph neighbours (pattern of A0) of a vertex owned by another rank."""
    S = T.structure(A0).tocoo()
    cut = owner[S.row] != owner[S.col]
    mark = np.zeros(A0.shape[0], dtype=bool)
    mark[S.row[cut]] = True
    G = T.structure(A0)
    for _ in range(rings - 1):
        mark = mark | ((G @ mark.astype(np.float64)) > 0)
    return mark


def extended_proxy(owned_rows, parts, r):
    """The overlapping velocity proxy of rank r as the ghost-row exchange builds it: its own owned rows (owned_rows[r], [nvo x nv_r], local
    columns) and, for every ghost, the owned row of its owner with the columns that are local to r (by global id), ascending; exact zeros
    off the diagonal dropped."""
    me = parts[r]
    nvo, nv = me.nvo, me.nvo + me.ng
    nvg = len(me.g2l)
    owner_of = -np.ones(nvg, dtype=np.int64)
    for q, p in enumerate(parts):
        owner_of[np.asarray(p.l2g[: p.nvo], dtype=np.int64)] = q
    rows, cols, vals = [], [], []
    C = sp.csr_matrix(owned_rows[r]).tocoo()
    rows.append(C.row), cols.append(C.col), vals.append(C.data)
    for g in range(me.ng):
        gid = int(me.l2g[nvo + g])
        q = int(owner_of[gid])
        M = sp.csr_matrix(owned_rows[q])
        i = int(parts[q].g2l[gid])
        cg = np.asarray(parts[q].l2g, dtype=np.int64)[M.indices[M.indptr[i]:M.indptr[i + 1]]]
        lc = me.g2l[cg]
        keep = lc >= 0
        rows.append(np.full(keep.sum(), nvo + g)), cols.append(lc[keep]), vals.append(M.data[M.indptr[i]:M.indptr[i + 1]][keep])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    keep = (vals != 0.0) | (rows == cols)
    return T.canonical(sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(nv, nv)))


# ---------------------------------------------------------------------------------------------------------------- level-0 formulas
def jacobian_blocks(J, dim, nr, nc):
    """A01 [dim nr x nc], A10 [nr x dim nc], A11 [nr x nc] of a monolithic Jacobian with nr row vertices and nc column vertices
    ([u vertex-interleaved | p] on both sides)."""
    J = sp.csr_matrix(J)
    return J[: dim * nr, dim * nc:].tocsr(), J[dim * nr:, : dim * nc].tocsr(), J[dim * nr:, dim * nc:].tocsr()


def proxy_rows(J, dim, nr, nc):
    """Scalar proxy of the velocity block: mean of the diagonal entries of every dim x dim vertex block, exact zeros off the diagonal
    dropped; returns (values, bound, depth) on [nr x nc]."""
    C = sp.csr_matrix(J)[: dim * nr, : dim * nc].tocoo()
    vel = C.row % dim == C.col % dim
    S = T.canonical(sp.csr_matrix((C.data[vel] / dim, (C.row[vel] // dim, C.col[vel] // dim)), shape=(nr, nc)))
    Sb = T.canonical(sp.csr_matrix((np.abs(C.data[vel]) / dim, (C.row[vel] // dim, C.col[vel] // dim)), shape=(nr, nc)))
    Cs = S.tocoo()
    keep = (Cs.row == Cs.col) | (Cs.data != 0.0)
    proxy = T.canonical(sp.csr_matrix((Cs.data[keep], (Cs.row[keep], Cs.col[keep])), shape=(nr, nc)))
    return proxy, T.restrict(Sb, proxy), dim


def lumped_mass(x, cells):
    import pcd_twin as P
    d = np.asarray(x).shape[1]
    _, vol = P.geometry(np.asarray(x)[:, :d], cells)
    ml = np.zeros(len(x))
    np.add.at(ml, np.asarray(cells).ravel(), np.repeat(vol / (d + 1), d + 1))
    return ml


def dirichlet_laplacian(x, cells, pbc):
    """The P1 stiffness with identity rows and dropped columns on the flagged vertices (the level-0 operator of the pressure hierarchies);
    returns (values, bound, depth), the bound as tests/test_gpu_amg.py takes it: vol |grad phi_a| |grad phi_b| per cell."""
    import pcd_twin as P
    x = np.asarray(x)
    d, nv = x.shape[1], len(x)
    g, vol = P.geometry(x, cells)
    Lp = T.canonical(P._scatter(np.asarray(cells), vol[:, None, None] * np.einsum("cai,cbi->cab", g, g), nv))
    gn = np.linalg.norm(g, axis=2)
    Lb = T.canonical(P._scatter(np.asarray(cells), vol[:, None, None] * gn[:, :, None] * gn[:, None, :], nv))
    cnt = int(P._scatter(np.asarray(cells), np.ones((len(cells), d + 1, d + 1)), nv).data.max())
    on = np.asarray(pbc) == 0
    eye = sp.csr_matrix((np.ones((~on).sum()), (np.nonzero(~on)[0], np.nonzero(~on)[0])), shape=(nv, nv))
    return T.add_keep(T._filter(Lp, on, on), eye), T.add_keep(T._filter(Lb, on, on), eye), cnt * d


def action_bound(ranks, hLg, ru_g, rp_g, schur_full, degree):
    """(c_u [nvg, dim], c_p [nvg], k) of the partitioned action as amg_twin.cc_bound gives them on one rank: every operator by its absolute
    value, every difference by a sum (the ghost layers always filled: an upper bound for both settings of the two switches), k the summed
    lengths of the longest rows a result passes through, the largest over the ranks at every stage."""
    nvg, dim = len(rp_g), ranks[0].dim
    own = [np.asarray(R.part.l2g[: R.part.nvo], dtype=np.int64) for R in ranks]
    loc = [np.asarray(R.part.l2g, dtype=np.int64) for R in ranks]
    ru = [np.abs(ru_g[o]) for o in own]
    rp = [np.abs(rp_g[o]) for o in own]
    k = 0

    def rowmax(M):
        M = sp.csr_matrix(M)
        return int(np.diff(M.indptr).max()) if M.nnz else 0

    def VB(Hs, bs):
        nonlocal k
        res = [T.vcycle_bound(H, b) for H, b in zip(Hs, bs)]
        k += max(q[1] for q in res)
        return [q[0] for q in res]

    hAs = [R.hA for R in ranks]
    yu = None
    if schur_full == 2:
        tp = rp
    else:
        yu = VB(hAs, ru)
        yu_g = _gather(ranks, yu, (nvg, dim))
        tp = [p + abs(R.A10) @ yu_g[l].reshape(-1) for R, p, l in zip(ranks, rp, loc)]
        k += max(rowmax(R.A10) for R in ranks)
    xs = []
    kk = 0
    for R, t in zip(ranks, tp):
        L = R.Hlev
        theta, delta = 0.5 * (L.lmax + L.lmin), 0.5 * (L.lmax - L.lmin)
        sigma = theta / delta
        rho = 1.0 / sigma
        d = np.maximum(np.abs(L.dinv) / theta, np.abs(L.w)) * t
        x, res, kk = d.copy(), t.copy(), 0
        for _ in range(1, max(degree, 2)):
            rho_new = 1.0 / (2.0 * sigma - rho)
            res = res + abs(L.A) @ d
            d = abs(rho_new * rho) * d + abs(2.0 * rho_new / delta) * (np.abs(L.dinv) * res)
            x = x + d
            rho = rho_new
            kk += rowmax(L.A) + 4
        xs.append(x)
    k += kk
    y = [np.abs(R.ml) * x for R, x in zip(ranks, xs)]
    y_g = _gather(ranks, y, nvg)
    if all(R.dl0 is not None for R in ranks):
        bs, xas = [], []
        bc = np.zeros(hLg.levels[1].n)
        for R, l in zip(ranks, loc):
            d0 = R.dl0
            b = y_g[l]
            xa = np.abs(d0.w) * b
            bc = bc + abs(d0.PT) @ (b[: R.part.nvo] + abs(d0.A) @ xa)
            bs.append(b), xas.append(xa)
        xc, kc = T.vcycle_bound(_sub_hierarchy(hLg, 1), bc)
        t = []
        for R, b, xa in zip(ranks, bs, xas):
            d0 = R.dl0
            x1 = xa + abs(d0.P) @ xc
            t.append(x1[: R.part.nvo] + np.abs(d0.w[: R.part.nvo]) * (b[: R.part.nvo] + abs(d0.A) @ x1))
        k += kc + max(2 * rowmax(R.dl0.A) + rowmax(R.dl0.P) + rowmax(R.dl0.PT) + 4 for R in ranks) + len(ranks)
    else:
        t_g, kc = T.vcycle_bound(hLg, y_g)
        k += kc
        t = [t_g[o] for o in own]
    zp = [np.maximum(p, abs(R.alpha) * tt + abs(R.beta) * x) for R, p, tt, x in zip(ranks, tp, t, xs)]
    zp_g = _gather(ranks, zp, nvg)
    if schur_full:
        tu = [u + (abs(R.A01) @ zp_g[l]).reshape(-1, dim) for R, u, l in zip(ranks, ru, loc)]
        k += max(rowmax(R.A01) for R in ranks)
        if schur_full == 2 and any(R.ras for R in ranks):
            tu_g = _gather(ranks, tu, (nvg, dim))
            zu = [q[: R.part.nvo] for R, q in zip(ranks, VB(hAs, [tu_g[l] for l in loc]))]
        else:
            zu = VB(hAs, tu)
    else:
        zu = yu
    return _gather(ranks, zu, (nvg, dim)), zp_g, k


def global_cycle_level0_sweeps(hLg, b, storage="fp64", fused=True):
    """One cycle of the replicated hierarchy with level 0 sweep by sweep on its fp64 operator and the levels 1.. as `coarse_cycle`: what the
    distributed level computes when the right-hand side is present on the ghosts -- stated on the whole mesh, without any partition."""
    L = hLg.levels[0]
    xa = L.w * b
    xc = coarse_cycle(hLg, L.P.T @ (b - L.A @ xa), storage, fused)
    x1 = xa + L.P @ xc
    return x1 + L.w * (b - L.A @ x1)
