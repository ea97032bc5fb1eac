"""What tests/test_gpu_amg.py and tests/test_gpu_part_pc.py share: a built hierarchy read through cfdh_get_amg_operator / cfdh_get_amg_vectors
(or through a recorded dump of those calls: anything with the two methods of _lib.Context serves as `ctx`) checked level by level against
the twin (tests/amg_twin.py), and the twin-side copies of the device operators that the action gates apply."""
import numpy as np
import scipy.sparse as sp

import amg_twin as T

from cfd_hemodynamic_amd import _lib

HA, HL, HH = _lib.AMG_HIER_A, _lib.AMG_HIER_P, _lib.AMG_HIER_H
OPS = {"A": _lib.AMG_OP_A, "P": _lib.AMG_OP_P, "G": _lib.AMG_OP_G, "Sb": _lib.AMG_OP_SB, "Sc": _lib.AMG_OP_SC}


def shape_of(ctx, hier):
    s = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_SHAPE)
    nl = int(s[0])
    lev = [dict(n=int(q[0]), Dn=int(q[1]), fine=bool(q[2]), sell=bool(q[3]), agg=bool(q[4])) for q in s[4:].reshape(nl, 5)]
    return dict(nl=nl, coarse_n=int(s[1]), ncol=int(s[2]), fused=bool(s[3]), lev=lev)


def _raw(ctx, hier, l, nm):
    return ctx.get_amg_operator(hier, l, OPS[nm], raw=True)


def _mat(raw):
    return sp.csr_matrix((raw[2], raw[1], raw[0]), shape=raw[3])


def _assert(v, log=None):
    if log is not None:
        log.append(v)
    assert v.ratio <= 1.0, v.where + " (%.3g times the bound)" % v.ratio


def hier_singular(c, hier):
    if hier == HA:
        return False
    if hier == _lib.AMG_HIER_PG:     # the replicated pressure space of a partitioned run: singular without a Dirichlet node anywhere
        return bool(c.pg_singular)
    if c.opt.pc_type == 0:
        return c.singular or not c.has_pbc
    pbc = c.ctx.get_amg_vectors(HL, 0, _lib.AMG_VEC_CC_PBC)
    return c.singular or not (pbc != 0).any()


def check_hierarchy(c, hier, label, report):
    """Every level of one hierarchy against the twin; returns the twin-side Hierarchy assembled from the verified device operators."""
    ctx = c.ctx
    sh = shape_of(ctx, hier)
    assert sh["fused"], "the fused cycle is what this test is about"
    ratio = c.opt.amg_smooth_ratio
    H = T.Hierarchy()
    H.singular = hier_singular(c, hier)
    worst = {}

    def op_check(nm, raw, triple):
        v = T.check_operator("%s %s level %d %s" % (c.name, label, l, nm), raw, triple)
        worst[nm] = max(worst.get(nm, 0.0), v.ratio)
        _assert(v)

    for l in range(sh["nl"]):
        info = sh["lev"][l]
        rawA = _raw(ctx, hier, l, "A")
        _assert(T.check_csr("%s %s level %d A" % (c.name, label, l), rawA[0], rawA[1], rawA[3], rawA[4]))
        assert rawA[3] == (info["n"], info["n"])
        lam = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_LAMBDA)
        L = T.Level(_mat(rawA), ratio=ratio, lm=lam[0] / 1.1)
        L.lmax, L.lmin = lam[0], lam[1]     # the device's own: every formula below uses them
        L.w = T.jacobi_weights(L.A, L.dinv, L.lmax, L.lmin)
        L.fine, L.sell = info["fine"], info["sell"]
        order = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_ORDER)
        assert np.array_equal(np.sort(order), np.arange(L.n)) and (l == 0 or np.array_equal(order, np.arange(L.n)))
        _assert(T.check_lmax("%s %s level %d" % (c.name, label, l), lam[0], lam[1], L, ratio, order))
        dinv, wdinv = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_DINV), ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_WDINV)
        _assert(T.check_weights("%s %s level %d" % (c.name, label, l), dinv, wdinv, L))
        H.levels.append(L)
        if l == sh["nl"] - 1:
            break
        rawP = _raw(ctx, hier, l, "P")
        na = rawP[3][1]
        assert na == sh["lev"][l + 1]["n"], "the aggregates number the next level"
        if info["agg"]:
            agg = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_AGG)
            _assert(T.check_aggregates("%s %s level %d aggregates" % (c.name, label, l), L.A, agg, na, c.theta))
            L.agg = agg.astype(np.int64)
            op_check("P", rawP, T.prolongator(L.A, L.dinv, L.lm, L.agg, na))
        elif c.etype != 1:
            # host-built hierarchy (pc_type 0): the aggregates are not kept, P is an input of the formulas below
            assert c.opt.pc_type == 0
            _assert(T.check_csr("%s %s level %d P" % (c.name, label, l), rawP[0], rawP[1], rawP[3], rawP[4]))
        else:
            # P2: the exact P1 interpolation; its columns are stored in the library's own vertex order, read off the vertex rows
            assert c.etype == 1 and l == 0
            Pt, verts = T.p1_interpolation(c.mesh.x, c.mesh.cells, c.dim + 1)
            _assert(T.check_csr("%s %s P1 interpolation" % (c.name, label), rawP[0], rawP[1], rawP[3], rawP[4]))
            Pd = _mat(rawP)
            first = Pd.indptr[verts]
            assert (np.diff(Pd.indptr)[verts] == 1).all() and (Pd.data[first] == 1.0).all()
            order = Pd.indices[first]
            assert np.array_equal(np.sort(order), np.arange(na))
            Pt = T.canonical(Pt @ sp.csr_matrix((np.ones(na), (np.arange(na), order)), shape=(na, na)))
            op_check("P", rawP, (Pt, abs(Pt), 1))
        L.P = _mat(rawP)
        tw = T.composites(L.A, L.P, L.w)
        raws = {nm: _raw(ctx, hier, l, nm) for nm in ("G", "Sb", "Sc")}
        for nm in ("G", "Sb", "Sc"):
            op_check(nm, raws[nm], tw[nm])
            setattr(L, nm, _mat(raws[nm]))
        op_check("A_c", _raw(ctx, hier, l + 1, "A"), tw["Ac"])
    last = H.levels[-1]
    res = None
    if sh["coarse_n"] > 0:
        n = sh["coarse_n"]
        assert n == last.n
        H.X = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_COARSE_INV).reshape(n, n)
        res = (T.coarse_residual(last.A, np.linalg.inv(T.coarse_matrix(last.A, H.singular)), H.singular),
               T.coarse_residual(last.A, H.X, H.singular))
        assert res[1] <= COARSE_FACTOR * res[0], "%s %s: |A_c X - I| = %.3g, numpy.linalg.inv reaches %.3g" % (c.name, label, res[1], res[0])
        U = H.levels[-2] if sh["nl"] >= 2 else None
        if U is not None and sh["lev"][-2]["Dn"] > 0:
            assert sh["lev"][-2]["Dn"] == n
            U.D = ctx.get_amg_vectors(hier, sh["nl"] - 2, _lib.AMG_VEC_D).reshape(U.n, n)
            v = T.check_fold("%s %s D" % (c.name, label), U.D, U.Sc, H.X)
            worst["D"] = v.ratio
            _assert(v)
    else:
        rawS = _raw(ctx, hier, sh["nl"] - 1, "Sb")
        W = T.diag(last.w)
        v = T.check_operator("%s %s closing Sb" % (c.name, label), rawS, (T.on_pattern(2.0 * W - W @ last.A @ W, last.A),
                                                                         T.on_pattern(2.0 * W + W @ abs(last.A) @ W, last.A), 2))
        worst["Sb(last)"] = v.ratio
        _assert(v)
        last.Sb = _mat(rawS)
    rows = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_SPGEMM_ROWS)
    report.append("%s %s: levels %s%s; SpGEMM rows hash %d small %d dense %d; worst ratio to the bound %s; coarse inverse residual numpy %s device %s"
                  % (c.name, label, [q["n"] for q in sh["lev"]], "" if sh["coarse_n"] else " (closed by Sb)", rows[0], rows[1], rows[2],
                     {k: float("%.3g" % v) for k, v in worst.items()}, *(("%.3g" % res[0], "%.3g" % res[1]) if res else ("-", "-"))))
    H.ncol, H.rows = sh["ncol"], rows
    return H


# |A_c X - I|_max of the device's Gauss-Jordan inverse (no pivoting) over that of numpy.linalg.inv on the same matrix: the next power of
# two at or above 4 x the worst ratio of the first GPU run, 8.6 (DESIGN.md section 6 lists the residuals per case)
COARSE_FACTOR = 64.0


def twin_hierarchy(c, hier):
    """The twin-side Hierarchy from the device operators as they are (no checks): used after option changes rebuilt a hierarchy."""
    ctx = c.ctx
    sh = shape_of(ctx, hier)
    H = T.Hierarchy()
    H.singular = hier_singular(c, hier)
    for l in range(sh["nl"]):
        L = T.Level.__new__(T.Level)
        L.A = ctx.get_amg_operator(hier, l, OPS["A"])
        L.n = L.A.shape[0]
        L.w = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_WDINV)
        L.dinv = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_DINV)
        L.lmax, L.lmin = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_LAMBDA)
        L.fine, L.sell = sh["lev"][l]["fine"], sh["lev"][l]["sell"]
        if sh["nl"] == 1:     # a hierarchy of one level runs its two Jacobi sweeps on the fp64 operator, not the float32 copy of Sb
            L.fine = L.sell = False
        L.P = L.G = L.Sb = L.Sc = L.D = None
        if l < sh["nl"] - 1 and not sh["fused"]:     # sweep-by-sweep cycle of the host build: transfer operators only
            L.P = ctx.get_amg_operator(hier, l, OPS["P"])
        elif l < sh["nl"] - 1:
            L.P, L.G, L.Sb, L.Sc = (ctx.get_amg_operator(hier, l, OPS[nm]) for nm in ("P", "G", "Sb", "Sc"))
            if sh["lev"][l]["Dn"] > 0:
                L.D = ctx.get_amg_vectors(hier, l, _lib.AMG_VEC_D).reshape(L.n, sh["lev"][l]["Dn"])
        elif sh["coarse_n"] == 0:
            L.Sb = ctx.get_amg_operator(hier, l, OPS["Sb"])
        H.levels.append(L)
    if sh["coarse_n"] > 0:
        H.X = ctx.get_amg_vectors(hier, 0, _lib.AMG_VEC_COARSE_INV).reshape(sh["coarse_n"], sh["coarse_n"])
    H.ncol = sh["ncol"]
    return H


def fp64_copy(H):
    """The same hierarchy with D = Sc X in fp64 (what the device holds is already rounded)."""
    G = T.Hierarchy()
    G.X, G.singular = H.X, H.singular
    for L in H.levels:
        M = T.Level.__new__(T.Level)
        M.__dict__.update(L.__dict__)
        if L.D is not None:
            M.D = np.asarray(L.Sc @ H.X)
        G.levels.append(M)
    return G


def check_h_level(c):
    """dinv, wdinv, lmax, lmin of the single level H against the twin (ratio 8, start vector in the library's numbering)."""
    ctx = c.ctx
    raw = _raw(ctx, HH, 0, "A")
    _assert(T.check_csr("%s H" % c.name, raw[0], raw[1], raw[3], raw[4]))
    lam = ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_LAMBDA)
    L = T.Level(_mat(raw), ratio=8.0, lm=lam[0] / 1.1)
    L.lmax, L.lmin = lam
    L.w = T.jacobi_weights(L.A, L.dinv, lam[0], lam[1])
    order = ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_ORDER)
    assert np.array_equal(np.sort(order), np.arange(L.n))
    _assert(T.check_lmax("%s H" % c.name, lam[0], lam[1], L, 8.0, order))
    _assert(T.check_weights("%s H" % c.name, ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_DINV), ctx.get_amg_vectors(HH, 0, _lib.AMG_VEC_WDINV), L))
