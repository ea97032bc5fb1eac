"""NumPy / SciPy restatement (fp64, no GPU) of the smoothed-aggregation hierarchies and of the Cahouet-Chabard action built from
them -- written from the formulas in csrc/cfdh_internal.hpp (AmgLevel) and csrc/cfdh_amg_dev.hip, not from the host build:

    dinv = 1 / a_ii (1 where the diagonal is absent or zero)          lm = 15 normalised products of D^-1 A from the LCG vector
    lmax = 1.1 lm, lmin = lmax / ratio                                w  = 2 / (lmax + lmin) dinv  (dinv on rows without off-diagonal entry)
    P  = (I - 4 / (3 lm) D^-1 A) T, T the 0/1 matrix of the aggregates, rows of aggregate -1 empty
    G  = P^T (I - A W)      Sb = 2 W - W A W      Sc = (I - W A) P      A_c = P^T A P      D = Sc A_c^-1

Two V-cycles: `vcycle_sweeps` is the textbook damped-Jacobi V(1,1), `vcycle_composite` applies G / Sb / Sc / D the way the fused
kernels do and can round the stored values to float32 exactly where the device stores float32 (accumulation stays fp64).

The checkers return `Violation(ratio, where)`: the worst entrywise violation as a multiple of its bound (<= 1 passes) and its
location, so that a red test names the entry.

Sparse products here keep the full structural pattern (scipy's own product drops sums that cancel to exactly zero, the device
kernels do not), see `spgemm`."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import scipy.sparse as sp

EPS = 2.0 ** -53          # unit roundoff of fp64
U32 = 2.0 ** -24          # unit roundoff of fp32

Violation = namedtuple("Violation", "ratio where")


def gamma(k):
    """gamma_k = k eps / (1 - k eps) of the standard summation bound (Higham, Accuracy and Stability, section 3.1)."""
    return k * EPS / (1.0 - k * EPS)


# ---------------------------------------------------------------------------------------------------------------- level quantities
def lcg_vector(n, seed=0x9E3779B97F4A7C15):
    """Element i = state i + 1 of st <- a st + c (mod 2^64) from the fixed seed, mapped to [-0.5, 0.5)."""
    a, c, m = 6364136223846793005, 1442695040888963407, (1 << 64) - 1
    st = seed
    out = np.empty(n)
    for i in range(n):
        st = (a * st + c) & m
        out[i] = (st >> 11) * (1.0 / 9007199254740992.0) - 0.5
    return out


def diag_inverse(A):
    d = A.diagonal()
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)


def power_lmax(A, dinv, its=15, order=None):
    """lm: norm of the last of `its` normalised products v <- D^-1 A v / |.| from the LCG vector (1 when it degenerates).  order:
    position of every row in the numbering the start vector is indexed by (the library renumbers level 0)."""
    v = lcg_vector(A.shape[0])
    if order is not None:
        v = v[np.asarray(order, dtype=np.int64)]
    lm = 1.0
    for _ in range(its):
        w = dinv * (A @ v)
        lm = np.sqrt(w @ w)
        v = w / lm
    return lm if (lm > 0 and np.isfinite(lm)) else 1.0


def offdiag_count(A):
    """Stored non-zero off-diagonal entries per row."""
    C = A.tocoo()
    keep = (C.row != C.col) & (C.data != 0.0)
    return np.bincount(C.row[keep], minlength=A.shape[0])


def jacobi_weights(A, dinv, lmax, lmin):
    return np.where(offdiag_count(A) == 0, dinv, dinv * (2.0 / (lmax + lmin)))


# ---------------------------------------------------------------------------------------------------------------- sparse helpers
def canonical(A):
    A = sp.csr_matrix(A).copy()
    A.sum_duplicates()
    A.sort_indices()
    return A


def _keys(A):
    A = canonical(A)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    return rows * A.shape[1] + A.indices, A


def structure(A):
    S = canonical(A)
    S.data = np.ones_like(S.data)
    return S


def on_pattern(C, S):
    """The values of C on the pattern S (which contains the pattern of C), zeros elsewhere."""
    ks, S = _keys(S)
    kc, C = _keys(C)
    out = S.copy()
    out.data = np.zeros(len(ks))
    pos = np.searchsorted(ks, kc)
    if len(kc) and (pos.max() >= len(ks) or not np.array_equal(ks[pos], kc)):
        raise ValueError("pattern does not contain the matrix")
    out.data[pos] = C.data
    return out


def restrict(C, S):
    """The values of C on the entries of S (zero where C has none); S need not contain the pattern of C."""
    ks, S = _keys(S)
    kc, C = _keys(C)
    out = S.copy()
    out.data = np.zeros(len(ks))
    pos = np.searchsorted(kc, ks)
    pos[pos >= len(kc)] = 0
    hit = kc[pos] == ks if len(kc) else np.zeros(len(ks), dtype=bool)
    out.data[hit] = C.data[pos[hit]]
    return out


def add_keep(A, B):
    """A + B on the union of the two patterns (scipy's own sum drops entries that come out as exactly zero)."""
    return on_pattern(canonical(A) + canonical(B), structure(A) + structure(B))


def spgemm(*factors):
    """Product of the factors with its full structural pattern, the entrywise bound |A| |B| ... on the same pattern, and the
    depth of the chained sums: the sum of the largest number of products an entry of each partial product receives."""
    S = structure(factors[0])
    C = canonical(factors[0])
    B = abs(C)
    depth = 0
    for F in factors[1:]:
        F = canonical(F)
        cnt = structure(S) @ structure(F)
        depth += int(cnt.data.max()) if cnt.nnz else 0
        S = structure(cnt)
        C = C @ F
        B = B @ abs(F)
    return on_pattern(C, S), on_pattern(B, S), depth


def diag(v):
    return sp.diags(v, format="csr")


# ---------------------------------------------------------------------------------------------------------------- operators
def tentative(agg, na):
    agg = np.asarray(agg, dtype=np.int64)
    i = np.nonzero(agg >= 0)[0]
    return sp.csr_matrix((np.ones(len(i)), (i, agg[i])), shape=(len(agg), na))


def _mask_rows(M, on):
    """Rows with on = 0 removed from the pattern."""
    M = canonical(M)
    keep = np.repeat(np.asarray(on) > 0, np.diff(M.indptr))
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    return sp.csr_matrix((M.data[keep], (rows[keep], M.indices[keep])), shape=M.shape)


def prolongator(A, dinv, lm, agg, na):
    """P = (I - 4 / (3 lm) D^-1 A) T with empty rows where agg = -1; returns (P, bound, depth).  The bound keeps the two terms of
    the left factor apart: (I + omega |D^-1 A|) T."""
    A = canonical(A)
    n = A.shape[0]
    on = np.asarray(agg) >= 0
    I = sp.identity(n, format="csr")
    S = structure(A) + I
    DA = diag(4.0 / 3.0 / lm * dinv) @ A
    M = _mask_rows(on_pattern(I - DA, S), on)
    Mb = _mask_rows(on_pattern(I + abs(DA), S), on)
    T = tentative(agg, na)
    P, _, depth = spgemm(M, T)
    return P, on_pattern(Mb @ T, P), depth


def p1_interpolation(x, cells, nloc_vertices):
    """Exact interpolation from the vertices to the nodes of straight-sided P2 simplices: 1 at a vertex node, 1/2 + 1/2 at an edge
    node, whose two vertices are found from the coordinates (the midpoint of two of the cell's first `nloc_vertices` nodes).
    Columns number the vertex nodes in ascending node order; returns (P [nodes x vertices], the vertex nodes)."""
    x, cells = np.asarray(x, dtype=np.float64), np.asarray(cells, dtype=np.int64)
    verts = np.unique(cells[:, :nloc_vertices])
    cidx = -np.ones(len(x), dtype=np.int64)
    cidx[verts] = np.arange(len(verts))
    rows, cols, vals = [verts], [cidx[verts]], [np.ones(len(verts))]
    h = np.linalg.norm(x[cells[:, 0]] - x[cells[:, 1]], axis=1)
    done = np.zeros(len(x), dtype=bool)
    done[verts] = True
    for q in range(nloc_vertices, cells.shape[1]):
        node = cells[:, q]
        found = np.zeros(len(cells), dtype=bool)
        for a in range(nloc_vertices):
            for b in range(a + 1, nloc_vertices):
                va, vb = cells[:, a], cells[:, b]
                hit = (np.linalg.norm(0.5 * (x[va] + x[vb]) - x[node], axis=1) <= 1e-9 * h) & ~found
                new = hit & ~done[node]
                _, first = np.unique(node[new], return_index=True)
                k = np.nonzero(new)[0][first]
                rows += [node[k], node[k]]
                cols += [cidx[va[k]], cidx[vb[k]]]
                vals += [0.5 * np.ones(len(k)), 0.5 * np.ones(len(k))]
                done[node[k]] = True
                found |= hit
        if not found.all():
            raise ValueError("a node of local index %d is not the midpoint of an edge of its cell" % q)
    P = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(x), len(verts)))
    return canonical(P), verts


def composites(A, P, w):
    """G, Sb, Sc, A_c of a level, each as (values, bound, depth) on its full structural pattern."""
    A, P = canonical(A), canonical(P)
    n = A.shape[0]
    W = diag(w)
    ImAW = on_pattern(sp.identity(n, format="csr") - A @ W, structure(A) + sp.identity(n, format="csr"))
    G = spgemm(P.T.tocsr(), ImAW)
    # bound of G with the two terms of I - A W separated: |P^T| (I + |A| W)
    G = (G[0], on_pattern(abs(P.T.tocsr()) @ (sp.identity(n, format="csr") + abs(A) @ W), structure(G[0])), G[2] + 1)
    Sb_v = on_pattern(2.0 * W - W @ A @ W, structure(A))
    Sb_b = on_pattern(2.0 * W + W @ abs(A) @ W, structure(A))
    AP = spgemm(A, P)
    Sc_v = on_pattern(P - W @ AP[0], structure(AP[0]))
    Sc_b = on_pattern(abs(P) + W @ AP[1], structure(AP[0]))
    Ac = spgemm(P.T.tocsr(), A, P)
    return {"G": G, "Sb": (Sb_v, Sb_b, 2), "Sc": (Sc_v, Sc_b, AP[2] + 1), "Ac": Ac}


def strength_graph(A, theta):
    """Directed strength graph of mis_init_kernel: j is a strong neighbour of i when |a_ij| >= theta sqrt(|a_ii| |a_jj|), j != i."""
    A = canonical(A)
    d = np.abs(A.diagonal())
    C = A.tocoo()
    keep = (C.row != C.col) & (np.abs(C.data) >= theta * np.sqrt(d[C.row] * d[C.col]))
    return sp.csr_matrix((np.ones(keep.sum()), (C.row[keep], C.col[keep])), shape=A.shape)


def greedy_aggregates(A, theta):
    """A simple sequential aggregation: an unaggregated vertex whose strong neighbours are all free founds an aggregate with them,
    leftovers join a neighbouring aggregate, vertices without strong neighbour get -1."""
    S = strength_graph(A, theta)
    S = ((S + S.T) > 0).tocsr()
    n = A.shape[0]
    agg = -np.ones(n, dtype=np.int64)
    na = 0
    for i in range(n):
        nb = S.indices[S.indptr[i]:S.indptr[i + 1]]
        if agg[i] < 0 and len(nb) and (agg[nb] < 0).all():
            agg[i] = na
            agg[nb] = na
            na += 1
    for _ in range(2):
        cur = agg.copy()
        for i in range(n):
            nb = S.indices[S.indptr[i]:S.indptr[i + 1]]
            if cur[i] < 0 and len(nb) and (cur[nb] >= 0).any():
                agg[i] = cur[nb][cur[nb] >= 0].min()
    return agg, na


# ---------------------------------------------------------------------------------------------------------------- hierarchy
class Level:
    """One level: A, dinv, w (= wdinv), lmax, lmin, lm; on all but the last level also agg, P, G, Sb, Sc.  fine / sell: the device's
    float32 storage flags (G in fp32; Sb, Sc in fp32); D: folded dense correction (fp64 here) or None."""

    def __init__(self, A, ratio=4.0, lm=None):
        self.A = canonical(A)
        self.n = A.shape[0]
        self.dinv = diag_inverse(self.A)
        self.lm = power_lmax(self.A, self.dinv) if lm is None else lm
        self.lmax = 1.1 * self.lm
        self.lmin = self.lmax / ratio
        self.w = jacobi_weights(self.A, self.dinv, self.lmax, self.lmin)
        self.agg = self.P = self.G = self.Sb = self.Sc = self.D = None
        self.fine = self.sell = False

    def coarsen(self, agg, na, P=None):
        """Transfer and composite operators for the given aggregates (or a given prolongator); returns A_c."""
        self.agg = agg
        self.P = prolongator(self.A, self.dinv, self.lm, agg, na)[0] if P is None else canonical(P)
        c = composites(self.A, self.P, self.w)
        self.G, self.Sb, self.Sc = c["G"][0], c["Sb"][0], c["Sc"][0]
        return c["Ac"][0]

    def close_with_sb(self):
        self.Sb = on_pattern(2.0 * diag(self.w) - diag(self.w) @ self.A @ diag(self.w), structure(self.A))


class Hierarchy:
    def __init__(self):
        self.levels = []
        self.X = None          # dense inverse of the last operator (None: the last level is closed by x = Sb b)
        self.singular = False


def coarse_matrix(A, singular):
    """Dense last operator; singular hierarchies add sum |a_ii| / n^2 to every entry."""
    D = np.asarray(A.todense(), dtype=np.float64)
    if singular:
        D = D + np.abs(A.diagonal()).sum() / A.shape[0] / A.shape[0]
    return D


def build_hierarchy(A0, theta, max_coarse=50, ratio=4.0, singular=False, aggregate=greedy_aggregates, first_P=None, dense_limit=2500):
    H = Hierarchy()
    H.singular = singular
    A = canonical(A0)
    while True:
        L = Level(A, ratio)
        H.levels.append(L)
        if L.n <= max_coarse or len(H.levels) >= 16:
            break
        if first_P is not None and len(H.levels) == 1:
            A = L.coarsen(None, first_P.shape[1], P=first_P)
            continue
        agg, na = aggregate(A, theta)
        if na >= L.n or na < 1:
            break
        A = L.coarsen(agg, na)
    last = H.levels[-1]
    if last.n > dense_limit:
        last.close_with_sb()
    else:
        H.X = np.linalg.inv(coarse_matrix(last.A, singular))
    return H


def _col(v, b):
    return v[:, None] if b.ndim == 2 else v


def vcycle_sweeps(H, b, l=0):
    """Textbook damped-Jacobi V(1,1): pre-smooth from zero, restrict the residual, recurse, prolong, post-smooth.  b: [n] or [n, ncol]."""
    L = H.levels[l]
    w = _col(L.w, b)
    if l == len(H.levels) - 1:
        if H.X is not None:
            return H.X @ b
        xa = w * b
        return xa + w * (b - L.A @ xa)
    xa = w * b
    r = b - L.A @ xa
    xc = vcycle_sweeps(H, L.P.T @ r, l + 1)
    x1 = xa + L.P @ xc
    return x1 + w * (b - L.A @ x1)


def f32(M):
    """Values rounded to float32 (sparse or dense), held in float64 again: products with them accumulate in fp64."""
    if sp.issparse(M):
        M = M.copy()
        M.data = M.data.astype(np.float32).astype(np.float64)
        return M
    return np.asarray(M).astype(np.float32).astype(np.float64)


def vcycle_composite(H, b, storage="fp64", round_D=True):
    """The same cycle through G / Sb / Sc / D.  storage "device": G of `fine` levels, Sb and Sc of `sell` levels and D are rounded to
    float32, as the device stores them; D = float32(Sc X) from the fp64 Sc (a folded level is never a SELL level).  round_D False
    leaves D alone (a seeded error of the CPU tests)."""
    dev = storage == "device"
    lv = H.levels
    nl = len(lv)
    bs = [b]
    for l in range(nl - 1):
        G = f32(lv[l].G) if dev and lv[l].fine else lv[l].G
        bs.append(G @ bs[l])

    def up(l):
        Sb, Sc = lv[l].Sb, lv[l].Sc
        if dev and lv[l].sell:
            Sb, Sc = f32(Sb), (f32(Sc) if Sc is not None else None)
        return Sb, Sc

    if nl >= 2 and lv[nl - 2].D is not None:
        U = lv[nl - 2]
        x = up(nl - 2)[0] @ bs[nl - 2] + (f32(U.D) if dev and round_D else U.D) @ bs[nl - 1]
        l = nl - 3
    else:
        x = H.X @ bs[nl - 1] if H.X is not None else up(nl - 1)[0] @ bs[nl - 1]
        l = nl - 2
    while l >= 0:
        Sb, Sc = up(l)
        x = Sb @ bs[l] + Sc @ x
        l -= 1
    return x


def vcycle_bound(H, b):
    """(c, k): c = the composite cycle with |G|, |Sb|, |Sc|, |D| (|X|) applied to |b|, k = the summed lengths of the longest rows of
    the operators one result passes through.  Any evaluation order of the cycle in fp64 stays within gamma_k c of any other
    (the standard bound of a chain of matrix-vector products): the floor of the fp32 gate where nothing is stored in fp32."""
    A = Hierarchy()
    A.X = None if H.X is None else np.abs(H.X)
    k = 0 if H.X is None else H.X.shape[0]
    for L in H.levels:
        M = Level.__new__(Level)
        M.fine = M.sell = False
        for nm in ("G", "Sb", "Sc"):
            op = getattr(L, nm)
            setattr(M, nm, None if op is None else abs(op))
            if op is not None and op.nnz:
                k += int(np.diff(op.indptr).max())
        M.D = None if L.D is None else np.abs(L.D)
        if L.D is not None:
            k += L.D.shape[1]
        A.levels.append(M)
    return vcycle_composite(A, np.abs(b)), k


def gate(dev, twin_rounded, twin_fp64, bound=None):
    """The fp32 gate: (distance of dev to the rounded twin, delta32, allowed distance, fp64 floor), all relative to |twin_rounded|.
    Allowed is 0.01 delta32.  Only where nothing on the way is stored in float32 (delta32 = 0) the fp64 floor gamma_(4 k) |c| / |twin| of
    `vcycle_bound` (bound = (c, k)) takes its place: two correct fp64 evaluations cannot be asked to agree more closely."""
    nrm = np.linalg.norm(np.ravel(twin_rounded))
    d32 = float(np.linalg.norm(np.ravel(twin_fp64) - np.ravel(twin_rounded)) / nrm)
    dist = float(np.linalg.norm(np.ravel(dev) - np.ravel(twin_rounded)) / nrm)
    floor = 0.0 if bound is None else gamma(4 * bound[1]) * float(np.linalg.norm(np.ravel(bound[0]))) / nrm
    return dist, d32, (0.01 * d32 if d32 > 0.0 else floor), floor


def fold_dense(H):
    """D = Sc X on the level above a dense last level (the device folds when that level is not a SELL level)."""
    if H.X is not None and len(H.levels) >= 2:
        U = H.levels[-2]
        U.D = np.asarray(U.Sc @ H.X)


# ---------------------------------------------------------------------------------------------------------------- checkers
def check_csr(name, rowptr, col, shape, nnz):
    """Well-formedness of a downloaded CSR: monotone rowptr from 0 to nnz, columns in range and strictly ascending in every row."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    if len(rowptr) != shape[0] + 1 or rowptr[0] != 0:
        return Violation(np.inf, "%s: rowptr has %d entries and starts at %d" % (name, len(rowptr), rowptr[0] if len(rowptr) else -1))
    d = np.diff(rowptr)
    if (d < 0).any():
        return Violation(np.inf, "%s: rowptr decreases at row %d" % (name, int(np.argmax(d < 0))))
    if rowptr[-1] != nnz or len(col) != nnz:
        return Violation(np.inf, "%s: nnz %d, rowptr ends at %d, %d columns" % (name, nnz, rowptr[-1], len(col)))
    bad = (col < 0) | (col >= shape[1])
    rows = np.repeat(np.arange(shape[0]), d)
    if bad.any():
        k = int(np.argmax(bad))
        return Violation(np.inf, "%s: row %d holds column %d outside [0, %d)" % (name, rows[k], col[k], shape[1]))
    if nnz > 1:
        same = rows[1:] == rows[:-1]
        dup = same & (col[1:] == col[:-1])
        if dup.any():
            k = int(np.argmax(dup))
            return Violation(np.inf, "%s: row %d holds column %d twice" % (name, rows[k], col[k]))
        desc = same & (col[1:] < col[:-1])
        if desc.any():
            k = int(np.argmax(desc))
            return Violation(np.inf, "%s: row %d: column %d stored before column %d" % (name, rows[k], col[k], col[k + 1]))
    return Violation(0.0, name)


def raw_csr(M):
    M = sp.csr_matrix(M)
    return M.indptr.copy(), M.indices.copy(), M.data.copy(), M.shape, int(M.indptr[-1])


def check_pattern(name, rowptr, col, twin):
    """The pattern equals the twin's exactly: no dropped and no invented entry (the CSR passed check_csr)."""
    twin = canonical(twin)
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    kd = rows * twin.shape[1] + col
    kt, _ = _keys(twin)
    missing = np.setdiff1d(kt, kd)
    extra = np.setdiff1d(kd, kt)
    if len(missing):
        return Violation(np.inf, "%s: entry (%d, %d) of the twin is missing (%d in all)" % (name, missing[0] // twin.shape[1], missing[0] % twin.shape[1], len(missing)))
    if len(extra):
        return Violation(np.inf, "%s: entry (%d, %d) is not in the twin (%d in all)" % (name, extra[0] // twin.shape[1], extra[0] % twin.shape[1], len(extra)))
    return Violation(0.0, name)


def check_values(name, dev, twin, bound, depth):
    """|dev - twin| <= gamma_(4 depth) bound entrywise on the common pattern; depth: the largest number of products an entry
    receives, the factor 4 covers the chained products inside every term (weights, the I - ... factors)."""
    kd, dev = _keys(dev)
    kt, twin = _keys(twin)
    if not np.array_equal(kd, kt):
        return Violation(np.inf, "%s: patterns differ" % name)
    bound = on_pattern(bound, twin)
    g = gamma(4 * max(int(depth), 1))
    diff = np.abs(dev.data - twin.data)
    lim = g * bound.data
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / lim)
    if not len(ratio):
        return Violation(0.0, name)
    k = int(np.argmax(ratio))
    return Violation(float(ratio[k]), "%s: entry (%d, %d): device %.17g, twin %.17g, bound %.3g" % (
        name, kd[k] // twin.shape[1], kd[k] % twin.shape[1], dev.data[k], twin.data[k], lim[k]))


def check_operator(name, raw, triple):
    """check_csr, check_pattern, check_values in that order; the first that fails is returned."""
    rowptr, col, val, shape, nnz = raw
    twin, bound, depth = triple
    v = check_csr(name, rowptr, col, shape, nnz)
    if v.ratio > 1:
        return v
    if tuple(shape) != tuple(twin.shape):
        return Violation(np.inf, "%s: shape %s, twin %s" % (name, tuple(shape), tuple(twin.shape)))
    v = check_pattern(name, rowptr, col, twin)
    if v.ratio > 1:
        return v
    return check_values(name, sp.csr_matrix((val, col, rowptr), shape=shape), twin, bound, depth)


def ulp_distance(a, b):
    """Largest distance of two float64 arrays in units in the last place."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return int(np.abs(ia - ib).max()) if len(a) else 0


def check_weights(name, dinv, wdinv, L):
    """dinv and wdinv within 1 ulp of the twin level L (built with the device's lmax)."""
    for nm, dv, tw in (("dinv", dinv, L.dinv), ("wdinv", wdinv, L.w)):
        dv = np.asarray(dv)
        ia = np.ascontiguousarray(dv, dtype=np.float64)
        worst = 0
        where = name
        for i in np.nonzero(ia != tw)[0]:
            u = ulp_distance(ia[i:i + 1], tw[i:i + 1])
            if u > worst:
                worst, where = u, "%s: %s[%d] = %.17g, twin %.17g" % (name, nm, i, ia[i], tw[i])
        if worst > 1:
            return Violation(float(worst), where)
    return Violation(0.0, name)


def check_aggregates(name, A, agg, na, theta, connected=True):
    """ids in [-1, na), no empty aggregate, -1 only on rows without strong neighbour, every aggregate connected in the
    (symmetrised) strength graph."""
    agg = np.asarray(agg)
    if (agg != np.round(agg)).any() or agg.min() < -1 or agg.max() >= na:
        return Violation(np.inf, "%s: aggregate ids outside [-1, %d)" % (name, na))
    agg = agg.astype(np.int64)
    cnt = np.bincount(agg[agg >= 0], minlength=na)
    if (cnt == 0).any():
        return Violation(np.inf, "%s: aggregate %d is empty" % (name, int(np.argmax(cnt == 0))))
    S = strength_graph(A, theta)
    has = np.diff(S.indptr) > 0
    bad = (agg < 0) & has
    if bad.any():
        return Violation(np.inf, "%s: row %d has a strong neighbour and no aggregate (%d such rows)" % (name, int(np.argmax(bad)), int(bad.sum())))
    if connected:
        U = ((S + S.T) > 0).tocoo()
        keep = (agg[U.row] == agg[U.col]) & (agg[U.row] >= 0)
        W = sp.csr_matrix((np.ones(keep.sum()), (U.row[keep], U.col[keep])), shape=S.shape)
        ncomp, lab = sp.csgraph.connected_components(W, directed=False)
        per = np.zeros(na, dtype=np.int64)
        seen = np.unique(np.stack([agg[agg >= 0], lab[agg >= 0]], 1), axis=0)
        np.add.at(per, seen[:, 0], 1)
        if (per > 1).any():
            return Violation(np.inf, "%s: aggregate %d falls into %d pieces of the strength graph" % (name, int(np.argmax(per > 1)), int(per.max())))
    return Violation(0.0, name)


def check_lmax(name, lmax, lmin, L, ratio, order=None):
    """lmax within 1e-10 of 1.1 power_lmax (fifteen normalised products of a smooth map), lmin = lmax / ratio."""
    t = 1.1 * power_lmax(L.A, L.dinv, order=order)
    e = abs(lmax - t) / t / 1e-10
    e2 = abs(lmin - lmax / ratio) / (lmax / ratio) / (4 * EPS)
    return Violation(max(e, e2), "%s: lmax %.17g (twin %.17g), lmin %.17g" % (name, lmax, t, lmin))


def coarse_residual(Ac, X, singular):
    """max |A_c X - I| with the trace shift of singular hierarchies."""
    D = coarse_matrix(Ac, singular)
    return float(np.abs(D @ X - np.eye(D.shape[0])).max())


def check_fold(name, D, Sc, X):
    """D = float32(Sc X) within 2^-23 (|Sc| |X|) entrywise; entries below the float32 range may flush to the next subnormal or to
    zero (2^-149, the spacing of float32 at zero, is added to the bound)."""
    t = np.asarray(Sc @ X)
    b = np.asarray(abs(Sc) @ np.abs(X))
    diff = np.abs(np.asarray(D) - t)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(diff == 0.0, 0.0, diff / (2.0 ** -23 * b + 2.0 ** -149))
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return Violation(float(ratio[k]), "%s: D[%d, %d] = %.9g, Sc X = %.9g" % (name, k[0], k[1], np.asarray(D)[k], t[k]))


def rel_distance(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / np.linalg.norm(np.ravel(b)))


# ---------------------------------------------------------------------------------------------------------------- Cahouet-Chabard
def chebyshev(L, b, degree):
    """Chebyshev smoothing of the given degree on a level from a zero guess, with the level's lmax / lmin (degree 1: b / (theta a_ii))."""
    theta, delta = 0.5 * (L.lmax + L.lmin), 0.5 * (L.lmax - L.lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    d = L.dinv * b / theta
    x, r = d.copy(), b.copy()
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        r = r - L.A @ d
        d = rho_new * rho * d + 2.0 * rho_new / delta * (L.dinv * r)
        x = x + d
        rho = rho_new
    return x


def chebyshev2_weighted(L, b, storage="fp64"):
    """The one-pass degree-2 variant of large levels: d = w b, r = b - A d, x = d + c1 d + c2 D^-1 r; the device streams
    float32(a_ij w_j) (rounded after the column-weight product)."""
    theta, delta = 0.5 * (L.lmax + L.lmin), 0.5 * (L.lmax - L.lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    rho_new = 1.0 / (2.0 * sigma - rho)
    AW = L.A @ diag(L.w)
    if storage == "device":
        AW = f32(AW)
    elif storage == "unweighted":   # a seeded error: the float32 copy taken before the column weight
        AW = f32(L.A) @ diag(L.w)
    d = L.w * b
    return d + (rho_new * rho * d + 2.0 * rho_new / delta * (L.dinv * (b - AW @ b)))


class CCOperators:
    """What the Cahouet-Chabard action needs: Hlev (a Level), ml, pbc, alpha, beta, the hierarchies hL and hA, the coupling blocks
    A01 [dim nv x nv], A10 [nv x dim nv], dim, schur_full, degree, singular, and `fused_h` (the one-pass degree-2 smoother)."""


def cc_action(r, op, cycle, storage="fp64", swap_alpha_beta=False):
    """z = P^-1 r of pc_type 1 for r = [u (vertex-interleaved) | p]: schur_full 2 (upper), 1 (full), 0 (lower).  cycle(H, b): one
    V-cycle of hierarchy H; storage: that of the one-pass smoother on H."""
    nv, dim = len(op.ml), op.dim
    ru, rp = r[: dim * nv], r[dim * nv:]

    def VA(b):
        return cycle(op.hA, b.reshape(nv, dim)).reshape(-1)

    yu = None
    if op.schur_full == 2:
        tp = rp
    else:
        yu = VA(ru)
        tp = rp - op.A10 @ yu
    if op.degree == 2 and op.fused_h:
        zH = chebyshev2_weighted(op.Hlev, tp, storage)
    else:
        zH = chebyshev(op.Hlev, tp, op.degree)
    t = cycle(op.hL, op.ml * zH)
    a, b = (op.beta, op.alpha) if swap_alpha_beta else (op.alpha, op.beta)
    zp = np.where((np.asarray(op.pbc).astype(np.int64) & 1) != 0, tp, a * t + b * zH)
    zu = VA(ru - op.A01 @ zp) if op.schur_full else yu
    if op.singular:
        zp = zp - zp.mean()
    return np.concatenate([zu, zp])


def cc_bound(r, op):
    """(c, k) of the whole action as `vcycle_bound` gives them for one cycle: every operator by its absolute value, every
    difference by a sum; k adds the longest rows of the operators a result passes through."""
    nv, dim = len(op.ml), op.dim
    ru, rp = np.abs(r[: dim * nv]), np.abs(r[dim * nv:])
    k = 0

    def VB(H, b):
        nonlocal k
        c, kk = vcycle_bound(H, b)
        k += kk
        return c

    def rowmax(M):
        return int(np.diff(sp.csr_matrix(M).indptr).max())

    L = op.Hlev
    yu = None
    if op.schur_full == 2:
        tp = rp
    else:
        yu = VB(op.hA, ru.reshape(nv, dim)).reshape(-1)
        tp = rp + abs(op.A10) @ yu
        k += rowmax(op.A10)
    theta, delta = 0.5 * (L.lmax + L.lmin), 0.5 * (L.lmax - L.lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    d = np.maximum(np.abs(L.dinv) / theta, np.abs(L.w)) * tp
    x, res = d.copy(), tp.copy()
    for _ in range(1, max(op.degree, 2)):
        rho_new = 1.0 / (2.0 * sigma - rho)
        res = res + abs(L.A) @ d
        d = abs(rho_new * rho) * d + abs(2.0 * rho_new / delta) * (np.abs(L.dinv) * res)
        x = x + d
        rho = rho_new
        k += rowmax(L.A) + 4
    t = VB(op.hL, np.abs(op.ml) * x)
    zp = np.maximum(tp, abs(op.alpha) * t + abs(op.beta) * x)
    if op.schur_full:
        zu = VB(op.hA, (ru + abs(op.A01) @ zp).reshape(nv, dim)).reshape(-1)
        k += rowmax(op.A01)
    else:
        zu = yu
    return np.concatenate([zu, zp]), k


class A00Level:
    """What `chebyshev` needs of the velocity block: A, dinv, lmax, lmin."""

    def __init__(self, A00, lmax, ratio):
        self.A = canonical(A00)
        self.dinv = 1.0 / self.A.diagonal()
        self.lmax, self.lmin = lmax, lmax / ratio


def a00_lmax(A00, dinv, order, dim, its=8):
    """1.15 times the norm of the last of eight normalised products of D^-1 A00 from the LCG vector of seed 0x2545F4914F6CDD1D,
    which is indexed by the library's own numbering (order: position of every node in it)."""
    raw = lcg_vector(dim * len(order), seed=0x2545F4914F6CDD1D).reshape(len(order), dim)
    v = raw[np.asarray(order, dtype=np.int64)].reshape(-1)
    lam = 1.0
    for _ in range(its):
        w = dinv * (A00 @ v)
        lam = np.sqrt(w @ w)
        v = w / lam
    return 1.15 * lam


def selfp_matrix(A11, A10, A01, dinv, dim):
    """S = A11 - A10 D^-1 A01 of pc_type 0 on the library's pattern: the entries of A11 and, for every vertex pair (i, w) whose
    block of A10 D^-1 is not exactly zero, the vertex-graph row of w.  Returns (S, bound, depth)."""
    A11, A10, A01 = canonical(A11), canonical(A10), canonical(A01)
    nv = A11.shape[0]
    B = canonical(A10 @ diag(dinv))
    Bb = on_pattern(abs(A10) @ diag(np.abs(dinv)), A10)
    C = B.tocoo()
    keep = C.data != 0.0
    Mv = structure(sp.csr_matrix((np.ones(keep.sum()), (C.row[keep], C.col[keep] // dim)), shape=(nv, nv)))
    C1 = A01.tocoo()     # the vertex-graph row of w: the stored blocks of A01 in its rows
    Gv = structure(sp.csr_matrix((np.ones(C1.nnz), (C1.row // dim, C1.col)), shape=(nv, nv)))
    pat = structure(A11) + structure(Mv @ Gv)
    cnt = structure(B) @ structure(A01)
    S = on_pattern(on_pattern(A11, pat) - on_pattern(B @ A01, pat), pat)
    return S, on_pattern(abs(A11), pat) + on_pattern(Bb @ abs(A01), pat), int(cnt.data.max()) + 1


def pc0_action(r, op, cycle):
    """z = P^-1 r of pc_type 0: y_u = C(A00) r_u, z_p = V(S)(r_p - A10 y_u), z_u = C(A00)(r_u - A01 z_p) (y_u when schur_full is 0),
    C the Chebyshev solve of op.degree on op.A00lev from a zero guess."""
    nu = op.A00lev.A.shape[0]
    ru, rp = r[:nu], r[nu:]
    yu = chebyshev(op.A00lev, ru, op.degree)
    zp = cycle(op.hS, rp - op.A10 @ yu)
    zu = chebyshev(op.A00lev, ru - op.A01 @ zp, op.degree) if op.schur_full else yu
    if op.singular:
        zp = zp - zp.mean()
    return np.concatenate([zu, zp])


def _cheb_bound(L, b, degree):
    theta, delta = 0.5 * (L.lmax + L.lmin), 0.5 * (L.lmax - L.lmin)
    sigma = theta / delta
    rho = 1.0 / sigma
    d = np.abs(L.dinv) / theta * b
    x, res, k = d.copy(), b.copy(), 2
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        res = res + abs(L.A) @ d
        d = abs(rho_new * rho) * d + abs(2.0 * rho_new / delta) * (np.abs(L.dinv) * res)
        x = x + d
        rho = rho_new
        k += int(np.diff(L.A.indptr).max()) + 4
    return x, k


def pc0_bound(r, op):
    """(c, k) of the pc_type 0 action, as `cc_bound`."""
    nu = op.A00lev.A.shape[0]
    ru, rp = np.abs(r[:nu]), np.abs(r[nu:])
    yu, k = _cheb_bound(op.A00lev, ru, op.degree)
    c, kk = vcycle_bound(op.hS, rp + abs(op.A10) @ yu)
    k += kk + int(np.diff(canonical(op.A10).indptr).max())
    zu = yu
    if op.schur_full:
        zu, k2 = _cheb_bound(op.A00lev, ru + abs(op.A01) @ c, op.degree)
        k += k2 + int(np.diff(canonical(op.A01).indptr).max())
    return np.concatenate([zu, c]), k


def _filter(M, rowmask, colmask):
    C = canonical(M).tocoo()
    k = rowmask[C.row] & colmask[C.col]
    return sp.csr_matrix((C.data[k], (C.row[k], C.col[k])), shape=M.shape)


def h_operator(A11, L, ml_full, pbc, alpha, beta):
    """H = (I + alpha T) M_l + beta A11, T = diag(A11) / diag(L) (0 where diag(L) <= 0); identity on the rows with pbc & 1, their
    columns dropped.  Returns (H, bound)."""
    A11, L = canonical(A11), canonical(L)
    n = A11.shape[0]
    dir_ = (np.asarray(pbc).astype(np.int64) & 1) != 0
    dl = L.diagonal()
    T = np.where(dl > 0, A11.diagonal() / np.where(dl > 0, dl, 1.0), 0.0)
    S = structure(A11) + sp.identity(n, format="csr")
    Hm = on_pattern(beta * A11 + diag((1.0 + alpha * T) * ml_full), S)
    Hb = on_pattern(abs(beta) * abs(A11) + diag((1.0 + abs(alpha * T)) * np.abs(ml_full)), S)
    eye = sp.csr_matrix((np.ones(dir_.sum()), (np.nonzero(dir_)[0], np.nonzero(dir_)[0])), shape=(n, n))
    return add_keep(_filter(Hm, ~dir_, ~dir_), eye), add_keep(_filter(Hb, ~dir_, ~dir_), eye)
