"""Host-side checks of one FGMRES cycle as cfdh_fgmres_solve traces it (tests/test_gpu_fgmres.py), in np.longdouble on the
Jacobian of cfdh_get_csr, and a plain float64 twin of the driver used for the orthogonality constants and for showing that the
checks have teeth (tests/test_fgmres_ref.py).

A cycle is a dict `tr` with
  V [k + 1, n], Z [k, n], H [k + 1, k] (unrotated), y [k], beta, x_start [n], x [n] (the iterate after the cycle),
  res [k] (recurrence residual after each column), second_pass [k], fp32_used.
FGMRES assumes nothing about z_j = P^-1 v_j, so no twin of the preconditioner is needed: every check uses J and the trace only.
Each check returns the largest ratio error / bound (<= 1 passes), so that a test can print the figure before it asserts.

  I1  Arnoldi relation, entrywise per column:  |J z_j - sum_{i <= j+1} H[i, j] v_i|_r
          <= eps (nnz_r (|J| |z_j|)_r + (2 j + 8) (|V_{0..j+1}| |H[:, j]|)_r)
      (the product: nnz_r terms per row, eps = 2 u covers product and sum; the Gram-Schmidt update: j + 1 terms in each of at most
      two passes, the scaling and the rounding of the coefficients h that the host holds against the ones the device applied.)
      fp32 copy of the basis: columns 0 .. j on the right are V.astype(float32) (what the copy holds); a refined column was
      corrected against the fp64 columns, so the difference (V - V32) h2 of size 2^-24 |V| |h| is allowed there.
  I2  start of a cycle:  |beta v_0 - (b - J x_start)|_r <= eps (nnz_r (|J| xmag)_r + 2 |b|_r + 4 |r|_r)  (product, difference, and
      the two roundings of the scaling by 1 / beta); beta against the long-double norm within the norm of that bound plus the
      dot bound of krylov_vec_ref on the sum of squares.  xmag = |x_start|, or |U| |y| for a projected guess (r0 = b - (J U) y).
  I3  least squares: res[j] against min_y |beta e_1 - H_j y| (long-double orthogonalisation) within 100 k eps cond(H_j) beta, the
      bound of test_krylov_host.py::test_recurrence scaled by beta; res non-increasing; |beta e_1 - H_k y| within the same bound.
  I4  update: |x - (x_start + Z y)|_r <= (k + 2) eps (|x_start| + |Z|^T |y|)_r.
  I5  optimality, independent of the basis: rho* = min_y |(b - J x_start) - J Z y|;
      |b - J x| <= sqrt((1 + eV) / (1 - eV)) rho* + 4 eps | nnz o (|J| |x|) + |b| |_2,  eV = |I - V^T V|_2; the recurrence estimate
      and the true residual within the same two terms of each other.  (With the Arnoldi relation exact the residual is
      V (beta e_1 - H y): its norm is within sqrt(1 +- eV) of the recurrence norm, for every y; the second term is the floor of
      a float64 residual.)  Applied where |b - J x| >= 1e-11 |b| and eV < 1.
  I6  orthogonality: refined basis |G_ij - delta_ij| <= 4 dot_bound(n, 1); one classical pass eV <= C eps kappa^2 with kappa the
      condition number of [r_start, J z_0 .. J z_{k-1}] scaled to unit columns (Giraud, Langou, Rozloznik, van den Eshof 2005:
      classical Gram-Schmidt loses orthogonality like eps kappa^2); fp32 copy: 2^-24 in place of eps.  C = 10 x ORTH_TABLE below.
"""
import numpy as np

import krylov_vec_ref as KV
from ipcs_krylov_ref import LD, Mat

EPS = 2.0 ** -52
U32 = 2.0 ** -24

# Largest eV / (unit kappa^2) of the float64 twin below over the cases of tests/test_fgmres_ref.py::ORTH_CASES (seed 20261020: four
# convection-diffusion operators x Jacobi / incomplete LU x natural and permuted summation order, 40 columns, every prefix of
# 3 .. 40 columns with unit kappa^2 < 0.1), rounded up to two digits.  test_fgmres_ref.py re-measures and fails when this is stale.
# The GPU test uses ORTH_FACTOR times these (another summation order, n in the thousands).
ORTH_TABLE = {"fp64": 0.46, "fp32": 0.011}
ORTH_FACTOR = 10.0


def ld(a):
    return np.asarray(a).astype(LD)


def norm(a):
    a = ld(a)
    return np.sqrt(np.sum(a * a))


class System:
    """J with its extended-precision products."""

    def __init__(self, J):
        J = J.tocsr()
        self.J, self.n = J, J.shape[0]
        self.M, self.Mabs = Mat(J, LD), Mat(abs(J), LD)
        self.nnz = ld(np.diff(J.indptr))

    def mul(self, x):
        return self.M(ld(x))

    def mulabs(self, x):
        return self.Mabs(np.abs(ld(x)))

    def floor(self, b, x, factor=4.0):
        return float(factor * EPS * norm(self.nnz * self.mulabs(x) + np.abs(ld(b))))


def _ratio(err, bound):
    """max err / bound over the entries; an entry with a zero bound has to be exact"""
    err, bound = np.abs(ld(err)), ld(bound)
    if err.size == 0:
        return 0.0
    pos = bound > 0
    if (err[~pos] > 0).any():
        return np.inf
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def ld_orth(A):
    """orthonormal basis of the columns of A [n, k], classical Gram-Schmidt applied twice per column in extended precision; a column
    that is dependent on the earlier ones (what is left below 1e-12 of it) is dropped"""
    A = ld(A)
    Q = np.zeros_like(A)
    r = 0
    for j in range(A.shape[1]):
        q = A[:, j].copy()
        n0 = norm(q)
        for _ in range(2):
            q = q - Q[:, :r] @ (Q[:, :r].T @ q)
        nq = norm(q)
        if n0 > 0 and nq > 1e-12 * n0:
            Q[:, r] = q / nq
            r += 1
    return Q[:, :r]


def ld_lsq_residual(A, b):
    """min_y |b - A y|"""
    Q = ld_orth(A)
    r = ld(b).copy()
    for _ in range(2):
        r = r - Q @ (Q.T @ r)
    return float(norm(r))


# ---- the invariants -------------------------------------------------------------------------------------------------------------
def i1_arnoldi(S, tr):
    V, Z, H = ld(tr["V"]), ld(tr["Z"]), ld(tr["H"])
    k = Z.shape[0]
    fp32 = bool(tr.get("fp32_used", False))
    V32 = ld(np.asarray(tr["V"], dtype=np.float64).astype(np.float32)) if fp32 else V
    if k == 0:
        return 0.0
    JZ, JZa = S.mul(Z.T), S.mulabs(Z.T)
    worst = 0.0
    for j in range(k):
        rhs = V32[:j + 1].T @ H[:j + 1, j] + H[j + 1, j] * V[j + 1]
        mag = np.abs(V[:j + 2]).T @ np.abs(H[:j + 2, j])
        bound = EPS * (S.nnz * JZa[:, j] + (2 * j + 8) * mag)
        if fp32 and tr["second_pass"][j]:
            bound = bound + U32 * (np.abs(V[:j + 1]).T @ np.abs(H[:j + 1, j]))
        worst = max(worst, _ratio(JZ[:, j] - rhs, bound))
    return worst


def i2_start(S, b, tr, xmag=None):
    """(entrywise ratio, ratio of beta)"""
    b, x, v0, beta = ld(b), ld(tr["x_start"]), ld(tr["V"][0]), LD(tr["beta"])
    r = b - S.mul(x)
    mag = S.Mabs(np.abs(x) if xmag is None else ld(xmag))
    bound = EPS * (S.nnz * mag + 2 * np.abs(b) + 4 * np.abs(r))
    rn = norm(r)
    bbeta = norm(bound) + KV.dot_bound(S.n, 1.0) * rn
    return _ratio(beta * v0 - r, bound), float(abs(beta - rn) / bbeta) if bbeta > 0 else (0.0 if beta == rn else np.inf)


def lsq_bound(H, j, k, beta):
    return 100.0 * k * EPS * np.linalg.cond(np.asarray(H[:j + 1, :j], dtype=np.float64)) * float(beta)


def i3_lsq(tr):
    H, y, beta = ld(tr["H"]), ld(tr["y"]), LD(tr["beta"])
    res = np.asarray(tr["res"], dtype=np.float64)
    k = H.shape[1]
    worst = 0.0
    prev = float(beta)
    for j in range(1, k + 1):
        e1 = np.zeros(j + 1, dtype=LD)
        e1[0] = beta
        ref = ld_lsq_residual(H[:j + 1, :j], e1)
        worst = max(worst, abs(res[j - 1] - ref) / lsq_bound(H, j, k, beta))
        if not res[j - 1] <= prev:
            return np.inf
        prev = res[j - 1]
        if j == k:
            worst = max(worst, abs(float(norm(e1 - H @ y)) - ref) / lsq_bound(H, j, k, beta))
    return float(worst)


def i4_update(tr):
    Z, y, xs, x = ld(tr["Z"]), ld(tr["y"]), ld(tr["x_start"]), ld(tr["x"])
    k = Z.shape[0]
    bound = (k + 2) * EPS * (np.abs(xs) + np.abs(Z).T @ np.abs(y))
    return _ratio(x - (xs + Z.T @ y), bound)


def gram_defect(V):
    V = ld(V)
    return V @ V.T - np.eye(V.shape[0], dtype=LD)


def eps_v(V):
    return float(np.linalg.norm(np.asarray(gram_defect(V), dtype=np.float64), 2))


def i5_optimal(S, b, tr):
    """(ratio of the true residual against the optimum, ratio of estimate against true residual); None when |r| < 1e-11 |b| or
    eV >= 1, where the bound says nothing"""
    b, x, xs, Z = ld(b), ld(tr["x"]), ld(tr["x_start"]), ld(tr["Z"])
    true = float(norm(b - S.mul(x)))
    if not true >= 1e-11 * float(norm(b)):
        return None
    rho = ld_lsq_residual(S.mul(Z.T), b - S.mul(xs))
    ev = eps_v(tr["V"])
    if ev >= 1.0:
        return None   # the bound is infinite: the basis is lost (I6 caps eV; one classical pass may lose it once eps kappa^2 ~ 1)
    f = np.sqrt((1.0 + ev) / (1.0 - ev))
    floor = S.floor(b, x)
    est = float(tr["res"][-1])
    return true / (f * rho + floor), max(true / (f * est + floor), est / (f * true + floor))


def kappa_unit(S, b, tr):
    """condition number of [r_start, J z_0 .. J z_{k-1}] with unit columns"""
    A = np.column_stack([ld(b) - S.mul(tr["x_start"]), S.mul(ld(tr["Z"]).T)])
    A = A / np.sqrt(np.sum(A * A, axis=0))
    s = np.linalg.svd(np.asarray(A, dtype=np.float64), compute_uv=False)
    return float(s[0] / s[-1]) if s[-1] > 0 else np.inf


def i6_refined(tr):
    n = np.asarray(tr["V"]).shape[1]
    return float(np.abs(gram_defect(tr["V"])).max() / (4.0 * KV.dot_bound(n, 1.0)))


def i6_single(S, b, tr, unit=EPS, key="fp64"):
    """eV / (C unit kappa^2) with C = ORTH_FACTOR x the recorded constant"""
    return eps_v(tr["V"]) / (ORTH_FACTOR * ORTH_TABLE[key] * unit * kappa_unit(S, b, tr) ** 2)


def check_cycle(S, b, tr, refined, xmag=None, label=""):
    """All six invariants of one traced cycle; prints every figure, then asserts."""
    fp32 = bool(tr.get("fp32_used", False))
    r1 = i1_arnoldi(S, tr)
    r2, r2b = i2_start(S, b, tr, xmag)
    r3 = i3_lsq(tr)
    r4 = i4_update(tr)
    r5 = i5_optimal(S, b, tr)
    r6 = i6_refined(tr) if refined else i6_single(S, b, tr, U32 if fp32 else EPS, "fp32" if fp32 else "fp64")
    print("%s k=%d I1 %.3f I2 %.3f beta %.3f I3 %.3g I4 %.3f I5 %s I6(%s) %.3g eV %.2e" % (
        label, len(tr["y"]), r1, r2, r2b, r3, r4, "-" if r5 is None else "%.3f %.3f" % r5, "refined" if refined else "single", r6, eps_v(tr["V"])))
    assert r1 <= 1.0, "I1 Arnoldi relation: %g of the bound" % r1
    assert r2 <= 1.0 and r2b <= 1.0, "I2 start of the cycle: %g, beta %g of the bound" % (r2, r2b)
    assert r3 <= 1.0, "I3 least squares: %g of the bound" % r3
    assert r4 <= 1.0, "I4 update: %g of the bound" % r4
    assert r5 is None or (r5[0] <= 1.0 and r5[1] <= 1.0), "I5 optimality: %s of the bound" % (r5,)
    assert r6 <= 1.0, "I6 orthogonality: %g of the cap" % r6


def guess_check(S, b, Ukept, x0, singular_p=None):
    """Projected guess x0 against the long-double minimiser of |b - J U y| over the span of the kept vectors Ukept [k, n] (independent
    ones).  Returns (|b - J x0|, minimum, allowance): the Gram system G y = g of W = J U is solved with a componentwise backward
    error of 4 k eps (test_krylov_host.py::test_gram_full_rank) from entries that are device dot products ((n + 2) u each), so
    G (y - y*) = d with |d| <= e (|W|^T |W| |y| + |W|^T |b|), e = 4 k eps + (n + 2) u, and
    |b - W y|^2 = min^2 + |W (y - y*)|^2, |W (y - y*)| <= |d| / sigma_min(W); the product J x0 against (J U) y adds the floor of a
    float64 residual on the magnitudes |U|^T |y|.  singular_p: slice of the pressure entries whose mean the device removes from x0.
    Also returns xmag = |U|^T |y| (+ the removed mean) for I2."""
    U = ld(Ukept)
    k = U.shape[0]
    W = S.mul(U.T)
    rmin = ld_lsq_residual(W, b)
    x0 = ld(x0)
    # the device's coefficients: x0 = U y (plus a constant pressure), recovered in extended precision
    A = U.T
    if singular_p is not None:
        one = np.zeros((S.n, 1), dtype=LD)
        one[singular_p] = 1
        A = np.column_stack([A, one])
    Q = ld_orth(A)
    R = Q.T @ A
    c = np.asarray(np.linalg.solve(np.asarray(R, dtype=np.float64), np.asarray(Q.T @ x0, dtype=np.float64)))
    y = ld(c[:k])
    xmag = np.abs(U).T @ np.abs(y) + (np.abs(ld(c[k])) * one[:, 0] if singular_p is not None else 0)
    e = 4 * k * EPS + KV.dot_bound(S.n, 1.0)
    Wa = np.abs(W)
    d = e * float(norm(Wa.T @ (Wa @ np.abs(y)) + Wa.T @ np.abs(ld(b))))
    smin = np.linalg.svd(np.asarray(W, dtype=np.float64), compute_uv=False)[-1]
    allow = d / smin + float(4 * EPS * norm(S.nnz * S.Mabs(xmag) + np.abs(ld(b))))
    return float(norm(ld(b) - S.mul(x0))), rmin, allow, xmag


# ---- float64 twin of the driver ---------------------------------------------------------------------------------------------------
def _dot(a, c, perm):
    return float(np.sum(a * c)) if perm is None else float(np.sum((a * c)[perm]))


def twin_cycle(A, pre, b, x, k, refine=None, fp32=False, perm=None, bug=None, unscaled_v0=False, stop=1e-9):
    """One cycle of at most k columns from x in float64, as fgmres_cycle takes it: z = pre(v_j), w = A z, h = V^T w and w.w from one
    pass, v_{j+1} = (w - V h) / s with s = sqrt(w.w - |h|^2) (the fp32 copy: h against the float32 columns, the norm measured);
    refine None: one pass, 'all': a second pass for every vector, 'dgks': where |w'|^2 <= 0.5 w.w.  The least-squares problem
    in extended precision (the host arithmetic has its own tests); the cycle ends early once the recurrence residual is below
    stop x beta.  bug: one of the driver mistakes of test_fgmres_ref.py, or None."""
    n = len(b)
    r = b - A @ x
    beta = float(np.sqrt(_dot(r, r, perm)))
    V = np.zeros((k + 1, n))
    V32 = np.zeros((k + 1, n), dtype=np.float32)
    Z = np.zeros((k, n))
    H = np.zeros((k + 1, k))
    second = np.zeros(k, dtype=np.int32)
    V[0] = r if unscaled_v0 else r / beta
    V32[0] = V[0]
    for j in range(k):
        Z[j] = pre(V[j])
        w = A @ Z[j]
        B = V32[:j + 1].astype(np.float64) if fp32 else V[:j + 1]
        h = np.array([_dot(B[i], w, perm) for i in range(j + 1)])
        ww = _dot(w, w, perm)
        wp = w - B.T @ h
        if fp32:
            s = float(np.sqrt(_dot(wp, wp, perm)))
            nrm2 = s * s
        else:
            nrm2 = ww - float(h @ h)
            s = float(np.sqrt(nrm2)) if 0.0 < nrm2 <= ww else float(np.sqrt(ww))
        vn = wp / s
        hnorm = float(np.sqrt(max(nrm2, 0.0)))
        if refine == "all" or (refine == "dgks" and not nrm2 > 0.5 * ww):
            second[j] = 1
            h2 = np.array([_dot(V[i], vn, perm) for i in range(j + 1)])
            vv = _dot(vn, vn, perm)
            vn = vn - V[:j + 1].T @ h2
            vnorm = float(np.sqrt(_dot(vn, vn, perm))) if fp32 else float(np.sqrt(max(vv - float(h2 @ h2), 0.0)))
            h = h + s * h2
            hnorm = vnorm if bug == "hnorm" else s * vnorm
            vn = vn / vnorm
        V[j + 1] = vn
        V32[j + 1] = vn
        H[:j + 1, j] = h
        H[j + 1, j] = hnorm
        e1 = np.zeros(j + 2, dtype=LD)
        e1[0] = beta
        if ld_lsq_residual(H[:j + 2, :j + 1], e1) <= stop * beta:
            k = j + 1
            V, V32, Z, H, second = V[:k + 1], V32[:k + 1], Z[:k], H[:k + 1, :k], second[:k]
            break
    if bug == "stale_h" and k >= 3:
        H[:2, 2] = H[:2, 1]  # column 2 read from the slot of iteration 1 (its leading entries; the rest of that slot is not h)
    # least squares in extended precision, residual history from the leading blocks
    res = np.zeros(k)
    for j in range(1, k + 1):
        e1 = np.zeros(j + 1, dtype=LD)
        e1[0] = beta
        res[j - 1] = ld_lsq_residual(H[:j + 1, :j], e1)
    Q = ld_orth(H)
    e1 = np.zeros(k + 1, dtype=LD)
    e1[0] = beta
    R = np.asarray(Q.T @ ld(H), dtype=np.float64)
    y = np.linalg.solve(R, np.asarray(Q.T @ e1, dtype=np.float64))
    xs = x.copy()
    if bug == "zshift":
        xn = xs + np.vstack([Z[1:], np.zeros((1, n))]).T @ y  # y applied to the columns one slot further on
    else:
        xn = xs + Z.T @ y
    return dict(V=V, Z=Z, H=H, y=y, beta=beta, x_start=xs, x=xn, res=res, second_pass=second, fp32_used=fp32)


def twin_solve(A, pre, b, m, rtol, max_cycles=50, refine=None, fp32=False, perm=None, bug=None, bug_cycle=0):
    """Restarted twin: cycles of m columns from the true residual until |b - A x| <= rtol |b|.  The mistake `bug` is made in cycle
    `bug_cycle` only ('v0': V_0 of that cycle is not rescaled).  Returns (x, true residuals per cycle start, traces)."""
    x = np.zeros(len(b))
    bn = float(np.linalg.norm(b))
    traces, betas = [], []
    for c in range(max_cycles):
        rn = float(np.linalg.norm(b - A @ x))
        betas.append(rn)
        if rn <= rtol * bn:
            break
        here = bug if c == bug_cycle else None
        tr = twin_cycle(A, pre, b, x, m, refine, fp32, perm, bug=here if here != "v0" else None, unscaled_v0=here == "v0")
        traces.append(tr)
        x = tr["x"]
    return x, betas, traces
