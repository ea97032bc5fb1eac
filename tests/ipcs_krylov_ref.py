"""Trajectory versions of the three Krylov recurrences of csrc/cfdh_ipcs_krylov.hip, written in the order the drivers and the stage
table of ip_scal_kernel take them, in np.longdouble (or any `dtype`): the references of tests/test_gpu_ipcs_krylov.py.

Each function runs `nit` iterations of ONE cycle from the true residual r_0 = b - A x_0 -- no convergence test, no restart --
and returns a list `tr` with tr[0] the start and tr[k] the state after iteration k, each a dict with
  x      the iterate x_k
  rn2    |r_k|^2 of the recurrence residual (k = 0: of the true residual)
  p      the search direction as the device holds it after iteration k when the solve ends there
  alpha, omega, beta, rho, rz   the scalars as the device holds them after iteration k (see each function).
`A`: scipy CSR (its float64 values are taken exactly); b, x0: [n] or [n, d] (d interleaved columns share the matrix);
`pre`: None for Jacobi with the weights fl64(1 / diag) the device keeps, an array of weights, or a callable.
`perm`: a permutation of range(b.size); the dot products then sum their terms in that order (rounding study).
"""
import numpy as np

LD = np.longdouble


class Mat:
    """CSR product in the working precision (scipy's own matvec is not used: it has no extended-precision path everywhere)."""

    def __init__(self, A, dtype):
        A = A.tocsr()
        A.sort_indices()
        assert (np.diff(A.indptr) > 0).all()
        self.ptr, self.col, self.val = A.indptr[:-1].astype(np.int64), A.indices.astype(np.int64), A.data.astype(dtype)
        self.diag = A.diagonal()

    def __call__(self, x):
        v = self.val if x.ndim == 1 else self.val[:, None]
        return np.add.reduceat(v * x[self.col], self.ptr, axis=0)


def _tools(A, b, x0, pre, dtype, perm):
    M = Mat(A, dtype)
    b, x0 = np.asarray(b).astype(dtype), np.asarray(x0).astype(dtype)
    if perm is None:
        dot = lambda a, c: np.sum(a * c, dtype=dtype)
    else:
        dot = lambda a, c: np.sum((a * c).ravel()[perm], dtype=dtype)
    if pre is None:
        pre = 1.0 / M.diag                      # float64, as the device (dinv1, dinvB) and cfdh_ipcs_host.hpp (dinv3) form dinv
    if not callable(pre):
        w = np.asarray(pre, dtype=np.float64).astype(dtype)
        w = w[:, None] if b.ndim == 2 else w
        pre = lambda v, w=w: w * v
    return M, b, x0, dot, pre


def bicgstab(A, b, x0, nit, pre=None, dtype=LD, perm=None):
    """BiCGStab, right-preconditioned, as ip_bicgstab: rh = r_0, p = v = 0, rho_0 = |r_0|^2, alpha = omega = 1, beta = 0; iteration k:
    p = r + beta (p - omega v), y = pre p, v = A y, alpha = rho / (rh . v), s = r - alpha v, z = pre s, t = A z,
    omega = (t . s) / (t . t) (0 when t . t = 0), x += alpha y + omega z, r = s - omega t, rho_new = rh . r,
    beta = (rho_new / rho) (alpha / omega).  After iteration k the scalars are alpha_k, omega_k, rho = rh . r_k and the beta that
    iteration k + 1 will use."""
    M, b, x, dot, pre = _tools(A, b, x0, pre, dtype, perm)
    one, zero = dtype(1), dtype(0)
    r = b - M(x)
    rh = r.copy()
    p, v = np.zeros_like(b), np.zeros_like(b)
    rho, alpha, omega, beta = dot(r, r), one, one, zero
    tr = [dict(x=x.copy(), rn2=rho, p=p.copy(), alpha=alpha, omega=omega, beta=beta, rho=rho, rz=zero)]
    for _ in range(nit):
        p = r + beta * (p - omega * v)
        y = pre(p)
        v = M(y)
        alpha = rho / dot(v, rh)
        s = r - alpha * v
        z = pre(s)
        t = M(z)
        ts, tt = dot(t, s), dot(t, t)
        omega = ts / tt if tt > 0 else zero
        x = x + (alpha * y + omega * z)
        r = s - omega * t
        rho_new, rn2 = dot(rh, r), dot(r, r)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = (rho_new / rho) * (alpha / omega)
        rho = rho_new
        tr.append(dict(x=x.copy(), rn2=rn2, p=p.copy(), alpha=alpha, omega=omega, beta=beta, rho=rho, rz=zero))
    return tr


def pcg(A, b, x0, nit, pre=None, dtype=LD, perm=None):
    """Preconditioned CG as ip_cg<D, true>: z = pre r, p = z, rz = r . z; iteration k: q = A p, alpha = rz / (q . p), x += alpha p,
    r -= alpha q, z = pre r, beta = (r . z) / rz, rz = r . z, p = z + beta p.  After iteration k: alpha_k, rz = r_k . z_k, the beta
    that formed the direction of iteration k + 1, and p that direction."""
    M, b, x, dot, pre = _tools(A, b, x0, pre, dtype, perm)
    r = b - M(x)
    z = pre(r)
    p = z.copy()
    rz = dot(r, z)
    tr = [dict(x=x.copy(), rn2=dot(r, r), p=p.copy(), alpha=dtype(1), omega=dtype(1), beta=dtype(0), rho=dtype(0), rz=rz)]
    for _ in range(nit):
        q = M(p)
        alpha = rz / dot(q, p)
        x = x + alpha * p
        r = r - alpha * q
        z = pre(r)
        rz_new, rn2 = dot(r, z), dot(r, r)
        beta = rz_new / rz
        rz = rz_new
        p = z + beta * p
        tr.append(dict(x=x.copy(), rn2=rn2, p=p.copy(), alpha=alpha, omega=dtype(1), beta=beta, rho=dtype(0), rz=rz))
    return tr


def fpcg(A, b, x0, nit, pre, dtype=LD, perm=None):
    """Flexible PCG as ip_cg<1, false>: z = pre r, p = z, rz = r . z; iteration k: q = A p, alpha = rz / (q . p), x += alpha p,
    r -= alpha q, |r|^2 -- and only when another iteration follows: z = pre r, beta = -alpha (q . z) / rz, rz = r . z,
    p = z + beta p.  So after iteration k the device holds alpha_k, the beta that formed the direction OF iteration k (0 for
    k = 1), rz = r_{k-1} . z_{k-1} and that direction; `pre` (a callable taking and returning float64) is called once per entry."""
    user = pre
    M, b, x, dot, pre = _tools(A, b, x0, pre, dtype, perm)
    if callable(user):
        pre = lambda v: np.asarray(user(np.asarray(v, dtype=np.float64))).astype(dtype)
    r = b - M(x)
    z = pre(r)
    p = z.copy()
    rz, beta = dot(r, z), dtype(0)
    tr = [dict(x=x.copy(), rn2=dot(r, r), p=p.copy(), alpha=dtype(1), omega=dtype(1), beta=beta, rho=dtype(0), rz=rz)]
    for k in range(nit):
        if k > 0:
            z = pre(r)
            beta = -alpha * dot(q, z) / rz
            rz = dot(r, z)
            p = z + beta * p
        q = M(p)
        alpha = rz / dot(q, p)
        x = x + alpha * p
        r = r - alpha * q
        tr.append(dict(x=x.copy(), rn2=dot(r, r), p=p.copy(), alpha=alpha, omega=dtype(1), beta=beta, rho=dtype(0), rz=rz))
    return tr


DRIVERS = (bicgstab, fpcg, pcg)                      # by `which` of cfdh_ipcs_krylov_solve
SCALARS = (("alpha", "omega", "beta", "rho"), ("alpha", "beta", "rz"), ("alpha", "beta", "rz"))


def rel(a, b):
    """|a - b| / |b| for scalars, max|a - b| / max|b| for vectors, in extended precision."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / den) if den > 0 else float(np.abs(a - b).max())


def spread(which, A, b, x0, nit, pre=None, seed=0):
    """Rounding spread of a float64 run against the extended-precision run over k = 1 .. nit: the float64 run in natural order and
    with the dot products summed in a fixed permuted order, the larger gap of the two.  Returns (iterates, scalars): the largest
    max|x_k - x_k^ref| / max|x_k^ref| and the largest relative difference of the scalars the GPU test compares."""
    fn = DRIVERS[which]
    ref = fn(A, b, x0, nit, pre=pre, dtype=LD)
    perm = np.random.default_rng(seed).permutation(np.asarray(b).size)
    gx = gs = 0.0
    for pm in (None, perm):
        tr = fn(A, b, x0, nit, pre=pre, dtype=np.float64, perm=pm)
        for k in range(1, nit + 1):
            gx = max(gx, rel(tr[k]["x"], ref[k]["x"]))
            gs = max([gs] + [rel(tr[k][s], ref[k][s]) for s in SCALARS[which]])
    return gx, gs


def residual_check(A, b, x, nnz_row_max=None):
    """(|b - A x|, bound) in extended precision: the bound (nnz_row_max + 3) u | |A| |x| + |b| |_2 with u = 2^-53 covers a float64
    evaluation of the residual and of its norm in any summation order."""
    M = Mat(A, LD)
    b, x = np.asarray(b).astype(LD), np.asarray(x).astype(LD)
    r = b - M(x)
    Mabs = Mat(abs(A), LD)
    mag = Mabs(np.abs(x)) + np.abs(b)
    w = int(np.diff(A.tocsr().indptr).max()) if nnz_row_max is None else nnz_row_max
    u = LD(2.0) ** -53
    return float(np.sqrt(np.sum(r * r))), float((w + 3) * u * np.sqrt(np.sum(mag * mag)))
