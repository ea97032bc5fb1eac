"""Plain numpy references of the Krylov vector wrappers (v_* of csrc/cfdh_krylov_vec.hip) and the inputs of their tests.

Every function states the CONTRACT of one wrapper (the comments of cfdh_internal.hpp and cfdh_krylov_vec.hip), not its loops, and
works in the arithmetic of its arguments:

* exact data -- int64 arrays.  Blocks hold integers in [-4, 4], coefficients integers in [-3, 3], and every scale is a power of
  two, so a product is at most 16 * 9 and any partial sum of any of the sizes used, taken in any order, stays far below 2^53
  (see max_partial_sum).  A device result in doubles must then equal the reference bit for bit whatever its summation order,
  and the fp32 copy of such a block loses nothing.
* random data -- np.longdouble arrays (64-bit significand): the reference error n 2^-64 sum|a_i b_i| is 2^-11 of the bounds the
  tests use.

Blocks are numpy arrays of shape (nvec, ld): flattened in C order that is the column-major layout A[v * ld + i] of the library,
and the entries behind n are zero.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit round-off of a double
VMAX, HMAX = 4, 3


# ---- leading dimensions of the solver ---------------------------------------------------------------------------------------
def ld_of(n):
    """even, so that every column of an fp64 block starts on a 16-byte boundary (krylov_ld)"""
    return (n + 1) & ~1


def ld32_of(ld):
    """columns of the fp32 copy start on 16-byte boundaries as well"""
    return (ld + 3) & ~3


# ---- references (dtype-generic: int64 in, int64 out; longdouble in, longdouble out) -------------------------------------------
def dot(x, y):
    return (x * y).sum()


def norm2_sq(x):
    return dot(x, x)


def norminf_diff(x, y=None):
    """max |x - y|, or max |x|; NaN as soon as one entry is NaN"""
    d = np.abs(x if y is None else x - y)
    return d.max() if not np.isnan(d.astype(np.float64)).any() else np.nan


def multidot(V, w, with_ww):
    """h[v] = V_v . w, then w . w"""
    n = len(w)
    h = [dot(V[v, :n], w) for v in range(V.shape[0])]
    if with_ww:
        h.append(dot(w, w))
    return np.array(h, dtype=V.dtype)


def gram(W, b):
    """out[8 i + q] = W_q . W_i for i < k, out[8 k + q] = W_q . b; the slots q >= k of the 8-wide rows are zero"""
    k, n = W.shape[0], len(b)
    out = np.zeros(8 * (k + 1), dtype=W.dtype)
    for q in range(k):
        for i in range(k):
            out[8 * i + q] = dot(W[q, :n], W[i, :n])
        out[8 * k + q] = dot(W[q, :n], b)
    return out


def combine(V, h, w, sign):
    """w + sign * sum_v h_v V_v, entry by entry"""
    n = len(w)
    return w + sign * (h[:, None] * V[:, :n]).sum(axis=0)


def multiaxpy(V, h, w):
    return combine(V, h, w, -1)


def lincomb(Z, y, x):
    return combine(Z, y, x, 1)


def gs_scale_sq(ww, hh2):
    """square of the scale of a Gram-Schmidt pass: w.w - |h|^2, or w.w when that difference is not positive or above w.w"""
    d = ww - hh2
    return d if (d > 0 and d <= ww) else ww


def gs_update(V, h, w):
    """the unnormalised update w - V h and its squared norm"""
    r = multiaxpy(V, h, w)
    return r, dot(r, r)


def guess(Umat, Wmat, y, b):
    """projected initial guess with the coefficients y of the Gram system: x = U y, r = b - W y, |r|^2"""
    n = len(b)
    x = lincomb(Umat, y, np.zeros(n, dtype=b.dtype))
    r = multiaxpy(Wmat, y, b)
    return x, r, dot(r, r)


def sub_mean_exact(x):
    """x - mean(x) for exact data as the doubles the wrapper must produce: the sum S is exact, the wrapper forms the mean as
    S * (1 / n) in doubles on one scalar (two roundings, no summation involved) and subtracts it from every entry (one rounding)"""
    S = float(x.sum())
    m = S * (1.0 / len(x))
    return x.astype(np.float64) - m, S


def scaled(num, s):
    """num / s in doubles; s = 0 gives zeros (a vector without a norm is not scaled to NaN)"""
    num = np.asarray(num, dtype=np.float64)
    return num / s if s != 0 else np.zeros_like(num)


# ---- second formulation of the same contracts in exact rationals (small n; tests of this module) -----------------------------
def frac_dot(x, y):
    return sum((Fraction(int(a)) * Fraction(int(b)) for a, b in zip(x, y)), Fraction(0))


def frac_combine(V, h, w, sign):
    n = len(w)
    return [Fraction(int(w[i])) + sign * sum((Fraction(int(h[v])) * Fraction(int(V[v][i])) for v in range(len(h))), Fraction(0))
            for i in range(n)]


# ---- exact inputs -----------------------------------------------------------------------------------------------------------
def max_partial_sum(n, nvec):
    """no partial sum of any op on exact data exceeds this: n products of at most 16 (dot products), or the entry bound below
    squared and summed over n entries (norm of an update)"""
    entry = VMAX + nvec * HMAX * VMAX
    return n * max(VMAX * VMAX, entry * entry)


def exact_block(rng, n, ld, nvec):
    A = np.zeros((nvec, ld), dtype=np.int64)
    A[:, :n] = rng.integers(-VMAX, VMAX + 1, size=(nvec, n))
    A[:, n - 1] = rng.choice([-3, -1, 2, 4], size=nvec)  # the scalar-tail entry always counts
    return A


def exact_vector(rng, n):
    x = rng.integers(-VMAX, VMAX + 1, size=n).astype(np.int64)
    x[n - 1] = rng.choice([-3, -1, 2, 4])
    return x


def exact_coef(rng, nvec):
    h = rng.integers(-HMAX, HMAX + 1, size=nvec).astype(np.int64)
    h[h == 0] = 1 + (np.arange(nvec)[h == 0] % 3)  # no column drops out of a test by chance
    return h


def pow4_counts(n):
    """(T, n1, n2, n3, n4): how many of n entries get the magnitudes 1, 2, 3, 4 so that the squares sum to T, a power of 4;
    None when no such choice without zero entries exists (n = 2, 3, ...)."""
    T = 1
    while T < n:
        T *= 4
    while T <= 16 * n:
        R = T - n  # = 3 n2 + 8 n3 + 15 n4
        for n3 in range(3):
            R2 = R - 8 * n3
            if R2 < 0 or R2 % 3:
                continue
            units = R2 // 3  # n2 + 5 n4
            n4 = max(0, -(-(units + n3 - n) // 4))
            n2 = units - 5 * n4
            if n2 >= 0 and n2 + n3 + n4 <= n:
                return T, n - n2 - n3 - n4, n2, n3, n4
        T *= 4
    return None


def pow4_vector(rng, n):
    """integers in [-4, 4] whose squared norm is a power of 4 (so the norm is a power of two), the last entry non-zero;
    returns (vector, norm)"""
    c = pow4_counts(n)
    if c is None:  # tiny n: one entry carries the norm
        t = np.zeros(n, dtype=np.int64)
        t[n - 1] = 2
        return t, 2.0
    T, n1, n2, n3, n4 = c
    mag = np.repeat(np.array([1, 2, 3, 4], dtype=np.int64), [n1, n2, n3, n4])
    rng.shuffle(mag)
    t = mag * rng.choice(np.array([-1, 1], dtype=np.int64), size=n)
    return t, float(np.sqrt(float(T)))


def diagonal_gram(rng, k):
    """Gram slots hd[8 (k + 1)] of k orthogonal directions with squared lengths 4^a and right-hand side y_i 4^a_i: the minimiser
    of |b - W y| is the integer vector y, every direction is kept (rank k)"""
    y = exact_coef(rng, k)
    d = 4 ** rng.integers(0, 4, size=k)
    hd = np.zeros(8 * (k + 1))
    for i in range(k):
        hd[8 * i + i] = float(d[i])
        hd[8 * k + i] = float(d[i] * y[i])
    return hd, y


# ---- random inputs ----------------------------------------------------------------------------------------------------------
def random_block(rng, n, ld, nvec, fp32=False):
    """standard normal draws (rounded to fp32 first when the op reads the fp32 copy, so that the copy is the reference's data)"""
    A = np.zeros((nvec, ld))
    A[:, :n] = rng.standard_normal((nvec, n))
    if fp32:
        A = A.astype(np.float32).astype(np.float64)
    return A


def cancelling_pair(rng, n):
    """x, y with x . y about 1e-10 of sum |x_i y_i| (n >= 4)"""
    x = rng.standard_normal(n)
    y = rng.standard_normal(n)
    xl, yl = x.astype(np.longdouble), y.astype(np.longdouble)
    target = 1e-10 * float(np.abs(xl * yl).sum())
    rest = float((xl[1:] * yl[1:]).sum())
    y[0] = (target - rest) / x[0]
    return x, y


def abs_dot(x, y):
    """sum |a_i b_i|, the scale of the error bound of a dot product"""
    return float((np.abs(x.astype(np.longdouble)) * np.abs(y.astype(np.longdouble))).sum())


def abs_entry(V, h, w):
    """|w_i| + sum_v |h_v| |V_vi|, the scale of the error bound of an update"""
    n = len(w)
    return np.abs(w) + (np.abs(h)[:, None] * np.abs(V[:, :n])).sum(axis=0)


def dot_bound(n, scale):
    """|computed - exact| of a sum of n products in any order: (n + 2) u sum|a_i b_i| covers the n roundings of the products
    (contracted or not) and the at most n - 1 additions any entry passes through, to first order with room for the second"""
    return (n + 2) * U * scale


def entry_bound(nvec, scale):
    return (nvec + 3) * U * scale
