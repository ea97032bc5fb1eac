"""The references and input generators of the Krylov vector tests (krylov_vec_ref.py) checked on the CPU: the exact data really is
exact, every reference agrees with a second formulation in rationals, and the Gram / leading-dimension conventions are the
library's."""
import math
from fractions import Fraction

import numpy as np
import pytest

import krylov_vec_ref as R
from test_krylov_host import gram_solve, kh  # noqa: F401  (the fixture compiles csrc/cfdh_krylov_host.hpp for the host)

SIZES = [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2049, 4099, 524288 + 515, 1048576 + 1029, 2097152 + 1027]
NVECS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 201]
SMALL_N = [1, 2, 3, 5, 8, 31, 64, 65]


def _frac(v):
    return [Fraction(int(a)) for a in v]


# ---- the exact data is exact ------------------------------------------------------------------------------------------------
def test_partial_sums_stay_below_2_53():
    for n in SIZES:
        for nvec in (NVECS if n <= 4099 else [9]):
            assert R.max_partial_sum(n, nvec) < 2 ** 53, (n, nvec)
    # the figure of the issue: 16 * 2.1 M * 9
    assert 16 * SIZES[-1] * 9 < 2 ** 53


@pytest.mark.parametrize("n", [1, 5, 257, 4099])
def test_exact_values_survive_float32_and_stay_in_range(n):
    rng = np.random.default_rng(n)
    ld = R.ld_of(n)
    A = R.exact_block(rng, n, ld, 9)
    x, h = R.exact_vector(rng, n), R.exact_coef(rng, 9)
    assert np.abs(A).max() <= R.VMAX and np.abs(x).max() <= R.VMAX and 1 <= np.abs(h).min() and np.abs(h).max() <= R.HMAX
    assert np.all(A[:, n:] == 0) and np.all(A[:, n - 1] != 0) and x[n - 1] != 0
    for a in (A, x, h):
        d = a.astype(np.float64)
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d) and np.array_equal(d.astype(np.int64), a)


@pytest.mark.parametrize("n", SIZES)
def test_pow4_vector_has_a_power_of_two_norm(n):
    t, nrm = R.pow4_vector(np.random.default_rng(n), n)
    assert len(t) == n and np.abs(t).max() <= R.VMAX and t[n - 1] != 0
    S = int((t * t).sum())
    assert S == int(nrm) ** 2 and math.frexp(nrm)[0] == 0.5  # a power of two
    if n >= 8:
        assert np.count_nonzero(t) == n  # dense: a dropped entry changes the result
    q = t.astype(np.float64) / nrm
    assert np.array_equal(q.astype(np.float32).astype(np.float64), q)
    assert [Fraction(v) for v in q[:50]] == [Fraction(int(a), int(nrm)) for a in t[:50]]


def test_pow4_counts_small():
    for n in range(1, 200):
        c = R.pow4_counts(n)
        if c is None:
            assert n < 8
            continue
        T, n1, n2, n3, n4 = c
        assert min(n1, n2, n3, n4) >= 0 and n1 + n2 + n3 + n4 == n and n1 + 4 * n2 + 9 * n3 + 16 * n4 == T
        assert math.frexp(float(T))[0] == 0.5 and int(math.log2(T)) % 2 == 0


# ---- the references against rationals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SMALL_N)
def test_dot_type_references(n):
    rng = np.random.default_rng(100 + n)
    ld = R.ld_of(n)
    x, y = R.exact_vector(rng, n), R.exact_vector(rng, n)
    assert Fraction(int(R.dot(x, y))) == R.frac_dot(x, y)
    assert Fraction(int(R.norm2_sq(x))) == R.frac_dot(x, x)
    assert Fraction(int(R.norminf_diff(x, y))) == max(abs(a - b) for a, b in zip(_frac(x), _frac(y)))
    assert Fraction(int(R.norminf_diff(x))) == max(abs(a) for a in _frac(x))
    for nvec in (1, 3, 9):
        V = R.exact_block(rng, n, ld, nvec)
        for ww in (False, True):
            h = R.multidot(V, x, ww)
            want = [R.frac_dot(V[v, :n], x) for v in range(nvec)] + ([R.frac_dot(x, x)] if ww else [])
            assert [Fraction(int(a)) for a in h] == want
    # the random-data path of the same functions: long doubles against fsum of exactly representable products
    xr, yr = R.cancelling_pair(rng, max(n, 4))
    got = float(R.dot(xr.astype(np.longdouble), yr.astype(np.longdouble)))
    exact = float(sum(Fraction(a) * Fraction(b) for a, b in zip(xr.tolist(), yr.tolist())))
    scale = R.abs_dot(xr, yr)
    assert abs(got - exact) <= 2.0 ** -60 * scale
    assert abs(exact) <= 2e-10 * scale and abs(exact) >= 0.5e-10 * scale  # the cancellation asked for
    assert abs(scale - math.fsum(abs(a * b) for a, b in zip(xr, yr))) <= 1e-12 * scale


def test_norminf_keeps_nan():
    x = np.array([1.0, np.nan, 3.0])
    assert math.isnan(R.norminf_diff(x)) and math.isnan(R.norminf_diff(np.ones(3), x))
    assert R.norminf_diff(np.array([1.0, np.inf])) == np.inf


@pytest.mark.parametrize("k", range(1, 9))
def test_gram_slot_layout(k):
    n = 37
    rng = np.random.default_rng(k)
    W, b = R.exact_block(rng, n, R.ld_of(n), k), R.exact_vector(rng, n)
    out = R.gram(W, b)
    assert out.shape == (8 * (k + 1),)
    for i in range(k + 1):
        for q in range(8):
            other = b if i == k else W[i, :n]
            want = R.frac_dot(W[q, :n], other) if q < k else 0
            assert Fraction(int(out[8 * i + q])) == want, (i, q)
    for i in range(k):
        for q in range(k):
            assert out[8 * i + q] == out[8 * q + i]


@pytest.mark.parametrize("n", SMALL_N)
def test_update_references(n):
    rng = np.random.default_rng(200 + n)
    ld = R.ld_of(n)
    for nvec in (1, 2, 4, 5, 9):
        V, h, w = R.exact_block(rng, n, ld, nvec), R.exact_coef(rng, nvec), R.exact_vector(rng, n)
        assert _frac(R.multiaxpy(V, h, w)) == R.frac_combine(V, h, w, -1)
        assert _frac(R.lincomb(V, h, w)) == R.frac_combine(V, h, w, 1)
        r, s2 = R.gs_update(V, h, w)
        assert _frac(r) == R.frac_combine(V, h, w, -1) and Fraction(int(s2)) == sum(a * a for a in R.frac_combine(V, h, w, -1))
        scale = R.abs_entry(V, h, w)
        assert _frac(scale) == [abs(Fraction(int(w[i]))) + sum(abs(Fraction(int(h[v] * V[v, i]))) for v in range(nvec)) for i in range(n)]
        # a chosen power-of-two norm: w = t + V h leaves t after the update
        t, nrm = R.pow4_vector(rng, n)
        w2 = t + R.combine(V, h, np.zeros(n, dtype=np.int64), 1)
        r2, s22 = R.gs_update(V, h, w2)
        assert np.array_equal(r2, t) and float(s22) == nrm * nrm
        assert [Fraction(v) for v in R.scaled(r2, nrm)] == [Fraction(int(a), int(nrm)) for a in t]
    assert np.array_equal(R.scaled(np.array([1, -2]), 0.0), np.zeros(2))


def test_gs_scale_branches():
    assert R.gs_scale_sq(20, 16) == 4       # the difference
    assert R.gs_scale_sq(16, 16) == 16      # cancelled: not positive
    assert R.gs_scale_sq(16, 25) == 16
    assert R.gs_scale_sq(4.0, -0.0) == 4.0  # the boundary ww - hh2 == ww
    assert R.gs_scale_sq(0, 0) == 0


def test_gs_scale_is_the_library_s(kh):  # noqa: F811
    for ww, hh2 in ((20.0, 16.0), (16.0, 16.0), (16.0, 25.0), (4.0, -0.0), (0.0, 0.0), (4.0, -1.0)):
        assert kh.kh_gs_scale(ww, hh2) == math.sqrt(R.gs_scale_sq(ww, hh2))


@pytest.mark.parametrize("n", SMALL_N)
def test_sub_mean_reference(n):
    x = R.exact_vector(np.random.default_rng(300 + n), n)
    got, S = R.sub_mean_exact(x)
    assert Fraction(S) == sum(_frac(x))
    mean = Fraction(int(x.sum()), n)
    for a, g in zip(_frac(x), got):
        assert abs(Fraction(g) - (a - mean)) <= 2 * Fraction(R.U) * (abs(a) + abs(mean))
    if n & (n - 1) == 0:  # a power of two: the mean is exact
        assert [Fraction(g) for g in got] == [a - mean for a in _frac(x)]


@pytest.mark.parametrize("k", range(1, 9))
def test_guess_reference_and_gram_solve_contract(kh, k):  # noqa: F811
    n = 33
    rng = np.random.default_rng(400 + k)
    hd, y = R.diagonal_gram(rng, k)
    # the library's own solve of these slots: exactly the integer coefficients, nothing dropped
    G = np.array([[hd[8 * i + q] for i in range(k)] for q in range(k)])
    used, rank, ylib = gram_solve(kh, G, hd[8 * k:8 * k + k])
    assert used and rank == k and np.array_equal(ylib, y.astype(np.float64))
    ld = R.ld_of(n)
    Um, Wm, b = R.exact_block(rng, n, ld, k), R.exact_block(rng, n, ld, k), R.exact_vector(rng, n)
    x, r, s2 = R.guess(Um, Wm, y, b)
    assert _frac(x) == R.frac_combine(Um, y, np.zeros(n, dtype=np.int64), 1)
    assert _frac(r) == R.frac_combine(Wm, y, b, -1)
    assert Fraction(int(s2)) == sum(a * a for a in _frac(r))
    # degenerate slots: the guess is not used and y = 0
    used, rank, ylib = gram_solve(kh, np.zeros((k, k)), np.zeros(k))
    assert not used and rank == 0 and np.all(ylib == 0)


def test_leading_dimensions():
    for n in list(range(1, 70)) + SIZES:
        ld = R.ld_of(n)
        assert ld == ((n + 1) & ~1) and ld >= n and ld % 2 == 0 and ld - n <= 1
        ld32 = R.ld32_of(ld)
        assert ld32 == ((ld + 3) & ~3) and ld32 >= ld and ld32 % 4 == 0 and ld32 - ld <= 2


def test_bounds_are_the_derived_ones():
    assert R.dot_bound(10, 3.0) == 12 * 2.0 ** -53 * 3.0
    assert R.entry_bound(4, 2.0) == 7 * 2.0 ** -53 * 2.0
    V = R.random_block(np.random.default_rng(1), 5, 6, 2, fp32=True)
    assert np.array_equal(V.astype(np.float32).astype(np.float64), V) and np.all(V[:, 5:] == 0)
