"""The Krylov vector kernels of csrc/cfdh_krylov_vec.hip one by one, through cfdh_krylov_vec_op (Context.krylov_vec_op), against the
plain references of krylov_vec_ref.py.

Exact data (integers in [-4, 4], coefficients in [-3, 3], power-of-two scales): every partial sum in any order is an integer
below 2^53, so the device result must equal the int64 reference BIT FOR BIT.  Random data: bounds derived from the unit round-off
(krylov_vec_ref.dot_bound / entry_bound), nothing measured.  Whole solves hide errors in these kernels -- FGMRES checks the true
residual and restarts, so a dropped tail entry costs iterations, not the answer.

op -> kernels reached by an exact-data test
  DOT, NORM2, NORM2_PAIR, NORM_SCALE_INV  reduce_partial_kernel<0>, reduce_final_kernel<0> (+ sqrt_kernel, scale_inv_dev_kernel)
  NORM2_TRIPLE                            norm3_partial_kernel, reduce_final_kernel<0>
  NORMINF_DIFF                            reduce_partial_kernel<1>, reduce_final_kernel<1>
  SUB_MEAN                                sum_partial_kernel, reduce_final_kernel<0>, sub_scalar_kernel
  MULTIDOT                                multidot_kernel, reduce_final_kernel<0> (host-mapped mirror)
  MULTIDOT32                              multidot32_kernel, reduce_final_kernel<0>
  GRAM                                    gram_kernel<2|3|4> (k = 2, 3, 4), multidot_kernel (k = 1, 5 .. 8)
  MULTIAXPY, LINCOMB                      multiaxpy_kernel
  LINCOMB_KEEP                            lincomb_keep_kernel
  GS_UPDATE_NORMALIZE                     gs_update_normalize_kernel
  GS_UPDATE32                             gs_update32_kernel, reduce_final_kernel<2>, scale_store32_kernel
  STORE32                                 store32_kernel
  GUESS                                   gram_solve_kernel, guess_combine_kernel, reduce_final_kernel<0>, scale_inv_sqrt_kernel
  AXPY, WAXPY, SCALE, SCALE_TO, PMULT     axpy_kernel, waxpy_kernel, scale_kernel, scale_to_kernel, pmult_kernel

Sizes: the smallest at which each mechanism first engages -- blocks that own nothing (n < 1024), wave and block boundaries, odd
and mod-4 tails, per-block chunks that differ between blocks (2049, 4099), a second trip of the multidot loops (per > 512, per >
1024), the 1024-block cap of the reductions and the 2048-block cap of the element-wise grids.

Largest error / bound seen on the random data (MI355X; information for a later tightening, table in DESIGN.md): 0.50 (v_axpy at
n = 5, where the bound is two roundings); the dot-type ops 0.13 .. 0.26.
"""
import math

import numpy as np
import pytest

import krylov_vec_ref as R
from cfd_hemodynamic_amd import _lib as L
from util import dfg_case, make_ctx

pytestmark = pytest.mark.gpu

TINY = [1, 2, 3, 5]
MID = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 2049, 4099]
LARGE = [524288 + 515, 1048576 + 1029, 2097152 + 1027]
ALL_N = TINY + MID + LARGE
NVECS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 201]
RAND_N = [5, 257, 1027, 4099, LARGE[0]]
UNTOUCHED = -7.25  # what cfdh_krylov_vec_op leaves in a host-mapped word no kernel wrote
RING = L.KVOP_FLAG_RING
U = R.U


def nvecs(n):
    return NVECS if n <= 4099 else [9]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def same(a, b):
    """bit-identical doubles / floats (NaN patterns and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ctx():
    return make_ctx(dfg_case(4))


RATIOS = {}


def ratio(name, err, bound):
    """err <= bound entry by entry; the largest err / bound per op is printed for DESIGN.md"""
    err, bound = np.atleast_1d(f64(err)), np.atleast_1d(f64(bound))
    r = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print("error/bound %-22s %.3e" % (name, r))
    assert r <= 1.0, (name, r)


# ---- exact data: reductions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_N)
def test_exact_reductions(ctx, n):
    rng = np.random.default_rng(n)
    ld = R.ld_of(n)
    x, y, z = R.exact_vector(rng, n), R.exact_vector(rng, n), R.exact_vector(rng, n)
    o = ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=x, y=y)
    assert same(o["host"], f64([R.dot(x, y)])) and same(o["dev"], o["host"]) and same(o["mirror"], o["host"])
    for with_y in (0, 1):
        o = ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=x, y=y if with_y else None, flags=with_y)
        assert same(o["host"], f64([R.norminf_diff(x, y if with_y else None)]))
        assert same(o["dev"], o["host"]) and same(o["mirror"], o["host"])
    # norms of vectors whose squared norm is a power of 4: the square root is exact too
    (a, na), (b, nb), (c, nc) = (R.pow4_vector(rng, n) for _ in range(3))
    o = ctx.krylov_vec_op(L.KVOP_NORM2, n, ld, x=a)
    assert same(o["host"], f64([na])) and same(o["dev"], f64([R.norm2_sq(a)])) and same(o["mirror"], o["dev"])
    o = ctx.krylov_vec_op(L.KVOP_NORM2_PAIR, n, ld, x=a, y=b)
    assert same(o["host"], f64([na, nb])) and same(o["dev"], f64([R.norm2_sq(a), R.norm2_sq(b)])) and same(o["mirror"], o["dev"])
    o = ctx.krylov_vec_op(L.KVOP_NORM2_TRIPLE, n, ld, x=a, y=b, A=c)
    assert same(o["host"], f64([na, nb, nc])) and same(o["dev"], f64([R.norm2_sq(v) for v in (a, b, c)])) and same(o["mirror"], o["dev"])
    o = ctx.krylov_vec_op(L.KVOP_NORM_SCALE_INV, n, ld, x=a)
    assert same(o["dev"], f64([na])) and same(o["out1"], R.scaled(a, na))
    want, S = R.sub_mean_exact(z)
    o = ctx.krylov_vec_op(L.KVOP_SUB_MEAN, n, ld, x=z)
    assert same(o["dev"], f64([S])) and same(o["out1"], want)


@pytest.mark.parametrize("n", ALL_N)
def test_exact_multidot(ctx, n):
    rng = np.random.default_rng(1000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    w = R.exact_vector(rng, n)
    for nvec in nvecs(n):
        V = R.exact_block(rng, n, ld, nvec)
        for ww in (0, 1):
            # the solver's mirror is a slot of the read-back ring; the plain scalar mirror is the other place kernels write to
            o = ctx.krylov_vec_op(L.KVOP_MULTIDOT, n, ld, nvec, A=V, x=w, flags=ww | (RING if ww else 0))
            assert same(o["dev"], f64(R.multidot(V, w, bool(ww)))), (nvec, ww)
            assert same(o["mirror"], o["dev"]), (nvec, ww)
        V32 = R.exact_block(rng, n, ld32, nvec)
        o = ctx.krylov_vec_op(L.KVOP_MULTIDOT32, n, ld32, nvec, A=V32, x=w, flags=RING)
        assert same(o["dev"], f64(R.multidot(V32, w, True))), nvec
        assert same(o["mirror"], o["dev"]), nvec


# ---- exact data: updates ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_N)
def test_exact_updates(ctx, n):
    rng = np.random.default_rng(2000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    w = R.exact_vector(rng, n)
    t, nrm = R.pow4_vector(rng, n)
    for nvec in nvecs(n):
        V, h = R.exact_block(rng, n, ld, nvec), R.exact_coef(rng, nvec)
        o = ctx.krylov_vec_op(L.KVOP_MULTIAXPY, n, ld, nvec, A=V, coef=h, x=w)
        assert same(o["out1"], f64(R.multiaxpy(V, h, w))), nvec
        want = f64(R.lincomb(V, h, w))
        o = ctx.krylov_vec_op(L.KVOP_LINCOMB, n, ld, nvec, A=V, coef=h, x=w)
        assert same(o["out1"], want), nvec
        o = ctx.krylov_vec_op(L.KVOP_LINCOMB_KEEP, n, ld, nvec, A=V, coef=h, x=w)
        assert same(o["out1"], want) and same(o["out2"], want), nvec
        # fused update and normalisation: w.w = |h|^2 + 4 makes the scale 2
        hh2 = int((h * h).sum())
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE_NORMALIZE, n, ld, nvec, A=V, coef=np.append(h, hh2 + 4), x=w)
        assert same(o["dev"], f64([2.0])) and same(o["out1"], R.scaled(R.multiaxpy(V, h, w), 2.0)), nvec
        # update against the fp32 copy with the measured norm: w = t + V h leaves t, whose norm is a power of two
        V32 = R.exact_block(rng, n, ld32, nvec)
        w2 = t + R.combine(V32, h, np.zeros(n, dtype=np.int64), 1)
        r, s2 = R.gs_update(V32, h, w2)
        assert float(s2) == nrm * nrm
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE32, n, ld32, nvec, A=V32, coef=h, x=w2, flags=RING)
        vn = R.scaled(r, nrm)
        assert same(o["dev"], f64([nrm])) and same(o["out1"], vn) and same(o["out32"], vn.astype(np.float32)), nvec
        assert same(o["out32"], o["out1"].astype(np.float32))
        assert same(o["mirror"][nvec + 1:], o["dev"]) and np.all(o["mirror"][:nvec + 1] == UNTOUCHED)
    o = ctx.krylov_vec_op(L.KVOP_STORE32, n, ld, x=w)
    assert same(o["out32"], f64(w).astype(np.float32))
    q = R.scaled(t, nrm)
    o = ctx.krylov_vec_op(L.KVOP_STORE32, n, ld, x=q)
    assert same(o["out32"], q.astype(np.float32)) and same(f64(o["out32"]), q)


@pytest.mark.parametrize("n", [1, 2, 5, 257, 1027, 4099])
def test_gs_scale_branches(ctx, n):
    """h[nvec] (the w.w slot) chosen to reach every branch of cfdh_krylov::gs_scale"""
    rng = np.random.default_rng(3000 + n)
    ld = R.ld_of(n)
    for nvec in (1, 4, 5):
        V, w = R.exact_block(rng, n, ld, nvec), R.exact_vector(rng, n)
        h = np.full(nvec, 3, dtype=np.int64) if nvec > 1 else np.array([4], dtype=np.int64)
        r = R.multiaxpy(V, h, w)
        hh2 = int((h * h).sum())
        assert hh2 >= 16
        # w.w - |h|^2 cancelled (not positive): the scale falls back to sqrt(w.w) = 4
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE_NORMALIZE, n, ld, nvec, A=V, coef=np.append(h, 16), x=w)
        assert math.sqrt(R.gs_scale_sq(16, hh2)) == 4.0
        assert same(o["dev"], f64([4.0])) and same(o["out1"], R.scaled(r, 4.0))
        # the boundary w.w - |h|^2 == w.w.  (|h|^2 = -0.0 cannot leave the kernel's own sum 0.0 + h h; h = 0 gives the same
        # comparison nrm2 <= ww with equality.)
        z = np.zeros(nvec, dtype=np.int64)
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE_NORMALIZE, n, ld, nvec, A=V, coef=np.append(z, 4), x=w)
        assert same(o["dev"], f64([2.0])) and same(o["out1"], R.scaled(w, 2.0))
        # no norm at all: zeros, not NaN
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE_NORMALIZE, n, ld, nvec, A=V, coef=np.append(z, 0), x=w)
        assert same(o["dev"], f64([0.0])) and np.array_equal(o["out1"], np.zeros(n))


# ---- exact data: Gram system and projected guess ------------------------------------------------------------------------------
def _gram_guess_cases():
    return [(n, k) for n in (3, 1025, 4099) for k in range(1, 9)] + [(LARGE[2], 2), (LARGE[2], 4)]


@pytest.mark.parametrize("n,k", _gram_guess_cases())
def test_exact_gram(ctx, n, k):
    rng = np.random.default_rng(4000 + 10 * n + k)
    ld = R.ld_of(n)
    W, b = R.exact_block(rng, n, ld, k), R.exact_vector(rng, n)
    o = ctx.krylov_vec_op(L.KVOP_GRAM, n, ld, k, A=W, x=b)
    out = o["dev"]
    assert same(out, f64(R.gram(W, b)))
    for i in range(k):
        for q in range(k):
            assert out[8 * i + q] == out[8 * q + i]
    unused = [8 * i + q for i in range(k + 1) for q in range(k, 8)]
    assert same(out[unused], np.zeros(len(unused)))


@pytest.mark.parametrize("n,k", _gram_guess_cases())
def test_exact_guess(ctx, n, k):
    rng = np.random.default_rng(5000 + 10 * n + k)
    ld = R.ld_of(n)
    hd, y = R.diagonal_gram(rng, k)
    Um, Wm = R.exact_block(rng, n, ld, k), R.exact_block(rng, n, ld, k)
    t, nrm = R.pow4_vector(rng, n)
    b = t + R.combine(Wm, y, np.zeros(n, dtype=np.int64), 1)  # so that r = b - W y = t
    x, r, s2 = R.guess(Um, Wm, y, b)
    assert np.array_equal(r, t) and float(s2) == nrm * nrm
    for scale in (0, 1):
        o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, k, A=Um, B=Wm, coef=hd, x=b, flags=scale)
        assert same(o["host"], f64([nrm, 1.0, k] + list(y)))       # |r|, used, rank, y
        assert same(o["mirror"], f64([nrm * nrm, 1.0, k] + list(y)))
        assert same(o["dev"], f64([nrm * nrm] + list(y)))             # what the kernels read: |r|^2 and y on the device
        assert same(o["out1"], f64(x))
        assert same(o["out2"], R.scaled(r, nrm) if scale else f64(r))


# ---- exact data: element-wise kernels -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ALL_N)
def test_exact_elementwise(ctx, n):
    rng = np.random.default_rng(6000 + n)
    ld = R.ld_of(n)
    x, y = R.exact_vector(rng, n), R.exact_vector(rng, n)
    for a in (-3.0, 0.25):
        want = f64(y) + a * f64(x)
        assert same(ctx.krylov_vec_op(L.KVOP_AXPY, n, ld, x=x, y=y, scalar=a)["out1"], want)
        assert same(ctx.krylov_vec_op(L.KVOP_WAXPY, n, ld, x=x, y=y, scalar=a)["out1"], want)
        assert same(ctx.krylov_vec_op(L.KVOP_SCALE, n, ld, x=x, scalar=a)["out1"], a * f64(x))
        assert same(ctx.krylov_vec_op(L.KVOP_SCALE_TO, n, ld, x=x, scalar=a)["out1"], a * f64(x))
    assert same(ctx.krylov_vec_op(L.KVOP_PMULT, n, ld, x=x, y=y)["out1"], f64(x) * f64(y))


# ---- vectors without a norm -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 1027, 4099])
def test_zero_norms_give_zeros(ctx, n):
    rng = np.random.default_rng(7000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    zero = np.zeros(n)
    o = ctx.krylov_vec_op(L.KVOP_NORM_SCALE_INV, n, ld, x=zero)
    assert same(o["dev"], f64([0.0])) and np.array_equal(o["out1"], zero)
    nvec = 3
    V32, h = R.exact_block(rng, n, ld32, nvec), R.exact_coef(rng, nvec)
    w = R.combine(V32, h, np.zeros(n, dtype=np.int64), 1)  # w - V h = 0
    o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE32, n, ld32, nvec, A=V32, coef=h, x=w)
    assert same(o["dev"], f64([0.0])) and np.array_equal(o["out1"], zero) and np.array_equal(o["out32"], zero.astype(np.float32))
    # a Gram system without a direction: the guess is not used, r = b, and b = 0 has no norm to divide by
    Um, Wm = R.exact_block(rng, n, ld, nvec), R.exact_block(rng, n, ld, nvec)
    o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, nvec, A=Um, B=Wm, coef=np.zeros(8 * (nvec + 1)), x=zero, flags=1)
    assert same(o["host"], f64([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])) and np.array_equal(o["out1"], zero) and np.array_equal(o["out2"], zero)
    b = R.exact_vector(rng, n)
    o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, nvec, A=Um, B=Wm, coef=np.zeros(8 * (nvec + 1)), x=b)
    assert o["host"][1] == 0.0 and np.array_equal(o["out1"], zero) and same(o["out2"], f64(b))
    assert same(o["dev"][:1], f64([R.norm2_sq(b)]))


# ---- random data: derived bounds ------------------------------------------------------------------------------------------------
def _ld(a):
    return a.astype(np.longdouble)


def _sumsq_bound(n, r, e):
    """|computed sum of squares of a computed vector - r . r| when the vector is r within e entry by entry: the perturbation
    2 sum |r_i| e_i + sum e_i^2, and the dot bound on the sum that was actually taken"""
    pert = float(2 * (np.abs(f64(r)) * e).sum() + (e * e).sum())
    return pert + R.dot_bound(n, float(R.dot(r, r)) + pert)


@pytest.mark.parametrize("n", RAND_N)
def test_random_reductions(ctx, n):
    rng = np.random.default_rng(8000 + n)
    ld = R.ld_of(n)
    x, y, z = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    pairs = [(x, y)] + ([R.cancelling_pair(rng, n)] if n >= 4 else [])
    for a, b in pairs:
        o = ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=a, y=b)
        ratio("dot", abs(_ld(o["host"][0]) - R.dot(_ld(a), _ld(b))), R.dot_bound(n, R.abs_dot(a, b)))
        assert same(o["dev"], o["host"]) and same(o["mirror"], o["host"])
    sq = [R.norm2_sq(_ld(v)) for v in (x, y, z)]
    for op, vecs, kw in ((L.KVOP_NORM2, 1, dict(x=x)), (L.KVOP_NORM2_PAIR, 2, dict(x=x, y=y)), (L.KVOP_NORM2_TRIPLE, 3, dict(x=x, y=y, A=z))):
        o = ctx.krylov_vec_op(op, n, ld, **kw)
        assert same(o["mirror"], o["dev"])
        for i in range(vecs):
            ratio("norm2 squared", abs(_ld(o["dev"][i]) - sq[i]), R.dot_bound(n, float(sq[i])))
            ratio("norm2 sqrt", abs(o["host"][i] - math.sqrt(o["dev"][i])), U * o["host"][i])
    for yy in (None, y):
        o = ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=x, y=yy, flags=int(yy is not None))
        assert same(o["host"], f64([np.abs(x if yy is None else x - yy).max()]))  # one rounding per entry, a maximum has none
    o = ctx.krylov_vec_op(L.KVOP_NORM_SCALE_INV, n, ld, x=x)
    nrm = o["dev"][0]
    ratio("norm_to_dev", abs(_ld(nrm) - np.sqrt(sq[0])), (R.dot_bound(n, 1.0) + U) * float(np.sqrt(sq[0])))
    ratio("scale_inv_dev", np.abs(_ld(o["out1"]) - _ld(x) / _ld(nrm)), 4 * U * np.abs(x / nrm))
    # mean: the sum within the dot bound, two roundings for S * (1 / n), one for the subtraction
    o = ctx.krylov_vec_op(L.KVOP_SUB_MEAN, n, ld, x=z)
    S, sabs = _ld(z).sum(), float(np.abs(z).sum())
    ratio("sub_mean sum", abs(_ld(o["dev"][0]) - S), R.dot_bound(n, sabs))
    m = float(S / n)
    e_m = R.dot_bound(n, sabs) / n + 2 * U * abs(m)
    ratio("sub_mean", np.abs(_ld(o["out1"]) - (_ld(z) - S / n)), e_m + U * (np.abs(z) + abs(m) + e_m))


@pytest.mark.parametrize("n", RAND_N)
def test_random_multidot_and_gram(ctx, n):
    rng = np.random.default_rng(9000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    w = rng.standard_normal(n)
    for nvec in ([1, 3, 4, 5, 9, 17] if n <= 4099 else [9]):
        for fp32 in (False, True):
            l = ld32 if fp32 else ld
            V = R.random_block(rng, n, l, nvec, fp32)
            o = ctx.krylov_vec_op(L.KVOP_MULTIDOT32 if fp32 else L.KVOP_MULTIDOT, n, l, nvec, A=V, x=w, flags=1 | RING)
            ref = R.multidot(_ld(V), _ld(w), True)
            scale = [R.abs_dot(V[v, :n], w) for v in range(nvec)] + [R.abs_dot(w, w)]
            ratio("multidot32" if fp32 else "multidot", np.abs(_ld(o["dev"]) - ref), R.dot_bound(n, f64(scale)))
            assert same(o["mirror"], o["dev"])
    for k in ([1, 2, 3, 4, 7] if n <= 4099 else [3]):
        W = R.random_block(rng, n, ld, k)
        o = ctx.krylov_vec_op(L.KVOP_GRAM, n, ld, k, A=W, x=w)
        ref = R.gram(_ld(W), _ld(w))
        scale = R.gram(np.abs(_ld(W)), np.abs(_ld(w)))
        ratio("gram", np.abs(_ld(o["dev"]) - ref), R.dot_bound(n, f64(scale)))


@pytest.mark.parametrize("n", RAND_N)
def test_random_updates(ctx, n):
    rng = np.random.default_rng(10000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    w = rng.standard_normal(n)
    for nvec in ([1, 3, 4, 5, 9, 17] if n <= 4099 else [9]):
        V, h = R.random_block(rng, n, ld, nvec), rng.standard_normal(nvec)
        e = R.entry_bound(nvec, R.abs_entry(V, h, w))
        ref = R.multiaxpy(_ld(V), _ld(h), _ld(w))
        o = ctx.krylov_vec_op(L.KVOP_MULTIAXPY, n, ld, nvec, A=V, coef=h, x=w)
        ratio("multiaxpy", np.abs(_ld(o["out1"]) - ref), e)
        o = ctx.krylov_vec_op(L.KVOP_LINCOMB_KEEP, n, ld, nvec, A=V, coef=h, x=w)
        ratio("lincomb_keep", np.abs(_ld(o["out1"]) - R.lincomb(_ld(V), _ld(h), _ld(w))), e)
        assert same(o["out1"], o["out2"])
        assert same(o["out1"], ctx.krylov_vec_op(L.KVOP_LINCOMB, n, ld, nvec, A=V, coef=h, x=w)["out1"])
        # fused normalisation: s^2 = ww - |h|^2 from the coefficients (sum of nvec + 1 terms), then sqrt; vn against the
        # reference numerator over the device's s: numerator error / s, plus reciprocal, product (4 u allowed)
        hh2 = float(R.dot(_ld(h), _ld(h)))
        ww = 2.0 * hh2 + 1.0
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE_NORMALIZE, n, ld, nvec, A=V, coef=np.append(h, ww), x=w)
        s = o["dev"][0]
        s2ref = _ld(np.float64(ww)) - R.dot(_ld(h), _ld(h))
        ratio("gs_update_normalize s", abs(_ld(s) - np.sqrt(s2ref)), ((nvec + 3) * U * (ww + hh2) / float(s2ref) + U) * float(np.sqrt(s2ref)))
        ratio("gs_update_normalize", np.abs(_ld(o["out1"]) - ref / _ld(s)), (e * (1 + 4 * U) + 4 * U * np.abs(f64(ref))) / s)
        # fp32 copy with the measured norm: s^2 is a dot product of the computed update (entry errors e_i on top)
        V32 = R.random_block(rng, n, ld32, nvec, fp32=True)
        e = R.entry_bound(nvec, R.abs_entry(V32, h, w))
        r, s2 = R.gs_update(_ld(V32), _ld(h), _ld(w))
        o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE32, n, ld32, nvec, A=V32, coef=h, x=w, flags=RING)
        s, sref = o["dev"][0], float(np.sqrt(s2))
        ratio("gs_update32 s", abs(_ld(s) - np.sqrt(s2)), _sumsq_bound(n, r, e) / sref + U * s)
        ratio("gs_update32", np.abs(_ld(o["out1"]) - r / _ld(s)), (e * (1 + 4 * U) + 4 * U * np.abs(f64(r))) / s)
        assert same(o["out32"], o["out1"].astype(np.float32)) and same(o["mirror"][nvec + 1:], o["dev"])
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    a = 0.7
    for op in (L.KVOP_AXPY, L.KVOP_WAXPY):  # a product and a sum, contracted or not
        o = ctx.krylov_vec_op(op, n, ld, x=x, y=y, scalar=a)
        ratio("axpy", np.abs(_ld(o["out1"]) - (_ld(y) + _ld(np.float64(a)) * _ld(x))), 2 * U * (np.abs(y) + np.abs(a * x)))
    # one rounding each: IEEE leaves no choice
    assert same(ctx.krylov_vec_op(L.KVOP_SCALE, n, ld, x=x, scalar=a)["out1"], a * x)
    assert same(ctx.krylov_vec_op(L.KVOP_SCALE_TO, n, ld, x=x, scalar=a)["out1"], a * x)
    assert same(ctx.krylov_vec_op(L.KVOP_PMULT, n, ld, x=x, y=y)["out1"], x * y)
    assert same(ctx.krylov_vec_op(L.KVOP_STORE32, n, ld, x=x)["out32"], x.astype(np.float32))


# ---- equalities the comments of the kernels promise (bitwise, random data) ----------------------------------------------------
@pytest.mark.parametrize("n,k", [(n, k) for n in (5, 1027, 4099) for k in (1, 3, 4, 5, 8)] + [(LARGE[2], 4)])
def test_guess_combine_is_lincomb_multiaxpy_and_dot(ctx, n, k):
    rng = np.random.default_rng(11000 + 10 * n + k)
    ld = R.ld_of(n)
    hd, y = R.diagonal_gram(rng, k)
    Um, Wm, b = R.random_block(rng, n, ld, k), R.random_block(rng, n, ld, k), rng.standard_normal(n)
    o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, k, A=Um, B=Wm, coef=hd, x=b)
    ydev = o["dev"][1:]
    assert same(ydev, f64(y)) and same(o["mirror"][3:], ydev) and same(o["mirror"][:1], o["dev"][:1])
    x = ctx.krylov_vec_op(L.KVOP_LINCOMB, n, ld, k, A=Um, coef=ydev, x=np.zeros(n))["out1"]        # v_zero + v_lincomb
    r = ctx.krylov_vec_op(L.KVOP_MULTIAXPY, n, ld, k, A=Wm, coef=ydev, x=b)["out1"]                # v_copy + v_multiaxpy
    rr = ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=r, y=r)["dev"]                                     # v_dot(r, r)
    assert same(o["out1"], x) and same(o["out2"], r) and same(o["dev"][:1], rr)
    # the same with entry-wise error bounds against the reference
    xr, rref, s2 = R.guess(_ld(Um), _ld(Wm), _ld(f64(y)), _ld(b))
    zero = np.zeros(n)
    ex, er = R.entry_bound(k, R.abs_entry(Um, f64(y), zero)), R.entry_bound(k, R.abs_entry(Wm, f64(y), b))
    ratio("guess x", np.abs(_ld(o["out1"]) - xr), ex)
    ratio("guess r", np.abs(_ld(o["out2"]) - rref), er)
    ratio("guess |r|^2", abs(_ld(o["dev"][0]) - s2), _sumsq_bound(n, rref, er))


@pytest.mark.parametrize("n", [5, 1027, 4099, LARGE[1]])
def test_fused_norms_are_single_norms(ctx, n):
    rng = np.random.default_rng(12000 + n)
    ld = R.ld_of(n)
    v = [rng.standard_normal(n) for _ in range(3)]
    single = [ctx.krylov_vec_op(L.KVOP_NORM2, n, ld, x=a)["host"][0] for a in v]
    assert same(ctx.krylov_vec_op(L.KVOP_NORM2_PAIR, n, ld, x=v[0], y=v[1])["host"], f64(single[:2]))
    assert same(ctx.krylov_vec_op(L.KVOP_NORM2_TRIPLE, n, ld, x=v[0], y=v[1], A=v[2])["host"], f64(single))


@pytest.mark.parametrize("n", [3, 1025, 4099, LARGE[2]])
def test_gram_is_symmetric_with_zero_padding(ctx, n):
    rng = np.random.default_rng(13000 + n)
    ld = R.ld_of(n)
    for k in (2, 3, 4):
        W, b = R.random_block(rng, n, ld, k), rng.standard_normal(n)
        out = ctx.krylov_vec_op(L.KVOP_GRAM, n, ld, k, A=W, x=b)["dev"]
        for i in range(k):
            for q in range(k):
                assert same(out[8 * i + q:8 * i + q + 1], out[8 * q + i:8 * q + i + 1]), (k, i, q)
        unused = [8 * i + q for i in range(k + 1) for q in range(k, 8)]
        assert same(out[unused], np.zeros(len(unused)))


# ---- determinism ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1027, 4099, LARGE[0]])
def test_reductions_are_deterministic(ctx, n):
    rng = np.random.default_rng(14000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    nvec = 9
    x, y, z = (rng.standard_normal(n) for _ in range(3))
    V, V32, h = R.random_block(rng, n, ld, nvec), R.random_block(rng, n, ld32, nvec, True), rng.standard_normal(nvec)
    hd, _ = R.diagonal_gram(rng, 4)
    calls = [
        (L.KVOP_DOT, ld, 1, dict(x=x, y=y)), (L.KVOP_NORM2_PAIR, ld, 1, dict(x=x, y=y)), (L.KVOP_NORM2_TRIPLE, ld, 1, dict(x=x, y=y, A=z)),
        (L.KVOP_NORMINF_DIFF, ld, 1, dict(x=x, y=y, flags=1)), (L.KVOP_SUB_MEAN, ld, 1, dict(x=x)),
        (L.KVOP_NORM_SCALE_INV, ld, 1, dict(x=x)), (L.KVOP_MULTIDOT, ld, nvec, dict(A=V, x=x, flags=1)),
        (L.KVOP_MULTIDOT32, ld32, nvec, dict(A=V32, x=x)), (L.KVOP_GRAM, ld, 3, dict(A=V[:3], x=x)), (L.KVOP_GRAM, ld, 7, dict(A=V[:7], x=x)),
        (L.KVOP_GS_UPDATE32, ld32, nvec, dict(A=V32, coef=h, x=x)), (L.KVOP_GUESS, ld, 4, dict(A=V[:4], B=V[4:8], coef=hd, x=x)),
    ]
    for op, l, nv, kw in calls:
        a, b = ctx.krylov_vec_op(op, n, l, nv, **kw), ctx.krylov_vec_op(op, n, l, nv, **kw)
        for key in a:
            assert same(a[key], b[key]), (op, key)


# ---- non-finite data ------------------------------------------------------------------------------------------------------------
def _bad_positions(n):
    # the scalar-tail entry; at the large sizes also entries of the last block of the chunked and of the grid-stride kernels
    return [n - 1] + ([n - 6, 1023 * 256 + 7] if n > 4099 else [])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("n", [5, 1027, 4099] + LARGE)
def test_one_non_finite_entry_reaches_the_affected_sums_only(ctx, n, bad):
    rng = np.random.default_rng(15000 + n)
    ld = R.ld_of(n)
    ld32 = R.ld32_of(ld)
    nvec = 9
    is_bad = np.isnan if np.isnan(bad) else (lambda v: np.isinf(v) & (v > 0))
    x0, y0, w0 = (f64(R.exact_vector(rng, n)) for _ in range(3))
    V0, V320 = f64(R.exact_block(rng, n, ld, nvec)), f64(R.exact_block(rng, n, ld32, nvec))
    for pos in _bad_positions(n):
        x, y, w, V, V32 = x0.copy(), y0.copy(), w0.copy(), V0.copy(), V320.copy()
        y[pos] = w[pos] = 1.0  # a product with the bad entry keeps its kind (inf * 0 would be NaN)
        x[pos] = bad
        o = ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=x, y=y)
        assert is_bad(o["host"][0]) and same(o["mirror"], o["dev"])
        o = ctx.krylov_vec_op(L.KVOP_NORM2_PAIR, n, ld, x=y, y=x)
        assert is_bad(o["host"][1]) and o["host"][0] == math.sqrt(R.norm2_sq(y))
        o = ctx.krylov_vec_op(L.KVOP_NORM2_TRIPLE, n, ld, x=y, y=x, A=w)
        assert is_bad(o["host"][1]) and o["host"][0] == math.sqrt(R.norm2_sq(y)) and o["host"][2] == math.sqrt(R.norm2_sq(w))
        for flags, yy in ((0, None), (1, y)):
            assert is_bad(ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=x, y=yy, flags=flags)["host"][0])
        assert is_bad(ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=y, y=x, flags=1)["host"][0])  # |1 - bad|
        V[5, pos] = V32[5, pos] = bad
        for op, l, blk in ((L.KVOP_MULTIDOT, ld, V), (L.KVOP_MULTIDOT32, ld32, V32)):
            o = ctx.krylov_vec_op(op, n, l, nvec, A=blk, x=w, flags=1 | RING)
            clean = blk.copy()
            clean[5, pos] = 0.0
            ref = R.multidot(clean.astype(np.int64), w.astype(np.int64), True)
            keep = np.arange(nvec + 1) != 5
            assert is_bad(o["dev"][5]) and same(o["dev"][keep], f64(ref)[keep]) and same(o["mirror"], o["dev"])
        if n <= 4099 or pos == n - 1:
            o = ctx.krylov_vec_op(L.KVOP_SUB_MEAN, n, ld, x=x)
            assert is_bad(o["dev"][0]) and (np.all(np.isnan(o["out1"])) if np.isnan(bad) else np.all(np.isinf(o["out1"][np.arange(n) != pos])))
            # Gram system: column 1 carries the entry; every slot with index 1 is affected, the others are exact
            k = 3
            W = V0[:k].copy()
            W[:, pos] = 1.0
            W[1, pos] = bad
            o = ctx.krylov_vec_op(L.KVOP_GRAM, n, ld, k, A=W, x=w)
            clean = W.copy()
            clean[1, pos] = 0.0
            ref = f64(R.gram(clean.astype(np.int64), w.astype(np.int64)))
            hit = np.zeros(8 * (k + 1), dtype=bool)
            for i in range(k + 1):
                for q in range(k):
                    hit[8 * i + q] = (i == 1 or q == 1)
            assert np.all(is_bad(o["dev"][hit])) and same(o["dev"][~hit], ref[~hit])
            # measured norm of an update, squared residual of the guess
            h = f64(R.exact_coef(rng, nvec))
            o = ctx.krylov_vec_op(L.KVOP_GS_UPDATE32, n, ld32, nvec, A=V320, coef=h, x=x)
            assert is_bad(o["dev"][0]) and same(o["mirror"][nvec + 1:], o["dev"])
            hd, yk = R.diagonal_gram(rng, k)
            o = ctx.krylov_vec_op(L.KVOP_GUESS, n, ld, k, A=V0[:k], B=V0[3:3 + k], coef=hd, x=x)
            assert is_bad(o["host"][0]) and same(o["out1"], f64(R.lincomb(V0[:k].astype(np.int64), yk, np.zeros(n, dtype=np.int64))))


@pytest.mark.parametrize("n", [1, 5, 1027, LARGE[1]])
def test_norminf_of_nan_is_nan(ctx, n):
    """fmax drops NaN: the inf-norm of a NaN field used to be 0, which Scenario.solve took for a steady state"""
    ld = R.ld_of(n)
    nan = np.full(n, np.nan)
    assert math.isnan(ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=nan)["host"][0])
    assert math.isnan(ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=nan, y=np.ones(n), flags=1)["host"][0])
    assert math.isnan(ctx.krylov_vec_op(L.KVOP_NORMINF_DIFF, n, ld, x=np.ones(n), y=nan, flags=1)["host"][0])


# ---- arguments the solver never produces are refused before anything is launched ------------------------------------------------
def test_bad_arguments_are_refused(ctx):
    n, ld = 5, 6
    x = np.ones(8)
    A = np.ones(8 * 9)
    hd = np.zeros(8 * 10)

    def refused(match, op, n, ld, nvec, **kw):
        with pytest.raises(ValueError, match=match):
            ctx.krylov_vec_op(op, n, ld, nvec, **kw)

    refused(r"odd ld = 5", L.KVOP_DOT, 5, 5, 1, x=x, y=x)
    refused(r"odd ld = 7", L.KVOP_MULTIDOT, 5, 7, 2, A=A, x=x)
    refused(r"ld = 6 is not a multiple of 4", L.KVOP_MULTIDOT32, n, ld, 2, A=A, x=x)
    refused(r"ld = 6 is not a multiple of 4", L.KVOP_GS_UPDATE32, n, ld, 2, A=A, coef=x, x=x)
    refused(r"ld = 4 < n = 5", L.KVOP_MULTIAXPY, 5, 4, 2, A=A, coef=x, x=x)
    refused(r"n = 0 < 1", L.KVOP_SCALE, 0, 2, 1, x=x)
    refused(r"n = -3 < 1", L.KVOP_SCALE, -3, 2, 1, x=x)
    refused(r"nvec = 0 < 1", L.KVOP_MULTIDOT, n, ld, 0, A=A, x=x)
    refused(r"k = 9 kept vectors outside 1 \.\. 8", L.KVOP_GUESS, n, ld, 9, A=A, B=A, coef=hd, x=x)
    refused(r"k = 9 kept vectors outside 1 \.\. 8", L.KVOP_GRAM, n, ld, 9, A=A, x=x)
    refused(r"unknown op 22", 22, n, ld, 1, x=x)
    refused(r"unknown op -1", -1, n, ld, 1, x=x)
    refused(r"misses an array", L.KVOP_DOT, n, ld, 1, x=x)
    # the context still works
    assert ctx.krylov_vec_op(L.KVOP_DOT, n, ld, x=x, y=x)["host"][0] == 5.0
