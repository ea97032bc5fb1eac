"""gram_solve_kernel<K> (csrc/cfdh_krylov_vec.hip): the K x K Gram system of the projected guess solved by one lane out of registers,
K = 1 .. 8, through cfdh_krylov_vec_op (KVOP_GUESS), which hands the kernel a Gram system given word by word.

What is compared, per fixed system of tests/golden/gram_solve_regs.json:
  * y (the host-mapped words and the device copy guess_combine_kernel reads), the rank and the "used" flag against the output of the
    kernel this one replaces (one kernel for all k, working out of scratch memory), recorded on an MI355X: BIT FOR BIT.  The golden
    file holds the inputs as well (hex doubles), so the comparison depends neither on a random generator nor on a BLAS.
  * used and rank against cfdh_krylov::gram_solve compiled for the host (the fixture of test_krylov_host.py), and y up to the one
    documented difference: hipcc contracts the multiply-subtracts of the Cholesky that the host build does not.
    Every entry of the factor and of y then carries at most K + 2 roundings that differ, each amplified by at most the condition of
    G in the solve: |y_dev - y_host| <= 8 (K + 2) K eps cond(G) max|y|, cond taken of the rows and columns the solve kept.  The
    systems are built with cond <= 1e6 for this purpose.

Systems (G = W^T W, g = W^T b from seeded normal W [12 x K] and b): one SPD system for each K (columns scaled by 0.1, 1 or 10, so
that the pivot order is not the natural one), two numerically rank-deficient ones (exactly dependent columns: rank < K, the guess
still used), a diagonal of NaN (rank 0, not used) and a NaN in the right-hand side (full rank, y not finite, not used) -- the
branches no whole solve of the suite reaches.

Kernel times of these launches (MI355X, median of five): 2.2 / 2.6 / 3.1 / 4.1 / 5.9 / 8.0 / 8.2 / 12.4 us for K = 1 .. 8, against
4.0 / 6.8 / 10.2 / 15.6 / 21.1 / 28.5 / 36.0 / 46.9 us of the kernel replaced.
"""
import json
import os

import numpy as np
import pytest

import krylov_vec_ref as R
from cfd_hemodynamic_amd import _lib as L
from test_krylov_host import gram_solve, kh  # noqa: F401  (the fixture compiles csrc/cfdh_krylov_host.hpp for the host)
from util import dfg_case, make_ctx

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gram_solve_regs.json")
EPS = np.finfo(float).eps
N = 3  # length of the vectors the guess is combined from: the solve does not see them


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=np.float64).ravel()]


def unhex(h):
    return np.array([float.fromhex(v) for v in h], dtype=np.float64)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def run(ctx, k, hd):
    """(used, rank, y in the host-mapped words, y on the device) of one launch"""
    rng = np.random.default_rng(17)
    ld = R.ld_of(N)
    Um, Wm, b = R.exact_block(rng, N, ld, k), R.exact_block(rng, N, ld, k), R.exact_vector(rng, N)
    o = ctx.krylov_vec_op(L.KVOP_GUESS, N, ld, k, A=Um, B=Wm, coef=hd, x=b)
    return int(o["mirror"][1]), int(o["mirror"][2]), np.array(o["mirror"][3:3 + k]), np.array(o["dev"][1:1 + k])


with open(GOLDEN) as _f:
    RECORDED = json.load(_f)


@pytest.fixture(scope="module")
def golden():
    return RECORDED


@pytest.fixture(scope="module")
def ctx():
    return make_ctx(dfg_case(4))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECORDED))
def test_equals_the_scratch_memory_kernel_bit_for_bit(ctx, golden, name):
    rec = golden[name]
    k, hd = rec["k"], unhex(rec["hd"])
    used, rank, y, ydev = run(ctx, k, hd)
    print("%s: used %d rank %d y %s" % (name, used, rank, hexes(y)))
    assert (used, rank) == (rec["used"], rec["rank"])
    assert same(y, unhex(rec["y"])) and same(ydev, y)
    if name.startswith("spd"):
        assert used == 1 and rank == k
    elif name.startswith("rankdef"):
        assert used == 1 and 0 < rank < k and np.count_nonzero(y) == rank
    elif name == "nan_diagonal_k3":
        assert used == 0 and rank == 0 and same(y, np.zeros(k))
    else:
        assert used == 0 and rank == k and same(y, np.zeros(k))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RECORDED))
def test_agrees_with_the_host_build(ctx, kh, golden, name):  # noqa: F811
    rec = golden[name]
    k, hd = rec["k"], unhex(rec["hd"])
    G = np.array([[hd[8 * i + q] for i in range(k)] for q in range(k)])
    hused, hrank, hy = gram_solve(kh, G, hd[8 * k:8 * k + k])
    used, rank, y, _ = run(ctx, k, hd)
    assert (used, rank) == (int(hused), hrank)
    if not used:
        assert same(y, hy)
        return
    taken = np.flatnonzero(hy)
    assert np.array_equal(np.flatnonzero(y), taken)
    cond = np.linalg.cond(G[np.ix_(taken, taken)])
    assert cond <= 1e6, cond
    bound = 8 * (k + 2) * k * EPS * cond * np.abs(hy).max()
    err = np.abs(y - hy).max()
    print("%s: cond %.2e |y_dev - y_host| %.3e bound %.3e" % (name, cond, err, bound))
    assert err <= bound
