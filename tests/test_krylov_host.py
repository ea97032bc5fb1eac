"""Host arithmetic of the linear solve (csrc/cfdh_krylov_host.hpp) on the CPU: the header is compiled with g++ behind the
extern "C" wrappers of krylov_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
EPS = np.finfo(float).eps
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def kh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("krylov_host") / "krylov_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC,
                           os.path.join(HERE, "krylov_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.kh_gram_solve.argtypes = [ctypes.c_int, dp, dp, ctypes.POINTER(ctypes.c_int)]
    L.kh_gs_scale.argtypes = [ctypes.c_double, ctypes.c_double]
    L.kh_gs_scale.restype = ctypes.c_double
    for name in ("kh_lsq_new", "kh_ahead_new"):
        getattr(L, name).restype = ctypes.c_void_p
    L.kh_lsq_new.argtypes = [ctypes.c_int]
    L.kh_lsq_free.argtypes = [ctypes.c_void_p]
    L.kh_lsq_start.argtypes = [ctypes.c_void_p, ctypes.c_double]
    L.kh_lsq_add_column.argtypes = [ctypes.c_void_p, ctypes.c_int, dp, ctypes.c_double]
    L.kh_lsq_residual.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.kh_lsq_residual.restype = ctypes.c_double
    L.kh_lsq_solve.argtypes = [ctypes.c_void_p, ctypes.c_int, dp]
    L.kh_ahead_free.argtypes = [ctypes.c_void_p]
    L.kh_ahead_start.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    L.kh_ahead_observe.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_int]
    L.kh_ahead_need.argtypes = [ctypes.c_void_p]
    L.kh_ahead_set_need.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.kh_ahead_in_flight.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.kh_ahead_process_upto.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 4
    ipt = ctypes.POINTER(ctypes.c_int)
    L.kh_between_cycles.argtypes = [ctypes.c_int] + [ctypes.c_double] * 6 + [ctypes.c_int] * 3 + [ipt, ipt, dp]
    L.kh_between_cycles.restype = None
    return L


def ptr(a):
    return a.ctypes.data_as(dp)


def device_layout(G, g):
    """hd[8 i + q] = W_q . W_i (i < k), hd[8 k + q] = W_q . b"""
    k = len(g)
    hd = np.zeros(8 * (k + 1))
    for i in range(k):
        hd[8 * i:8 * i + k] = G[:, i]
    hd[8 * k:8 * k + k] = g
    return hd


def gram_solve(kh, G, g):
    k = len(g)
    hd = device_layout(np.asarray(G, float), np.asarray(g, float))
    y = np.full(8, 7.0)  # every entry up to k must be written
    rank = ctypes.c_int(-1)
    used = kh.kh_gram_solve(k, ptr(hd), ptr(y), ctypes.byref(rank))
    return bool(used), rank.value, y[:k].copy()


def scaled_columns(rng, k):
    W = rng.standard_normal((64, k)) * 10.0 ** rng.uniform(-3, 3, k)
    return W, rng.standard_normal(64)


# ---- Gram solve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(1, 9))
def test_gram_full_rank(kh, k):
    # bound: a NumPy restatement of the algorithm over 300 seeds x 8 sizes of these inputs had a worst componentwise backward
    # error of 0.79 k eps; the factor of five covers another summation order and FMA contraction
    for seed in range(5):
        W, b = scaled_columns(np.random.default_rng(1000 * k + seed), k)
        G, g = W.T @ W, W.T @ b
        used, rank, y = gram_solve(kh, G, g)
        assert used and rank == k
        berr = np.max(np.abs(G @ y - g) / (np.abs(G) @ np.abs(y) + np.abs(g)))
        assert berr <= 4 * k * EPS, (seed, berr / (k * EPS))


def _dependent_case(rng, k):
    W, b = scaled_columns(rng, k)
    if k == 4:
        W[:, 3] = W[:, 1]
        return W, b, 3
    W[:, 5] = 3.0 * W[:, 0]
    W[:, 7] = W[:, 2] - W[:, 4]
    return W, b, 6


@pytest.mark.parametrize("k", [4, 8])
def test_gram_dependent_columns(kh, k):
    # (the restatement over 200 seeds each: these ranks every time, worst relative difference of the residuals 2.6e-16)
    for seed in range(5):
        W, b, want = _dependent_case(np.random.default_rng(77 * k + seed), k)
        used, rank, y = gram_solve(kh, W.T @ W, W.T @ b)
        assert used and rank == want
        assert np.count_nonzero(y == 0.0) == k - want  # the dropped columns
        ref = np.linalg.norm(b - W @ np.linalg.lstsq(W, b, rcond=None)[0])
        assert abs(np.linalg.norm(b - W @ y) - ref) <= 1e-12 * ref


def test_gram_degenerate(kh):
    used, rank, y = gram_solve(kh, np.zeros((3, 3)), np.ones(3))
    assert (used, rank) == (False, 0) and np.all(y == 0.0)
    G = np.eye(3)
    G[2, 2] = np.nan
    used, rank, y = gram_solve(kh, G, np.ones(3))
    assert (used, rank) == (False, 0) and np.all(y == 0.0)
    used, rank, y = gram_solve(kh, np.eye(3), np.array([1.0, np.inf, 1.0]))
    assert not used and np.all(y == 0.0)


# ---- Arnoldi recurrence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 7, 30])
def test_recurrence(kh, m):
    rng = np.random.default_rng(m)
    H = np.triu(np.eye(m + 1, m) + 0.3 * rng.standard_normal((m + 1, m)), -1)
    q = kh.kh_lsq_new(m)
    try:
        kh.kh_lsq_start(q, 1.0)
        for j in range(m):
            col = np.ascontiguousarray(H[:j + 1, j])
            assert kh.kh_lsq_add_column(q, j, ptr(col), H[j + 1, j]) == 1
            Hj = H[:j + 2, :j + 1]
            e1 = np.zeros(j + 2)
            e1[0] = 1.0
            yref = np.linalg.lstsq(Hj, e1, rcond=None)[0]
            bound = 100 * m * EPS * np.linalg.cond(Hj)
            assert abs(kh.kh_lsq_residual(q, j + 1) - np.linalg.norm(e1 - Hj @ yref)) <= bound
            y = np.zeros(j + 1)
            kh.kh_lsq_solve(q, j + 1, ptr(y))
            assert np.linalg.norm(y - yref) <= bound * np.linalg.norm(yref)
    finally:
        kh.kh_lsq_free(q)


def test_recurrence_breakdown(kh):
    q = kh.kh_lsq_new(3)
    try:
        kh.kh_lsq_start(q, 1.0)
        col = np.array([1.0, 0.0])
        assert kh.kh_lsq_add_column(q, 0, ptr(col), 0.5) == 1
        zero = np.zeros(2)
        assert kh.kh_lsq_add_column(q, 1, ptr(zero), 0.0) == 0
    finally:
        kh.kh_lsq_free(q)


# ---- launch-ahead policy ---------------------------------------------------------------------------------------------------
TOL, LAGMAX = 1e-5, 9


@pytest.fixture()
def ahead(kh):
    p = kh.kh_ahead_new()
    yield p
    kh.kh_ahead_free(p)


def test_ahead_start(kh, ahead):
    kh.kh_ahead_start(ahead, 1.0, 0, 0)
    assert kh.kh_ahead_need(ahead) == 1 and kh.kh_ahead_in_flight(ahead, 0, LAGMAX) == 1
    kh.kh_ahead_start(ahead, 1.0, 10, 0)
    assert kh.kh_ahead_need(ahead) == 3


@pytest.mark.parametrize("e_its, its, need, in_flight", [(0, 0, 15, 10), (6, 2, 6, 5)])
def test_ahead_rate(kh, ahead, e_its, its, need, in_flight):
    kh.kh_ahead_start(ahead, 1.0, e_its, 0)
    kh.kh_ahead_observe(ahead, 0.5, TOL, 1 if e_its else 0)
    assert kh.kh_ahead_need(ahead) == 3  # one sample of the rate is capped at 3
    kh.kh_ahead_observe(ahead, 0.25, TOL, its)
    assert math.ceil(math.log(4e-5) / math.log(0.5)) == 15
    assert kh.kh_ahead_need(ahead) == need
    assert kh.kh_ahead_in_flight(ahead, 0, LAGMAX) == in_flight
    assert kh.kh_ahead_in_flight(ahead, 1, LAGMAX) == 1  # sync_now: always 1


def test_ahead_stagnation(kh, ahead):
    kh.kh_ahead_start(ahead, 1.0, 0, 0)
    kh.kh_ahead_observe(ahead, 0.98, TOL, 1)
    kh.kh_ahead_observe(ahead, 0.98 ** 2, TOL, 2)
    assert kh.kh_ahead_need(ahead) == 1 << 20
    assert kh.kh_ahead_in_flight(ahead, 0, LAGMAX) == LAGMAX + 1
    assert kh.kh_ahead_in_flight(ahead, 1, LAGMAX) == 1


def test_ahead_process_upto(kh, ahead):
    maxl = 6
    for need, sync_now, j, jl in itertools.product([1, 2, 3, 5], [0, 1], range(0, maxl), range(1, maxl + 1)):
        if jl <= j:
            continue
        kh.kh_ahead_set_need(ahead, need)
        leave = (not sync_now) and jl - j > 1 and jl < maxl and need > jl - j
        assert kh.kh_ahead_process_upto(ahead, j, jl, maxl, sync_now) == (jl - 1 if leave else jl)


# ---- scale of a Gram-Schmidt pass ------------------------------------------------------------------------------------------
def test_gs_scale(kh):
    assert kh.kh_gs_scale(4.0, 3.0) == 1.0               # nrm2 in (0, ww]
    assert kh.kh_gs_scale(4.0, 0.0) == 2.0               # nrm2 = ww
    assert kh.kh_gs_scale(4.0, 4.0) == 2.0               # nrm2 = 0: cancelled
    assert kh.kh_gs_scale(4.0, 5.0) == 2.0               # nrm2 < 0
    assert kh.kh_gs_scale(4.0, -5.0) == 2.0              # nrm2 > ww
    assert kh.kh_gs_scale(0.0, 0.0) == 0.0


# ---- the checks between two cycles -----------------------------------------------------------------------------------------
PROCEED, RETRY, STOP = 0, 1, 2
QUIET, FP32_OFF, REFINE_ON = 0, 1, 2


def between(kh, j_prev=5, beta=1.0, est_prev=1.0, tol=1e-5, bn=1.0, beta_start=10.0, last_true=-1.0, use32=0, refine=0, no_stop=0):
    flow, dog, lt = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_double(np.nan)
    kh.kh_between_cycles(j_prev, beta, est_prev, tol, bn, beta_start, last_true, use32, refine, no_stop,
                         ctypes.byref(flow), ctypes.byref(dog), ctypes.byref(lt))
    return flow.value, dog.value, lt.value


def test_between_watchdog_threshold(kh):
    # trips strictly above 10 max(est, tol); the estimate bounds it when it is the larger of the two, the tolerance otherwise
    est, tol = 3e-4, 1e-5
    up = np.nextafter(10.0 * est, np.inf)
    assert between(kh, beta=10.0 * est, est_prev=est, tol=tol) == (PROCEED, QUIET, -1.0)
    assert between(kh, beta=up, est_prev=est, tol=tol) == (PROCEED, REFINE_ON, -1.0)
    est, tol = 1e-7, 1e-5
    up = np.nextafter(10.0 * tol, np.inf)
    assert between(kh, beta=10.0 * tol, est_prev=est, tol=tol, no_stop=1) == (PROCEED, QUIET, -1.0)
    assert between(kh, beta=up, est_prev=est, tol=tol, no_stop=1) == (PROCEED, REFINE_ON, -1.0)
    # no cycle behind this residual (first pass after a take-back is j_prev > 0; j_prev = 0 never trips)
    assert between(kh, j_prev=0, beta=1e3, est_prev=1e-9) == (PROCEED, QUIET, -1.0)
    # the fp32 copy is the first suspect, whether or not the context refines already; no take-back with it
    for refine in (0, 1):
        assert between(kh, beta=1.0, est_prev=1e-3, beta_start=0.5, use32=1, refine=refine) == (PROCEED, FP32_OFF, -1.0)
    assert between(kh, beta=1e-3, est_prev=1e-3, use32=1) == (PROCEED, QUIET, -1.0)


def test_between_retry(kh):
    # taken back only when the cycle made the true residual worse (strictly), and only by the trip that switches refinement on
    assert between(kh, beta=1.0, est_prev=1e-3, beta_start=1.0) == (PROCEED, REFINE_ON, -1.0)
    assert between(kh, beta=1.0, est_prev=1e-3, beta_start=np.nextafter(1.0, 0.0)) == (RETRY, REFINE_ON, -1.0)
    assert between(kh, beta=1.0, est_prev=1e-3, beta_start=0.5, refine=1) == (PROCEED, QUIET, -1.0)
    # a take-back leaves last_true alone (the cycle did not happen)
    assert between(kh, beta=1.0, est_prev=1e-9, tol=1e-5, beta_start=0.5, last_true=0.25) == (RETRY, REFINE_ON, 0.25)
    # not lost: no retry however the residual moved
    assert between(kh, beta=1.0, est_prev=0.2, beta_start=0.5) == (PROCEED, QUIET, -1.0)


def test_between_attainable_stop(kh):
    tol, bn = 1e-5, 1.0
    conv = dict(est_prev=0.9 * tol, tol=tol, bn=bn, refine=1)
    # first recurrence-converged cycle whose true residual stays above the tolerance: remembered, no stop
    assert between(kh, beta=3 * tol, last_true=-1.0, **conv) == (PROCEED, QUIET, 3 * tol)
    # the second in a row stops if the residual was not halved (strictly above half) ...
    assert between(kh, beta=3 * tol, last_true=4 * tol, **conv) == (STOP, QUIET, 4 * tol)
    assert between(kh, beta=2 * tol, last_true=4 * tol, **conv) == (PROCEED, QUIET, 2 * tol)
    assert between(kh, beta=np.nextafter(2 * tol, 1.0), last_true=4 * tol, **conv) == (STOP, QUIET, 4 * tol)
    # ... and only within 10 tol or six orders below |b|
    assert between(kh, beta=10 * tol, last_true=10 * tol, **conv) == (STOP, QUIET, 10 * tol)
    b11 = np.nextafter(10 * tol, 1.0)
    assert between(kh, beta=b11, last_true=b11, **conv) == (PROCEED, QUIET, b11)
    big = dict(conv, bn=1e3)               # 1e-6 |b| = 1e-3 = 100 tol
    assert between(kh, beta=1e-6 * 1e3, last_true=1e-3, **big) == (STOP, QUIET, 1e-3)
    b = np.nextafter(1e-6 * 1e3, 1.0)
    assert between(kh, beta=b, last_true=b, **big) == (PROCEED, QUIET, b)
    # the recurrence estimate has to be at or below the tolerance, the true residual above it
    assert between(kh, beta=3 * tol, est_prev=tol, tol=tol, last_true=4 * tol, refine=1) == (STOP, QUIET, 4 * tol)
    assert between(kh, beta=3 * tol, est_prev=np.nextafter(tol, 1.0), tol=tol, last_true=4 * tol, refine=1) == (PROCEED, QUIET, -1.0)
    assert between(kh, beta=tol, last_true=4 * tol, **conv) == (PROCEED, QUIET, -1.0)
    # a cycle that ended at the restart length in between resets the memory: the next converged one is a FIRST again
    f, w, lt = between(kh, beta=3 * tol, last_true=-1.0, **conv)
    f, w, lt = between(kh, beta=3 * tol, est_prev=2.5 * tol, tol=tol, last_true=lt, refine=1)
    assert (f, w, lt) == (PROCEED, QUIET, -1.0)
    assert between(kh, beta=3 * tol, last_true=lt, **conv) == (PROCEED, QUIET, 3 * tol)
    # no cycle yet
    assert between(kh, j_prev=0, beta=3 * tol, last_true=4 * tol, **conv) == (PROCEED, QUIET, -1.0)
    # the watchdog's switches do not shadow the stop: six orders below |b|, lost by more than 10 tol
    assert between(kh, beta=50 * tol, est_prev=0.9 * tol, tol=tol, bn=1e3, last_true=60 * tol, use32=1) == (STOP, FP32_OFF, 60 * tol)
    assert between(kh, beta=50 * tol, est_prev=0.9 * tol, tol=tol, bn=1e3, beta_start=1.0, last_true=60 * tol) == (STOP, REFINE_ON, 60 * tol)


def test_between_no_attainable_stop_switch(kh):
    tol = 1e-5
    assert between(kh, beta=3 * tol, est_prev=0.9 * tol, tol=tol, last_true=4 * tol, refine=1, no_stop=0)[0] == STOP
    # switched off: never a stop, and nothing is remembered
    assert between(kh, beta=3 * tol, est_prev=0.9 * tol, tol=tol, last_true=4 * tol, refine=1, no_stop=1) == (PROCEED, QUIET, -1.0)
