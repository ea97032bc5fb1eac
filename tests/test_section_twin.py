"""The cut-plane sections on the CPU: the brute-force NumPy twin (section_twin.py) against closed forms, the conditions the GPU
tests rest on (clip balls with straddling == 0), build_cut and the per-entry arithmetic of csrc/cfdh_section_host.hpp (compiled with
g++ behind the extern "C" wrappers of section_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU) against the twin, the
same header once more in a stand-alone program built with AddressSanitizer and UBSan (section_host_main.cpp, a child process), the
helpers of cfd_hemodynamic_amd/sections.py and the Python refusals."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import sample_util as SU
import section_twin as T
import section_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
dp = ctypes.POINTER(ctypes.c_double)
lp = ctypes.POINTER(ctypes.c_longlong)
bp = ctypes.POINTER(ctypes.c_ubyte)


# --------------------------------------------------------------------------------------------------------------------- the twin
def test_moments():
    M1, M2, M3 = T.moments(2)
    assert np.allclose(M1, 1 / 3) and np.allclose(M2, (1 + np.eye(3)) / 12)
    assert np.isclose(M3[0, 0, 0], 1 / 10) and np.isclose(M3[0, 0, 1], 1 / 30) and np.isclose(M3[0, 1, 2], 1 / 60)
    assert np.isclose(M1.sum(), 1) and np.isclose(M2.sum(), 1) and np.isclose(M3.sum(), 1)
    M1, M2, M3 = T.moments(1)
    assert np.allclose(M1, 1 / 2) and np.allclose(M2, (1 + np.eye(2)) / 6)
    assert np.isclose(M3[0, 0, 0], 1 / 4) and np.isclose(M3[0, 0, 1], 1 / 12) and np.isclose(M3.sum(), 1)


@pytest.mark.parametrize("name", ["cube", "square"])
def test_twin_areas_and_affine_closed_forms(name):
    """The areas of the issue, and every slot for affine fields against the integral over the analytically known polygon."""
    m = U.mesh(name)
    u, p, ufun, pfun = U.affine_state(m)
    for key, c in U.cases(name).items():
        sec = U.twin_cuts(name)[key]
        print(key, "cells", len(sec.cells), "area", sec.measure.sum())
        assert abs(sec.measure.sum() - c["area"]) <= U.TOL_EXACT, key
        assert (np.diff(sec.cells) > 0).all()
        row = T.rows(sec, m.cells, u, p, U.RHO)
        if c["area"] == 0.0:
            assert len(sec.cells) == 0 and (row == 0.0).all() and not np.signbit(row).any()
            continue
        want = T.polygon_rows(c["polygon"], ufun, pfun, c["normal"], U.RHO)
        assert U.worst(name + " " + key, row, want, U.TOL_EXACT * U.row_scale(c["area"], u, p))
    if name == "cube":
        # a plane of mesh facets is seen from below only: no cell with a vertex beyond x = 0.5; 32 cells have a facet in it, and
        # the cells below that touch it with an edge or a vertex are cut in a polygon of measure 0
        sec = U.twin_cuts(name)["x05_facets"]
        assert (m.x[m.cells[sec.cells], 0].max(axis=1) <= 0.5).all() and (sec.measure > 0).sum() == 32
        assert np.allclose(sec.measure[sec.measure > 0], 1 / 32, rtol=0, atol=1e-15)


def test_clip_balls_of_the_gpu_tests():
    """The two balls select one daughter each with straddling == 0 and add up to the unbounded plane; the bad ball straddles."""
    m = U.mesh("bifurcation")
    cuts = U.twin_cuts("bifurcation")
    both, left, right = cuts["both"], cuts["left"], cuts["right"]
    assert left.straddling == 0 and right.straddling == 0 and cuts["left_oblique"].straddling == 0
    assert len(left.cells) > 20 and len(right.cells) > 20 and len(cuts["parent"].cells) > 20
    assert np.array_equal(np.sort(np.concatenate([left.cells, right.cells])), both.cells)
    u, p = U.random_state("bifurcation")
    r = [T.rows(s, m.cells, u, p, U.RHO) for s in (both, left, right)]
    assert U.worst("left + right = both", r[1] + r[2], r[0], U.TOL_EXACT * U.row_scale(r[0], u, p))
    assert cuts["bad_ball"].straddling > 0 and 0 < len(cuts["bad_ball"].cells) < len(right.cells)
    bad = U.twin_cuts("stenosis")["bad_ball"]
    assert bad.straddling > 0 and len(bad.cells) > 0
    for key in ("proximal", "throat", "distal", "oblique", "inlet_outward"):
        assert len(U.twin_cuts("stenosis")[key].cells) >= 3, key
    # the channel is narrower at the throat
    assert U.twin_cuts("stenosis")["throat"].measure.sum() < 0.95 * U.twin_cuts("stenosis")["proximal"].measure.sum()


# ------------------------------------------------------------------------------------------------------------------ the header
@pytest.fixture(scope="module")
def sh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("section_host") / "section_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "section_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int = ctypes.c_int
    L.sc_build.argtypes = [c_int, c_int, c_int, dp, ip, ip, bp, c_int, dp, ctypes.c_longlong, lp, ctypes.c_char_p, c_int]
    L.sc_get.argtypes = [lp, ip, ip, dp, dp, ip, dp]
    L.sc_eval.argtypes = [ip, dp, dp, ctypes.c_double, dp]
    return L


def build(sh, x, cells, cs, caller_index=None, flipped=None, max_entries=0, planes=None, K=None, fields=()):
    """(0, cut) or (-1, message).  cut: ptr, cell (stored ids), code, t, meas, straddling, normal, and rows: [K, 10] per (u, p) of
    `fields`, evaluated at once (the shim keeps the cut built last)."""
    d = x.shape[1]
    cells = np.ascontiguousarray(cells, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    if planes is None:
        o, n, r = U.arrays(cs)
        planes = np.hstack([o, n, r[:, None]])
    planes = np.ascontiguousarray(planes, dtype=np.float64)
    K = len(planes) if K is None else K
    sizes = np.zeros(2, dtype=np.int64)
    msg = ctypes.create_string_buffer(256)
    ci = None if caller_index is None else np.ascontiguousarray(caller_index, dtype=np.int32)
    fl = None if flipped is None else np.ascontiguousarray(flipped, dtype=np.uint8)
    rc = sh.sc_build(d, len(x), len(cells), x.ctypes.data_as(dp), cells.ctypes.data_as(ip), None if ci is None else ci.ctypes.data_as(ip),
                     None if fl is None else fl.ctypes.data_as(bp), K, planes.ctypes.data_as(dp), max_entries, sizes.ctypes.data_as(lp), msg, 256)
    if rc != 0:
        return rc, msg.value.decode()
    total, np_, nt = int(sizes[0]), (2 if d == 2 else 4), (1 if d == 2 else 2)
    C = types.SimpleNamespace(total=total, maxlen=int(sizes[1]), ptr=np.zeros(K + 1, dtype=np.int64), cell=np.zeros(total, dtype=np.int32),
                              code=np.zeros(total, dtype=np.int32), t=np.zeros((total, np_)), meas=np.zeros((total, nt)),
                              straddling=np.zeros(K, dtype=np.int32), normal=np.zeros((K, 3)))
    sh.sc_get(C.ptr.ctypes.data_as(lp), C.cell.ctypes.data_as(ip), C.code.ctypes.data_as(ip), C.t.ctypes.data_as(dp), C.meas.ctypes.data_as(dp),
              C.straddling.ctypes.data_as(ip), C.normal.ctypes.data_as(dp))

    def evaluate(u, p, rho=U.RHO):
        out = np.full((K, 10), np.nan)
        u, p = np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(p, dtype=np.float64)
        sh.sc_eval(cells.ctypes.data_as(ip), u.ctypes.data_as(dp), p.ctypes.data_as(dp), rho, out.ctypes.data_as(dp))
        return out
    C.rows = [evaluate(u, p) for u, p in fields]
    return 0, C


@pytest.mark.parametrize("d", [2, 3])
def test_every_split_of_one_cell(sh, d):
    """All 6 splits of a triangle and all 14 of a tetrahedron, in both stored orientations: the affine function with chosen vertex
    values of either sign defines the plane; measure and rows against the twin."""
    rng = np.random.default_rng(5)
    x = np.vstack([np.zeros(d), np.eye(d)]) + rng.uniform(-0.1, 0.1, (d + 1, d))
    cell = np.arange(d + 1, dtype=np.int32)[None, :]
    u, p = rng.uniform(-1, 1, (d + 1, d)), rng.uniform(-1, 1, d + 1)
    splits = T.all_splits(d)
    assert len(splits) == (6 if d == 2 else 14)
    cs = []
    for above in splits:
        s = -rng.uniform(0.2, 1.0, d + 1)
        s[list(above)] *= -1.0
        sol = np.linalg.solve(np.hstack([x, np.ones((d + 1, 1))]), s)       # s_v = g . x_v + c
        g, c = sol[:d], sol[d]
        cs.append(U.case(-c * g / (g @ g), g))
    swapped = cell.copy()
    swapped[0, [d - 1, d]] = swapped[0, [d, d - 1]]
    for stored, flipped in ((cell, None), (swapped, np.ones(1, dtype=np.uint8))):
        rc, C = build(sh, x, stored, cs, flipped=flipped, fields=[(u, p)])
        assert rc == 0, C
        assert np.array_equal(C.ptr, np.arange(len(cs) + 1)) and C.maxlen == 1
        got = C.rows[0]
        for k, (above, c) in enumerate(zip(splits, cs)):
            sec = T.cut(x, cell, c["origin"], c["normal"])
            assert len(sec.cells) == 1
            npoly = (C.code[k] >> 16) & 7
            assert npoly == (2 if d == 2 else (4 if len(above) == 2 else 3))
            assert abs(C.meas[k].sum() - sec.measure[0]) <= U.TOL_EXACT
            want = T.rows(sec, cell, u, p, U.RHO)
            assert U.worst("split %s" % (above,), got[k], want, U.TOL_EXACT * U.row_scale(max(want[0], 1e-300), u, p))
        if flipped is None:
            first = (C.t.copy(), C.meas.copy())
        else:  # the polygon is built in the caller's local order: t and the measures do not see the stored orientation
            assert np.array_equal(first[0], C.t) and np.array_equal(first[1], C.meas)


@pytest.mark.parametrize("name", U.MESHES)
def test_lists_against_the_twin(sh, name):
    """Cells in ascending order, measures, straddling, the longest list, and the rows of an affine and a random field."""
    m = U.mesh(name)
    keys = list(U.cases(name))
    u, p = U.random_state(name)
    ua, pa = U.affine_state(m)[:2]
    rc, C = build(sh, m.x, m.cells, [U.cases(name)[k] for k in keys], fields=[(u, p), (ua, pa)])
    assert rc == 0, C
    got, got_a = C.rows
    longest = 0
    for k, key in enumerate(keys):
        sec = U.twin_cuts(name)[key]
        lo, hi = C.ptr[k], C.ptr[k + 1]
        print(name, key, "entries", hi - lo, "straddling", C.straddling[k])
        assert np.array_equal(C.cell[lo:hi], sec.cells), key
        assert C.straddling[k] == sec.straddling
        scale = max(sec.measure.sum(), 1e-300)
        assert U.worst(key + " measures", C.meas[lo:hi].sum(axis=1), sec.measure, U.TOL_EXACT * scale)
        assert U.worst(key + " random", got[k], T.rows(sec, m.cells, u, p, U.RHO), U.TOL_EXACT * U.row_scale(scale, u, p))
        assert U.worst(key + " affine", got_a[k], T.rows(sec, m.cells, ua, pa, U.RHO), U.TOL_EXACT * U.row_scale(scale, ua, pa))
        if hi == lo:
            assert (got[k] == 0.0).all() and not np.signbit(got[k]).any()
        if m.d == 2:
            assert (got[k, 9] == 0.0) and not np.signbit(got[k, 9])
        longest = max(longest, hi - lo)
    assert C.maxlen == longest and C.total == C.ptr[-1]
    assert ((C.t >= 0.0) & (C.t < 1.0)).all() and (C.meas >= 0.0).all()


@pytest.mark.parametrize("name", ["square", "bifurcation"])
def test_lists_do_not_depend_on_numbering_or_storage(sh, name):
    """(a) The caller renumbers the cells and reorders their vertices: the lists are permuted accordingly, the rows agree.
    (b) The context stores the cells in another order and orientation than the caller: the same lists in the caller's ids."""
    m, q = U.mesh(name), SU.permuted(name)
    keys = list(U.cases(name))
    cs = [U.cases(name)[k] for k in keys]
    u, p = U.random_state(name)
    rc, C = build(sh, m.x, m.cells, cs, fields=[(u, p)])
    rc2, Q = build(sh, q.x, q.cells, cs, fields=[(u, p)])
    assert rc == 0 and rc2 == 0
    assert np.array_equal(Q.ptr, C.ptr) and np.array_equal(Q.straddling, C.straddling)
    for k in range(len(cs)):
        lo, hi = C.ptr[k], C.ptr[k + 1]
        assert np.array_equal(Q.cell[lo:hi], np.sort(q.new_of_old[C.cell[lo:hi]]))
        order = np.argsort(q.new_of_old[C.cell[lo:hi]])
        scale = max(C.meas[lo:hi].sum(), 1e-300)
        assert U.worst("measures", Q.meas[lo:hi].sum(axis=1), C.meas[lo:hi].sum(axis=1)[order], U.TOL_EXACT * scale)
    rows, rows_q = C.rows[0], Q.rows[0]
    for k in range(len(cs)):
        assert U.worst(keys[k] + " rows", rows_q[k], rows[k], U.TOL_EXACT * U.row_scale(max(rows[k, 0], 1e-300), u, p))
    # (b): stored cell e is the caller's cell user_of[e], every second one with its last two vertices swapped
    rng = np.random.default_rng(3)
    user_of = rng.permutation(m.nc).astype(np.int32)
    stored = m.cells[user_of].copy()
    flipped = (np.arange(m.nc) % 2).astype(np.uint8)
    sw = flipped == 1
    stored[sw, -2], stored[sw, -1] = stored[sw, -1].copy(), stored[sw, -2].copy()
    rc, S = build(sh, m.x, stored, cs, caller_index=user_of, flipped=flipped, fields=[(u, p)])
    assert rc == 0, S
    assert np.array_equal(S.ptr, C.ptr) and np.array_equal(user_of[S.cell], C.cell) and np.array_equal(S.straddling, C.straddling)
    assert np.array_equal(S.t, C.t) and np.array_equal(S.meas, C.meas)
    for k in range(len(cs)):  # the same polygon vertices; the two terms of an interpolation may be added in the other order
        assert U.worst(keys[k] + " rows, stored", S.rows[0][k], rows[k], U.TOL_EXACT * U.row_scale(max(rows[k, 0], 1e-300), u, p))


def test_refusals(sh):
    m = U.mesh("square")
    cs = [U.SQUARE["x037"], U.SQUARE["diag11"]]
    o, n, r = U.arrays(cs)
    planes = np.hstack([o, n, r[:, None]])
    assert "K must lie in [0, 256]" in build(sh, m.x, m.cells, None, planes=np.tile(planes[:1], (257, 1)))[1]
    assert "K must lie" in build(sh, m.x, m.cells, None, planes=planes, K=-1)[1]
    assert build(sh, m.x, m.cells, None, planes=np.tile(planes[:1], (256, 1)))[0] == 0
    for j in range(planes.shape[1]):
        for v in (np.nan, np.inf, -np.inf):
            bad = planes.copy()
            bad[1, j] = v
            assert "entry %d of section 1 is not finite" % j in build(sh, m.x, m.cells, None, planes=bad)[1]
    bad = planes.copy()
    bad[0, 2:4] = 0.0
    assert "normal of section 0 is zero" in build(sh, m.x, m.cells, None, planes=bad)[1]
    rc, C = build(sh, m.x, m.cells, cs)
    assert "more than %d entries" % (C.total - 1) in build(sh, m.x, m.cells, cs, max_entries=C.total - 1)[1]
    assert build(sh, m.x, m.cells, cs, max_entries=C.total)[0] == 0
    cells = m.cells.copy()
    cells[5, 1] = m.nv
    assert "vertex out of range in cell 5" in build(sh, m.x, cells, cs)[1]
    ci = np.arange(m.nc, dtype=np.int32)
    ci[3] = ci[4]
    assert "no permutation" in build(sh, m.x, m.cells, cs, caller_index=ci)[1]
    x = m.x.copy()
    x[7, 1] = np.nan
    assert "non-finite coordinate of vertex 7" in build(sh, x, m.cells, cs)[1]
    # huge and tiny normals are normalised without overflow
    for f in (1e300, 1e-300):
        big = planes.copy()
        big[:, 2:4] *= f
        rc, B = build(sh, m.x, m.cells, None, planes=big)
        assert rc == 0 and np.array_equal(B.cell, C.cell) and np.allclose(B.normal, C.normal, rtol=0, atol=1e-15)


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("section_host_san") / "section_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "section_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", SU.ALL_MESHES)
def test_cut_under_sanitizers(sanitized, tmp_path, name):
    m = U.mesh(name)
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([m.d, m.nv, m.nc], np.int32).tobytes())
        f.write(np.ascontiguousarray(m.x, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(m.cells, dtype=np.int32).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------- sections.py
def test_plane_stations_and_derive(tmp_path):
    from cfd_hemodynamic_amd import sections as S
    pl = S.plane([1, 2, 3], [0, 0, 2], 0.5)
    assert np.array_equal(pl["origin"], [1, 2, 3]) and np.array_equal(pl["normal"], [0, 0, 2]) and pl["radius"] == 0.5
    for bad in (([0, 0], [0, 0]), ([0, 0], [1, 0, 0]), ([np.nan, 0], [1, 0])):
        with pytest.raises(ValueError):
            S.plane(*bad)
    with pytest.raises(ValueError):
        S.plane([0, 0], [1, 0], np.inf)
    st = S.stations([[0, 0], [2, 0], [2, 2]], 5, radius=0.25)
    assert np.allclose([s["origin"] for s in st], [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2]])
    assert np.allclose([s["normal"] for s in st], [[1, 0], [1, 0], [0, 1], [0, 1], [0, 1]]) and all(s["radius"] == 0.25 for s in st)
    assert np.allclose(S.stations([[0, 0, 0], [0, 0, 4]], 1)[0]["origin"], [0, 0, 2])
    with pytest.raises(ValueError):
        S.stations([[0, 0]], 3)
    o, n, r = S.as_arrays(st)
    assert o.shape == (5, 2) and n.shape == (5, 2) and r.shape == (5,)
    rows = np.zeros((3, 10))
    rows[0] = [2.0, 4.0, 20.0, 9.0, 10.0, 41.0, 1.5, 4.0, 0.2, 0.0]
    rows[1] = [1.0, 1.0, 8.0, 1.2, 1.3, 8.5, 0.5, 1.0, 0.0, 0.0]
    d = S.derive(rows, reference=0)
    assert np.allclose(d["mean_pressure"][:2], [10.0, 8.0]) and np.isnan(d["mean_pressure"][2])
    assert np.allclose(d["mean_normal_velocity"][:2], [2.0, 1.0]) and np.allclose(d["mean_velocity"][0], [2.0, 0.1, 0.0])
    assert np.isclose(d["momentum_factor"][0], 2.0 * 9.0 / 16.0) and np.isnan(d["momentum_factor"][2])
    assert np.allclose(d["energy_flux"], [42.5, 9.0, 0.0]) and np.allclose(d["flow_split"][:2], [1.0, 0.25])
    assert np.allclose(d["pressure_ratio"][:2], [1.0, 0.8]) and np.isnan(d["pressure_ratio"][2])
    series = np.stack([rows, 2 * rows])
    assert S.derive(series)["flow"].shape == (2, 3)
    S.write_npz(str(tmp_path / "s.npz"), t=[0.1, 0.2], rows=series, nothing=None)
    z = np.load(str(tmp_path / "s.npz"))
    assert set(z.files) == {"t", "rows"} and np.array_equal(z["rows"], series)
    S.write_txt(str(tmp_path / "s.txt"), [0.1, 0.2], series, np.zeros((3, 2)), np.ones((3, 2)), np.zeros(3), [0, 1, 0])
    text = open(str(tmp_path / "s.txt")).read()
    assert text.count("# section") == 3 and "straddling 1" in text and len(text.splitlines()) == 3 * 5


def test_command_line_planes():
    from cfd_hemodynamic_amd.__main__ import parse_sections
    pl = parse_sections("0,1.5;1,0 | 2,1,0;0,1,0;0.5")
    assert len(pl) == 2 and np.array_equal(pl[0]["origin"], [0, 1.5]) and pl[0]["radius"] == 0.0
    assert np.array_equal(pl[1]["normal"], [0, 1, 0]) and pl[1]["radius"] == 0.5
    for bad in ("", "0,1", "0,1;1,0;1;2", "0,1;0,0"):
        with pytest.raises(ValueError):
            parse_sections(bad)


# ------------------------------------------------------------------------------------------------------------ Python refusals
def test_solver_kinds_refuse_before_device_work():
    """SolverBase raises NotImplementedError, as for the sampler, on solvers without a context, on generic-element and
    pressure-correction contexts and on a part of a partitioned run -- before anything reaches the library."""
    from cfd_hemodynamic_amd import _lib
    from cfd_hemodynamic_amd.solverBase import SolverBase

    class Stub(SolverBase):
        def __init__(self, ctx=None, part=None):
            self.ctx, self._part = ctx, part

        def setup(self, bcu, bcp):
            pass

        def solveStep(self):
            pass

    class NoLibraryIpcs(_lib.IpcsContext):
        def __init__(self):
            self.h = None

        def close(self):
            pass

    stubs = [Stub(), Stub(types.SimpleNamespace(etype=1)), Stub(types.SimpleNamespace(etype=0), part=object()), Stub(NoLibraryIpcs())]
    for s in stubs:
        calls = ((s.section_set, ([U.SQUARE["x037"]],)), (s.section_cut, ()), (s.section_now, ()), (s.section_record, (0.1,)),
                 (s.section_series, ()), (s.section_mean_reset, ()), (s.section_mean_accumulate, (0.1,)), (s.section_mean, ()))
        for fn, a in calls:
            with pytest.raises(NotImplementedError, match="sections"):
                fn(*a)
    assert _lib.INFO_SECTION_COUNT == 120 and _lib.INFO_SECTION_KERNEL_NS == 125 and _lib.SECTION_NQ == 10
