"""The point sampler on the CPU: the brute-force NumPy twin (sample_twin.py) against connectivity and closed forms, the conditions
the GPU tests rest on (the ambiguity cap of the grids, the points outside the domain), the bin grid of csrc/cfdh_sample_host.hpp
(compiled with g++ behind the extern "C" wrappers of sample_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU) against
its definition, the same header once more in a stand-alone program built with AddressSanitizer and UBSan (sample_host_main.cpp, a
child process), the helpers of cfd_hemodynamic_amd/sampling.py and the Python refusals."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import sample_twin as T
import sample_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
dp = ctypes.POINTER(ctypes.c_double)
lp = ctypes.POINTER(ctypes.c_longlong)


# --------------------------------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_twin_against_connectivity(name):
    """Seeds in known cells, every vertex and every interior facet midpoint: the expected cell comes from `cells`."""
    m = U.mesh(name)
    for what, (pts, want) in (("seeds", U.seeds(m, 257)), ("vertices", U.vertex_points(m)), ("facets", U.facet_points(m))):
        cell, lam, amb, count = T.locate(m.x, m.cells, pts, U.TOL)
        assert np.array_equal(cell, want), what
        assert not amb.any()
        if len(pts):
            assert U.worst(what + " sum", lam.sum(axis=1), 1.0, U.TOL_EXACT)
            assert U.worst(what + " lam.X", np.einsum("na,nai->ni", lam, m.x[m.cells[cell]]), pts, U.TOL_EXACT * m.size)
        if what == "facets" and len(pts):
            assert (count == 2).all()
    if name == "cube":
        assert T.locate(m.x, m.cells, m.x, U.TOL)[3].max() == 24  # the valence of the centre vertices


@pytest.mark.parametrize("name", U.MESHES)
def test_twin_outside(name):
    m = U.mesh(name)
    assert (T.locate(m.x, m.cells, U.outside_box(m), U.TOL)[0] == -1).all()
    if name in ("stenosis", "bifurcation"):
        pts = U.outside_domain(name)
        lo, hi = m.x.min(axis=0), m.x.max(axis=0)
        print("%s: %d points inside the box, outside the domain" % (name, len(pts)))
        assert len(pts) >= 100 and (pts >= lo).all() and (pts <= hi).all()
        assert (T.locate(m.x, m.cells, pts, U.TOL)[0] == -1).all()


@pytest.mark.parametrize("name", U.MESHES)
def test_grid_ambiguity_cap(name):
    """The grid of the GPU test: at most 1 % of its nodes may have a cell with min lambda in (-10 tol, -tol / 10) (they are left out
    there); the stenosis and the bifurcation locate at least 500 nodes."""
    m = U.mesh(name)
    origin, spacing, dims = U.margin_grid(m, U.GRID_N[name])
    pts = U.grid_points(m, origin, spacing, dims)
    cell, lam, amb, count = U.twin_location(name, "grid", pts)
    print("%s: located %d / %d nodes, exact ties %d, left out %d" % (name, (cell >= 0).sum(), len(pts), (count > 1).sum(), amb.sum()))
    assert amb.mean() <= U.MAX_AMBIGUOUS
    assert len(pts) == dims.prod() and (cell < 0).any()
    if name == "square":
        assert (len(pts), int((cell >= 0).sum()), int((count > 1).sum())) == (625, 484, 22)
    elif name == "cube":
        assert (len(pts), int((cell >= 0).sum()), int((count > 1).sum())) == (2197, 1000, 280)
    else:
        assert (cell >= 0).sum() >= 500


@pytest.mark.parametrize("name", ["square", "bifurcation"])
def test_twin_does_not_depend_on_the_numbering(name):
    """Cells in another order and with other local vertex orders: the same cells under the renumbering, the same samples."""
    m, q = U.mesh(name), U.permuted(name)
    pts = np.vstack([U.seeds(m, 65)[0], m.x[::7], U.facet_points(m)[0][::11]])
    cell, lam = T.locate(m.x, m.cells, pts, U.TOL)[:2]
    holders = T.containing(m.x, m.cells, pts, U.TOL)
    want = np.array([q.new_of_old[h].min() for h in holders], dtype=np.int32)
    cell_q, lam_q = T.locate(q.x, q.cells, pts, U.TOL)[:2]
    assert np.array_equal(cell_q, want)
    u, p, exact = U.affine_state(m)
    assert U.worst("affine, permuted", T.rows(q, cell_q, lam_q, u, p), exact(pts), U.TOL_EXACT * np.abs(exact(pts)).max())


@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_twin_samples_affine_fields_exactly(name):
    m = U.mesh(name)
    pts = np.vstack([U.seeds(m, 63)[0], m.x, U.outside_box(m)])
    cell, lam = T.locate(m.x, m.cells, pts, U.TOL)[:2]
    u, p, exact = U.affine_state(m)
    got = T.rows(m, cell, lam, u, p)
    inside = cell >= 0
    assert inside.sum() == 63 + m.nv and (got[~inside] == 0.0).all()
    assert U.worst("affine", got[inside], exact(pts[inside]), U.TOL_EXACT * np.abs(exact(pts[inside])).max())


# ----------------------------------------------------------------------------------------------------------------- the bin grid
@pytest.fixture(scope="module")
def sh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sample_host") / "sample_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "sample_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int = ctypes.c_int
    L.sh_build.argtypes = [c_int, c_int, c_int, dp, ip, ip, ctypes.c_double, lp, dp, ctypes.c_char_p, c_int]
    L.sh_get.argtypes = [ip, ip]
    L.sh_point_bins.argtypes = [ctypes.c_longlong, dp, lp]
    return L


def build(sh, m, tol=U.TOL, visit=None, cells=None):
    cells = np.ascontiguousarray(m.cells if cells is None else cells, dtype=np.int32)
    x = np.ascontiguousarray(m.x, dtype=np.float64)
    sizes, lengths = np.zeros(7, dtype=np.int64), np.zeros(8)
    msg = ctypes.create_string_buffer(256)
    rc = sh.sh_build(m.d, m.nv, len(cells), x.ctypes.data_as(dp), cells.ctypes.data_as(ip), None if visit is None else visit.ctypes.data_as(ip),
                     tol, sizes.ctypes.data_as(lp), lengths.ctypes.data_as(dp), msg, 256)
    if rc != 0:
        return rc, msg.value.decode()
    B = types.SimpleNamespace(nbins=int(sizes[0]), total=int(sizes[1]), maxlen=int(sizes[2]), doublings=int(sizes[3]), nb=sizes[4:7].copy(),
                              edge=lengths[0], first_edge=lengths[1], lo=lengths[2:5].copy(), hi=lengths[5:8].copy(),
                              ptr=np.zeros(int(sizes[0]) + 1, dtype=np.int32), list=np.zeros(int(sizes[1]), dtype=np.int32))
    sh.sh_get(B.ptr.ctypes.data_as(ip), B.list.ctypes.data_as(ip))
    return 0, B


def bins_of(sh, pts):
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.zeros(len(pts), dtype=np.int64)
    sh.sh_point_bins(len(pts), pts.ctypes.data_as(dp), out.ctypes.data_as(lp))
    return out


def every_test_point(name):
    """The points of the GPU location tests on this mesh."""
    m = U.mesh(name)
    sets = [U.seeds(m, 1000)[0], m.x, U.facet_points(m)[0], U.outside_box(m)]
    if name in U.GRID_N:
        sets.append(U.grid_points(m, *U.margin_grid(m, U.GRID_N[name])))
    if name in ("stenosis", "bifurcation"):
        sets.append(U.outside_domain(name))
    return np.vstack(sets)


@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_bins(sh, name):
    """Shape: ascending lists without duplicates, at most 16 nc entries, the reported longest list.  Completeness: the list of
    every test point's bin holds every cell that contains the point under tol (the twin names them)."""
    m = U.mesh(name)
    rc, B = build(sh, m)
    assert rc == 0, B
    assert B.nbins == B.nb.prod() and B.ptr[0] == 0 and B.ptr[-1] == B.total == len(B.list)
    assert B.total <= 16 * m.nc and B.maxlen == np.diff(B.ptr).max() and (np.diff(B.ptr) >= 0).all()
    assert B.edge == B.first_edge * 2.0 ** B.doublings
    box = np.sort(m.x[m.cells], axis=1)
    assert B.first_edge == np.sort((box[:, -1] - box[:, 0]).max(axis=1))[m.nc // 2]  # the median of the cells' longest box edges
    print("%s: edge %.4g (%d doublings), %d bins, %d entries = %.2f nc, longest list %d" % (name, B.edge, B.doublings, B.nbins, B.total, B.total / m.nc, B.maxlen))
    for b in range(B.nbins):
        assert (np.diff(B.list[B.ptr[b]:B.ptr[b + 1]]) > 0).all()
    assert np.array_equal(np.unique(B.list), np.arange(m.nc))
    pts = every_test_point(name)
    bins = bins_of(sh, pts)
    holders = T.containing(m.x, m.cells, pts, U.TOL)
    checked = 0
    for b, h in zip(bins, holders):
        if len(h):
            assert b >= 0 and np.isin(h, B.list[B.ptr[b]:B.ptr[b + 1]]).all()
            checked += len(h)
    assert checked > len(pts) // 4
    outside = (pts[:, :m.d] < B.lo[:m.d]).any(axis=1) | (pts[:, :m.d] > B.hi[:m.d]).any(axis=1)
    assert np.array_equal(bins < 0, outside) and outside.any()


def test_bins_at_the_largest_tolerance(sh):
    """tol = 1e-3: points as far outside their cell as the definition admits (1 + d tol on one vertex, -tol on the others) are in a
    bin that lists the cell."""
    for name in ("stenosis", "cube"):
        m = U.mesh(name)
        rc, B = build(sh, m, tol=1e-3)
        assert rc == 0, B
        for a in range(m.d + 1):
            lam = np.full(m.d + 1, -1e-3)
            lam[a] = 1.0 + m.d * 1e-3
            pts = np.einsum("a,cai->ci", lam, m.x[m.cells])
            bins = bins_of(sh, pts)
            assert (bins >= 0).all()
            assert all(c in B.list[B.ptr[b]:B.ptr[b + 1]] for c, b in enumerate(bins))


def test_bins_in_a_visiting_order(sh):
    """The context keeps its cells in another order than the caller: the lists are ascending in the caller's index."""
    m = U.mesh("stenosis")
    rng = np.random.default_rng(3)
    user_of = rng.permutation(m.nc).astype(np.int32)     # stored cell e is the caller's cell user_of[e]
    stored = np.ascontiguousarray(m.cells[user_of])
    visit = np.argsort(user_of).astype(np.int32)
    rc, B = build(sh, m, visit=visit, cells=stored)
    assert rc == 0, B
    rc, ref = build(sh, m)
    assert np.array_equal(B.ptr, ref.ptr) and np.array_equal(user_of[B.list], ref.list)


def test_bins_degenerate_cases_and_refusals(sh):
    for name in ("triangle", "tetrahedron"):  # one cell
        m = U.mesh(name)
        rc, B = build(sh, m)
        assert rc == 0 and (B.list == 0).all() and B.total <= 16 and B.maxlen == 1
        corner = B.hi[:m.d].copy()
        assert bins_of(sh, corner[None])[0] == B.nbins - 1  # a point exactly on the upper corner of the box: the last bin
        assert bins_of(sh, B.lo[None, :m.d])[0] == 0
        assert bins_of(sh, np.nextafter(corner, np.inf)[None])[0] == -1
        assert bins_of(sh, np.full((1, m.d), np.nan))[0] == -1
    m = U.mesh("square")
    bad = m.cells.copy()
    bad[5, 1] = m.nv
    assert "vertex out of range in cell 5" in build(sh, m, cells=bad)[1]
    visit = np.arange(m.nc, dtype=np.int32)
    visit[3] = visit[4]
    assert "no permutation" in build(sh, m, visit=visit)[1]
    for tol in (-1e-12, 1.1e-3, np.nan, np.inf):
        assert "tol" in build(sh, m, tol=tol)[1]


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sample_host_san") / "sample_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "sample_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", U.ALL_MESHES)
def test_bins_under_sanitizers(sanitized, tmp_path, name):
    m = U.mesh(name)
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([m.d, m.nv, m.nc], np.int32).tobytes())
        f.write(np.ascontiguousarray(m.x, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(m.cells, dtype=np.int32).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------- sampling.py
def test_line_and_grid_over():
    from cfd_hemodynamic_amd import sampling as S
    pts = S.line([0.0, 1.0], [2.0, 1.0], 5)
    assert pts.shape == (5, 2) and np.array_equal(pts[:, 0], [0.0, 0.5, 1.0, 1.5, 2.0]) and (pts[:, 1] == 1.0).all()
    assert np.array_equal(S.line([1.0, 2.0, 3.0], [4.0, 5.0, 6.0], 1), [[1.0, 2.0, 3.0]])
    with pytest.raises(ValueError):
        S.line([0.0, 0.0], [1.0, 1.0, 1.0], 3)
    m = U.mesh("stenosis")
    lo, hi = m.x.min(axis=0), m.x.max(axis=0)
    origin, spacing, dims = S.grid_over(m, 0.5, pad=0.25)
    assert origin.shape == spacing.shape == dims.shape == (3,) and dims[2] == 1 and origin[2] == 0.0
    assert np.array_equal(origin[:2], lo - 0.25) and (spacing[:2] == 0.5).all()
    last = origin[:2] + (dims[:2] - 1) * 0.5
    assert (last >= hi + 0.25 - 1e-9).all() and (last < hi + 0.25 + 0.5).all()
    origin, spacing, dims = S.grid_over(U.mesh("cube"), dims=(5, 3, 2))
    assert np.array_equal(dims, [5, 3, 2]) and np.allclose(origin + (dims - 1) * spacing, 1.0)
    with pytest.raises(ValueError):
        S.grid_over(m, spacing=0.5, dims=4)
    with pytest.raises(ValueError):
        S.grid_over(m, spacing=-1.0)


def test_vti_round_trip(tmp_path):
    from cfd_hemodynamic_amd import sampling as S
    rng = np.random.default_rng(1)
    dims = (4, 3, 2)
    u, p, mask = rng.uniform(-1, 1, (24, 3)), rng.uniform(-1, 1, 24), rng.uniform(0, 1, 24) > 0.5
    path = str(tmp_path / "a.vti")
    S.write_vti(path, (0.5, -1.0, 2.0), (0.1, 0.2, 0.3), dims, {"velocity": u, "pressure": p}, located=mask)
    z = S.read_vti(path)
    assert np.array_equal(z["dims"], dims) and np.array_equal(z["origin"], [0.5, -1.0, 2.0]) and np.array_equal(z["spacing"], [0.1, 0.2, 0.3])
    assert np.array_equal(z["velocity"], u) and np.array_equal(z["pressure"], p) and np.array_equal(z["located"], mask.astype(np.uint8))
    head = open(path, "rb").read(400).decode(errors="replace")
    assert 'type="ImageData"' in head and 'WholeExtent="0 3 0 2 0 1"' in head
    u2 = rng.uniform(-1, 1, (12, 2))  # 2-D vectors are padded to three components
    S.write_vti(path, (0, 0, 0), (1, 1, 1), (4, 3, 1), {"velocity": u2})
    z = S.read_vti(path)
    assert z["velocity"].shape == (12, 3) and np.array_equal(z["velocity"][:, :2], u2) and (z["velocity"][:, 2] == 0).all()
    S.write_npz(str(tmp_path / "b.npz"), t=[0.1, 0.2], x=u2)
    assert np.array_equal(np.load(str(tmp_path / "b.npz"))["t"], [0.1, 0.2])


# ------------------------------------------------------------------------------------------------------------ Python refusals
def test_solver_kinds_refuse_before_device_work():
    """SolverBase raises NotImplementedError, as for the flow diagnostics, on solvers without a context, on generic-element and
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
        calls = ((s.sample_set_points, (np.zeros((1, 2)),)), (s.sample_set_grid, ((0, 0, 0), (1, 1, 1), (2, 2, 1))), (s.sample_location, ()),
                 (s.sample_now, ()), (s.sample_record, (0.1,)), (s.sample_series, ()), (s.sample_mean_reset, ()),
                 (s.sample_mean_accumulate, (0.1,)), (s.sample_mean, ()))
        for fn, a in calls:
            with pytest.raises(NotImplementedError, match="sampling"):
                fn(*a)
    assert _lib.INFO_SAMPLE_POINTS == 111 and _lib.INFO_SAMPLE_KERNEL_NS == 116
