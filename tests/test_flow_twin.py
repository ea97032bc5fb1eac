"""The volumetric flow diagnostics on the CPU: the NumPy twin (flow_twin.py) against the closed forms of flow_util.py, the inverted
index of csrc/cfdh_flow_host.hpp (compiled with g++ behind the extern "C" wrappers of flow_host_shim.cpp and loaded with ctypes --
no libcfdh.so, no GPU) against its definition, the same header once more in a stand-alone program built with AddressSanitizer and
UBSan (flow_host_main.cpp, a child process), the conditions the GPU tests rest on, and the recovery under refinement."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import flow_twin as T
import flow_util as U
from util import lid_case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
MESHES = ("square", "cube", "stenosis", "bifurcation")


def P(a):
    return a.ctypes.data_as(ip)


# ---------------------------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("mesh_name,case_name", U.affine_cases())
def test_twin_closed_forms(mesh_name, case_name):
    case = U.affine_case(mesh_name, case_name)
    assert U.check_affine(case, U.twin_result(case["m"], case["u"]))


def test_meshes_are_the_stated_ones():
    sizes = {n: (U.mesh(n).nv, U.mesh(n).nc) for n in MESHES + ("triangle", "tetrahedron")}
    assert sizes == {"square": (81, 128), "cube": (125, 384), "stenosis": (343, 576), "bifurcation": (1681, 6288), "triangle": (3, 1),
                     "tetrahedron": (4, 1)}
    val = {n: np.diff(T.vertex_cells(U.mesh(n).nv, U.mesh(n).cells)[0]) for n in MESHES}
    assert val["square"].min() == 1 and (val["cube"].min(), val["cube"].max()) == (2, 24)
    assert (val["stenosis"].min(), val["stenosis"].max()) == (1, 8) and (val["bifurcation"].min(), val["bifurcation"].max()) == (2, 24)
    m = U.mesh("stenosis")
    vol = T.cell_gradients(m.x, m.cells, np.zeros((m.nv, 2)))[0]
    assert 6.0 < vol.max() / vol.min() < 7.0  # cell areas spread 6.5 x


@pytest.mark.parametrize("name", ["cube", "bifurcation"])
def test_lnh_condition_of_the_gpu_test(name):
    """At most 1 % of the vertices may have |u||omega| below 1e-6 of its maximum on the fields of the device-against-twin test."""
    tw = U.twin_case(name)["twin"]
    w = tw["lnh_weight"]
    print("%s: smallest |u||omega| / max = %.2e, left out %d of %d" % (name, w.min() / w.max(), (~U.lnh_mask(tw)).sum(), len(w)))
    assert (~U.lnh_mask(tw)).mean() <= U.LNH_MAX_EXCLUDED
    assert (np.abs(tw["lnh"]) <= 1.0 + 1e-15).all()


def test_lnh_is_zero_where_a_norm_is():
    m = U.mesh("cube")
    u = U.random_field("cube").copy()
    u[[0, 64]] = 0.0
    lnh = T.fields(m.x, m.cells, u, U.MU)["lnh"]
    assert (lnh[[0, 64]] == 0.0).all() and (lnh[1:64] != 0.0).all()
    assert (T.fields(m.x, m.cells, np.ones((m.nv, 3)), U.MU)["lnh"] == 0.0).all()


def test_window_twin():
    m = U.mesh("stenosis")
    ua, ub = U.window_fields("stenosis")
    win = T.Window(m.x, m.cells, U.MU)
    win.accumulate(ua, 0.3)
    win.accumulate(ub, 0.7)
    got = win.get()
    assert (win.W, win.count) == (1.0, 2)
    fa, fb = T.fields(m.x, m.cells, ua, U.MU), T.fields(m.x, m.cells, ub, U.MU)
    assert np.allclose(got["mean_shear_rate"], 0.3 * fa["shear_rate"] + 0.7 * fb["shear_rate"], rtol=1e-14)
    assert np.array_equal(got["peak_shear_rate"], np.maximum(fa["shear_rate"], fb["shear_rate"]))
    assert np.allclose(got["fluctuation"], 0.5 * 0.21 * ((ua - ub) ** 2).sum(axis=1), rtol=1e-12)  # two states: w_a w_b |u_a - u_b|^2 / 2
    win.reset()
    assert win.W == 0.0 and not win.sU.any() and not win.sMax.any()


# ------------------------------------------------------------------------------------------------------ the inverted index
@pytest.fixture(scope="module")
def fh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("flow_host") / "flow_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "flow_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int = ctypes.c_int
    L.fh_build.argtypes = [c_int, c_int, c_int, ip, ip, ip, ctypes.c_char_p, c_int]
    L.fh_get.argtypes = [ip, ip, ip, ip]
    L.fh_field_width.argtypes = [c_int, c_int]
    return L


def build(fh, m, visit=None, cells=None, nv=None):
    cells = m.cells if cells is None else cells
    nv = m.nv if nv is None else nv
    sizes = np.zeros(4, dtype=np.int32)
    msg = ctypes.create_string_buffer(256)
    rc = fh.fh_build(m.d, nv, len(cells), P(cells), None if visit is None else P(visit), P(sizes), msg, 256)
    if rc != 0:
        return rc, msg.value.decode()
    ninc, nslices, maxlen, ncol = (int(v) for v in sizes)
    out = types.SimpleNamespace(ninc=ninc, nslices=nslices, maxlen=maxlen, rptr=np.zeros(nv + 1, dtype=np.int32), inc=np.zeros(ninc, dtype=np.int32),
                                sptr=np.zeros(nslices + 1, dtype=np.int32), dinc=np.zeros(ncol * 64, dtype=np.int32))
    fh.fh_get(P(out.rptr), P(out.inc), P(out.sptr), P(out.dinc))
    return 0, out


@pytest.mark.parametrize("name", MESHES + ("triangle", "tetrahedron"))
def test_inverted_index(fh, name):
    """Every incidence exactly once, ascending per vertex; the slice layout equals the by-row layout."""
    m = U.mesh(name)
    rc, w = build(fh, m)
    assert rc == 0, w
    assert fh.fh_slice() == T.SLICE == 64
    rptr, inc = T.vertex_cells(m.nv, m.cells)
    assert w.ninc == m.nc * (m.d + 1) and np.array_equal(w.rptr, rptr) and np.array_equal(w.inc, inc)
    # the definition, without the twin: the pairs (vertex, cell) are those of `cells`, once each, sorted
    vert = np.repeat(np.arange(m.nv), np.diff(w.rptr))
    pairs = np.stack([vert, w.inc], axis=1)
    want = np.stack([m.cells.ravel(), np.repeat(np.arange(m.nc), m.d + 1)], axis=1)
    assert np.array_equal(pairs, want[np.lexsort((want[:, 1], want[:, 0]))])
    assert w.maxlen == np.diff(rptr).max()
    sptr, dinc = T.sliced(m.nv, rptr, inc)
    assert w.nslices == (m.nv + 63) // 64 and np.array_equal(w.sptr, sptr) and np.array_equal(w.dinc, dinc)
    assert (w.dinc >= 0).sum() == w.ninc and len(w.dinc) == w.sptr[-1] * 64  # the last slice is allocated in full


def test_inverted_index_in_a_visiting_order(fh):
    """The context keeps its cells in another order than the caller: with visit[k] = the stored cell the caller numbered k, the
    cells of a vertex come in ascending caller's index."""
    m = U.mesh("stenosis")
    rng = np.random.default_rng(3)
    user_of = rng.permutation(m.nc).astype(np.int32)     # stored cell e is the caller's cell user_of[e]
    stored = np.ascontiguousarray(m.cells[user_of])      # the stored list
    visit = np.argsort(user_of).astype(np.int32)
    rc, w = build(fh, m, visit=visit, cells=stored)
    assert rc == 0, w
    rptr, inc = T.vertex_cells(m.nv, m.cells)
    assert np.array_equal(w.rptr, rptr) and np.array_equal(user_of[w.inc], inc)


def test_index_refusals_and_widths(fh):
    m = U.mesh("square")
    bad = m.cells.copy()
    bad[5, 1] = m.nv
    assert "vertex out of range in cell 5" in build(fh, m, cells=bad)[1]
    twice = m.cells.copy()
    twice[7, 2] = twice[7, 0]
    assert "names a vertex twice" in build(fh, m, cells=twice)[1]
    visit = np.arange(m.nc, dtype=np.int32)
    visit[3] = visit[4]
    assert "no permutation" in build(fh, m, visit=visit)[1]
    assert [fh.fh_field_width(2, w) for w in range(-1, 8)] == [0, 4, 1, 1, 1, 1, 0, 0, 0]
    assert [fh.fh_field_width(3, w) for w in range(-1, 8)] == [0, 9, 3, 1, 1, 1, 1, 1, 0]


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("flow_host_san") / "flow_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "flow_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", MESHES)
def test_index_under_sanitizers(sanitized, tmp_path, name):
    m = U.mesh(name)
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([m.d, m.nv, m.nc], np.int32).tobytes())
        f.write(np.ascontiguousarray(m.cells, dtype=np.int32).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok %d incidences" % (m.nc * (m.d + 1))), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------------ refinement
def test_recovered_vorticity_improves_under_refinement():
    """u = (sin pi y, 0), omega = -pi cos pi y: the largest error of the recovered vorticity over the vertices on no boundary facet
    is smaller on lid_case(16) than on lid_case(8).  (The observed ratio is in DESIGN.md section 9; it is not asserted.)"""
    err = []
    for n in (8, 16):
        mesh = lid_case(n).mesh
        x = np.asarray(mesh.x, dtype=float)[:, :2]
        cells = np.ascontiguousarray(mesh.cells, dtype=np.int32)
        u = np.stack([np.sin(np.pi * x[:, 1]), np.zeros(len(x))], axis=1)
        w = T.fields(x, cells, u, U.MU)["vorticity"]
        inner = (x > 1e-12).all(axis=1) & (x < 1 - 1e-12).all(axis=1)
        assert inner.sum() == (n - 1) ** 2
        err.append(np.abs(w + np.pi * np.cos(np.pi * x[:, 1]))[inner].max())
    print("largest interior vorticity error: n = 8 %.4e, n = 16 %.4e, ratio %.2f" % (err[0], err[1], err[0] / err[1]))
    assert err[1] < err[0]


# ------------------------------------------------------------------------------------------------------------ Python refusals
def test_solver_kinds_refuse_before_device_work():
    """SolverBase raises NotImplementedError, as for transport and particles, on solvers without a context, on generic-element and
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
        for fn, a in ((s.flow_field, ("vorticity",)), (s.flow_integrals, ()), (s.flow_stats_reset, ()), (s.flow_stats_accumulate, (0.1,)),
                      (s.flow_stats, ())):
            with pytest.raises(NotImplementedError, match="flow diagnostics"):
                fn(*a)
