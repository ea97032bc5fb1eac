"""The host tables of the particle tracker (csrc/cfdh_particles_host.hpp) on the CPU: the header is compiled with g++ behind the
extern "C" wrappers of particles_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU.  The neighbour table is checked
against its definition in NumPy (every interior facet paired symmetrically, every exterior facet mapped to its index in the facet
list), the affine table against the twin's.  The same steps run once more in a stand-alone program built with AddressSanitizer
and UBSan (particles_host_main.cpp), as a child process."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import particles_twin as T
from cfd_hemodynamic_amd.mesh3d import create_bifurcation, create_unit_cube
from util import dfg_case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
dp = ctypes.POINTER(ctypes.c_double)


def _plain(m):
    d = m.cells.shape[1] - 1
    return types.SimpleNamespace(D=d, x=np.ascontiguousarray(np.asarray(m.x, dtype=np.float64)[:, :d]), cells=np.ascontiguousarray(m.cells, dtype=np.int32),
                                 fcell=np.ascontiguousarray(m.facet_cells, dtype=np.int32), flocal=np.ascontiguousarray(m.facet_local, dtype=np.int32))


MESHES = {"dfg6": _plain(dfg_case(6).mesh), "cube4": _plain(create_unit_cube(4)), "bifurcation": _plain(create_bifurcation(1.2e-3)[0])}
NAMES = sorted(MESHES)


def P(a):
    return a.ctypes.data_as(dp if a.dtype == np.float64 else ip)


@pytest.fixture(scope="module")
def ph(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("particles_host") / "particles_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "particles_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int, msg = ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]
    L.ph_neighbours.argtypes = [c_int, c_int, c_int, ip, c_int, ip, ip, ip] + msg
    L.ph_affine.argtypes = [c_int, c_int, ip, dp, dp] + msg
    L.ph_barycentric.argtypes = [c_int, dp, dp, dp]
    L.ph_check_seeds.argtypes = [c_int, ctypes.c_longlong, dp, ip, ctypes.c_longlong, ip, dp, ctypes.c_double, ip] + msg
    L.ph_constants.argtypes = [dp, dp]
    return L


def neighbours(ph, s, nfac=None, fcell=None, flocal=None):
    nb = np.zeros((len(s.cells), s.D + 1), dtype=np.int32)
    msg = ctypes.create_string_buffer(256)
    fcell, flocal = s.fcell if fcell is None else fcell, s.flocal if flocal is None else flocal
    rc = ph.ph_neighbours(s.D, len(s.x), len(s.cells), P(s.cells), len(fcell) if nfac is None else nfac, P(fcell), P(flocal), P(nb), msg, 256)
    return rc, nb, msg.value.decode()


def affine(ph, s, x=None):
    aff = np.zeros((len(s.cells), s.D * s.D + s.D))
    msg = ctypes.create_string_buffer(256)
    rc = ph.ph_affine(s.D, len(s.cells), P(s.cells), P(s.x if x is None else x), P(aff), msg, 256)
    return rc, aff, msg.value.decode()


@pytest.mark.parametrize("name", NAMES)
def test_neighbour_table(ph, name):
    s = MESHES[name]
    rc, nb, why = neighbours(ph, s)
    assert rc == 0, why
    n1 = s.D + 1
    # interior facets: the neighbour lists the cell back exactly once, across the facet with the same vertices
    e, f = np.nonzero(nb >= 0)
    o = nb[e, f]
    back = nb[o] == e[:, None]
    assert (back.sum(axis=1) == 1).all()
    g = back.argmax(axis=1)
    mine = np.sort(np.stack([np.delete(s.cells[c], a) for c, a in zip(e, f)]), axis=1)
    theirs = np.sort(np.stack([np.delete(s.cells[c], a) for c, a in zip(o, g)]), axis=1)
    assert np.array_equal(mine, theirs) and (o != e).all()
    # exterior facets: -1 - k with k the facet's index in the list, every facet of the list exactly once
    ee, ff = np.nonzero(nb < 0)
    k = -1 - nb[ee, ff]
    assert np.array_equal(np.sort(k), np.arange(len(s.fcell)))
    assert np.array_equal(s.fcell[k], ee) and np.array_equal(s.flocal[k], ff)
    # every facet of the mesh is one or the other: (d + 1) nc = 2 interior + exterior
    assert n1 * len(s.cells) == len(e) + len(s.fcell)
    assert np.array_equal(nb, T.neighbours(s.cells, s.fcell, s.flocal))


@pytest.mark.parametrize("name", NAMES)
def test_affine_table_and_seed_checks(ph, name):
    s = MESHES[name]
    rc, aff, why = affine(ph, s)
    assert rc == 0, why
    want = T.affine(s.x, s.cells)
    assert np.abs(aff - want).max() <= 1e-13 * np.abs(want).max()
    X = s.x[s.cells]
    lam = np.zeros(s.D + 1)
    for e in (0, len(s.cells) // 2, len(s.cells) - 1):
        for b in range(s.D + 1):
            ph.ph_barycentric(s.D, P(np.ascontiguousarray(aff[e])), P(np.ascontiguousarray(X[e, b])), P(lam))
            assert np.abs(lam - np.eye(s.D + 1)[b]).max() <= 1e-12
    # seeds: the caller's numbering goes through cell_int; a point 1e-10 outside its cell passes, one 1e-8 outside does not
    nc = len(s.cells)
    rng = np.random.default_rng(2)
    cell_int = rng.permutation(nc).astype(np.int32)
    aff_int = np.zeros_like(aff)
    aff_int[cell_int] = aff
    cells = rng.integers(0, nc, 50).astype(np.int32)
    cen = X[cells].mean(axis=1)

    def check(x, c, t=0.0):
        ci = np.zeros(len(c), dtype=np.int32)
        msg = ctypes.create_string_buffer(256)
        rc = ph.ph_check_seeds(s.D, len(c), P(np.ascontiguousarray(x)), P(c), nc, P(cell_int), P(aff_int), t, P(ci), msg, 256)
        return rc, ci, msg.value.decode()

    rc, ci, why = check(cen, cells)
    assert rc == 0 and np.array_equal(ci, cell_int[cells]), why
    for eps, ok in ((1e-10, True), (1e-8, False)):
        lam = np.full((50, s.D + 1), (1.0 + eps) / s.D)
        lam[:, 0] = -eps
        rc, _, why = check(np.einsum("ka,kai->ki", lam, X[cells]), cells)
        assert (rc == 0) == ok, why
    assert check(cen, np.roll(cells, 1))[0] == -1 or np.array_equal(np.roll(cells, 1), cells)
    assert check(cen, cells, np.nan)[2] == "t_birth is not finite"
    bad = cen.copy()
    bad[3, 0] = np.inf
    assert check(bad, cells)[2] == "position 3 is not finite"
    out = cells.copy()
    out[5] = nc
    assert check(cen, out)[0] == -1


def test_refusals(ph):
    s = MESHES["dfg6"]
    assert neighbours(ph, s, nfac=len(s.fcell) - 1)[0] == -1                     # an exterior facet missing from the list
    e, f = np.nonzero(T.neighbours(s.cells, s.fcell, s.flocal) >= 0)
    fc, fl = s.fcell.copy(), s.flocal.copy()
    fc[0], fl[0] = e[0], f[0]
    assert "interior or listed twice" in neighbours(ph, s, fcell=fc, flocal=fl)[2]  # an interior facet in the list
    dup = types.SimpleNamespace(D=s.D, x=s.x, cells=np.ascontiguousarray(np.vstack([s.cells, s.cells[:1]])), fcell=s.fcell, flocal=s.flocal)
    assert "more than two cells" in neighbours(ph, dup)[2] or neighbours(ph, dup)[0] == -1
    flat = s.x.copy()
    flat[s.cells[7]] = flat[s.cells[7, 0]]
    F = flat[s.cells]
    r1, r2 = F[:, 1] - F[:, 0], F[:, 2] - F[:, 0]
    first = int(np.nonzero(r1[:, 0] * r2[:, 1] - r1[:, 1] * r2[:, 0] == 0.0)[0][0])  # cell 7, or a lower one that shares two of its vertices
    assert first <= 7 and affine(ph, s, x=flat)[2] == "particle tables: cell %d has no volume" % first
    a, b = ctypes.c_double(), ctypes.c_double()
    assert ph.ph_constants(ctypes.byref(a), ctypes.byref(b)) == T.MAX_CROSSINGS and (a.value, b.value) == (T.TOL_INSIDE, T.TOL_SEED)


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("particles_host_san") / "particles_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "particles_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", NAMES)
def test_tables_under_sanitizers(sanitized, tmp_path, name):
    s = MESHES[name]
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([s.D, len(s.x), len(s.cells), len(s.fcell)], np.int32).tobytes())
        for a in (s.cells, s.fcell, s.flocal):
            f.write(np.ascontiguousarray(a, dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(s.x, dtype=np.float64).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
