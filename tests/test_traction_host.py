"""The work list of the traction kernel (csrc/cfdh_traction_host.hpp) on the CPU: the header is compiled with g++ behind the
extern "C" wrappers of traction_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU.  Expected values come from a numpy
construction of the definition, not from a second copy of the loops.  The same builder runs once more in a stand-alone program
built with AddressSanitizer and UBSan (traction_host_main.cpp), as a child process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
import trac_util as U

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def th(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("traction_host") / "traction_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "traction_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int, msg = ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]
    L.th_build.argtypes = [c_int, c_int, c_int, ip, c_int, ip, ip, ip, c_int, ip, ctypes.c_uint, ip, ip, ip] + msg
    L.th_get.argtypes = [ip] * 9
    L.th_check.argtypes = [c_int, c_int, ip, dp, ctypes.c_double, dp] + msg
    return L


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def P(a):
    return a.ctypes.data_as(dp if a.dtype == np.float64 else ip)


def graph(mesh):
    """Vertex graph: row v lists the vertices that share a cell with v (v included), ascending."""
    nv, n1 = mesh.num_vertices, mesh.cells.shape[1]
    adj = [set() for _ in range(nv)]
    for c in mesh.cells:
        for a in c:
            adj[a].update(int(b) for b in c)
    vptr = np.zeros(nv + 1, dtype=np.int32)
    vptr[1:] = np.cumsum([len(s) for s in adj])
    return vptr, i32(np.concatenate([sorted(s) for s in adj]))


def expected(mesh, marker, markers, tangential, vptr, vcol):
    """{row: [(cell, a, f, k, slots)]}: for every exterior facet, in order, that lies on boundary k, one pair for each vertex of its
    cell -- the vertex opposite the facet only when the boundary carries the tangential terms."""
    n1 = mesh.cells.shape[1]
    rows = {}
    for q in range(len(marker)):
        if marker[q] not in markers:
            continue
        k = markers.index(marker[q])
        e, f = int(mesh.facet_cells[q]), int(mesh.facet_local[q])
        for a in range(n1):
            if a == f and not tangential[k]:
                continue
            v = int(mesh.cells[e, a])
            cols = vcol[vptr[v]:vptr[v + 1]]
            slots = [int(vptr[v] + np.nonzero(cols == w)[0][0]) for w in mesh.cells[e]]
            rows.setdefault(v, []).append((e, a, f, k, slots))
    return rows


def build(th, mesh, marker, markers, tangential, vptr=None, vcol=None):
    D, n1 = mesh.x.shape[1], mesh.cells.shape[1]
    if vptr is None:
        vptr, vcol = graph(mesh)
    sizes, msg = np.zeros(4, dtype=np.int32), ctypes.create_string_buffer(256)
    mk = i32(markers) if len(markers) else np.zeros(1, dtype=np.int32)
    tang = sum(1 << k for k, t in enumerate(tangential) if t)
    rc = th.th_build(D, mesh.num_vertices, len(mesh.cells), P(i32(mesh.cells)), len(marker), P(i32(mesh.facet_cells)), P(i32(mesh.facet_local)),
                     P(i32(marker)), len(markers), P(mk), tang, P(vptr), P(vcol), P(sizes), msg, 256)
    if rc != 0:
        return None, msg.value.decode()
    nrows, npairs, nslices, ncols = (int(s) for s in sizes)
    z = lambda n: np.zeros(max(n, 1), dtype=np.int32)  # noqa: E731
    out = dict(row=z(nrows), rptr=z(nrows + 1), pcell=z(npairs), pmeta=z(npairs), pslot=z(n1 * npairs), sptr=z(nslices + 1), dcell=z(64 * ncols),
               dmeta=z(64 * ncols), dslot=z(64 * n1 * ncols))
    th.th_get(*(P(out[k]) for k in ("row", "rptr", "pcell", "pmeta", "pslot", "sptr", "dcell", "dmeta", "dslot")))
    out.update(nrows=nrows, npairs=npairs, nslices=nslices, ncols=ncols)
    return out, ""


def check(mesh, marker, markers, tangential, w, vptr, vcol):
    n1 = mesh.cells.shape[1]
    want = expected(mesh, marker, markers, tangential, vptr, vcol)
    rows = sorted(want)
    assert w["nrows"] == len(rows) and list(w["row"][: len(rows)]) == rows
    assert w["npairs"] == sum(len(v) for v in want.values()) and w["nslices"] == (len(rows) + 63) // 64
    for r, v in enumerate(rows):
        j0, j1 = w["rptr"][r], w["rptr"][r + 1]
        got = [(int(w["pcell"][j]), int(w["pmeta"][j]) & 3, (int(w["pmeta"][j]) >> 2) & 3, int(w["pmeta"][j]) >> 4,
                [int(s) for s in w["pslot"][n1 * j: n1 * (j + 1)]]) for j in range(j0, j1)]
        assert got == want[v], v
        # the sliced copy: slice r // 64, lane r % 64, pair c of the row in column sptr[s] + c, -1 behind the row's last pair
        s, l = divmod(r, 64)
        width = w["sptr"][s + 1] - w["sptr"][s]
        assert width == max(len(want[u]) for u in rows[64 * s: 64 * (s + 1)])
        for c in range(width):
            k = (w["sptr"][s] + c) * 64 + l
            if c >= len(got):
                assert w["dcell"][k] == -1
                continue
            assert w["dcell"][k] == got[c][0] and w["dmeta"][k] == w["pmeta"][j0 + c]
            assert [int(w["dslot"][((w["sptr"][s] + c) * n1 + b) * 64 + l]) for b in range(n1)] == got[c][4]
    # lanes behind the last row of the last slice hold no pair
    if rows:
        s = w["nslices"] - 1
        for c in range(w["sptr"][s], w["sptr"][s + 1]):
            assert (w["dcell"][c * 64 + len(rows) - 64 * s: (c + 1) * 64] == -1).all()


def cases():
    sq = create_unit_square(4, 3)
    m2 = U.mark_ends(sq)                       # one corner triangle with an OUTLET facet and an INLET facet
    cu = create_unit_cube(2)                   # 2^3 bricks
    m3 = U.mark_ends(cu)
    big = create_unit_square(40, 3)            # more than one slice of rows
    mb = np.full(big.num_facets, U.INLET, dtype=np.int32)
    return {"square": (sq, m2), "cube": (cu, m3), "long": (big, mb)}


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("tangential", [(1, 0), (0, 1), (1, 1), (0, 0)])
def test_work_list_matches_its_definition(th, name, tangential):
    mesh, marker = CASES[name]
    vptr, vcol = graph(mesh)
    w, why = build(th, mesh, marker, [U.INLET, U.OUTLET], tangential)
    assert w is not None, why
    check(mesh, marker, [U.INLET, U.OUTLET], tangential, w, vptr, vcol)
    if name == "long":
        assert w["nslices"] > 1


def test_corner_cell_and_shared_vertex(th):
    """The corner triangle with two exterior facets on two different boundaries gives each of its vertices a pair per facet it
    belongs to (plus the opposite vertex of the tangential one); a vertex shared by an inlet and an outlet facet lists both, in
    facet order."""
    mesh, marker = CASES["square"]
    fc = mesh.facet_cells
    both = [e for e in set(fc[marker == U.INLET].tolist()) if e in set(fc[marker == U.OUTLET].tolist())]
    assert len(both) == 1
    e = both[0]
    w, _ = build(th, mesh, marker, [U.INLET, U.OUTLET], (1, 0))
    pairs_of_cell = [(int(w["row"][r]), int(w["pmeta"][j]) >> 4) for r in range(w["nrows"]) for j in range(w["rptr"][r], w["rptr"][r + 1])
                     if w["pcell"][j] == e]
    # inlet facet (tangential): all three vertices; outlet facet: its two vertices
    assert sorted(k for _, k in pairs_of_cell) == [0, 0, 0, 1, 1]
    shared = [v for v in mesh.cells[e] if sum(1 for r, _ in pairs_of_cell if r == v) == 2]
    assert shared                                           # the vertex between the two facets, and the tangential facet's opposite vertex
    for v in shared:
        r = list(w["row"][: w["nrows"]]).index(v)
        ks = [int(w["pmeta"][j]) >> 4 for j in range(w["rptr"][r], w["rptr"][r + 1]) if w["pcell"][j] == e]
        q = [[f for f in range(len(marker)) if fc[f] == e and marker[f] == (U.INLET, U.OUTLET)[k]][0] for k in ks]
        assert q == sorted(q)                               # facet order of the mesh


def test_dirichlet_rows_stay_in_the_list(th):
    """The list depends on mesh, markers and switches only: rows of constrained vertices (the wall vertices at the ends of the inlet
    and the outlet) are listed like every other row -- the kernel masks them with the Dirichlet flags it reads -- so Dirichlet
    data may change without a new list."""
    mesh, marker = CASES["cube"]
    w, _ = build(th, mesh, marker, [U.INLET, U.OUTLET], (1, 0))
    wall = set(U.wall_nodes(mesh, marker).tolist())
    rows = set(w["row"][: w["nrows"]].tolist())
    on_traction = set(np.asarray(mesh.facet_vertices)[marker != U.WALL].ravel().tolist())
    assert wall & on_traction and (wall & on_traction) <= rows and on_traction <= rows


@pytest.mark.parametrize("name", sorted(CASES))
def test_empty_boundary(th, name):
    mesh, marker = CASES[name]
    for markers, tang in (([], ()), ([77], (1,))):          # no boundary; a boundary without facets
        w, why = build(th, mesh, marker, markers, tang)
        assert w is not None and (w["nrows"], w["npairs"], w["nslices"], w["ncols"]) == (0, 0, 0, 0) and w["rptr"][0] == 0


def test_missing_graph_column_is_refused(th):
    mesh, marker = CASES["square"]
    vptr, vcol = graph(mesh)
    vcol = vcol.copy()
    row = int(np.asarray(mesh.facet_vertices)[marker == U.INLET][0, 0])
    vcol[vptr[row]: vptr[row + 1]] = -5
    w, why = build(th, mesh, marker, [U.INLET, U.OUTLET], (1, 0), vptr, vcol)
    assert w is None and "is no column of row %d" % row in why


def test_argument_checks(th):
    msg = ctypes.create_string_buffer(256)

    def chk(markers, values, beta, bf=None, nmax=8):
        m, v = i32(markers), np.ascontiguousarray(values, dtype=np.float64)
        b = None if bf is None else np.ascontiguousarray(bf, dtype=np.float64)
        rc = th.th_check(len(m), nmax, P(m) if len(m) else None, P(v) if len(v) else None, float(beta), None if b is None else P(b), msg, 256)
        return rc, msg.value.decode()
    assert chk([1, 2], [1.0, 0.0], 10.0)[0] == 0 and chk([], [], 0.0)[0] == 0 and chk([1, 2], [1.0, 0.0], 0.0, [0.0, 0.4])[0] == 0
    for args, word in [(([1, 1], [1.0, 0.0], 1.0), "twice"), (([1, 2], [np.inf, 0.0], 1.0), "not finite"), (([1, 2], [np.nan, 0.0], 1.0), "not finite"),
                       (([1, 2], [1.0, 0.0], -1.0), "beta_nitsche"), (([1, 2], [1.0, 0.0], np.nan), "beta_nitsche"),
                       (([1, 2], [1.0, 0.0], 1.0, [0.0, -0.1]), "beta_backflow 1"), (([1, 2], [1.0, 0.0], 1.0, [np.inf, 0.0]), "beta_backflow 0"),
                       ((list(range(9)), [0.0] * 9, 1.0), "n <= 8")]:
        rc, why = chk(*args)
        assert rc == -1 and word in why, (args, why)


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("traction_host_san") / "traction_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "traction_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("tang", [1, 2])
def test_builder_under_sanitizers(sanitized, tmp_path, name, tang):
    mesh, marker = CASES[name]
    vptr, vcol = graph(mesh)
    path = str(tmp_path / "list.bin")
    with open(path, "wb") as f:
        f.write(np.array([mesh.x.shape[1], mesh.num_vertices, len(mesh.cells), len(marker), 2, tang, len(vcol)], np.int32).tobytes())
        for a in (mesh.cells, mesh.facet_cells, mesh.facet_local, marker, [U.INLET, U.OUTLET], vptr, vcol):
            f.write(i32(a).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
    w = expected(mesh, marker, [U.INLET, U.OUTLET], [(tang >> k) & 1 for k in range(2)], vptr, vcol)
    assert r.stdout.split()[1:3] == [str(len(w)), str(sum(len(v) for v in w.values()))]
