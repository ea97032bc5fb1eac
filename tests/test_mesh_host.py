"""The host mesh set-up shared by the context builders (csrc/cfdh_mesh_host.hpp) on the CPU: the header is compiled with g++
behind the extern "C" wrappers of mesh_host_shim.cpp and loaded with ctypes -- no libcfdh.so, no GPU.  Expected values come from
the definitions in numpy, not from a second copy of the loops.  The same steps run once more in a stand-alone program built with
AddressSanitizer and UBSan (mesh_host_main.cpp), as a child process."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

import amg_twin
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
from cfd_hemodynamic_amd.parallel import LocalPart, partition_vertices_rcb
from gen3_util import node_mesh3
from gen_util import node_mesh
from util import dfg_case

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cfd_hemodynamic_amd", "csrc")
ip = ctypes.POINTER(ctypes.c_int)
dp = ctypes.POINTER(ctypes.c_double)
i64 = ctypes.c_int64
TRI_EDGES = np.array([[1, 2], [0, 2], [0, 1]], dtype=np.int32)                             # edge of P2 node 3 + q
TET_EDGES = np.array([[2, 3], [1, 3], [1, 2], [0, 3], [0, 2], [0, 1]], dtype=np.int32)     # edge of P2 node 4 + q (include/cfdh.h)


@pytest.fixture(scope="module")
def mh(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mesh_host") / "mesh_host_shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I", CSRC, os.path.join(HERE, "mesh_host_shim.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    c_int, msg = ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]
    L.mh_check_sizes.argtypes = [i64, i64, i64, c_int, ip, i64, i64] + msg
    L.mh_check_facets.argtypes = [i64, ip, ip, i64, c_int] + msg
    L.mh_morton.argtypes = [c_int] * 5 + [dp, ip, ip, dp] + msg
    L.mh_select_cells.argtypes = [c_int] * 3 + [ip] * 5
    L.mh_node_graph.argtypes = [c_int] * 3 + [ip] * 7 + msg
    L.mh_graph_slots.argtypes = [c_int] * 3 + [ip] * 4
    L.mh_staging_order.argtypes = [c_int] * 4 + [ip, c_int] + [ip] * 4
    L.mh_scatter.argtypes = [c_int] * 3 + [ip, ip, c_int] + [dp] * 5
    L.mh_p1_subspace.argtypes = [c_int, c_int, ip, c_int, c_int, ip, ip, ip, dp]
    L.mh_tri_det.argtypes = [dp, ip]
    L.mh_tri_det.restype = ctypes.c_double
    L.mh_is_parallelogram.argtypes = [dp, ip, ctypes.c_double]
    L.mh_is_parallelepiped.argtypes = [dp, ip, ctypes.c_double]
    L.mh_p2_bent_edge.argtypes = [c_int, ip, dp, ip, ctypes.c_double]
    L.mh_lcg.argtypes = [i64, dp]
    return L


def P(a):
    return a.ctypes.data_as(dp if a.dtype == np.float64 else ip)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# ---------------------------------------------------------------------------------------------------------------- meshes
def _plain(kind, D, m):
    nl = m.cells.shape[1]
    return types.SimpleNamespace(kind=kind, D=D, NL=nl, NV=D + 1 if kind != "Q1" else 2 ** D, NF={3: 3, 6: 3, 4: 4 if D == 2 else 4, 10: 4, 8: 6}[nl],
                                 x=np.ascontiguousarray(m.x, dtype=np.float64), cells=i32(m.cells), nvo=len(m.x), fcell=i32(m.facet_cells),
                                 flocal=i32(m.facet_local), edges=(TRI_EDGES if D == 2 else TET_EDGES) if kind == "P2" else None)


def _part(s, rank=0):
    """Part `rank` of a 2-part split with two layers of cells: ghost nodes and cells that touch no owned node are present."""
    g = types.SimpleNamespace(x=s.x, cells=s.cells, num_vertices=len(s.x), num_cells=len(s.cells), facet_cells=s.fcell, facet_local=s.flocal,
                              facet_marker=np.zeros(len(s.fcell), dtype=np.int32))
    lp = LocalPart(g, partition_vertices_rcb(s.x, 2), rank, layers=2)
    assert 0 < lp.nvo < lp.nv
    return types.SimpleNamespace(kind=s.kind, D=s.D, NL=s.NL, NV=s.NV, NF=s.NF, x=np.ascontiguousarray(lp.x), cells=i32(lp.cells), nvo=lp.nvo,
                                 fcell=i32(lp.facet_cells), flocal=i32(lp.facet_local), edges=s.edges,
                                 second_layer=int((~(lp.cells < lp.nvo).any(axis=1)).sum()))


def _meshes():
    out = {}
    for kind in ("P1", "P2", "Q1"):
        out["%s-2d" % kind] = _plain(kind, 2, node_mesh(kind, 3, 0.1))
        out["%s-3d" % kind] = _plain(kind, 3, node_mesh3(kind, 2 if kind == "P2" else 3, 0.1))
    out["dfg6"] = _plain("P1", 2, dfg_case(6).mesh)
    out["cube3"] = _plain("P1", 3, create_unit_cube(3))
    for name in list(out):
        out[name + "-part"] = _part(out[name], rank=1 if name == "dfg6" else 0)
    # cells that touch no owned node: the smallest meshes are too small to have any, these have
    assert all(out[n + "-part"].second_layer > 0 for n in ("dfg6", "cube3", "P1-3d", "Q1-3d"))
    return out


MESHES = _meshes()
NAMES = sorted(MESHES)
BITS = {2: (16,), 3: (10, 21)}


# ---------------------------------------------------------------------------------------------- numpy side of the definitions
def morton_keys(x, nvo, bits):
    """Bits of the quantised coordinates interleaved, axis 0 lowest; the box is that of ALL nodes, scaled by its longest side."""
    lo, D = x.min(axis=0), x.shape[1]
    ext = (x.max(axis=0) - lo).max()
    qmax = float(2 ** bits - 1)
    q = np.minimum(qmax, (x[:nvo] - lo) / ext * qmax).astype(np.uint64)
    key = np.zeros(nvo, dtype=np.uint64)
    for b in range(bits):
        for i in range(D):
            key |= ((q[:, i] >> np.uint64(b)) & np.uint64(1)) << np.uint64(D * b + i)
    return key


def numbering(mh, s, bits, renumber=True):
    nv = len(s.x)
    perm, iperm, X = np.zeros(nv, np.int32), np.zeros(nv, np.int32), np.zeros_like(s.x)
    msg = ctypes.create_string_buffer(256)
    assert mh.mh_morton(s.D, bits, int(renumber), nv, s.nvo, P(s.x), P(perm), P(iperm), P(X), msg, 256) == 0, msg.value
    return perm, iperm, X


def context_cells(mh, s, perm):
    """Cells of the context in internal numbering: the generic builders keep them all, in user order."""
    return i32(perm[s.cells])


def graph(mh, s, h_cells, iperm):
    nc, NL = h_cells.shape
    iptr, vptr, vdiag = np.zeros(s.nvo + 1, np.int32), np.zeros(s.nvo + 1, np.int32), np.zeros(s.nvo, np.int32)
    inc, vcol = np.zeros(NL * nc, np.int32), np.zeros(NL * NL * nc, np.int32)
    msg = ctypes.create_string_buffer(256)
    nnz = mh.mh_node_graph(NL, nc, s.nvo, P(h_cells), P(iperm), P(iptr), P(inc), P(vptr), P(vcol), P(vdiag), msg, 256)
    return nnz, iptr, inc[:iptr[-1]], vptr, vcol[:max(nnz, 0)], vdiag, msg.value.decode()


def built(mh, s):
    """numbering -> cells -> graph -> graph slots of one mesh (the steps of a generic builder)"""
    perm, iperm, X = numbering(mh, s, BITS[s.D][0])
    hc = context_cells(mh, s, perm)
    nnz, iptr, inc, vptr, vcol, vdiag, why = graph(mh, s, hc, iperm)
    assert nnz > 0, why
    slot = np.zeros(hc.size * s.NL, np.int32)
    mh.mh_graph_slots(s.NL, len(hc), s.nvo, P(hc), P(vptr), P(vcol), P(slot))
    return types.SimpleNamespace(perm=perm, iperm=iperm, X=X, hc=hc, nnz=nnz, iptr=iptr, inc=inc, vptr=vptr, vcol=vcol, vdiag=vdiag, slot=slot)


# ----------------------------------------------------------------------------------------------------------------- Morton
@pytest.mark.parametrize("name", NAMES)
def test_morton_numbering(mh, name):
    s = MESHES[name]
    nv = len(s.x)
    for bits in BITS[s.D]:
        perm, iperm, X = numbering(mh, s, bits)
        assert np.array_equal(np.sort(perm), np.arange(nv)) and np.array_equal(perm[iperm], np.arange(nv))
        assert np.array_equal(perm[s.nvo:], np.arange(s.nvo, nv))  # ghosts keep their place
        assert np.array_equal(iperm[:s.nvo], np.argsort(morton_keys(s.x, s.nvo, bits), kind="stable"))
        assert np.array_equal(X, s.x[iperm])
    perm, iperm, X = numbering(mh, s, BITS[s.D][0], renumber=False)
    assert np.array_equal(perm, np.arange(nv)) and np.array_equal(iperm, np.arange(nv)) and np.array_equal(X, s.x)


def test_morton_ties_keep_input_order(mh):
    # 4000 points in a cube quantised to 10 bits per axis, most of them drawn inside 16 quantisation cells: many equal keys
    rng = np.random.default_rng(3)
    x = np.vstack([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], rng.integers(0, 4, (3598, 3)) / 4.0 + rng.uniform(0, 0.9 / 1023, (3598, 3)), rng.uniform(0, 1, (400, 3))])
    s = types.SimpleNamespace(D=3, x=np.ascontiguousarray(x), nvo=3500)
    key = morton_keys(x, s.nvo, 10)
    assert len(np.unique(key)) < s.nvo // 4
    perm, iperm, _ = numbering(mh, s, 10)
    assert np.array_equal(iperm[:s.nvo], np.argsort(key, kind="stable"))
    srt = key[iperm[:s.nvo]]
    tie = srt[1:] == srt[:-1]
    assert tie.sum() > 2000 and (np.diff(iperm[:s.nvo])[tie] > 0).all()
    assert np.array_equal(iperm[s.nvo:], np.arange(s.nvo, len(x)))


def test_morton_refuses_zero_extent(mh):
    x = np.full((5, 2), 0.25)
    msg = ctypes.create_string_buffer(256)
    out = np.zeros(5, np.int32)
    for renumber in (0, 1):
        assert mh.mh_morton(2, 16, renumber, 5, 5, P(x), P(out), P(out.copy()), P(np.zeros_like(x)), msg, 256) == -1
        assert msg.value == b"degenerate coordinates"


# ------------------------------------------------------------------------------------------------- closed-form cell selection
@pytest.mark.parametrize("name", [n for n in NAMES if MESHES[n].kind == "P1"])
def test_select_cells(mh, name):
    s = MESHES[name]
    perm, _, _ = numbering(mh, s, BITS[s.D][-1])
    ncu = len(s.cells)
    hc, cu, cmap = np.zeros((ncu, s.NL), np.int32), np.zeros(ncu, np.int32), np.zeros(ncu, np.int32)
    nc = mh.mh_select_cells(s.NL, ncu, s.nvo, P(s.cells), P(perm), P(hc), P(cu), P(cmap))
    smallest = perm[s.cells].min(axis=1)
    keep = np.nonzero(smallest < s.nvo)[0]
    want = keep[np.argsort(smallest[keep], kind="stable")]
    assert nc == len(want) and np.array_equal(cu[:nc], want) and np.array_equal(hc[:nc], perm[s.cells[want]])
    assert np.array_equal(cmap[want], np.arange(nc)) and (np.delete(cmap, want) == -1).all()
    if name.endswith("-part"):
        assert ncu - nc == s.second_layer  # cells that touch no owned node are dropped by the closed forms


# ------------------------------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("name", NAMES)
def test_node_graph(mh, name):
    s = MESHES[name]
    b = built(mh, s)
    assert len(b.vptr) == s.nvo + 1 and b.vptr[0] == 0 and b.vptr[-1] == b.nnz  # rows for owned nodes only
    t = np.arange(b.hc.size)
    for v in range(s.nvo):
        mine = t[b.hc.ravel() == v]                         # positions of v in the cells, ascending
        assert np.array_equal(b.inc[b.iptr[v]:b.iptr[v + 1]], mine)
        want = np.unique(b.hc[mine // s.NL])
        assert np.array_equal(b.vcol[b.vptr[v]:b.vptr[v + 1]], want)
        assert b.vcol[b.vdiag[v]] == v and b.vptr[v] <= b.vdiag[v] < b.vptr[v + 1]


def test_node_in_no_cell_is_reported_by_its_user_number(mh):
    s = MESHES["P2-2d"]
    perm, iperm, _ = numbering(mh, s, 16)
    lonely = 17
    cells = s.cells[~(s.cells == lonely).any(axis=1)]
    nnz, *_, why = graph(mh, s, i32(perm[cells]), iperm)
    assert nnz == -1 and why == "node %d belongs to no cell" % lonely


# ----------------------------------------------------------------------------------------------------------------- staging
@pytest.mark.parametrize("name", NAMES)
def test_staging_order(mh, name):
    s = MESHES[name]
    b = built(mh, s)
    nc, NL = b.hc.shape
    ghost_row = np.repeat(b.hc.ravel() >= s.nvo, NL)
    # the graph slot of (cell, a, b) is the position of node b in the row of node a; -1 in the row of a ghost
    assert (b.slot[ghost_row] == -1).all() and (b.slot[~ghost_row] >= 0).all()
    rows, cols = np.repeat(b.hc.ravel(), NL), np.repeat(b.hc, NL, axis=0).ravel()
    ok = ~ghost_row
    assert np.array_equal(b.vcol[b.slot[ok]], cols[ok]) and (b.vptr[rows[ok]] <= b.slot[ok]).all() and (b.slot[ok] < b.vptr[rows[ok] + 1]).all()
    own = np.nonzero(ok)[0]
    order = own[np.argsort(b.slot[own], kind="stable")]  # by graph entry, then ascending (cell, a, b)
    want = np.full(b.slot.size, -1)
    want[order] = np.arange(len(own))
    want_eptr = np.concatenate([[0], np.cumsum(np.bincount(b.slot[own], minlength=b.nnz))])
    node = b.hc.ravel()
    town = np.nonzero(node < s.nvo)[0]
    torder = town[np.argsort(node[town], kind="stable")]  # by node, then ascending (cell, a)
    for fper in (1, NL):
        st, eptr, fptr, fdst = b.slot.copy(), np.zeros(b.nnz + 1, np.int32), np.zeros(s.nvo + 1, np.int32), np.zeros(nc * NL * fper, np.int32)
        mh.mh_staging_order(NL, nc, s.nvo, b.nnz, P(b.hc), fper, P(st), P(eptr), P(fptr), P(fdst))
        assert np.array_equal(eptr, want_eptr) and np.array_equal(st, want)
        assert np.array_equal(np.sort(st[own]), np.arange(eptr[-1]))  # a bijection onto [0, eptr[nnz])
        wf = np.full((nc * NL, fper), -1)
        wf[torder] = np.arange(len(town) * fper).reshape(-1, fper)
        assert np.array_equal(fdst, wf.ravel())
        assert np.array_equal(fptr, fper * np.concatenate([[0], np.cumsum(np.bincount(node[town], minlength=s.nvo))]))
        assert np.array_equal(np.sort(fdst[fdst >= 0]), np.arange(fptr[-1]))


# -------------------------------------------------------------------------------------------------------------- P1 subspace
@pytest.mark.parametrize("name", [n for n in NAMES if MESHES[n].kind == "P2"])
def test_p1_subspace(mh, name):
    s = MESHES[name]
    b = built(mh, s)
    nv = len(s.x)
    rp, col, val = np.zeros(nv + 1, np.int32), np.zeros(2 * nv, np.int32), np.zeros(2 * nv)
    nvert = mh.mh_p1_subspace(s.NL, s.NV, P(s.edges), len(b.hc), nv, P(b.hc), P(rp), P(col), P(val))
    Pw, verts = amg_twin.p1_interpolation(b.X, b.hc, s.NV)
    assert nvert == len(verts) == Pw.shape[1] and rp[-1] == Pw.nnz
    assert np.array_equal(rp, Pw.indptr) and np.array_equal(col[:rp[-1]], Pw.indices) and np.array_equal(val[:rp[-1]], Pw.data)


# ------------------------------------------------------------------------------------------------------------------ scatter
def _measure(s, X, hc):
    e = [X[hc[:, a]] - X[hc[:, 0]] for a in ((1, 2) if s.D == 2 else (1, 2, 4 if s.kind == "Q1" else 3))]
    det = np.abs(np.linalg.det(np.stack(e, axis=1)))
    return det if s.kind == "Q1" else det / (2.0 if s.D == 2 else 6.0)


@pytest.mark.parametrize("name", NAMES)
def test_scatter_stiffness_mass(mh, name):
    s = MESHES[name]
    b = built(mh, s)
    nc, NL = b.hc.shape
    nv = len(s.x)
    rng = np.random.default_rng(11)
    Wm = rng.uniform(0.1, 1.0, (nc, NL, NL))
    Wm = Wm + Wm.transpose(0, 2, 1)
    K = np.ascontiguousarray(-Wm)
    for a in range(NL):
        K[:, a, a] = 0.0
        K[:, a, a] = -K[:, a, :].sum(axis=1)  # Laplacian-like: every row of a cell matrix sums to zero
    Md, meas = rng.uniform(0.5, 1.5, (nc, NL)), _measure(s, b.X, b.hc)
    Lval, Ml = np.zeros(b.nnz), np.zeros(nv)
    mh.mh_scatter(NL, nc, nv, P(b.hc), P(b.slot), b.nnz, P(K), P(Md), P(meas), P(Lval), P(Ml))
    ok = b.slot >= 0
    want = np.bincount(b.slot[ok], weights=K.ravel()[ok], minlength=b.nnz)
    # a row holds at most a few dozen terms of size at most max|L|: reordering moves an entry, and a row sum, by under 30 eps
    bound = 1e-13 * np.abs(want).max()
    assert np.abs(Lval - want).max() <= bound
    assert np.abs(np.add.reduceat(Lval, b.vptr[:-1])).max() <= bound
    # HRZ: the diagonal mass scaled to the mesh measure, ghost nodes included; a sum of under 1000 terms, each a few eps off
    wm = np.bincount(b.hc.ravel(), weights=Md.ravel(), minlength=nv) * (meas.sum() / Md.sum())
    assert np.abs(Ml - wm).max() <= 1e-13 * wm.max() and abs(Ml.sum() - meas.sum()) <= 1e-12 * meas.sum()


# ---------------------------------------------------------------------------------------------------------------- refusals
def _sizes(mh, s, cells=None, nvo=None):
    cells = s.cells if cells is None else cells
    msg = ctypes.create_string_buffer(256)
    rc = mh.mh_check_sizes(len(s.x), s.nvo if nvo is None else nvo, len(cells), s.NL, P(cells), 1 << 28, 1 << 24, msg, 256)
    return rc, msg.value.decode()


def _facets(mh, s, flocal):
    msg = ctypes.create_string_buffer(256)
    return mh.mh_check_facets(len(s.fcell), P(s.fcell), P(flocal), len(s.cells), s.NF, msg, 256), msg.value.decode()


@pytest.mark.parametrize("name", NAMES)
def test_index_refusals(mh, name):
    s = MESHES[name]
    assert _sizes(mh, s) == (0, "") and _facets(mh, s, s.flocal) == (0, "")
    for bad in (len(s.x), -1):
        cells = s.cells.copy()
        cells[len(cells) // 2, s.NL - 1] = bad
        assert _sizes(mh, s, cells=cells) == (-1, "cell node index out of range")
    for bad in (s.NF, -1):
        fl = s.flocal.copy()
        fl[len(fl) // 2] = bad
        assert _facets(mh, s, fl) == (-1, "facet (cell, local) out of range")
    assert _sizes(mh, s, nvo=len(s.x) + 1) == (-1, "bad owned node count")
    assert _sizes(mh, s, nvo=0) == (-1, "bad owned node count")
    msg = ctypes.create_string_buffer(256)
    assert mh.mh_check_sizes(len(s.x), s.nvo, len(s.cells), s.NL, P(s.cells), len(s.x) - 1, 1 << 24, msg, 256) == -1
    assert msg.value == b"mesh too large for int32 indexing"


def _adet(s, X, v):
    return _measure(s, X, v[None, :])[0] * (1.0 if s.kind == "Q1" else (2.0 if s.D == 2 else 6.0))


@pytest.mark.parametrize("name", [n for n in NAMES if MESHES[n].kind != "P1"])
def test_shape_refusals(mh, name):
    s = MESHES[name]
    b = built(mh, s)
    X = b.X

    def bad_cells(Xc):
        out = []
        for e, v in enumerate(b.hc):
            a = _adet(s, Xc, v)
            if s.kind == "P2":
                q = mh.mh_p2_bent_edge(s.D, P(s.edges), P(Xc), P(np.ascontiguousarray(v)), a)
                if q >= 0:
                    out.append((e, q))
            elif not (mh.mh_is_parallelogram if s.D == 2 else mh.mh_is_parallelepiped)(P(Xc), P(np.ascontiguousarray(v)), a):
                out.append(e)
        return out

    assert bad_cells(X) == []  # the sheared affine meshes are accepted
    h = _adet(s, X, b.hc[0]) ** (1.0 / s.D)
    e = len(b.hc) // 2
    if s.kind == "Q1":
        for corner in range(1, s.NV):  # corner 0 carries the affine map: moving it alone moves the whole reference frame
            Xm = X.copy()
            Xm[b.hc[e, corner], s.D - 1] += 1e-6 * h
            assert e in bad_cells(Xm)
        Xm = X.copy()
        Xm[b.hc[e, s.NV - 1], 0] += 1e-12 * h  # below the tolerance of 1e-9 h
        assert bad_cells(Xm) == []
    else:
        for q in range(len(s.edges)):
            Xm = X.copy()
            Xm[b.hc[e, s.NV + q], q % s.D] += 1e-6 * h
            hit = bad_cells(Xm)
            assert (e, q) in hit and all(b.hc[c, s.NV + qq] == b.hc[e, s.NV + q] for c, qq in hit)


def test_zero_area_cell(mh):
    s = MESHES["P1-2d"]
    b = built(mh, s)
    dets = np.array([mh.mh_tri_det(P(b.X), P(np.ascontiguousarray(v))) for v in b.hc])
    assert (np.abs(dets) > 0).all() and np.allclose(np.abs(dets), 2.0 * _measure(s, b.X, b.hc), rtol=1e-13)
    Xm = b.X.copy()
    Xm[b.hc[4, 2]] = Xm[b.hc[4, 1]]  # two corners of cell 4 coincide
    assert mh.mh_tri_det(P(Xm), P(np.ascontiguousarray(b.hc[4]))) == 0.0


# --------------------------------------------------------------------------------------------------------------------- LCG
def test_lcg_vector(mh):
    n = 4096
    st, want = np.uint64(0x2545F4914F6CDD1D), np.zeros(64)
    with np.errstate(over="ignore"):
        for k in range(64):
            st = st * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
            want[k] = float(st >> np.uint64(11)) * 2.0 ** -53 - 0.5
    a, b = np.zeros(n), np.zeros(100)
    mh.mh_lcg(n, P(a))
    mh.mh_lcg(100, P(b))
    assert np.array_equal(a[:64], want) and np.array_equal(a[:100], b)  # a shorter vector is a prefix of a longer one
    assert a.min() >= -0.5 and a.max() < 0.5 and abs(a.mean()) < 0.05


# -------------------------------------------------------------------------------------------------- the same under sanitizers
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mesh_host_san") / "mesh_host_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "mesh_host_main.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", NAMES)
def test_steps_under_sanitizers(sanitized, tmp_path, name):
    s = MESHES[name]
    ne = 0 if s.edges is None else len(s.edges)
    path = str(tmp_path / "mesh.bin")
    with open(path, "wb") as f:
        f.write(np.array([s.D, s.NL, s.NV, s.NF, BITS[s.D][-1 if s.kind == "P1" else 0], len(s.x), s.nvo, len(s.cells), len(s.fcell), ne], np.int32).tobytes())
        for a in (s.cells, s.fcell, s.flocal) + (() if s.edges is None else (s.edges,)):
            f.write(i32(a).tobytes())
        f.write(np.ascontiguousarray(s.x, dtype=np.float64).tobytes())
    r = subprocess.run([sanitized, path], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr
