"""Host side of the Lagrangian particle tracker (cfdh_particles_*, include/cfdh.h): where to release particles, how to find the
cell of an arbitrary point, and what to make of the result -- residence times per exit, output files, a VTU point cloud.

The device wants every seed with the cell that holds it (all barycentric coordinates >= -1e-9).  The helpers here return both:
`sample_in_cells` and `sample_on_marker` draw points in known cells, `locate` finds the cells of points that come from elsewhere."""
from __future__ import annotations

import os
import struct

import numpy as np

STATUS_ACTIVE, STATUS_LOST = 0, -1  # an exit through a facet of marker m is 1 + m


def _simplex(mesh):
    cells = np.asarray(mesh.cells)
    d = cells.shape[1] - 1
    if d not in (2, 3) or np.asarray(mesh.x).shape[1] < d:
        raise NotImplementedError("particles live on P1 simplex meshes (triangles, tetrahedra)")
    return np.asarray(mesh.x, dtype=float)[:, :d], cells, d


def barycentric(mesh, cells, points):
    """lambda [n, d + 1] of points[k] in the mesh cell cells[k]."""
    x, conn, d = _simplex(mesh)
    X = x[conn[np.asarray(cells)]]
    M = np.transpose(X[:, 1:, :] - X[:, :1, :], (0, 2, 1))  # columns x_a - x_0
    l = np.linalg.solve(M, (np.asarray(points, dtype=float)[:, :d] - X[:, 0, :])[:, :, None])[:, :, 0]
    return np.concatenate([1.0 - l.sum(axis=1, keepdims=True), l], axis=1)


def neighbours(mesh):
    """nb [nc, d + 1]: the cell across the facet opposite local vertex f, -1 on the boundary."""
    x, conn, d = _simplex(mesh)
    nc, n1 = conn.shape
    keys = np.stack([np.sort(np.delete(conn, f, axis=1), axis=1) for f in range(n1)], axis=1).reshape(nc * n1, d)
    order = np.lexsort(keys.T[::-1])
    ks = keys[order]
    same = (ks[1:] == ks[:-1]).all(axis=1)
    nb = np.full(nc * n1, -1, dtype=np.int64)
    a, b = order[:-1][same], order[1:][same]
    nb[a], nb[b] = b // n1, a // n1
    return nb.reshape(nc, n1)


def sample_in_cells(mesh, cells, rng, pull=1e-3):
    """One point per listed cell, uniform in the cell shrunk towards its centroid by `pull`.  Returns (x [n, d], cells [n])."""
    x, conn, d = _simplex(mesh)
    cells = np.asarray(cells, dtype=np.int32)
    lam = rng.dirichlet(np.ones(d + 1), size=len(cells))
    lam = (1.0 - pull) * lam + pull / (d + 1)
    return np.einsum("ka,kai->ki", lam, x[conn[cells]]), cells


def sample_on_marker(mesh, facets, n, rng, offset=1e-3):
    """n points on the exterior facets `facets` (indices into mesh.facet_cells / facet_local, e.g. facet_tags.find(marker)), drawn
    with probability proportional to the facet's measure and pulled inside the owning cell by a barycentric offset: the coordinate of
    the opposite vertex is `offset`, the facet's own coordinates are scaled by 1 - offset and keep at least offset / 2 each.
    Returns (x [n, d], cells [n])."""
    x, conn, d = _simplex(mesh)
    facets = np.asarray(facets, dtype=np.int64)
    if len(facets) == 0:
        raise ValueError("no facet to release particles from")
    fc, fl = np.asarray(mesh.facet_cells)[facets], np.asarray(mesh.facet_local)[facets]
    loc = np.stack([np.delete(np.arange(d + 1), f) for f in range(d + 1)])[fl]  # local vertices of the facet
    V = x[np.take_along_axis(conn[fc], loc, axis=1)]
    if d == 2:
        meas = np.linalg.norm(V[:, 1] - V[:, 0], axis=1)
    else:
        meas = 0.5 * np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]), axis=1)
    pick = rng.choice(len(facets), size=int(n), p=meas / meas.sum())
    mu = rng.dirichlet(np.ones(d), size=int(n))
    mu = (1.0 - 0.5 * d * offset) * mu + 0.5 * offset
    lam = np.zeros((int(n), d + 1))
    np.put_along_axis(lam, loc[pick], (1.0 - offset) * mu, axis=1)
    lam[np.arange(int(n)), fl[pick]] = offset
    cells = fc[pick].astype(np.int32)
    return np.einsum("ka,kai->ki", lam, x[conn[cells]]), cells


def locate(mesh, points, tol=1e-9, max_steps=256):
    """Cells of arbitrary points: start at the cell with the nearest centroid (scipy cKDTree), then walk towards the point across
    the facet with the most negative barycentric coordinate.  Returns cells [n], -1 for a point outside the mesh (the walk ran
    into the boundary or did not end within `max_steps`)."""
    from scipy.spatial import cKDTree
    x, conn, d = _simplex(mesh)
    pts = np.asarray(points, dtype=float).reshape(-1, np.asarray(points).shape[-1])[:, :d]
    cur = cKDTree(x[conn].mean(axis=1)).query(pts)[1].astype(np.int64)
    nb = neighbours(mesh)
    out = np.full(len(pts), -1, dtype=np.int32)
    todo = np.arange(len(pts))
    for _ in range(max_steps):
        if len(todo) == 0:
            break
        lam = barycentric(mesh, cur[todo], pts[todo])
        worst = lam.argmin(axis=1)
        inside = lam[np.arange(len(todo)), worst] >= -tol
        out[todo[inside]] = cur[todo[inside]]
        nxt = nb[cur[todo], worst]
        go = ~inside & (nxt >= 0)
        cur[todo[go]] = nxt[go]
        todo = todo[go]
    return out


def residence_times(status, age):
    """Per status value (0 active, 1 + marker for an exit, -1 lost): dict(count, ages, mean, median, p95)."""
    status, age = np.asarray(status), np.asarray(age, dtype=float)
    out = {}
    for s in np.unique(status):
        a = age[status == s]
        out[int(s)] = dict(count=int(len(a)), ages=a, mean=float(a.mean()), median=float(np.median(a)), p95=float(np.percentile(a, 95)))
    return out


def write_npz(path, fields, summary=None):
    """particles.npz: the final fields (x, cell, status, age, path, exposure, t_end) and per status s `count_<s>` and `ages_<s>`."""
    summary = residence_times(fields["status"], fields["age"]) if summary is None else summary
    extra = {}
    for s, r in summary.items():
        extra["count_%d" % s] = np.int64(r["count"])
        extra["ages_%d" % s] = r["ages"]
    np.savez(path, **{k: np.asarray(v) for k, v in fields.items()}, **extra)


def write_summary(path, summary, t_end):
    """particles.txt: one line per status."""
    with open(path, "w") as f:
        f.write("# particles at t = %.12g: status (0 active, 1 + marker exit, -1 lost), count, mean / median / 95 %% age\n" % t_end)
        for s, r in sorted(summary.items()):
            f.write("%d %d %.9g %.9g %.9g\n" % (s, r["count"], r["mean"], r["median"], r["p95"]))


def write_vtu(path, x, fields):
    """Point cloud: one VTK_VERTEX per particle with the arrays of `fields` (status, age, path, exposure, ...) as point data."""
    x = np.asarray(x, dtype=float)
    n = len(x)
    pts = np.zeros((n, 3))
    pts[:, :x.shape[1]] = x
    data = {k: np.asarray(v, dtype=np.float64).reshape(n, -1) for k, v in fields.items()}
    arrays = [pts.ravel(), np.arange(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), np.full(n, 1, dtype=np.uint8)] + [v.ravel() for v in data.values()]
    offs, blob = [], bytearray()
    for a in arrays:
        offs.append(len(blob))
        raw = np.ascontiguousarray(a).tobytes()
        blob += struct.pack("<Q", len(raw)) + raw
    point_data = "\n".join('<DataArray type="Float64" Name="%s" NumberOfComponents="%d" format="appended" offset="%d"/>' % (k, v.shape[1], off)
                           for (k, v), off in zip(data.items(), offs[4:]))
    head = ('<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
            '<UnstructuredGrid><Piece NumberOfPoints="%d" NumberOfCells="%d">\n'
            '<Points><DataArray type="Float64" NumberOfComponents="3" format="appended" offset="%d"/></Points>\n'
            '<Cells>\n<DataArray type="Int32" Name="connectivity" format="appended" offset="%d"/>\n'
            '<DataArray type="Int32" Name="offsets" format="appended" offset="%d"/>\n'
            '<DataArray type="UInt8" Name="types" format="appended" offset="%d"/>\n</Cells>\n<PointData>%s</PointData>\n'
            '</Piece></UnstructuredGrid>\n<AppendedData encoding="raw">\n_' % (n, n, offs[0], offs[1], offs[2], offs[3], point_data))
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(bytes(blob))
        f.write(b"\n</AppendedData>\n</VTKFile>\n")


class CloudWriter:
    """The point clouds of a run: <folder>/particles_NNNNNN.vtu per written step and particles.pvd as the time index."""

    def __init__(self, folder):
        self.folder, self.steps = folder, []
        os.makedirs(folder, exist_ok=True)

    def write(self, t, fields):
        fn = "particles_%06d.vtu" % len(self.steps)
        write_vtu(os.path.join(self.folder, fn), fields["x"], {k: v for k, v in fields.items() if k not in ("x", "cell")})
        self.steps.append((float(t), fn))
        with open(os.path.join(self.folder, "particles.pvd"), "w") as f:
            f.write('<?xml version="1.0"?>\n<VTKFile type="Collection" version="0.1" byte_order="LittleEndian">\n<Collection>\n')
            for tt, name in self.steps:
                f.write('<DataSet timestep="%.12g" part="0" file="%s"/>\n' % (tt, name))
            f.write("</Collection>\n</VTKFile>\n")
