"""Sample sets for the point sampler (cfdh_sample_*, SolverBase.sample_*) and the files it writes: points along a line, a regular
grid over a mesh, VTK ImageData (`.vti`, raw-appended binary like the project's VTU files) and npz archives.

The grid is described by (origin, spacing, dims); node (i, j, k) is at origin + (i, j, k) * spacing and has index
i + dims[0] (j + dims[1] k), the point order of VTK ImageData.  The coordinates themselves are generated on the device; nothing here
recomputes them."""
from __future__ import annotations

import re
import struct

import numpy as np


def line(p0, p1, n):
    """n points from p0 to p1, ends included [n, gdim] (n = 1: p0)."""
    p0, p1 = np.asarray(p0, dtype=float), np.asarray(p1, dtype=float)
    if p0.shape != p1.shape or p0.ndim != 1 or int(n) < 1:
        raise ValueError("line: p0 and p1 must be points of one dimension and n >= 1")
    s = np.linspace(0.0, 1.0, int(n))[:, None]
    return (1.0 - s) * p0 + s * p1


def grid_over(mesh, spacing=None, pad=0.0, dims=None):
    """(origin, spacing, dims), each of length 3, of a regular grid over the bounding box of `mesh` widened by `pad` on every side.
    Either `spacing` (a number or one per axis; the grid then reaches at least to the upper corner) or `dims` (nodes per axis; the
    grid then ends on the upper corner) is given.  In 2-D the third entries are (0, 1, 1)."""
    x = np.asarray(getattr(mesh, "x", mesh), dtype=float)
    gdim = int(getattr(getattr(mesh, "geometry", None), "dim", x.shape[1]))
    lo, hi = x[:, :gdim].min(axis=0) - pad, x[:, :gdim].max(axis=0) + pad
    origin, h, n = np.zeros(3), np.ones(3), np.ones(3, dtype=np.int64)
    if (spacing is None) == (dims is None):
        raise ValueError("grid_over: give either spacing or dims")
    if dims is not None:
        d = np.broadcast_to(np.asarray(dims, dtype=np.int64), (gdim,)) if np.ndim(dims) == 0 else np.asarray(dims, dtype=np.int64)[:gdim]
        if (d < 1).any():
            raise ValueError("grid_over: dims must be >= 1")
        n[:gdim] = d
        ext = hi - lo
        h[:gdim] = np.where(d > 1, ext / np.maximum(d - 1, 1), np.where(ext > 0, ext, 1.0))
    else:
        s = np.broadcast_to(np.asarray(spacing, dtype=float), (gdim,)) if np.ndim(spacing) == 0 else np.asarray(spacing, dtype=float)[:gdim]
        if not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("grid_over: the spacing must be finite and positive")
        h[:gdim] = s
        n[:gdim] = np.ceil((hi - lo) / s - 1e-12).astype(np.int64) + 1
    origin[:gdim] = lo
    return origin, h, n


def write_vti(path, origin, spacing, dims, fields, located=None):
    """VTK ImageData with the arrays of `fields` (name -> [n] or [n, k]) as point data, Float64, and, when given, the mask
    `located` (UInt8: 1 where the node lies in a cell)."""
    dims = [int(d) for d in dims]
    n = dims[0] * dims[1] * dims[2]
    data = {k: np.asarray(v, dtype=np.float64).reshape(n, -1) for k, v in fields.items()}
    if any(v.shape[1] == 2 for v in data.values()):  # vectors have three components in VTK
        data = {k: (np.hstack([v, np.zeros((n, 1))]) if v.shape[1] == 2 else v) for k, v in data.items()}
    arrays = [("Float64", k, v) for k, v in data.items()]
    if located is not None:
        arrays.append(("UInt8", "located", np.asarray(located).astype(np.uint8).reshape(n, 1)))
    decl, blob = [], bytearray()
    for typ, k, v in arrays:
        decl.append('<DataArray type="%s" Name="%s" NumberOfComponents="%d" format="appended" offset="%d"/>' % (typ, k, v.shape[1], len(blob)))
        raw = np.ascontiguousarray(v).tobytes()
        blob += struct.pack("<Q", len(raw)) + raw
    ext = "0 %d 0 %d 0 %d" % (dims[0] - 1, dims[1] - 1, dims[2] - 1)
    head = ('<?xml version="1.0"?>\n<VTKFile type="ImageData" version="1.0" byte_order="LittleEndian" header_type="UInt64">\n'
            '<ImageData WholeExtent="%s" Origin="%.17g %.17g %.17g" Spacing="%.17g %.17g %.17g">\n<Piece Extent="%s">\n'
            '<PointData>\n%s\n</PointData>\n</Piece>\n</ImageData>\n<AppendedData encoding="raw">\n_'
            % (ext, origin[0], origin[1], origin[2], spacing[0], spacing[1], spacing[2], ext, "\n".join(decl)))
    with open(path, "wb") as f:
        f.write(head.encode())
        f.write(bytes(blob))
        f.write(b"\n</AppendedData>\n</VTKFile>\n")


def read_vti(path):
    """Minimal reader of the files written above: dict(origin, spacing, dims, name -> array)."""
    raw = open(path, "rb").read()
    k = raw.index(b'<AppendedData encoding="raw">')
    head = raw[:k].decode()
    start = raw.index(b"_", k) + 1
    m = re.search(r'WholeExtent="0 (\d+) 0 (\d+) 0 (\d+)" Origin="([^"]*)" Spacing="([^"]*)"', head)
    out = {"dims": np.array([int(m.group(i)) + 1 for i in (1, 2, 3)]), "origin": np.array(m.group(4).split(), dtype=float),
           "spacing": np.array(m.group(5).split(), dtype=float)}
    for a in re.finditer(r'<DataArray type="(\w+)" Name="([^"]*)" NumberOfComponents="(\d+)" format="appended" offset="(\d+)"/>', head):
        typ, name, ncomp, off = a.group(1), a.group(2), int(a.group(3)), int(a.group(4))
        nbytes = struct.unpack_from("<Q", raw, start + off)[0]
        dt = {"Float64": np.float64, "UInt8": np.uint8}[typ]
        arr = np.frombuffer(raw, dtype=dt, count=nbytes // np.dtype(dt).itemsize, offset=start + off + 8)
        out[name] = arr.reshape(-1, ncomp) if ncomp > 1 else arr
        assert len(out[name]) == out["dims"].prod()
    return out


def write_npz(path, **arrays):
    """An npz archive of the given arrays (probes.npz: t, x, cell, u, p)."""
    np.savez(path, **{k: np.asarray(v) for k, v in arrays.items()})
