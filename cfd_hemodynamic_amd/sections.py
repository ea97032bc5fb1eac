"""Cut-plane sections (cfdh_section_*): helpers that describe the planes, derive the clinical numbers from the rows and write them.

A row has ten slots (cfd_hemodynamic_amd._lib.SECTION_*): A, Q = int u.n, int p, int (u.n)^2, int |u|^2, int p u.n,
int rho/2 |u|^2 u.n, int u_x, int u_y, int u_z over the exact intersection of the plane with the mesh."""
import numpy as np

NQ = 10
NAMES = ("area", "flow", "int_p", "int_un2", "int_u2", "int_p_un", "kinetic_flux", "int_ux", "int_uy", "int_uz")


def plane(origin, normal, radius=None):
    """One section: the plane (2-D: the line) through `origin` with normal `normal` (any non-zero length).  `radius` (None or
    <= 0: unbounded) keeps the cut polygons whose centre lies within that distance of the origin."""
    o, n = np.asarray(origin, dtype=float).reshape(-1), np.asarray(normal, dtype=float).reshape(-1)
    if o.shape != n.shape or len(o) not in (2, 3):
        raise ValueError("plane: origin and normal need the same 2 or 3 components")
    if not (np.isfinite(o).all() and np.isfinite(n).all()) or not (n != 0.0).any():
        raise ValueError("plane: origin and normal must be finite and the normal non-zero")
    r = 0.0 if radius is None else float(radius)
    if not np.isfinite(r):
        raise ValueError("plane: the radius must be finite")
    return {"origin": o, "normal": n, "radius": r}


def stations(polyline, n, radius=None):
    """n planes normal to the centreline `polyline` [m, gdim] (m >= 2), at equal arc length from its first to its last point
    (n = 1: the middle).  The normal is the direction of the segment the station lies on."""
    P = np.asarray(polyline, dtype=float)
    if P.ndim != 2 or len(P) < 2 or P.shape[1] not in (2, 3) or int(n) < 1:
        raise ValueError("stations: a polyline [m >= 2, gdim] and n >= 1")
    seg = np.diff(P, axis=0)
    length = np.linalg.norm(seg, axis=1)
    if not (length > 0.0).all():
        raise ValueError("stations: the polyline repeats a point")
    s = np.concatenate([[0.0], np.cumsum(length)])
    at = np.array([0.5 * s[-1]]) if int(n) == 1 else np.linspace(0.0, s[-1], int(n))
    out = []
    for a in at:
        k = min(int(np.searchsorted(s, a, side="right")) - 1, len(seg) - 1)
        out.append(plane(P[k] + (a - s[k]) / length[k] * seg[k], seg[k] / length[k], radius))
    return out


def as_arrays(planes):
    """(origin [K, gdim], normal [K, gdim], radius [K]) of a list of plane() entries, or of such a triple."""
    if isinstance(planes, tuple) and len(planes) == 3 and not isinstance(planes[0], dict):
        o, n = np.atleast_2d(np.asarray(planes[0], dtype=float)), np.atleast_2d(np.asarray(planes[1], dtype=float))
        r = np.zeros(len(o)) if planes[2] is None else np.asarray(planes[2], dtype=float).reshape(-1)
        return o, n, r
    planes = list(planes)
    if not planes:
        return np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0)
    if not all(isinstance(p, dict) and {"origin", "normal"} <= set(p) for p in planes):
        raise ValueError("sections: a list of sections.plane(...) entries")
    return (np.array([p["origin"] for p in planes], dtype=float), np.array([p["normal"] for p in planes], dtype=float),
            np.array([p.get("radius") or 0.0 for p in planes], dtype=float))


def _ratio(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=(b != 0.0))
    return out


def derive(rows, rho=None, reference=0):
    """The numbers one reads off a section, from rows [..., K, 10]: area, flow, mean_pressure (int p / A), mean_velocity
    (int u / A, [..., K, 3]), mean_normal_velocity (Q / A), momentum_factor (A int (u.n)^2 / Q^2), energy_flux (int p u.n +
    int rho/2 |u|^2 u.n), flow_split (Q / Q of section `reference`) and pressure_ratio (mean pressure / that of `reference`: the
    FFR when `reference` is the proximal station).  nan where A or Q is 0.  rho is not needed: the rows carry it in slot 6."""
    rows = np.asarray(rows, dtype=float)
    if rows.shape[-1] != NQ:
        raise ValueError("derive: rows [..., K, %d]" % NQ)
    A, Q = rows[..., 0], rows[..., 1]
    pm = _ratio(rows[..., 2], A)
    return {"area": A, "flow": Q, "mean_pressure": pm, "mean_velocity": _ratio(rows[..., 7:10], A[..., None]),
            "mean_normal_velocity": _ratio(Q, A), "momentum_factor": _ratio(A * rows[..., 3], Q * Q),
            "energy_flux": rows[..., 5] + rows[..., 6], "flow_split": _ratio(Q, Q[..., reference:reference + 1]),
            "pressure_ratio": _ratio(pm, pm[..., reference:reference + 1])}


def write_npz(path, **arrays):
    np.savez(path, **{k: np.asarray(v) for k, v in arrays.items() if v is not None})


def write_txt(path, t, rows, origin, normal, radius, straddling=None):
    """One block per section: its plane, then one line per record with t and the ten slots."""
    t, rows = np.asarray(t, dtype=float), np.asarray(rows, dtype=float)
    with open(path, "w") as f:
        for k in range(rows.shape[1] if rows.ndim == 3 else len(origin)):
            f.write("# section %d: origin %s normal %s radius %.9g%s\n" % (
                k, " ".join("%.9g" % v for v in origin[k]), " ".join("%.9g" % v for v in normal[k]), radius[k],
                "" if straddling is None else " straddling %d" % straddling[k]))
            f.write("# t " + " ".join(NAMES) + "\n")
            for i in range(len(t)):
                f.write("%.9g " % t[i] + " ".join("%.12e" % v for v in rows[i, k]) + "\n")
            f.write("\n")
