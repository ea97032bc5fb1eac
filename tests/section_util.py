"""Planes, expected areas, analytic polygons and fields shared by test_section_twin.py (CPU) and test_gpu_section.py (GPU).  The
meshes are those of sample_util.py: "square" lid_case(8), "cube" create_unit_cube(4), "stenosis" stenosis_case(6), "bifurcation"
create_bifurcation(1.2e-3).  Everything is built once and left unchanged.

A case is a dict: origin, normal, radius (None: unbounded), and where they are known area (closed form) and polygon (the cut as
a convex polygon [k, 3] or a segment [2, 2], known analytically, for the closed forms of affine fields)."""
import numpy as np

import sample_util as SU
import section_twin as T

TOL_EXACT = 1e-12   # closed forms, lists and measures: of the scale (the sampler's tolerance for the same kind of check)
TOL_TWIN = 1e-11    # device gather against a twin that takes another route
TOL_FLIP = 1e-13    # opposite normals
TOL_MEAN = 1e-13    # means against NumPy on the rows
RHO = 1.06
MESHES = ("square", "cube", "stenosis", "bifurcation")
mesh = SU.mesh
cached = SU.cached
S2, S3 = np.sqrt(2.0), np.sqrt(3.0)


def case(origin, normal, radius=None, area=None, polygon=None):
    return dict(origin=np.array(origin, dtype=float), normal=np.array(normal, dtype=float), radius=radius, area=area,
                polygon=None if polygon is None else np.array(polygon, dtype=float))


# the planes of the issue on create_unit_cube(4); the hexagon of (1, 1, 1) through the centre has its corners on the edge midpoints
CUBE = {
    "x037": case([0.37, 0.5, 0.5], [1, 0, 0], area=1.0, polygon=[[0.37, 0, 0], [0.37, 1, 0], [0.37, 1, 1], [0.37, 0, 1]]),
    "x05_facets": case([0.5, 0.2, 0.3], [3, 0, 0], area=1.0, polygon=[[0.5, 0, 0], [0.5, 1, 0], [0.5, 1, 1], [0.5, 0, 1]]),
    "x1_outward": case([1.0, 0.5, 0.5], [1, 0, 0], area=1.0, polygon=[[1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 1]]),
    "x0_inward": case([0.0, 0.5, 0.5], [1, 0, 0], area=0.0),
    "diag110": case([0.5, 0.5, 0.5], [1, 1, 0], area=S2, polygon=[[1, 0, 0], [0, 1, 0], [0, 1, 1], [1, 0, 1]]),
    "diag111": case([0.5, 0.5, 0.5], [1, 1, 1], area=3 * S3 / 4,
                    polygon=[[1, 0.5, 0], [0.5, 1, 0], [0, 1, 0.5], [0, 0.5, 1], [0.5, 0, 1], [1, 0, 0.5]]),
    "y061_down": case([0.1, 0.61, 0.9], [0, -2, 0], area=1.0, polygon=[[0, 0.61, 0], [1, 0.61, 0], [1, 0.61, 1], [0, 0.61, 1]]),
    "outside": case([1.5, 0.5, 0.5], [1, 0, 0], area=0.0),
}
# ... and the same kinds of lines on lid_case(8): x = 0.5 runs through a row of vertices, the diagonal through the corners
SQUARE = {
    "x037": case([0.37, 0.5], [1, 0], area=1.0, polygon=[[0.37, 0], [0.37, 1]]),
    "x05_vertices": case([0.5, 0.1], [2, 0], area=1.0, polygon=[[0.5, 0], [0.5, 1]]),
    "x1_outward": case([1.0, 0.5], [1, 0], area=1.0, polygon=[[1, 0], [1, 1]]),
    "x0_inward": case([0.0, 0.5], [1, 0], area=0.0),
    "diag11": case([0.5, 0.5], [1, 1], area=S2, polygon=[[1, 0], [0, 1]]),
    "diag1m1": case([0.5, 0.5], [1, -1], area=S2, polygon=[[0, 0], [1, 1]]),
    "y061_down": case([0.3, 0.61], [0, -1], area=1.0, polygon=[[0, 0.61], [1, 0.61]]),
    "outside": case([0.5, -0.25], [0, 1], area=0.0),
}
# stations across the stenosed channel (inlet x = 0, outlet x = 20, throat in the middle); the last has a ball that keeps the lower
# part of the channel only and cuts through cells: straddling > 0, reported and not refused
STENOSIS = {
    "proximal": case([2.0, 1.57], [1, 0]),
    "throat": case([10.0, 1.57], [1, 0]),
    "distal": case([18.0, 1.57], [1, 0]),
    "oblique": case([6.0, 1.57], [2, 1]),
    "inlet_outward": case([0.0, 1.57], [-1, 0]),
    "bad_ball": case([10.0, 1.2], [1, 0], radius=0.3),
}
# the bifurcation: parent along +y from y = 0, daughters leave at y = 0.0312 around x = -+0.0106.  One plane crosses both daughters;
# with a ball around the centre of each daughter's cut it selects one.  The centres and the radius come from the twin's unbounded
# cut (bifurcation_cases), and test_section_twin.py asserts straddling == 0 for them before the GPU tests use them.
Y_DAUGHTERS, Y_PARENT = 0.025, 0.006


def bifurcation_cases():
    def make():
        m = mesh("bifurcation")
        both = case([0.0, Y_DAUGHTERS, 0.0], [0, 1, 0])
        sec = twin_cut(m, both)
        P = np.einsum("sma,sac->smc", sec.sub_bary, m.x[m.cells[sec.sub_cell]]).reshape(-1, 3)
        left, right = P[P[:, 0] < 0.0], P[P[:, 0] > 0.0]
        assert len(left) and len(right) and len(left) + len(right) == len(P)
        out = {"parent": case([0.0, Y_PARENT, 0.0], [0, 1, 0]), "both": both}
        for name, Q in (("left", left), ("right", right)):
            c = 0.5 * (Q.min(axis=0) + Q.max(axis=0))
            c[1] = Y_DAUGHTERS
            reach = np.sqrt(((Q - c) ** 2).sum(axis=1).max())
            gap = np.sqrt((((right if name == "left" else left) - c) ** 2).sum(axis=1).min())
            assert gap > 1.5 * reach
            out[name] = case(c, [0, 1, 0], radius=0.5 * (reach + gap))
        out["lengthwise"] = case([0.0, 0.015, 0.0003], [0, 0, 1])  # along the vessels: more entries than five blocks of 256 hold
        out["left_oblique"] = case(out["left"]["origin"], [-0.3, 1, 0.1], radius=out["left"]["radius"])
        out["bad_ball"] = case(out["right"]["origin"], [0, 1, 0], radius=0.4 * np.sqrt(((right - out["right"]["origin"]) ** 2).sum(axis=1).max()))
        return out
    return cached(("section cases", "bifurcation"), make)


def cases(name):
    return {"cube": CUBE, "square": SQUARE, "stenosis": STENOSIS}[name] if name != "bifurcation" else bifurcation_cases()


def arrays(cs):
    """(origin [K, d], normal [K, d], radius [K]) of a list of cases."""
    return (np.array([c["origin"] for c in cs]), np.array([c["normal"] for c in cs]), np.array([c["radius"] or 0.0 for c in cs]))


def twin_cut(m, c):
    return T.cut(m.x, m.cells, c["origin"], c["normal"], c["radius"])


def twin_cuts(name):
    """name -> the twin's cut of every case of the mesh, computed once."""
    return cached(("section twin", name), lambda: {k: twin_cut(mesh(name), c) for k, c in cases(name).items()})


# ----------------------------------------------------------------------------------------------------------------------- fields
def affine_state(m):
    """Nodal (u, p) of u = M x + b, p = c . x + e, and (ufun, pfun) of points."""
    A, b, c = SU.A_FULL[:m.d, :m.d], SU.B_FULL[:m.d], SU.C_FULL[:m.d]
    return m.x @ A.T + b, m.x @ c + SU.E_FULL, (lambda x: x @ A.T + b), (lambda x: x @ c + SU.E_FULL)


def random_state(name, seed=0):
    return SU.random_state(name, seed)


def row_scale(row_or_area, u, p, rho=RHO):
    """The magnitude of every slot for fields bounded by U = max |u|, P = max |p| over an area A: the bound of the integrand times A."""
    A = float(np.asarray(row_or_area).reshape(-1)[0])
    U, P = float(np.linalg.norm(u, axis=1).max()), float(np.abs(p).max())
    return A * np.array([1.0, U, P, U * U, U * U, P * U, 0.5 * rho * U ** 3, U, U, U])


def worst(what, got, want, bound):
    got, want, bound = np.asarray(got, dtype=float), np.asarray(want, dtype=float), np.asarray(bound, dtype=float)
    err = np.abs(got - want)
    rel = float((err / np.where(bound > 0, bound, 1.0)).max()) if err.size else 0.0
    print("%-28s worst err / bound %.3e" % (what, rel))
    return bool((err <= bound).all())
