"""Meshes and boundary sets shared by the traction-boundary tests (tests/test_trac_twin.py, tests/test_gpu_traction.py,
tests/test_traction_host.py)  --  TEST INFRASTRUCTURE."""
import numpy as np

from cfd_hemodynamic_amd.mesh import Mesh, create_unit_square
from cfd_hemodynamic_amd.mesh3d import Mesh3D, _voxel_tets, create_unit_cube

INLET, OUTLET, WALL = 1, 2, 3


def mark_ends(mesh, corner=True):
    """Markers: INLET on the facets at the smallest x, OUTLET at the largest x, WALL elsewhere.  corner: one cell that has an
    OUTLET facet and a WALL facet gets the latter re-marked INLET, so that one cell carries two traction facets of two different
    boundaries and its vertices are shared by an inlet and an outlet facet."""
    fv = np.asarray(mesh.facet_vertices)
    xf = mesh.x[fv][..., 0]
    marker = np.full(len(fv), WALL, dtype=np.int32)
    marker[np.all(np.isclose(xf, mesh.x[:, 0].min()), axis=1)] = INLET
    marker[np.all(np.isclose(xf, mesh.x[:, 0].max()), axis=1)] = OUTLET
    if corner:
        out_cells = set(mesh.facet_cells[marker == OUTLET].tolist())
        k = [f for f in range(len(fv)) if marker[f] == WALL and int(mesh.facet_cells[f]) in out_cells]
        assert k, "no cell with an outlet facet and a wall facet"
        marker[k[0]] = INLET
    return marker


def sets_of(marker):
    return [np.nonzero(marker == m)[0] for m in (INLET, OUTLET, WALL)]


def wall_nodes(mesh, marker):
    return np.unique(np.asarray(mesh.facet_vertices)[marker == WALL]).astype(np.int32)


def square(nx, ny, seed=0):
    """nx x ny unit-square triangulation with the interior vertices moved at random."""
    m = create_unit_square(nx, ny)
    rng = np.random.default_rng(seed)
    interior = np.abs(m.x - 0.5).max(axis=1) < 0.49
    return Mesh(m.cells, m.x + (0.12 / max(nx, ny)) * rng.standard_normal(m.x.shape) * interior[:, None]), rng


def cube(n, seed=0):
    """The cube of tests/test_gpu_3d.py::_cube."""
    m = create_unit_cube(n)
    rng = np.random.default_rng(seed)
    interior = np.abs(m.x - 0.5).max(axis=1) < 0.49
    return Mesh3D(m.cells, m.x + (0.12 / n) * rng.standard_normal(m.x.shape) * interior[:, None]), rng


def channel(nx, ny, L, H=1.0):
    m = create_unit_square(nx, ny)
    return Mesh(m.cells, m.x * np.array([L, H]))


def duct(nx, n, L):
    """[0, L] x [0, 1]^2 with nx x n x n bricks of six Kuhn tetrahedra (the duct of tests/test_rot_twin3.py)."""
    xs, ys, zs = np.linspace(0.0, L, nx + 1), np.linspace(0.0, 1.0, n + 1), np.linspace(0.0, 1.0, n + 1)
    cells, pts = _voxel_tets(np.ones((nx, n, n), bool), xs, ys, zs)
    return Mesh3D(cells, pts, name="duct")
