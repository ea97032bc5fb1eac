"""Meshes and set-ups shared by the tests of the backflow-stabilised rotational form (tests/test_rot_backflow_twin.py on the CPU,
tests/test_gpu_rot_backflow.py on the GPU)."""
import numpy as np

from cfd_hemodynamic_amd.elements import NodeMesh, create_rectangle
from cfd_hemodynamic_amd.mesh import create_unit_square
from gen_util import ETYPE, facet_node_set
from gen3_util import ETYPE3, facet_node_set3
from oracle import np_twin as T, np_twin_nd as TN
import rot_backflow_twin as BT
from test_rot_twin3 import duct, ends3

DISTORT = 0.05
SCHEMES = {"midpoint": dict(), "bdf2": dict(theta=1.0, a0=1.5, a1=-2.0, a2=0.5)}
KINDS = [(2, "P1"), (2, "P2"), (2, "Q1"), (3, "P2"), (3, "Q1")]
IDS = ["%dd-%s" % k for k in KINDS]


def channel(kind, nx=4, ny=2, distort=DISTORT):
    """[0, 2] x [0, 1] with nx x ny distorted cells: sheared rectangles (Q1) or a triangulation bent along y (P1 / P2)."""
    if kind == "Q1":
        m = create_rectangle((0.0, 0.0), (2.0, 1.0), (nx, ny))
        m.x[:, 0] += distort * m.x[:, 1]
        return m
    m = create_unit_square(nx, ny)
    m.x[:, 0] *= 2.0
    m.x[:, 0] += distort * np.sin(3.0 * m.x[:, 1])
    return m if kind == "P1" else NodeMesh(m)


def channel_ends(m, kind, distort=DISTORT):
    """Left / right ends and the wall facets of channel(), from the undistorted end vertices of each facet."""
    x = m.x[np.asarray(m.facet_vertices)[:, :2]]
    x0 = x[..., 0] - distort * (x[..., 1] if kind == "Q1" else np.sin(3.0 * x[..., 1]))
    left = np.nonzero(np.all(np.isclose(x0, x0.min()), axis=1))[0]
    right = np.nonzero(np.all(np.isclose(x0, x0.max()), axis=1))[0]
    return left, right, np.setdiff1d(np.arange(m.num_facets), np.concatenate([left, right]))


def small_mesh(dim, kind):
    """The 4 x 2 channel of distorted cells (2-D) or the 2 x 2 x 2 duct (3-D) with its (left, right, walls) facet sets."""
    if dim == 2:
        m = channel(kind)
        return m, channel_ends(m, kind)
    m = duct(kind, 2, 2, 1.0)
    return m, ends3(m)


def params(dim, dt=0.02, rho=1.3, mu=0.04, scheme="midpoint", f=(0.2, -0.1, 0.3)):
    return (T if dim == 2 else TN).Params(dt, rho, mu, tuple(f)[:dim], **SCHEMES[scheme])


def twin(dim, kind, m, prm):
    cls, et = (BT.Problem, ETYPE[kind]) if dim == 2 else (BT.Problem3, ETYPE3[kind])
    return cls(et, m.x, m.cells, m.facet_cells, m.facet_local, prm)


def wall_nodes(dim, m, walls):
    return (facet_node_set if dim == 2 else facet_node_set3)(m, walls)


def random_state(dim, nv, seed):
    """x = (u, p), u_prev, u_prev2 of a seeded generator."""
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal((dim + 1) * nv), 0.3 * rng.standard_normal((nv, dim)), 0.3 * rng.standard_normal((nv, dim)))


def sign_pattern(sn):
    """(some point < 0, some point > 0, some single facet with both) of u_prev . n at the outlet points [facet, point]."""
    return bool((sn < 0).any()), bool((sn > 0).any()), bool(((sn < 0).any(axis=1) & (sn > 0).any(axis=1)).any())
