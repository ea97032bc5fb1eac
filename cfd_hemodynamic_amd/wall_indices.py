"""Cycle-averaged wall shear indices: the NumPy restatement of what `cfdh_wall_stats_get` forms on the device (include/cfdh.h),
the window test of the time loop, and the files `Scenario.solve(..., wall_indices=...)` writes.

With tau_k the wall shear stress after step k and w_k its weight (the step's dt), per vertex
    S = sum w_k tau_k,   A = sum w_k |tau_k|,   M = max_k |tau_k|,   W = sum w_k,
the indices are
    TAWSS = A / W,   OSI = (1 - |S| / A) / 2,   RRT = W / |S| = 1 / ((1 - 2 OSI) TAWSS),
the mean vector S / W and the peak M.  Away from the wall tau is zero: there TAWSS, OSI and RRT are 0."""
from __future__ import annotations

import os

import numpy as np

FIELDS = ("tawss", "osi", "rrt", "wss_mean", "wss_peak")


def indices_from_sums(S, A, M, W):
    """dict tawss, osi, rrt [nv], wss_mean [nv, gdim], wss_peak [nv] from the sums S [nv, gdim], A, M [nv] and the scalar W > 0.
    OSI is clamped to [0, 1/2] (rounding can push |S| / A past 1) and is 0 where A == 0; RRT is +inf where |S| == 0 < A and 0
    where A == 0."""
    S = np.asarray(S, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    W = float(W)
    if not W > 0.0:
        raise ValueError("the sum of the weights must be > 0")
    sn = np.sqrt((S * S).sum(axis=1))
    wall = A != 0.0
    a1 = np.where(wall, A, 1.0)
    osi = np.where(wall, np.clip(0.5 * (1.0 - sn / a1), 0.0, 0.5), 0.0)
    with np.errstate(divide="ignore"):
        rrt = np.where(wall, np.where(sn == 0.0, np.inf, W / np.where(sn == 0.0, 1.0, sn)), 0.0)
    return {"tawss": A / W, "osi": osi, "rrt": rrt, "wss_mean": S / W, "wss_peak": M.copy()}


def step_in_window(t_end, dt, window):
    """True when the step that ends at t_end counts for the window (t0, t1]: t0 < t_end <= t1 with a slack of 1e-6 dt on both
    comparisons (the time loop accumulates t += dt in floating point).  window True: every step."""
    if window is True:
        return True
    t0, t1 = window
    eps = 1e-6 * dt
    return bool(t_end > t0 + eps and t_end <= t1 + eps)


def summary_lines(ind, W, steps):
    """The lines of wall_indices.txt."""
    wall = ind["tawss"] > 0.0
    nw = int(wall.sum())
    tw, ow, rw = ind["tawss"][wall], ind["osi"][wall], ind["rrt"][wall]
    fin = rw[np.isfinite(rw)]
    return ["W (accumulated time): %.17g" % W,
            "steps: %d" % steps,
            "wall vertices: %d" % nw,
            "TAWSS max: %.17g" % (tw.max() if nw else 0.0),
            "TAWSS mean over wall vertices: %.17g" % (tw.mean() if nw else 0.0),
            "OSI max: %.17g" % (ow.max() if nw else 0.0),
            "RRT max (finite): %.17g" % (fin.max() if len(fin) else 0.0)]


def write_outputs(folder, mesh, ind, W, steps):
    """wall_indices.npz (x, cells of the vertex mesh, the five fields, W, steps), wall_indices.vtu (the fields as point data) and
    wall_indices.txt."""
    from .io import write_vtu
    np.savez(os.path.join(folder, "wall_indices.npz"), x=mesh.x, cells=mesh.cells, W=W, steps=steps, **{k: ind[k] for k in FIELDS})
    write_vtu(os.path.join(folder, "wall_indices.vtu"), mesh, {k: ind[k] for k in FIELDS})
    with open(os.path.join(folder, "wall_indices.txt"), "w") as f:
        f.write("\n".join(summary_lines(ind, W, steps)) + "\n")
