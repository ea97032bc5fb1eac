#!/usr/bin/env python
"""What the point sampler (`cfdh_sample_*`) costs: the bin grid, the locate kernel for 1e3 probes and for a voxel grid of about
1.6e7 nodes over the bounding box, the sample kernel on both sets, and what a user pays per step for 1e3 probes with
`sample_record` next to what that replaces, on one GPU, profiler off.

    python tools/sample_measure.py [--cases stenosis115,bifurcation2e-4] [--steps 20] [--warmup 5] [--grid_nodes 1.6e7] [--out profiles/sample_measure.json]

Per case one scenario is built (`stenosis` ny = 115 in mm / g / s, `simple_bifurcation` res = 2e-4 in SI units, both on
`stabilized_schur`, dt = 0.01) and run from rest, as in tools/flow_measure.py.  The probes are 1e3 points in random cells.  In the
scenario's after-step hook, which runs after the flow step and before the state is advanced, two things are clocked on the host, in
alternating order from step to step: `sample_record` (one launch, no synchronisation, no copy), and what it replaces:
`get_solution` (a copy of the whole field and a synchronisation) followed by lambda . values in NumPy at the cells and
coordinates already known -- the cheapest host evaluation there is; the host locate is not counted.  The kernel times are those of
the device events the library records around its own launches (`cfdh_info` 115: locate, 116: sample).  After the run, with the last
state still on the device, the voxel grid is set three times (the locate time) and sampled into the series buffer and into the means
three times each.  Medians with minimum and maximum.

Next to each sample-kernel time: its algorithmic bytes -- per point the cell and the output row, per located point its coordinates
and vertex ids, and every vertex value once -- and the time those bytes take at 5.9 TB/s, the rate the project's SpMV reaches
(README).  The ratio is reported, nothing is gated on it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="stenosis115,bifurcation2e-4")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--probes", type=int, default=1000)
ap.add_argument("--grid_nodes", type=float, default=1.6e7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_RATE = 5.9e12  # B/s


def _scenario(case):
    if case.startswith("stenosis"):
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        return StenosisSimulation("stabilized_schur", 0.01, 1.0, grade="moderate", ny=int(case[8:] or 115), v_max=100.0, quiet=True)
    if case.startswith("bifurcation"):
        from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
        return MicrovasculatureSimulation("stabilized_schur", 0.01, 1.0, v_inlet=1.5, res=float(case[11:] or 2e-4), quiet=True,
                                          options=dict(remove_p_mean=0))
    raise SystemExit("unknown case " + case)


def _stat(v, scale=1.0):
    v = scale * np.asarray(v, dtype=float)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def _sample_bytes(n, located, nv, d):
    values = min(located * (d + 1), nv) * 8 * (d + 1)
    return int(4 * n + located * 12 * (d + 1) + values + 8 * (d + 1) * n)


def _kernel(ms, nbytes):
    ideal = 1e3 * nbytes / HBM_RATE
    return dict(_stat(ms), algorithmic_bytes=nbytes, **{"ms_at_5.9_TB_per_s": ideal, "measured_over_ideal": float(np.median(ms)) / ideal})


def _run(sim):
    from cfd_hemodynamic_amd import _lib
    s = sim.solver
    ctx = s.ctx
    s.u_prev.x.array[:] = 0.0
    s.p_prev.x.array[:] = 0.0
    sim.early_stop_tolerance = 0
    d = sim.mesh.geometry.dim
    x = np.asarray(sim.mesh.x, dtype=float)[:, :d]
    cells = np.asarray(sim.mesh.cells)
    nv, nc = len(x), len(cells)
    rng = np.random.default_rng(0)
    lam0 = rng.dirichlet(np.ones(d + 1), size=args.probes)
    pts = np.einsum("ka,kai->ki", lam0, x[cells[rng.choice(nc, size=args.probes)]])

    def ms(what):
        return ctx.info(what) * 1e-6

    locate_probes = []
    for _ in range(5):
        s.sample_set_points(pts)
        locate_probes.append(ms(_lib.INFO_SAMPLE_LOCATE_NS))
    box = x[cells]
    first_edge = float(np.sort((box.max(axis=1) - box.min(axis=1)).max(axis=1))[nc // 2])  # the median the builder starts from
    bins = {"edge": first_edge * 2.0 ** ctx.info(_lib.INFO_SAMPLE_BIN_DOUBLINGS), "doublings": ctx.info(_lib.INFO_SAMPLE_BIN_DOUBLINGS), "total": ctx.info(_lib.INFO_SAMPLE_BIN_TOTAL),
            "total_over_cells": ctx.info(_lib.INFO_SAMPLE_BIN_TOTAL) / nc, "longest": ctx.info(_lib.INFO_SAMPLE_BIN_LONGEST)}
    cell, lam, _ = s.sample_location()
    located = int((cell >= 0).sum())
    ctx.sample_series_enable(args.warmup + args.steps)
    rec = {"record_host": [], "replaced_host": [], "replaced_copy": [], "kernel": []}

    def record(t):
        t0 = time.perf_counter()
        s.sample_record(t)
        rec["record_host"].append(time.perf_counter() - t0)

    def replaced(t):
        t0 = time.perf_counter()
        u, p = ctx.get_solution()
        t1 = time.perf_counter()
        k = np.maximum(cell, 0)
        np.einsum("na,nai->ni", lam, np.asarray(u).reshape(-1, d)[cells[k]])
        np.einsum("na,na->n", lam, np.asarray(p)[cells[k]])
        rec["replaced_host"].append(time.perf_counter() - t0)
        rec["replaced_copy"].append(t1 - t0)

    def after(t):
        for fn in ((record, replaced) if len(rec["kernel"]) % 2 == 0 else (replaced, record)):
            fn(t)
        rec["kernel"].append(ms(_lib.INFO_SAMPLE_KERNEL_NS))

    sim.solve(None, max_steps=args.warmup + args.steps, write_every=0, afterStepCallback=after)
    flow = 1e3 * np.array([dt for dt, _ in sim.step_stats[args.warmup:]])
    w = args.warmup
    probes = {"points": args.probes, "located": located, "locate_ms": _stat(locate_probes),
              "sample_kernel_ms": _kernel(rec["kernel"][w:], _sample_bytes(args.probes, located, nv, d)),
              "record_host_ms_per_step": _stat(rec["record_host"][w:], 1e3),
              "get_solution_plus_numpy_host_ms_per_step": _stat(rec["replaced_host"][w:], 1e3),
              "get_solution_alone_host_ms_per_step": _stat(rec["replaced_copy"][w:], 1e3)}
    t0 = time.perf_counter()
    s.sample_series()
    probes["series_download_ms"] = 1e3 * (time.perf_counter() - t0)

    # the voxel grid over the bounding box, on the state of the last step
    lo, hi = x.min(axis=0), x.max(axis=0)
    h = float((np.prod(hi - lo) / args.grid_nodes) ** (1.0 / d))
    from cfd_hemodynamic_amd.sampling import grid_over
    origin, spacing, dims = grid_over(sim.mesh, spacing=h)
    n = int(dims.prod())
    locate_grid, t_set = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        s.sample_set_grid(origin, spacing, dims)
        t_set.append(time.perf_counter() - t0)
        locate_grid.append(ms(_lib.INFO_SAMPLE_LOCATE_NS))
    located = ctx.info(_lib.INFO_SAMPLE_LOCATED)
    ctx.sample_series_enable(3)
    s.sample_mean_reset()
    k_rec, k_acc = [], []
    for k in range(3):
        s.sample_record(float(k))
        k_rec.append(ms(_lib.INFO_SAMPLE_KERNEL_NS))
        s.sample_mean_accumulate(sim.dt)
        k_acc.append(ms(_lib.INFO_SAMPLE_KERNEL_NS))
    nb = _sample_bytes(n, located, nv, d)
    grid = {"nodes": n, "dims": [int(v) for v in dims], "spacing": h, "located": int(located), "located_share": located / n,
            "idle_lane_share_of_the_sample_kernel": 1.0 - located / n, "locate_ms": _stat(locate_grid),
            "set_grid_host_ms": _stat(t_set, 1e3), "locate_ns_per_node": 1e6 * float(np.median(locate_grid)) / n,
            "sample_kernel_ms": _kernel(k_rec, nb),
            "accumulate_kernel_ms": _kernel(k_acc, nb - 8 * (d + 1) * n + 2 * 8 * (d + 2) * located)}
    s.sample_set_points(np.zeros((0, d)))  # frees the buffers
    return {"flow_ms_per_step": _stat(flow), "bins": bins, "probes": probes, "grid": grid}


def main():
    res = {"steps": args.steps, "warmup": args.warmup, "gpus": 1, "hbm_rate_bytes_per_s": HBM_RATE}
    for case in args.cases.split(","):
        sim = _scenario(case)
        sim.setup()
        sizes = {"vertices": sim.mesh.num_vertices, "cells": len(sim.mesh.cells), "gdim": sim.mesh.geometry.dim}
        res[case] = dict(sizes, **_run(sim))
        print(case, json.dumps(res[case]), flush=True)
        del sim
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
