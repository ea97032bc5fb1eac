#!/usr/bin/env python
"""What the cut-plane sections (`cfdh_section_*`) cost: the cut lists of 16 stations, the host time of building them, the
evaluation kernels, and what a user pays per step with `section_record` next to what that replaces, on one GPU, profiler off.

    python tools/section_measure.py [--cases stenosis115,bifurcation2e-4] [--steps 20] [--warmup 5] [--stations 16] [--out profiles/section_measure.json]

Per case one scenario is built (`stenosis` ny = 115 in mm / g / s, `simple_bifurcation` res = 2e-4 in SI units, both on
`stabilized_schur`, dt = 0.01) and run from rest, as in tools/sample_measure.py.  The stations are planes normal to the main axis
(x in the channel, y in the bifurcation, where the upper ones cross both daughters) at equal spacing between 5 % and 95 % of the
extent, offset so that they pass through no layer of vertices.  `section_set` is clocked on the host five times: it holds
cfdh_section::build_cut and the upload.  In the scenario's after-step hook, which runs after the flow step and before the state is
advanced, two things are clocked on the host, in alternating order from step to step: `section_record` (two launches, no
synchronisation, no copy), and what it replaces: `get_solution` (a copy of the whole field and a synchronisation) followed by the
NumPy evaluation of tests/section_twin.py on lists cut before the run -- the host cut is not counted.  The kernel time is that of
the device events the library records around its own launches (`cfdh_info` 125).  Medians with minimum and maximum.  The recorded
rows are compared with the host's, relative to the area times the bound of each integrand."""
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
ap.add_argument("--stations", type=int, default=16)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def _run(sim):
    import section_twin as T
    from cfd_hemodynamic_amd import _lib
    s = sim.solver
    ctx = s.ctx
    s.u_prev.x.array[:] = 0.0
    s.p_prev.x.array[:] = 0.0
    sim.early_stop_tolerance = 0
    d = sim.mesh.geometry.dim
    x = np.asarray(sim.mesh.x, dtype=float)[:, :d]
    cells = np.asarray(sim.mesh.cells)
    axis = 0 if d == 2 else 1
    lo, hi = x.min(axis=0), x.max(axis=0)
    K = args.stations
    at = lo[axis] + (hi[axis] - lo[axis]) * (0.05 + 0.9 * (np.arange(K) + 0.37) / K)
    origin = np.tile(0.5 * (lo + hi), (K, 1))
    origin[:, axis] = at
    normal = np.zeros((K, d))
    normal[:, axis] = 1.0

    t_set = []
    for _ in range(5):
        t0 = time.perf_counter()
        s.section_set((origin, normal, None))
        t_set.append(time.perf_counter() - t0)
    ptr, cell, meas, strad = s.section_cut()
    entry_bytes = 8 + 8 * (2 if d == 2 else 4) + 8 * (1 if d == 2 else 2)
    gather_bytes = 4 * (d + 1) + 8 * (d + 1) * (d + 1)
    t0 = time.perf_counter()
    twin = [T.cut(x, cells, origin[k], normal[k]) for k in range(K)]
    t_twin_cut = time.perf_counter() - t0
    assert all(np.array_equal(cell[ptr[k]:ptr[k + 1]], twin[k].cells) for k in range(K))
    rho = 1.06e-3 if d == 2 else 1.0  # the densities the two scenarios hand to their solver (stenosis: g / mm^3; bifurcation: scaled)
    ctx.section_series_enable(args.warmup + args.steps)
    rec = {"record_host": [], "replaced_host": [], "replaced_copy": [], "kernel": [], "rows": [], "bound": []}

    def record(t):
        t0 = time.perf_counter()
        s.section_record(t)
        rec["record_host"].append(time.perf_counter() - t0)

    def replaced(t):
        t0 = time.perf_counter()
        u, p = ctx.get_solution()
        t1 = time.perf_counter()
        u, p = np.asarray(u).reshape(-1, d), np.asarray(p)
        rec["rows"].append(np.stack([T.rows(sec, cells, u, p, rho) for sec in twin]))
        U, P = float(np.linalg.norm(u, axis=1).max()), float(np.abs(p).max())
        rec["bound"].append(np.array([1.0, U, P, U * U, U * U, P * U, 0.5 * rho * U ** 3, U, U, U]))
        rec["replaced_host"].append(time.perf_counter() - t0)
        rec["replaced_copy"].append(t1 - t0)

    def after(t):
        for fn in ((record, replaced) if len(rec["kernel"]) % 2 == 0 else (replaced, record)):
            fn(t)
        rec["kernel"].append(ctx.info(_lib.INFO_SECTION_KERNEL_NS) * 1e-6)

    sim.solve(None, max_steps=args.warmup + args.steps, write_every=0, afterStepCallback=after)
    flow = 1e3 * np.array([dt for dt, _ in sim.step_stats[args.warmup:]])
    w = args.warmup
    t0 = time.perf_counter()
    t, rows = s.section_series()
    t_series = time.perf_counter() - t0
    host = np.stack(rec["rows"])
    # against the magnitude of the integrals: the area times the bound of each integrand (max |u|, max |p| of the step)
    scale = host[:, :, :1] * np.stack(rec["bound"])[:, None, :]
    diff = float((np.abs(rows - host) / np.where(scale > 0, scale, 1.0)).max())
    s.section_set([])
    return {"flow_ms_per_step": _stat(flow), "stations": K, "axis": "xyz"[axis], "entries": int(ptr[-1]), "longest_list": int(np.diff(ptr).max()),
            "shortest_list": int(np.diff(ptr).min()), "straddling": int(strad.sum()), "bytes_per_entry": entry_bytes,
            "gathered_bytes_per_entry": gather_bytes, "area_first_last": [float(meas[ptr[0]:ptr[1]].sum()), float(meas[ptr[-2]:ptr[-1]].sum())],
            "section_set_host_ms": _stat(t_set, 1e3), "twin_cut_host_ms": 1e3 * t_twin_cut,
            "eval_kernels_ms": _stat(rec["kernel"][w:]), "record_host_ms_per_step": _stat(rec["record_host"][w:], 1e3),
            "get_solution_plus_numpy_host_ms_per_step": _stat(rec["replaced_host"][w:], 1e3),
            "get_solution_alone_host_ms_per_step": _stat(rec["replaced_copy"][w:], 1e3), "series_download_ms": 1e3 * t_series,
            "device_against_host_rows_largest_difference_over_magnitude": diff}


def main():
    res = {"steps": args.steps, "warmup": args.warmup, "gpus": 1}
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
