#!/usr/bin/env python
"""What the volumetric flow diagnostics cost next to the flow step: device time of the cell-gradient pass, of the vertex kernel of
every field, of `cfdh_flow_integrals` and of `cfdh_flow_stats_accumulate`, beside the flow step's ms/step on the same run, on one GPU,
profiler off.

    python tools/flow_measure.py [--cases stenosis115,bifurcation2e-4] [--steps 20] [--warmup 5] [--out profiles/flow_measure.json]

Per case one scenario is built (`stenosis` ny = 115 in mm / g / s, `simple_bifurcation` res = 2e-4 in SI units, both on
`stabilized_schur`, dt = 0.01) and run from rest.  In the scenario's after-step hook, which runs after the flow step and before the
state is advanced, every entry point is called once; the kernel times are those of the device events the library records around its
own launches (`cfdh_info` 109: the cell pass, 110: the kernel behind it), the flow step's time is the host clock around
`solveStep()` (`Scenario.step_stats`; the step ends in a read-back).  Medians over the steps after the warm-up.

Next to each time: the kernel's algorithmic bytes -- every operand once, the contribution rows and the vertex values counted once
however many lanes gather them, the index with its padding -- and the time those bytes take at 5.9 TB/s, the rate the project's
SpMV reaches (README).  The ratio is reported, nothing is gated on it."""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="stenosis115,bifurcation2e-4")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
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


def _bytes(mesh):
    """Algorithmic bytes of every kernel."""
    cells = np.asarray(mesh.cells)
    nc, n1 = cells.shape
    d, nv = n1 - 1, mesh.num_vertices
    valence = np.bincount(cells.ravel(), minlength=nv)
    pad = np.zeros(-(-nv // 64) * 64, dtype=np.int64)
    pad[:nv] = valence
    slots = int(pad.reshape(-1, 64).max(axis=1).sum()) * 64       # entries of the sliced index, padding included
    rows = 8 * (d * d + 1) * nc                                   # the contribution rows, once
    mesh_read = 4 * n1 * nc + 2 * 8 * d * nv                      # vertex ids, coordinates, velocities
    index = 4 * slots + 4 * (len(pad) // 64 + 1)
    width = {"gradient": d * d, "vorticity": 1 if d == 2 else 3, "q_criterion": 1, "shear_rate": 1, "dissipation": 1, "helicity": 1, "lnh": 1}
    out = {"cell_pass": mesh_read + rows, "integrals": mesh_read, "accumulate": index + rows + 8 * d * nv + 2 * 8 * (d + 4) * nv}
    for k, w in width.items():
        if d == 3 or k not in ("helicity", "lnh"):
            out[k] = index + rows + 8 * w * nv + (8 * d * nv if k in ("helicity", "lnh") else 0)
    return out, {"valence_median": float(np.median(valence)), "valence_max": int(valence.max()), "index_entries": slots,
                 "incidences": int(valence.sum())}


def _run(sim):
    from cfd_hemodynamic_amd import _lib
    s = sim.solver
    ctx = s.ctx
    s.u_prev.x.array[:] = 0.0
    s.p_prev.x.array[:] = 0.0
    sim.early_stop_tolerance = 0
    nbytes, index = _bytes(sim.mesh)
    fields = [k for k in _lib.FLOW_FIELDS if k in nbytes]
    rec = {k: [] for k in ["cell_pass", "integrals", "accumulate"] + fields}
    s.flow_stats_reset()

    def ns(what):
        return ctx.info(what) * 1e-6  # ms

    def after(t):
        for k in fields:
            s.flow_field(k)
            rec[k].append(ns(_lib.INFO_FLOW_KERNEL_NS))
        rec["cell_pass"].append(ns(_lib.INFO_FLOW_CELL_PASS_NS))
        s.flow_integrals()
        rec["integrals"].append(ns(_lib.INFO_FLOW_KERNEL_NS))
        s.flow_stats_accumulate(sim.dt)
        rec["accumulate"].append(ns(_lib.INFO_FLOW_KERNEL_NS))

    sim.solve(None, max_steps=args.warmup + args.steps, write_every=0, afterStepCallback=after)
    flow = 1e3 * np.array([dt for dt, _ in sim.step_stats[args.warmup:]])
    flow_med = float(np.median(flow))
    kernels = {}
    for k, v in rec.items():
        v = np.array(v[args.warmup:])
        ms, ideal = float(np.median(v)), 1e3 * nbytes[k] / HBM_RATE
        kernels[k] = {"ms_median": ms, "ms_min": float(v.min()), "ms_max": float(v.max()), "algorithmic_bytes": int(nbytes[k]),
                      "ms_at_5.9_TB_per_s": ideal, "measured_over_ideal": ms / ideal, "percent_of_flow_step": 100.0 * ms / flow_med}
    integrals = s.flow_integrals()
    return {"flow_ms_per_step_median": flow_med, "flow_ms_min": float(flow.min()), "flow_ms_max": float(flow.max()), "index": index,
            "kernels": kernels, "integrals_last_step": [float(v) for v in integrals], "cell_passes": int(ctx.info(_lib.INFO_FLOW_CELL_PASSES))}


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
