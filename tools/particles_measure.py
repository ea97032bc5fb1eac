#!/usr/bin/env python
"""What the particle tracker costs next to the flow step: the advection kernel's ms per step (device events) for 1e5 and 1e6
particles, beside the flow step's ms/step on the same run, on one GPU, profiler off.

    python tools/particles_measure.py [--cases stenosis115,bifurcation2e-4] [--counts 100000,1000000] [--nsub 2,8] [--steps 20] [--warmup 5]
                                      [--out profiles/particles_measure.json]

Per case one scenario is built (`stenosis` ny = 115 in mm / g / s, `simple_bifurcation` res = 2e-4 in SI units, both on
`stabilized_schur`, dt = 0.01) and run from rest once per particle count.  The particles are seeded uniformly over the cells (one
random point in a random cell each, unsorted: the worst case for the gathers) before the first step and moved by
`cfdh_particles_step` in the scenario's after-step hook, which runs after the flow step and before the state is advanced.  The flow
step's time is the host clock around `solveStep()` (`Scenario.step_stats`; the step ends in a read-back), the kernel's time is
`cfdh_particle_stats.ms_kernel`.  Particles that reach a boundary stop, so `stepped` falls during a run: the rate is the sum of the
particles stepped over the sum of the kernel times, in particle-steps (of nsub substeps each) per second.  Both scenarios run at a
Courant number far above one (tens of cells per step), so with few substeps many particles cross more than 64 cells in one walk and
are lost: every run is made once per entry of --nsub, and the lost count is part of the record."""
import argparse
import json
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="stenosis115,bifurcation2e-4")
ap.add_argument("--counts", default="100000,1000000")
ap.add_argument("--nsub", default="2,8")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _scenario(case):
    if case.startswith("stenosis"):
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        return StenosisSimulation("stabilized_schur", 0.01, 1.0, grade="moderate", ny=int(case[8:] or 115), v_max=100.0, quiet=True)
    if case.startswith("bifurcation"):
        from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
        return MicrovasculatureSimulation("stabilized_schur", 0.01, 1.0, v_inlet=1.5, res=float(case[11:] or 2e-4), quiet=True,
                                          options=dict(remove_p_mean=0))
    raise SystemExit("unknown case " + case)


def _run(sim, n, nsub):
    from cfd_hemodynamic_amd import particles as P
    s = sim.solver
    s.u_prev.x.array[:] = 0.0   # from rest: every run does the same flow steps
    s.p_prev.x.array[:] = 0.0
    sim.early_stop_tolerance = 0
    rng = np.random.default_rng(0)
    x, cells = P.sample_in_cells(sim.mesh, rng.integers(0, len(sim.mesh.cells), n), rng)
    s.ctx.particles_enable(n, nsub)  # a context holds one capacity: every count gets a scenario of its own
    s.particles_seed(x, cells, 0.0)
    rec = []

    def after(t):
        st = s.particles_step(t - sim.dt)
        rec.append((st.ms_kernel, st.ms_total, st.stepped, st.active, st.exited, st.lost))

    sim.solve(None, max_steps=args.warmup + args.steps, write_every=0, afterStepCallback=after)
    rec = np.array(rec[args.warmup:], dtype=float)
    flow = 1e3 * np.array([dt for dt, _ in sim.step_stats[args.warmup:]])
    kern, flow_med = float(np.median(rec[:, 0])), float(np.median(flow))
    path = s.particles_get(4)
    return {"particles": n, "nsub": nsub, "flow_ms_per_step_median": flow_med, "flow_ms_min": float(flow.min()), "flow_ms_max": float(flow.max()),
            "kernel_ms_per_step_median": kern, "kernel_ms_min": float(rec[:, 0].min()), "kernel_ms_max": float(rec[:, 0].max()),
            "call_ms_per_step_median": float(np.median(rec[:, 1])), "kernel_over_flow_percent": 100.0 * kern / flow_med,
            "stepped_first": int(rec[0, 2]), "stepped_last": int(rec[-1, 2]), "active_end": int(rec[-1, 3]), "exited_end": int(rec[-1, 4]),
            "lost_end": int(rec[-1, 5]), "particle_steps_per_second": float(rec[:, 2].sum() / (rec[:, 0].sum() * 1e-3)),
            "path_mean": float(path.mean()), "advection_launches": int(s.ctx.info(105)), "particle_steps": int(s.ctx.info(104))}


def main():
    res = {"steps": args.steps, "warmup": args.warmup, "gpus": 1}
    for case in args.cases.split(","):
        runs, sizes = [], None
        for nsub in [int(v) for v in args.nsub.split(",")]:
            for n in [int(float(v)) for v in args.counts.split(",")]:
                sim = _scenario(case)
                sim.setup()
                sizes = {"vertices": sim.mesh.num_vertices, "cells": len(sim.mesh.cells), "gdim": sim.mesh.geometry.dim}
                runs.append(_run(sim, n, nsub))
                print(case, json.dumps(runs[-1]), flush=True)
                del sim
        res[case] = dict(sizes, runs=runs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
