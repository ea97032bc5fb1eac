#!/usr/bin/env python3
"""stabilized_pcd_pressurebc on the two pressure-driven workloads of DESIGN.md section 9, against the Cahouet-Chabard Schur
approximation (pc_type 1) under the same plugin settings: ms/step, Newton iterations per step, FGMRES iterations per Newton step,
preconditioner builds, and the HIP-event time of the K assembly (cfdh_profile kind 10).  One JSON line per run.
  python tools/pcd_pressurebc_measure.py --workload stenosis --variant pcd_t1_ew
  python tools/pcd_pressurebc_measure.py --workload q1h --variant cc_ew
workloads: stenosis (ny 81, 10.6 / 10 mmHg, dt 0.01, timed steps 101-110: --warmup 100 --steps 10),
           q1h (unit_cube_pipe on 1065 x 8 x 8 hexahedra, 8.85 / 0 Pa, dt 0.01, five steps after one warm-up step);
variants: pcd_t{1,0}_{ew,noew} (time term in K on / off, Eisenstat-Walker on / off), cc_{ew,noew} (pc_type 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfd_hemodynamic_amd import _lib  # noqa: E402

SOLVER = "stabilized_pcd_pressurebc"
DEFAULT_STEPS = {"stenosis": (100, 10), "q1h": (1, 5)}   # (warm-up, timed)


def build(a):
    if a.workload == "stenosis":
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        return StenosisSimulation(SOLVER, a.dt, 1e9, ny=a.ny, p_inlet=10.6, p_outlet=10.0, quiet=True)
    from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation
    return UnitCubePipeSimulation(SOLVER, a.dt, 1e9, p_inlet=8.85, p_outlet=0.0, quiet=True, nx=a.nx, ny=8, nz=8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["stenosis", "q1h"], default="stenosis")
    ap.add_argument("--variant", default="pcd_t1_ew")
    ap.add_argument("--ny", type=int, default=81)
    ap.add_argument("--nx", type=int, default=1065)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    a = ap.parse_args()
    warmup, steps = DEFAULT_STEPS[a.workload]
    warmup = warmup if a.warmup is None else a.warmup
    steps = steps if a.steps is None else a.steps
    t0 = time.perf_counter()
    sc = build(a)   # (the scenario runs Solver.setup)
    s = sc.solver
    ctx = s.ctx
    v = a.variant
    if v.startswith("cc"):
        s.options.pc_type = _lib.PC_CAHOUET_CHABARD
        ctx.set_options(s.options)
    else:
        ctx.set_schur_pcd(sc.tags["inlet"], sc.tags["outlet"], 1 if "_t1" in v else 0)
    if v.endswith("noew"):
        ctx.set_ksp_forcing(0)
    t_setup = time.perf_counter() - t0
    ndof = (s.mesh.geometry.dim + 1) * s.mesh.num_vertices
    walls, newton, krylov = [], [], []
    builds0 = None
    failed_at, error = None, None
    for k in range(warmup + steps):
        if k == warmup:
            builds0 = ctx.info(74)
        t1 = time.perf_counter()
        try:
            s.solveStep()
        except RuntimeError as exc:
            failed_at, error = k + 1, str(exc)
            break
        s.advance()
        if k >= warmup:
            walls.append(1e3 * (time.perf_counter() - t1))
            newton.append(s.last_stats.newton_its)
            krylov.append(s.last_stats.krylov_its)
    out = dict(tool="pcd_pressurebc_measure", workload=a.workload, variant=v, ndof=ndof, dt=a.dt, warmup=warmup, setup_s=round(t_setup, 2),
               schur=ctx.info(78), forcing=ctx.info(79), form=ctx.info(77))
    if walls:
        out.update(ms_per_step=float(np.median(walls)), newton_per_step=float(np.mean(newton)), fgmres_per_step=float(np.mean(krylov)),
                   fgmres_per_newton=float(np.sum(krylov) / max(np.sum(newton), 1)), pc_builds=ctx.info(74) - builds0,
                   pc_builds_total=ctx.info(74), q_out=s.functional(7, sc.outlet_marker))
    if failed_at is not None:
        out.update(failed_at_step=failed_at, error=error[:200])
    elif v.startswith("pcd"):
        # kernel time (HIP events; profiling replaces the graph replay by direct launches): one more step
        ctx.profile_enable(True)
        ctx.profile_reset()
        s.solveStep()
        ka, na = ctx.profile_get(10)
        pa, npa = ctx.profile_get(11)
        ctx.profile_enable(False)
        out.update(k_assembly_ms=ka / max(na, 1), k_assemblies=na, pcd_apply_ms=pa / max(npa, 1), pcd_applies=npa)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
