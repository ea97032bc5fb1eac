#!/usr/bin/env python3
"""Pressure-driven flow with `stabilized_schur_pressure_backflow` at size: ms/step, Newton and FGMRES iterations per step, and the
assembly pass (cfdh_profile kind 0) with and without the traction boundaries on the same context and state -- without them the
pass is the volume kernel alone, the code path of a context that never set a boundary.  Prints one JSON line per run.
  python tools/pressure_backflow_measure.py stenosis [--ny 81] [--p_inlet 10.6] [--R 0.05] [--steps 10] [--warmup 2] [--dt 0.001]
        (stenosis_pressure; then the rotational plugin stabilized_schur_vascularbc on the same mesh, for comparison)
  python tools/pressure_backflow_measure.py bifurcation [--res 2e-4] [--p_inlet 50] [--R 1e5]
A step that does not converge ends the run; the line then says at which step and why."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def assembly_ms(ctx, reps):
    ctx.profile_enable(True)
    ctx.assemble(True)  # warm
    ctx.profile_reset()
    for _ in range(reps):
        ctx.assemble(True)
    ms, n = ctx.profile_get(0)
    ctx.profile_enable(False)
    return ms / max(n, 1)


def run(sc, a, out):
    s = sc.solver
    walls, newton, krylov = [], [], []
    failed_at, error = None, None
    for k in range(a.warmup + a.steps):
        t1 = time.perf_counter()
        try:
            s.solveStep()
        except RuntimeError as exc:
            failed_at, error = k + 1, str(exc)
            break
        s.advance()
        if k >= a.warmup:
            walls.append(1e3 * (time.perf_counter() - t1))
            newton.append(s.last_stats.newton_its)
            krylov.append(s.last_stats.krylov_its)
    out.update(steps_timed=len(walls), u_max=s.functional(4), q_outlet=s.functional(7, sc.outlet_marker), singular=s.ctx.info(76))
    if walls:
        out.update(ms_per_step=float(np.median(walls)), newton_per_step=float(np.mean(newton)), fgmres_per_step=float(np.mean(krylov)),
                   fgmres_per_newton=float(np.sum(krylov) / max(np.sum(newton), 1)))
    if getattr(s, "outlet_history", None):
        out.update(p_c_last=s.outlet_history[-1][1])
    if failed_at is not None:
        out.update(failed_at_step=failed_at, error=error[:200])
    return failed_at is None


def traction_assembly(s, a, out):
    ctx = s.ctx
    with_tb = assembly_ms(ctx, a.reps)
    launches = ctx.info(94)
    ctx.set_traction_boundaries([], [])
    without = assembly_ms(ctx, a.reps)
    assert ctx.info(94) == launches
    out.update(asm_ms_with_traction=with_tb, asm_ms_without=without, asm_added_us=1e3 * (with_tb - without))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["stenosis", "bifurcation"])
    ap.add_argument("--ny", type=int, default=81)
    ap.add_argument("--res", type=float, default=2e-4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dt", type=float, default=None)
    ap.add_argument("--p_inlet", type=float, default=None)
    ap.add_argument("--R", type=float, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no_rotational", action="store_true")
    a = ap.parse_args()
    name = "stabilized_schur_pressure_backflow"
    if a.case == "stenosis":
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        from cfd_hemodynamic_amd.scenarios.stenosis_pressure import StenosisPressureSimulation
        dt = 1e-3 if a.dt is None else a.dt
        p_in = 10.6 if a.p_inlet is None else a.p_inlet
        R = 0.05 if a.R is None else a.R
        t0 = time.perf_counter()
        sc = StenosisPressureSimulation(name, dt, 1e9, p_inlet=p_in, R_resistance=R, ny=a.ny, quiet=True)
        out = dict(tool="pressure_backflow_measure", case="stenosis_pressure", solver=name, ndof=3 * sc.mesh.num_vertices, ny=a.ny, dt=dt,
                   p_inlet_mmHg=p_in, R_resistance=R, setup_s=round(time.perf_counter() - t0, 2))
        if run(sc, a, out):
            sc._compute_ffr(None)
            out.update(ffr=sc.ffr)
            traction_assembly(sc.solver, a, out)
        print(json.dumps(out), flush=True)
        if not a.no_rotational:
            rot = "stabilized_schur_vascularbc"
            t0 = time.perf_counter()
            sr = StenosisSimulation(rot, dt, 1e9, ny=a.ny, p_inlet=p_in, R_resistance=R, quiet=True)
            outr = dict(tool="pressure_backflow_measure", case="stenosis", solver=rot, ndof=3 * sr.mesh.num_vertices, ny=a.ny, dt=dt,
                        p_inlet_mmHg=p_in, R_resistance=R, setup_s=round(time.perf_counter() - t0, 2))
            if run(sr, a, outr):
                sr._compute_ffr(None)
                outr.update(ffr=sr.ffr)
            print(json.dumps(outr), flush=True)
    else:
        from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
        dt = 1e-2 if a.dt is None else a.dt
        p_in = 50.0 if a.p_inlet is None else a.p_inlet
        R = 1e5 if a.R is None else a.R
        t0 = time.perf_counter()
        sc = MicrovasculatureSimulation(name, dt, 1e9, res=a.res, p_inlet=p_in, R_resistance=R, quiet=True)
        out = dict(tool="pressure_backflow_measure", case="simple_bifurcation", solver=name, ndof=4 * sc.mesh.num_vertices, res=a.res, dt=dt,
                   p_inlet=p_in, R_resistance=R, setup_s=round(time.perf_counter() - t0, 2))
        if run(sc, a, out):
            qi, q1, q2 = sc.flow_rates()
            out.update(q_inlet=qi, q_outlet1=q1, q_outlet2=q2)
            traction_assembly(sc.solver, a, out)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
