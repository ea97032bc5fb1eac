#!/usr/bin/env python3
"""Pressure-driven unit_cube_pipe (80 x 1.5 x 1.5 mm, p_inlet 8.85 / p_outlet 0) with `stabilized_schur_pressurebc` in 3-D: ms/step,
Newton and FGMRES iterations per step, and the assembly pass of the rotational kernels against the convective ones on the same
mesh and state (cfdh_profile kind 0), for three meshes -- hexahedra at the q1h mesh (1065 x 8 x 8 cells, 345 k DOF), hexahedra at
about 1 M DOF (853 x 16 x 16 cells, square cells as in the reference's box) and P2 tetrahedra at the p2t mesh (426 x 4 x 4 bricks
x 6).  Prints one JSON line.
  python tools/pressurebc3_measure.py [--steps 5] [--warmup 1] [--dt 0.01] [--reps 10] [--only q1h,q1h_1m,p2t]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfd_hemodynamic_amd import _lib  # noqa: E402
from cfd_hemodynamic_amd.scenarios.unit_cube_pipe import UnitCubePipeSimulation  # noqa: E402

MESHES = {
    "q1h": dict(nx=1065, ny=8, nz=8),
    "q1h_1m": dict(nx=853, ny=16, nz=16),
    "p2t": dict(nx=426, ny=4, nz=4, cell_type="tetrahedron", p_grade=2),
}


def assembly_ms(ctx, reps):
    ctx.profile_enable(True)
    ctx.assemble(True)  # warm
    ctx.profile_reset()
    for _ in range(reps):
        ctx.assemble(True)
    ms, n = ctx.profile_get(0)
    ctx.profile_enable(False)
    return ms / max(n, 1)


def measure(name, a):
    t0 = time.perf_counter()
    sc = UnitCubePipeSimulation("stabilized_schur_pressurebc", a.dt, 1e9, p_inlet=8.85, p_outlet=0.0, quiet=True, **MESHES[name])
    s = sc.solver
    out = dict(ndof=4 * s._dm.num_vertices, setup_s=round(time.perf_counter() - t0, 2))
    walls, newton, krylov = [], [], []
    for k in range(a.warmup + a.steps):
        t1 = time.perf_counter()
        try:
            s.solveStep()
        except RuntimeError as exc:
            out.update(failed_at_step=k + 1, error=str(exc)[:200])
            break
        s.advance()
        if k >= a.warmup:
            walls.append(1e3 * (time.perf_counter() - t1))
            newton.append(s.last_stats.newton_its)
            krylov.append(s.last_stats.krylov_its)
    if walls:
        out.update(ms_per_step=float(np.median(walls)), newton_per_step=float(np.mean(newton)), fgmres_per_step=float(np.mean(krylov)))
    q_in, q_out = -s.functional(7, sc.inlet_marker), s.functional(7, sc.outlet_marker)
    out.update(q_in=q_in, q_out=q_out, u_mean_mm_s=q_out / (sc.W * sc.H))
    ctx = s.ctx
    rot = assembly_ms(ctx, a.reps)
    ctx.set_pressure_boundaries([], [], 0.0)
    ctx.set_formulation(_lib.FORM_CONVECTIVE)
    conv = assembly_ms(ctx, a.reps)
    out.update(asm_ms_rotational=rot, asm_ms_convective=conv, asm_ratio_rot_over_conv=rot / conv)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=",".join(MESHES))
    a = ap.parse_args()
    out = dict(tool="pressurebc3_measure", dt=a.dt, steps=a.steps, warmup=a.warmup)
    for name in a.only.split(","):
        out[name] = measure(name, a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
