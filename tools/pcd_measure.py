#!/usr/bin/env python3
"""stabilized_pcd against the same form under the Cahouet-Chabard Schur approximation (pc_type 1): ms/step, Newton iterations per
step, FGMRES iterations per Newton step, preconditioner builds, and the HIP-event times of the PCD kernels (cfdh_profile kinds 10:
K assembly, 11: apply pass).  One JSON line per run.
  python tools/pcd_measure.py --workload stenosis --v_max 300 --variant pcd_t1_ew [--steps 5] [--warmup 1]
workloads: stenosis (reference geometry, --ny 115), dfg_1 (--m 200, ~1 M DOF), simple_bifurcation (--res 2e-4, ~1 M DOF, tetrahedra);
variants: pcd_t{1,0}_{ew,noew} (time term in K on / off, Eisenstat-Walker on / off), cc_{ew,noew} (pc_type 1, same form)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cfd_hemodynamic_amd import _lib  # noqa: E402


def build(a):
    kw = dict(quiet=True)
    if a.workload == "stenosis":
        from cfd_hemodynamic_amd.scenarios.stenosis import StenosisSimulation
        return StenosisSimulation("stabilized_pcd", a.dt, 1e9, ny=a.ny, v_max=a.v_max, **kw)
    if a.workload == "dfg_1":
        from cfd_hemodynamic_amd.scenarios.dfg_1 import DFG1Benchmark
        return DFG1Benchmark("stabilized_pcd", a.dt, 1e9, m=a.m, **kw)
    from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
    return MicrovasculatureSimulation("stabilized_pcd", a.dt, 1e9, res=a.res, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["stenosis", "dfg_1", "simple_bifurcation"], default="stenosis")
    ap.add_argument("--variant", default="pcd_t1_ew")
    ap.add_argument("--ny", type=int, default=115)
    ap.add_argument("--v_max", type=float, default=100.0)
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--res", type=float, default=2e-4)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
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
    for k in range(a.warmup + a.steps):
        if k == a.warmup:
            builds0 = ctx.info(74)
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
    out = dict(tool="pcd_measure", workload=a.workload, variant=v, ndof=ndof, dt=a.dt, setup_s=round(t_setup, 2),
               schur=ctx.info(78), forcing=ctx.info(79))
    if a.workload == "stenosis":
        out.update(ny=a.ny, v_max=a.v_max)
    if walls:
        out.update(ms_per_step=float(np.median(walls)), newton_per_step=float(np.mean(newton)),
                   fgmres_per_newton=float(np.sum(krylov) / max(np.sum(newton), 1)), pc_builds=ctx.info(74) - builds0,
                   pc_builds_total=ctx.info(74))
    if failed_at is not None:
        out.update(failed_at_step=failed_at, error=error[:200])
    elif v.startswith("pcd"):
        # kernel times (HIP events; profiling replaces the graph replay by direct launches): one more step
        ctx.profile_enable(True)
        ctx.profile_reset()
        s.solveStep()
        ka, na = ctx.profile_get(10)
        pa, npa = ctx.profile_get(11)
        ev, nev = ctx.profile_get(7)
        ctx.profile_enable(False)
        ovh = ev / max(nev, 1)
        nvo, nnz = ctx.info(0), ctx.info(3)
        # bytes of one apply pass: fp32 K M_d^-1 + int32 columns per entry (SELL padding ignored), the gather of r counted once,
        # per row reads of r, 1/m_d, flag and writes of t, s, q
        apply_bytes = 8 * nnz + nvo * (8 + 8 + 1 + 24)
        t_apply = pa / max(npa, 1) - ovh
        out.update(k_assembly_ms=ka / max(na, 1), k_assemblies=na, pcd_apply_ms=pa / max(npa, 1), pcd_applies=npa,
                   event_overhead_ms=ovh, apply_bytes=apply_bytes,
                   apply_GBps=apply_bytes / max(t_apply, 1e-6) / 1e6, apply_frac_of_8TBps=apply_bytes / max(t_apply, 1e-6) / 8e9)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
