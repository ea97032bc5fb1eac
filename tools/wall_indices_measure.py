#!/usr/bin/env python
"""What the cycle-averaged wall shear indices cost in the time loop: ms/step of `Scenario.solve(write_every=0)` with
`wall_indices` off and with `wall_indices=True`, on one GPU, profiler off.

    python tools/wall_indices_measure.py [--cases dfg200,bifurcation2e-4] [--steps 20] [--warmup 5] [--reps 4] [--tree DIR] [--out FILE]

Per case one scenario is built (the workloads of bench.py's c3 and c5b lines: `dfg_1` m = 200, `simple_bifurcation` res = 2e-4, both
on `stabilized_schur`, dt = 0.01).  After a warm-up block the two variants alternate, `--reps` blocks of `--steps` steps each; every
block starts from the state at rest (u_prev = p_prev = 0), so the blocks do the same work, and is timed with the host clock around
the whole `solve` call, which ends in a device synchronisation (the final functionals).  Reported per variant: the median ms/step over
its blocks, the smallest and largest block, and the FGMRES iterations per step (equal iterations = equal work); and the cost of
the added call itself, `accumulate_call_us`, next to the wall shear stress call the loop pays anyway, `wss_call_us`.

`--tree DIR` imports the package from another checkout (the parent commit, built there) instead of this one: a tree without the
feature runs "off" in both slots, which gives the parent's number and the run-to-run spread of a lease in one go."""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="dfg200,bifurcation2e-4")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))


def _scenario(case):
    if case.startswith("dfg"):
        from cfd_hemodynamic_amd.scenarios.dfg_1 import DFG1Benchmark
        return DFG1Benchmark("stabilized_schur", 0.01, 1.0, m=int(case[3:] or 200), quiet=True)
    if case.startswith("bifurcation"):
        from cfd_hemodynamic_amd.scenarios.simple_bifurcation import MicrovasculatureSimulation
        return MicrovasculatureSimulation("stabilized_schur", 0.01, 1.0, v_inlet=1.5, res=float(case[11:] or 2e-4), quiet=True,
                                          options=dict(remove_p_mean=0))
    raise SystemExit("unknown case " + case)


def _block(sim, steps, on):
    s = sim.solver
    s.u_prev.x.array[:] = 0.0   # from rest: every block does the same steps
    s.p_prev.x.array[:] = 0.0
    kw = dict(wall_indices=True) if on else {}
    sim.early_stop_tolerance = 0
    t0 = time.perf_counter()
    sim.solve(None, max_steps=steps, write_every=0, **kw)
    ms = 1e3 * (time.perf_counter() - t0) / sim.num_steps
    its = float(np.mean([st.krylov_its for _, st in sim.step_stats]))
    return ms, its


def _calls(sim, n=200):
    """microseconds per `wall_stats_accumulate` (wall shear stress + the accumulate kernel) and per `wall_shear_stress` alone on the
    final state: n calls back to back between two device synchronisations, host clock"""
    s, out = sim.solver, []
    s.ctx.wall_stats_reset()
    for call in (lambda: s.ctx.wall_stats_accumulate(0.01), lambda: s.ctx.wall_shear_stress(download=False)):
        call()
        s.functional(4)
        t0 = time.perf_counter()
        for _ in range(n):
            call()
        s.functional(4)
        out.append(1e6 * (time.perf_counter() - t0) / n)
    return out


def main():
    import inspect

    from cfd_hemodynamic_amd.scenario import Scenario
    has_feature = "wall_indices" in inspect.signature(Scenario.solve).parameters
    res = {"tree": os.path.abspath(args.tree), "has_feature": has_feature, "steps": args.steps, "reps": args.reps}
    for case in args.cases.split(","):
        sim = _scenario(case)
        sim.setup()
        nv = sim.mesh.num_vertices
        _block(sim, args.warmup, False)
        if has_feature:
            _block(sim, args.warmup, True)
        rec = {"off": [], "on": []}
        for _ in range(args.reps):
            for slot in ("off", "on"):
                rec[slot].append(_block(sim, args.steps, slot == "on" and has_feature))
        r = {"vertices": nv, "dof": (sim.mesh.geometry.dim + 1) * nv}
        for slot in ("off", "on"):
            ms = [b[0] for b in rec[slot]]
            name = slot if has_feature else "off_slot_" + slot
            r[name] = {"ms_per_step_median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)),
                       "krylov_its_per_step": float(np.mean([b[1] for b in rec[slot]])), "blocks": ms}
        if has_feature:
            r["on_minus_off_ms"] = r["on"]["ms_per_step_median"] - r["off"]["ms_per_step_median"]
            r["on_minus_off_percent"] = 100.0 * r["on_minus_off_ms"] / r["off"]["ms_per_step_median"]
            r["accumulations_last_block"] = int(sim.solver.ctx.info(90))
            r["accumulate_call_us"], r["wss_call_us"] = _calls(sim)
        res[case] = r
        print(case, json.dumps(r), flush=True)
        del sim
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
