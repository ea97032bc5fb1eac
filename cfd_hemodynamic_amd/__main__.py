"""`python -m cfd_hemodynamic_amd simulate --simulation dfg_1 --solver stabilized_schur --T 1.0 --dt 0.01 --name X`
-- the `simulate` sub-command of the reference's CLI (/root/reference/main.py:87-139,253-254);
unknown `--key value` pairs are literal-evaluated and passed to the scenario (main.py:12-31).
`--wall_indices_from T0 --wall_indices_to T1` (defaults 0 and T; either switches it on) writes the cycle-averaged wall shear
indices of that window next to the other results (wall_indices.npz / .vtu / .txt).
`--transport age` or `--transport bolus [--bolus_from T0 --bolus_to T1]` (defaults 0 and T), with `--transport_diffusivity D`, steps a
passive scalar on the device behind every flow step and writes transport.npz and the `transport` VTU series.
`--particles N [--particles_every K --particles_nsub M]` releases N massless particles on the inlet (once at t = 0, or every K steps),
tracks them on the device behind every flow step and writes particles.npz and the `particles` VTU point clouds.
`--flow_fields vorticity,q_criterion[,shear_rate,dissipation,helicity,lnh]` and / or `--flow_window_from T0 --flow_window_to T1`
(defaults 0 and T; either switches the window averages on) compute the volumetric flow diagnostics on the device behind every flow
step: the fields join the VTU series, the per-step energy integrals and the window averages go to flow_diagnostics.npz / .txt.
`--probes "x,y[,z];x,y[,z];..."` and / or `--probe_line "x0,y0[,z0];x1,y1[,z1];n"` sample velocity and pressure at those points on
the device after every `--sample_every`-th step (default 1) and write probes.npz; `--sample_grid_spacing H` samples them on a regular
grid over the mesh's bounding box instead (grid/grid_NNNNNN.vti at `--sample_every`), and `--sample_window_from T0 --sample_window_to
T1` (defaults 0 and T) adds the window means on that grid (grid_mean.vti).  Probes and a grid exclude each other (one sample set
per run), and the window and `--sample_every` flags without the set they belong to are refused before the scenario is built.
`--sections "ox,oy[,oz];nx,ny[,nz][;r] | ..."` integrates flow rate, pressure and energy flux exactly over those cut planes on the
device after every `--sections_every`-th step (default 1) and writes sections.npz and sections.txt; `--sections_window_from T0
--sections_window_to T1` (defaults 0 and T) adds the window means of the rows.  Sections go with every other feature."""
from __future__ import annotations

import argparse
import ast
import inspect
import os
import sys
from importlib import import_module

from .scenario import Scenario


def _parse_extra(extra):
    out = {}
    it = iter(extra)
    for k in it:
        if not k.startswith("--"):
            raise ValueError(f"unexpected argument {k}")
        v = next(it, None)
        if v is None:
            raise ValueError(f"missing value for {k}")
        try:
            out[k[2:]] = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            out[k[2:]] = v
    return out


def _check_sampler_flags(ap, args):
    """The sampler holds one sample set per context: probes or a grid, and the flags that belong to neither are refused."""
    probes = args.probes is not None or args.probe_line is not None
    grid = args.sample_grid_spacing is not None
    if probes and grid:
        ap.error("--probes / --probe_line and --sample_grid_spacing exclude each other: the sampler holds one sample set per run")
    if not grid and (args.sample_window_from is not None or args.sample_window_to is not None):
        ap.error("--sample_window_from / --sample_window_to need --sample_grid_spacing (the window means live on the grid)")
    if not probes and not grid and args.sample_every is not None:
        ap.error("--sample_every needs --probes, --probe_line or --sample_grid_spacing")


def parse_sections(text):
    """The planes of `--sections`: "origin;normal[;radius]" separated by "|"."""
    from .sections import plane
    out = []
    for part in text.split("|"):
        if not part.strip():
            continue
        f = [q.strip() for q in part.split(";")]
        if len(f) not in (2, 3):
            raise ValueError("--sections: every plane is 'ox,oy[,oz];nx,ny[,nz][;r]', got %r" % part)
        out.append(plane([float(v) for v in f[0].split(",")], [float(v) for v in f[1].split(",")], float(f[2]) if len(f) == 3 else None))
    if not out:
        raise ValueError("--sections: no plane given")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="cfd_hemodynamic_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("simulate")
    s.add_argument("--simulation", required=True)
    s.add_argument("--solver", default="stabilized_schur")
    s.add_argument("--T", type=float, required=True)
    s.add_argument("--dt", type=float, required=True)
    s.add_argument("--name", default="run")
    s.add_argument("--output_dir", default="results")
    # cycle-averaged wall shear indices (TAWSS, OSI, RRT) over the steps that end in (from, to]; either switch turns them on
    s.add_argument("--wall_indices_from", type=float, default=None)
    s.add_argument("--wall_indices_to", type=float, default=None)
    # passive scalar on the device: blood age, or a contrast bolus with inlet c = 1 for the steps that end in (bolus_from, bolus_to]
    s.add_argument("--transport", choices=["age", "bolus"], default=None)
    s.add_argument("--transport_diffusivity", type=float, default=0.0)
    s.add_argument("--bolus_from", type=float, default=None)
    s.add_argument("--bolus_to", type=float, default=None)
    # Lagrangian particles on the device: N per release on the inlet, released every K steps (default: once), M substeps per step
    s.add_argument("--particles", type=int, default=None)
    s.add_argument("--particles_every", type=int, default=None)
    s.add_argument("--particles_nsub", type=int, default=None)
    # volumetric flow diagnostics on the device: point fields for the VTU series, window (t0, t1] of the pulsatile averages
    s.add_argument("--flow_fields", type=str, default=None)
    s.add_argument("--flow_window_from", type=float, default=None)
    s.add_argument("--flow_window_to", type=float, default=None)
    # point sampler on the device: probe points / a line of probes, or a voxel grid with its window means
    s.add_argument("--probes", type=str, default=None)
    s.add_argument("--probe_line", type=str, default=None)
    s.add_argument("--sample_grid_spacing", type=float, default=None)
    s.add_argument("--sample_every", type=int, default=None)
    s.add_argument("--sample_window_from", type=float, default=None)
    s.add_argument("--sample_window_to", type=float, default=None)
    # cut-plane sections on the device: planes, the recording interval and the window of the means
    s.add_argument("--sections", type=str, default=None)
    s.add_argument("--sections_every", type=int, default=None)
    s.add_argument("--sections_window_from", type=float, default=None)
    s.add_argument("--sections_window_to", type=float, default=None)
    args, extra = ap.parse_known_args(argv)
    _check_sampler_flags(ap, args)
    if args.sections is None and (args.sections_every is not None or args.sections_window_from is not None or args.sections_window_to is not None):
        ap.error("--sections_every / --sections_window_from / --sections_window_to need --sections")
    if args.sections is not None:
        try:
            section_planes = parse_sections(args.sections)
        except ValueError as e:
            ap.error(str(e))
    kw = _parse_extra(extra)
    try:
        mod = import_module(f"{__package__}.scenarios.{args.simulation}")
    except ImportError as e:
        raise ImportError(f"unknown simulation '{args.simulation}': {e}") from e
    cls = next(c for _, c in inspect.getmembers(mod, inspect.isclass) if issubclass(c, Scenario) and c is not Scenario)
    sim = cls(args.solver, args.dt, args.T, **kw)
    out = os.path.join(args.output_dir, args.simulation, args.name)
    sim.setup()  # the reference calls setup() a second time in Simulation.run (simulation.py:269)
    solve_kw = {}
    if args.wall_indices_from is not None or args.wall_indices_to is not None:
        solve_kw["wall_indices"] = (0.0 if args.wall_indices_from is None else args.wall_indices_from,
                                    args.T if args.wall_indices_to is None else args.wall_indices_to)
    if args.transport == "age":
        solve_kw["transport"] = "age"
    elif args.transport == "bolus":
        solve_kw["transport"] = ("bolus", 0.0 if args.bolus_from is None else args.bolus_from, args.T if args.bolus_to is None else args.bolus_to)
    if args.transport:
        solve_kw["transport_diffusivity"] = args.transport_diffusivity
    if args.particles is not None:
        solve_kw["particles"] = {"n": args.particles}
        if args.particles_every is not None:
            solve_kw["particles"]["every"] = args.particles_every
        if args.particles_nsub is not None:
            solve_kw["particles"]["nsub"] = args.particles_nsub
    if args.flow_fields is not None or args.flow_window_from is not None or args.flow_window_to is not None:
        solve_kw["flow_diagnostics"] = {}
        if args.flow_fields is not None:
            solve_kw["flow_diagnostics"]["fields"] = tuple(k for k in args.flow_fields.split(",") if k)
        if args.flow_window_from is not None or args.flow_window_to is not None:
            solve_kw["flow_diagnostics"]["window"] = (0.0 if args.flow_window_from is None else args.flow_window_from,
                                                      args.T if args.flow_window_to is None else args.flow_window_to)
    if args.probes is not None or args.probe_line is not None:
        from .sampling import line
        pts = []
        if args.probes is not None:
            pts += [[float(v) for v in q.split(",")] for q in args.probes.split(";") if q]
        if args.probe_line is not None:
            p0, p1, n = args.probe_line.split(";")
            pts += line([float(v) for v in p0.split(",")], [float(v) for v in p1.split(",")], int(n)).tolist()
        solve_kw["probes"] = {"points": pts}
        if args.sample_every is not None:
            solve_kw["probes"]["every"] = args.sample_every
    if args.sample_grid_spacing is not None:
        solve_kw["sample_grid"] = {"spacing": args.sample_grid_spacing}
        if args.sample_every is not None:
            solve_kw["sample_grid"]["every"] = args.sample_every
        if args.sample_window_from is not None or args.sample_window_to is not None:
            solve_kw["sample_grid"]["window"] = (0.0 if args.sample_window_from is None else args.sample_window_from,
                                                 args.T if args.sample_window_to is None else args.sample_window_to)
    if args.sections is not None:
        solve_kw["sections"] = {"planes": section_planes}
        if args.sections_every is not None:
            solve_kw["sections"]["every"] = args.sections_every
        if args.sections_window_from is not None or args.sections_window_to is not None:
            solve_kw["sections"]["window"] = (0.0 if args.sections_window_from is None else args.sections_window_from,
                                              args.T if args.sections_window_to is None else args.sections_window_to)
    sim.solve(out, **solve_kw)
    print("results in", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
