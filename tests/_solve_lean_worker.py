"""Worker of tests/test_gpu_solve_lean.py: runs time steps in a process of its own, started with the environment it is meant to
see: the library reads CFDH_KSP_LAG and CFDH_GS_ETA2 at context creation.  Usage: _solve_lean_worker.py <case> <nsteps> <ksp_rtol> <out.npz>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    from test_gpu_solve_lean import CASES, run_steps
    key, nsteps, rtol, out = sys.argv[1], int(sys.argv[2]), float(sys.argv[3]), sys.argv[4]
    r = run_steps(CASES[key](), nsteps, dict(ksp_rtol=rtol))
    np.savez(out, x=r["x"], krylov=np.array(r["krylov"]), newton=np.array(r["newton"]), discarded=r["discarded"])


if __name__ == "__main__":
    main()
