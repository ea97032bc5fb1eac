"""Drop-in `Solver` for the reference's `--solver ipcs_midpoint` (`src/solvers/ipcs_midpoint.py:60-80` there): the
pressure-correction scheme on P2 velocity / P1 pressure triangles and tetrahedra with the vector-coupled epsilon form
sigma = 2 mu eps(u) - p I at the midpoint, the ds pair p n . v - mu (nabla_grad(u) n) . v on every exterior facet (what makes an
open outlet behave in this form) and EXPLICIT convection rho (u_prev . grad) u_prev.  The momentum matrix is therefore constant:
it is assembled once per run (again only when dt, rho, mu or the set of constrained velocity nodes changes), where `ipcs_bdf2`
reassembles every step.  The price is a CFL-limited step: dt has to stay of the order of h / |u| (for P2 elements, a fraction of
it), or the run blows up -- there is no implicit convection to damp it.

Runs on the context of `ipcs_bdf2` (include/cfdh.h: cfdh_ipcs_set_scheme) and keeps that plugin's surface: the constructor,
`setup(bcu, bcp, facet_tags=None, tags=None)` -- the reference file still has the two-argument `setup` its own `Scenario` cannot
call --, `solveStep()`, the state Functions plus `u_star` and `phi`, the lazy host copies, `assemble_wss()` and the wall
indices.  What differs from `ipcs_bdf2`:

* a pressure Dirichlet VALUE is imposed on p itself (the correction takes value - p_prev), so non-homogeneous pressure data are
  right and nothing is warned about;
* `u_n1` exists but is neither used nor shifted;
* `consistent=True` (default) scales the force with rho (rho u_t + ... = rho f); `consistent=False` is the reference's literal
  dot(f, v).  The convection term carries rho in both, as in the reference.

Linear solvers: BiCGStab + point Jacobi on the d nn block system (reference: BiCGStab + BoomerAMG), flexible PCG + one V-cycle,
CG + Jacobi.  Quadrilateral / hexahedral meshes and a partitioned `comm` are refused before any device work.
"""
from __future__ import annotations

from .. import _lib
from .ipcs_bdf2 import Solver as _Bdf2Solver


class Solver(_Bdf2Solver):
    _name = "ipcs_midpoint"

    def _configure_scheme(self, rho):
        self.ctx.set_scheme(_lib.IPCS_MIDPOINT)
        if not self.consistent:
            self.ctx.set_form(rho, 1.0)   # ipcs_midpoint.py:64,67: rho on the convection term, - dot(f, v) in the residual

    def _check_pressure_values(self):
        pass   # the value goes into p: right for any data
