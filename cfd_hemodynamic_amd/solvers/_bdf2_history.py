"""History handling shared by the BDF2 plugins (`stabilized_schur_bdf2`, `stabilized_pcd_bdf2`): `u_prev2` in HBM, the
`bdf_a0/a1/a2` Constants, BDF1 on the first step and BDF2 afterwards, and the device-side shift after every step
(/root/reference/src/solvers/stabilized_schur_bdf2.py:72, :82-86, :298-305, :323-325).

A mixin in front of a `stabilized_schur`-derived Solver: the plugin's `__init__` calls `_init_bdf2_history(mesh)` once the base
class has built the context.
"""
from __future__ import annotations

from ..fem import Constant, Function


class Bdf2History:
    def _init_bdf2_history(self, mesh):
        self._u_prev2 = Function(self.V)  # u at time n-1 (:72)
        self.bdf_a0 = Constant(mesh, 1.0)
        self.bdf_a1 = Constant(mesh, -1.0)
        self.bdf_a2 = Constant(mesh, 0.0)
        self.step_count = 0
        self._prev2_host_dirty = True
        self._prev2_dev_newer = False
        self._u_prev2.x._pre_access = self._sync_previous2
        self._u_prev2.x._post_access = self._mark_prev2_dirty
        self.ctx.set_time_scheme(1.0, 1.0, -1.0, 0.0)

    @property
    def u_prev2(self):
        return self._u_prev2

    def _sync_previous2(self):
        if self._prev2_dev_newer:
            self._prev2_dev_newer = False
            lu = self.ctx.get_previous2()
            if self._part is None:
                self._u_prev2.x._array[:] = lu
            else:
                self._u_prev2.x._array[:] = self._comm.allgather_owned(lu, 2, self.mesh.num_vertices)

    def _mark_prev2_dirty(self):
        self._prev2_host_dirty = True

    def solveStep(self):
        # BDF1 for the first step, BDF2 thereafter (:298-305)
        if self.step_count == 0:
            self.bdf_a0.value, self.bdf_a1.value, self.bdf_a2.value = 1.0, -1.0, 0.0
        else:
            self.bdf_a0.value, self.bdf_a1.value, self.bdf_a2.value = 1.5, -2.0, 0.5
        self.ctx.set_time_scheme(1.0, float(self.bdf_a0.value), float(self.bdf_a1.value), float(self.bdf_a2.value))
        if self._prev2_host_dirty and not self._prev2_dev_newer:
            self.ctx.set_previous2(self._loc_u(self._u_prev2.x._array))
        self._prev2_host_dirty = False
        # u_prev must be on the device before the shift below reads it
        super().solveStep()
        # u_prev2 <- u_prev for the next step (:323-325)
        self.ctx.shift_history()
        self._prev2_dev_newer = True
        self.step_count += 1
