"""Host side of the plugins `stabilized_schur_pressure_backflow` and `stabilized_schur_velocity_vascular_backflow` and of the
`stenosis_pressure` scenario: everything that is decided before a context exists -- no GPU needed."""
from importlib import import_module

import pytest

from cfd_hemodynamic_amd.elements import create_box, create_rectangle
from cfd_hemodynamic_amd.mesh import create_unit_square
from cfd_hemodynamic_amd.mesh3d import create_unit_cube
from cfd_hemodynamic_amd.solvers.stabilized_schur_pressure_backflow import damped_outlet_pressure

ARGS = (0.01, 1.0, 0.01, [0.0, 0.0, 0.0])
PLUGINS = [("stabilized_schur_pressure_backflow", "p_inlet", dict(p_inlet=1.0, R_resistance=2.0)),
           ("stabilized_schur_velocity_vascular_backflow", "v_max", dict(v_max=1.0, R_resistance=2.0))]


class _Comm:
    size, rank = 2, 0


def _solver(name):
    return import_module("cfd_hemodynamic_amd.solvers." + name).Solver


@pytest.mark.parametrize("name,first,kw", PLUGINS)
def test_required_keywords_raise_the_references_errors(name, first, kw):
    Solver = _solver(name)
    with pytest.raises(ValueError, match="%s is required for %s. Pass it via CLI: --%s <value>" % (first, name, first)):
        Solver(create_unit_square(2), *ARGS, R_resistance=2.0)
    with pytest.raises(ValueError, match="R_resistance is required for %s. Pass it via CLI: --R_resistance <value>" % name):
        Solver(create_unit_square(2), *ARGS, **{first: 1.0})


@pytest.mark.parametrize("name,first,kw", PLUGINS)
def test_unsupported_configurations_are_refused_before_a_context_exists(name, first, kw):
    """NotImplementedError, not the RuntimeError a context would raise without a GPU."""
    Solver = _solver(name)
    with pytest.raises(NotImplementedError, match="p_grade=2"):
        Solver(create_unit_square(2), *ARGS, p_grade=2, **kw)
    with pytest.raises(NotImplementedError, match="p_grade=2"):
        Solver(create_unit_cube(1), *ARGS, p_grade=2, **kw)
    with pytest.raises(NotImplementedError, match="quadrilateral"):
        Solver(create_rectangle((0.0, 0.0), (2.0, 1.0), (2, 1)), *ARGS, **kw)
    with pytest.raises(NotImplementedError, match="hexahedron"):
        Solver(create_box((0.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2, 1, 1), cell_type="hexahedron"), *ARGS, **kw)
    for mesh in (create_unit_square(2), create_unit_cube(1)):
        with pytest.raises(NotImplementedError, match="partitioned"):
            Solver(mesh, *ARGS, comm=_Comm(), **kw)


def test_damped_update_follows_the_rule_by_hand():
    """p_c <- alpha R |Q| + (1 - alpha) p_c over three steps, R = 4, alpha = 0.75, p_c0 = R |Q0| with Q0 = 0.5."""
    R, a = 4.0, 0.75
    p = R * abs(0.5)
    assert p == 2.0
    p = damped_outlet_pressure(p, 1.0, R, a)        # 0.75 * 4 + 0.25 * 2
    assert p == 3.5
    p = damped_outlet_pressure(p, -0.25, R, a)      # 0.75 * 1 + 0.25 * 3.5: the flux enters by its magnitude
    assert p == 1.625
    p = damped_outlet_pressure(p, 0.0, R, a)        # 0.25 * 1.625
    assert p == 0.40625
    assert damped_outlet_pressure(7.0, 3.0, 2.0, 1.0) == 6.0 and damped_outlet_pressure(7.0, 3.0, 2.0, 0.0) == 7.0


class _Stop(Exception):
    pass


def test_stenosis_pressure_forwards_half_the_inlet_pressure_in_pascal(monkeypatch):
    from cfd_hemodynamic_amd import scenario
    from cfd_hemodynamic_amd.scenarios.stenosis_pressure import _MMHG_2D, StenosisPressureSimulation
    seen = {}

    def init(self, solver_name, scenario_name, rho, mu, dt, T, f, **solver_kwargs):
        seen.update(solver_kwargs, solver_name=solver_name, rho=rho, mu=mu)
        raise _Stop

    monkeypatch.setattr(scenario.Scenario, "__init__", init)
    with pytest.raises(_Stop):
        StenosisPressureSimulation("stabilized_schur_pressure_backflow", 0.01, 0.03, R_resistance=3.0, ny=8, quiet=True)
    assert seen["p_inlet"] == 80 * 133.322 / 2 == 80 * _MMHG_2D          # 80 mmHg by default
    assert seen["R_resistance"] == 3.0 and seen["beta_nitsche"] == 100.0 and seen["beta_backflow"] == 0.2
    assert seen["alpha_damping"] == 0.75 and seen["p_grade"] == 1 and "p_outlet" not in seen and "v_max" not in seen
    assert seen["rho"] == 1.06e-3 and seen["mu"] == 3.5e-3
    seen.clear()
    with pytest.raises(_Stop):
        StenosisPressureSimulation("stabilized_schur_pressure_backflow", 0.01, 0.03, p_inlet=10.6, R_resistance=3.0, beta_nitsche=50.0,
                                   beta_backflow=0.3, alpha_damping=0.5, p_grade=2, v_max=100.0)
    assert seen["p_inlet"] == 10.6 * 0.5 * 133.322
    assert (seen["beta_nitsche"], seen["beta_backflow"], seen["alpha_damping"], seen["p_grade"]) == (50.0, 0.3, 0.5, 2)


def test_stenosis_pressure_requires_the_resistance():
    from cfd_hemodynamic_amd.scenarios.stenosis_pressure import StenosisPressureSimulation
    with pytest.raises(ValueError, match="R_resistance is required for pressure-driven inlet"):
        StenosisPressureSimulation("stabilized_schur_pressure_backflow", 0.01, 0.03)
