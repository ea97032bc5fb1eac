"""Meshes, fields, closed forms and bounds shared by test_flow_twin.py (CPU) and test_gpu_flow.py (GPU).  The meshes are those of
particles_util.py plus one triangle and one tetrahedron; everything is built once and left unchanged.

A result is a dict: the vertex fields under the names of flow_twin.fields() and "integrals" [8]; `check_affine` and `check_twin`
take one from the twin or from the device alike."""
import types

import numpy as np

import flow_twin as T
import particles_util as PU

MU = PU.MU
RHO = 1.06e-3
TOL = PU.TOL          # closed forms: 1e-12 of the natural scale
TOL_TWIN = 1e-11      # device against the twin on non-affine fields, as in test_gpu_particles.py
TOL_LNH = 1e-9        # LNH is a ratio: absolute, where |u||omega| >= LNH_FLOOR of its maximum
LNH_FLOOR = 1e-6
LNH_MAX_EXCLUDED = 0.01
FIELDS_2D = ("vorticity", "q_criterion", "shear_rate", "dissipation")
FIELDS_3D = FIELDS_2D + ("helicity", "lnh")
_CACHE = {}


def mesh(name):
    """particles_util.mesh plus "triangle" and "tetrahedron": one cell, every facet exterior with marker 1."""
    if name not in ("triangle", "tetrahedron"):
        return PU.mesh(name)
    if name not in _CACHE:
        d = 2 if name == "triangle" else 3
        x = np.vstack([np.zeros(d), np.eye(d)])
        _CACHE[name] = types.SimpleNamespace(name=name, d=d, x=x, cells=np.arange(d + 1, dtype=np.int32)[None, :].copy(),
                                             facet_cells=np.zeros(d + 1, dtype=np.int32), facet_local=np.arange(d + 1, dtype=np.int32),
                                             facet_marker=np.ones(d + 1, dtype=np.int32), size=float(np.sqrt(d)), nv=d + 1, nc=1)
    return _CACHE[name]


def volume(m):
    return {"square": 1.0, "cube": 1.0, "triangle": 0.5, "tetrahedron": 1.0 / 6.0}[m.name]


def twin_result(m, u, mu=MU, rho=RHO):
    res = T.fields(m.x, m.cells, u, mu)
    res["integrals"] = T.integrals(m.x, m.cells, u, rho, mu)
    return res


# ---------------------------------------------------------------------------------------------------------------- closed forms
# P1 interpolates u = A x + b exactly, so G_v = A at every vertex, boundary vertices included, on any mesh.  A case: A, b, the
# closed-form constants of the vertex fields (`fields`: name -> constant or [nv] array) and of some integrals (`integrals`: index
# -> value).  Bound: TOL times |A|_F for gradient, vorticity and shear rate, |A|_F^2 for Q (and for helicity / LNH times the scale
# of u, which only the helical case states), mu |A|_F^2 for the dissipation; for an integral the magnitude of its closed form, or
# |A|_F^2 V where that is 0.
def _embed(m, A2):
    A = np.zeros((m.d, m.d))
    A[:2, :2] = A2
    return A


def case_rotation(m, om=1.7):
    A = _embed(m, [[0.0, -om], [om, 0.0]])
    V = volume(m)
    w = 2 * om if m.d == 2 else np.array([0.0, 0.0, 2 * om])
    return dict(A=A, b=-A @ np.full(m.d, 0.5), fields=dict(vorticity=w, q_criterion=om * om, shear_rate=0.0, dissipation=0.0),
                integrals={0: V, 2: 2 * om * om * V, 3: 0.0, 5: 0.0, 6: om * om * V, 7: 0.0})


def case_shear(m, gam=1.5):
    A = _embed(m, [[0.0, gam], [0.0, 0.0]])
    V = volume(m)
    w = -gam if m.d == 2 else np.array([0.0, 0.0, -gam])  # |omega| = gam
    return dict(A=A, b=np.zeros(m.d), fields=dict(vorticity=w, q_criterion=0.0, shear_rate=gam, dissipation=MU * gam * gam),
                integrals={0: V, 3: MU * gam * gam * V, 5: 0.0, 6: 0.0, 7: 0.0})


def case_strain(m, a=0.8):
    A = _embed(m, [[a, 0.0], [0.0, -a]])
    V = volume(m)
    w = 0.0 if m.d == 2 else np.zeros(3)
    return dict(A=A, b=np.full(m.d, 0.1), fields=dict(vorticity=w, q_criterion=-a * a, shear_rate=2 * a),
                integrals={0: V, 2: 0.0, 5: 0.0, 6: -a * a * V, 7: 0.0})


def case_dilatation(m, a=0.6):
    A = a * np.eye(m.d)
    V = volume(m)
    return dict(A=A, b=np.full(m.d, -0.2), fields=dict(vorticity=0.0 if m.d == 2 else np.zeros(3)),
                integrals={0: V, 2: 0.0, 5: m.d * a * V, 7: m.d * m.d * a * a * V})


A_FULL = np.array([[0.7, -1.3, 0.4], [0.9, 0.2, -0.6], [-0.5, 1.1, -0.3]])
B_FULL = np.array([0.35, -0.8, 0.55])


def case_full(m):
    """Fixed non-symmetric A and b; the kinetic energy in closed form on the unit box (V = 1)."""
    A, b = A_FULL[:m.d, :m.d].copy(), B_FULL[:m.d].copy()
    ints = {0: volume(m), 5: np.trace(A) * volume(m), 7: np.trace(A) ** 2 * volume(m)}
    if m.name in ("square", "cube"):
        mom = np.full((m.d, m.d), 0.25) + np.eye(m.d) * (1.0 / 3.0 - 0.25)
        ints[1] = 0.5 * RHO * sum(b[i] ** 2 + b[i] * A[i].sum() + A[i] @ mom @ A[i] for i in range(m.d))
    return dict(A=A, b=b, fields={}, integrals=ints)


def case_helical(m, om=1.3, w0=0.45):
    """u = (-om y', om x', w0) about the axis through (1/2, 1/2): u . omega = 2 om w0, LNH = w0 / sqrt(om^2 r^2 + w0^2)."""
    assert m.d == 3
    A = _embed(m, [[0.0, -om], [om, 0.0]])
    b = -A @ np.array([0.5, 0.5, 0.0]) + np.array([0.0, 0.0, w0])
    r2 = ((m.x[:, :2] - 0.5) ** 2).sum(axis=1)
    V = volume(m)
    return dict(A=A, b=b, fields=dict(helicity=2 * om * w0, lnh=w0 / np.sqrt(om * om * r2 + w0 * w0)), integrals={0: V, 4: 2 * om * w0 * V},
                u_scale=float(np.sqrt(om * om * r2.max() + w0 * w0)))


AFFINE_MESHES = ("square", "cube", "triangle", "tetrahedron")
AFFINE_CASES = {"rotation": case_rotation, "shear": case_shear, "strain": case_strain, "dilatation": case_dilatation, "full": case_full}


def affine_cases():
    """(mesh name, case name) of every closed-form case."""
    out = [(mn, cn) for mn in AFFINE_MESHES for cn in AFFINE_CASES]
    return out + [("cube", "helical"), ("tetrahedron", "helical")]


def affine_case(mesh_name, case_name):
    m = mesh(mesh_name)
    case = case_helical(m) if case_name == "helical" else AFFINE_CASES[case_name](m)
    case["m"] = m
    case["u"] = PU.affine_field(m, case["A"], case["b"])
    return case


def _worst(what, got, want, bound):
    err = float(np.abs(np.asarray(got) - want).max())
    print("%-14s err %.3e bound %.3e" % (what, err, bound))
    return err <= bound


def check_affine(case, res):
    m, A = case["m"], case["A"]
    nA = float(np.linalg.norm(A))
    ok = _worst("gradient", res["gradient"], A[None], TOL * nA)
    # what follows from G_v = A alone, then the constants the case states
    one = A[None]
    derived = dict(vorticity=T.vorticity(one)[0], q_criterion=T.q_criterion(one)[0], shear_rate=T.shear_rate(one)[0],
                   dissipation=T.dissipation(one, MU)[0])
    us = case.get("u_scale", 1.0)
    scale = dict(vorticity=nA, q_criterion=nA * nA, shear_rate=nA, dissipation=MU * nA * nA, helicity=nA * us, lnh=1.0)
    for name, want in list(derived.items()) + list(case["fields"].items()):
        ok = _worst(name, res[name], want, TOL * scale[name]) and ok
    V = volume(m)
    for k, want in case["integrals"].items():
        ok = _worst("integral %d" % k, res["integrals"][k], want, TOL * (abs(want) if want != 0.0 else nA * nA * V)) and ok
    if m.d == 2:
        ok = (res["integrals"][4] == 0.0) and ok
    return ok


# --------------------------------------------------------------------------------------------------- non-affine fields, the twin
def random_field(name):
    """The field of the device-against-twin tests on this mesh."""
    key = ("field", name)
    if key not in _CACHE:
        m = mesh(name)
        if name in ("stenosis", "bifurcation"):
            u = PU.drift_fields(m, 11, 3.0, 0.01, 2)[1]  # not zero on the walls; noise as large as the drift
        else:
            u = np.random.default_rng(5).uniform(-1.0, 1.0, (m.nv, m.d))
        _CACHE[key] = np.ascontiguousarray(u)
    return _CACHE[key]


def window_fields(name):
    """Two random P1 fields of the window-average tests."""
    m = mesh(name)
    rng = np.random.default_rng(17)
    return rng.uniform(-1.0, 1.0, (m.nv, m.d)), rng.uniform(-1.0, 1.0, (m.nv, m.d))


def twin_case(name):
    key = ("twin", name)
    if key not in _CACHE:
        m = mesh(name)
        u = random_field(name)
        _CACHE[key] = dict(m=m, u=u, twin=twin_result(m, u))
    return _CACHE[key]


def lnh_mask(tw):
    """The vertices where LNH is compared: |u||omega| of the twin at least LNH_FLOOR of its maximum."""
    w = tw["lnh_weight"]
    return w >= LNH_FLOOR * w.max()


def twin_scales(m, tw, u, mu=MU):
    """Scales of the bound TOL_TWIN: as for the closed forms with |A|_F replaced by max_v |G_v|_F of the twin."""
    g = float(np.sqrt((tw["gradient"] ** 2).sum(axis=(1, 2))).max())
    us = float(np.linalg.norm(u, axis=1).max())
    V = tw["integrals"][0]
    fields = dict(gradient=g, vorticity=g, q_criterion=g * g, shear_rate=g, dissipation=mu * g * g, helicity=g * us)
    # an integral: the magnitude of the twin's value, or g^2 V where that is 0 (the helicity in 2-D)
    ints = np.where(tw["integrals"] != 0.0, np.abs(tw["integrals"]), g * g * V)
    return fields, ints


def check_twin(case, res, mu=MU):
    m, tw = case["m"], case["twin"]
    fs, ints = twin_scales(m, tw, case["u"], mu)
    ok = True
    for name in ("gradient",) + (FIELDS_3D[:-1] if m.d == 3 else FIELDS_2D):
        ok = _worst(name, res[name], tw[name], TOL_TWIN * fs[name]) and ok
    for k in range(8):
        ok = _worst("integral %d" % k, res["integrals"][k], tw["integrals"][k], TOL_TWIN * ints[k]) and ok
    if m.d == 3:
        keep = lnh_mask(tw)
        assert (~keep).mean() <= LNH_MAX_EXCLUDED
        ok = _worst("lnh", res["lnh"][keep], tw["lnh"][keep], TOL_LNH) and ok
    return ok
