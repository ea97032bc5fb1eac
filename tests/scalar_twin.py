"""NumPy / SciPy restatement of the passive-scalar transport step (include/cfdh.h, "passive scalar transport"), written from the
formulas, for the tests: dc/dt + w . grad c - D lap c = s with P1, SUPG and a theta-scheme on triangles and tetrahedra.  It assembles
with scipy.sparse and steps with a direct solve.  Test infrastructure: no product code calls it.

Per cell K with d = gdim, g_a = grad(lambda_a), |K|, h = largest vertex distance, w_a = theta u_sol,a + (1 - theta) u_prev,a,
wbar = mean_a w_a, tau = [(2/dt)^2 + (2 |wbar| / h)^2 + (4 D / h^2)^2]^(-1/2), p_a = tau wbar . g_a:
  M_ab = |K| (1 + d_ab) / ((d+1)(d+2))                 Ms_ab = p_a |K| / (d+1)
  C_ab = |K| / ((d+1)(d+2)) (sum_c w_c + w_a) . g_b    Cs_ab = p_a |K| wbar . g_b
  K_ab = D |K| g_a . g_b                               b_a   = s |K| (1 / (d+1) + p_a)
  [(M + Ms)/dt + theta (C + K + Cs)] c1 = [(M + Ms)/dt - (1 - theta)(C + K + Cs)] c0 + b,  Dirichlet rows = identity rows.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def geometry(x, cells):
    """g [nc, d+1, d] = grad(lambda_a), vol [nc], h [nc] (largest vertex distance)."""
    X = np.asarray(x, dtype=np.float64)[np.asarray(cells)]
    d = X.shape[2]
    assert X.shape[1] == d + 1
    M = X[:, 1:, :] - X[:, :1, :]                      # rows x_a - x_0
    Minv = np.linalg.inv(M)                            # columns = grad(lambda_a), a >= 1
    g = np.empty((len(X), d + 1, d))
    g[:, 1:, :] = np.transpose(Minv, (0, 2, 1))
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    vol = np.abs(np.linalg.det(M)) / (2.0 if d == 2 else 6.0)
    h = np.zeros(len(X))
    for a in range(d + 1):
        for b in range(a + 1, d + 1):
            h = np.maximum(h, np.linalg.norm(X[:, a] - X[:, b], axis=1))
    return g, vol, h


def cell_velocity(cells, u_sol, u_prev, theta):
    d = np.asarray(cells).shape[1] - 1
    w = theta * np.asarray(u_sol, dtype=np.float64).reshape(-1, d) + (1.0 - theta) * np.asarray(u_prev, dtype=np.float64).reshape(-1, d)
    return w[np.asarray(cells)]                        # [nc, d+1, d]


def tau_c(wbar, h, dt, D):
    return 1.0 / np.sqrt((2.0 / dt) ** 2 + (2.0 * np.linalg.norm(wbar, axis=1) / h) ** 2 + (4.0 * D / h ** 2) ** 2)


def element_matrices(x, cells, u_sol, u_prev, dt, D, s, theta):
    """dict of M, C, K, Ms, Cs [nc, d+1, d+1] and b [nc, d+1], from the closed forms."""
    g, vol, h = geometry(x, cells)
    n1 = g.shape[1]
    d = n1 - 1
    wv = cell_velocity(cells, u_sol, u_prev, theta)
    wbar = wv.mean(axis=1)
    tau = tau_c(wbar, h, dt, D)
    p = tau[:, None] * np.einsum("ci,cai->ca", wbar, g)
    cm = vol / ((d + 1.0) * (d + 2.0))
    M = cm[:, None, None] * (1.0 + np.eye(n1))[None]
    wsum = wv.sum(axis=1)[:, None, :] + wv            # sum_c w_c + w_a
    C = cm[:, None, None] * np.einsum("cai,cbi->cab", wsum, g)
    K = D * vol[:, None, None] * np.einsum("cai,cbi->cab", g, g)
    Ms = (p * (vol / (d + 1.0))[:, None])[:, :, None] * np.ones((1, 1, n1))
    Cs = (p * vol[:, None])[:, :, None] * np.einsum("ci,cbi->cb", wbar, g)[:, None, :]
    b = s * vol[:, None] * (1.0 / (d + 1.0) + p)
    return dict(M=M, C=C, K=K, Ms=Ms, Cs=Cs, b=b, tau=tau, wbar=wbar, p=p, g=g, vol=vol, h=h)


def _scatter(cells, E, nv):
    cells = np.asarray(cells)
    n1 = cells.shape[1]
    rows = np.repeat(cells, n1, axis=1).ravel()
    cols = np.tile(cells, (1, n1)).ravel()
    return sp.csr_matrix((E.ravel(), (rows, cols)), shape=(nv, nv))


def assemble(x, cells, u_sol, u_prev, c0, dt, D, s, theta, dir_nodes=(), dir_vals=()):
    """(A csr [nv, nv], rhs [nv]) of one step from c0."""
    nv = len(x)
    E = element_matrices(x, cells, u_sol, u_prev, dt, D, s, theta)
    mass = (E["M"] + E["Ms"]) / dt
    spat = E["C"] + E["K"] + E["Cs"]
    A = _scatter(cells, mass + theta * spat, nv).tolil()
    R = _scatter(cells, mass - (1.0 - theta) * spat, nv)
    rhs = R @ np.asarray(c0, dtype=np.float64)
    np.add.at(rhs, np.asarray(cells).ravel(), E["b"].ravel())
    dir_nodes = np.asarray(dir_nodes, dtype=np.int64).reshape(-1)
    dir_vals = np.broadcast_to(np.asarray(dir_vals, dtype=np.float64), dir_nodes.shape)
    for n, v in zip(dir_nodes, dir_vals):                # a node listed twice keeps the later value
        A.rows[n], A.data[n] = [int(n)], [1.0]
        rhs[n] = v
    A = A.tocsr()
    A.sort_indices()
    return A, rhs


def step(x, cells, u_sol, u_prev, c0, dt, D, s, theta, dir_nodes=(), dir_vals=()):
    A, rhs = assemble(x, cells, u_sol, u_prev, c0, dt, D, s, theta, dir_nodes, dir_vals)
    return spla.spsolve(A.tocsc(), rhs)


def bicgstab_jacobi(A, b, x0, rtol, atol=1e-50, max_it=1000):
    """Right-preconditioned BiCGStab with Jacobi, stopped on the recurrence |r| <= max(rtol |b|, atol) and then checked on the true
    residual (restart from it when it is not there yet) -- the algorithm of the device driver in plain NumPy.  As in stage 3 of
    sc_scal_kernel, a finite recurrence |r| within the tolerance is convergence whatever beta is (a solve that lands on the solution
    has s = t = 0, omega = 0, r = 0 and beta = 0 * inf); a beta that is not finite above the tolerance is a breakdown and ends the
    solve where it is."""
    A = sp.csr_matrix(A)
    dinv = 1.0 / A.diagonal()
    x = np.array(x0, dtype=np.float64)
    tol = max(rtol * np.linalg.norm(b), atol)
    its = 0
    r = b - A @ x
    broken = False
    while np.linalg.norm(r) > tol and its < max_it and not broken:
        rh, p, v = r.copy(), np.zeros_like(r), np.zeros_like(r)
        rho, rho_old, alpha, omega, beta = r @ r, 1.0, 1.0, 1.0, 0.0
        while its < max_it:
            p = r + beta * (p - omega * v)
            y = dinv * p
            v = A @ y
            alpha = rho / (v @ rh)
            sv = r - alpha * v
            z = dinv * sv
            t = A @ z
            tt = t @ t
            omega = (t @ sv) / tt if tt > 0 else 0.0
            x = x + alpha * y + omega * z
            r = sv - omega * t
            rho_old, rho = rho, rh @ r
            beta = (rho / rho_old) * (alpha / omega) if omega != 0 else np.inf
            its += 1
            if np.linalg.norm(r) <= tol:
                break
            if not np.isfinite(beta):
                broken = True
                break
        r = b - A @ x
    return x, its


def integral(x, cells, c):
    _, vol, _ = geometry(x, cells)
    return float(np.sum(vol * np.asarray(c)[np.asarray(cells)].mean(axis=1)))


def flux(x, cells, facet_cells, facet_local, facet_marker, marker, u, c):
    """int c (u . n) ds over the exterior facets of `marker`: n |F| = -d |K| grad(lambda_f), int_F l_a l_b = |F| (1 + d_ab) / (d (d+1))."""
    g, vol, _ = geometry(x, cells)
    cells = np.asarray(cells)
    d = cells.shape[1] - 1
    u = np.asarray(u, dtype=np.float64).reshape(-1, d)
    out = 0.0
    for q in np.nonzero(np.asarray(facet_marker) == marker)[0]:
        e, f = int(facet_cells[q]), int(facet_local[q])
        nF = -d * vol[e] * g[e, f]
        on = [a for a in range(d + 1) if a != f]
        for a in on:
            for b in on:
                out += c[cells[e, a]] * (u[cells[e, b]] @ nF) * (1.0 + (a == b)) / (d * (d + 1.0))
    return float(out)
