/*
 * cfdh.h -- C ABI of libcfdh.so: the MI355X (gfx950) implementation of the
 * per-time-step hot path of the reference's `stabilized_schur` solver.
 *
 * The reference has no C-level interface for this path: its boundary is the
 * duck-typed Python plugin surface
 *     Solver(mesh, dt, rho, mu, f, initial_velocity=None, **kw)
 *     Solver.setup(bcu, bcp, facet_tags=None, tags=None)
 *     Solver.solveStep()
 * (/root/reference/src/solvers/stabilized_schur.py:40-52,177-183,313 and
 * /root/reference/src/solverBase.py:25-40,96-102), behind which DOLFINx/PETSc
 * do the arithmetic.  Each entry point below cites the reference lines whose
 * work it performs; INTEGRATION.md shows the ctypes stub that binds them from
 * the reference's own `Solver` class.
 *
 * Conventions: every function returns 0 on success or a negative CFDH_E_*
 * code and never throws; cfdh_last_error() gives the message.  All pointer
 * arguments are caller-owned, C-contiguous host buffers that are copied at the
 * call; outputs are written into caller-allocated buffers.  One context per
 * GPU / per process rank; a context is not thread-safe.  Doubles are IEEE
 * binary64, indices int32 (sizes int64), as in the reference
 * (PETSc.ScalarType = float64, /root/reference/src/solverBase.py:37).
 *
 * Local numbering (multi-GPU): a context holds the vertices [0,nv) of its
 * part, the first nv_owned of them owned, the rest ghosts (the
 * ghost contract is stated at cfdh_create_elem_part).  Velocity arrays are vertex-major/component-minor
 * (u[gdim*v+i]), as DOLFINx lays out the blocked P1 space
 * (stabilized_schur.py:55-57).
 *
 * Dimension: gdim = 2 (triangles) or 3 (tetrahedra,
 * /root/reference/src/scenarios/simple_bifurcation.py, scenario_factory.py:47-49)
 * is fixed at cfdh_create; "d" below stands for it.  Tetrahedral contexts are
 * single-GPU in this version (cfdh_set_halo returns CFDH_E_ARG) and use pc_type 1 or 2
 * (pc_type 2 also on the degree-1 generic contexts of the rotational form, cfdh_set_schur_pcd).
 */
#ifndef CFDH_H
#define CFDH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFDH_ABI_VERSION 1

enum {
  CFDH_OK = 0,
  CFDH_E_ARG = -1,      /* bad argument (ValueError on the Python side) */
  CFDH_E_HIP = -2,      /* HIP runtime / device error */
  CFDH_E_STATE = -3,    /* call out of order (e.g. solve before set_params) */
  CFDH_E_DIVERGED = -4, /* Newton / Krylov did not converge (RuntimeError) */
  CFDH_E_COMM = -5,     /* RCCL / halo exchange failure */
  CFDH_E_NOMEM = -6
};

/* converged reasons, numbered after PETSc's SNESConvergedReason
 * (stabilized_schur.py:332-334 raises on reason < 0) */
enum {
  CFDH_CONVERGED_FNORM_ABS = 2,
  CFDH_CONVERGED_FNORM_RELATIVE = 3,
  CFDH_CONVERGED_SNORM_RELATIVE = 4,
  CFDH_DIVERGED_LINEAR_SOLVE = -3,
  CFDH_DIVERGED_MAX_IT = -5,
  CFDH_DIVERGED_LINE_SEARCH = -6,
  CFDH_DIVERGED_FNORM_NAN = -4
};
/* reasons of the linear solve (numbered after PETSc's KSPConvergedReason: 2 = CONVERGED_RTOL/ATOL on the true residual,
 * -3 = DIVERGED_ITS, -9 = DIVERGED_NANORINF).  One code has no PETSc counterpart: the solve was stopped ABOVE its tolerance
 * because two cycles in a row converged by the recurrence without moving the true residual (attainable accuracy of the
 * system; only within 10x the tolerance or below 1e-6 |b|).  Such stops are counted: cfdh_info(ctx, 72). */
enum {
  CFDH_KSP_CONVERGED_RTOL = 2,
  CFDH_KSP_CONVERGED_ATTAINABLE = 12,
  CFDH_KSP_DIVERGED_ITS = -3,
  CFDH_KSP_DIVERGED_NANORINF = -9
};

typedef struct cfdh_ctx cfdh_ctx;

typedef struct cfdh_options {
  /* Newton: PETSc SNES defaults, cap of stabilized_schur.py:270 */
  double snes_rtol, snes_atol, snes_stol;
  int32_t snes_max_it;
  /* outer FGMRES: PETSc KSP defaults, caps of stabilized_schur.py:272-273 */
  double ksp_rtol, ksp_atol;
  int32_t ksp_max_it, ksp_restart;
  /* GPU preconditioner (replaces PCFIELDSPLIT Schur FULL/SELFP + ILU(0),
   * stabilized_schur.py:231-264) */
  int32_t cheb_degree;      /* Jacobi-Chebyshev sweeps per A00 solve */
  double cheb_ratio;        /* lambda_max / lambda_min targeted */
  int32_t schur_full;       /* 2 (default): block UPPER-triangular factor (one A00 solve), 1: FULL
                             * factorisation as PC_FIELDSPLIT_SCHUR_FACT_FULL, stabilized_schur.py:225 (two A00
                             * solves), 0: LOWER.  All are right preconditioners of the same FGMRES. */
  int32_t amg_smooth_degree;
  double amg_smooth_ratio;
  double amg_theta;         /* strength threshold of the aggregation; < 0 (default): 0.07 for gdim 2, 0.02 for gdim 3 */
  int32_t amg_max_coarse;
  int32_t pc_refresh;       /* 0: adaptive lagging of the Sp hierarchy, n>0: every n steps, -1: every Jacobian */
  int32_t remove_p_mean;    /* nullsp.remove(x_n), stabilized_schur.py:319 */
  int32_t verbose;
  int32_t pc_type;          /* 0: SELFP Schur matrix + Chebyshev(A00) (the reference's SELFP, :235);
                             * 1: Cahouet-Chabard Schur approximation + AMG(A00) (mesh-independent);
                             * 2: pressure convection-diffusion (PCD) Schur approximation + AMG(A00), cfdh_set_schur_pcd */
  int32_t cc_smooth_degree; /* pc_type 1: Chebyshev steps on the mass-like operator H (default 2) */
  int32_t ksp_guess;        /* initial guess of the linear solves (PETSc: KSPGuess, -ksp_guess_type fischer): for each Newton index the
                             * corrections of the last ksp_guess time steps are kept (at the end of a step: iterate minus converged
                             * solution) and the new solve starts from their best combination, x0 = U y with
                             * y = argmin |b - J U y| on the CURRENT Jacobian (so |r0| <= |b|); convergence is still tested against
                             * rtol |b|.  0: zero initial guess (what the reference's KSP does); default 4.  Converged results do
                             * not depend on it, iteration counts do. */
} cfdh_options;

typedef struct cfdh_stats {
  int32_t newton_its, krylov_its, reason, pc_refreshes;
  double fnorm0, fnorm;
  double ms_assemble, ms_solve, ms_pc_setup, ms_total;
} cfdh_stats;

/* ---- life cycle --------------------------------------------------------- */

/* Upload a (part of a) P1 triangle or tetrahedron mesh and build the fixed CSR pattern.
 * Replaces: functionspace/Function/create_matrix_block/create_vector_block
 * (solverBase.py:104-142, stabilized_schur.py:55-57,191-193) and the DG0 cell
 * size h = mesh.h (stabilized_schur.py:82-88).
 * gdim 2 or 3.  cells [nc][gdim+1] (any orientation); coords [nv][gdim];
 * exterior facets: owning cell, local facet index (= local index of the
 * opposite vertex), marker (0 = untagged; facet_marker may be NULL, see
 * cfdh_set_facet_markers). */
int cfdh_create(cfdh_ctx **out, int device, int gdim, int64_t nv, int64_t nv_owned, int64_t nc,
                const int32_t *cells, const double *coords, int64_t nfacets, const int32_t *facet_cells,
                const int32_t *facet_local, const int32_t *facet_marker);
/* The same for nodal equal-order elements beyond P1 simplices: `p_grade = 2` of
 * stabilized_schur_backflow.py:84-87 (P2/P2 triangles on a straight-sided triangulation) and quadrilateral cells as
 * unit_square_pipe.py:101-105 builds them (Q1/Q1; parallelograms only: the geometry map must be affine).
 * cells [nc][nloc] list NODE ids in the DOLFINx/Basix local order -- P2 triangle: vertices 0,1,2 then the edge nodes opposite
 * to them (nloc 6); Q1 quadrilateral: (0,0),(1,0),(0,1),(1,1) (nloc 4); node_coords [nn][2].  Local facets: triangle f =
 * opposite vertex f; quadrilateral 0:(0,1) 1:(0,2) 2:(1,3) 3:(2,3).  Every node carries (u_x, u_y, p): all other calls take
 * node ids / per-node arrays where they say vertex.  gdim 3 (round 4): CFDH_ELEM_Q1 = hexahedral cells as unit_cube_pipe.py:103-109
 * builds them (parallelepipeds; nloc 8, vertex v = i + 2 j + 4 k, local facets 0:(0,1,2,3) 1:(0,1,4,5) 2:(0,2,4,6) 3:(1,3,5,7)
 * 4:(2,3,6,7) 5:(4,5,6,7)), CFDH_ELEM_P2 = P2/P2 tetrahedra (nloc 10: vertices, then the edge nodes in Basix edge order (2,3) (1,3) (1,2)
 * (0,3) (0,2) (0,1); facet f opposite vertex f); node_coords [nn][3].  This entry point creates a whole mesh on one GPU (parts of a
 * partitioned run: cfdh_create_elem_part).  CFDH_ELEM_P1_GENERIC runs P1 triangles / tetrahedra through the
 * quadrature kernels of the P2/Q1 path (a cross-check of the closed-form P1 kernels). */
enum { CFDH_ELEM_P1 = 0, CFDH_ELEM_P2_TRIANGLE = 1, CFDH_ELEM_Q1_QUADRILATERAL = 2, CFDH_ELEM_P1_GENERIC = 3 };
int cfdh_create_elem(cfdh_ctx **out, int device, int gdim, int elem, int64_t nn, int64_t nc, const int32_t *cells,
                     const double *node_coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local,
                     const int32_t *facet_marker);
/* The same for one part of a partitioned run (SURVEY.md 8e for the 8f-4 elements: the reference runs every solver under
 * mpirun, /root/reference/src/simulation_hpc.sh:14-19): nodes [0, nn_owned) are owned, the rest are ghost nodes, numbered
 * contiguously per neighbour as cfdh_set_halo expects.  Any ghost set that is closed under the halo plan is accepted (one layer
 * of cells around the owned nodes, or more: PartComm.make_part passes two by default); cells = the cells of the part, of which
 * those of a deeper layer touch no owned node.  Rows are assembled for owned nodes only, and a cell is integrated in global
 * functionals by the rank that owns its first node.  This holds for every builder (cfdh_create with nv_owned < nv included). */
int cfdh_create_elem_part(cfdh_ctx **out, int device, int gdim, int elem, int64_t nn, int64_t nn_owned, int64_t nc, const int32_t *cells,
                          const double *node_coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local,
                          const int32_t *facet_marker);
/* (Re)assign the markers of the exterior facets after cfdh_create: the reference hands `facet_tags` / `tags` to
 * Solver.setup(), not to the constructor (/root/reference/src/scenario.py:137-149;
 * stabilized_schur_backflow.py:158-163 builds ds_out from them there).  markers[nfacets] in the facet order of
 * cfdh_create (nfacets must equal its nfacets; a rank keeps the entries of the facets whose cell it holds).
 * Drag/lift by marker (cfdh_functional) and the backflow marker of cfdh_set_boundary_terms follow the new values;
 * an active backflow term invalidates Jacobian and preconditioner. */
int cfdh_set_facet_markers(cfdh_ctx *ctx, int64_t nfacets, const int32_t *markers);
void cfdh_destroy(cfdh_ctx *ctx);
const char *cfdh_last_error(const cfdh_ctx *ctx); /* ctx may be NULL after a failed create */
int cfdh_abi_version(void);

/* dt, rho, mu Constants and body force (solverBase.py:36-40; f[2] is read for gdim 3 only); mu_facet is the
 * raw python float used in the ds term (stabilized_schur.py:79). */
int cfdh_set_params(cfdh_ctx *ctx, double dt, double rho, double mu, double mu_facet, const double f[3]);
int cfdh_default_options(cfdh_options *opt);
int cfdh_set_options(cfdh_ctx *ctx, const cfdh_options *opt);

/* ---- Dirichlet data ------------------------------------------------------ */

/* Drop all DirichletBC objects (stabilized_schur.py:198-199 rebuilds them in setup). */
int cfdh_clear_dirichlet(cfdh_ctx *ctx);
/* Append one DirichletBC object (boundaryCondition.py:41-52): field 0 = velocity
 * (values [n][gdim]), 1 = pressure (values [n]).  A later object overrides the
 * value of a shared dof; the matrix diagonal counts the objects holding it.
 * Re-callable every step (bc.update(), stabilized_schur.py:170). */
int cfdh_add_dirichlet(cfdh_ctx *ctx, int field, int64_t n, const int32_t *nodes, const double *values);
/* New VALUES for dofs that are already constrained (`bc.update()` of a time-dependent condition, stabilized_schur.py:170, when
 * the dof sets of all objects are unchanged): no object is added, the matrix diagonal keeps its counts, only the listed
 * vertices are re-sent to the device.  The caller passes the dofs whose value this object determines (a later object that
 * holds the same dof keeps its value).  CFDH_E_ARG if a listed dof is not constrained. */
int cfdh_update_dirichlet(cfdh_ctx *ctx, int field, int64_t n, const int32_t *nodes, const double *values);

/* ---- state ---------------------------------------------------------------- */

/* u_prev/p_prev (solverBase.py:121,139) and the Newton iterate x_n = (u,p)
 * (stabilized_schur.py:216-223).  NULL keeps the device copy.  Arrays cover
 * all nv local vertices (ghost entries are overwritten by the halo exchange). */
int cfdh_set_state(cfdh_ctx *ctx, const double *u_prev, const double *p_prev, const double *u, const double *p);
/* u_sol/p_sol after the step = the Newton iterate (updateSolution, :125-142) */
int cfdh_get_solution(cfdh_ctx *ctx, double *u, double *p);
/* u_prev/p_prev as held on the device (after cfdh_advance they equal the last solution) */
int cfdh_get_previous(cfdh_ctx *ctx, double *u_prev, double *p_prev);
/* u_residual/p_residual (_updateResidual, :295-311) */
int cfdh_get_residual(cfdh_ctx *ctx, double *ru, double *rp);
/* device-side u_prev <- u_sol, p_prev <- p_sol (scenario.py:306-307) */
int cfdh_advance(cfdh_ctx *ctx);
/* one line of that copy: field 0: u_prev <- u_sol (scenario.py:306), field 1: p_prev <- p_sol (:307); lets a binding
 * map the reference's literal `u_prev.x.array[:] = u_sol.x.array[:]` onto the device without a host round trip */
int cfdh_advance_field(cfdh_ctx *ctx, int field);

/* ---- time scheme (the `stabilized_schur_bdf2` variant) ------------------------ */

/* Spatial terms are evaluated at theta*u + (1-theta)*u_prev and the time term is
 * (a0*u + a1*u_prev + a2*u_prev2)/dt.  Default (1/2; 1,-1,0) is the midpoint form of
 * stabilized_schur.py:72-80.  stabilized_schur_bdf2.py:79-80 (u_mid = u_sol) and :95-110,
 * :298-305 (a0,a1,a2 Constants switched by step_count) map to (1; 1,-1,0) on the first
 * step and (1; 1.5,-2,0.5) afterwards.  theta in (0,1], a0 > 0. */
int cfdh_set_time_scheme(cfdh_ctx *ctx, double theta, double a0, double a1, double a2);
/* ---- boundary terms (the `stabilized_schur_backflow` variant) --------------------- */

/* ds_terms != 0 (default): the pair `dot(p n, v) ds - dot(mu grad(u_mid) n, v) ds` of
 * stabilized_schur.py:79 on ALL exterior facets.  stabilized_schur_backflow.py:107 drops it
 * (do-nothing outlet): ds_terms = 0.  beta > 0 adds the backflow stabilisation
 * -beta rho (u_prev.n)_- (u_mid . v) ds, (s)_- = (s-|s|)/2, on the exterior facets whose marker
 * (facet_marker of cfdh_create) equals backflow_marker (`ds_out`, tags["outlet"],
 * stabilized_schur_backflow.py:158-176), integrated with a rule of FFCx's estimated degree 3:
 * 2-point Gauss on edges, the 6-point Strang-Fix rule on the triangles of a tetrahedral mesh.  CFDH_E_ARG for beta > 0 on a
 * rotational context: the rotational form takes its backflow term per pressure boundary, cfdh_set_pressure_boundaries_ex. */
int cfdh_set_boundary_terms(cfdh_ctx *ctx, int ds_terms, int backflow_marker, double beta);

/* ---- pressure-driven flow (the `stabilized_schur_pressurebc` / `_vascularbc` variants) -------- */

/* Weak form assembled by the generic element kernels.  CFDH_FORM_CONVECTIVE (default): the form of stabilized_schur.py:67-123.
 * CFDH_FORM_ROTATIONAL: the curl-curl / rotational form of stabilized_schur_pressurebc.py:111-160, with omega = curl(u_mid) --
 *   rho w_t . v + mu omega . curl(v) - p div v + rho (omega x u_mid) . v - rho/2 |u_mid|^2 div v - rho f . v + q div u_mid
 *   + SUPG / PSPG / LSIC with the strong residual R = rho (w_t + omega x u_mid) + grad p - rho f (no viscous part).
 * In gdim 2 omega = d_x u_y - d_y u_x is a scalar and omega x a = (-omega a_y, omega a_x).  The time scheme of
 * cfdh_set_time_scheme applies as before.  Contexts: gdim 2 on the generic kernels, gdim 3 for CFDH_ELEM_P2 (tetrahedra) and
 * CFDH_ELEM_Q1 (hexahedra).  CFDH_E_ARG on the closed-form P1 path (gdim 2: create the context with CFDH_ELEM_P1_GENERIC), for
 * P1 tetrahedra in gdim 3 (closed-form or generic), on a part of a partitioned run, with an active backflow term of
 * cfdh_set_boundary_terms (beta > 0: the rotational form takes its backflow term per pressure boundary,
 * cfdh_set_pressure_boundaries_ex), and when switching back to the convective form while pressure boundaries are set.  A change invalidates Jacobian and
 * preconditioner. */
enum { CFDH_FORM_CONVECTIVE = 0, CFDH_FORM_ROTATIONAL = 1 };
int cfdh_set_formulation(cfdh_ctx *ctx, int form);
/* Natural pressure boundaries of the rotational form (stabilized_schur_pressurebc.py:177-205): on the exterior facets whose marker
 * is markers[k] (k < n <= 8, distinct), with outward normal n, w_T = w - (w . n) n, omega = curl(u_mid) and the owning cell's size
 * h (largest vertex distance),
 *   + values[k] v . n  - mu (omega x n) . v_T - mu (curl(v) x n) . u_mid_T + (beta_nitsche mu / h) u_mid_T . v_T;
 * in gdim 2, with the tangent t = (-n_y, n_x): values[k] v . n - mu omega (t . v) - mu omega(v) (t . u_mid)
 * + (beta_nitsche mu / h) (t . u_mid)(t . v).
 * values[k] enters the residual only (the caller passes the reference's halved values, e.g. p_inlet / 2).  The facets follow later
 * cfdh_set_facet_markers calls.  A call that changes only `values` keeps Jacobian and preconditioner valid (the per-step resistance
 * update of the vascular outlet); any other change invalidates both.  n = 0 removes the terms.  Requires CFDH_FORM_ROTATIONAL
 * (and the contexts it allows).  Use with ds_terms = 0 (cfdh_set_boundary_terms): the preconditioner's pressure Laplacian then
 * takes Dirichlet rows on every exterior facet that is not fully velocity-constrained, the pressure boundaries among them. */
int cfdh_set_pressure_boundaries(cfdh_ctx *ctx, int n, const int32_t *markers, const double *values, double beta_nitsche);
/* The same with two per-boundary switches (the outlet of stabilized_schur_vascularbc_backflow.py:214-244 is a pure traction boundary
 * with backflow stabilisation).  nitsche[k] == 0 drops the three tangential terms on boundary k, which keeps values[k] v . n alone;
 * NULL: all on.  beta_backflow[k] > 0 adds on boundary k
 *   - beta_backflow[k] rho (u_prev . n)_- (u_mid . v),   (s)_- = (s - |s|) / 2
 * (Moghadam et al. 2011, eq. 10; the same term as cfdh_set_boundary_terms adds to the convective form), coefficient from u_prev,
 * so the Jacobian gains theta (-beta_backflow[k] rho (u_prev . n)_-) phi_a phi_b delta_ij in A00; integrated with the facet rule of
 * the pressure terms.  NULL: all 0.  CFDH_E_ARG for a negative or non-finite beta_backflow[k].  cfdh_set_pressure_boundaries is
 * this call with both arrays NULL.  A call that changes only `values` keeps Jacobian and preconditioner valid; a change of
 * nitsche[k] or beta_backflow[k] invalidates both, as a marker change does. */
int cfdh_set_pressure_boundaries_ex(cfdh_ctx *ctx, int n, const int32_t *markers, const double *values, double beta_nitsche,
                                    const uint8_t *nitsche, const double *beta_backflow);

/* ---- pressure-driven flow on the closed-form P1 kernels (the `stabilized_schur_pressure_backflow` variant) -------- */

/* Traction boundaries of the CONVECTIVE form (stabilized_schur_pressure_backflow.py:191-217; its volume form is the one of
 * stabilized_schur_backflow.py, which the closed-form kernels assemble).  On the exterior facets whose marker is markers[k]
 * (k < n <= 8, distinct), with outward normal n, ubar = theta u + (1 - theta) u_prev of the time scheme in force,
 * w_T = w - (w . n) n and the owning cell's size h (largest vertex distance, the h of tau), F_v gains
 *   always                 + values[k] int v . n                                                          (residual only)
 *   tangential[k] != 0     - int (2 mu eps(ubar) n) . v_T - int (2 mu eps(v) n) . ubar_T + (beta_nitsche mu / h) int ubar_T . v_T
 *                          (the weak pressure inlet with its Nitsche tangential condition, :191-201)
 *   tangential[k] == 0     - int (2 mu eps(ubar) n) . v                                          (the outlet, :208-209)
 *   beta_backflow[k] > 0   - beta_backflow[k] rho int (u_prev . n)_- ubar . v,  (s)_- = (s - |s|) / 2        (:213-217)
 * tangential NULL: all on; beta_backflow NULL: all 0.  The backflow term is integrated with the facet rule of
 * cfdh_set_boundary_terms (2-point Gauss on edges, 6-point Strang-Fix on triangles), everything else in closed form.  The
 * Jacobian is theta times the ubar-derivative; all of it lies in A00 on couplings of the vertices of one cell (the symmetry term
 * reaches the row of the vertex opposite the facet as well).  values[k] and the pressure do not enter it: the caller passes the
 * value the form should see (the reference's outlet passes p_c / 2).  One extra kernel per assembly, behind the volume pass; a
 * context without traction boundaries never launches it (cfdh_info 93: boundaries set, 94: launches since creation).
 * A call that changes only `values` keeps Jacobian and preconditioner valid; any other change, and a cfdh_set_facet_markers call
 * while boundaries are set, invalidates both.  n = 0 removes the terms.
 * Contexts: closed-form P1 contexts of cfdh_create (gdim 2 and 3), the whole mesh on one GPU, CFDH_FORM_CONVECTIVE, ds_terms = 0
 * and no backflow term of cfdh_set_boundary_terms.  CFDH_E_ARG, with the context unchanged, on generic-element contexts, on
 * contexts of cfdh_create_ipcs, on a part of a partitioned run, in the rotational form, with ds_terms != 0 or an active backflow
 * term, for non-finite or negative coefficients, non-finite values and duplicate markers.  While boundaries are set,
 * cfdh_set_boundary_terms with ds_terms != 0 or beta > 0 and cfdh_set_formulation(CFDH_FORM_ROTATIONAL) return CFDH_E_ARG.
 * With ds_terms = 0 the preconditioner's pressure Laplacian takes Dirichlet rows on the open facets, these boundaries included. */
int cfdh_set_traction_boundaries(cfdh_ctx *ctx, int n, const int32_t *markers, const double *values, double beta_nitsche,
                                 const uint8_t *tangential, const double *beta_backflow);

/* ---- pressure convection-diffusion preconditioner and forcing (the `stabilized_pcd` variant) ---------------- */

/* Data of the PCD Schur approximation selected by cfdh_options.pc_type = 2 (fenicsx_pctools.pc.PCDPC_vY of
 * /root/reference/src/solvers/stabilized_pcd.py:204-276, restated -- DESIGN.md section 9).  With theta, a0 of cfdh_set_time_scheme,
 * w = theta u + (1 - theta) u_prev at the current Newton iterate and the P1 pressure basis phi:
 *   M_d = diagonal of the consistent P1 mass matrix (the reference's Jacobi on M_p, :273-274);
 *   K   = rho N(w) - rho R_in(w) + c_t M,  N_ij = int phi_i (w . grad phi_j) dx,  R_in,ij = int_{inlet} (w . n) phi_i phi_j ds over the
 *         exterior facets whose marker is inlet_marker (ds_in, :220-231), M the consistent mass, c_t = rho a0 / (theta dt) when
 *         time_term = 1, 0 when time_term = 0 (the reference's literal operator);
 *   A_p = the P1 pressure Laplacian with Dirichlet rows on every vertex of a facet marked outlet_marker (bcs_pcd, :215-218) and on
 *         the pressure-Dirichlet vertices, applied as one AMG V-cycle (the reference: CG + hypre, :275-276);
 *   z_p = mu t + y,  t = M_d^-1 r_p,  s = K t (0 on the Dirichlet rows of A_p),  y = A_p^-1 s (0 on those rows);  z_p = r_p on the
 *         pressure-Dirichlet rows of the Jacobian.
 * In this library's convention S = A11 - A10 A00^-1 A01 is positive; the reference's -(I + A_p^-1 K_p) M_p^-1 with K_p = K / mu (no
 * time term) differs by the factor -1/mu.  K is assembled from the current iterate in every preconditioner update, once per Newton
 * iteration.  One GPU.  Contexts: P1 triangles and tetrahedra on the closed-form kernels (cfdh_create), and the degree-1 cells of the
 * rotational form on the generic element kernels -- CFDH_ELEM_P1_GENERIC triangles, CFDH_ELEM_Q1 parallelograms (gdim 2) and
 * parallelepipeds (gdim 3) -- once cfdh_set_formulation(CFDH_FORM_ROTATIONAL) has been called; there "P1" above reads "the element's
 * own", the vertices are the nodes, and cfdh_set_formulation refuses to go back to the convective form while this data is set.
 * CFDH_E_ARG on generic-element contexts in the convective form, on P2 contexts and on parts of a partitioned run; pc_type 2
 * without this call fails with CFDH_E_STATE at the solve. */
int cfdh_set_schur_pcd(cfdh_ctx *ctx, int inlet_marker, int outlet_marker, int time_term);
/* Eisenstat-Walker forcing of the linear tolerance (snes_ksp_ew, stabilized_pcd.py:249).  version 0: off (default; ksp_rtol of
 * cfdh_options for every solve).  version 2 (PETSc's default variant; its defaults 0.3, 0.9, 1.0, (1 + sqrt 5)/2, 0.1): the first
 * solve of a step uses rtol_0; after that rtol_k = gamma (|F_k| / |F_k-1|)^alpha, raised to gamma rtol_k-1^alpha when that exceeds
 * threshold, then capped at rtol_max.  ksp_atol and ksp_max_it keep their meaning. */
int cfdh_set_ksp_forcing(cfdh_ctx *ctx, int version, double rtol_0, double rtol_max, double gamma, double alpha, double threshold);
/* Per Newton iteration of the last cfdh_solve_step: |F| at the iterate, the linear tolerance used, the FGMRES iterations (a solve
 * retried after a hierarchy rebuild counts both attempts) and the achieved true |r| / |b| of the accepted solve.  *n receives the count; arrays may be NULL (query) or hold *n entries. */
int cfdh_get_newton_history(cfdh_ctx *ctx, int32_t *n, double *fnorm, double *ksp_rtol, int32_t *ksp_its, double *ksp_rel_res);
/* K of cfdh_set_schur_pcd, assembled from the current state (cfdh_set_state), as CSR of the owned rows in user numbering (columns
 * ascending), and M_d (mass_diag[nv_owned], may be NULL).  Query convention of cfdh_get_csr (nnz first with rowptr = col = vals =
 * NULL).  The contexts of cfdh_set_schur_pcd, CFDH_E_ARG elsewhere.  Exposed for parity tests, like cfdh_spmv. */
int cfdh_get_pcd_operator(cfdh_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals, double *mass_diag);
/* z = P^-1 r with the current preconditioner (built, and for pc_type 2 with K assembled, at the current state when needed) on the
 * assembled Jacobian; r, z monolithic [gdim*nv | nv] as for cfdh_spmv.  Exposed for parity tests. */
int cfdh_apply_preconditioner(cfdh_ctx *ctx, const double *r, double *z);
/* The operator of one FGMRES iteration, launched exactly as the solver launches it: z = P^-1 r, then w = J z on the solver's
 * stream (r, z as for cfdh_apply_preconditioner, w as y of cfdh_spmv).  On the lean solve path (environment CFDH_SOLVE_LEAN, default
 * on, read by cfdh_create; 0 selects the general paths) the product reuses A01 z_p from the preconditioner application instead of
 * reading that block again.  Exposed for tests. */
int cfdh_apply_operator(cfdh_ctx *ctx, const double *r, double *z, double *w);

/* ---- read-only view of the built preconditioner (parity tests) ---------------------------------------------------------
 * hier: which hierarchy; level: 0 = finest (ignored for CFDH_AMG_HIER_H, which has one level). */
#define CFDH_AMG_HIER_A 0 /* scalar proxy of the velocity block (pc_type 1, 2) */
#define CFDH_AMG_HIER_P 1 /* pressure hierarchy: the Laplacian (pc_type 1, 2) or the SELFP Schur matrix (pc_type 0) */
#define CFDH_AMG_HIER_H 2 /* the single level H of the Cahouet-Chabard approximation */
#define CFDH_AMG_HIER_PG 3  /* partitioned run: the replicated hierarchy of the global pressure space (every rank holds all of it; level 0 in
                              the global vertex ids of cfdh_set_global_pressure_space) */
#define CFDH_AMG_HIER_DL0 4 /* partitioned run: this rank's share of level 0 of CFDH_AMG_HIER_PG, the distributed finest level (level ignored):
                              CFDH_AMG_OP_A [owned x local], CFDH_AMG_OP_P [local x level 1], CFDH_AMG_OP_PT [level 1 x owned] */
#define CFDH_AMG_OP_A 0   /* level operator */
#define CFDH_AMG_OP_P 1   /* prolongator to the next level */
#define CFDH_AMG_OP_G 2   /* G = P^T (I - A W) */
#define CFDH_AMG_OP_SB 3  /* Sb = 2W - W A W */
#define CFDH_AMG_OP_SC 4  /* Sc = (I - W A) P */
#define CFDH_AMG_OP_PT 5  /* CFDH_AMG_HIER_DL0: the restriction, P^T of the owned rows; the entries of a row in the order they are summed in */
/* One operator of one level as CSR with ascending columns.  Query convention of cfdh_get_csr: with rowptr = col = vals = NULL
 * only *nrow, *ncol, *nnz are set.  Indices that number level 0 are returned in the caller's node numbering (as
 * cfdh_get_pcd_operator does; the entries of such a row are re-sorted after the renumbering, so the stored order of its columns
 * is not visible to the caller, duplicates are), coarse indices as stored.  On one part of a partitioned run the hierarchies are this
 * rank's: local numbering (owned nodes, then ghosts), the velocity hierarchy on owned + ghost nodes where the overlapping cycle runs,
 * H and the rank's own pressure hierarchy on the owned nodes.  Rank-local: no exchange runs inside a getter.  CFDH_E_STATE on a
 * pressure-correction context, before the preconditioner exists, and for an operator the build did not keep: the device build
 * releases P (one GPU) and the aggregate ids unless CFDH_AMG_KEEP=1 is in the environment when the hierarchy is built. */
int cfdh_get_amg_operator(cfdh_ctx *ctx, int hier, int level, int which, int64_t *nrow, int64_t *ncol, int64_t *nnz, int32_t *rowptr,
                          int32_t *col, double *vals);
#define CFDH_AMG_VEC_DINV 0        /* 1 / a_ii of the level [n] */
#define CFDH_AMG_VEC_WDINV 1       /* Jacobi weight times dinv [n] */
#define CFDH_AMG_VEC_AGG 2         /* aggregate ids [n], -1: row without coarse correction (needs CFDH_AMG_KEEP=1) */
#define CFDH_AMG_VEC_COARSE_INV 3  /* dense inverse of the coarsest operator, row-major [coarse_n^2] (level ignored; level 0 in a hierarchy of one level) */
#define CFDH_AMG_VEC_D 4           /* folded dense correction D = Sc A_c^-1 of the level, row-major [n x Dn], fp32 widened */
#define CFDH_AMG_VEC_LAMBDA 5      /* lmax, lmin of the level [2] */
#define CFDH_AMG_VEC_CC_SCALARS 6  /* cc_alpha, cc_beta [2] */
#define CFDH_AMG_VEC_CC_ML 7       /* lumped pressure mass, 0 on the Dirichlet rows of the pressure hierarchy [nv] */
#define CFDH_AMG_VEC_CC_PBC 8      /* their flags [nv] */
#define CFDH_AMG_VEC_SPGEMM_ROWS 9 /* rows the last device build of the hierarchy gave to the hash / small / dense kernels [3] */
#define CFDH_AMG_VEC_SHAPE 10      /* levels, coarse_n, right-hand sides per cycle, fused; then per level n, Dn, fine, sell, has agg */
#define CFDH_AMG_VEC_ORDER 11      /* position of every row of the level in the library's own numbering [n] (level 0: the node permutation;
                                      the fixed start vector of the spectral estimate is indexed by it) */
#define CFDH_AMG_VEC_A00_LMAX 12   /* pc_type 0: the spectral bound lmaxA of D^-1 A00 used by the Chebyshev solve [1] */
#define CFDH_AMG_VEC_A00_DINV 13   /* pc_type 0: 1 / diag(A00), [gdim nv] as the velocity part of a monolithic vector */
#define CFDH_AMG_VEC_DL0_SHAPE 14  /* CFDH_AMG_HIER_DL0 (which also answers WDINV [local] and ORDER): n1, ghost layer of the right-hand side exchanged,
                                      SELL taken by the pre-sweep / post-sweep / prolongation, fused cycle on the replicated levels, owned, local [8] */
/* Vectors and scalars of the same, as doubles; *n receives the count, out may be NULL (query).  Level-0 vectors in the caller's
 * numbering.  Error codes as above. */
int cfdh_get_amg_vectors(cfdh_ctx *ctx, int hier, int level, int which, int64_t *n, double *out);
/* Head copy of one SELL-64 operator (tests): *width = entries per row that a sweep addresses from the slice index alone, 0 when the
 * operator has no head.  which: CFDH_AMG_OP_SB / _SC of a hierarchy level, CFDH_AMG_OP_A of CFDH_AMG_HIER_H (the Chebyshev matrix).
 * Error codes as above. */
int cfdh_get_amg_head(cfdh_ctx *ctx, int hier, int level, int which, int32_t *width);

/* ---- one Krylov vector kernel at a time (tests) ---------------------------------------------------------------------------
 * The small vector kernels of the linear solve (dot products, Gram-Schmidt updates, the fp32 basis copy, the prologue of the
 * projected guess, axpy-style updates) behind the wrapper the solver itself calls, on the context's stream. */
#define CFDH_KVOP_DOT 0                  /* host[0] = x . y */
#define CFDH_KVOP_NORM2 1                /* host[0] = |x| */
#define CFDH_KVOP_NORM2_PAIR 2           /* host = |x|, |y|; dev / mirror hold the squares */
#define CFDH_KVOP_NORM2_TRIPLE 3         /* host = |x|, |y|, |A_0| */
#define CFDH_KVOP_NORMINF_DIFF 4         /* host[0] = max |x - y| (flags 1) or max |x| */
#define CFDH_KVOP_SUB_MEAN 5             /* out1 = x - mean(x); dev[0] = sum(x) */
#define CFDH_KVOP_NORM_SCALE_INV 6       /* dev[0] = |x| left on the device, out1 = x / dev[0] (zeros for a zero norm) */
#define CFDH_KVOP_MULTIDOT 7             /* dev[v] = A_v . x for v < nvec, dev[nvec] = x . x with flags 1; mirrored */
#define CFDH_KVOP_MULTIDOT32 8           /* the same against the fp32 copy of A, x . x always; mirrored */
#define CFDH_KVOP_GRAM 9                 /* dev[8 i + q] = A_q . A_i (i < nvec), dev[8 nvec + q] = A_q . x; nvec = k in 1 .. 8 */
#define CFDH_KVOP_MULTIAXPY 10           /* out1 = x - sum coef_v A_v */
#define CFDH_KVOP_LINCOMB 11             /* out1 = x + sum coef_v A_v */
#define CFDH_KVOP_LINCOMB_KEEP 12        /* the same, stored in out1 and out2 */
#define CFDH_KVOP_GS_UPDATE_NORMALIZE 13 /* out1 = (x - sum coef_v A_v) / s, dev[0] = s from coef[nvec] = x . x and |coef|^2 */
#define CFDH_KVOP_GS_UPDATE32 14         /* the same against the fp32 copy with the measured norm: out1, out32, dev[0] = mirror[nvec + 1] = s */
#define CFDH_KVOP_STORE32 15             /* out32 = (float)x */
#define CFDH_KVOP_GUESS 16               /* coef = Gram slots of nvec = k kept vectors: out1 = A y, out2 = x - B y (flags 1: divided by
                                            its norm on the device); host = |out2|, used, rank, y; dev = |out2|^2, y; mirror = |out2|^2, used, rank, y */
#define CFDH_KVOP_AXPY 17                /* out1 = y + scalar x */
#define CFDH_KVOP_WAXPY 18               /* the same through the three-vector kernel */
#define CFDH_KVOP_SCALE 19               /* out1 = scalar x, in place */
#define CFDH_KVOP_SCALE_TO 20            /* out1 = scalar x */
#define CFDH_KVOP_PMULT 21               /* out1 = x y entry by entry */
#define CFDH_KVOP_COUNT 22
/* Runs ONE op: A and B are column-major blocks [ld * nvec], x and y vectors [n], coef the op's coefficients; every array the op does
 * not use may be NULL.  Each array gets a device allocation of its own for the call (ld entries per column, zero behind n), the
 * wrapper runs on the solver's stream exactly as the solver calls it, and the results come back: out1 / out2 [n], out32 [n],
 * scal_host (what the wrapper returned to its caller), scal_dev (the scalars it left on the device) and scal_mirror (the
 * host-mapped words the host reads instead of a copy: behind the context's scalar mirror, or with flags 2 in a slot of the FGMRES
 * read-back ring), with their counts in nscal[3].  The three scalar arrays hold max(nvec + 2, 72) entries.  Nothing of the call
 * stays in the context, and no solver state changes.  Arguments the solver never produces are refused with CFDH_E_ARG before
 * anything is launched: n < 1, nvec < 1, ld < n, an odd ld, an ld that is no multiple of 4 for the fp32 ops, nvec above 8 for
 * CFDH_KVOP_GRAM and CFDH_KVOP_GUESS.  One GPU only (CFDH_E_STATE on a partitioned or pressure-correction context).  Exposed for tests. */
int cfdh_krylov_vec_op(cfdh_ctx *ctx, int op, int n, int ld, int nvec, const double *A, const double *B, const double *x, const double *y,
                       const double *coef, double scalar, int flags, double *out1, double *out2, float *out32, int32_t *nscal,
                       double *scal_host, double *scal_dev, double *scal_mirror);

/* ---- incremental pressure correction on P2/P1 Taylor-Hood elements (the `ipcs_bdf2` solver) -------------------------- */

/* The second solver family of the reference (/root/reference/src/solvers/ipcs_bdf2.py:66-91,127-172): P2 velocity / P1 pressure,
 * linear, three solves per step.  With the P2 basis phi, the P1 basis psi, w = 1.5 u_prev - 0.5 u_n1, per velocity component
 * (the d components share ONE scalar matrix on the P2 node graph):
 *   1. A1 u* = b1,  A1 = rho/dt M + c/2 N(w) + mu/2 K,  b1 = (rho/dt M - c/2 N(w) - mu/2 K) u_prev + B^T p_sol + s_f F,
 *      N_ij = int phi_i (w . grad phi_j), (B_d)_ij = int psi_i d_d phi_j, F_i = f int phi_i; velocity Dirichlet objects as
 *      cfdh_add_dirichlet documents them (lifting, identity rows whose diagonal counts the objects, later object wins; the
 *      right-hand side of such a row is count * value).  BiCGStab + Jacobi on the interleaved d-component vector.
 *   2. L phi = -rho/dt sum_d B_d u*_d, L the P1 stiffness matrix with the pressure Dirichlet objects applied the same way (the
 *      object's VALUE goes into phi: right for homogeneous data only, as in the reference); p_sol += phi.  Flexible PCG
 *      preconditioned by one V-cycle of the smoothed-aggregation hierarchy.  Without a pressure Dirichlet object the problem is
 *      solved mean-free (right-hand side and phi have zero mean).
 *   3. rho M u_sol = rho M u* - dt G phi, (G_d)_ij = int phi_i d_d psi_j, no boundary condition.  CG + Jacobi.
 *   4. u_n1 <- u_prev.
 * Every solve stops on the true residual, |b - A x| <= max(rtol |b|, atol); phi starts from zero, steps 1 and 3 from the previous
 * step's u* / u_sol.
 *
 * cells [nc][6 | 10] list the P2 nodes in the local order of cfdh_create_elem; the vertices must be the nodes [0, nvert) (the
 * pressure lives there), the edge nodes the rest; node_coords [nn][gdim]; exterior facets as for cfdh_create.  One GPU.
 * A context of this kind answers cfdh_set_params, cfdh_clear / add / update_dirichlet (field 0: P2 node ids, field 1: vertex
 * ids), cfdh_set_state / cfdh_get_solution / cfdh_get_previous (velocity arrays [nn][gdim], pressure arrays [nvert]; cfdh_set_state
 * with u, p sets u_sol, p_sol), cfdh_set_previous2 / cfdh_get_previous2 (u_n1), cfdh_advance, cfdh_advance_field,
 * cfdh_set_facet_markers, cfdh_functional (kinds 2-6; 0 / 1 for gdim 2 with P2 velocity gradients and P1 pressure),
 * cfdh_wall_shear_stress, cfdh_wall_stats_reset / accumulate / get,
 * cfdh_info (0, 1: nn; 2: nc; 3: entries of A1; 6: levels of the pressure hierarchy; 15: host synchronisations and 80: kernel
 * launches of the last step; 81: nvert; 82: whole-field host copies since creation; 83: 1 (the context kind); 84 and 90:
 * accumulations of the wall shear indices since the last reset; 91: the scheme and 92: assemblies of A1 since creation, see
 * cfdh_ipcs_set_scheme), cfdh_last_error, cfdh_destroy.  Every other entry point returns CFDH_E_STATE on it, and the cfdh_ipcs_* entry points return CFDH_E_STATE on every
 * other context. */
int cfdh_create_ipcs(cfdh_ctx **out, int device, int gdim, int64_t nn, int64_t nvert, int64_t nc, const int32_t *cells,
                     const double *node_coords, int64_t nfacets, const int32_t *facet_cells, const int32_t *facet_local,
                     const int32_t *facet_marker);
/* c = conv_coeff and s_f = force_coeff of the scheme above.  Before this call the context uses the consistent momentum
 * equation rho u_t + rho (w . grad) u - mu lap u + grad p = rho f, i.e. (rho, +rho) of the current cfdh_set_params; the
 * reference's literal form is (1, -1). */
int cfdh_ipcs_set_form(cfdh_ctx *ctx, double conv_coeff, double force_coeff);
/* per solve (1, 2, 3): relative tolerance and iteration cap; one absolute tolerance.  Defaults 1e-5 (PETSc's), 1e-50, 10000.
 * The cap bounds the iterations LAUNCHED (BiCGStab / CG iterations go out in batches of up to four ahead of the convergence test,
 * the last batch cut to what is left), so its[k] <= max_it[k] always; a solve that has not met its tolerance on the true residual
 * by then ends with CFDH_KSP_DIVERGED_ITS, one that meets a NaN / inf or a breakdown (a zero denominator) with
 * CFDH_KSP_DIVERGED_NANORINF. */
int cfdh_ipcs_set_tolerances(cfdh_ctx *ctx, const double rtol[3], double atol, const int32_t max_it[3]);
typedef struct cfdh_ipcs_stats {
  int32_t its[3], reason[3];   /* CFDH_KSP_* */
  double rel_res[3];           /* achieved true |b - A x| / |b| */
  double ms_assemble, ms_solve[3], ms_total;
  /* kernels launched and stream synchronisations made by the scheme's own code in the step (assembly, right-hand sides, Krylov
   * loops).  NOT counted: the kernels inside the V-cycles (one cycle per pressure iteration), memsets and copies.  Two of the
   * synchronisations only delimit the phase times above. */
  int32_t launches, host_syncs;
} cfdh_ipcs_stats;
/* One step: 1-4 above.  CFDH_E_DIVERGED with a reason <= 0 when a solve hit its cap or met a NaN (the plugin raises
 * RuntimeError("Did not converge, reason: r.")). */
int cfdh_ipcs_step(cfdh_ctx *ctx, cfdh_ipcs_stats *stats);
/* Operators as CSR in the caller's numbering, columns ascending; query convention of cfdh_get_csr (nnz first).  which 0: A1 as
 * last assembled, Dirichlet treatment included (assembled from the current state when no step has run); 1: L with its Dirichlet
 * rows; 2: rho M; 3 .. 3 + gdim - 1: B_d; 3 + gdim .. 3 + 2 gdim - 1: G_d.  Exposed for parity tests, like
 * cfdh_get_pcd_operator. */
int cfdh_ipcs_get_operator(cfdh_ctx *ctx, int which, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals);
/* Vectors of the last step (or, for b1, of the assembly cfdh_ipcs_get_operator(0) triggered): which 0: u* [nn][gdim], 1: phi
 * [nvert], 2: b1 [nn][gdim], 3: b2 [nvert], 4: b3 [nn][gdim]; the search direction p as the last velocity-sized (5, [nn][gdim])
 * or pressure (6, [nvert]) Krylov solve left it -- work vectors, exposed so that a test can see that the iterations launched
 * behind a converged one moved nothing. */
int cfdh_ipcs_get_intermediate(cfdh_ctx *ctx, int which, double *out);
/* z = V r, one V-cycle of the pressure hierarchy for the current pressure Dirichlet set ([nvert] host arrays).  Exposed so that
 * a test can measure how symmetric the cycle is (it decides between PCG and flexible PCG). */
int cfdh_ipcs_apply_pressure_pc(cfdh_ctx *ctx, const double *r, double *z);
/* One of the step's three Krylov drivers on data of the caller's: which 0: BiCGStab + Jacobi on A1 (assembled from the current
 * state by this call), 1: flexible PCG + one V-cycle on L, 2: CG + Jacobi on rho M.  b, x0, x: host arrays with that solve's
 * unknowns ([nn][gdim] for 0 and 2, [nvert] for 1); the same kernels, matrix, Jacobi weights and work vectors as in
 * cfdh_ipcs_step, with rtol, atol and max_it of this call.  No mean is subtracted: on a singular pressure problem pass a
 * mean-free b.  The time state (u_sol, u_prev, u_n1, p_sol, u*, phi, b1 .. b3) and the tolerances of cfdh_ipcs_set_tolerances
 * stay as they were.  A capped or broken-down solve is no failed call: 0 is returned, x is the last iterate and
 * stats->reason[which] says what happened (of stats only its / reason / rel_res [which] are meaningful).  CFDH_E_ARG, before
 * anything is launched, for a null b / x0 / x / stats, which outside 0 .. 2, max_it < 1, rtol outside [0, 1) or atol < 0.
 * scalars (or NULL) receives the CFDH_IPCS_NSCAL words of the device's scalar block after the solve:
 *    0 IP_RHO      rh . r (BiCGStab) after the last iteration       6 IP_TOL2  max(rtol |b|, atol)^2
 *    1 IP_RHO_OLD  the one before                                  7 IP_BN2   |b|^2
 *    2 IP_ALPHA    of the last iteration                           8 IP_RN2   |b - A x|^2 of the returned x
 *    3 IP_OMEGA    of the last iteration (BiCGStab)                9 IP_DONE  1 when the solve stopped by itself
 *    4 IP_BETA     computed last: by iteration k for k + 1        10 IP_ITS   iterations
 *                  (flexible PCG: by k - 1 for k, none after k)   11 IP_BAD   1 after a NaN / inf or a breakdown
 *    5 IP_RZ       r . z: after the last iteration (CG), at the    12 .. 15 unused
 *                  start of the last one (flexible PCG)
 * On the device the closing true-residual stage resets words 0 .. 4 (to |r|^2, 1, 1, 1, 0, for a restart); the call returns them
 * as they were just before it, as the last iteration left them.  A solve that ends at its = 0 returns the reset values.
 * Exposed for tests, like cfdh_krylov_vec_op. */
#define CFDH_IPCS_NSCAL 16
int cfdh_ipcs_krylov_solve(cfdh_ctx *ctx, int which, const double *b, const double *x0, double rtol, double atol, int max_it,
                           double *x, cfdh_ipcs_stats *stats, double *scalars);

/* The scheme of a cfdh_create_ipcs context.  CFDH_IPCS_BDF2 (default) is the one described above.  CFDH_IPCS_MIDPOINT is the
 * reference's other pressure-correction solver (src/solvers/ipcs_midpoint.py:60-80 there): the vector-coupled epsilon
 * form sigma = 2 mu eps(u) - p I at the midpoint, its ds pair p n . v - mu (nabla_grad(u) n) . v over ALL exterior facets, and
 * EXPLICIT convection, so that the momentum matrix is constant over a run (the step is CFL-limited in exchange).  Rows and
 * columns of the block operators are (node i, component a), (node j, component b) on the interleaved vectors:
 *   V = mu (K x I + E) - mu S,   E(ia, jb) = int d_b phi_i d_a phi_j dx,   S(ia, jb) = int_{dOmega} phi_i d_a phi_j n_b ds,
 *   Pn(ia, k) = int_{dOmega} phi_i psi_k n_a ds,   C(w)(ia) = int phi_i (w . grad) w_a dx
 *   1. A1 u* = b1,  A1_free = rho/dt M x I + V / 2,
 *      b1 = (rho/dt M x I - V / 2) u_prev - c C(u_prev) + (B^T - Pn) p_prev + s_f f m1;  velocity Dirichlet objects as above (all
 *      d components of a node at once).  BiCGStab + point Jacobi on the d nn diagonal.  A1 is assembled only when dt, rho, mu, the
 *      scheme, the set of constrained velocity nodes or their counts changed -- not by a step or a value-only
 *      cfdh_update_dirichlet.
 *   2. L phi = -rho/dt sum_d B_d u*_d with the pressure Dirichlet VALUE g imposed on p: phi takes g - p_prev on the constrained
 *      vertices (lifting and fixed rows are formed on the device every step), so non-homogeneous pressure data are right.
 *      p_sol = p_prev + phi.  Without a pressure object phi is mean-free.  Flexible PCG + one V-cycle, as above.
 *   3. rho M u_sol = rho M u* - dt G phi, as above.  u_n1 is neither used nor shifted.
 * c = conv_coeff and s_f = force_coeff of cfdh_ipcs_set_form (defaults rho and +rho; the reference's literal form is (rho, 1)).
 * cfdh_ipcs_step, _get_intermediate, _krylov_solve (which 0 drives BiCGStab on the block A1), _set_form, _set_tolerances, the
 * functionals and the wall shear act on the current scheme's operators.  A change of scheme invalidates A1 and resets the initial
 * guess of solve 1 to zero.  CFDH_E_ARG on an unknown value.  cfdh_info 91: the scheme; 92: assemblies of A1 since creation. */
enum { CFDH_IPCS_BDF2 = 0, CFDH_IPCS_MIDPOINT = 1 };
int cfdh_ipcs_set_scheme(cfdh_ctx *ctx, int scheme);
/* The block A1 of CFDH_IPCS_MIDPOINT as block CSR on the P2 node pattern, columns ascending, vals [nnz][gdim][gdim] row-major
 * (a, b); query convention of cfdh_get_csr.  which 0: with the Dirichlet treatment, 1: A1_free.  Like cfdh_ipcs_get_operator(0) it
 * assembles from the current state when no step has run, and forms b1 for cfdh_ipcs_get_intermediate(2).  CFDH_E_STATE under
 * CFDH_IPCS_BDF2; conversely cfdh_ipcs_get_operator(0) returns CFDH_E_STATE under CFDH_IPCS_MIDPOINT (which >= 1 stay
 * available).  Exposed for parity tests. */
int cfdh_ipcs_get_block_operator(cfdh_ctx *ctx, int which, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals);

/* u_prev2 (stabilized_schur_bdf2.py:72): upload / download; nv local vertices x gdim */
int cfdh_set_previous2(cfdh_ctx *ctx, const double *u_prev2);
int cfdh_get_previous2(cfdh_ctx *ctx, double *u_prev2);
/* device-side u_prev2 <- u_prev (stabilized_schur_bdf2.py:324, end of solveStep) */
int cfdh_shift_history(cfdh_ctx *ctx);

/* ---- assembly (exposed for parity tests) ---------------------------------- */

/* assembleResidual (+ assembleJacobian when want_jacobian) at the current
 * iterate: stabilized_schur.py:144-175. */
int cfdh_assemble(cfdh_ctx *ctx, int want_jacobian);
/* Monolithic scalar CSR of the owned rows in the reference's block ordering
 * ([all u dofs | all p dofs], stabilized_schur.py:194-196,237-252), local
 * column numbering.  Call with rowptr=col=vals=NULL to query nnz. */
int cfdh_get_csr(cfdh_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals);
/* y = J x on the device with the assembled Jacobian; x: [gdim*nv | nv] monolithic
 * local vector, y: owned rows [gdim*nv_owned | nv_owned]. */
int cfdh_spmv(cfdh_ctx *ctx, const double *x, double *y);

/* The step's own FGMRES on a right-hand side of the caller's: J d = b with cfdh_fgmres itself -- the same kernels, workspace,
 * read-back ring, stream and captured graphs as inside cfdh_solve_step -- on the assembled Jacobian, with the preconditioner built
 * as cfdh_apply_preconditioner builds it, under the context's current options (ksp_rtol, ksp_atol, ksp_max_it, ksp_restart,
 * ksp_guess) and environment switches.  b [gdim*nv | nv] and x [gdim*nv | nv] are monolithic host arrays in the caller's numbering,
 * as for cfdh_spmv; they live in two device buffers of the hook's own, allocated by its first call.  One GPU only (CFDH_E_STATE on
 * a part of a partitioned run, and before a Jacobian is assembled).
 * newton_index selects the ring of the projected initial guess: -1 leaves every ring untouched and starts from zero; 0 .. 3 use
 * and feed that ring exactly as the Newton solve of that index does (the returned x is kept only after a converged solve).
 * A capped, broken-down or attainable-accuracy solve is no failed call: 0 is returned, x is the last iterate, *its and *reason
 * (CFDH_KSP_*) say what happened.  CFDH_E_ARG, before anything is launched, for a null b / x / its / reason, for newton_index
 * outside -1 .. 3, and for a trace whose m is below ksp_restart.  The time state, F, the Newton history, the options and the
 * tolerances stay as they were; with newton_index -1 so do the watchdog's switches (fp32 copy, refinement of long cycles); the
 * statistics counters of cfdh_info may advance.
 *
 * trace (or NULL) describes the LAST cycle of the solve and the residual history of the whole solve.  The caller sets the three
 * capacities and the array pointers (each may be NULL: not wanted); n = (gdim + 1) nv.  A solve without a trace launches exactly
 * what cfdh_solve_step launches; with one, the iterate and V_0 are copied on the device at the start of every cycle (V_0 is
 * overwritten by the next true residual).
 *   V  [(m + 1) n]  column i at V + i n: the basis v_0 .. v_k            Z  [m n]  z_j = P^-1 v_j, j < k
 *   H  [(m + 1) m]  column j at H + j (m + 1): [h_0 .. h_j ; hnorm], UNROTATED, the values handed to the least-squares update
 *   ww, nrm2 [m]    w.w and the squared norm of the FIRST Gram-Schmidt pass of column j (what the refinement criterion saw)
 *   second_pass [m] 0: one pass; 1: refined; 2: refined while later iterations were in flight (they were launched again)
 *   y  [m]          the k coefficients of the update x = x_start + Z y
 *   x0 [n]          the iterate before the first cycle (zero or the projected guess); x_start [n]: before the last cycle
 *   res [max_res]   recurrence residual after every processed iteration of the whole solve (n_res of them, its unless capped)
 *   cycle_beta, cycle_est [max_cycles]  per cycle: the true residual norm it started from, the recurrence estimate it ended with */
typedef struct cfdh_fgmres_trace {
  int32_t m, max_res, max_cycles;              /* in: capacities */
  int32_t cycles, k, guess_used, fp32_used;    /* out: cycles run, columns of the last one, projected guess used, fp32 basis copy in use in the last cycle */
  int32_t n_res, pad_;
  double bn, tol, beta;                        /* |b|, the absolute tolerance, the true residual norm the last cycle started from */
  double *V, *Z, *H, *ww, *nrm2, *y, *x0, *x_start, *res, *cycle_beta, *cycle_est;
  int32_t *second_pass;
} cfdh_fgmres_trace;
int cfdh_fgmres_solve(cfdh_ctx *ctx, const double *b, int newton_index, double *x, int32_t *its, int32_t *reason, cfdh_fgmres_trace *trace);

/* ---- the step ------------------------------------------------------------- */

/* solveStep (stabilized_schur.py:313-334): null-space handling, Newton with
 * line search, FGMRES + block-Schur preconditioner; returns CFDH_E_DIVERGED
 * with stats->reason < 0 when the reference would raise RuntimeError. */
int cfdh_solve_step(cfdh_ctx *ctx, cfdh_stats *stats);

/* kind 0: F_D, 1: F_L over the exterior facets of `marker`
 * (/root/reference/src/scenarios/dfg_1.py:183-202; the scenario prints 500*F),
 * 2: ||u||_L2, 3: ||p||_L2 (/root/reference/src/scenario.py:315-324),
 * 4: ||u_sol||_inf, 5: ||u_prev||_inf, 6: ||u_sol-u_prev||_inf (scenario.py:268-280),
 * 7: volume flux  int u_sol . n ds  over the exterior facets of `marker` (outward normal; the outlet flow rates the
 * tree and bifurcation scenarios report), 8: the same flux of u_prev (the resistance outlet of
 * stabilized_schur_pressure_backflow.py:204-207, :383-392 is driven by it).  Kinds 0/1 exist for gdim 2 only: for them on gdim 3, and for a kind outside 0 .. 8,
 * the call returns CFDH_E_ARG on every context of cfdh_create / cfdh_create_elem (parts included) and leaves it usable.
 * Sums/maxima over the owned part; the caller (or the communicator) reduces. */
int cfdh_functional(cfdh_ctx *ctx, int kind, int marker, double *out);

/* Wall shear stress, the per-step `assemble_wss()` of solverBase.py:163-195,
 * (1/FacetArea) * inner(w, Tt) * ds with T = -sigma(u_sol, p_sol) n, Tt = T - (T.n) n, assembled on
 * the device from the current solution into a vector field on the context's nodes.  On every kind of context a node that lies on no
 * exterior facet holds exactly 0.0: each facet adds to its own nodes only (cfdh_wall_stats_* take A == 0 to mean "not a wall").
 * On P1 and Q1 contexts the field is tested with the vertex basis, as the reference's CG1 `vector` space.  On a P2 context of
 * cfdh_create_elem the field lives on ALL P2 nodes and is tested with the P2 basis (the edge nodes of a wall facet receive 2/3 of a
 * constant Tt, its vertices 1/6 each in 2-D) -- unlike the reference's CG1 field and unlike the context of cfdh_create_ipcs below.
 * shear: nv x gdim host array, or NULL to compute without downloading.
 * On a context of cfdh_create_ipcs the field is that of the P2 u_sol on the VERTICES (the test space `vector` of
 * solverBase.py:144-162 is CG1 whatever the velocity degree): shear [nvert][gdim], T = -mu (grad u + grad u^T) n, and per vertex v
 * the sum over its exterior facets f of (1/|f|) int_f lambda_v Tt ds, integrated exactly (the integrand is quadratic) and gathered
 * per vertex in ascending facet index without atomics: two calls on one state return the same bytes. */
int cfdh_wall_shear_stress(cfdh_ctx *ctx, double *shear);

/* Cycle-averaged wall shear indices, accumulated on the device over a window of time steps.  Per vertex of the wall-shear field
 * (nv vertices; nvert on a context of cfdh_create_ipcs), with tau_k the wall shear stress at accumulation k and w_k its weight:
 *   S [gdim] = sum w_k tau_k,   A = sum w_k |tau_k|,   M = max_k |tau_k|,   and the scalars W = sum w_k and the count.
 * cfdh_wall_stats_reset allocates on first use and zeroes.  cfdh_wall_stats_accumulate computes the wall shear stress of the
 * current solution as cfdh_wall_shear_stress(ctx, NULL) does and updates S, A, M in one pointwise kernel (rank-local on a part of a
 * partitioned run: owned entries are meaningful); weight must be finite and > 0 (CFDH_E_ARG); CFDH_E_STATE before any reset.
 * cfdh_wall_stats_get forms the field `which` on the device and downloads it in the caller's numbering; *n receives the number of
 * doubles, out may be NULL (query):
 *   0: TAWSS = A / W [nv]                 1: OSI = (1 - |S| / A) / 2, clamped to [0, 1/2], 0 where A == 0 [nv]
 *   2: RRT = W / |S| (= 1 / ((1 - 2 OSI) TAWSS)), +inf where |S| == 0 < A, 0 where A == 0 [nv]
 *   3: mean vector S / W [nv][gdim]       4: peak M [nv]       5: {W, count} [2]
 * which 0 .. 4 with W == 0 and any call before a reset: CFDH_E_STATE; an unknown which: CFDH_E_ARG.  cfdh_info(ctx, 90): the count. */
int cfdh_wall_stats_reset(cfdh_ctx *ctx);
int cfdh_wall_stats_accumulate(cfdh_ctx *ctx, double weight);
int cfdh_wall_stats_get(cfdh_ctx *ctx, int which, int64_t *n, double *out);

/* ---- passive scalar transport (blood age, contrast bolus; not in the reference) ------------------------------------------
 *
 * dc/dt + w . grad c - D lap c = s for ONE P1 scalar c on the context's vertices, advected by the velocity the flow step has just
 * computed: SUPG in space, a theta-scheme in time.  Call cfdh_scalar_step after cfdh_solve_step and before cfdh_advance: at that
 * point u_sol and u_prev are the two ends of the step.
 *
 * Per cell K (a P1 simplex, d = gdim, local vertices a): g_a = grad(lambda_a), |K|, h = the cell size of the flow's tau (largest
 * vertex distance); nodal advecting velocity w_a = theta_c u_sol,a + (1 - theta_c) u_prev,a with mean wbar = sum_a w_a / (d + 1);
 *   tau_c = [(2 / dt)^2 + (2 |wbar| / h)^2 + (4 D / h^2)^2]^(-1/2),     p_a = tau_c wbar . g_a
 * (the SUPG test function is lambda_a + p_a with the cell-mean velocity).  Element matrices, all closed form:
 *   M_ab  = |K| (1 + delta_ab) / ((d + 1)(d + 2))                        Ms_ab = p_a |K| / (d + 1)
 *   C_ab  = |K| / ((d + 1)(d + 2)) (sum_c w_c + w_a) . g_b               Cs_ab = p_a |K| wbar . g_b
 *   K_ab  = D |K| g_a . g_b                                              b_a   = s |K| (1 / (d + 1) + p_a)
 * The step, with dt of cfdh_set_params:
 *   [(M + Ms) / dt + theta_c (C + K + Cs)] c1 = [(M + Ms) / dt - (1 - theta_c)(C + K + Cs)] c0 + b.
 * Dirichlet rows become identity rows with the value on the right-hand side; columns are not eliminated.  Nothing is added on the
 * other boundaries: zero diffusive flux, free advective outflow.  SUPG does not capture discontinuities: under- and overshoots
 * next to a sharp front (a bolus) are expected and are not clipped.
 *
 * One assembly kernel per step writes the left-hand values on the vertex graph and the right-hand side (the right-hand operator is
 * applied to c0 on the fly and never stored): one owner per row, fixed summation order, no atomics -- two assemblies give the same
 * bytes.  The system is solved by BiCGStab + Jacobi on the true residual, |b - A c| <= max(rtol |b|, atol), from c0 with the
 * Dirichlet values imposed.
 *
 * Contexts: closed-form P1 contexts of cfdh_create (gdim 2 and 3), the whole mesh on one GPU.  cfdh_scalar_enable returns
 * CFDH_E_ARG, with the context unchanged, on generic-element contexts, on contexts of cfdh_create_ipcs and on a part of a
 * partitioned run, for a non-finite or negative D, a non-finite s and theta_c outside (0, 1].  Every other cfdh_scalar_* call
 * returns CFDH_E_STATE before cfdh_scalar_enable.  A context that never enables the scalar allocates nothing and launches nothing
 * for it (cfdh_info 95: enabled, 96: scalar steps taken, 97: launches of the assembly kernel since cfdh_create). */
typedef struct cfdh_scalar_stats {
  int32_t its, reason;   /* BiCGStab iterations, CFDH_KSP_* */
  double rel_res;        /* final true |b - A c| / |b| */
  double ms_assemble;    /* the assembly kernel (device events) */
  double ms_total;       /* the call (host clock) */
} cfdh_scalar_stats;
/* Allocates on first use (c = 0); a later call changes D, s and theta_c and keeps c, the Dirichlet set and the tolerances. */
int cfdh_scalar_enable(cfdh_ctx *ctx, double D, double s, double theta_c);
/* Replaces the Dirichlet set (caller's vertex numbering; a vertex listed twice keeps the later value); n = 0 clears it.  CFDH_E_ARG,
 * with the set unchanged, for an out-of-range node or a non-finite value. */
int cfdh_scalar_set_dirichlet(cfdh_ctx *ctx, int64_t n, const int32_t *nodes, const double *values);
/* c [nv] in the caller's vertex numbering; CFDH_E_ARG for a non-finite entry. */
int cfdh_scalar_set_state(cfdh_ctx *ctx, const double *c);
int cfdh_scalar_get_state(cfdh_ctx *ctx, double *c);
/* Defaults 1e-8, 1e-50, 1000.  CFDH_E_ARG for rtol outside [0, 1), atol < 0 or max_it < 1. */
int cfdh_scalar_set_tolerances(cfdh_ctx *ctx, double rtol, double atol, int32_t max_it);
/* One step.  CFDH_E_DIVERGED (reason CFDH_KSP_DIVERGED_ITS / _NANORINF) when the solve hits max_it or breaks down: c is then left
 * unchanged.  Needs cfdh_set_params and a state (cfdh_set_state or a solved step): CFDH_E_STATE otherwise.  stats may be NULL. */
int cfdh_scalar_step(cfdh_ctx *ctx, cfdh_scalar_stats *stats);
/* Left-hand matrix (CSR in the caller's numbering, columns ascending) and right-hand side [nv] of the NEXT step at the current
 * state, assembled by this call with the step's kernel.  Query convention of cfdh_get_csr (nnz first with rowptr = col = vals =
 * rhs = NULL).  Exposed for parity tests, like cfdh_get_pcd_operator. */
int cfdh_scalar_get_operator(cfdh_ctx *ctx, int64_t *nnz, int32_t *rowptr, int32_t *col, double *vals, double *rhs);
/* kind 0: int c dx, 1: int c (u_sol . n) ds over the exterior facets of `marker` (outward normal; exact for the P1 fields),
 * 2 / 3: min / max of c over the vertices. */
int cfdh_scalar_functional(cfdh_ctx *ctx, int kind, int marker, double *out);
/* The step's BiCGStab + Jacobi driver on data of the caller's: the left-hand matrix of the NEXT step at the current state (assembled
 * by this call, as cfdh_scalar_get_operator does), b, x0, x: [nv] host arrays in the caller's vertex numbering; the same kernels,
 * Jacobi weights and work vectors as in cfdh_scalar_step, with rtol, atol and max_it of this call.  c, the tolerances of
 * cfdh_scalar_set_tolerances and cfdh_info 96 / 97 stay as they were; b and x live in two buffers of the hook's own, allocated by
 * its first call.  A capped or broken-down solve is no failed call: 0 is returned, x is the last iterate and stats->reason says
 * what happened (of stats only its / reason / rel_res are meaningful).  CFDH_E_ARG, before anything is launched, for a null b / x0
 * / x / stats, a non-finite entry of b or x0, max_it < 1, rtol outside [0, 1) or atol < 0; CFDH_E_STATE before cfdh_scalar_enable,
 * cfdh_set_params or a state.  scalars (or NULL) receives the CFDH_SCALAR_NSCAL words of the device's scalar block after the solve:
 *    0 SC_RHO      rh . r after the last iteration                 5 SC_TOL2  max(rtol |b|, atol)^2
 *    1 SC_RHO_OLD  the one before                                  6 SC_BN2   |b|^2
 *    2 SC_ALPHA    of the last iteration                           7 SC_RN2   |b - A x|^2 of the returned x
 *    3 SC_OMEGA    of the last iteration                           8 SC_DONE  1 when the solve stopped by itself
 *    4 SC_BETA     computed last: by iteration k for k + 1         9 SC_ITS   iterations
 *                                                                 10 SC_BAD   1 after a NaN / inf or a breakdown
 * On the device the closing true-residual stage resets words 0 .. 4 (to |r|^2, 1, 1, 1, 0, for a restart); the call returns them
 * as they were just before it, as the last iteration left them.  A solve that ends at its = 0 returns the reset values.
 * p (or NULL) receives the search direction [nv] as the last launched iteration left it.  Exposed for tests, like
 * cfdh_ipcs_krylov_solve. */
enum { SC_RHO = 0, SC_RHO_OLD, SC_ALPHA, SC_OMEGA, SC_BETA, SC_TOL2, SC_BN2, SC_RN2, SC_DONE, SC_ITS, SC_BAD };
#define CFDH_SCALAR_NSCAL 16
int cfdh_scalar_krylov_solve(cfdh_ctx *ctx, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                             cfdh_scalar_stats *stats, double *scalars, double *p);
/* row [nv]: the device row of every vertex (the library renumbers the vertices; the kernels' grid-stride loops, block partial
 * sums and the slices of the assembly's work list run over device rows).  Exposed for tests that place data on chosen rows. */
int cfdh_scalar_get_order(cfdh_ctx *ctx, int32_t *row);

/* ---- Lagrangian particle tracking (pathlines, residence times, shear exposure; not in the reference) ---------------------
 *
 * Massless particles follow the velocity of the step the flow solver has just taken.  Call cfdh_particles_step after
 * cfdh_solve_step and before cfdh_advance: over the step the velocity is w(x, s) = (1 - s) u_prev(x) + s u_sol(x), s in [0, 1],
 * P1 in space on the context's cells.
 *
 * One step of one particle: nsub substeps of h = dt / nsub, substep k with s0 = k / nsub, explicit midpoint:
 *   k1 = w(x, s0), from the barycentric coordinates lambda of x in the particle's cell;
 *   xm = x + (h / 2) k1, located by the walk below; when that walk leaves the domain the substep degrades to Euler, k2 = k1,
 *   otherwise k2 = w(xm, s0 + 1 / (2 nsub)) in the cell the walk ended in;
 *   xn = x + h k2; the particle is moved from x to xn by the same walk;
 *   path += |x_new - x| and exposure += tau mu gamma_dot, gamma_dot = sqrt(2 D:D), D = sym grad w at s0 + 1 / (2 nsub) in the
 *   midpoint's cell (the start cell after the Euler fallback), tau = h, or the fraction of h travelled when the substep ends at
 *   an exit.  mu is that of cfdh_set_params.
 * The walk from x to a target y, starting in cell c: with lambda(y) in c, every lambda_f(y) >= -1e-12 ends the walk.  Otherwise,
 * among the facets with lambda_f(y) < -1e-12 (facet f is opposite local vertex f), the one with the smallest crossing parameter
 * t_f = lambda_f(x) / (lambda_f(x) - lambda_f(y)) is crossed, ties to the lowest f, and the walk goes on in the cell behind it
 * with the same x and y.  At an exterior facet the particle stops at x + clamp(t_f, 0, 1)(y - x) with status 1 + the facet's
 * CURRENT marker (cfdh_set_facet_markers needs no rebuild) and end time t0 + (k + clamp(t_f, 0, 1)) h, and never moves again:
 * walls, inlets and outlets alike.  More than 64 crossings in one walk: status -1 (lost), the particle stays where the substep
 * started, its end time is t0 + k h.
 *
 * One lane per particle, no atomics; two steps from the same state give the same bytes.  Contexts: closed-form P1 contexts of
 * cfdh_create (gdim 2 and 3), the whole mesh on one GPU.  cfdh_particles_enable returns CFDH_E_ARG, with the context unchanged, on
 * generic-element contexts, on contexts of cfdh_create_ipcs and on a part of a partitioned run, for nsub < 1 and capacity < 1.
 * Every other cfdh_particles_* call returns CFDH_E_STATE before cfdh_particles_enable.  A context that never enables particles
 * allocates nothing and launches nothing for them (cfdh_info 103: enabled, 104: particle steps taken, 105: launches of the
 * advection kernel since cfdh_create). */
typedef struct cfdh_particle_stats {
  int64_t active, exited, lost;  /* particles with status 0 / > 0 / < 0 after the step */
  int64_t stepped;               /* particles that were active when the step began */
  double ms_kernel;              /* the advection kernel (device events) */
  double ms_total;               /* the call (host clock) */
} cfdh_particle_stats;
/* Allocates room for `capacity` particles and builds the neighbour and affine-map tables.  A later call may change nsub only:
 * another capacity is CFDH_E_ARG. */
int cfdh_particles_enable(cfdh_ctx *ctx, int64_t capacity, int32_t nsub);
/* Appends n active particles born at t_birth: x [n][gdim], cell [n] in the caller's cell numbering.  Every point must lie in its
 * cell (every lambda >= -1e-9).  CFDH_E_ARG, with nothing appended, for a point outside its cell, a cell out of range, a
 * non-finite coordinate or t_birth, and for more particles than the capacity still holds. */
int cfdh_particles_seed(cfdh_ctx *ctx, int64_t n, const double *x, const int32_t *cell, double t_birth);
/* Removes all particles; capacity, nsub and the tables stay. */
int cfdh_particles_clear(cfdh_ctx *ctx);
/* One step over [t0, t0 + dt] with dt of cfdh_set_params.  Needs cfdh_set_params and a state (cfdh_set_state or a solved step):
 * CFDH_E_STATE otherwise; CFDH_E_ARG for a non-finite t0.  stats may be NULL. */
int cfdh_particles_step(cfdh_ctx *ctx, double t0, cfdh_particle_stats *stats);
/* Field `which` of all particles in seeding order; *n receives their number, out may be NULL (query).
 *   0: x [n][gdim] double      1: cell [n] int32, caller's numbering      2: status [n] int32 (0 active, 1 + marker, -1 lost)
 *   3: age [n] double = (t_end when stopped, else the time after the last step) - t_birth, 0 for a particle not stepped yet
 *   4: path [n] double         5: exposure [n] double                     6: t_end [n] double, NaN while active
 * An unknown which: CFDH_E_ARG. */
int cfdh_particles_get(cfdh_ctx *ctx, int which, int64_t *n, void *out);

/* ---- volumetric flow diagnostics (vorticity, Q-criterion, shear rate, dissipation, helicity, energy; not in the reference) ----
 *
 * What the velocity does inside the lumen, from u_sol while it sits on the device (between cfdh_solve_step and cfdh_advance, or
 * after cfdh_set_state).
 *
 * Per cell c: G_c[i][j] = d u_i / d x_j of the P1 velocity (one constant matrix per cell), |c| its area / volume,
 * S = (G + G^T) / 2, W = (G - G^T) / 2.
 * Per vertex v, the recovered gradient: G_v = sum_{c contains v} |c| G_c / sum_{c contains v} |c|, both sums over the cells of v in
 * ascending cell index (the caller's numbering).  Every pointwise vertex quantity below is formed from G_v: S, W and the vorticity
 * omega mean those of G_v; u_v is the nodal velocity.  A vertex of no cell has G_v = 0.
 *
 * cfdh_flow_field(ctx, which, &n, out): vertex fields in the caller's vertex numbering; *n receives the number of doubles,
 * out == NULL only queries it.
 *   0 gradient            G_v, row-major                                                      [nv][d d]
 *   1 vorticity           2-D: G10 - G01 ; 3-D: (G21 - G12, G02 - G20, G10 - G01)             [nv] / [nv][3]
 *   2 Q-criterion         (|W|_F^2 - |S|_F^2) / 2                                             [nv]
 *   3 shear rate          gamma_dot = sqrt(2 S:S), the rate behind the particle exposure      [nv]
 *   4 dissipation density phi = 2 mu S:S, mu of cfdh_set_params                               [nv]
 *   5 helicity density    u_v . omega_v ; gdim 3 only                                         [nv]
 *   6 LNH                 u_v . omega_v / (|u_v| |omega_v|), exactly 0 where either norm is 0 ; gdim 3 only   [nv]
 * which 5 and 6 in 2-D and any other which: CFDH_E_ARG.  Without a state (and, for which 4, without cfdh_set_params): CFDH_E_STATE.
 *
 * cfdh_flow_integrals(ctx, out[8]): cell-exact integrals of the current u_sol, one launch and one read-back.
 *   0 sum |c|
 *   1 (rho / 2) int |u|^2, exact for P1: int_c |u|^2 = |c| (sum_a |u_a|^2 + |sum_a u_a|^2) / ((d + 1)(d + 2))
 *   2 (1 / 2) int |omega|^2        3 int 2 mu S:S
 *   4 int u . omega = sum |c| u_mean,c . omega_c (u_mean,c the cell mean); 0.0 in 2-D
 *   5 int div u                    6 int Q                    7 int (div u)^2
 * Entries 2, 3, 6 and 7 are sum |c| (value of G_c).  Needs cfdh_set_params and a state: CFDH_E_STATE otherwise.
 *
 * Window averages, shaped like cfdh_wall_stats_*: cfdh_flow_stats_reset allocates on first use and zeroes;
 * cfdh_flow_stats_accumulate(weight) takes the current u_sol and adds, per vertex, w u [d], w |u|^2, w phi, w gamma_dot, and keeps
 * max gamma_dot; per context W = sum w and the count.  weight must be finite and > 0 (CFDH_E_ARG); before a reset: CFDH_E_STATE.
 * cfdh_flow_stats_get(ctx, which, &n, out):
 *   0 mean velocity sum w u / W                                                     [nv][d]
 *   1 fluctuation energy per unit mass k' = max(0, (sum w |u|^2 / W - |sum w u / W|^2) / 2)   [nv]
 *   2 mean phi      3 mean gamma_dot      4 peak gamma_dot                          [nv]
 *   5 {W, count}                                                                    [2]
 * which 0 .. 4 with W == 0, or any which before a reset: CFDH_E_STATE; an unknown which: CFDH_E_ARG.
 *
 * A cell pass (one lane per cell) writes the rows (|c|, G_c); a vertex pass (one lane per vertex) gathers them through an inverted
 * index and ends in the formula asked for.  No atomics: two calls on one state return the same bytes.  Contexts: closed-form P1
 * contexts of cfdh_create (gdim 2 and 3), the whole mesh on one GPU.  Every entry point returns CFDH_E_ARG with a reason, before any
 * device work and with the context unchanged, on generic-element contexts, on contexts of cfdh_create_ipcs and on a part of a
 * partitioned run.  A context that never calls them allocates and launches nothing (cfdh_info 106: 1 once a flow-diagnostics
 * buffer exists, 107: launches of the cell pass since cfdh_create, 108: accumulations since the last reset; 109 / 110: device time
 * of the last cell pass / of the last kernel behind it, see cfdh_info). */
int cfdh_flow_field(cfdh_ctx *ctx, int which, int64_t *n, double *out);
int cfdh_flow_integrals(cfdh_ctx *ctx, double *out);
int cfdh_flow_stats_reset(cfdh_ctx *ctx);
int cfdh_flow_stats_accumulate(cfdh_ctx *ctx, double weight);
int cfdh_flow_stats_get(cfdh_ctx *ctx, int which, int64_t *n, double *out);

/* ---- point sampler: the solution at probe points, along lines and on voxel grids (not in the reference) ----
 *
 * The value of (u, p) of u_sol at places the caller chooses, taken while the state sits on the device (between cfdh_solve_step
 * and cfdh_advance, or after cfdh_set_state), without a copy of the whole field.
 *
 * The sample set.  cfdh_sample_set_points(ctx, n, x[n][d], tol) takes explicit points.  cfdh_sample_set_grid(ctx, origin[3],
 * spacing[3], dims[3], tol) takes a regular grid: node (i, j, k) is at origin + (i, j, k) * spacing (one rounding per coordinate:
 * fma(index, spacing, origin)), its index is i + dims[0] * (j + dims[1] * k), the point order of VTK ImageData; in 2-D dims[2]
 * must be 1 and origin[2], spacing[2] are not read.  The coordinates of a grid are generated on the device and never uploaded.
 * A new call replaces the set and drops the series and the means below; n = 0 removes the set and frees its buffers.
 * CFDH_E_ARG: a non-finite coordinate, origin or spacing; a spacing that is not positive; a dims entry below 1 or a product above
 * 2^31 - 1; tol not finite or outside [0, 1e-3].
 *
 * Location, once per set.  Point x belongs to the cell with the lowest index, in the caller's cell numbering, among the cells in
 * which every barycentric coordinate of x is >= -tol; its cell is -1 if there is none.  The answer does not depend on the order in
 * which the context stores its cells nor on how the search is organised, and a point on a vertex, an edge or a face has one answer.
 * The search goes through a uniform bin grid over the bounding box of the mesh, built on the host: per bin the cells whose bounding
 * box, inflated by d tol times its diagonal (a point with lambda >= -tol can lie that far outside it), overlaps the bin, in
 * ascending caller's index; the bin edge starts at the median cell-box edge and is doubled until the lists hold at most 16 nc
 * entries (a mesh of more than 2^31 / 16 cells is refused: CFDH_E_ARG).  One lane per point scans the list of its bin in order and stops at the first cell that holds the point; a point outside
 * the bounding box takes no trip.  Gather only: two calls return the same bytes.
 * cfdh_sample_get_location(ctx, &n, cell[n], lambda[n][d + 1], x[n][d]): the cells in the caller's numbering, the barycentric
 * coordinates in the order of the caller's vertices of that cell (0 for an unlocated point) and the coordinates the device used;
 * any of the three may be NULL.  Without a set *n = 0.  A point that equals a vertex of a cell bit for bit lies in that cell with the
 * unit row (1 at that vertex), whatever tol is: a probe on a mesh vertex returns the nodal values exactly.
 *
 * Sampling.  One lane per point gathers u and p at the d + 1 vertices of its cell and writes the row (u [d], p) = lambda . values;
 * an unlocated point gets zeros.  All calls below need a set and a state (CFDH_E_STATE otherwise).
 * cfdh_sample_now(ctx, &n, out[n][d + 1]): one launch and one download; *n receives the number of points, out == NULL only
 * queries it.
 * cfdh_sample_series_enable(ctx, rows) allocates a device buffer of `rows` row blocks [n][d + 1] (0 frees it; a negative rows or a
 * buffer above 2^40 bytes: CFDH_E_ARG);
 * cfdh_sample_record(ctx, t) appends the block of the current state and keeps t on the host: no synchronisation, no copy.  When the
 * buffer is full: CFDH_E_STATE, the message names cfdh_sample_series_get(ctx, &rows, t[rows], out[rows][n][d + 1]), which
 * downloads what was recorded and empties the buffer (out == NULL only queries *rows).
 * Means, shaped like cfdh_flow_stats_*: cfdh_sample_mean_reset allocates on first use and zeroes;
 * cfdh_sample_mean_accumulate(weight) adds, per point, w u [d], w p and w |u|^2, per context W = sum w and the count.  weight must
 * be finite and > 0 (CFDH_E_ARG); before a reset: CFDH_E_STATE.  cfdh_sample_mean_get(ctx, which, &n, out):
 *   0 mean velocity sum w u / W                                                      [n][d]
 *   1 mean pressure sum w p / W                                                      [n]
 *   2 fluctuation energy k' = max(0, (sum w |u|^2 / W - |sum w u / W|^2) / 2)         [n]
 *   3 {W, count}                                                                     [2]
 * which 0 .. 2 with W == 0, or any which before a reset: CFDH_E_STATE; an unknown which: CFDH_E_ARG.
 *
 * Contexts: closed-form P1 contexts of cfdh_create (gdim 2 and 3), the whole mesh on one GPU.  Every entry point returns
 * CFDH_E_ARG with a reason, before any device work and with the context unchanged, on generic-element contexts, on contexts of
 * cfdh_create_ipcs and on a part of a partitioned run.  A context that never calls them allocates and launches nothing
 * (cfdh_info 111 .. 119). */
int cfdh_sample_set_points(cfdh_ctx *ctx, int64_t n, const double *x, double tol);
int cfdh_sample_set_grid(cfdh_ctx *ctx, const double *origin, const double *spacing, const int64_t *dims, double tol);
int cfdh_sample_get_location(cfdh_ctx *ctx, int64_t *n, int32_t *cell, double *lambda, double *x);
int cfdh_sample_now(cfdh_ctx *ctx, int64_t *n, double *out);
int cfdh_sample_series_enable(cfdh_ctx *ctx, int64_t rows);
int cfdh_sample_record(cfdh_ctx *ctx, double t);
int cfdh_sample_series_get(cfdh_ctx *ctx, int64_t *rows, double *t, double *out);
int cfdh_sample_mean_reset(cfdh_ctx *ctx);
int cfdh_sample_mean_accumulate(cfdh_ctx *ctx, double weight);
int cfdh_sample_mean_get(cfdh_ctx *ctx, int which, int64_t *n, double *out);

/* ---- cut-plane sections: flow rate, mean pressure and energy flux through a plane inside the domain (not in the reference) ----
 *
 * Exact integrals of the P1 fields of u_sol over the intersection of a plane (a line in 2-D) with the mesh, taken while the state
 * sits on the device, without a copy of the field.
 *
 * Definition.  Section k is a point o_k, a unit normal n_k and a radius r_k; r_k <= 0 (or radius == NULL) means unbounded.  The
 * caller passes any non-zero normal and the library normalises it.  In 2-D the "plane" is the line through o with normal n.
 *   Signed distance: s_v = n . (x_v - o), computed by one function once per vertex and section, so that two cells which share a
 *     vertex agree on its sign.
 *   Above and below: a vertex is above if s_v >= 0 and below otherwise.  Zero counts as above.
 *   Cut cells: a cell is cut iff it has at least one vertex above and one below.
 *   Polygon vertices: on the edges that join an above vertex a and a below vertex b, at t = s_a / (s_a - s_b) in [0, 1) from a.
 *   Shapes: in 3-D a 1-3 split gives a triangle, a 2-2 split the convex quadrilateral (a0b0, a0b1, a1b1, a1b0), divided into two
 *     triangles along the diagonal from a0b0 to a1b1.  In 2-D the cut is a segment.
 *   Consequence: a facet that lies exactly in the plane belongs to the one cell on its below side (its t are 0 there) and the
 *     cell above is not cut: it is counted once, never twice.  A section placed on a boundary whose outward normal is +n sees
 *     that boundary's facets; on one whose outward normal is -n it sees nothing.
 *   Clip ball: with r > 0 a cut polygon is taken whole if the arithmetic mean of its vertices lies within r of o, and dropped
 *     otherwise; no polygon is clipped by the ball.  That picks one vessel out of a plane that crosses several.  The number of
 *     taken or dropped polygons with vertices on both sides of the sphere is kept per section (straddling); a well placed ball
 *     has 0.
 * The row of a section has CFDH_SECTION_NQ = 10 doubles, integrals over the taken polygons (dA: area in 3-D, length in 2-D; rho
 * of cfdh_set_params):
 *   0 A = int dA              1 Q = int u.n dA          2 int p dA            3 int (u.n)^2 dA        4 int |u|^2 dA
 *   5 int p (u.n) dA          6 int rho/2 |u|^2 (u.n) dA                      7 .. 9 int u_i dA (slot 9 is +0.0 in 2-D)
 * All are exact up to rounding: the integrands have degree <= 3 and are integrated by 2-point Gauss on segments and a 7-point
 * rule of degree 3 on triangles.  A section that cuts nothing returns ten +0.0.
 *
 * cfdh_section_set(ctx, K, origin[K][d], normal[K][d], radius[K] or NULL) builds the cut on the host, once: per section the cut
 * and taken cells in ascending caller's cell index, each with the local edges that carry its polygon vertices, their t and the
 * measures of its sub-simplices.  The device re-derives no sign and no t.  The lists do not depend on the order or orientation in
 * which the context stores its cells.  A new call replaces the set and drops the series and the means; K = 0 removes the set and
 * frees its buffers.  CFDH_E_ARG: K < 0 or K > 256, a non-finite origin, normal or radius, a zero normal, more than 2^31 - 1
 * entries in all; a refused call leaves the previous set in place.
 * cfdh_section_get_cut(ctx, &K, ptr[K + 1], cell, measure, straddling[K]): the lists as built, with the query convention of
 * cfdh_get_csr: *K always; ptr and straddling when not NULL; cell (caller's ids) and measure (of the whole polygon) both or
 * neither, ptr[K] entries each.  Without a set *K = 0.
 *
 * Evaluation.  One lane per entry gathers u and p at the d + 1 vertices of its cell and forms the ten partial integrals; a block
 * holds entries of one section only and adds them in a fixed order, and the blocks of a section are added in block order.  No
 * atomics: two calls return the same bytes, and the row of a section does not depend on the other sections of the set.  The calls
 * below need a set, cfdh_set_params and a state (CFDH_E_STATE otherwise).
 * cfdh_section_now(ctx, &K, out[K][10]): one evaluation and one download; out == NULL only queries *K.
 * cfdh_section_series_enable(ctx, rows) allocates a device buffer of `rows` blocks [K][10] (0 frees it; negative or above 2^40
 * bytes: CFDH_E_ARG).  cfdh_section_record(ctx, t) appends the block of the current state and keeps t on the host: no
 * synchronisation, no copy.  When the buffer is full: CFDH_E_STATE, the message names cfdh_section_series_get(ctx, &rows, t[rows],
 * out[rows][K][10]), which downloads what was recorded and empties the buffer (out == NULL only queries *rows).
 * cfdh_section_mean_reset allocates K x 10 accumulators on first use and zeroes them; cfdh_section_mean_accumulate(weight) adds
 * w times the current rows, W += w and count += 1 (weight finite and > 0, else CFDH_E_ARG; before a reset: CFDH_E_STATE);
 * cfdh_section_mean_get(ctx, &K, out[K][10], w_count[2]) returns sum w row / W and {W, count}; either may be NULL; out with
 * W == 0, or any call before a reset: CFDH_E_STATE.
 *
 * Contexts: as for cfdh_sample_*: closed-form P1 contexts of cfdh_create (gdim 2 and 3), the whole mesh on one GPU.  Every entry
 * point returns CFDH_E_ARG with a reason, before any device work and with the context unchanged, on generic-element contexts, on
 * contexts of cfdh_create_ipcs and on a part of a partitioned run.  A context that never sets sections allocates and launches
 * nothing (cfdh_info 120 .. 125). */
#define CFDH_SECTION_NQ 10
int cfdh_section_set(cfdh_ctx *ctx, int32_t K, const double *origin, const double *normal, const double *radius);
int cfdh_section_get_cut(cfdh_ctx *ctx, int32_t *K, int64_t *ptr, int32_t *cell, double *measure, int32_t *straddling);
int cfdh_section_now(cfdh_ctx *ctx, int32_t *K, double *out);
int cfdh_section_series_enable(cfdh_ctx *ctx, int64_t rows);
int cfdh_section_record(cfdh_ctx *ctx, double t);
int cfdh_section_series_get(cfdh_ctx *ctx, int64_t *rows, double *t, double *out);
int cfdh_section_mean_reset(cfdh_ctx *ctx);
int cfdh_section_mean_accumulate(cfdh_ctx *ctx, double weight);
int cfdh_section_mean_get(cfdh_ctx *ctx, int32_t *K, double *out, double *w_count);

/* ---- multi-GPU ---------------------------------------------- */

/* Halo plan in local vertex numbers: for neighbour k, send_idx[send_ptr[k]..send_ptr[k+1])
 * are owned vertices whose values go to rank nbr_rank[k]; recv_idx likewise the
 * ghosts filled from it (ghosts must be numbered contiguously per neighbour, in
 * neighbour order, starting at nv_owned). */
int cfdh_set_halo(cfdh_ctx *ctx, int nnbr, const int32_t *nbr_rank, const int64_t *send_ptr,
                  const int32_t *send_idx, const int64_t *recv_ptr, const int32_t *recv_idx);
/* Global pressure space of a partitioned run.  The pressure part of the preconditioner is a Poisson-type
 * solve whose low modes couple all parts; a rank-local (block-Jacobi) version multiplies the FGMRES
 * iterations by ~10.  Every rank therefore receives the whole (replicated, geometry-only) mesh and the
 * global pressure-Dirichlet set, builds the same global Laplacian hierarchy and applies it redundantly to
 * the all-reduced right-hand side.  owned_global[nv_owned]: global vertex id of each owned local vertex
 * (local numbering of cfdh_create).  Call after the Dirichlet data are known; no-op need for one rank. */
int cfdh_set_global_pressure_space(cfdh_ctx *ctx, int64_t nv_global, int64_t nc_global, const int32_t *cells_global,
                                   const double *coords_global, const int32_t *owned_global, int64_t n_pbc,
                                   const int32_t *pbc_nodes_global);
/* RCCL over xGMI: rank 0 creates the 128-byte unique id, the launcher
 * broadcasts it, every rank calls cfdh_comm_init. */
int cfdh_comm_unique_id(void *id128);
int cfdh_comm_init(cfdh_ctx *ctx, const void *id128, int rank, int nranks);
/* Host-staged alternative (CPU/gloo tests, debugging): the library calls back
 * with host buffers.  allreduce: in-place sum (op 0) / max (op 1) of n doubles;
 * exchange: send/recv byte buffers per neighbour as laid out by cfdh_set_halo
 * (3 doubles per vertex: ux, uy, p). */
typedef int (*cfdh_allreduce_fn)(void *user, double *buf, int n, int op);
typedef int (*cfdh_exchange_fn)(void *user, const double *sendbuf, double *recvbuf);
int cfdh_comm_set_callbacks(cfdh_ctx *ctx, cfdh_allreduce_fn ar, cfdh_exchange_fn ex, void *user, int rank, int nranks);

/* ---- measurement ------------------------------------------------------------ */

/* HIP-event timing of the hot kernels on the library's stream.
 * kind 0: fused residual+Jacobian assembly, 1: monolithic SpMV, 2: tau moments, 10: PCD K assembly, 11: PCD apply pass,
 * 3: A00 SpMV (Chebyshev sweep, pc_type 0), 4: level-0 up-sweep of the pressure hierarchy (x = Sb b + Sc x_c; a
 * Jacobi sweep of the unfused cycle), 5: the same for the velocity hierarchy (two right-hand sides),
 * 8 / 9: level-0 down-sweep (b_c = G b) of the pressure / velocity hierarchy,
 * 7: EMPTY event pairs recorded when profiling is switched on (the per-launch overhead of the method). */
int cfdh_profile_enable(cfdh_ctx *ctx, int on);
int cfdh_profile_get(cfdh_ctx *ctx, int kind, double *total_ms, int64_t *launches);
int cfdh_profile_reset(cfdh_ctx *ctx);
/* sizes for roofline accounting: 0 nv_owned, 1 nv, 2 nc, 3 vertex-graph nnz,
 * 4 Sp nnz, 5 incidences, 6 AMG levels, 7 assembly workgroups, 8 velocity-proxy nnz;
 * communicator state: 9 padded part size of the pressure all-gather (0: all-reduce path), 10: RCCL attached,
 * 11: size of the replicated coarse level below the distributed finest pressure level (0: fully replicated cycle),
 * 12: overlapping (restricted additive Schwarz) velocity cycle in use;
 * counters since cfdh_create / cfdh_profile_reset: 13 all-reduce calls, 14 halo exchanges, 15 host synchronisations
 * (stream/event waits for scalars), 16 FGMRES iterations, 17 all-gathers; 18: communicator size;
 * fused AMG cycle: 19 / 20 entries of Sb + Sc on level 0 (pressure / velocity hierarchy), 21 / 22 entries of G on
 * level 0, 23 / 24 size of level 1, 25: fused cycle in use; 26: gdim;
 * 27: microseconds the last preconditioner build took on the device (0: it was built on the host); 28: element type (CFDH_ELEM_*),
 * 29: nodes per cell;
 * 30 + l / 40 + l: rows / entries of level l of the velocity hierarchy, 50 + l / 60 + l: of the pressure hierarchy (l < 10, 0 past the end);
 * 70: linear solves that started from a projected initial guess (cfdh_options.ksp_guess), 71: their mean |r0| / |b| in units of 1e-6;
 * 84: FGMRES cycles whose true residual was read back, 86: linear solves whose prologue projected an initial guess (used or not) -- both
 * reset with 13..17, like 87: the host synchronisations inside the FGMRES cycles (one per batch of iterations the host processes, one
 * per re-orthogonalised vector); 85: 1 when the lean solve path is switched on (CFDH_SOLVE_LEAN);
 * 88 / 89: rank found in, and size of, the Gram system of the last projected initial guess (-1 / 0: none yet);
 * 74: preconditioner builds since cfdh_create, 75: 1 while the preconditioner is valid (built, not invalidated since), 76: 1 when the
 * last null-space test of cfdh_solve_step found the constant pressure in the null space of the Jacobian, 77: formulation (CFDH_FORM_*),
 * 78: Schur approximation in use (cfdh_options.pc_type: 0 SELFP, 1 Cahouet-Chabard, 2 PCD), 79: Eisenstat-Walker forcing version;
 * 90: accumulations of the wall shear indices since the last cfdh_wall_stats_reset (every context kind);
 * 93: traction boundaries set (cfdh_set_traction_boundaries), 94: launches of the traction kernel since cfdh_create;
 * 95: 1 when the passive scalar is enabled (cfdh_scalar_enable), 96: scalar steps taken, 97: launches of the scalar assembly
 * kernel since cfdh_create;
 * 98 / 99: longest / shortest per-workgroup vertex list of the P1 triangle assembly, 100 / 101: the same of its cell lists (0 on
 * other contexts), 102: 1 when that assembly reads them at a fixed stride (CFDH_ASM_STAGE, read by cfdh_create);
 * 103: 1 when particles are enabled (cfdh_particles_enable), 104: particle steps taken, 105: launches of the advection kernel
 * since cfdh_create;
 * 106: 1 once a flow-diagnostics buffer exists (cfdh_flow_*), 107: launches of its cell-gradient pass since cfdh_create, 108:
 * cfdh_flow_stats_accumulate calls since the last cfdh_flow_stats_reset, 109 / 110: nanoseconds, by device events, of the last
 * cell-gradient pass / of the last vertex, accumulation or integral kernel (0 before the first; the call waits for that kernel);
 * 111: points in the sample set (cfdh_sample_*), 112: points located, 113: launches of the sample kernel since cfdh_create, 114:
 * row blocks waiting in the series, 115 / 116: nanoseconds, by device events, of the last locate / of the last sample kernel (as
 * 109 / 110), 117 .. 119: the bin grid built last: the number of times its edge was doubled, the total length of its
 * lists, the longest list;
 * 120: sections set (cfdh_section_*), 121: entries of their cut lists in all, 122: the longest list, 123: evaluations launched
 * since cfdh_create, 124: row blocks waiting in the series, 125: nanoseconds, by device events, of the last evaluation (as 109) */
int64_t cfdh_info(const cfdh_ctx *ctx, int what);

#ifdef __cplusplus
}
#endif
#endif /* CFDH_H */
