// State of an incremental pressure-correction context (cfdh_create_ipcs) and the internals its three files share:
// cfdh_ipcs_setup.cpp (creation, Dirichlet data, uploads of what cfdh_ipcs_host.hpp computes), cfdh_ipcs_krylov.hip (Krylov
// kernels, drivers, ip_solve) and cfdh_ipcs.hip (assembly, right-hand sides, the step, functionals).  Node numbering is the caller's.
#pragma once
#include "cfdh_internal.hpp"
#include "cfdh_ipcs_host.hpp"
#include "cfdh_wave.hpp"

using cfdh_ipcs_host::IpMid;
using cfdh_ipcs_host::IpOps;
using cfdh_ipcs_host::IpRef;

#define IP_NB 2048  // most blocks (= partial sums per dot product) of the reducing kernels

// scalars of the Krylov loops (device array of IP_NS doubles; [IP_RN2, IP_BAD] are mirrored into host-mapped memory); the indices
// are part of cfdh_ipcs_krylov_solve's contract (include/cfdh.h)
enum { IP_RHO = 0, IP_RHO_OLD, IP_ALPHA, IP_OMEGA, IP_BETA, IP_RZ, IP_TOL2, IP_BN2, IP_RN2, IP_DONE, IP_ITS, IP_BAD, IP_NS = 16 };
static_assert(IP_NS == CFDH_IPCS_NSCAL, "include/cfdh.h documents the scalar block");

struct IpcsData {
  int D = 2, NL = 6, nn = 0, nvert = 0, nc = 0;
  // host mesh, reference tensors and constant operators (cfdh_ipcs_host.hpp; op.eptr / op.elist are dropped once uploaded)
  std::vector<int> cells, fcell, flocal, fmarker;
  std::vector<double> coords, geo;   // geo[cell] = (Jinv [D][D], |det|)
  IpRef ref;
  IpOps op;
  // device copies
  dbuf<int> d_cells, rp2, col2, eptr, elist, d_gptr, d_gcol, d_bptr, d_bcol, rp1, col1, d_fcell, d_flocal, d_fmarker;
  dbuf<double> d_coords, d_geo, d_T2, Mv, Kv, Gv, BTv, Bv, d_m1, Mpv, Lv, Afree, A1v, RMv, dinv1, dinv3, cw, fout;
  // wall shear stress (cfdh_wallstats.hip): the vertices of the exterior facets and, per wall vertex, its exterior facets in
  // ascending facet index (cfdh_mesh::wall_vertex_facets)
  int n_wallv = 0;
  dbuf<int> wv_list, wv_ptr, wv_fac;
  // state and work vectors: velocity-sized [nn D], pressure-sized [nvert]
  dbuf<double> u_sol, u_prev, u_n1, us, b1, b3, kr, krh, kp, kv, ks, kt, ky, kz, uval, ucnt;
  dbuf<double> p_sol, p_prev, phi, b2, pr, pz, pp, pq, lift2, prhs;
  dbuf<unsigned char> uflag, pflag;
  dbuf<double> S, P;                 // Krylov scalars, partial sums
  // Dirichlet data (host master copies)
  std::vector<unsigned char> h_uflag, h_pflag;
  std::vector<double> h_ucnt, h_uval, h_pcnt, h_pval;
  bool ubc_dirty = true, pbc_dirty = true, pset_dirty = true;
  AmgHier hLam;                      // hierarchy of the pressure Laplacian, rebuilt when the pressure Dirichlet SET changes
  bool singular = true, assembled = false;
  double rm_rho = -1.0;              // density RMv / dinv3 were built for
  double conv_coeff = -1.0, force_coeff = 0.0;  // cfdh_ipcs_set_form; before that call: rho and +rho
  bool force_default = true;
  double rtol[3] = {1e-5, 1e-5, 1e-5}, atol = 1e-50;
  int max_it[3] = {10000, 10000, 10000};
  long long n_launch = 0, n_sync = 0, n_field_copies = 0;  // of the step in progress; whole-field host copies since creation
  cfdh_ipcs_stats last = {};
  // cfdh_ipcs_krylov_solve: right-hand side and iterate of its own, and the scalar block as the last iteration left it
  dbuf<double> hk_b, hk_x;
  bool snap_on = false, snap_set = false;
  double snap[IP_NS] = {};
  // ---- scheme `ipcs_midpoint` (cfdh_ipcs_set_scheme): vector-coupled momentum matrix, constant over the run.  Host: E - S as
  // [nnz][D][D] blocks on the P2 pattern, Pn as [nnzG][D] on the gptr / gcol pattern (mid, built once, cells and facets ascending);
  // device: those, the block matrices A1_free / A1 and the Jacobi weights of the D nn diagonal, the cells of every node
  // (nptr / nlist: cell * NL + local node, ascending) for the matrix-free convection, the unconstrained L and the pressure
  // Dirichlet values / counts for the per-step lifting.
  int scheme = 0;                    // CFDH_IPCS_BDF2 | CFDH_IPCS_MIDPOINT
  bool mid_built = false, mid_valid = false, uset_dirty = true;
  double mid_key[3] = {0, 0, 0};     // dt, rho, mu of the block A1
  std::vector<unsigned char> mid_flag;  // constrained velocity nodes and their counts the block A1 was assembled for
  std::vector<double> mid_cnt;
  long long n_assemblies = 0;        // assemblies of A1 since creation (cfdh_info 92)
  IpMid mid;
  dbuf<int> nptr, nlist;
  dbuf<double> ESv, BTPv, AfreeB, A1B, dinvB, conv, Lfree, pval, pcnt;
};

// ---- internals shared by the three files
#define IP(c) ((c)->ipcs)
#define IPL(c, kern, grid, shm, ...)                                                  \
  do {                                                                                \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(TPB), shm, (c)->stream, __VA_ARGS__);   \
    IP(c)->n_launch++;                                                                \
  } while (0)
static inline int ip_sync(cfdh_ctx *c) {
  IP(c)->n_sync++;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
static inline int ip_grid8(int nrows) { return (int)((8ll * nrows + TPB - 1) / TPB); }
static inline int ip_nb(long long n, int per) {  // blocks of a reducing grid-stride kernel
  long long g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : (g > IP_NB ? IP_NB : g));
}
struct IpMat { int n; const int *rp, *col; const double *val; };
struct IpTol { double rtol, atol; int max_it; };

int ip_prepare(cfdh_ctx *c);        // uploads whatever host data changed: Dirichlet data, the pressure hierarchy, rho M (setup)
int ip_assemble_bdf2(cfdh_ctx *c);  // A1 and b1 of ipcs_bdf2 at the current state (cfdh_ipcs.hip)
int ip_mid_matrix(cfdh_ctx *c);     // the block A1 of ipcs_midpoint, if it is out of date (cfdh_ipcs.hip)
int ip_sub_mean(cfdh_ctx *c, int n, double *x);
// The one place that knows which solve uses what: solve `which` (0 tentative velocity, 1 pressure, 2 velocity update) of the
// current scheme on the caller's b and x (x holds the initial guess).  Instantiated for D = 2, 3 in cfdh_ipcs_krylov.hip.
template <int D>
int ip_solve(cfdh_ctx *c, int which, IpTol tol, const double *b, double *x, cfdh_ipcs_stats *st);

int cfdh_ipcs_create(cfdh_ctx *c, int gdim, int64_t nn, int64_t nvert, int64_t nc, const int32_t *cells, const double *coords, int64_t nfac,
                     const int32_t *fcell, const int32_t *flocal, const int32_t *fmarker);
void cfdh_ipcs_free(cfdh_ctx *c);
int cfdh_ipcs_clear_dirichlet(cfdh_ctx *c);
int cfdh_ipcs_add_dirichlet(cfdh_ctx *c, int field, int64_t n, const int32_t *nodes, const double *values, bool update);
int cfdh_ipcs_assemble(cfdh_ctx *c);   // A1, b1 at the current state (of the current scheme)
int cfdh_ipcs_set_scheme_impl(cfdh_ctx *c, int scheme);
int cfdh_ipcs_step_impl(cfdh_ctx *c, cfdh_ipcs_stats *st);
int cfdh_ipcs_apply_pc(cfdh_ctx *c, const double *r, double *z);
int cfdh_ipcs_krylov_solve_impl(cfdh_ctx *c, int which, const double *b, const double *x0, double rtol, double atol, int max_it, double *x,
                                cfdh_ipcs_stats *st, double *scalars);
int cfdh_ipcs_functional(cfdh_ctx *c, int kind, int marker, double *out);
