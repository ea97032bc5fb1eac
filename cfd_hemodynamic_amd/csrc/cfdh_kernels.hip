// Hand-written gfx950 (CDNA4, wave64) kernels of the stabilized_schur hot path on P1 triangles: the closed-form element
// kernels and the products with the block matrix they assemble (cfdh3_kernels.hip is the same for tetrahedra).
//
//  * k_moments    : tau / tau_LSIC moments per cell (stabilized_schur.py:100-118)
//  * asm_kernel   : fused element residual + Jacobian, one lane per (row vertex, cell)
//                   incidence; patch data staged in LDS; the cells of a vertex form a
//                   counter-clockwise fan, so off-diagonal blocks are completed by one
//                   lane shuffle and the diagonal block / residual by a segmented
//                   wavefront reduction -- no LDS accumulation, no atomics, fixed order
//                   (bitwise reproducible); plain stores of complete 3x3 blocks
//                   (stabilized_schur.py:67-123,144-175,185-189)
//  * spmv kernels : 8 lanes per vertex row over the block CSR, DPP reductions; the lean-solve variants with their wrappers
//  * diagonal of A00, Chebyshev on D^-1 A00, null-space test, sparse Dirichlet update
//  * functionals, wall shear stress, halo pack
//  * quadrature upload and the profiling brackets (prof_begin / prof_end) every kernel file uses
//
// The AMG cycles and the other steps of a preconditioner application live in cfdh_amg_apply.hip, the vector kernels of FGMRES
// in cfdh_krylov_vec.hip, the scalar reductions in cfdh_reduce.hip.
//
// Everything is HBM-bound fp64 stream/gather work; MFMA is not used (nothing
// here is a dense contraction).  Algebra: SURVEY.md Appendix A / DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>

#include "cfdh_internal.hpp"
#include "cfdh_quad_tri.h"
#include "cfdh_wave.hpp"

__constant__ double d_qw[CFDH_NQ];
__constant__ double d_ql[CFDH_NQ][3];

int k_upload_quadrature(cfdh_ctx *c) {
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(d_qw), CFDH_QW, sizeof(CFDH_QW)));
  HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(d_ql), CFDH_QL, sizeof(CFDH_QL)));
  return 0;
}

// ---------------------------------------------------------------- profiling
void prof_begin(cfdh_ctx *c, int kind) {
  if (!c->prof_on || c->capturing) return;
  if (c->ev_next + 2 > c->ev_pool.size()) {
    for (int i = 0; i < 64; i++) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; c->ev_pool.push_back(e); }
  }
  cfdh_ctx::EvRec r;
  r.kind = kind; r.a = c->ev_pool[c->ev_next++]; r.b = c->ev_pool[c->ev_next++];
  (void)hipEventRecord(r.a, c->stream);
  c->ev_pending.push_back(r);
}
void prof_end(cfdh_ctx *c, int kind) {
  if (!c->prof_on || c->capturing || c->ev_pending.empty()) return;
  (void)kind;
  (void)hipEventRecord(c->ev_pending.back().b, c->stream);
  if (c->ev_pending.size() >= 4096) prof_flush(c);
}
void prof_flush(cfdh_ctx *c) {
  if (c->ev_pending.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  for (auto &r : c->ev_pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->prof[r.kind].total_ms += ms; c->prof[r.kind].launches++; }
  }
  c->ev_pending.clear();
  c->ev_next = 0;
}

// vector layout: [u owned 2*nvo | p owned nvo | ghosts (ux,uy,p) x ng]
__device__ __forceinline__ int uoff(int w, int nvo) { return w < nvo ? 2 * w : 3 * w; }
__device__ __forceinline__ int poff(int w, int nvo) { return w < nvo ? 2 * nvo + w : 3 * w + 2; }

// ---------------------------------------------------------------- tau moments
// M_ab = int_K tau l_a l_b, L = int_K tau_L on the 49-point rule; tau, tau_L
// depend on u_prev only (stabilized_schur.py:91-93,100-108,116-118) so this
// runs once per time step.  One lane per cell, coalesced 64-B records out.
__global__ __launch_bounds__(TPB) void moments_kernel(int nc, int nvo, const int *__restrict__ cells,
                                                      const double *__restrict__ coords,
                                                      const double *__restrict__ un, double *__restrict__ mom,
                                                      double dt, double nu) {
  int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= nc) return;
  int v0 = cells[3 * e], v1 = cells[3 * e + 1], v2 = cells[3 * e + 2];
  double2 X0 = *(const double2 *)(coords + 2 * v0), X1 = *(const double2 *)(coords + 2 * v1), X2 = *(const double2 *)(coords + 2 * v2);
  double u0x = un[uoff(v0, nvo)], u0y = un[uoff(v0, nvo) + 1];
  double u1x = un[uoff(v1, nvo)], u1y = un[uoff(v1, nvo) + 1];
  double u2x = un[uoff(v2, nvo)], u2y = un[uoff(v2, nvo) + 1];
  double det = (X1.x - X0.x) * (X2.y - X0.y) - (X1.y - X0.y) * (X2.x - X0.x);
  double area = 0.5 * fabs(det);
  double d01 = hypot(X0.x - X1.x, X0.y - X1.y), d12 = hypot(X1.x - X2.x, X1.y - X2.y), d20 = hypot(X2.x - X0.x, X2.y - X0.y);
  double h = fmax(d01, fmax(d12, d20));
  double ih2 = 1.0 / (h * h);
  double t2 = 4.0 / (dt * dt), t3 = 16.0 * nu * nu * ih2 * ih2;
  double hr = h / (2.0 * nu);
  double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0, L = 0;
#pragma unroll 7
  for (int q = 0; q < CFDH_NQ; q++) {
    double l0 = d_ql[q][0], l1 = d_ql[q][1], l2 = d_ql[q][2], wq = d_qw[q];
    double ux = l0 * u0x + l1 * u1x + l2 * u2x;
    double uy = l0 * u0y + l1 * u1y + l2 * u2y;
    double s = ux * ux + uy * uy;
    double t1 = fmax(4.0 * s, 1e-30) * ih2;  // (max(2|u|, eps))^2 / h^2, eps = 1e-15
    double tau = cfdh_rsqrt(t1 + t2 + t3);
    double vn = s > 1e-280 ? s * cfdh_rsqrt(s) : 0.0;
    double Re = vn * hr;
    double z = (Re <= 3.0) ? Re * (1.0 / 3.0) : 1.0;
    double tl = vn * h * z * 0.5;
    double w = wq * tau;
    m00 += w * l0 * l0; m01 += w * l0 * l1; m02 += w * l0 * l2;
    m11 += w * l1 * l1; m12 += w * l1 * l2; m22 += w * l2 * l2;
    L += wq * tl;
  }
  double4 *o = (double4 *)(mom + 8 * (size_t)e);
  o[0] = make_double4(area * m00, area * m01, area * m02, area * m11);
  o[1] = make_double4(area * m12, area * m22, area * L, 0.0);
}

int k_moments(cfdh_ctx *c) {
  if (c->gen) { c->mom_valid = true; return 0; }  // tau is evaluated inside the quadrature loop of the generic kernels
  if (c->dim == 3) return k3_moments(c);
  prof_begin(c, 2);
  hipLaunchKernelGGL(moments_kernel, dim3((c->nc + TPB - 1) / TPB), dim3(TPB), 0, c->stream, c->nc, c->nvo, c->cells.p,
                     c->coords.p, c->xprev.p, c->mom.p, c->dt, c->mu / c->rho);
  prof_end(c, 2);
  HIPCHK(c, hipGetLastError());
  c->mom_valid = true;
  return 0;
}

// ---------------------------------------------------------------- fused assembly
struct AsmArgs {
  const double *coords, *mom, *x, *un, *un2, *bcval, *bcmult;
  const int *vptr, *blk_row, *blk_vptr, *blk_vlist, *blk_cptr, *blk_clist, *wave_maxlen;
  const int *blk_vfix, *blk_cfix;  // the two lists at the fixed strides CFDH_MAX_BV / CFDH_MAX_BC, -1 padded (STG)
  const unsigned *inc_slot, *inc_rank, *inc_loc;
  const unsigned char *cflag, *bcflag;
  double *A00, *A01, *A10, *A11, *F;
  int nvo;
  double dt, rho, mu, muf, fx, fy;
  double theta, a0, a1, a2;  // time scheme (cfdh_set_time_scheme)
  double beta_bf;            // backflow coefficient beta*rho on facets flagged in cflag bits 3..5 (cfdh_set_boundary_terms)
  int ds_terms;              // the ds pair of stabilized_schur.py:79 on all exterior facets
#ifdef CFDH_ASM_TIMING
  long long *dbg;            // [nblk][8] phase time stamps of wave 0 (diagnostic build only)
#endif
};

// MODE 0: residual only; 1: residual + Jacobian; 2: residual with lifting (Jacobian in registers only)
//
// Workgroup = a run of whole matrix rows.  Prologue: the vertices and cells the block touches
// (compact per-block lists built at setup) are loaded ONCE, coalesced, into LDS -- nodal
// coordinates, iterate, u_prev, Dirichlet flags, and the 64-B tau-moment records; every lane then
// gathers its element from LDS only (a per-lane gather from global memory costs one L1 line
// per lane per load and made the first version of this kernel L1/TA-bound).
// HIST2: the time term carries a2*u_prev2 (BDF2 steps of stabilized_schur_bdf2.py:95-110).
#ifndef CFDH_BF_OCC
#define CFDH_BF_OCC 2  // the backflow variant needs ~10 more VGPRs than the 168 of 3 waves/SIMD: run it at 2
#endif
// BF: backflow facets present (compiled out otherwise so that the base solver keeps its register budget).
#ifndef CFDH_ASM_OCC
#define CFDH_ASM_OCC 3
#endif
#ifndef MOMS
#define MOMS 5
#endif
// STG false: the lists through blk_vptr / blk_cptr -- three dependent memory trips before the barrier (descriptors -> lists ->
//            gathers);
//     true:  the lists through blk_vfix / blk_cfix, whose address is a function of block and lane alone: the ids are requested
//            together with the descriptors and the lane records, the gathers follow one trip later.  Padded slots (-1) load
//            nothing and write nothing, so LDS holds the same values in the same places and everything behind the barrier is
//            the same code: F and the matrix agree bit for bit (tests/test_gpu_asm_stage.py).
namespace asm_stage {
constexpr int VT = (CFDH_MAX_BV + CFDH_MAX_INC - 1) / CFDH_MAX_INC;      // list entries a lane requests: vertices ...
constexpr int CT = (4 * CFDH_MAX_BC + CFDH_MAX_INC - 1) / CFDH_MAX_INC;  // ... and quarters of cell records
static_assert(CFDH_MAX_INC % 4 == 0, "the quarter of a cell record a lane copies must not depend on the trip");
}  // namespace asm_stage
template <int MODE, bool HIST2 = false, bool BF = false, bool STG = false, int OCC = (BF ? CFDH_BF_OCC : CFDH_ASM_OCC)>
__global__ __launch_bounds__(CFDH_MAX_INC, OCC) void asm_kernel(AsmArgs p) {
  constexpr bool JAC = (MODE != 0);
  constexpr bool WJ = (MODE == 1);
  __shared__ double2 sX[CFDH_MAX_BV], sU[CFDH_MAX_BV], sUn[CFDH_MAX_BV];
  __shared__ double2 sUn2[HIST2 ? CFDH_MAX_BV : 1];
  __shared__ double sP[CFDH_MAX_BV];
  __shared__ int sVid[CFDH_MAX_BV];
  __shared__ unsigned char sFl[CFDH_MAX_BV];
  __shared__ double2 sMom[CFDH_MAX_BC * MOMS];  // 64-B records at a stride of 80 B: with stride 64 the k-th quarter of every record
                                                // falls into the same 4 of the 64 LDS banks (16-way conflict on every read)
  __shared__ unsigned char sCf[CFDH_MAX_BC];
  __shared__ int sRow[CFDH_MAX_ROWS + 1];
  const int t = threadIdx.x, blk = blockIdx.x;
#ifdef CFDH_ASM_TIMING
  long long ts[6];
  ts[0] = __builtin_readcyclecounter();
#endif
  const int row0 = p.blk_row[blk], row1 = p.blk_row[blk + 1];
  const int nrows = row1 - row0;
  const int nvo = p.nvo;
  // the lane's own incidence record does not depend on the staged data: requested first, so that its latency
  // overlaps the staging loads instead of following the barrier
  const size_t lk = (size_t)blk * CFDH_MAX_INC + t;
  const unsigned loc = p.inc_loc[lk], meta = p.inc_slot[lk], seg = p.inc_rank[lk];
  const int wmax = p.wave_maxlen[blk * (CFDH_MAX_INC / 64) + (t >> 6)];
  if (STG) {
    int vid[asm_stage::VT], cid[asm_stage::CT];
#pragma unroll
    for (int k = 0; k < asm_stage::VT; k++) {
      const int i = t + k * CFDH_MAX_INC;
      vid[k] = i < CFDH_MAX_BV ? p.blk_vfix[(size_t)blk * CFDH_MAX_BV + i] : -1;
    }
#pragma unroll
    for (int k = 0; k < asm_stage::CT; k++) {
      const int i = t + k * CFDH_MAX_INC;
      cid[k] = i < 4 * CFDH_MAX_BC ? p.blk_cfix[(size_t)blk * CFDH_MAX_BC + (i >> 2)] : -1;
    }
#pragma unroll
    for (int k = 0; k < asm_stage::VT; k++) {
      const int i = t + k * CFDH_MAX_INC, v = vid[k];
      if (v < 0) continue;
      const int uo = uoff(v, nvo), po = poff(v, nvo);
      sVid[i] = v;
      sX[i] = *(const double2 *)(p.coords + 2 * (size_t)v);
      sU[i] = make_double2(p.x[uo], p.x[uo + 1]);
      sP[i] = p.x[po];
      sUn[i] = make_double2(p.un[uo], p.un[uo + 1]);
      if (HIST2) sUn2[i] = make_double2(p.un2[uo], p.un2[uo + 1]);
      sFl[i] = p.bcflag[v];
    }
#pragma unroll
    for (int k = 0; k < asm_stage::CT; k++) {  // 4 x 16 B per cell record, consecutive lanes; the lane of the first quarter brings the flags
      const int i = t + k * CFDH_MAX_INC, e = cid[k];
      if (e < 0) continue;
      sMom[MOMS * (i >> 2) + (i & 3)] = *(const double2 *)(p.mom + 8 * (size_t)e + 2 * (i & 3));
      if ((t & 3) == 0) sCf[i >> 2] = p.cflag[e];
    }
    for (int i = t; i <= nrows; i += CFDH_MAX_INC) sRow[i] = p.vptr[row0 + i];
  } else {
    const int v0 = p.blk_vptr[blk], nvl = p.blk_vptr[blk + 1] - v0;
    for (int i = t; i < nvl; i += CFDH_MAX_INC) {
      const int vid = p.blk_vlist[v0 + i];
      const int uo = uoff(vid, nvo), po = poff(vid, nvo);
      sVid[i] = vid;
      sX[i] = *(const double2 *)(p.coords + 2 * (size_t)vid);
      sU[i] = make_double2(p.x[uo], p.x[uo + 1]);
      sP[i] = p.x[po];
      sUn[i] = make_double2(p.un[uo], p.un[uo + 1]);
      if (HIST2) sUn2[i] = make_double2(p.un2[uo], p.un2[uo + 1]);
      sFl[i] = p.bcflag[vid];
    }
    const int c0 = p.blk_cptr[blk], ncl = p.blk_cptr[blk + 1] - c0;
    for (int i = t; i < 4 * ncl; i += CFDH_MAX_INC) {  // 4 x 16 B per cell record, consecutive lanes
      const int cid = p.blk_clist[c0 + (i >> 2)];
      sMom[MOMS * (i >> 2) + (i & 3)] = *(const double2 *)(p.mom + 8 * (size_t)cid + 2 * (i & 3));
    }
    for (int i = t; i < ncl; i += CFDH_MAX_INC) sCf[i] = p.cflag[p.blk_clist[c0 + i]];
    for (int i = t; i <= nrows; i += CFDH_MAX_INC) sRow[i] = p.vptr[row0 + i];
  }
#ifdef CFDH_ASM_TIMING
  ts[1] = __builtin_readcyclecounter();
#endif
  __syncthreads();
#ifdef CFDH_ASM_TIMING
  ts[2] = __builtin_readcyclecounter();
#endif

  const bool active = loc != 0xFFFFFFFFu;
  double Fr[3] = {0, 0, 0};
  double J00[3][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}}, J01[3][2] = {{0, 0}, {0, 0}, {0, 0}},
         J10[3][2] = {{0, 0}, {0, 0}, {0, 0}}, J11[3] = {0, 0, 0};
  int row = 0;
  unsigned fl0 = 0;
  double xrow[3] = {0, 0, 0};
  if (active) {
    const int a = (meta >> 24) & 3;
    const int lc = loc & 255;
    const int lv[3] = {(int)((loc >> 8) & 255), (int)((loc >> 16) & 255), (int)((loc >> 24) & 255)};
    const int vv[3] = {sVid[lv[0]], sVid[lv[1]], sVid[lv[2]]};
    const int v0 = vv[0], v1 = vv[1], v2 = vv[2];
    row = v0;
    const unsigned cfraw = sCf[lc];
    unsigned cf = cfraw & 7u, cb = cfraw >> 3;
    cf = ((cf >> a) | (cf << (3 - a))) & 7u;
    cb = ((cb >> a) | (cb << (3 - a))) & 7u;
    if (!p.ds_terms) cf = 0;
    // moments, rotated
    const double2 m0 = sMom[MOMS * lc], m1 = sMom[MOMS * lc + 1], m2 = sMom[MOMS * lc + 2], m3 = sMom[MOMS * lc + 3];
    const double o00 = m0.x, o01 = m0.y, o02 = m1.x, o11 = m1.y, o12 = m2.x, o22 = m2.y, Lm = m3.x;
    double M[3][3];
    M[0][0] = a == 0 ? o00 : (a == 1 ? o11 : o22);
    M[1][1] = a == 0 ? o11 : (a == 1 ? o22 : o00);
    M[2][2] = a == 0 ? o22 : (a == 1 ? o00 : o11);
    M[0][1] = M[1][0] = a == 0 ? o01 : (a == 1 ? o12 : o02);
    M[0][2] = M[2][0] = a == 0 ? o02 : (a == 1 ? o01 : o12);
    M[1][2] = M[2][1] = a == 0 ? o12 : (a == 1 ? o02 : o01);
    // geometry and nodal values from LDS
    double X[3][2], ue[3][2], une[3][2], pe[3];
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const double2 xx = sX[lv[b]], uu = sU[lv[b]], un2 = sUn[lv[b]];
      X[b][0] = xx.x; X[b][1] = xx.y;
      ue[b][0] = uu.x; ue[b][1] = uu.y; pe[b] = sP[lv[b]];
      une[b][0] = un2.x; une[b][1] = un2.y;
    }
    const double det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
    const double idet = 1.0 / det;
    double g[3][2];
    g[0][0] = (X[1][1] - X[2][1]) * idet; g[0][1] = (X[2][0] - X[1][0]) * idet;
    g[1][0] = (X[2][1] - X[0][1]) * idet; g[1][1] = (X[0][0] - X[2][0]) * idet;
    g[2][0] = (X[0][1] - X[1][1]) * idet; g[2][1] = (X[1][0] - X[0][0]) * idet;
    const double area = 0.5 * fabs(det);
    const double rho = p.rho, mu = p.mu, idt = 1.0 / p.dt;
    const double th = p.theta, a0idt = p.a0 * idt;
    double ub[3][2], w[3][2], G[2][2] = {{0, 0}, {0, 0}}, gp[2] = {0, 0};
#pragma unroll
    for (int b = 0; b < 3; b++) {
      double h2[2] = {0, 0};
      if (HIST2) {
        const double2 q = sUn2[lv[b]];
        h2[0] = p.a2 * q.x; h2[1] = p.a2 * q.y;
      }
#pragma unroll
      for (int i = 0; i < 2; i++) {
        ub[b][i] = th * ue[b][i] + (1.0 - th) * une[b][i];
        w[b][i] = (p.a0 * ue[b][i] + p.a1 * une[b][i] + h2[i]) * idt;
      }
    }
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int i = 0; i < 2; i++) {
        gp[i] += pe[b] * g[b][i];
#pragma unroll
        for (int j = 0; j < 2; j++) G[i][j] += g[b][i] * ub[b][j];
      }
    const double divu = G[0][0] + G[1][1];
    double Cn[3][2], R[3][2], beta[3][3], mt[3], Q[3][2];
    const double ff[2] = {p.fx, p.fy};
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int j = 0; j < 2; j++) {
        Cn[b][j] = ub[b][0] * G[0][j] + ub[b][1] * G[1][j];
        R[b][j] = rho * (w[b][j] + Cn[b][j]) + gp[j] - rho * ff[j];
      }
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
      for (int b = 0; b < 3; b++) beta[d][b] = ub[d][0] * g[b][0] + ub[d][1] * g[b][1];
    double T = 0;
#pragma unroll
    for (int b = 0; b < 3; b++) { mt[b] = M[b][0] + M[b][1] + M[b][2]; T += mt[b]; }
#pragma unroll
    for (int d = 0; d < 3; d++)
#pragma unroll
      for (int i = 0; i < 2; i++) Q[d][i] = M[0][d] * R[0][i] + M[1][d] * R[1][i] + M[2][d] * R[2][i];
    const double E01 = 0.5 * (G[0][1] + G[1][0]);
    const double E[2][2] = {{G[0][0], E01}, {E01, G[1][1]}};
    const double pbar = (pe[0] + pe[1] + pe[2]) * (1.0 / 3.0);
    const double mab0[3] = {area * (2.0 / 12.0), area * (1.0 / 12.0), area * (1.0 / 12.0)};
    // ---- residual rows of local vertex 0
#pragma unroll
    for (int i = 0; i < 2; i++) {
      double v = 0;
#pragma unroll
      for (int b = 0; b < 3; b++) v += rho * mab0[b] * (w[b][i] + Cn[b][i]);
      v -= rho * ff[i] * area * (1.0 / 3.0);
      v += area * (2.0 * mu * (E[i][0] * g[0][0] + E[i][1] * g[0][1]) - pbar * g[0][i]);
#pragma unroll
      for (int d = 0; d < 3; d++) v += beta[d][0] * Q[d][i];
      v += rho * Lm * divu * g[0][i];
      Fr[i] = v;
    }
    {
      double v = area * (1.0 / 3.0) * divu;
#pragma unroll
      for (int b = 0; b < 3; b++) v += mt[b] * (R[b][0] * g[0][0] + R[b][1] * g[0][1]) / rho;
      Fr[2] = v;
    }
    // ---- Jacobian row block of local vertex 0
    if (JAC) {
      double MBa[3], mtB[3];
#pragma unroll
      for (int cidx = 0; cidx < 3; cidx++) MBa[cidx] = M[cidx][0] * beta[0][0] + M[cidx][1] * beta[1][0] + M[cidx][2] * beta[2][0];
#pragma unroll
      for (int b = 0; b < 3; b++) mtB[b] = mt[0] * beta[0][b] + mt[1] * beta[1][b] + mt[2] * beta[2][b];
#pragma unroll
      for (int b = 0; b < 3; b++) {
        const double mBa = mab0[0] * beta[0][b] + mab0[1] * beta[1][b] + mab0[2] * beta[2][b];
        const double BMBa = beta[0][b] * MBa[0] + beta[1][b] * MBa[1] + beta[2][b] * MBa[2];
        const double gg0b = g[0][0] * g[b][0] + g[0][1] * g[b][1];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
          for (int j = 0; j < 2; j++) {
            const double dij = (i == j) ? 1.0 : 0.0;
            double v = rho * mab0[b] * dij * a0idt;
            v += rho * th * (mab0[b] * G[j][i] + dij * mBa);
            v += area * mu * th * (g[b][i] * g[0][j] + gg0b * dij);
            v += rho * ((dij * a0idt + th * G[j][i]) * MBa[b] + th * dij * BMBa);
            v += th * g[0][j] * Q[b][i];
            v += rho * Lm * th * g[b][j] * g[0][i];
            J00[b][i][j] = v;
          }
          J01[b][i] = -area * (1.0 / 3.0) * g[0][i] + g[b][i] * mtB[0];
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
          const double Gg = G[j][0] * g[0][0] + G[j][1] * g[0][1];
          J10[b][j] = area * (1.0 / 3.0) * th * g[b][j] + mt[b] * (g[0][j] * a0idt + th * Gg) + th * g[0][j] * mtB[b];
        }
        J11[b] = T * gg0b / rho;
      }
    }
    // ---- backflow stabilisation on outlet facets that contain local vertex 0:
    //      F -= beta rho oint (u_prev.n)_- (ubar.v), 2-point Gauss (stabilized_schur_backflow.py:165-176)
    if (BF && (cb & 6u)) {
#pragma unroll
      for (int f = 1; f < 3; f++) {
        if (!((cb >> f) & 1u)) continue;
        const int other = (f == 1) ? 2 : 1;
        const double gl = hypot(g[f][0], g[f][1]);
        const double n[2] = {-g[f][0] / gl, -g[f][1] / gl};
        const double elen = 2.0 * area * gl;
        // nodal values re-read from LDS (keeps the register live ranges of the element algebra short)
        const double2 un0 = sUn[lv[0]], uno = sUn[lv[other]];
        const double s0 = un0.x * n[0] + un0.y * n[1], so = uno.x * n[0] + uno.y * n[1];
        const double gq = 0.28867513459481288;  // 1/(2 sqrt 3)
        double w00 = 0.0, w0o = 0.0;  // sum_q c_q l0 l0, sum_q c_q l0 lo
#pragma unroll
        for (int q = 0; q < 2; q++) {
          const double t = q == 0 ? 0.5 - gq : 0.5 + gq;
          const double l0 = 1.0 - t, lo = t;
          const double sq = l0 * s0 + lo * so;
          const double cq = p.beta_bf * 0.25 * (sq - fabs(sq)) * elen;
          w00 += cq * l0 * l0;
          w0o += cq * l0 * lo;
        }
        const double2 u0 = sU[lv[0]], uo = sU[lv[other]];
        Fr[0] -= w00 * (th * u0.x + (1.0 - th) * un0.x) + w0o * (th * uo.x + (1.0 - th) * uno.x);
        Fr[1] -= w00 * (th * u0.y + (1.0 - th) * un0.y) + w0o * (th * uo.y + (1.0 - th) * uno.y);
        if (JAC) {
          J00[0][0][0] -= th * w00; J00[0][1][1] -= th * w00;
          J00[other][0][0] -= th * w0o; J00[other][1][1] -= th * w0o;
        }
      }
    }
    // ---- exterior facets that contain local vertex 0 (facets 1 and 2)
    if (cf & 6u) {
#pragma unroll
      for (int f = 1; f < 3; f++) {
        if (!((cf >> f) & 1u)) continue;
        const int other = (f == 1) ? 2 : 1;
        const double gl = hypot(g[f][0], g[f][1]);
        const double n[2] = {-g[f][0] / gl, -g[f][1] / gl};
        const double elen = 2.0 * area * gl;
        const double pint = (2.0 * pe[0] + pe[other]) * (1.0 / 6.0);
#pragma unroll
        for (int i = 0; i < 2; i++) {
          const double Gn = G[i][0] * n[0] + G[i][1] * n[1];
          Fr[i] += n[i] * elen * pint - p.muf * Gn * elen * 0.5;
          if (JAC) {
            J01[0][i] += n[i] * elen * (2.0 / 6.0);
            J01[other][i] += n[i] * elen * (1.0 / 6.0);
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
              for (int j = 0; j < 2; j++) J00[b][i][j] -= p.muf * (0.5 * th) * g[b][i] * n[j] * elen;
          }
        }
      }
    }
    // ---- Dirichlet: lifting F += J[:,bc](g - x), zero bc columns and rows
    fl0 = sFl[lv[0]];
    const unsigned fl1 = sFl[lv[1]], fl2 = sFl[lv[2]];
    (void)v1; (void)v2;
    xrow[0] = ue[0][0]; xrow[1] = ue[0][1]; xrow[2] = pe[0];
    if (fl0 | fl1 | fl2) {
      const unsigned flb[3] = {fl0, fl1, fl2};
#pragma unroll
      for (int b = 0; b < 3; b++) {
        if (!flb[b]) continue;
#pragma unroll
        for (int j = 0; j < 2; j++)
          if ((flb[b] >> j) & 1u) {
            if (JAC) {
              const double gx = p.bcval[3 * vv[b] + j] - ue[b][j];
              if (MODE == 2 || gx != 0.0) { Fr[0] += J00[b][0][j] * gx; Fr[1] += J00[b][1][j] * gx; Fr[2] += J10[b][j] * gx; }
              J00[b][0][j] = 0.0; J00[b][1][j] = 0.0; J10[b][j] = 0.0;
            }
          }
        if (flb[b] & 4u) {
          if (JAC) {
            const double gx = p.bcval[3 * vv[b] + 2] - pe[b];
            if (MODE == 2 || gx != 0.0) { Fr[0] += J01[b][0] * gx; Fr[1] += J01[b][1] * gx; Fr[2] += J11[b] * gx; }
            J01[b][0] = 0.0; J01[b][1] = 0.0; J11[b] = 0.0;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 2; i++)
        if ((fl0 >> i) & 1u) {
          Fr[i] = 0.0;
          if (JAC) {
#pragma unroll
            for (int b = 0; b < 3; b++) { J00[b][i][0] = 0.0; J00[b][i][1] = 0.0; J01[b][i] = 0.0; }
          }
        }
      if (fl0 & 4u) {
        Fr[2] = 0.0;
        if (JAC) {
#pragma unroll
          for (int b = 0; b < 3; b++) { J10[b][0] = 0.0; J10[b][1] = 0.0; J11[b] = 0.0; }
        }
      }
    }
  }
#ifdef CFDH_ASM_TIMING
  ts[3] = __builtin_readcyclecounter();
#endif
  // ---- wavefront-level segmented reduction (all 64 lanes take part; idle lanes carry zeros)
  const int lane = t & 63;
  const int seg_pos = seg & 255, seg_len = (seg >> 8) & 255, prev_off = (int)((seg >> 16) & 255) - 64;
  const bool has_prev = (meta >> 27) & 1u, emit_v2 = (meta >> 26) & 1u;
  if (WJ) {
    // off-diagonal block of the edge (i, v1): this cell's B1 plus B2 of the previous cell of the fan
    const int src = lane + (has_prev ? prev_off : 0);
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
      for (int j = 0; j < 2; j++) { const double v = __shfl(J00[2][i][j], src); if (has_prev) J00[1][i][j] += v; }
      { const double v = __shfl(J01[2][i], src); if (has_prev) J01[1][i] += v; }
      { const double v = __shfl(J10[2][i], src); if (has_prev) J10[1][i] += v; }
    }
    { const double v = __shfl(J11[2], src); if (has_prev) J11[1] += v; }
  }
  // diagonal block and residual: sum over the lanes of the row, result in its first lane
  for (int off = 1; off < wmax; off <<= 1) {
    const bool take = active && (seg_pos + off < seg_len);
#pragma unroll
    for (int i = 0; i < 3; i++) { const double v = __shfl_down(Fr[i], off); if (take) Fr[i] += v; }
    if (WJ) {
#pragma unroll
      for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int j = 0; j < 2; j++) { const double v = __shfl_down(J00[0][i][j], off); if (take) J00[0][i][j] += v; }
        { const double v = __shfl_down(J01[0][i], off); if (take) J01[0][i] += v; }
        { const double v = __shfl_down(J10[0][i], off); if (take) J10[0][i] += v; }
      }
      { const double v = __shfl_down(J11[0], off); if (take) J11[0] += v; }
    }
  }
#ifdef CFDH_ASM_TIMING
  ts[4] = __builtin_readcyclecounter();
#endif
  // ---- every block of the row now sits complete in exactly one lane: plain stores
  if (active) {
    const size_t sb = (size_t)sRow[row - row0];
    if (WJ) {
      {
        const size_t s1 = sb + ((meta >> 8) & 255);
        *(double2 *)(p.A00 + 4 * s1) = make_double2(J00[1][0][0], J00[1][0][1]);
        *(double2 *)(p.A00 + 4 * s1 + 2) = make_double2(J00[1][1][0], J00[1][1][1]);
        *(double2 *)(p.A01 + 2 * s1) = make_double2(J01[1][0], J01[1][1]);
        *(double2 *)(p.A10 + 2 * s1) = make_double2(J10[1][0], J10[1][1]);
        p.A11[s1] = J11[1];
      }
      if (emit_v2) {
        const size_t s2 = sb + ((meta >> 16) & 255);
        *(double2 *)(p.A00 + 4 * s2) = make_double2(J00[2][0][0], J00[2][0][1]);
        *(double2 *)(p.A00 + 4 * s2 + 2) = make_double2(J00[2][1][0], J00[2][1][1]);
        *(double2 *)(p.A01 + 2 * s2) = make_double2(J01[2][0], J01[2][1]);
        *(double2 *)(p.A10 + 2 * s2) = make_double2(J10[2][0], J10[2][1]);
        p.A11[s2] = J11[2];
      }
    }
    if (seg_pos == 0) {
      // Dirichlet rows: diagonal = number of bc objects, F = x - g (everything else in the row is zero)
      if (fl0) {
        if (fl0 & 1u) { J00[0][0][0] = p.bcmult[3 * row]; Fr[0] = xrow[0] - p.bcval[3 * row]; }
        if (fl0 & 2u) { J00[0][1][1] = p.bcmult[3 * row + 1]; Fr[1] = xrow[1] - p.bcval[3 * row + 1]; }
        if (fl0 & 4u) { J11[0] = p.bcmult[3 * row + 2]; Fr[2] = xrow[2] - p.bcval[3 * row + 2]; }
      }
      if (WJ) {
        const size_t s0 = sb + (meta & 255);
        *(double2 *)(p.A00 + 4 * s0) = make_double2(J00[0][0][0], J00[0][0][1]);
        *(double2 *)(p.A00 + 4 * s0 + 2) = make_double2(J00[0][1][0], J00[0][1][1]);
        *(double2 *)(p.A01 + 2 * s0) = make_double2(J01[0][0], J01[0][1]);
        *(double2 *)(p.A10 + 2 * s0) = make_double2(J10[0][0], J10[0][1]);
        p.A11[s0] = J11[0];
      }
      *(double2 *)(p.F + 2 * (size_t)row) = make_double2(Fr[0], Fr[1]);
      p.F[2 * (size_t)nvo + row] = Fr[2];
    }
  }
#ifdef CFDH_ASM_TIMING
  __builtin_amdgcn_s_waitcnt(0);
  ts[5] = __builtin_readcyclecounter();
  if (t == 0 && p.dbg)
    for (int k = 0; k < 6; k++) p.dbg[8 * (size_t)blk + k] = ts[k];
#endif
}

int k_assemble(cfdh_ctx *c, const double *xstate, int mode) {
  if (c->gen) return c->dim == 3 ? kg3_assemble(c, xstate, mode) : kg_assemble(c, xstate, mode);
  if (c->dim == 3) return k3_assemble(c, xstate, mode);
  AsmArgs a;
  a.coords = c->coords.p; a.mom = c->mom.p; a.x = xstate; a.un = c->xprev.p; a.un2 = c->xprev2.p; a.bcval = c->bcval.p; a.bcmult = c->bcmult.p;
  a.vptr = c->vptr.p;
  a.blk_vptr = c->blk_vptr.p; a.blk_vlist = c->blk_vlist.p; a.blk_cptr = c->blk_cptr.p; a.blk_clist = c->blk_clist.p; a.inc_loc = c->inc_loc.p; a.wave_maxlen = c->wave_maxlen.p;
  a.blk_row = c->blk_row.p; a.blk_vfix = c->blk_vfix.p; a.blk_cfix = c->blk_cfix.p;
  a.inc_slot = c->inc_slot.p; a.inc_rank = c->inc_rank.p; a.cflag = c->cflag.p; a.bcflag = c->bcflag.p;
  a.A00 = c->A00.p; a.A01 = c->A01.p; a.A10 = c->A10.p; a.A11 = c->A11.p; a.F = c->F.p;
  a.nvo = c->nvo; a.dt = c->dt; a.rho = c->rho; a.mu = c->mu; a.muf = c->muf; a.fx = c->f[0]; a.fy = c->f[1];
  a.theta = c->ts_theta; a.a0 = c->ts_a[0]; a.a1 = c->ts_a[1]; a.a2 = c->ts_a[2];
  a.beta_bf = c->bf_beta * c->rho; a.ds_terms = c->ds_terms ? 1 : 0;
  const bool hist2 = c->ts_a[2] != 0.0;
#ifdef CFDH_ASM_TIMING
  static long long *dbg = nullptr;
  static int dbg_calls = 0;
  if (!dbg) hipMalloc(&dbg, sizeof(long long) * 8 * (size_t)c->nblk);
  a.dbg = dbg;
#endif
  prof_begin(c, 0);
  const dim3 gr(c->nblk), bl(CFDH_MAX_INC);
  const bool bf = c->bf_beta > 0.0 && c->bf_marker >= 0;
#define CFDH_ASM_LAUNCH3(H2, BFV, STG)                                                             \
  do {                                                                                             \
    if (mode == 1) hipLaunchKernelGGL((asm_kernel<1, H2, BFV, STG>), gr, bl, 0, c->stream, a);    \
    else if (mode == 2) hipLaunchKernelGGL((asm_kernel<2, H2, BFV, STG>), gr, bl, 0, c->stream, a); \
    else hipLaunchKernelGGL((asm_kernel<0, H2, BFV, STG>), gr, bl, 0, c->stream, a);              \
  } while (0)
#define CFDH_ASM_LAUNCH(H2, BFV)                          \
  do {                                                    \
    if (c->env.asm_stage) CFDH_ASM_LAUNCH3(H2, BFV, true); \
    else CFDH_ASM_LAUNCH3(H2, BFV, false);                \
  } while (0)
  if (!hist2 && !bf) CFDH_ASM_LAUNCH(false, false);
  else if (hist2 && !bf) CFDH_ASM_LAUNCH(true, false);
  else if (!hist2 && bf) CFDH_ASM_LAUNCH(false, true);
  else CFDH_ASM_LAUNCH(true, true);
#undef CFDH_ASM_LAUNCH3
#undef CFDH_ASM_LAUNCH
  HIPCHK(c, hipGetLastError());
  if (!c->tb_markers.empty()) CHK(k_traction(c, xstate, mode));  // traction boundaries: one small launch behind the volume pass
  prof_end(c, 0);
#ifdef CFDH_ASM_TIMING
  if (mode == 1 && (++dbg_calls % 20) == 0) {
    std::vector<long long> h(8 * (size_t)c->nblk);
    hipStreamSynchronize(c->stream);
    hipMemcpy(h.data(), dbg, sizeof(long long) * h.size(), hipMemcpyDeviceToHost);
    double acc[5] = {0, 0, 0, 0, 0};
    long long tmin = h[0], tmax = h[5];
    for (int b = 0; b < c->nblk; b++) {
      for (int k = 0; k < 5; k++) acc[k] += (double)(h[8 * (size_t)b + k + 1] - h[8 * (size_t)b + k]);
      tmin = std::min(tmin, h[8 * (size_t)b]); tmax = std::max(tmax, h[8 * (size_t)b + 5]);
    }
    fprintf(stderr, "[asm timing] ticks per block: stage-issue %.0f, barrier %.0f, element %.0f, reduce %.0f, stores+drain %.0f; kernel span %lld ticks, %d blocks\n",
            acc[0] / c->nblk, acc[1] / c->nblk, acc[2] / c->nblk, acc[3] / c->nblk, acc[4] / c->nblk, tmax - tmin, c->nblk);
  }
#endif
  if (mode == 1) c->jac_valid = true;
  return 0;
}

// ---------------------------------------------------------------- block SpMV
// 8 lanes per vertex row: lane l of a group takes block k = rowstart + l (+8,...),
// so the value arrays are streamed fully coalesced across the wave; partial
// sums are combined with DPP shuffles.  y = J x over the monolithic vector.
__global__ __launch_bounds__(TPB) void spmv_full_kernel(int nvo, const int *__restrict__ vptr,
                                                        const int *__restrict__ vcol, const double *__restrict__ A00,
                                                        const double *__restrict__ A01, const double *__restrict__ A10,
                                                        const double *__restrict__ A11, const double *__restrict__ x,
                                                        double *__restrict__ y) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0 = 0, a1 = 0, a2 = 0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      const int uo = uoff(w, nvo), po = poff(w, nvo);
      const double xu0 = x[uo], xu1 = x[uo + 1], xp = x[po];
      const double2 b0 = *(const double2 *)(A00 + 4 * (size_t)k), b1 = *(const double2 *)(A00 + 4 * (size_t)k + 2);
      const double2 c01 = *(const double2 *)(A01 + 2 * (size_t)k), c10 = *(const double2 *)(A10 + 2 * (size_t)k);
      const double c11 = A11[k];
      a0 += b0.x * xu0 + b0.y * xu1 + c01.x * xp;
      a1 += b1.x * xu0 + b1.y * xu1 + c01.y * xp;
      a2 += c10.x * xu0 + c10.y * xu1 + c11 * xp;
    }
  }
  a0 = group8_sum(a0); a1 = group8_sum(a1); a2 = group8_sum(a2);
  if (row < nvo && l == 0) {
    *(double2 *)(y + 2 * (size_t)row) = make_double2(a0, a1);
    y[2 * (size_t)nvo + row] = a2;
  }
}


// The same product for NV vectors at once (leading dimension ld): the Jacobian is read once -- the projected initial guess of
// the linear solves multiplies its 2-4 kept corrections with the current matrix (cfdh_solver.cpp::guess_project).
template <int NV>
__global__ __launch_bounds__(TPB) void spmv_full_multi_kernel(int nvo, const int *__restrict__ vptr, const int *__restrict__ vcol,
                                                              const double *__restrict__ A00, const double *__restrict__ A01,
                                                              const double *__restrict__ A10, const double *__restrict__ A11,
                                                              const double *__restrict__ X, double *__restrict__ Y, size_t ld) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0[NV], a1[NV], a2[NV];
#pragma unroll
  for (int v = 0; v < NV; v++) a0[v] = a1[v] = a2[v] = 0.0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      const int uo = uoff(w, nvo), po = poff(w, nvo);
      const double2 b0 = *(const double2 *)(A00 + 4 * (size_t)k), b1 = *(const double2 *)(A00 + 4 * (size_t)k + 2);
      const double2 c01 = *(const double2 *)(A01 + 2 * (size_t)k), c10 = *(const double2 *)(A10 + 2 * (size_t)k);
      const double c11 = A11[k];
#pragma unroll
      for (int v = 0; v < NV; v++) {
        const double *x = X + (size_t)v * ld;
        const double xu0 = x[uo], xu1 = x[uo + 1], xp = x[po];
        a0[v] += b0.x * xu0 + b0.y * xu1 + c01.x * xp;
        a1[v] += b1.x * xu0 + b1.y * xu1 + c01.y * xp;
        a2[v] += c10.x * xu0 + c10.y * xu1 + c11 * xp;
      }
    }
  }
#pragma unroll
  for (int v = 0; v < NV; v++) {
    const double s0 = group8_sum(a0[v]), s1 = group8_sum(a1[v]), s2 = group8_sum(a2[v]);
    if (row < nvo && l == 0) {
      double *y = Y + (size_t)v * ld;
      *(double2 *)(y + 2 * (size_t)row) = make_double2(s0, s1);
      y[2 * (size_t)nvo + row] = s2;
    }
  }
}

// Y_v = J X_v for v < nvec (vectors ld apart; ghost tails of X filled by the caller)
int k_spmv_full_multi(cfdh_ctx *c, const double *X, double *Y, int ld, int nvec) {
  if (c->dim == 3) return k3_spmv_full_multi(c, X, Y, ld, nvec);
  if (nvec < 2 || nvec > 4) {
    for (int v = 0; v < nvec; v++) CHK(k_spmv_full(c, X + (size_t)v * ld, Y + (size_t)v * ld));
    return 0;
  }
  const long long nthreads = 8ll * c->nvo;
  const dim3 gr((unsigned)((nthreads + TPB - 1) / TPB)), bl(TPB);
#define CFDH_SPMM(NV) hipLaunchKernelGGL((spmv_full_multi_kernel<NV>), gr, bl, 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, c->A00.p, \
                                         c->A01.p, c->A10.p, c->A11.p, X, Y, (size_t)ld)
  if (nvec == 2) CFDH_SPMM(2); else if (nvec == 3) CFDH_SPMM(3); else CFDH_SPMM(4);
#undef CFDH_SPMM
  HIPCHK(c, hipGetLastError());
  return 0;
}

int k_spmv_full(cfdh_ctx *c, const double *x, double *y) {
  if (c->dim == 3) return k3_spmv_full(c, x, y);
  const long long nthreads = 8ll * c->nvo;
  prof_begin(c, 1);
  hipLaunchKernelGGL(spmv_full_kernel, dim3((unsigned)((nthreads + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, c->nvo,
                     c->vptr.p, c->vcol.p, c->A00.p, c->A01.p, c->A10.p, c->A11.p, x, y);
  prof_end(c, 1);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// sub-block products on owned columns only (the preconditioner is rank-local):
// BLK 1: y_u = A00 x_u, 2: y_u = A01 x_p, 3: y_p = A10 x_u, 4: y_p = A11 x_p;  MODE 1: y = b - A x
template <int BLK, int MODE>
__global__ __launch_bounds__(TPB) void spmv_blk_kernel(int nvo, const int *__restrict__ vptr, const int *__restrict__ vcol,
                                                       const double *__restrict__ A, const double *__restrict__ x,
                                                       double *__restrict__ y, const double *__restrict__ bvec) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0 = 0, a1 = 0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      if (w >= nvo) continue;
      if (BLK == 1) {
        const double2 xx = *(const double2 *)(x + 2 * (size_t)w);
        const double2 b0 = *(const double2 *)(A + 4 * (size_t)k), b1 = *(const double2 *)(A + 4 * (size_t)k + 2);
        a0 += b0.x * xx.x + b0.y * xx.y; a1 += b1.x * xx.x + b1.y * xx.y;
      } else if (BLK == 2) {
        const double xp = x[w];
        const double2 cc = *(const double2 *)(A + 2 * (size_t)k);
        a0 += cc.x * xp; a1 += cc.y * xp;
      } else if (BLK == 3) {
        const double2 xx = *(const double2 *)(x + 2 * (size_t)w);
        const double2 cc = *(const double2 *)(A + 2 * (size_t)k);
        a0 += cc.x * xx.x + cc.y * xx.y;
      } else {
        a0 += A[k] * x[w];
      }
    }
  }
  a0 = group8_sum(a0);
  if (BLK <= 2) a1 = group8_sum(a1);
  if (row < nvo && l == 0) {
    if (BLK <= 2) {
      double2 o = make_double2(a0, a1);
      if (MODE == 1) { const double2 bb = *(const double2 *)(bvec + 2 * (size_t)row); o.x = bb.x - o.x; o.y = bb.y - o.y; }
      *(double2 *)(y + 2 * (size_t)row) = o;
    } else {
      y[row] = (MODE == 1) ? bvec[row] - a0 : a0;
    }
  }
}

// y_u = b_u - A01 x_p (the coupling product of the block-triangular preconditioner, once per FGMRES iteration) with four
// lanes per row and the first two entries of every lane requested together: 16 B of matrix per entry is too little per
// load for the 8-lane scheme, which left this kernel at 3.6 TB/s (16.1 us for 58 MB; this form: 12.2 us.  The same
// change does nothing for the full product, whose lanes already carry 72 B of matrix per entry: 37.3 vs 36.6 us)
// KEEP: the product itself, q = A01 x_p, is stored as well (16 B per row from the lane that holds the sums): the Krylov product
// that follows the preconditioner reuses it instead of reading the A01 block again (spmv_full_lean_kernel<true, false>)
template <bool KEEP>
__global__ __launch_bounds__(TPB) void spmv_a01_resid_kernel(int nvo, const int *__restrict__ vptr, const int *__restrict__ vcol,
                                                             const double *__restrict__ A, const double *__restrict__ x,
                                                             double *__restrict__ y, const double *__restrict__ bvec,
                                                             double *__restrict__ q) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 2, l = gid & 3;
  double a0 = 0, a1 = 0;
  double2 bb = make_double2(0.0, 0.0);
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    if (l == 0) bb = *(const double2 *)(bvec + 2 * (size_t)row);
    const int k0 = ks + l, k1 = k0 + 4;
    const bool h0 = k0 < ke, h1 = k1 < ke;
    const int q0 = h0 ? k0 : ks, q1 = h1 ? k1 : ks;  // ks is always a valid entry (the diagonal block exists)
    const int w0 = vcol[q0], w1 = vcol[q1];
    const double2 c0 = *(const double2 *)(A + 2 * (size_t)q0), c1 = *(const double2 *)(A + 2 * (size_t)q1);
    const double x0 = (h0 && w0 < nvo) ? x[w0] : 0.0, x1 = (h1 && w1 < nvo) ? x[w1] : 0.0;
    a0 = c0.x * x0 + c1.x * x1;
    a1 = c0.y * x0 + c1.y * x1;
    for (int k = k1 + 4; k < ke; k += 4) {
      const int w = vcol[k];
      if (w >= nvo) continue;
      const double xp = x[w];
      const double2 cc = *(const double2 *)(A + 2 * (size_t)k);
      a0 += cc.x * xp; a1 += cc.y * xp;
    }
  }
  a0 = quad_sum(a0); a1 = quad_sum(a1);
  if (row < nvo && l == 0) {
    *(double2 *)(y + 2 * (size_t)row) = make_double2(bb.x - a0, bb.y - a1);
    if (KEEP) *(double2 *)(q + 2 * (size_t)row) = make_double2(a0, a1);
  }
}

// coupling blocks INCLUDING ghost columns: xv is a full vector in the [u | p | ghost triplets] layout whose
// ghost tail was refreshed by comm_halo.  GB 2: y_u = b_u - A01 x_p ; GB 3: y_p = b_p - A10 x_u.
template <int GB>
__global__ __launch_bounds__(TPB) void spmv_blk_ghost_kernel(int nvo, const int *__restrict__ vptr, const int *__restrict__ vcol,
                                                             const double *__restrict__ A, const double *__restrict__ xv,
                                                             double *__restrict__ y, const double *__restrict__ bvec) {
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0 = 0, a1 = 0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      const double2 cc = *(const double2 *)(A + 2 * (size_t)k);
      if (GB == 2) {
        const double xp = xv[poff(w, nvo)];
        a0 += cc.x * xp; a1 += cc.y * xp;
      } else {
        const int uo = uoff(w, nvo);
        a0 += cc.x * xv[uo] + cc.y * xv[uo + 1];
      }
    }
  }
  a0 = group8_sum(a0);
  if (GB == 2) a1 = group8_sum(a1);
  if (row < nvo && l == 0) {
    if (GB == 2) {
      const double2 bb = *(const double2 *)(bvec + 2 * (size_t)row);
      *(double2 *)(y + 2 * (size_t)row) = make_double2(bb.x - a0, bb.y - a1);
    } else {
      y[row] = bvec[row] - a0;
    }
  }
}
int k_spmv_block_ghost(cfdh_ctx *c, int blk, const double *xv, double *y, const double *b) {
  if (c->dim == 3) return k3_spmv_block_ghost(c, blk, xv, y, b);
  const long long nthreads = 8ll * c->nvo;
  dim3 grid((unsigned)((nthreads + TPB - 1) / TPB)), block(TPB);
  if (blk == 2) hipLaunchKernelGGL((spmv_blk_ghost_kernel<2>), grid, block, 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, c->A01.p, xv, y, b);
  else hipLaunchKernelGGL((spmv_blk_ghost_kernel<3>), grid, block, 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, c->A10.p, xv, y, b);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int k_spmv_block(cfdh_ctx *c, int blk, const double *x, double *y, const double *b, double /*alpha*/) {
  if (c->dim == 3) return k3_spmv_block(c, blk, x, y, b);
  const long long nthreads = 8ll * c->nvo;
  dim3 grid((unsigned)((nthreads + TPB - 1) / TPB)), block(TPB);
  const int mode = b ? 1 : 0;
#define LAUNCH_BLK(B, M, AP) hipLaunchKernelGGL((spmv_blk_kernel<B, M>), grid, block, 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, AP, x, y, b)
  if (blk == 1) { if (mode) LAUNCH_BLK(1, 1, c->A00.p); else LAUNCH_BLK(1, 0, c->A00.p); }
  else if (blk == 2) {
    if (mode) {
      const long long n4 = 4ll * c->nvo;
      hipLaunchKernelGGL(spmv_a01_resid_kernel<false>, dim3((unsigned)((n4 + TPB - 1) / TPB)), block, 0, c->stream, c->nvo, c->vptr.p,
                         c->vcol.p, c->A01.p, x, y, b, (double *)nullptr);
    } else {
      LAUNCH_BLK(2, 0, c->A01.p);
    }
  }
  else if (blk == 3) { if (mode) LAUNCH_BLK(3, 1, c->A10.p); else LAUNCH_BLK(3, 0, c->A10.p); }
  else { if (mode) LAUNCH_BLK(4, 1, c->A11.p); else LAUNCH_BLK(4, 0, c->A11.p); }
#undef LAUNCH_BLK
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- products of the lean solve path (CFDH_SOLVE_LEAN, one rank, P1 triangles; cfdh_solver.cpp).  Kernels of their own: the
// plain product above stays as it is.
//   KEPT : y = J x for the x the preconditioner has just written, with q = A01 x_p taken from the coupling product of that
//          application (spmv_a01_resid_kernel<true>): y_u = A00 x_u + q, y_p = A10 x_u + A11 x_p -- 60 instead of 76 B per entry
//   RESID: y = b - J x and the block partials of |y|^2 (the true residual after a cycle: product, waxpy and the first
//          reduction pass in one kernel)
template <bool KEPT, bool RESID>
__global__ __launch_bounds__(TPB) void spmv_full_lean_kernel(int nvo, const int *__restrict__ vptr, const int *__restrict__ vcol,
                                                             const double *__restrict__ A00, const double *__restrict__ A01,
                                                             const double *__restrict__ A10, const double *__restrict__ A11,
                                                             const double *__restrict__ x, double *__restrict__ y,
                                                             const double *__restrict__ q, const double *__restrict__ b,
                                                             double *__restrict__ partial) {
  __shared__ double sh[4];
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0 = 0, a1 = 0, a2 = 0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      const int uo = uoff(w, nvo), po = poff(w, nvo);
      const double xu0 = x[uo], xu1 = x[uo + 1], xp = x[po];
      const double2 b0 = *(const double2 *)(A00 + 4 * (size_t)k), b1 = *(const double2 *)(A00 + 4 * (size_t)k + 2);
      const double2 c10 = *(const double2 *)(A10 + 2 * (size_t)k);
      const double c11 = A11[k];
      if (KEPT) {
        a0 += b0.x * xu0 + b0.y * xu1;
        a1 += b1.x * xu0 + b1.y * xu1;
      } else {
        const double2 c01 = *(const double2 *)(A01 + 2 * (size_t)k);
        a0 += b0.x * xu0 + b0.y * xu1 + c01.x * xp;
        a1 += b1.x * xu0 + b1.y * xu1 + c01.y * xp;
      }
      a2 += c10.x * xu0 + c10.y * xu1 + c11 * xp;
    }
  }
  a0 = group8_sum(a0); a1 = group8_sum(a1); a2 = group8_sum(a2);
  double ss = 0.0;
  if (row < nvo && l == 0) {
    if (KEPT) { const double2 qq = *(const double2 *)(q + 2 * (size_t)row); a0 += qq.x; a1 += qq.y; }
    if (RESID) {
      const double2 bu = *(const double2 *)(b + 2 * (size_t)row);
      a0 = bu.x - a0; a1 = bu.y - a1; a2 = b[2 * (size_t)nvo + row] - a2;
      ss = a0 * a0 + a1 * a1 + a2 * a2;
    }
    *(double2 *)(y + 2 * (size_t)row) = make_double2(a0, a1);
    y[2 * (size_t)nvo + row] = a2;
  }
  if (RESID) {
    ss = block_sum(ss, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = ss;
  }
}

// t_u = r_u - A01 x_p as k_spmv_block(c, 2, ...) forms it, and q = A01 x_p kept for the product that follows
int k_spmv_a01_keep(cfdh_ctx *c, const double *x, double *y, const double *b, double *q) {
  const long long n4 = 4ll * c->nvo;
  hipLaunchKernelGGL(spmv_a01_resid_kernel<true>, dim3((unsigned)((n4 + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, c->nvo, c->vptr.p,
                     c->vcol.p, c->A01.p, x, y, b, q);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// y = J x with the kept coupling product q = A01 x_p
int k_spmv_full_kept(cfdh_ctx *c, const double *x, double *y, const double *q) {
  const long long nthreads = 8ll * c->nvo;
  hipLaunchKernelGGL((spmv_full_lean_kernel<true, false>), dim3((unsigned)((nthreads + TPB - 1) / TPB)), dim3(TPB), 0, c->stream, c->nvo,
                     c->vptr.p, c->vcol.p, c->A00.p, c->A01.p, c->A10.p, c->A11.p, x, y, q, (const double *)nullptr, (double *)nullptr);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// true residual r = b - J x and its norm with one kernel over the matrix and ONE read-back; false in *done when the partial
// sums of this mesh do not fit the reduction workspace (the caller then takes the three-kernel path)
int k_resid_norm(cfdh_ctx *c, const double *x, const double *b, double *r, double *nrm, bool *done) {
  const long long nthreads = 8ll * c->nvo;
  const long long nb = (nthreads + TPB - 1) / TPB;
  *done = false;
  if (c->dim != 2 || (size_t)nb > c->red_partial.n) return 0;
  hipLaunchKernelGGL((spmv_full_lean_kernel<false, true>), dim3((unsigned)nb), dim3(TPB), 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, c->A00.p,
                     c->A01.p, c->A10.p, c->A11.p, x, r, (const double *)nullptr, b, c->red_partial.p);
  HIPCHK(c, hipGetLastError());
  CHK(red_final(c, 0, 1, (int)nb, (int)nb, c->red_partial.p, c->red_out.p + RO_LEAN_S2, scalars_mirror(c)));
  double s2;
  CHK(scalars_read(c, scalars_mirrored(1), &s2));
  *nrm = sqrt(s2);
  *done = true;
  return 0;
}

__global__ __launch_bounds__(TPB) void extract_diag_kernel(int nvo, const int *__restrict__ vdiag,
                                                           const double *__restrict__ A00, double *__restrict__ dinv) {
  const int row = blockIdx.x * TPB + threadIdx.x;
  if (row >= nvo) return;
  const size_t k = (size_t)vdiag[row];
  const double d0 = A00[4 * k], d1 = A00[4 * k + 3];
  *(double2 *)(dinv + 2 * (size_t)row) = make_double2(1.0 / d0, 1.0 / d1);
}

int k_extract_diag(cfdh_ctx *c) {
  hipLaunchKernelGGL(extract_diag_kernel, dim3((c->nvo + TPB - 1) / TPB), dim3(TPB), 0, c->stream, c->nvo, c->vdiag.p,
                     c->A00.p, c->dinvA.p);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- Chebyshev on D^-1 A00
// one step: r_out = r_in - A00 d_old ; d_new = c1 d_old + c2 D^-1 r_out ; x += d_new
// FIRST: fused with the zero-guess initialisation (d_old = D^-1 r_in / theta formed while gathering,
// x = d_old + d_new); LAST: r_out / d_new not written.  Coefficients come from device memory so that
// a captured graph of the preconditioner survives a refresh of the spectral bound of D^-1 A00.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(TPB) void cheb_a00_step_kernel(int nvo, const int *__restrict__ vptr,
                                                            const int *__restrict__ vcol, const double *__restrict__ A00,
                                                            const double *__restrict__ dinv, const double *__restrict__ rin,
                                                            double *__restrict__ rout, const double *__restrict__ dold,
                                                            double *__restrict__ dnew, double *__restrict__ x,
                                                            const double *__restrict__ coef, int kstep) {
  const double c1 = coef[2 * kstep], c2 = coef[2 * kstep + 1], itheta = coef[0];
  const int gid = blockIdx.x * TPB + threadIdx.x;
  const int row = gid >> 3, l = gid & 7;
  double a0 = 0, a1 = 0;
  if (row < nvo) {
    const int ks = vptr[row], ke = vptr[row + 1];
    for (int k = ks + l; k < ke; k += 8) {
      const int w = vcol[k];
      if (w >= nvo) continue;
      double2 xx;
      if (FIRST) {
        const double2 dj = *(const double2 *)(dinv + 2 * (size_t)w), rj = *(const double2 *)(rin + 2 * (size_t)w);
        xx = make_double2(dj.x * rj.x * itheta, dj.y * rj.y * itheta);
      } else {
        xx = *(const double2 *)(dold + 2 * (size_t)w);
      }
      const double2 b0 = *(const double2 *)(A00 + 4 * (size_t)k), b1 = *(const double2 *)(A00 + 4 * (size_t)k + 2);
      a0 += b0.x * xx.x + b0.y * xx.y; a1 += b1.x * xx.x + b1.y * xx.y;
    }
  }
  a0 = group8_sum(a0); a1 = group8_sum(a1);
  if (row < nvo && l == 0) {
    const size_t o = 2 * (size_t)row;
    const double2 ri = *(const double2 *)(rin + o), di = *(const double2 *)(dinv + o);
    double2 dd;
    if (FIRST) dd = make_double2(di.x * ri.x * itheta, di.y * ri.y * itheta);
    else dd = *(const double2 *)(dold + o);
    const double r0 = ri.x - a0, r1 = ri.y - a1;
    const double n0 = c1 * dd.x + c2 * di.x * r0, n1 = c1 * dd.y + c2 * di.y * r1;
    if (!LAST) {
      *(double2 *)(rout + o) = make_double2(r0, r1);
      *(double2 *)(dnew + o) = make_double2(n0, n1);
    }
    if (FIRST) {
      *(double2 *)(x + o) = make_double2(dd.x + n0, dd.y + n1);
    } else {
      double2 xo = *(double2 *)(x + o);
      xo.x += n0; xo.y += n1;
      *(double2 *)(x + o) = xo;
    }
  }
}

// d0 = D^-1 b / theta ; x = d0
__global__ __launch_bounds__(TPB) void cheb_init_kernel(int n, const double *__restrict__ dinv, const double *__restrict__ b,
                                                        double *__restrict__ d0, double *__restrict__ x, double itheta,
                                                        int accumulate, const double *__restrict__ coef) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  if (coef) itheta = coef[0];
  const double v = dinv[i] * b[i] * itheta;
  d0[i] = v;
  x[i] = accumulate ? x[i] + v : v;
}
// its launch: the start of the A00 solve below and of the level smoother in cfdh_amg_apply.hip
int k_cheb_init(cfdh_ctx *c, int n, const double *dinv, const double *b, double *d0, double *x, double itheta, int accumulate,
                const double *coef) {
  hipLaunchKernelGGL(cheb_init_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, dinv, b, d0, x, itheta, accumulate, coef);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Chebyshev coefficients of the A00 solve -> device (called whenever lmaxA changes)
int k_cheb_a00_coeffs(cfdh_ctx *c) {
  const double lmax = c->lmaxA, lmin = lmax / c->opt.cheb_ratio;
  const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin);
  const double sigma = theta / delta;
  double rho = 1.0 / sigma;
  std::vector<double> h(2 * 16 + 2, 0.0);
  h[0] = 1.0 / theta;
  for (int k = 1; k < c->opt.cheb_degree && k < 16; k++) {
    const double rho_new = 1.0 / (2.0 * sigma - rho);
    h[2 * k] = rho_new * rho; h[2 * k + 1] = 2.0 * rho_new / delta;
    rho = rho_new;
  }
  HIPCHK(c, c->cheb_coef.alloc(h.size()));
  HIPCHK(c, hipMemcpyAsync(c->cheb_coef.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // h is a host temporary
  return 0;
}

// x = Cheb_k(D^-1 A00) b with zero initial guess; lambda in [lmax/ratio, lmax]
int k_cheb_a00(cfdh_ctx *c, const double *b, double *x) {
  const int nu = 2 * c->nvo, deg = c->opt.cheb_degree;
  double *dold = c->pu1.p, *dnew = c->pu2.p, *r = c->pr.p;
  if (deg == 1) {
    return k_cheb_init(c, nu, c->dinvA.p, b, dold, x, 0.0, 0, c->cheb_coef.p);
  }
  const long long nthreads = 8ll * c->nvo;
  dim3 grid((unsigned)((nthreads + TPB - 1) / TPB)), block(TPB);
  for (int k = 1; k < deg; k++) {
    const bool first = (k == 1), last = (k == deg - 1);
    prof_begin(c, 3);
#define LAUNCH_A00(F, LST) hipLaunchKernelGGL((cheb_a00_step_kernel<F, LST>), grid, block, 0, c->stream, c->nvo, c->vptr.p, c->vcol.p, c->A00.p, c->dinvA.p, first ? b : r, r, dold, dnew, x, c->cheb_coef.p, k)
    if (first) { if (last) LAUNCH_A00(true, true); else LAUNCH_A00(true, false); }
    else { if (last) LAUNCH_A00(false, true); else LAUNCH_A00(false, false); }
#undef LAUNCH_A00
    prof_end(c, 3);
    std::swap(dold, dnew);
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ||J n|| and || |J| n || for the constant-pressure vector n (MatNullSpaceTest, stabilized_schur.py:314; the second norm makes
// the decision scale-free, see cfdh_newton_step)
__global__ __launch_bounds__(TPB) void nulltest_kernel(int nvo, const int *__restrict__ vptr, const double *__restrict__ A01,
                                                       const double *__restrict__ A11, double *__restrict__ partial) {
  __shared__ double sh[4];
  double a = 0, b = 0;
  for (int row = blockIdx.x * TPB + threadIdx.x; row < nvo; row += gridDim.x * TPB) {
    double s0 = 0, s1 = 0, s2 = 0, t0 = 0, t1 = 0, t2 = 0;
    for (int k = vptr[row]; k < vptr[row + 1]; k++) {
      const double c0 = A01[2 * (size_t)k], c1 = A01[2 * (size_t)k + 1], c2 = A11[k];
      s0 += c0; s1 += c1; s2 += c2;
      t0 += fabs(c0); t1 += fabs(c1); t2 += fabs(c2);
    }
    a += s0 * s0 + s1 * s1 + s2 * s2;
    b += t0 * t0 + t1 * t1 + t2 * t2;
  }
  a = block_sum(a, sh);
  b = block_sum(b, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = a; partial[gridDim.x + blockIdx.x] = b; }
}
int k_nullspace_test(cfdh_ctx *c, double *nrm, double *absnrm) {
  const int nb = c->dim == 3 ? 256 : red_grid(c, c->nvo);
  if (c->dim == 3) CHK(k3_nullspace_partials(c, nb));
  else hipLaunchKernelGGL(nulltest_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->nvo, c->vptr.p, c->A01.p, c->A11.p, c->red_partial.p);
  HIPCHK(c, hipGetLastError());
  ScalarRead h;
  CHK(scalars_finish(c, c->red_out.p, 2, 0, nb, &h));
  double s[2];
  CHK(scalars_read(c, h, s));
  *nrm = sqrt(s[0]);
  *absnrm = sqrt(s[1]);
  return 0;
}
// |F| and the two numbers of the null-space test with ONE read-back (one rank, triangles): each value is reduced exactly as
// v_norm2 / k_nullspace_test reduce it
int k_fnorm_nulltest(cfdh_ctx *c, int n, const double *F, double *fn, double *nrm, double *absnrm) {
  const int nbf = red_grid(c, n), nb = red_grid(c, c->nvo);
  if ((size_t)nbf + 2 * (size_t)nb > c->red_partial.n) return cfdh_fail(c, CFDH_E_STATE, "reduction workspace too small");
  double *mir = scalars_mirror(c), *pn = c->red_partial.p + nbf;
  CHK(red_partials_launch(c, 0, nbf, n, F, F, c->red_partial.p));
  hipLaunchKernelGGL(nulltest_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->nvo, c->vptr.p, c->A01.p, c->A11.p, pn);
  HIPCHK(c, hipGetLastError());
  CHK(red_final(c, 0, 1, nbf, nbf, c->red_partial.p, c->red_out.p, mir));
  CHK(red_final(c, 0, 2, nb, nb, pn, c->red_out.p + RO_RESULT + 1, mir + 1));
  double m[3];
  CHK(scalars_read(c, scalars_mirrored(3), m));
  *fn = sqrt(m[0]); *nrm = sqrt(m[1]); *absnrm = sqrt(m[2]);
  return 0;
}

// sparse update of the Dirichlet arrays (cfdh_solver.cpp::upload_bc): entry k describes vertex idx[k] completely
__global__ __launch_bounds__(TPB) void bc_scatter_kernel(int n, int ncomp, const int *__restrict__ idx, const unsigned char *__restrict__ flag,
                                                         const double *__restrict__ val, const double *__restrict__ mult,
                                                         unsigned char *__restrict__ bcflag, double *__restrict__ bcval,
                                                         double *__restrict__ bcmult) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= n) return;
  const int v = idx[k];
  bcflag[v] = flag[k];
  for (int i = 0; i < ncomp; i++) { bcval[(size_t)ncomp * v + i] = val[(size_t)ncomp * k + i]; bcmult[(size_t)ncomp * v + i] = mult[(size_t)ncomp * k + i]; }
}
int k_bc_scatter(cfdh_ctx *c, int n, int ncomp, const int *idx, const unsigned char *flag, const double *val, const double *mult) {
  hipLaunchKernelGGL(bc_scatter_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, ncomp, idx, flag, val, mult, c->bcflag.p,
                     c->bcval.p, c->bcmult.p);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------- functionals
// kind 0/1: drag / lift over exterior facets with the given marker (dfg_1.py:183-202)
__global__ __launch_bounds__(TPB) void draglift_kernel(int nfac, int marker, int nvo, const int *__restrict__ fcell,
                                                       const int *__restrict__ flocal, const int *__restrict__ fmarker,
                                                       const int *__restrict__ cells, const unsigned char *__restrict__ cown,
                                                       const double *__restrict__ coords,
                                                       const double *__restrict__ x, double mu, double *__restrict__ partial) {
  __shared__ double sh[4];
  double aD = 0, aL = 0;
  for (int k = blockIdx.x * TPB + threadIdx.x; k < nfac; k += gridDim.x * TPB) {
    if (fmarker[k] != marker) continue;
    const int e = fcell[k], fl = flocal[k];
    if (!cown[e]) continue;
    int vs[3];
    double X[3][2];
    for (int a = 0; a < 3; a++) { vs[a] = cells[3 * e + a]; X[a][0] = coords[2 * vs[a]]; X[a][1] = coords[2 * vs[a] + 1]; }
    const double det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
    double g[3][2];
    g[0][0] = (X[1][1] - X[2][1]) / det; g[0][1] = (X[2][0] - X[1][0]) / det;
    g[1][0] = (X[2][1] - X[0][1]) / det; g[1][1] = (X[0][0] - X[2][0]) / det;
    g[2][0] = (X[0][1] - X[1][1]) / det; g[2][1] = (X[1][0] - X[0][0]) / det;
    const double area = 0.5 * fabs(det);
    const double gfx = fl == 0 ? g[0][0] : (fl == 1 ? g[1][0] : g[2][0]);
    const double gfy = fl == 0 ? g[0][1] : (fl == 1 ? g[1][1] : g[2][1]);
    const double gl = hypot(gfx, gfy);
    const double n0 = gfx / gl, n1 = gfy / gl;  // n = -FacetNormal
    const double elen = 2.0 * area * gl;
    const double t0 = n1, t1 = -n0;
    double gu0 = 0, gu1 = 0;
    for (int a = 0; a < 3; a++) {
      const int uo = uoff(vs[a], nvo);
      const double ut = x[uo] * t0 + x[uo + 1] * t1;
      gu0 += ut * g[a][0]; gu1 += ut * g[a][1];
    }
    const double dn = gu0 * n0 + gu1 * n1;
    const int a1 = vs[(fl + 1) % 3], a2 = vs[(fl + 2) % 3];
    const double pm = 0.5 * (x[poff(a1, nvo)] + x[poff(a2, nvo)]);
    aD += elen * (mu * dn * n1 - pm * n0);
    aL -= elen * (mu * dn * n0 + pm * n1);
  }
  aD = block_sum(aD, sh);
  aL = block_sum(aL, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = aD; partial[gridDim.x + blockIdx.x] = aL; }
}
// kind 7: volume flux  sum_facets |e| n . (u_a + u_b) / 2  with the outward normal n = -grad(lambda_fl) / |grad(lambda_fl)|
// and |e| |grad(lambda_fl)| = |det|
__global__ __launch_bounds__(TPB) void flux_kernel(int nfac, int marker, int nvo, const int *__restrict__ fcell,
                                                   const int *__restrict__ flocal, const int *__restrict__ fmarker,
                                                   const int *__restrict__ cells, const unsigned char *__restrict__ cown,
                                                   const double *__restrict__ coords, const double *__restrict__ x,
                                                   double *__restrict__ partial) {
  __shared__ double sh[4];
  double q = 0;
  for (int k = blockIdx.x * TPB + threadIdx.x; k < nfac; k += gridDim.x * TPB) {
    if (fmarker[k] != marker) continue;
    const int e = fcell[k], fl = flocal[k];
    if (!cown[e]) continue;
    int vs[3];
    double X[3][2];
    for (int a = 0; a < 3; a++) { vs[a] = cells[3 * e + a]; X[a][0] = coords[2 * vs[a]]; X[a][1] = coords[2 * vs[a] + 1]; }
    const double det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
    const int a1 = (fl + 1) % 3, a2 = (fl + 2) % 3;
    // det * grad(lambda_fl) = rot(X[a1] - X[a2])
    const double gx = X[a1][1] - X[a2][1], gy = X[a2][0] - X[a1][0];
    const int u1 = uoff(vs[a1], nvo), u2 = uoff(vs[a2], nvo);
    const double sgn = det > 0 ? -0.5 : 0.5;
    q += sgn * (gx * (x[u1] + x[u2]) + gy * (x[u1 + 1] + x[u2 + 1]));
  }
  q = block_sum(q, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = q; partial[gridDim.x + blockIdx.x] = 0.0; }
}
// kind 2/3: int u.u, int p^2; with overlapping parts a cell is integrated only by
// the rank that owns its first vertex (cell_owned), so global sums count it once
__global__ __launch_bounds__(TPB) void l2_kernel(int nc, int nvo, const int *__restrict__ cells, const unsigned char *__restrict__ cown,
                                                 const double *__restrict__ coords, const double *__restrict__ x,
                                                 double *__restrict__ partial) {
  __shared__ double sh[4];
  double au = 0, ap = 0;
  for (int e = blockIdx.x * TPB + threadIdx.x; e < nc; e += gridDim.x * TPB) {
    if (cown && !cown[e]) continue;
    int vs[3];
    double X[3][2];
    for (int a = 0; a < 3; a++) { vs[a] = cells[3 * e + a]; X[a][0] = coords[2 * vs[a]]; X[a][1] = coords[2 * vs[a] + 1]; }
    const double det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
    const double area = 0.5 * fabs(det);
    double ux[3], uy[3], pp[3];
    for (int a = 0; a < 3; a++) { const int uo = uoff(vs[a], nvo); ux[a] = x[uo]; uy[a] = x[uo + 1]; pp[a] = x[poff(vs[a], nvo)]; }
    double su = 0, sp = 0;
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        const double m = (a == b ? 2.0 : 1.0);
        su += m * (ux[a] * ux[b] + uy[a] * uy[b]);
        sp += m * pp[a] * pp[b];
      }
    au += area * su * (1.0 / 12.0);
    ap += area * sp * (1.0 / 12.0);
  }
  au = block_sum(au, sh);
  ap = block_sum(ap, sh);
  if (threadIdx.x == 0) { partial[blockIdx.x] = au; partial[gridDim.x + blockIdx.x] = ap; }
}

// wall shear stress (solverBase.py:163-195): shear[v] += (1/|e|) oint lambda_v Tt ds = Tt/2 for both vertices of each
// exterior facet, Tt = T - (T.n) n, T = -sigma(u,p) n (the pressure part is purely normal).  A boundary vertex of a
// 2-D mesh receives two contributions, so the atomic sum is order-independent.
__global__ __launch_bounds__(TPB) void wss_kernel(int nfac, int nvo, const int *__restrict__ fcell, const int *__restrict__ flocal,
                                                  const int *__restrict__ cells, const double *__restrict__ coords,
                                                  const double *__restrict__ x, double mu, double *__restrict__ out) {
  const int k = blockIdx.x * TPB + threadIdx.x;
  if (k >= nfac) return;
  const int e = fcell[k], fl = flocal[k];
  int vs[3];
  double X[3][2], u[3][2];
  for (int a = 0; a < 3; a++) {
    vs[a] = cells[3 * e + a];
    X[a][0] = coords[2 * vs[a]]; X[a][1] = coords[2 * vs[a] + 1];
    const int uo = uoff(vs[a], nvo);
    u[a][0] = x[uo]; u[a][1] = x[uo + 1];
  }
  const double det = (X[1][0] - X[0][0]) * (X[2][1] - X[0][1]) - (X[1][1] - X[0][1]) * (X[2][0] - X[0][0]);
  double g[3][2];
  g[0][0] = (X[1][1] - X[2][1]) / det; g[0][1] = (X[2][0] - X[1][0]) / det;
  g[1][0] = (X[2][1] - X[0][1]) / det; g[1][1] = (X[0][0] - X[2][0]) / det;
  g[2][0] = (X[0][1] - X[1][1]) / det; g[2][1] = (X[1][0] - X[0][0]) / det;
  const double gfx = fl == 0 ? g[0][0] : (fl == 1 ? g[1][0] : g[2][0]);
  const double gfy = fl == 0 ? g[0][1] : (fl == 1 ? g[1][1] : g[2][1]);
  const double gl = hypot(gfx, gfy);
  const double n[2] = {-gfx / gl, -gfy / gl};
  double G[2][2] = {{0, 0}, {0, 0}};  // G_ij = d_i u_j
  for (int a = 0; a < 3; a++)
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 2; j++) G[i][j] += g[a][i] * u[a][j];
  const double E01 = 0.5 * (G[0][1] + G[1][0]);
  const double T[2] = {-2.0 * mu * (G[0][0] * n[0] + E01 * n[1]), -2.0 * mu * (E01 * n[0] + G[1][1] * n[1])};
  const double Tn = T[0] * n[0] + T[1] * n[1];
  const double Tt[2] = {0.5 * (T[0] - Tn * n[0]), 0.5 * (T[1] - Tn * n[1])};
  const int v1 = vs[(fl + 1) % 3], v2 = vs[(fl + 2) % 3];
  atomicAdd(out + 2 * (size_t)v1, Tt[0]); atomicAdd(out + 2 * (size_t)v1 + 1, Tt[1]);
  atomicAdd(out + 2 * (size_t)v2, Tt[0]); atomicAdd(out + 2 * (size_t)v2 + 1, Tt[1]);
}
int k_wss(cfdh_ctx *c, double *out) {
  if (c->gen) return c->dim == 3 ? kg3_wss(c, out) : kg_wss(c, out);
  if (c->dim == 3) return k3_wss(c, out);
  HIPCHK(c, hipMemsetAsync(out, 0, sizeof(double) * 2 * (size_t)c->nv, c->stream));
  if (c->nfac > 0)
    hipLaunchKernelGGL(wss_kernel, dim3((c->nfac + TPB - 1) / TPB), dim3(TPB), 0, c->stream, c->nfac, c->nvo, c->d_fac_cell.p,
                       c->d_fac_local.p, c->cells.p, c->coords.p, c->x.p, c->mu, out);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// kinds 0 .. 3 and 7: 256 blocks of partial sums by the kernel of the element family, then one tail for all of them
int k_functional(cfdh_ctx *c, int kind, int marker, double *out) {
  const int nb = 256;
  int nval = 2;  // rows of partial sums the kernel writes
  // (the generic branch below takes every kind <= 3: a negative kind ran the drag / lift kernel of a 2-D P2 / Q1 context)
  if (kind < 0 || kind > 8) return cfdh_fail(c, CFDH_E_ARG, "unknown functional kind %d", kind);
  if (kind == 8) {
    // flux of u_prev: the kernels of kind 7 (every element family) read the iterate through c->x, so they run on the other vector
    std::swap(c->x.p, c->xprev.p);
    const int rc = k_functional(c, 7, marker, out);
    std::swap(c->x.p, c->xprev.p);
    return rc;
  }
  if (kind >= 4 && kind <= 6) {
    const double *a = kind == 5 ? c->xprev.p : c->x.p;
    const double *b = kind == 6 ? c->xprev.p : nullptr;
    return v_norminf_diff(c, c->dim * c->nvo, a, b, out);
  } else if (c->dim == 3 && kind != 2 && kind != 3 && kind != 7) {
    return cfdh_fail(c, CFDH_E_ARG, "functional kind %d is not available for tetrahedra (2, 3: L2 norms; 4-6: inf-norms; 7: flux)", kind);
  } else if (c->gen && (kind <= 3 || kind == 7)) {  // the element's own quadrature (cfdh_gen.hip, cfdh_gen3.hip)
    CHK(c->dim == 3 ? kg3_functional_partials(c, kind, marker, nb) : kg_functional_partials(c, kind, marker, nb));
  } else if (c->dim == 3) {
    CHK(k3_functional_partials(c, kind, marker, nb));
    if (kind == 7) nval = 1;
  } else if (kind == 0 || kind == 1) {
    // a part without exterior facets (nfac == 0) still launches: the kernel then only writes zero partials, and the
    // rank takes part in the reduction below like every other one (skipping it would desynchronise the collectives)
    hipLaunchKernelGGL(draglift_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->nfac, marker, c->nvo, c->d_fac_cell.p,
                       c->d_fac_local.p, c->d_fac_marker.p, c->cells.p, c->cell_owned.p, c->coords.p, c->x.p, c->mu,
                       c->red_partial.p);
  } else if (kind == 7) {
    hipLaunchKernelGGL(flux_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->nfac, marker, c->nvo, c->d_fac_cell.p, c->d_fac_local.p,
                       c->d_fac_marker.p, c->cells.p, c->cell_owned.p, c->coords.p, c->x.p, c->red_partial.p);
  } else if (kind == 2 || kind == 3) {
    hipLaunchKernelGGL(l2_kernel, dim3(nb), dim3(TPB), 0, c->stream, c->nc, c->nvo, c->cells.p, c->cell_owned.p, c->coords.p,
                       c->x.p, c->red_partial.p);
  } else {
    return cfdh_fail(c, CFDH_E_ARG, "unknown functional kind %d", kind);
  }
  HIPCHK(c, hipGetLastError());
  ScalarRead h;
  CHK(scalars_finish(c, c->red_out.p, nval, 0, nb, &h));
  double v[2];
  CHK(scalars_read(c, h, v));
  if (kind == 0 || kind == 7) *out = v[0];
  else if (kind == 1) *out = v[1];
  else if (kind == 2) *out = sqrt(v[0]);
  else *out = sqrt(v[1]);
  return 0;
}

// ---------------------------------------------------------------- halo pack
__global__ __launch_bounds__(TPB) void halo_pack_kernel(int n, int nvo, const int *__restrict__ idx, const double *__restrict__ vec,
                                                        double *__restrict__ buf) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int v = idx[i];
  buf[3 * (size_t)i] = vec[2 * (size_t)v];
  buf[3 * (size_t)i + 1] = vec[2 * (size_t)v + 1];
  buf[3 * (size_t)i + 2] = vec[2 * (size_t)nvo + v];
}
__global__ __launch_bounds__(TPB) void halo_pack3_kernel(int n, int nvo, const int *__restrict__ idx, const double *__restrict__ vec,
                                                         double *__restrict__ buf) {
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const int v = idx[i];
  buf[4 * (size_t)i] = vec[3 * (size_t)v];
  buf[4 * (size_t)i + 1] = vec[3 * (size_t)v + 1];
  buf[4 * (size_t)i + 2] = vec[3 * (size_t)v + 2];
  buf[4 * (size_t)i + 3] = vec[3 * (size_t)nvo + v];
}
int k_halo_pack(cfdh_ctx *c, const double *vec) {
  const int n = (int)c->send_idx.n;
  if (n == 0) return 0;
  if (c->dim == 3) {
    hipLaunchKernelGGL(halo_pack3_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, c->nvo, c->send_idx.p, vec, c->send_buf.p);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(halo_pack_kernel, dim3((n + TPB - 1) / TPB), dim3(TPB), 0, c->stream, n, c->nvo, c->send_idx.p, vec,
                     c->send_buf.p);
  HIPCHK(c, hipGetLastError());
  return 0;
}
