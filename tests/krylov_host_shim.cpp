// extern "C" wrappers around csrc/cfdh_krylov_host.hpp for tests/test_krylov_host.py: compiled by the host compiler, loaded with
// ctypes.  No HIP, no libcfdh.so.
#include "cfdh_krylov_host.hpp"

using namespace cfdh_krylov;

extern "C" {

int kh_gram_solve(int k, const double *hd, double *y, int *rank) { return gram_solve(k, hd, y, rank) ? 1 : 0; }

double kh_gs_scale(double ww, double hh2) { return gs_scale(ww, hh2); }

void *kh_lsq_new(int m) { return new ArnoldiLsq(m); }
void kh_lsq_free(void *p) { delete (ArnoldiLsq *)p; }
void kh_lsq_start(void *p, double beta) { ((ArnoldiLsq *)p)->start(beta); }
int kh_lsq_add_column(void *p, int j, const double *h, double hnorm) { return ((ArnoldiLsq *)p)->add_column(j, h, hnorm) ? 1 : 0; }
double kh_lsq_residual(void *p, int j) { return ((ArnoldiLsq *)p)->residual(j); }
void kh_lsq_solve(void *p, int j, double *y) {
  const double *s = ((ArnoldiLsq *)p)->solve(j);
  for (int i = 0; i < j; i++) y[i] = s[i];
}

void *kh_ahead_new() { return new LaunchAhead(); }
void kh_ahead_free(void *p) { delete (LaunchAhead *)p; }
void kh_ahead_start(void *p, double beta, int e_its, int its) { ((LaunchAhead *)p)->start(beta, e_its, its); }
void kh_ahead_observe(void *p, double res, double tol, int its) { ((LaunchAhead *)p)->observe(res, tol, its); }
int kh_ahead_need(void *p) { return ((LaunchAhead *)p)->need; }
void kh_ahead_set_need(void *p, int need) { ((LaunchAhead *)p)->need = need; }
int kh_ahead_in_flight(void *p, int sync_now, int lagmax) { return ((LaunchAhead *)p)->in_flight(sync_now != 0, lagmax); }
int kh_ahead_process_upto(void *p, int j, int jl, int maxl, int sync_now) { return ((LaunchAhead *)p)->process_upto(j, jl, maxl, sync_now != 0); }

// flow: 0 proceed, 1 retry, 2 stop; watchdog: 0 quiet, 1 fp32 copy off, 2 refinement on
void kh_between_cycles(int j_prev, double beta, double est_prev, double tol, double bn, double beta_start, double last_true, int use32,
                       int gs_refine_long, int no_attainable_stop, int *flow, int *watchdog, double *last_true_out) {
  const BetweenCycles d = between_cycles(j_prev, beta, est_prev, tol, bn, beta_start, last_true, use32 != 0, gs_refine_long != 0, no_attainable_stop != 0);
  *flow = (int)d.flow;
  *watchdog = (int)d.watchdog;
  *last_true_out = d.last_true;
}

}
