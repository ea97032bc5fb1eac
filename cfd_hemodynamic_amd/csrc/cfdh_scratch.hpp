// Layout of the two scratch buffers every scalar reduction and read-back goes through ("Scalar reductions and
// read-backs"): the device words cfdh_ctx::red_out and the pinned, host-mapped words cfdh_ctx::h_pinned / h_pinned_dev.
// Every user names its words here; the static_asserts keep the regions apart and inside the allocations of
// cfdh_alloc_reduction.  Plain C++: no HIP needed.
#pragma once

#define CFDH_KSP_RESTART_MAX 1000  // largest cfdh_options.ksp_restart: the longest copy read-back is sized by it

// red_out: RO_x = first word, RO_x_N = words
enum {
  RO_WORDS = 1024,
  RO_RESULT = 0, RO_RESULT_N = 4,            // results of the reduce-and-read calls (v_dot .. k_functional), at most three today
  RO_POWER = 4, RO_POWER_N = 1,              // norm of the power iteration for lambda_max(D^-1 A00)
  RO_MEAN = 8, RO_MEAN_N = 2,                // v_sub_mean: [sum, count]
  RO_LEAN_S2 = 12, RO_LEAN_S2_N = 1,         // squared residual norm of the lean prologue / epilogue
  RO_HOST_SCALAR = 16, RO_HOST_SCALAR_N = 1, // comm_allreduce_host: one host scalar on its way through the all-reduce
  RO_AMG_NORM = 20, RO_AMG_NORM_N = 1,       // power iteration of the device-side hierarchy set-up
  RO_FLOW = 24, RO_FLOW_N = 8,               // the 8 integrals of cfdh_flow_integrals (RO_RESULT holds 4)
  RO_END = RO_FLOW + RO_FLOW_N
};
static_assert(RO_RESULT + RO_RESULT_N <= RO_POWER && RO_POWER + RO_POWER_N <= RO_MEAN && RO_MEAN + RO_MEAN_N <= RO_LEAN_S2 &&
                  RO_LEAN_S2 + RO_LEAN_S2_N <= RO_HOST_SCALAR && RO_HOST_SCALAR + RO_HOST_SCALAR_N <= RO_AMG_NORM && RO_AMG_NORM + RO_AMG_NORM_N <= RO_FLOW && RO_END <= RO_WORDS,
              "red_out slots overlap or leave the buffer");

// h_pinned: HP_x = first word, HP_x_N = words
enum {
  HP_WORDS = 2048,
  HP_COPY = 0, HP_COPY_N = 1008,          // target of the copy read-backs (scalars_read of a handle that is not mirrored)
  HP_MIRROR = 1008, HP_MIRROR_N = 512,    // host-mapped copies of reduced scalars, written by kernels
  HP_CB_STAGE = 1520, HP_CB_STAGE_N = 512,  // staging of the callback all-reduce (longer vectors go through cfdh_ctx::h_big)
  HP_IPCS = 2032, HP_IPCS_N = 4,          // mirror of the pressure-correction Krylov drivers: |r|^2, done, its, bad
  HP_END = HP_IPCS + HP_IPCS_N
};
enum { SCALARS_MIRROR_MAX = 64 };  // most scalars one reduce-and-read call mirrors
static_assert(HP_COPY + HP_COPY_N <= HP_MIRROR && HP_MIRROR + HP_MIRROR_N <= HP_CB_STAGE && HP_CB_STAGE + HP_CB_STAGE_N <= HP_IPCS &&
                  HP_END <= HP_WORDS,
              "h_pinned regions overlap or leave the buffer");
static_assert(HP_COPY_N >= CFDH_KSP_RESTART_MAX + 4, "second Gram-Schmidt pass: ksp_restart + 4 words in one copy");
static_assert(HP_COPY_N >= 8 * 9, "Gram system of the projected guess: 8 (k + 1) words, k <= 8");
static_assert(HP_MIRROR_N >= SCALARS_MIRROR_MAX && HP_MIRROR_N >= 3 + 8, "mirror: the lean prologue publishes 3 + k words, k <= 8");
