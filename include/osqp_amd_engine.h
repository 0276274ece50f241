/*
 * osqp_amd_engine.h -- thin C-ABI shim between the C host code and the HIP
 * (gfx950) device engine.  Plain pointers and sizes only; no C++ or torch
 * types.  Each entry point names the reference function(s) it replaces
 * (paths relative to /root/reference).
 *
 * One `hipeng` = one QP resident on one GPU, with its own HIP stream; no
 * process-global state (unlike lin_sys/direct/pardiso/pardiso_loader.c:29-32).
 * All functions return 0 on success or a negative HIPENG_* code; they never
 * fall back to the CPU.
 */
#ifndef OSQP_AMD_ENGINE_H
#define OSQP_AMD_ENGINE_H

#include "osqp_amd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HIPENG_OK            0
#define HIPENG_ERR_NO_DEVICE (-101)  /* no HIP device / runtime failure at create */
#define HIPENG_ERR_HIP       (-102)  /* a HIP call failed (message on stderr)      */
#define HIPENG_ERR_ARG       (-103)
#define HIPENG_ERR_ALLOC     (-104)

typedef struct hipeng hipeng;

/* Mutable scalar parameters read by the kernels at launch. */
typedef struct {
  c_float sigma;        /* settings->sigma                                  */
  c_float alpha;        /* settings->alpha                                  */
  c_float pcg_eps_rel;  /* PCG stops at ||r||_2 <= max(eps_rel*||b||_2, eps_abs) */
  c_float pcg_eps_abs;
  c_int   pcg_max_iter; /* hard cap per linear solve                        */
  c_int   no_restart;   /* 1: any loss of positivity in the CG recurrence counts as negative
                           curvature (setup-time convexity probe); 0: restart at the rounding floor */
} hipeng_params;

/* Scalars produced by one residual evaluation (replaces the reductions inside
 * update_info / compute_pri_res / compute_dua_res / compute_pri_tol /
 * compute_dua_tol / compute_rho_estimate, src/auxil.c:13-52, 227-359, and the
 * cheap parts of is_primal_infeasible / is_dual_infeasible, :361-512). */
typedef struct {
  c_float pri_res_u, pri_res_s;     /* ||Einv(Ax-z)||, ||Ax-z||              */
  c_float z_u, z_s, Ax_u, Ax_s;     /* ||Einv z||, ||z||, ||Einv Ax||, ||Ax|| */
  c_float dua_res_u, dua_res_s;     /* ||Dinv(q+Px+A'y)|| (no cinv), scaled  */
  c_float q_u, q_s, Aty_u, Aty_s, Px_u, Px_s;
  c_float obj_scaled;               /* 1/2 x'Px + q'x in scaled space         */
  c_float dy_norm_u, dy_norm_s;     /* ||E dy_proj||, ||dy_proj||             */
  c_float dy_lhs;                   /* u'max(dy,0) + l'min(dy,0)              */
  c_float dx_norm_u, dx_norm_s;     /* ||D dx||, ||dx||                       */
  c_float q_dx;                     /* q'dx                                   */
  /* filled by hipeng_certificates only */
  c_float Atdy_u, Atdy_s;           /* ||Dinv A'dy_proj||, ||A'dy_proj||       */
  c_float Pdx_u, Pdx_s;             /* ||Dinv P dx||, ||P dx||                 */
  c_float Adx_viol;                 /* number of rows violating the A dx test */
} hipeng_scalars;

typedef struct {
  c_int admm_done;       /* iterations completed by the last hipeng_run_admm  */
  c_int pcg_iters_total; /* PCG iterations since create/reset                 */
  c_int pcg_iters_last;  /* PCG iterations of the most recent linear solve    */
  c_int pcg_iters_max;   /* max per solve since the last hipeng_run_admm call */
  c_int pcg_forced;      /* solves accepted at pcg_max_iter without converging */
  c_int graph_launches;
  c_int kernels_per_pcg_iter;
  c_int neg_curvature;   /* solves in which CG met p'Kp <= 0 (K not positive definite) */
  c_int resident;        /* 1: linear solves as resident launches (k_pcg_resident) */
} hipeng_stats;

/* Create the device-resident problem.  P (upper triangle) and A are the
 * workspace's scaled matrices in CSC with int64 indices; they are re-indexed
 * to int32 and uploaded as CSR(A) and the fused row matrix [P | A'].
 * Replaces the allocation + init part of init_linsys_solver
 * (src/lin_sys.c:56-75, lin_sys/direct/qdldl/qdldl_interface.c:177-323). */
int hipeng_create(hipeng **out, const csc *P, const csc *A, const c_float *q,
                  const c_float *l, const c_float *u, const c_float *rho_vec,
                  const hipeng_params *prm, int device);
void hipeng_destroy(hipeng *e);

int hipeng_set_params(hipeng *e, const hipeng_params *prm);
/* D, E, Dinv, Einv vectors (NULL = identity) and cost scaling c: needed only
 * for the unscaled norms of hipeng_residuals (src/scaling.c:177-192). */
int hipeng_set_scaling(hipeng *e, const c_float *D, const c_float *E, c_float c);
/* scale_data (src/scaling.c:44-156) on the device: Ruiz-equilibrates the resident raw problem
 * in place (`passes` = settings->scaling) and returns D, E, c and the scaled q, l, u, triu(P) and A
 * values (CSC order of the matrices given to hipeng_create) for the host mirrors. */
int hipeng_ruiz_scale(hipeng *e, c_int passes, c_float *D, c_float *E, c_float *cost,
                      c_float *q, c_float *l, c_float *u, c_float *Px, c_float *Ax);
int hipeng_matrices_changed(hipeng *e);   /* after an in-place rescale: preconditioner, z~, rhs parts */
int hipeng_upload_q(hipeng *e, const c_float *q);                      /* osqp_update_lin_cost, osqp.c:765 */
int hipeng_upload_bounds(hipeng *e, const c_float *l, const c_float *u); /* osqp_update_bounds, osqp.c:797 */
/* update_rho_vec of the vtable (qdldl_interface.c:396-410): re-uploads rho and
 * rebuilds the Jacobi preconditioner diag(P)+sigma+sum_i rho_i A_ij^2. */
int hipeng_upload_rho(hipeng *e, const c_float *rho_vec);
/* update_matrices of the vtable (qdldl_interface.c:381-393): new values, same
 * sparsity. */
int hipeng_upload_matrices(hipeng *e, const csc *P, const csc *A);
/* cold_start (auxil.c:155) / osqp_warm_start* (osqp.c:942-1007): x, y NULL =
 * keep; z is recomputed as A x on the device when x is given. */
int hipeng_cold_start(hipeng *e);
int hipeng_set_iterates(hipeng *e, const c_float *x, const c_float *y);
/* overwrite z; the PCG's warm-start image z~ = A x~ left by hipeng_set_iterates stays -- used when polish adopts
 * its (x, z, y) (src/polish.c:321-325) or puts the ADMM iterates back */
int hipeng_set_z(hipeng *e, const c_float *z);

/* Run `count` ADMM iterations (osqp.c:356-370: swap, update_xz_tilde,
 * update_x, update_z, update_y) entirely on the device. */
int hipeng_run_admm(hipeng *e, c_int count);
/* hipeng_run_admm followed by hipeng_residuals for a window that ends where the residuals are looked at: the residual pass
 * is enqueued directly behind the window and both come back after one wait.  *have = 1: *out holds the scalars of the
 * iterate the call ended on.  *have = 0 (the window needed a continuation, a resident launch gave up, a slow-wait record
 * was cleared, or OSQP_AMD_FUSED_CHECK=0): *out is untouched and the caller asks hipeng_residuals. */
int hipeng_run_admm_check(hipeng *e, c_int count, hipeng_scalars *out, int *have);
/* the rule behind *have, on the fields of the window's read-back (no device needed) */
int hipeng_early_scalars_usable(c_int remaining, int res_fail, int res_slow, int res_repub);
/* Evaluate all residual scalars for the current iterates (device reductions,
 * one small D2H copy). */
int hipeng_residuals(hipeng *e, hipeng_scalars *out);
/* Second stage of the infeasibility tests: A'dy, P dx, A dx (auxil.c:401-417,
 * 456-497).  eps_dx = eps_dual_inf * ||dx|| threshold for the A dx row test;
 * unscaled != 0 applies Einv to A dx first. */
int hipeng_certificates(hipeng *e, c_float eps_dx, int unscaled, hipeng_scalars *inout);
/* Copy device vectors to host arrays (NULL = skip).  dy is the projected
 * delta_y when `dy_projected` is nonzero. */
int hipeng_download(hipeng *e, c_float *x, c_float *y, c_float *z, c_float *dx,
                    c_float *dy, int dy_projected);
int hipeng_get_stats(hipeng *e, hipeng_stats *st);
int hipeng_reset_stats(hipeng *e);   /* zero the counters (after the setup-time convexity probe) */
int hipeng_sync(hipeng *e);

/* Plugin-boundary solve (LinSysSolver.solve, include/types.h:300-301;
 * qdldl_interface.c:350-376): b = [sigma x - q ; z - y/rho] on the host is
 * overwritten by [x_tilde ; z_tilde]. */
int hipeng_kkt_solve(hipeng *e, c_float *b);
/* The same solve without the refinement step hipeng_kkt_solve takes on the direct forms (form 3 / 4): one application of
 * the inverse the engine iterates with.  Used by the setup-time convexity probe and the direct-solve tests. */
int hipeng_kkt_solve_unrefined(hipeng *e, c_float *b);

/* Kernel-level entry points used by the parity tests (host in, host out):
 * which = 0: y = A x   (mat_vec, lin_alg.c:241-271)
 *         1: y = A' x  (mat_tpose_vec, lin_alg.c:273-322)
 *         2: y = P x   (mat_vec + mat_tpose_vec skip_diag on triu P) */
int hipeng_spmv(hipeng *e, int which, const c_float *x, c_float *y);
/* The same products on device pointers (d_x, d_y: n or m doubles in HBM), enqueued on the engine's stream
 * without a sync -- hipeng_sync() orders them before other streams read d_y.  Building block of the
 * row-partitioned multi-GPU variant. */
int hipeng_spmv_dev(hipeng *e, int which, const c_float *d_x, c_float *d_y);
/* Time `reps` back-to-back launches of one hot kernel on the engine stream with
 * HIP events; returns average microseconds per launch in *usec.
 * which = 0: k_cg_A, 1: k_cg_B, 3 / 4: k_cg_A update-only / apply-only (split mode), 5: k_pcg_init,
 * 6: k_cg_A + k_cg_B in loop order, 7: an empty dependent launch, 8: k_pcg_init + k_pcg_resident (the
 * right-hand side and the whole linear solve of one ADMM iteration; resident engines only). */
int hipeng_time_kernel(hipeng *e, int which, int reps, double *usec);
/* Algorithmic bytes of one launch of the kernels above. */
int hipeng_kernel_bytes(hipeng *e, int which, double *bytes);
int hipeng_is_split(hipeng *e);   /* k_cg_A as two launches (update-only + apply-only)? */
/* For the tests: how the PCG kernels see (P, A).  Copies host-side fields only (no kernel, no launch): out[0] dense diagonal
 * blocks of P, [1] rows inside them, [2] stream blocks of A, [3] long (one-wavefront) rows of A, [4] huge rows of A, [5] huge
 * rows folded into k_cg_B, [6] split, [7] A has 16-bit column ids, [8] M = [P | A'] has them, [9] the matrix k_cg_B streams
 * (the remainder Mr when it exists, else M) has them, [10] long rows of that matrix, [11] gridA, [12] gridM; the rest 0. */
int hipeng_pcg_layout(hipeng *e, long long out[16]);
/* Slack-like variables (one entry in their column of A, no coupling in P) are eliminated from the linear system exactly
 * (engine_aux_kernels.h, k_elim_refresh; launch-per-step engines).  hipeng_row_eliminated: does row i of A carry such a variable?
 * hipeng_elim_count: how many variables are eliminated. */
int hipeng_row_eliminated(hipeng *e, c_int i);
c_int hipeng_elim_count(hipeng *e);
/* For the tests: copies one per-row array of the elimination to out[m] (reads only, no kernel).  which = 0: rhoe (the row's
 * effective rho), 1: ecoef (A(i, y)), 2: edinv (1 / D_y), 3: xte (x~ of the row's eliminated variable); rows without an
 * eliminated variable hold rho, 0, 0 and whatever was there.  An error when no variable is eliminated (the arrays do not exist). */
int hipeng_elim_peek(hipeng *e, int which, c_float *out);
/* Resident PCG (the reduced matrix K = P + sigma I + A' rho A held in registers, one launch per linear
 * solve; engine_pcg_resident.h, k_pcg_resident).  out[0] structures built, [1] in use, [2] entries of K per thread,
 * [3] workgroups, [4] nnz(K), [5] LDS bytes per workgroup, [6] PCG iterations of the most recent linear
 * solve, [7] pipelined recurrences switched off for the current K, [8] true-residual checks that failed since create
 * (each continued its solve from the true residual), [9] form (1: k_pcg_resident, 2: k_pcg_blockres), [10] launches that
 * gave up waiting since create (each sends the rest of its run_admm call to the launch-per-step kernels), [11] waits inside
 * resident launches that ended well but took more than 50 us, [12] the longest of them in ticks of the 100 MHz clock,
 * [13] flags / granules stored again by a workgroup whose own wait went on, [14] give-ups in a row (the third ends the mode
 * for this engine; a run_admm call without one starts the count again), [15] block-direct form: coupling rows of A carried as the low-rank term (0: the plain form, huge rows only).  [1] stays 1 until that third one. */
int hipeng_resident_info(hipeng *e, long long out[16]);
/* k_pcg_resident since create: out[0] vector trips of its launches (a pipelined solve of N iterations makes N + 3: the
 * start-up product, N iterations, one trip that only learns "converged", the true-residual check; N + 2 when the trip
 * predicted to be the last carried x - x0 and was the last, N + 4 when it was not), [1] launches that ran a solve,
 * [2] predicted last trips whose products served the check (hits), [3] predicted last trips that were not the last
 * (misses), [4] predicted trips switched off for the current K (misses outnumbered hits over a window of 16 solves),
 * [5] the switch OSQP_AMD_RESIDENT_PREDICT as the engine read it, [6] solves and [7] misses minus hits of the current window. */
int hipeng_resident_trips(hipeng *e, long long out[8]);
/* For the CPU tests (needs no device): the host side of the resident set-up -- symbolic K, row partition, positions in
 * the exchanged vector, register layout -- for a grid of exactly `nwg` workgroups (nwg > 0) or, nwg < 0, with the grid sized
 * to the problem as the engine does on a machine of -nwg CUs (stats[4] then tells the grid).  stats: [0] qualifies, [1] entries of K per thread,
 * [2] length of the exchanged vector, [3] nnz(K), [4] workgroups that own rows, [5] most rows, [6] most entries per
 * workgroup, [7] threads that hold entries (448).  Optional outputs may be NULL. */
int hipeng_resident_plan(const csc *P, const csc *A, int nwg, long long stats[8], int *Kptr, int *Kcol, int *kdst, long long cap,
                         unsigned short *rowpos, unsigned short *slotcol, int *wg4);
/* The contribution lists of that plan, from which k_form_K_lists forms the values of K: entry e of K (in the order of the
 * plan's Kcol) is P_ij + sigma [i == j] plus the terms Kcp[e] .. Kcp[e + 1]; term q is rho_k a_ki a_kj with a_ki at slot Kcm[q] of
 * M = [P | A'] (its column there is n + k) and a_kj at slot Kca[q] of the CSR copy of A, rows k ascending.  Kcp: nnz(K) + 1, Kcm /
 * Kca: cap terms at most; outputs may be NULL.  Returns the number of terms (the sum over the rows of A of nnz^2), -1 when the
 * problem does not qualify, -2 when the lists are switched off (OSQP_AMD_FORM_K_LISTS=0) or over their budget
 * (OSQP_AMD_FORM_K_LIST_MB, default 128; more than 2^31 - 1 terms count as over), or a HIPENG_ERR_* code. */
long long hipeng_resident_plan_lists(const csc *P, const csc *A, int nwg, int *Kcp, int *Kcm, int *Kca, long long cap);
/* How the resident PCG forms K: out[0] 1 from contribution lists (k_form_K_lists), 0 by the merge on the device (k_form_K);
 * [1] terms, [2] bytes of the list arrays on the device, [3] their budget in bytes. */
int hipeng_form_k_info(hipeng *e, long long out[4]);
/* For the tests: K as the resident kernel holds it, as triplets; returns nnz(K) or a negative code. */
long long hipeng_resident_dump(hipeng *e, int *row, int *col, double *val, long long cap);

/* Dense-direct solve (engine.hip FORM_DENSE_DIRECT, csrc/dense_direct.h): test / measurement hook for its blocked inversion.
 * A: n x n row-major symmetric positive definite host matrix, n a multiple of 128; Ainv: its inverse (explicit, by blocked
 * Gauss-Jordan on v_mfma_f64_16x16x4_f64); ms[0]: device time of the inversion, ms[1]: of one n x n x n GEMM of the same
 * kernel.  Returns 0, 1 when a pivot was not positive, or a HIPENG_ERR_* code.  The route is the blocked Cholesky one unless
 * OSQP_AMD_DENSE_CHOL=0 (then the block sweeps); the GEMM kernel is the one the engines of this process use. */
int hipeng_dense_invert_selftest(int n, const double *A, double *Ainv, double *ms);
/* The same inversion with both choices explicit: route 0 block sweeps (dd_invert_sweep), 1 blocked Cholesky (dd_invert_chol);
 * gemm 0 k_dd_gemm_tn (operands from global memory), 1 k_dd_gemm_tn_lds.  What the process's engines have latched from
 * OSQP_AMD_DENSE_GEMM_LDS is as it was afterwards.  Returns 0, 1 when a pivot was not positive, or a HIPENG_ERR_* code. */
int hipeng_dense_invert_route(int n, const double *A, double *Ainv, int route, int gemm);
/* The two once-per-process switches of the dense-direct solve as this process has latched them: out[0] the LDS-staged GEMM kernel
 * (OSQP_AMD_DENSE_GEMM_LDS), out[1] Cholesky before the sweeps (OSQP_AMD_DENSE_CHOL); 0 / 1, or -1 while no engine has read it. */
int hipeng_dense_switches(int out[2]);
/* One launch of one of its GEMM kernels by name (kernel 0: k_dd_gemm_tn, 1: k_dd_gemm_tn_lds), grid (ceil(N / 128), ceil(M / 128),
 * slices):  C = beta C + alpha T' diag(w) B.  T: [K][ldt] (T' is M x K), B: [K][ldb], w: [K] or NULL, all row-major on the host.
 * C: [Mp][ldc] with Mp = M rounded up to a multiple of 128, in: C0, out: the result -- rows M.. and columns N.. are uploaded and
 * downloaded too, so that the caller can see they were left alone.  Masks as the kernels have them: 128 x 128 tiles whose rows start in
 * [sr0, sr1) or columns in [sc0, sc1) and, with `lower`, tiles above the diagonal are not written; kmode 1 / 2 starts k at the tile's first
 * column / row.  ksl > 0: split K -- ceil(K / ksl) slices into a scratch, summed into C by k_dd_sum_slices (M = 128, beta = 0 and no
 * masked tile: that kernel sums 128 rows and overwrites).  HIPENG_ERR_ARG and no launch for an odd ld, an ld below its extent (ldt < M,
 * ldb < N, ldc < N) or a split K outside those limits.  Returns 0 or a HIPENG_ERR_* code. */
int hipeng_dense_gemm_selftest(int kernel, int M, int N, int K, const double *T, int ldt, const double *B, int ldb, const double *w,
                               double *C, int ldc, double alpha, double beta, int sr0, int sr1, int sc0, int sc1, int lower, int kmode, int ksl);

/* The OSQP_AMD_* switches of the single-QP engine (the table ahead of struct hipeng in csrc/engine.hip), for the tests: neither call
 * needs a device.  hipeng_switch_row: row `index` -- name, kind (0 flag: atoi != 0, 1 int: atoi, 2 double: atof, 3 pair of ints: "a,b",
 * 4 text), default as text ("unset" where an unset variable is a value of its own: the engine then works the default out from the
 * problem or the caller), that bit, a one-line description; outputs may be NULL, def_text holds def_cap bytes.  Returns the number of rows.
 * hipeng_switch_values: what the engine's reader makes of the current environment, two doubles per row for `rows` rows at most --
 * out[2 i] the value (-1 where unset is distinct and the variable is not set; the length of a text), out[2 i + 1] the second
 * number of a pair, else 0.  Returns the number of rows. */
int hipeng_switch_row(int index, const char **name, int *kind, char *def_text, int def_cap, int *unset_distinct, const char **what);
int hipeng_switch_values(double *out, int rows);

/* O(nnz) parts of the single-QP engine's solution derivatives (csrc/kkt_sens.h: k_sens_grad, k_sens_tan_rhs).  One hipsens per
 * workspace, created at its first osqp_amd_adjoint / osqp_amd_tangent call and kept until cleanup; every call runs on the stream
 * of `pe`, the polish-mode instance's engine whose solves it accompanies.  P, A: the patterns in the caller's CSC order.
 * hipsens_set_point: the point (x~, y~ on the active rows and 0 elsewhere, act = -1 / +1 / 0 per row, D, E (NULL = ones), c).
 * hipsens_grad: dPx [nnzP] / dAx [nnzA] (NULL = skip) of the adjoint from rx [n] and rnu scattered to the m rows.
 * hipsens_tan_rhs: g [ndir][n + m], per direction -(dq~ + dP~ x~ + dA~' y~_act) and, on the rows, db~ - dA~ x~ (0 on an
 * inactive row); any NULL tangent = 0. */
typedef struct hipsens hipsens;
int hipsens_create(hipsens **out, c_int n, c_int m, c_int nnzP, c_int nnzA, int device);
void hipsens_destroy(hipsens *s);
int hipsens_set_point(hipsens *s, hipeng *pe, const c_float *x, const c_float *yact, const c_int *act,
                      const c_float *D, const c_float *E, c_float c);
int hipsens_grad(hipsens *s, hipeng *pe, const csc *P, const csc *A, const c_float *rx, const c_float *rnu,
                 c_float *dPx, c_float *dAx);
int hipsens_tan_rhs(hipsens *s, hipeng *pe, const csc *P, const csc *A, c_int ndir, const c_float *dq, const c_float *dl,
                    const c_float *du, const c_float *dPx, const c_float *dAx, c_float *g);

/* The device side of osqp_amd_verify (csrc/verify.h: k_ver_point, k_ver_cert, k_ver_combine).  One hipver per workspace, created at its
 * first osqp_amd_verify call and kept until cleanup; every call runs on the stream of `e`, the workspace's engine, and returns with it
 * synchronised.  It holds the patterns of triu(P) and A (hipver_create reads the CSC pointers and indices only, and refuses arrays
 * that are not a pattern with HIPENG_ERR_ARG), device copies of the raw values and the partial records; nothing of `e` is read or
 * written.  HIPENG_ERR_ALLOC: the host or the device has no room (the caller destroys what was made).
 * hipver_upload: the raw values named by `parts` (bit 0 Px [nnzP], 1 Ax [nnzA], 2 q [n], 3 l [m], 4 u [m]) from host arrays.
 * hipver_run: the record V [16] of the host arrays x, dx [n], y, dy [m] against the values last uploaded.
 * hipver_info (no device, no object): the kernels' constants -- out[0] threads per workgroup, [1] rows (or columns) a workgroup takes
 * per sweep, [2] the most workgroups of a launch, [3] the number of entries above which a row or column is taken by a whole workgroup.
 * The grid of a launch is min(out[2], ceil(max(n, m) / out[1])): it follows from the sizes and these constants alone.
 * hipver_uploads: uploads since create of P values, of A values, of q / l / u (one counter: each vector counts one). */
typedef struct hipver hipver;
int hipver_create(hipver **out, const csc *P, const csc *A, int device);
void hipver_destroy(hipver *v);
int hipver_upload(hipver *v, hipeng *e, int parts, const c_float *Px, const c_float *Ax, const c_float *q, const c_float *l,
                  const c_float *u);
int hipver_run(hipver *v, hipeng *e, const c_float *x, const c_float *y, const c_float *dx, const c_float *dy, c_float eps_abs,
               c_float eps_rel, c_float eps_prim_inf, c_float eps_dual_inf, c_float *V);
int hipver_info(int out[4]);
int hipver_uploads(const hipver *v, c_int out[3]);

#ifdef __cplusplus
}
#endif
#endif
