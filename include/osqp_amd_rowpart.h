/* osqp_amd_rowpart.h -- ONE QP solved over several GPUs by rows (BASELINE config 5
 * "1 -> 8 MI355X"), driven from C.
 *
 * The reference has no counterpart: its linear solve is one thread (lin_sys/direct/qdldl/qdldl_interface.c:216) and a
 * GPU / indirect solver is a TODO (ROADMAP.md:1-3).  What this replaces is therefore the reference's osqp_solve loop
 * itself (src/osqp.c:354-532: compute_rhs / solve / update_x / update_z / update_y, src/auxil.c:161-225; residuals and
 * termination src/auxil.c:240-359, 681-740; rho adaptation src/auxil.c:13-74) for a problem whose rows of A and
 * columns of triu(P) are sharded over `world` ranks, one process per GPU:
 *
 *   - every rank holds the n-vectors (x, x~, q, the PCG vectors) replicated and the m-vectors (z, y, l, u, rho) of its
 *     own rows only; its shard (P_g, A_g) is resident in an ordinary engine (hipeng, set up with scaling = 0 on
 *     already scaled data);
 *   - the data-path traffic is ONE all-reduce of an n-vector per PCG iteration (K u = sigma u + sum_g [P_g u +
 *     A_g' rho_g (A_g u)]), one per ADMM iteration for the right-hand side, and two n-vectors + six scalars at a
 *     termination check: two all-reduces per check, and two more (2n + 1 doubles summed, two doubles maximised) once
 *     osqp_amd_rp_set_infeasibility has switched the infeasibility tests on, so at most four.  Every rank holds the
 *     same bits after an all-reduce, so the PCG scalars are computed redundantly on each device and need no
 *     collective of their own;
 *   - the whole loop -- kernels, collectives, the decision when a PCG solve has converged -- is issued from
 *     osqp_amd_rp_solve on the shard engine's stream; the host reads one flag per group of PCG iterations and a
 *     handful of scalars per termination check.
 *
 * The collective is a callback, so that the caller's process group decides how ranks talk: the built-in provider
 * (osqp_amd_rp_use_rccl) calls ncclAllReduce of librccl.so on the engine's stream (RCCL over xGMI); a test harness can
 * pass any function with the same meaning (tests: torch.distributed with gloo).
 *
 * Statuses: OSQP_SOLVED, OSQP_SOLVED_INACCURATE, OSQP_MAX_ITER_REACHED, and after osqp_amd_rp_set_infeasibility
 * OSQP_PRIMAL_INFEASIBLE, OSQP_DUAL_INFEASIBLE and their inaccurate forms with certificates (no polish and no matrix
 * updates in this variant).  q, the bounds, the iterates and rho of a live handle can be replaced (osqp_amd_rp_update_*,
 * osqp_amd_rp_warm_start).  All functions return 0 or a HIPENG_ERR_* code unless stated otherwise. */
#ifndef OSQP_AMD_ROWPART_H
#define OSQP_AMD_ROWPART_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osqp_amd_rp osqp_amd_rp;

/* In-place all-reduce of `count` doubles at device address `buf` over all ranks; op 0 = sum, 1 = max.  Must be ordered
 * after the work already in `hip_stream` and before work submitted to it later (a stream-ordered collective on that
 * stream, or a synchronous one that synchronises the stream itself).  Returns 0 on success. */
typedef int (*osqp_amd_rp_allreduce_fn)(void *user, void *buf, long long count, int op, void *hip_stream);

typedef struct {
  double rho, sigma, alpha, eps_abs, eps_rel, adaptive_rho_tolerance, pcg_eps_rel;
  int max_iter, check_termination, adaptive_rho, adaptive_rho_interval, scaled_termination, pcg_max_iter;
} osqp_amd_rp_settings;                 /* meaning and defaults of the fields: OSQPSettings (include/osqp_amd_types.h) */

typedef struct {
  int status;                           /* OSQP_SOLVED, OSQP_SOLVED_INACCURATE or OSQP_MAX_ITER_REACHED (include/osqp_amd_types.h); with the infeasibility
                                           tests on also OSQP_PRIMAL_INFEASIBLE, OSQP_DUAL_INFEASIBLE and their _INACCURATE forms */
  int iter, rho_updates;
  long long pcg_iters, collectives;
  double obj_val, pri_res, dua_res, rho_estimate;
} osqp_amd_rp_info;

/* shard_engine: a hipeng (osqp_amd_engine.h) that holds this rank's (P_g, A_g) with scaling = 0: n columns, m_loc rows.
 * q, D: n doubles; l_loc, u_loc, E_loc: m_loc doubles (the scaled problem and its scaling, src/scaling.c:44-156);
 * c: cost scaling; has_eq_any: some rank has an equality row (tightens the PCG stop as osqp_solve does). */
osqp_amd_rp *osqp_amd_rp_create(void *shard_engine, const double *q, const double *l_loc, const double *u_loc,
                                const double *D, const double *E_loc, double c, int m_total, int has_eq_any,
                                const osqp_amd_rp_settings *settings, int world, int rank,
                                osqp_amd_rp_allreduce_fn allreduce, void *user);
/* Replace the callback by ncclAllReduce on the engine's stream.  unique_id: the ncclUniqueId bytes of rank 0
 * (osqp_amd_rp_rccl_unique_id), the same on every rank.  Collective: every rank calls it.  (NULL, 0) detaches again. */
int  osqp_amd_rp_rccl_unique_id(void *out, int cap_bytes);          /* returns the number of bytes written, < 0 on error */
int  osqp_amd_rp_use_rccl(osqp_amd_rp *rp, const void *unique_id, int id_bytes);
/* A handle starts from zero iterates and settings->rho.  Every later solve on the same handle continues as the reference's
 * osqp_solve does on one workspace: from the iterates x, x~, z, y the previous solve left, with the rho that solve ended on
 * (not settings->rho), and info->rho_updates counts on across solves; rho per row and the preconditioner are built at
 * the first solve and again only when rho changes.  A PCG solve that meets p'Kp <= 0 (K not positive definite: the problem
 * is not convex) ends the call with HIPENG_ERR_ARG; the handle can still be freed. */
int  osqp_amd_rp_solve(osqp_amd_rp *rp, osqp_amd_rp_info *info);
/* x: n doubles (unscaled, the same on every rank); y_loc: m_loc doubles (unscaled duals of this rank's rows) */
int  osqp_amd_rp_get_solution(osqp_amd_rp *rp, double *x, double *y_loc);
void osqp_amd_rp_free(osqp_amd_rp *rp);

/* ---- infeasibility (is_primal_infeasible / is_dual_infeasible, src/auxil.c:361-512; placed as check_termination does,
 * src/auxil.c:681-783, its approximate branch with 10 x the tolerances at max_iter included) ----
 * Off until this call; a tolerance of 0 leaves that test off, and with both 0 (or without the call) a solve launches the
 * kernels, makes the collectives and leaves the bits it did before the tests existed (the buffers of the tests and of
 * osqp_amd_rp_update_bounds, 4 n + 4 m_loc + 1 doubles of device memory, are part of every handle all the same).  With a test on, an iteration that
 * ends in a termination check keeps x and y as they were before update_x / update_y, and the check forms dx, the projected
 * dy and seven more scalars: TWO more all-reduces per check (a sum of [P_g dx ; A_g' dy ; u'dy+ + l'dy-], 2n + 1 doubles,
 * and a max of [|E dy|_inf ; the largest violation of a row of A dx]) and no further synchronisation: the scalars travel
 * in the read-back of the fifteen.  Every decision is taken on all-reduced or replicated values, so all ranks leave the
 * loop together.  Every rank must make the call with the same values.
 * On an infeasible status obj_val is +-OSQP_INFTY, osqp_amd_rp_get_solution returns NaN, and the iterates x, x~, z, y of
 * the handle are zero again (cold_start; rho and rho_updates stay). */
int  osqp_amd_rp_set_infeasibility(osqp_amd_rp *rp, double eps_prim_inf, double eps_dual_inf);
/* The certificate of the last solve, as store_solution leaves it (src/auxil.c:545-555): dy (times E unless
 * scaled_termination) or dx (times D) divided by its infinity norm over all ranks.  dual_inf_cert: n doubles, the same on
 * every rank; prim_inf_cert_loc: m_loc doubles, this rank's rows.  The one the last status does not call for is NaN. */
int  osqp_amd_rp_get_certificates(osqp_amd_rp *rp, double *dual_inf_cert, double *prim_inf_cert_loc);

/* ---- a live handle.  Collective like osqp_amd_rp_use_rccl: every rank calls each of them.  The arrays are UNSCALED host
 * arrays; they are scaled on the device with the handle's D, E, c.  The iterates stay, so the next solve is warm. ----
 * update_lin_cost: q_s = c D q (n doubles).  update_bounds: l_loc, u_loc (m_loc doubles) are clamped to +-OSQP_INFTY and
 * scaled by E; one max-all-reduce of three flags comes before anything is written: l > u on some rank makes EVERY rank
 * return 1 with the handle unchanged; a row that changes class (free / inequality / equality) on some rank makes every rank
 * rebuild rho per row and the preconditioner; has_eq_any is refreshed.  Both reset rho_updates as the reference's
 * reset_info does.  warm_start: x (n doubles or NULL) gives x_s = Dinv x, x~ = x_s and z = A_g x_s on the rank's rows;
 * y_loc (m_loc doubles or NULL) gives y_s = c Einv y (src/osqp.c:942-1010).  update_rho: rho <= 0 returns 1 and changes
 * nothing; otherwise rho is clipped to [1e-6, 1e6] and rho per row and the preconditioner are rebuilt at once (one
 * all-reduce); rho_updates is not reset. */
int  osqp_amd_rp_update_lin_cost(osqp_amd_rp *rp, const double *q);
int  osqp_amd_rp_update_bounds(osqp_amd_rp *rp, const double *l_loc, const double *u_loc);
int  osqp_amd_rp_warm_start(osqp_amd_rp *rp, const double *x, const double *y_loc);
int  osqp_amd_rp_update_rho(osqp_amd_rp *rp, double rho);

/* ---- for the tests ---- */
/* One array of the handle's state, in the scaled space the loop iterates in: synchronises the engine's stream, copies the
 * array to out[0, count) and returns count, or a negative HIPENG_ERR_* code (cap < count, unknown `which`).  Nothing is
 * written on the device.  x, x~, minv, b, r: n doubles (r: the last PCG residual); z, y, rho per row: m_loc doubles;
 * S: the PCG's device-side record as nine doubles: rz[0] rz[1] rr tol2 bb done iters cap bad.
 * SC15: the fifteen scalars of the last termination check as the device left them; SC7: the seven of the last check with the
 * infeasibility tests on (the first three as the all-reduces left them); DESIGN.md section 7 has the table of the twenty-two slots.
 * DX, DY: dx (n) and the projected dy (m_loc) of that check (after an infeasible status: the certificates).
 * Q, L, U: the scaled q (n) and bounds (m_loc) the loop reads, as osqp_amd_rp_update_lin_cost / _bounds left them. */
enum { OSQP_AMD_RP_PEEK_X = 0, OSQP_AMD_RP_PEEK_XT, OSQP_AMD_RP_PEEK_Z, OSQP_AMD_RP_PEEK_Y, OSQP_AMD_RP_PEEK_RHO_VEC, OSQP_AMD_RP_PEEK_MINV,
       OSQP_AMD_RP_PEEK_B, OSQP_AMD_RP_PEEK_R, OSQP_AMD_RP_PEEK_SC15, OSQP_AMD_RP_PEEK_S,
       OSQP_AMD_RP_PEEK_DX, OSQP_AMD_RP_PEEK_DY, OSQP_AMD_RP_PEEK_SC7, OSQP_AMD_RP_PEEK_Q, OSQP_AMD_RP_PEEK_L, OSQP_AMD_RP_PEEK_U };
int  osqp_amd_rp_peek(osqp_amd_rp *rp, int which, double *out, long long cap);
/* The host's decision at a termination check on given scalars (no handle, no device): sc22 = the fifteen + the seven;
 * unscaled: the _u forms decide (scaled data without scaled_termination); eps4 = eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
 * approximate: 10 x each.  Returns the verdict as rowpart_native.h names it: RP_GO_ON = 0, RP_RESIDUALS_PASS = 1, RP_PRIMAL_INF = 3,
 * RP_DUAL_INF = 4.  A test whose tolerance is 0 reads none of its scalars. */
int  osqp_amd_rp_test_verdict(const double *sc22, int unscaled, double c, int m_total, const double *eps4,
                              double pri_res, double dua_res, int approximate);

#ifdef __cplusplus
}
#endif
#endif
