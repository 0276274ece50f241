/*
 * osqp_amd.h -- public C API of libosqp_amd.so, the MI355X-native drop-in for
 * the reference's osqp_setup / osqp_solve / osqp_update_* path.
 *
 * Same names, argument meaning, return codes and struct layouts as the
 * reference's include/osqp.h (cited per function, paths relative to
 * /root/reference).  The ADMM loop, the KKT solve (indirect: Jacobi-PCG on the
 * reduced system) and every residual reduction run on the GPU; there is no CPU
 * fallback -- without a HIP device osqp_setup fails with
 * OSQP_LINSYS_SOLVER_LOAD_ERROR and says why on stderr.
 */
#ifndef OSQP_AMD_H
#define OSQP_AMD_H

#include "osqp_amd_types.h"
#include "osqp_amd_helpers.h"   /* cs.h / lin_alg.h / kkt.h helper symbols, allocator hook */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- main API (include/osqp.h:32-96; src/osqp.c:24-757) ------------------ */
void  osqp_set_default_settings(OSQPSettings *settings);
c_int osqp_setup(OSQPWorkspace **workp, const OSQPData *data, const OSQPSettings *settings);
c_int osqp_solve(OSQPWorkspace *work);
c_int osqp_cleanup(OSQPWorkspace *work);

/* ---- data updates (include/osqp.h:108-258; src/osqp.c:765-1332) ---------- */
c_int osqp_update_lin_cost(OSQPWorkspace *work, const c_float *q_new);
c_int osqp_update_bounds(OSQPWorkspace *work, const c_float *l_new, const c_float *u_new);
c_int osqp_update_lower_bound(OSQPWorkspace *work, const c_float *l_new);
c_int osqp_update_upper_bound(OSQPWorkspace *work, const c_float *u_new);
c_int osqp_warm_start(OSQPWorkspace *work, const c_float *x, const c_float *y);
c_int osqp_warm_start_x(OSQPWorkspace *work, const c_float *x);
c_int osqp_warm_start_y(OSQPWorkspace *work, const c_float *y);
c_int osqp_update_P(OSQPWorkspace *work, const c_float *Px_new, const c_int *Px_new_idx, c_int P_new_n);
c_int osqp_update_A(OSQPWorkspace *work, const c_float *Ax_new, const c_int *Ax_new_idx, c_int A_new_n);
c_int osqp_update_P_A(OSQPWorkspace *work, const c_float *Px_new, const c_int *Px_new_idx, c_int P_new_n,
                      const c_float *Ax_new, const c_int *Ax_new_idx, c_int A_new_n);
c_int osqp_update_rho(OSQPWorkspace *work, c_float rho_new);

/* ---- settings setters (include/osqp.h:270-421; src/osqp.c:1339-1617) ----- */
c_int osqp_update_max_iter(OSQPWorkspace *work, c_int max_iter_new);
c_int osqp_update_eps_abs(OSQPWorkspace *work, c_float eps_abs_new);
c_int osqp_update_eps_rel(OSQPWorkspace *work, c_float eps_rel_new);
c_int osqp_update_eps_prim_inf(OSQPWorkspace *work, c_float eps_prim_inf_new);
c_int osqp_update_eps_dual_inf(OSQPWorkspace *work, c_float eps_dual_inf_new);
c_int osqp_update_alpha(OSQPWorkspace *work, c_float alpha_new);
c_int osqp_update_warm_start(OSQPWorkspace *work, c_int warm_start_new);
c_int osqp_update_scaled_termination(OSQPWorkspace *work, c_int scaled_termination_new);
c_int osqp_update_check_termination(OSQPWorkspace *work, c_int check_termination_new);
c_int osqp_update_delta(OSQPWorkspace *work, c_float delta_new);
c_int osqp_update_polish(OSQPWorkspace *work, c_int polish_new);
c_int osqp_update_polish_refine_iter(OSQPWorkspace *work, c_int polish_refine_iter_new);
c_int osqp_update_verbose(OSQPWorkspace *work, c_int verbose_new);
c_int osqp_update_time_limit(OSQPWorkspace *work, c_float time_limit_new);

/* ---- helpers callers of the reference use (include/auxil.h; the cs.h / lin_alg.h / kkt.h
 *      ones are declared in osqp_amd_helpers.h) ------------------------------------------ */
void  cold_start(OSQPWorkspace *work);                                           /* auxil.h:62 */

/* ---- linear-system plugin boundary (include/lin_sys.h:20-45) -------------
 * Constructor of the HIP PCG plugin, in the shape of
 * init_linsys_solver_qdldl (lin_sys/direct/qdldl/qdldl_interface.h:89).  The
 * returned object starts with the reference's vtable prefix
 * (include/types.h:298-319). */
c_int init_linsys_solver_hip_pcg(LinSysSolver **sp, const csc *P, const csc *A,
                                 c_float sigma, const c_float *rho_vec, c_int polish);
c_int load_linsys_solver(enum linsys_solver_type linsys_solver);      /* lin_sys.c:15 */
c_int unload_linsys_solver(enum linsys_solver_type linsys_solver);    /* lin_sys.c:35 */
c_int init_linsys_solver(LinSysSolver **s, const csc *P, const csc *A, c_float sigma,
                         const c_float *rho_vec, enum linsys_solver_type linsys_solver,
                         c_int polish);                                /* lin_sys.c:56 */

/* ---- side channel for knobs OSQPSettings has no room for ------------------
 * (OSQPSettings is ABI; SURVEY.md section 5 "config / flags").  Process-wide
 * defaults picked up by the next osqp_setup / init_linsys_solver_hip_pcg;
 * also settable through the environment:
 *   OSQP_AMD_PCG_EPS_REL (default 1e-9), OSQP_AMD_PCG_EPS_ABS (1e-15),
 *   OSQP_AMD_PCG_MAX_ITER (0 = max(20000, 10n): see DESIGN.md), OSQP_AMD_DEVICE (0). */
typedef struct {
  c_float pcg_eps_rel;
  c_float pcg_eps_abs;
  c_int   pcg_max_iter;
  c_int   device;
  c_int   pcg_adaptive;   /* 1: inexact solves, PCG tolerance tied to the ADMM residuals (not parity-exact; OSQP_AMD_PCG_ADAPTIVE) */
} osqp_amd_options;
void  osqp_amd_get_options(osqp_amd_options *opt);
void  osqp_amd_set_options(const osqp_amd_options *opt);
/* Statistics of the device engine behind a workspace (PCG iteration counts,
 * graph launches); returns nonzero if the workspace has no engine. */
typedef struct {
  c_int pcg_iters_total;
  c_int pcg_iters_last;
  c_int pcg_forced;
  c_int graph_launches;
  c_int host_syncs;
  c_int resident;        /* 1: the linear solves run as one resident launch each (K in registers, engine_pcg_resident.h k_pcg_resident);
                            0: launch-per-step PCG kernels (problem too large for the register files, OSQP_AMD_RESIDENT=0,
                            or a resident launch found the GPU shared and the engine fell back) */
} osqp_amd_stats;
c_int osqp_amd_get_stats(const OSQPWorkspace *work, osqp_amd_stats *st);
/* Derivatives of the solution at the point the workspace holds (the polished one where settings->polish ran and was accepted,
 * the ADMM iterate otherwise), for one QP what osqp_amd_batch_adjoint / osqp_amd_batch_tangent (osqp_amd_batch.h) are for a batch
 * member, in the CSC order of triu(P) / A as given to osqp_setup.  With the active rows (polish's two tests on the scaled z, y,
 * l, u; lows first, then upps), Ar those rows of A and M = [P, Ar'; Ar, 0]:
 *   adjoint  M [rx; rnu] = [dx; dy_act]:  dq = -rx, dl_i (du_i) = rnu at a row active at its lower (upper) bound,
 *            dA_ij = -(y_i rx_j + rnu_i x_j) on active rows, dP_ij = -(rx_i x_j + rx_j x_i) (an off-diagonal slot of triu(P) stands
 *            for both halves; -rx_i x_i on the diagonal);
 *   tangent  M [dx; dnu] = [-(dq + dP x + dA' y_act); db_act - (dA x)_act], dy = dnu on the active rows, ndir directions that share
 *            the KKT instance (dl = du is expected on an equality row; the tangent of the bound a row is active at is used).
 * The solve is polish's, in the scaled space with D, E, c as constants: d' = max(delta, 1e-3), at least polish_refine_iter
 * refinement steps, at most max(polish_refine_iter, 15), the same stop rule.  kkt_res is the last |g - M s|_inf / max(|g|_inf, 1)
 * of that space, reported and not judged.  active: -1 / +1 / 0 per row.
 * status: 1 computed; -1 a linear solve failed (negative curvature, a HIP error, a non-finite value), outputs 0; 0 not tried
 * (info->status_val != OSQP_SOLVED), outputs 0.
 * Return 0, OSQP_WORKSPACE_NOT_INIT_ERROR (NULL workspace; no osqp_solve since setup, since the last osqp_update_* of data,
 * matrices or rho, or since an osqp_warm_start*), OSQP_DATA_VALIDATION_ERROR (NULL dx / dq / status, NULL dl / du with m > 0,
 * ndir < 1 or ndir > OSQP_AMD_MAX_NDIR = 65535: the directions of a call are one dimension of one kernel launch).
 * The first call after a solve builds the KKT instance (Ared and a polish-mode plugin instance); it is kept until the next
 * osqp_solve, update, warm start or osqp_cleanup, so a backward pass, a forward pass and all directions share it (it is built with
 * the delta of that moment: osqp_update_delta drops it, and the next call builds one with the new value; polish_refine_iter is read
 * by every call).  Nothing of the
 * workspace changes: x, y, z, solution, info, the engine's iterates, rho and statistics stay bit-equal. */
#define OSQP_AMD_MAX_NDIR 65535
c_int osqp_amd_adjoint(OSQPWorkspace *work, const c_float *dx /*[n]*/, const c_float *dy /*[m], NULL = 0*/,
                       c_float *dq, c_float *dl, c_float *du,
                       c_float *dPx /*[nnzP], NULL = skip*/, c_float *dAx /*[nnzA], NULL = skip*/,
                       c_int *active /*[m], NULL = skip*/, c_int *status, c_float *kkt_res /*NULL = skip*/);
c_int osqp_amd_tangent(OSQPWorkspace *work, c_int ndir,
                       const c_float *dq /*[ndir][n]*/, const c_float *dl, const c_float *du /*[ndir][m]*/,
                       const c_float *dPx /*[ndir][nnzP]*/, const c_float *dAx /*[ndir][nnzA]*/,   /* any NULL = 0 */
                       c_float *dx /*[ndir][n]*/, c_float *dy /*[ndir][m], NULL = skip*/,
                       c_int *active, c_int *status, c_float *kkt_res /*[ndir], NULL = skip*/);
/* for the tests: out[0] KKT instances built since setup, [1] one is alive, [2] its active rows, [3] linear solves since setup */
c_int osqp_amd_sens_info(OSQPWorkspace *work, c_int out[4]);
/* for the tests: the KKT instance of the last polish, recorded before polish freed it.  out[0] polish instances run since setup,
 * [1] the linear-solve form the last one took (hipeng_resident_info [9]; -1: none yet, or it could not be read), [2] its active
 * rows, [3] its resident launches that gave up plus its negative-curvature stops (0: the form served every solve; -1 unread) */
c_int osqp_amd_polish_info(OSQPWorkspace *work, c_int out[4]);
/* The verdict on a point against the RAW problem the workspace holds now, computed on the device from P, q, A, l, u as the caller gave
 * and last updated them and from the unscaled point alone -- nothing of D, E, c, rho, the linear-solve form or the engine's iterates:
 * for one QP what osqp_amd_batch_verify (osqp_amd_batch.h) is for a batch member.  V receives the same 16 slots with the same
 * definitions:
 *    0 obj = x'Px / 2 + q'x      1 pri_res = |Ax - z|oo, z = clamp(Ax, l, u)      2 dua_res = |Px + q + A'y|oo
 *    3 |Ax|oo   4 |z|oo   5 |Px|oo   6 |A'y|oo   7 |q|oo     8 eps_pri = eps_abs + eps_rel max(3, 4)
 *    9 eps_dua = eps_abs + eps_rel max(5, 6, 7)      10 comp = max_i max(y+_i (u_i - z_i), y-_i (z_i - l_i))
 *   11 dual_obj = -x'Px / 2 - sum_i (u_i y+_i - l_i y-_i)      12 gap = obj - dual_obj
 *   13 optimal: 1 < 8 and 2 < 9      14 prim_inf: is_primal_infeasible on dy      15 dual_inf: is_dual_infeasible on dx
 * (13-15 are 1.0 or 0.0; the two tests are auxil.c:361-512 with D = E = I, c = 1 and settings->eps_prim_inf / eps_dual_inf).  A bound
 * with |bound| > 1e26 is infinite: a term of 10 or 11 whose multiplier part is 0 counts 0, a nonzero multiplier part on an infinite
 * bound makes 10 +OSQP_INFTY, 11 -OSQP_INFTY, 12 +OSQP_INFTY.  "NaN" is an IEEE NaN or the number OSQP_NAN: one in x or y makes 0-12
 * OSQP_NAN and 13 0, one in dy / dx makes 14 / 15 0.
 * x, dx [n], y, dy [m]: unscaled host arrays; NULL = the workspace's own at the moment of the call -- work->solution->x,
 * work->solution->y, work->delta_x, work->delta_y.  eps_abs, eps_rel: negative = settings->eps_abs / eps_rel.  Needs no solve; m = 0 is
 * served; returns with the engine's stream synchronised.
 * Returns, in this order and with nothing done: OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL workspace or one without an engine;
 * OSQP_DATA_VALIDATION_ERROR for a NULL V or a non-finite eps_abs / eps_rel; OSQP_MEM_ALLOC_ERROR when the host or the device has no room
 * for the call's arrays (the workspace stays usable); -102 when a HIP call fails.
 * The first call builds the device side (patterns, copies of the raw values); each osqp_update_lin_cost, _bounds, _lower_bound,
 * _upper_bound, _P, _A, _P_A marks what it changes and the next call copies those parts again, nothing else.  osqp_update_rho, the warm
 * starts and the osqp_update_<setting> calls mark nothing; a workspace that never calls this allocates and launches nothing for it.
 * Nothing of the workspace changes: x, y, z, solution, info, the engine's iterates, rho, the statistics and a live KKT instance of the
 * derivatives keep their bits.  A record is reproducible to the bit: it depends on the pattern, the values and the point, not on the
 * linear-solve form, the device or earlier calls. */
c_int osqp_amd_verify(OSQPWorkspace *work, const c_float *x, const c_float *y, const c_float *dx, const c_float *dy,
                      c_float eps_abs, c_float eps_rel, c_float V[16]);
/* for the tests: out[0] osqp_amd_verify calls served since setup, [1] uploads of P values, [2] of A values, [3] of q / l / u (one
 * counter, each vector counts one).  OSQP_WORKSPACE_NOT_INIT_ERROR / OSQP_DATA_VALIDATION_ERROR as above (NULL out). */
c_int osqp_amd_verify_info(OSQPWorkspace *work, c_int out[4]);
/* The options above are the DEFAULTS a new workspace / plugin instance copies at creation; afterwards
 * each instance has its own (no knob is shared between live workspaces).  These two read / change the
 * copy of one workspace (the device cannot be changed after setup). */
c_int osqp_amd_get_workspace_options(const OSQPWorkspace *work, osqp_amd_options *opt);
c_int osqp_amd_set_workspace_options(OSQPWorkspace *work, const osqp_amd_options *opt);
/* Binary problem files: one little-endian file per QP (layout in osqp_host.c); the data the
 * reference's generators emit as C headers (tests/utils/codegen_utils.py:172-347).
 * Return 0, or 1 bad argument / 2 cannot open / 3 malformed / 4 out of memory. */
c_int osqp_amd_write_problem(const char *path, const OSQPData *data);
c_int osqp_amd_read_problem(const char *path, OSQPData **data);
void  osqp_amd_free_problem(OSQPData *data);
/* Raw engine handle of a workspace (for the kernel-level tests / bench). */
void *osqp_amd_engine(const OSQPWorkspace *work);
/* ... and of the live KKT instance of the solution derivatives (NULL: none alive).  The instance chooses its linear-solve form
 * from (P, Ared) on its own: hipeng_resident_info / hipeng_pcg_layout / hipeng_elim_count on this handle say which. */
void *osqp_amd_sens_engine(const OSQPWorkspace *work);

#ifdef __cplusplus
}
#endif
#endif
