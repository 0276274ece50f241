/*
 * osqp_amd_batch.h -- C ABI of the batched engine: many independent QPs that
 * share one sparsity pattern (MPC-style, BASELINE config 4), one workgroup per
 * QP on the GPU.  The reference has no batch API: semantically every QP of the
 * batch goes through what osqp_setup + osqp_solve (src/osqp.c:76-654) do for a
 * single problem, with the same settings struct; results are per-QP
 * OSQPInfo-like records.  Plain pointers and sizes only.
 */
#ifndef OSQP_AMD_BATCH_H
#define OSQP_AMD_BATCH_H

#include "osqp_amd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osqp_amd_batch osqp_amd_batch;

/* P (upper triangle) and A give the shared CSC pattern (and the shared values
 * when Px_all / Ax_all are NULL).  Px_all [batch][nnzP] / Ax_all [batch][nnzA]
 * optionally give per-QP values.  Q [batch][n], L, U [batch][m] row-major.
 * Returns 0 or an osqp_error_type code (include/constants.h:42-50 numbering):
 * OSQP_NONCVX_ERROR when some member's K = P + sigma I + A' rho A is not positive definite
 * (stderr names the first such member), OSQP_SETTINGS_VALIDATION_ERROR for settings->polish != 0
 * (polish is a call on a solved handle: osqp_amd_batch_polish) or time_limit > 0 (still refused at setup: a time
 * limit is given per call, osqp_amd_batch_solve_limited). */
c_int osqp_amd_batch_setup(osqp_amd_batch **out, c_int batch, const csc *P, const csc *A,
                           const c_float *Px_all, const c_float *Ax_all,
                           const c_float *Q, const c_float *L, const c_float *U,
                           const OSQPSettings *settings, c_int device);
/* Engines of a batch handle.  TILED: the engine of osqp_amd_batch_setup (n <= 128, K^-1 in registers, the
 * pattern, values and vectors of a member in LDS).  STREAMED: 1 <= n <= 1024, any m as long as the member's
 * vectors fit 160 KiB of LDS; K^-1 of every member lives in HBM (B x NP x NP doubles, NP = n rounded up to
 * 32) and is streamed once per ADMM iteration. */
#define OSQP_AMD_BATCH_TILED    0
#define OSQP_AMD_BATCH_STREAMED 1
/* osqp_amd_batch_setup with a choice of engine; TILED is osqp_amd_batch_setup itself.  Same return codes:
 * OSQP_SETTINGS_VALIDATION_ERROR for polish / time_limit > 0 (or an unknown engine), OSQP_LINSYS_SOLVER_INIT_ERROR
 * with a stderr line naming the limit when the shape does not fit, OSQP_NONCVX_ERROR naming the first
 * non-convex member, OSQP_MEM_ALLOC_ERROR when the device arrays cannot be allocated. */
c_int osqp_amd_batch_setup_engine(osqp_amd_batch **out, c_int engine, c_int batch, const csc *P, const csc *A,
                                  const c_float *Px_all, const c_float *Ax_all,
                                  const c_float *Q, const c_float *L, const c_float *U,
                                  const OSQPSettings *settings, c_int device);
/* The common-K engine: one model, many right-hand sides.  Every member shares P and A (there are no per-member
 * matrix values: that is the point of this entry), so the batch has ONE K^-1, and the B linear solves of an ADMM
 * iteration are one product K^-1 R (NP x B) on the matrix cores instead of B streamed GEMVs.  osqp_amd_batch_shape
 * reports OSQP_AMD_BATCH_COMMON for such a handle; osqp_amd_batch_setup_engine does not take the id (it keeps
 * returning OSQP_SETTINGS_VALIDATION_ERROR for it).
 * A member is what osqp_setup + osqp_solve make of its own problem (P, Q[b], A, L[b], U[b]), with three things held
 * in common:
 *  1. Scaling.  D, E and c are what the reference's scale_data gives for (P, q^, A) with q^_j = max_b |Q[b][j]|.
 *     They are computed once at setup and kept across osqp_amd_batch_update, as the reference keeps its scaling
 *     across osqp_update_lin_cost.  scaling = 0: the identity.  For one member, or identical members, this is the
 *     reference's own scaling to the bit (Ruiz sees norms only).
 *  2. Row classes.  Every row has one class (loose, inequality or equality: src/auxil.c:76-98, on the scaled
 *     bounds) in every member; setup returns OSQP_DATA_VALIDATION_ERROR otherwise and stderr names the first
 *     (member, row).  osqp_amd_batch_update (and _update_dev) with bounds after which the members would no longer
 *     agree returns 1, names member and row and writes nothing; bounds that move a row to the same new class in
 *     every member are accepted, and K is re-formed and re-inverted before the next solve.  L > U: 1, as ever.
 *  3. rho.  One rho for the batch.  adaptive_rho = 0: it never moves.  adaptive_rho = 1: at the multiples of
 *     adaptive_rho_interval (0: the deterministic stand-in of the other engines) every member still running forms
 *     the reference's compute_rho_estimate from its own residuals; the host takes, in member order, that value
 *     itself when all running members agree and exp(mean(log .)) otherwise, clips it to [1e-6, 1e6] and adopts it
 *     under the reference's adaptive_rho_tolerance rule.  On adoption the one K is re-formed and re-inverted and
 *     rho_updates of every running member goes up by one; a finished member keeps the rho, count and estimate it
 *     finished with.  For one member, or identical members, this is the reference's adaptation exactly.
 *     osqp_amd_batch_update_rho takes a scalar only: per_member = 1 returns 1 and changes nothing.
 * Everything else is per member as in the other engines: the iteration, update_info, check_termination with both
 * infeasibility tests and certificates, scaled_termination, check_termination = 0, max_iter, store_solution, warm
 * start from the kept scaled iterates.  A finished member is frozen: later iterations change nothing of it.
 * The explicit-inverse solve is probed in the first iterations after each inversion (refine_tol) as in the streamed
 * engine, with one verdict for the batch: osqp_amd_batch_rounds reports rounds = 1 + inversions during the solve
 * and refined = batch or 0.  Solves carry no floating-point atomics and are reproducible to the bit; a member's
 * bits do not depend on its position in the batch or on the batch's size as long as rho is fixed.
 * Limits, each OSQP_LINSYS_SOLVER_INIT_ERROR with a stderr line naming the limit: 1 <= n <= 1024; a member's vectors
 * fit 160 KiB of LDS (the streamed engine's limit).  polish / time_limit > 0: OSQP_SETTINGS_VALIDATION_ERROR.
 * OSQP_NONCVX_ERROR when K is not positive definite.
 * Served: _update, _warm_start, _update_rho, _solve, _solve_members, _common_columns, _get, _device_ptrs, _shape,
 * _rounds, _cleanup, _update_dev, _warm_start_dev, _get_dev, _check_dev_ptr, _member (the common D, E, c, rho,
 * classes, Pv, Av and the one K^-1, NP x NP, for any qp).  Served once osqp_amd_batch_common_kkt(b, 1) has built the
 * shared KKT pieces, and refused without them: _polish, _polish_status_dev, _adjoint*, _tangent*, _kkt_info.  Never
 * served: _update_matrices(_dev) (its per-member value flags contradict the engine; new values of the one model go
 * through osqp_amd_batch_common_update_model below).
 * A refused call returns OSQP_LINSYS_SOLVER_INIT_ERROR with a stderr line naming the engine and leaves the handle
 * untouched and usable. */
#define OSQP_AMD_BATCH_COMMON 2   /* what osqp_amd_batch_shape reports for such a handle; setup_engine does not take it */
c_int osqp_amd_batch_setup_common(osqp_amd_batch **out, c_int batch, const csc *P, const csc *A,
                                  const c_float *Q, const c_float *L, const c_float *U,
                                  const OSQPSettings *settings, c_int device);
/* New values for the shared model of a live common-K handle: osqp_update_P / _A / _P_A (src/osqp.c:1012-1279) applied
 * to the one model.  One value array [k] serves the batch.  Px / Ax NULL = keep.  Px_idx / Ax_idx NULL: all nnzP / nnzA
 * values in CSC order of triu(P) / A; otherwise P_n / A_n values for the listed slots.
 * The equilibration is recomputed from scratch on the new raw values and q^_j = max_b |Q[b][j]| over the raw Q the
 * handle holds now (as last given by setup or _update) -- the scale_data of setup -- and every member's scaled q, l, u
 * are rewritten from its stored raw ones with the new D, E, c.  The row classes stay as stored (the reference does not
 * re-run set_rho_vec in a matrix update), so the call has no class-clash outcome; a later _update with bounds classifies
 * under the new E as ever.  rho stays the adapted value of the last solve.  The scaled iterates x, z, y of every member
 * stay; rho_updates of every member is reset; the handle counts as unsolved and a kept KKT inversion is dropped.  K is
 * re-formed and re-inverted inside the call and the refinement verdict is taken again.  Where the handle carries the
 * shared KKT pieces, H and Wt are rebuilt from the new scaled values.
 * Returns, in this order and with nothing written: OSQP_WORKSPACE_NOT_INIT_ERROR for NULL;
 * OSQP_LINSYS_SOLVER_INIT_ERROR (stderr names osqp_amd_batch_update_matrices) for a handle of another engine; 1 when
 * P_n > nnzP; 2 when A_n > nnzA; OSQP_DATA_VALIDATION_ERROR for a negative count or an index outside [0, nnz); 0 when
 * both Px and Ax are NULL (nothing changes).  After the values are written: OSQP_NONCVX_ERROR when a pivot of the new K
 * is not positive -- the handle stays alive, osqp_amd_batch_solve returns OSQP_NONCVX_ERROR until a later call of this
 * function succeeds, and H and Wt are rebuilt by that call; OSQP_NONCVX_ERROR, with the stderr line of
 * osqp_amd_batch_common_kkt, when K passes but a pivot of P~ + delta I does not -- the shared pieces are freed, the
 * handle is a common-K handle without them and solves are served; OSQP_MEM_ALLOC_ERROR; -102 when a HIP call fails. */
c_int osqp_amd_batch_common_update_model(osqp_amd_batch *b,
                                         const c_float *Px, const c_int *Px_idx, c_int P_n,
                                         const c_float *Ax, const c_int *Ax_idx, c_int A_n);
/* Polish, adjoint and tangent of a common-K handle, on a shared Hessian inverse.  The (1,1) block of the regularised
 * KKT matrix [P~ + delta I, Ar'; Ar, -delta I] (P~, A~: the handle's scaled values) is the same for every member
 * until osqp_amd_batch_common_update_model brings new values, so the calls below eliminate it once: H = (P~ + delta I)^-1, Wt = A~ H, and per member only
 * S = Ar H Ar' + delta I of order mred is formed and inverted; t = H g1, nu = S^-1 (Ar t - g2), x = t - Wt[rows]' nu
 * is the same regularised solve, followed by the same polish_refine_iter refinement steps against [P, Ar'; Ar, 0].
 * on = 1: build (once; a second call is a no-op returning 0) the shared KKT pieces of a common-K handle -- H = (P~ + delta I)^-1,
 * NP x NP, and Wt = A~ H, m x NP -- with delta as given at setup; from then on osqp_amd_batch_polish, _polish_status_dev,
 * _adjoint, _adjoint_multi, _tangent, their _dev twins and _kkt_info are served on the handle, with the semantics, statuses and
 * return codes written below for the other engines.  on = 0: free them; the calls are refused again as before.
 * Returns 0; OSQP_LINSYS_SOLVER_INIT_ERROR (stderr line) for a handle of another engine; OSQP_NONCVX_ERROR when a pivot of
 * P~ + delta I is not positive (nothing is kept, the handle stays usable for solves); OSQP_MEM_ALLOC_ERROR likewise;
 * OSQP_WORKSPACE_NOT_INIT_ERROR for NULL; -102 when a HIP call fails: nothing is kept
 * then either.  Solves, updates and warm starts neither read nor invalidate H and Wt.
 * On such a handle the KKT buffer holds NS x NS doubles per member, NS = the largest number of active rows in the batch
 * rounded up to 32 (at least 32); osqp_amd_batch_kkt_info reports out[0] = passes of formation and inversion of the
 * members' S (H does not count), out[2] = NS, out[3] = the members kept.  The limits n + active rows <= 2176 and
 * 160 KiB of LDS hold as for the other engines.  Either switch drops a kept inversion. */
c_int osqp_amd_batch_common_kkt(osqp_amd_batch *b, c_int on);
/* For the tests: H [NP*NP], Wt [m*NP] (NULL = skip), and of member qp of the inversion currently kept (osqp_amd_batch_kkt_info
 * out[1] = 1): mred, NS and Sinv [NS*NS] as stored (each NULL = skip).  OSQP_WORKSPACE_NOT_INIT_ERROR for NULL, for a
 * handle without the pieces, and when nothing is kept and something of a member is asked for;
 * OSQP_DATA_VALIDATION_ERROR for a qp outside the batch or one whose last solve did not end OSQP_SOLVED; -102 when a
 * HIP call fails. */
c_int osqp_amd_batch_common_kkt_peek(osqp_amd_batch *b, c_float *H, c_float *Wt, c_int qp, c_int *mred, c_int *NS, c_float *Sinv);
/* The engine of a handle and the padded order NP of its K^-1 (the Kinv buffer of osqp_amd_batch_member is
 * NP x NP).  NULL = skip. */
c_int osqp_amd_batch_shape(osqp_amd_batch *b, c_int *engine, c_int *NP);
/* Of the last solve: rounds = launches of the ADMM loop (streamed engine: 1 + rounds that resumed members after
 * a K^-1 rebuild; tiled engine: 1), refined = members whose K^-1 solve takes the refinement step.  NULL = skip. */
c_int osqp_amd_batch_rounds(osqp_amd_batch *b, c_int *rounds, c_int *refined);
/* osqp_update_lin_cost / osqp_update_bounds for every QP (NULL = keep). */
c_int osqp_amd_batch_update(osqp_amd_batch *b, const c_float *Q, const c_float *L, const c_float *U);
/* osqp_update_P / osqp_update_A / osqp_update_P_A (src/osqp.c:1012-1279) for every QP: new values, same pattern.
 * Px / Ax NULL = keep.  Px_idx / Ax_idx NULL: all nnzP / nnzA values in CSC order of triu(P) / A; otherwise P_n /
 * A_n values for the listed slots (one index list for the batch: it belongs to the pattern).  *_per_member = 0: one
 * value array [k] for every member; 1: [batch][k] row-major.  A handle set up with shared values that receives
 * per-member values switches to per-member storage (one allocation, kept); a shared update of a per-member handle
 * writes every member.  Per member as the reference: the equilibration is recomputed from scratch on the new raw
 * data (q, l, u as last given) and K is re-formed and re-inverted with the member's current rho (the adapted value of
 * the last solve) and its current row classes; the scaled iterates stay as they are; rho_updates is reset.
 * Returns, before anything is written: 1 when P_n > nnzP, 2 when A_n > nnzA (the reference's codes),
 * OSQP_DATA_VALIDATION_ERROR for an index outside [0, nnz).  OSQP_NONCVX_ERROR when some member's new K has a
 * non-positive pivot (stderr names the first such member): the values are written, the handle stays alive,
 * osqp_amd_batch_solve returns OSQP_NONCVX_ERROR until a later osqp_amd_batch_update_matrices succeeds. */
c_int osqp_amd_batch_update_matrices(osqp_amd_batch *b,
                                     const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                     const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member);
/* osqp_update_rho (src/osqp.c:1281-1332) for every QP: rho points at one value (per_member = 0) or at [batch].  Any
 * value <= 0: returns 1 and changes nothing.  Each member's rho becomes min(max(rho, 1e-6), 1e6) and its K^-1 is
 * rebuilt at the start of the next solve; rho_updates is not reset. */
c_int osqp_amd_batch_update_rho(osqp_amd_batch *b, const c_float *rho, c_int per_member);
/* osqp_warm_start / _x / _y (src/osqp.c:942-1010) for every QP: X [batch][n], Y [batch][m], unscaled, either may
 * be NULL.  x = D^-1 x and z = A x (when X is given), y = c E^-1 y (when Y is given), on the device; turns
 * settings->warm_start on for the handle, as the reference does. */
c_int osqp_amd_batch_warm_start(osqp_amd_batch *b, const c_float *X, const c_float *Y);
/* osqp_solve for every QP; iterates persist on the device between calls
 * (warm start, settings->warm_start). */
c_int osqp_amd_batch_solve(osqp_amd_batch *b);
/* osqp_solve for `count` chosen members of a common-K handle: members [count], strictly ascending, each in [0, batch).
 * Only the listed members are loaded, iterated, checked, counted in the rho estimate (in member order) and stored: the
 * columns of the solve are the listed members, so the GEMM and every other kernel shrink with the list.  Of a member
 * that is not listed nothing changes: X, Y, info8 (all eight, its rho and rho_updates among them), both certificates
 * and the stored scaled iterates keep their bits.  The listed members get the bits a handle set up on them alone would
 * give as long as the scaling and rho agree (rho fixed, or adapted from the same members).  Where rho is adopted it is
 * the batch's one rho from then on: K is re-formed and re-inverted as in a full solve and rho_updates of the running
 * listed members goes up.
 * The refinement verdict (osqp_amd_batch_rounds) is the batch's, but "off" binds only members that were probed under the
 * current K^-1: a call that lists a member no solve has probed since the last inversion probes through its first four
 * iterations, so solve_members(S) then solve_members(the rest) refines the rest exactly when a handle of their own
 * would.  The flags are kept per listed member, not per probed column: after a rho move in mid-solve the new window
 * counts for every member of that call's list, those that had finished before the move included -- what a full solve
 * has always done.  "On" stays through every later inversion (a rho move, osqp_amd_batch_update_rho, a class change in an
 * update); only osqp_amd_batch_common_update_model clears it.
 * It counts as a solve: a kept KKT inversion is dropped and a polish is forgotten.  The handle keeps one flag per member,
 * "solved on the current problem": every update and warm start that makes polish, adjoint and tangent return
 * OSQP_WORKSPACE_NOT_INIT_ERROR clears all of them, osqp_amd_batch_solve sets all, this call sets the listed ones, and
 * those calls are served once every member's flag is set -- after update, solve_members(S) they are refused, after
 * solve_members(the rest) they are served.
 * Returns, in this order and with nothing of the handle changed: OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle;
 * OSQP_LINSYS_SOLVER_INIT_ERROR, with a stderr line naming the call and the engine, for a tiled or streamed handle;
 * OSQP_DATA_VALIDATION_ERROR for NULL members, count < 1, count > batch, an index outside [0, batch) or a list that is
 * not strictly ascending; OSQP_NONCVX_ERROR as osqp_amd_batch_solve.  count == batch is osqp_amd_batch_solve, to the bit. */
c_int osqp_amd_batch_solve_members(osqp_amd_batch *b, const c_int *members, c_int count);
/* Of the last solve of a common-K handle (either call): out[0] = the columns it started with (batch, or count),
 * out[1] = packs, out[2] = the columns in use when it ended.  Whenever the members still running fit fewer groups of
 * 64 columns than the columns in use, the solve moves them to the front, in member order, and every kernel runs on
 * the shorter range from then on (a pack); results do not depend on it.  OSQP_AMD_BATCH_COMMON_PACK=0 in the
 * environment when the handle is set up switches packing off.  Touches no GPU memory.  OSQP_WORKSPACE_NOT_INIT_ERROR
 * for a NULL handle, OSQP_DATA_VALIDATION_ERROR for NULL out, OSQP_LINSYS_SOLVER_INIT_ERROR (stderr line) for a handle
 * of another engine. */
c_int osqp_amd_batch_common_columns(osqp_amd_batch *b, c_int out[3]);
/* osqp_amd_batch_solve / _solve_members with two limits that hold for this call only.
 * members NULL (count ignored): every member, on any engine.  members non-NULL: the checks, refusals and
 * semantics of osqp_amd_batch_solve_members (common-K only).
 * max_iter   0: settings->max_iter of setup;  > 0: the cap of this call.  The call leaves the results and the whole
 *            handle state that a handle set up with that max_iter leaves after a solve, to the bit; the next plain solve
 *            runs with the setup's value again.
 * time_limit 0: none;  > 0: seconds, counted from the start of the call's device work.  The clock is looked at only
 *            at clock iterations -- those of a termination check or, with check_termination == 0, every 25th -- and
 *            after that check: a member that passes it leaves as ever.  Every other member then ends as it ends at
 *            max_iter (which wins when both hold) -- the approximate test, then OSQP_TIME_LIMIT_REACHED -- with x, y,
 *            info8 and the stored iterates of its last iteration; polish, adjoint and tangent skip it (status 0).
 *            A member runs at most one clock interval of iterations past the deadline; with more members than the
 *            device runs workgroups at once, each later wave of workgroups adds that interval again.  On the tiled
 *            and streamed engines the deadline is a device word that one thread of each workgroup compares with
 *            wall_clock64(); the common-K engine, whose members move in lockstep, compares a host clock.
 * Refusals, in this order, with nothing of the handle changed: OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle;
 * OSQP_SETTINGS_VALIDATION_ERROR for max_iter < 0 (or beyond INT_MAX), time_limit < 0 or not finite; the refusals of
 * osqp_amd_batch_solve_members when members is given; OSQP_NONCVX_ERROR as osqp_amd_batch_solve.
 * (NULL, ., 0, 0) is osqp_amd_batch_solve to the bit, with the same launches. */
c_int osqp_amd_batch_solve_limited(osqp_amd_batch *b, const c_int *members, c_int count,
                                   c_int max_iter, c_float time_limit);
/* Of the last solve by any call: out[0] max_iter in force, out[1] time_limit in force (0 = none),
 * out[2] seconds between the two device stamps of a clocked solve (0 when time_limit was 0),
 * out[3] members that the clock cut.  Before the first solve: settings->max_iter, 0, 0, 0.  Touches no GPU memory.
 * OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle, OSQP_DATA_VALIDATION_ERROR for NULL out. */
c_int osqp_amd_batch_solve_report(osqp_amd_batch *b, c_float out[4]);
/* polish (src/polish.c:19-350) for every member whose last solve ended OSQP_SOLVED; the others are skipped.
 * Polish is this call on a solved handle, with settings->delta and settings->polish_refine_iter as given at setup;
 * settings->polish != 0 itself stays refused by the setup functions.  Per member, in its scaled space: the active
 * rows are guessed from the iterates of the solve, the dense regularised KKT matrix [P + delta I, Ar'; Ar, -delta I]
 * is inverted on the device, exactly polish_refine_iter refinement steps against the unregularised matrix follow,
 * and the reference's three-clause rule accepts or rejects the polished point.  An accepted member's X, Y,
 * info8[2..4] (obj_val, pri_res, dua_res) and stored iterates (the start of the next warm-started solve) are
 * overwritten; of a rejected or skipped member nothing changes.  rho, K^-1, row classes and rho_updates never change.
 * status_polish [batch] (NULL = skip): 1 accepted, -1 tried and rejected (a KKT pivot of the wrong sign included),
 * 0 not tried.  A second call without a solve in between does no work and reports the same values.
 * Memory: the KKT matrices are NPOL x NPOL doubles per member, NPOL = n + the largest number of active rows in the
 * batch, rounded up to 32, in one buffer separate from K^-1, allocated at the first call and freed by cleanup.  The
 * solved members go through it in chunks; the buffer never exceeds 8 GiB (or the number of bytes the environment
 * variable OSQP_AMD_BATCH_POLISH_CAP_BYTES held when the handle was set up; one member's matrix at the least).
 * Returns 0; OSQP_WORKSPACE_NOT_INIT_ERROR when no solve has run since setup or since the last update of data,
 * matrices or rho (or a warm start with arrays: the stored iterates are then not a solve's);
 * OSQP_MEM_ALLOC_ERROR when the buffer cannot be allocated (the handle stays usable);
 * OSQP_LINSYS_SOLVER_INIT_ERROR with a stderr line when n + active rows exceeds 2176, which only the tiled engine
 * with many rows can reach. */
c_int osqp_amd_batch_polish(osqp_amd_batch *b, c_int *status_polish);
/* Adjoint derivatives of the solution, for every member whose last solve ended OSQP_SOLVED: from dX = dl/dx
 * [batch][n] and dY = dl/dy [batch][m] (NULL = 0; only its active rows matter) of a scalar l, the gradients
 * dQ [batch][n], dL and dU [batch][m] and, where asked for, dPx [batch][nnzP] and dAx [batch][nnzA] on the pattern of
 * setup (CSC order of triu(P) / A; NULL = skip; an off-diagonal slot of triu(P) stands for both halves of P).  The
 * point differentiated is the one the handle holds: the polished one where osqp_amd_batch_polish was accepted,
 * the ADMM iterate otherwise.  Per member, in its scaled space: the active rows as polish guesses them (lows first,
 * then upps), the same regularised KKT matrix inverted on the device, one solve M [rx; rnu] = [dX; dY_active] with
 * exactly polish_refine_iter refinement steps against the unregularised M = [P, Ar'; Ar, 0], then dQ = -rx,
 * dL_i / dU_i = rnu at a row active at its lower / upper bound and 0 elsewhere, dA_ij = -(y_i rx_j + rnu_i x_j) on
 * active rows, dP_ii = -rx_i x_i, dP_ij = -(rx_i x_j + rx_j x_i).  Where active rows are linearly dependent the
 * multipliers are not unique and neither are dL, dU, dAx; where strict complementarity fails the solution is not
 * differentiable and the values are those of the guessed active set.
 * active [batch][m] (NULL = skip): -1 active at the lower bound, +1 at the upper, 0 inactive.  status_adjoint
 * [batch] (NULL = skip): 1 computed; -1 a KKT pivot of the wrong sign (that member's outputs are 0); 0 not tried, the
 * member's last solve did not end OSQP_SOLVED (outputs 0).  Nothing of the handle changes: X, Y, info8, the stored
 * iterates, rho, K^-1 and the status_polish a later osqp_amd_batch_polish reports stay bit-equal.
 * Memory: polish's KKT buffer with its cap and chunks, plus the one staging set of the derivative calls (this one,
 * osqp_amd_batch_adjoint_multi, osqp_amd_batch_tangent and their _dev twins share it: each returns with the handle's
 * stream synchronised, so nothing is queued on it between calls): inputs and outputs at the first call, room for
 * dPx / dAx at the first call that asks for them; it grows when a later call needs more and is freed by cleanup.
 * Returns as osqp_amd_batch_polish: 0; OSQP_WORKSPACE_NOT_INIT_ERROR when no solve has run on the current problem;
 * OSQP_MEM_ALLOC_ERROR (the handle stays usable); OSQP_LINSYS_SOLVER_INIT_ERROR with a stderr line when
 * n + active rows exceeds 2176 or the LDS does not fit; OSQP_DATA_VALIDATION_ERROR when dX, dQ (or, with m > 0,
 * dL, dU) is NULL. */
c_int osqp_amd_batch_adjoint(osqp_amd_batch *b, const c_float *dX, const c_float *dY /*NULL = 0*/,
                             c_float *dQ, c_float *dL, c_float *dU,
                             c_float *dPx /*[batch][nnzP], NULL = skip*/, c_float *dAx /*[batch][nnzA], NULL = skip*/,
                             c_int *active /*[batch][m], NULL = skip*/, c_int *status_adjoint /*[batch]*/);
/* osqp_amd_batch_adjoint for ncot cotangents per member in one call -- ncot rows of the Jacobian, where one call of
 * osqp_amd_batch_adjoint gives one: dX [batch][ncot][n] and dY [batch][ncot][m] (NULL = 0) in, dQ [batch][ncot][n], dL
 * and dU [batch][ncot][m] and, where asked for, dPx [batch][ncot][nnzP] and dAx [batch][ncot][nnzA] out.  Cotangent d of
 * a member gets exactly what osqp_amd_batch_adjoint gives for (dX[.][d], dY[.][d]), to the bit: the same point, the same
 * scaled-space solve with exactly polish_refine_iter refinement steps, the same formulas, zeros for members whose status
 * is not 1, and nothing of the handle's solve state written.  The ncot cotangents of a member share one formation and
 * one inversion of its KKT matrix; a cotangent's bits depend neither on ncot, nor on the other cotangents, nor on the
 * chunking.  active [batch][m] and status_adjoint [batch] (NULL = skip) are per member, as osqp_amd_batch_adjoint
 * reports them.
 * Memory: as osqp_amd_batch_adjoint, of which this is the general form (that call is ncot = 1): the same staging set,
 * which grows when a later call brings a larger ncot and is freed by cleanup.
 * Returns as osqp_amd_batch_adjoint, plus OSQP_DATA_VALIDATION_ERROR when ncot < 1 or ncot > 65535. */
c_int osqp_amd_batch_adjoint_multi(osqp_amd_batch *b, c_int ncot,
                                   const c_float *dX /*[batch][ncot][n]*/, const c_float *dY /*[batch][ncot][m], NULL = 0*/,
                                   c_float *dQ /*[batch][ncot][n]*/, c_float *dL, c_float *dU /*[batch][ncot][m]*/,
                                   c_float *dPx /*[batch][ncot][nnzP], NULL = skip*/, c_float *dAx /*[batch][ncot][nnzA], NULL = skip*/,
                                   c_int *active /*[batch][m], NULL = skip*/, c_int *status_adjoint /*[batch], NULL = skip*/);
/* One KKT inversion per solve.  osqp_amd_batch_adjoint, _adjoint_multi, _tangent and their _dev twins all need the
 * active rows and the inverted KKT matrix of every solved member at the point the handle holds.  When all of them fit
 * the KKT buffer at once (one chunk under OSQP_AMD_BATCH_POLISH_CAP_BYTES), the first such call after a solve keeps what
 * it built -- with the pivot verdicts -- and the later ones run only their own kernel, with the same results and
 * statuses to the bit.  The kept inversion is dropped by osqp_amd_batch_solve, by every update and warm start that
 * withdraws the permission to call, by an osqp_amd_batch_polish that does work (polish neither reads nor leaves one; a
 * repeated polish that finds the work done drops nothing), by a regrowth of the KKT buffer and by cleanup.  With more
 * than one chunk nothing is kept.  OSQP_AMD_BATCH_KKT_CACHE=0 in the environment at setup switches the sharing off.
 * osqp_amd_batch_kkt_info, for the tests and tools: out[0] builds since setup (one pass of formation and inversion over
 * the solved members; polish's passes included), out[1] 1 when an inversion is currently kept, out[2] its padded order
 * NPOL, out[3] the members in it (0, 0 when none is kept).  Touches no GPU memory.  Returns 0,
 * OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle, OSQP_DATA_VALIDATION_ERROR for a NULL out. */
c_int osqp_amd_batch_kkt_info(osqp_amd_batch *b, c_int out[4]);
/* Forward sensitivities of the solution, for every member whose last solve ended OSQP_SOLVED: from ndir tangents per
 * member of the data -- dQ [batch][ndir][n], dL and dU [batch][ndir][m], dPx [batch][ndir][nnzP] and dAx
 * [batch][ndir][nnzA] on the pattern of setup (CSC order of triu(P) / A; an off-diagonal slot of triu(P) stands for
 * both halves of P); any of them NULL = 0 -- the tangents dX [batch][ndir][n] and dY [batch][ndir][m] (NULL = skip)
 * of the solution: one column of the Jacobian per direction, where osqp_amd_batch_adjoint gives one row per call.
 * The point differentiated is the one the handle holds: the polished one where osqp_amd_batch_polish was accepted,
 * the ADMM iterate otherwise.  Per member, in its scaled space: the active rows as polish guesses them (lows first,
 * then upps), the same regularised KKT matrix inverted on the device once for all ndir directions, and per direction
 * one solve M [dx; dnu] = [-(dQ + dP x + dA' y_act); db_act - (dA x)_act] with exactly polish_refine_iter refinement
 * steps against the unregularised M = [P, Ar'; Ar, 0]; dY = dnu on the active rows and 0 elsewhere.  y_act is y on
 * the active rows and 0 elsewhere; db is dL_i on a row active at its lower bound and dU_i on one active at its upper
 * bound.  The tangent of the other bound of a row, of an inactive row and of an infinite bound has no effect.  An
 * equality row (l = u) follows the one bound it is classified active at, by the sign of its multiplier: give dL = dU
 * there.  Where active rows are linearly dependent the multipliers are not unique and neither is dY (and a tangent
 * that moves dependent rows apart has no solution: the values are those of the regularised solve); where strict
 * complementarity fails the solution is not differentiable and the values are those of the guessed active set.
 * For a loss with gradients gx, gy and the adjoint's outputs for them, gx.dX + gy.dY = dQ_adj.dQ + dL_adj.dL +
 * dU_adj.dU + dPx_adj.dPx + dAx_adj.dAx.  The results carry no atomics and are reproducible to the bit; a
 * direction's bits do not depend on the other directions of the call.
 * active [batch][m] (NULL = skip): as osqp_amd_batch_adjoint reports it.  status_tangent [batch] (NULL = skip): 1
 * computed; -1 a KKT pivot of the wrong sign (that member's outputs are 0); 0 not tried, the member's last solve did
 * not end OSQP_SOLVED (outputs 0).  Nothing of the handle changes: X, Y, info8, the stored iterates, rho, K^-1, the
 * status_polish a later osqp_amd_batch_polish reports and what a later osqp_amd_batch_adjoint returns stay bit-equal.
 * Memory: polish's KKT buffer with its cap and chunks, plus the staging set it shares with osqp_amd_batch_adjoint:
 * room for the tangents that are passed (host route) and for the outputs; it grows when a later call brings a larger
 * ndir and is freed by cleanup.
 * Returns 0; OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle or when no solve has run on the current problem;
 * OSQP_DATA_VALIDATION_ERROR when ndir < 1, ndir > 65535 or dX is NULL; OSQP_MEM_ALLOC_ERROR (the handle stays
 * usable); OSQP_LINSYS_SOLVER_INIT_ERROR with a stderr line when n + active rows exceeds 2176 or the kernel would
 * need more than 160 KiB of LDS. */
c_int osqp_amd_batch_tangent(osqp_amd_batch *b, c_int ndir,
                             const c_float *dQ /*[batch][ndir][n]*/, const c_float *dL, const c_float *dU /*[batch][ndir][m]*/,
                             const c_float *dPx /*[batch][ndir][nnzP]*/, const c_float *dAx /*[batch][ndir][nnzA]*/,
                             c_float *dX /*[batch][ndir][n]*/, c_float *dY /*[batch][ndir][m], NULL = skip*/,
                             c_int *active /*[batch][m], NULL = skip*/, c_int *status_tangent /*[batch], NULL = skip*/);
/* Results: X [batch][n], Y [batch][m] (unscaled; OSQP_NAN when infeasible),
 * info8 [batch][8] = {iter, status_val, obj_val, pri_res, dua_res, rho_updates,
 * rho_estimate, rho}; DX / DY infeasibility certificates.  NULL = skip. */
c_int osqp_amd_batch_get(osqp_amd_batch *b, c_float *X, c_float *Y, c_float *info8,
                         c_float *DX, c_float *DY);
/* The verdict on a point against the RAW problem the handle holds now (osqp_amd/csrc/batch_verify.h): the values on the
 * setup pattern (shared, per member, or the common-K engine's one model), q, l, u as setup read them and every update
 * has rewritten them.  It reads nothing of the scaling, rho, K^-1 or the stored iterates, needs no solve and writes
 * nothing of the handle; all three engines serve it.  The point is X [batch][n], Y [batch][m], unscaled, the
 * certificates DX [batch][n], DY [batch][m]; NULL = the handle's own (what osqp_amd_batch_get returns).  P is the full
 * symmetric matrix of the stored triangle.  With ax = A x, z = clamp(ax, l, u), px = P x, aty = A'y, yp = max(y, 0),
 * ym = max(-y, 0), V [batch][16] receives per member
 *    0 obj = x'px / 2 + q'x         1 pri_res = |ax - z|oo         2 dua_res = |px + q + aty|oo
 *    3 |ax|oo    4 |z|oo    5 |px|oo    6 |aty|oo    7 |q|oo
 *    8 eps_pri = eps_abs + eps_rel max(3, 4)         9 eps_dua = eps_abs + eps_rel max(5, 6, 7)
 *   10 comp = max_i max(yp_i (u_i - z_i), ym_i (z_i - l_i))
 *   11 dual_obj = -x'px / 2 - sum_i (u_i yp_i - l_i ym_i)          12 gap = obj - dual_obj
 *   13 optimal   1.0 when pri_res < eps_pri and dua_res < eps_dua (strict), else 0.0
 *   14 prim_inf  the reference's is_primal_infeasible on DY, 15 dual_inf its is_dual_infeasible on DX, with identity
 *                scaling on the raw data and the handle's eps_prim_inf / eps_dual_inf, its inequalities as coded.
 * eps_abs, eps_rel: of this call; a negative value means the handle's setting.
 * A bound is infinite as in the reference without scaling: u > 1e26, l < -1e26 (OSQP_INFTY * MIN_SCALING).  In 10 and 11
 * a term whose multiplier part (yp_i, ym_i) is 0 counts 0; a nonzero multiplier part on an infinite bound makes 10
 * +OSQP_INFTY, 11 -OSQP_INFTY and 12 +OSQP_INFTY.
 * "NaN" is an IEEE NaN or the number OSQP_NAN, which the handle stores in X and Y of a member without a solution.  One
 * in a member's x or y: slots 0-12 are OSQP_NAN and 13 is 0.0, 14 and 15 are computed all the same.  One in its dy (dx):
 * 14 (15) is 0.0.
 * A member's record is reproducible to the bit and does not depend on the batch around it or on the form of the call.
 * Refusals, in this order, with nothing written: OSQP_WORKSPACE_NOT_INIT_ERROR for a NULL handle; in the _members forms
 * the list's (OSQP_DATA_VALIDATION_ERROR); OSQP_DATA_VALIDATION_ERROR for a NULL V, a non-finite eps_abs or eps_rel and,
 * in the _dev forms, a non-NULL pointer that is not device memory of the handle's device; -102 for a HIP failure. */
c_int osqp_amd_batch_verify(osqp_amd_batch *b, const c_float *X, const c_float *Y, const c_float *DX, const c_float *DY,
                            c_float eps_abs, c_float eps_rel, c_float *V /*[batch][16]*/);
/* Device pointers of the result arrays, for device-side gathers (RCCL). */
c_int osqp_amd_batch_device_ptrs(osqp_amd_batch *b, void **X, void **Y, void **info8);
void  osqp_amd_batch_cleanup(osqp_amd_batch *b);

/* ---- Device arrays in and out -------------------------------------------------------------------------------
 * The calls below are the calls above with DEVICE pointers in place of host pointers: a caller whose data lives in
 * HBM (a torch CUDA tensor, an array of its own hipMalloc) updates, warm-starts and reads a handle without a host
 * copy of any [batch][.] array.  Each has the semantics and the return codes of its twin (the same name without
 * _dev), runs the twin's kernels on the same workspace and leaves the handle in the state the twin would.
 * Pointers: every non-NULL device pointer must be device memory (hipMalloc and the like, not managed and not
 * registered host memory) of the handle's device, known to the HIP runtime this library runs on.  Each is classified
 * on the host (hipPointerGetAttributes) before any copy or launch; a pointer that does not pass -- a host pointer,
 * another device's memory, an allocation of a second HIP runtime mapped into the process -- makes the call return
 * OSQP_DATA_VALIDATION_ERROR with nothing written.  The sizes are the caller's promise, as for host pointers.
 * Ordering: the work runs on the handle's own stream.  The caller's inputs must be complete when the call is made
 * (synchronise the stream that produced them first); every _dev call returns with the handle's stream synchronised,
 * so its outputs are ready on return for any stream.  No stream or event handle crosses this interface. */

/* osqp_amd_batch_update from device arrays (NULL = keep).  The bounds are clamped to +-OSQP_INFTY on the device.
 * Returns 1 when L and U are both given and some L[k] > U[k] after the clamp; the raw q, l, u of the handle, its
 * scaled workspace, flags and info8 are then exactly as before the call. */
c_int osqp_amd_batch_update_dev(osqp_amd_batch *b, const c_float *Q, const c_float *L, const c_float *U);
/* osqp_amd_batch_update_matrices with the value arrays Px / Ax on the device.  The index lists Px_idx / Ax_idx stay
 * HOST pointers (they belong to the pattern) and are validated before anything is written, with the twin's codes in
 * the twin's order: 1, 2, OSQP_DATA_VALIDATION_ERROR; then the device pointers. */
c_int osqp_amd_batch_update_matrices_dev(osqp_amd_batch *b,
                                         const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                         const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member);
/* osqp_amd_batch_common_update_model with the value arrays Px / Ax on the device; the index lists stay HOST pointers.
 * The twin's refusals in the twin's order, then OSQP_DATA_VALIDATION_ERROR for a pointer that is not device memory of
 * the handle's device, then 0 for both NULL. */
c_int osqp_amd_batch_common_update_model_dev(osqp_amd_batch *b,
                                             const c_float *Px, const c_int *Px_idx, c_int P_n,
                                             const c_float *Ax, const c_int *Ax_idx, c_int A_n);
/* osqp_amd_batch_warm_start from device arrays X [batch][n], Y [batch][m] (either may be NULL). */
c_int osqp_amd_batch_warm_start_dev(osqp_amd_batch *b, const c_float *X, const c_float *Y);
/* osqp_amd_batch_adjoint with every array on the device.  active [batch][m] and status_adjoint [batch] are 32-bit
 * ints there (int, not c_int), as the kernel writes them. */
c_int osqp_amd_batch_adjoint_dev(osqp_amd_batch *b, const c_float *dX, const c_float *dY /*NULL = 0*/,
                                 c_float *dQ, c_float *dL, c_float *dU,
                                 c_float *dPx /*NULL = skip*/, c_float *dAx /*NULL = skip*/,
                                 int *active /*NULL = skip*/, int *status_adjoint /*NULL = skip*/);
/* osqp_amd_batch_adjoint_multi with every array on the device: the cotangents are read in place, the outputs arrive by
 * device-to-device copies.  active [batch][m] and status_adjoint [batch] are 32-bit ints there.  Every non-NULL pointer
 * is classified before any copy or launch, after the checks of ncot and of the NULL arguments. */
c_int osqp_amd_batch_adjoint_multi_dev(osqp_amd_batch *b, c_int ncot, const c_float *dX, const c_float *dY /*NULL = 0*/,
                                       c_float *dQ, c_float *dL, c_float *dU,
                                       c_float *dPx /*NULL = skip*/, c_float *dAx /*NULL = skip*/,
                                       int *active /*NULL = skip*/, int *status_adjoint /*NULL = skip*/);
/* osqp_amd_batch_tangent with every array on the device: the tangents are read in place, the outputs arrive by
 * device-to-device copies.  active [batch][m] and status_tangent [batch] are 32-bit ints there, as the kernel writes
 * them. */
c_int osqp_amd_batch_tangent_dev(osqp_amd_batch *b, c_int ndir,
                                 const c_float *dQ, const c_float *dL, const c_float *dU,
                                 const c_float *dPx, const c_float *dAx, c_float *dX, c_float *dY /*NULL = skip*/,
                                 int *active /*NULL = skip*/, int *status_tangent /*NULL = skip*/);
/* osqp_amd_batch_get into caller-owned device arrays (NULL = skip): copies, which a later solve does not touch
 * (the arrays of osqp_amd_batch_device_ptrs are the handle's own and change with the next solve). */
c_int osqp_amd_batch_get_dev(osqp_amd_batch *b, c_float *X, c_float *Y, c_float *info8, c_float *DX, c_float *DY);
/* osqp_amd_batch_verify with every array on the device: the given X, Y, DX, DY are read in place, V [batch][16] arrives
 * by a device-to-device copy.  The records carry the bits of the host form. */
c_int osqp_amd_batch_verify_dev(osqp_amd_batch *b, const c_float *X, const c_float *Y, const c_float *DX,
                                const c_float *DY, c_float eps_abs, c_float eps_rel, c_float *V /*[batch][16]*/);
/* status_polish [batch] (32-bit ints on the device) as osqp_amd_batch_polish reports it; all 0 when polish has not
 * run since the last solve.  Runs no polish.  OSQP_WORKSPACE_NOT_INIT_ERROR as osqp_amd_batch_polish: no solve has
 * run on the current problem. */
c_int osqp_amd_batch_polish_status_dev(osqp_amd_batch *b, int *status_polish);
/* For the tests: the pointer check of the _dev calls alone.  0 when p passes, OSQP_DATA_VALIDATION_ERROR otherwise
 * (NULL included).  Asks the runtime about the address; reads and writes no GPU memory. */
c_int osqp_amd_batch_check_dev_ptr(osqp_amd_batch *b, const void *p);

/* ---- Chosen members: the calls around the solve -----------------------------------------------------------------
 * Each call below is the twin named in its comment "for the listed members": `members [count]`, a HOST list (in the
 * _dev forms too: it belongs to the call, not to the data), strictly ascending, every index in [0, batch) -- the checks
 * of osqp_amd_batch_solve_members -- in front of the twin's arguments, and every per-member array COMPACT: [count][.],
 * row k belongs to member members[k].  All three engines serve them (osqp_amd_batch_update_matrices_members: the tiled and
 * the streamed engine, as its twin).  Of a member that is not listed nothing changes:
 * its raw and scaled q, l, u, its row classes and flags, X, Y, info8, both certificates, the stored iterates, its solved
 * flag and its status_polish keep their bits.  count == batch is the whole-batch twin to the bit, in every output and
 * in every piece of handle state: it runs the twin's own code.
 * Refusals come first, in this order, with nothing written:
 *   1. OSQP_WORKSPACE_NOT_INIT_ERROR   handle is NULL;
 *   2. OSQP_DATA_VALIDATION_ERROR      the list: NULL, count < 1, count > batch, an index out of range, not strictly
 *                                      ascending;
 *   3. the twin's own refusals, in the twin's order (a common-K handle without its shared KKT pieces refuses the polish,
 *      adjoint and tangent forms with OSQP_LINSYS_SOLVER_INIT_ERROR and the twin's line on stderr, naming the call).
 * The handle keeps one solved flag and one polished flag per member.  A member's solved flag is set by a solve that
 * lists it (or a whole solve) and cleared by every update or warm start that touches it; its polished flag is set when
 * polish has run on it, by either polish call, and cleared with the solved flag and by the member's next solve. */

/* osqp_amd_batch_update for the listed members: Q [count][n], L, U [count][m] (NULL = keep).  The raw rows of the listed
 * members are replaced, scaled with the stored D, E, c and re-classified; a class change requests the member's K^-1
 * again; rho_updates of the listed members restarts.  Clears the solved flag of the listed members only and drops a kept
 * KKT inversion.  Returns 1, with nothing of the handle changed, when some listed row has L > U (_dev: after the clamp
 * to +-OSQP_INFTY) or, on a common-K handle with count < batch, when a listed member's new bounds would give a row
 * another class than the handle holds for it (stderr names member and row): the unlisted members keep that class. */
c_int osqp_amd_batch_update_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                    const c_float *Q, const c_float *L, const c_float *U);
c_int osqp_amd_batch_update_members_dev(osqp_amd_batch *b, const c_int *members, c_int count,
                                        const c_float *Q, const c_float *L, const c_float *U);
/* osqp_amd_batch_warm_start for the listed members: X [count][n], Y [count][m], unscaled (NULL = keep).  Turns the
 * warm_start setting on; with arrays it rewrites the listed members' scaled x, z = A x and y, clears their solved flags
 * and drops a kept KKT inversion.  Both NULL: 0 after the argument checks, no GPU work. */
c_int osqp_amd_batch_warm_start_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                        const c_float *X, const c_float *Y);
c_int osqp_amd_batch_warm_start_members_dev(osqp_amd_batch *b, const c_int *members, c_int count,
                                            const c_float *X, const c_float *Y);
/* osqp_amd_batch_update_matrices for the listed members.  *_per_member = 0: one value array [k], written to every listed
 * member; 1: COMPACT [count][k], row r for member members[r].  The index lists belong to the pattern, as in the twin.  A
 * handle that holds shared raw values switches to per-member storage on the first such call with count < batch, whatever
 * *_per_member says; the unlisted members' rows then hold the values that were shared.  A listed member gets what the twin
 * does to a member: the new raw values, the equilibration from scratch on its raw data (q, l, u as last given), K re-formed
 * and re-inverted inside the call with its current rho and row classes, the scaled iterates kept, rho_updates reset, the
 * refinement verdict taken again; its solved and polished flags are cleared and a kept KKT inversion is dropped.  Its bits
 * are those of the twin given [batch][k] arrays.  Of an unlisted member nothing changes: not its scaling (the twin would
 * recompute it from the q it holds now), not its rho_updates, K^-1, flags or results.
 * Refusals after the list's, with nothing written: OSQP_LINSYS_SOLVER_INIT_ERROR on a common-K handle (the twin's line on
 * stderr, naming this call), then the twin's in the twin's order -- 1 for P_n > nnzP, 2 for A_n > nnzA,
 * OSQP_DATA_VALIDATION_ERROR for an index outside [0, nnz), in the _dev form for a value pointer that is not device memory
 * of the handle's device -- and 0 for both NULL.
 * OSQP_NONCVX_ERROR exactly when, after the values are written, SOME member of the batch has a K with a non-positive pivot,
 * listed or not (stderr names the first such member): a call that repairs other members while a bad one stays bad still
 * returns it, and osqp_amd_batch_solve refuses until a matrix update returns 0.  So 0 means solves are served.  The handle
 * keeps the verdict per member, and only a matrix update that lists the member (or a whole-batch one) takes it again:
 * osqp_amd_batch_update, _update_rho and _warm_start, in any form, leave it. */
c_int osqp_amd_batch_update_matrices_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                             const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                             const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member);
/* ... with the value arrays Px / Ax on the device; the index lists and members stay HOST lists. */
c_int osqp_amd_batch_update_matrices_members_dev(osqp_amd_batch *b, const c_int *members, c_int count,
                                                 const c_float *Px, const c_int *Px_idx, c_int P_n, c_int Px_per_member,
                                                 const c_float *Ax, const c_int *Ax_idx, c_int A_n, c_int Ax_per_member);
/* osqp_amd_batch_update_rho for the listed members: rho points at one value (per_member = 0) or at COMPACT [count].  Each
 * listed member's rho becomes min(max(rho, 1e-6), 1e6) and its K^-1 is rebuilt at the start of the next solve;
 * rho_updates is not reset; its solved and polished flags are cleared and a kept KKT inversion is dropped.  The unlisted
 * members keep every bit.  OSQP_DATA_VALIDATION_ERROR for a NULL rho; any value <= 0: returns 1 and changes nothing; on a
 * common-K handle (one rho for the batch) count < batch returns 1 with a line on stderr and changes nothing. */
c_int osqp_amd_batch_update_rho_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                        const c_float *rho, c_int per_member);
/* osqp_amd_batch_polish for the listed members; status_polish [count].  Needs every LISTED member solved on the current
 * problem (OSQP_WORKSPACE_NOT_INIT_ERROR otherwise, nothing changed).  The work is done for the listed members whose
 * polished flag is unset, with the padded orders of their largest active set; a repeat does no work and reports the
 * same values.  A call that does work drops a kept KKT inversion.  osqp_amd_batch_polish keeps its own rule: it works
 * once per solve on every member, whatever the member calls have done, and sets every member's polished flag. */
c_int osqp_amd_batch_polish_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int *status_polish);
/* osqp_amd_batch_adjoint_multi for the listed members: ncot >= 1 cotangents per member, dX [count][ncot][n], dY
 * [count][ncot][m] (NULL = 0), dQ, dL, dU, dPx, dAx [count][ncot][.], active [count][m], status_adjoint [count].  Needs
 * every listed member solved on the current problem.  Plan, buffer cap, chunks, statuses and the zero outputs of members
 * whose solve did not end OSQP_SOLVED are the twin's; the bits of a listed member are those of the whole-batch call on
 * the same state.  A one-chunk build is kept together with its list: a later _members call on the same solve reuses it
 * exactly when its list is identical, a whole-batch call reuses only a whole-batch build (osqp_amd_batch_kkt_info:
 * out[3] = the members kept). */
c_int osqp_amd_batch_adjoint_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                     const c_float *dX, const c_float *dY /*NULL = 0*/,
                                     c_float *dQ, c_float *dL, c_float *dU, c_float *dPx /*NULL = skip*/,
                                     c_float *dAx /*NULL = skip*/, c_int *active /*NULL = skip*/, c_int *status_adjoint);
c_int osqp_amd_batch_adjoint_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ncot,
                                         const c_float *dX, const c_float *dY, c_float *dQ, c_float *dL, c_float *dU,
                                         c_float *dPx, c_float *dAx, int *active, int *status_adjoint);
/* osqp_amd_batch_tangent for the listed members: tangents [count][ndir][.] in, dX [count][ndir][n], dY [count][ndir][m],
 * active [count][m], status_tangent [count] out; precondition and kept inversion as osqp_amd_batch_adjoint_members. */
c_int osqp_amd_batch_tangent_members(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                     const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                     const c_float *dAx, c_float *dX, c_float *dY /*NULL = skip*/,
                                     c_int *active /*NULL = skip*/, c_int *status_tangent);
c_int osqp_amd_batch_tangent_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_int ndir,
                                         const c_float *dQ, const c_float *dL, const c_float *dU, const c_float *dPx,
                                         const c_float *dAx, c_float *dX, c_float *dY, int *active, int *status_tangent);
/* osqp_amd_batch_get for the listed members: a gather of their rows into X, DX [count][n], Y, DY [count][m], info8
 * [count][8] (NULL = skip).  The _dev form writes caller-owned device arrays, exactly count rows of each. */
c_int osqp_amd_batch_get_members(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                 c_float *info8, c_float *DX, c_float *DY);
c_int osqp_amd_batch_get_members_dev(osqp_amd_batch *b, const c_int *members, c_int count, c_float *X, c_float *Y,
                                     c_float *info8, c_float *DX, c_float *DY);
/* osqp_amd_batch_verify for the listed members: X, DX [count][n], Y, DY [count][m] (NULL = the handle's own rows of the
 * listed members), V [count][16].  A listed member's record carries the bits of the whole-batch call on the same point. */
c_int osqp_amd_batch_verify_members(osqp_amd_batch *b, const c_int *members, c_int count,
                                    const c_float *X, const c_float *Y, const c_float *DX, const c_float *DY,
                                    c_float eps_abs, c_float eps_rel, c_float *V /*[count][16]*/);
c_int osqp_amd_batch_verify_members_dev(osqp_amd_batch *b, const c_int *members, c_int count,
                                        const c_float *X, const c_float *Y, const c_float *DX, const c_float *DY,
                                        c_float eps_abs, c_float eps_rel, c_float *V /*[count][16]*/);
/* out [batch]: 1 where the member's results are those of a solve of the problem the handle holds now (what the polish,
 * adjoint and tangent forms above require of the members they list), 0 otherwise.  OSQP_DATA_VALIDATION_ERROR for a
 * NULL out.  Touches no GPU memory. */
c_int osqp_amd_batch_solved_members(osqp_amd_batch *b, c_int *out);

/* For the tests: member qp's workspace as the last setup / update / solve left it.  NULL = skip.
 * D [n], E [m], c [1], rho [1] (current scalar rho), ctype [m] (-1 free, 0 ineq, 1 eq),
 * Pv [nnzP], Av [nnzA] (scaled values, CSC order), Kinv [NP*NP] row-major, *NP = 64 or 128
 * (K^-1 of the kernel, padded with identity rows and columns; un-permuted from the kernel's
 * GEMV order with the kernel's own index function).  Streamed engine: *NP = n rounded up to 32
 * (osqp_amd_batch_shape), K^-1 as stored.  Returns 0 or an osqp_error_type code. */
c_int osqp_amd_batch_member(osqp_amd_batch *b, c_int qp, c_float *D, c_float *E, c_float *c, c_float *rho,
                            c_int *ctype, c_float *Pv, c_float *Av, c_float *Kinv, c_int *NP);

#ifdef __cplusplus
}
#endif
#endif
