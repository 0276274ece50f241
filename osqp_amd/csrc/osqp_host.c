/*
 * osqp_host.c -- host side (plain C) of the MI355X-native OSQP drop-in.
 *
 * Implements the reference's public API (include/osqp.h) on top of the HIP
 * engine's C-ABI shim (include/osqp_amd_engine.h).  What stays on the host is
 * what the reference does once per setup / per termination check on scalars:
 * validation (src/auxil.c:791-1065), Ruiz equilibration at setup and on matrix
 * updates (src/scaling.c:44-175), constraint classification for rho
 * (src/auxil.c:76-142), the status decision of check_termination on the
 * device-reduced scalars (src/auxil.c:681-786), rho adaptation
 * (src/auxil.c:13-74) and bookkeeping.  Every per-iteration vector operation,
 * SpMV and reduction runs on the GPU; nothing here falls back to CPU numerics
 * for the hot path.
 *
 * The solve loop runs the device in windows that end at the next event the
 * reference would act on (termination check, rho adaptation, print, max_iter),
 * so info->iter and the iterate trajectory are the reference's.
 * Documented deviations:
 *   - adaptive_rho_interval == 0 uses the reference's non-PROFILING rule
 *     (osqp.c:267-279) instead of wall-clock (osqp.c:453-485), SURVEY.md F5;
 *   - time_limit and the window cap are polled between windows (<= 8 iterations
 *     when a time limit is set), not every iteration (osqp.c:387-407);
 *   - no SIGINT handler is installed.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <time.h>
#include "../../include/osqp_amd.h"
#include "../../include/osqp_amd_engine.h"
#include "../../include/osqp_amd_helpers.h"

#define HMAX(a, b) (((a) > (b)) ? (a) : (b))
#define HMIN(a, b) (((a) < (b)) ? (a) : (b))
#define BOUND_INF (OSQP_INFTY * MIN_SCALING)
#define POLISH_DELTA_MIN  1e-3   /* regularisation of the polish solves (see run_polish) */
#define POLISH_MAX_REFINE 15     /* refinement steps at most (the reference's polish_refine_iter at least) */

struct OSQP_TIMER { double t0; };

static double now_s(void) {
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
static void tic(OSQPTimer *t) { t->t0 = now_s(); }
static double toc(const OSQPTimer *t) { return now_s() - t->t0; }

/* ------------------------------------------------------------------------ */
/* engine options (side channel, see include/osqp_amd.h).  g_opt is only the  */
/* template new solver objects are initialised from (environment + the last   */
/* osqp_amd_set_options); every workspace / plugin instance carries its own   */
/* copy, so two workspaces never read each other's knobs after setup.         */
/* ------------------------------------------------------------------------ */
static osqp_amd_options g_opt;
static int g_opt_init = 0;
/* OSQP_AMD_PCG_EPS_FACTOR: experiment knob for tools/pcg_tol_sweep.py -- the 1e-5 of osqp_solve's PCG stop.  Read with the others, kept
 * beside them: osqp_amd_options is ABI and does not grow. */
static double g_pcg_eps_factor = 1e-5;

static void opt_init(void) {
  if (g_opt_init) return;
  const char *s;
  g_opt.pcg_eps_rel = 1e-9; g_opt.pcg_eps_abs = 1e-15; g_opt.pcg_max_iter = 0; g_opt.device = 0;
  g_opt.pcg_adaptive = 0;
  if ((s = getenv("OSQP_AMD_PCG_ADAPTIVE"))) g_opt.pcg_adaptive = atoll(s);
  if ((s = getenv("OSQP_AMD_PCG_EPS_REL")))  g_opt.pcg_eps_rel = atof(s);
  if ((s = getenv("OSQP_AMD_PCG_EPS_ABS")))  g_opt.pcg_eps_abs = atof(s);
  if ((s = getenv("OSQP_AMD_PCG_MAX_ITER"))) g_opt.pcg_max_iter = atoll(s);
  if ((s = getenv("OSQP_AMD_DEVICE")))       g_opt.device = atoll(s);
  else if ((s = getenv("LOCAL_RANK")))       g_opt.device = atoll(s);   /* one process per GPU */
  if ((s = getenv("OSQP_AMD_PCG_EPS_FACTOR")) && atof(s) > 0) g_pcg_eps_factor = atof(s);
  g_opt_init = 1;
}
void osqp_amd_get_options(osqp_amd_options *o) { opt_init(); *o = g_opt; }
void osqp_amd_set_options(const osqp_amd_options *o) { opt_init(); g_opt = *o; }

static void fill_params(hipeng_params *p, const osqp_amd_options *o, c_float sigma, c_float alpha, c_int n) {
  p->sigma = sigma; p->alpha = alpha;
  /* solves outside an ADMM loop (LinSysSolver.solve, the convexity probe, polish) have no eps_abs/eps_rel to relate to:
   * 1e-10 unless the option asks for less; osqp_solve sets its own stop from the option and the tolerances */
  p->pcg_eps_rel = HMIN(o->pcg_eps_rel, 1e-10); p->pcg_eps_abs = o->pcg_eps_abs;
  /* the cap is for pathological systems only: in the 120-case random sweep (tools/stress.py) max(1000, 2n) cut 10 ill-conditioned small QPs short
   * (pcg_forced), 20000 none, at the same run time */
  p->pcg_max_iter = o->pcg_max_iter > 0 ? o->pcg_max_iter : HMAX(20000, 10 * n);
  p->no_restart = 0;
}

/* ------------------------------------------------------------------------ */
/* the plugin object (vtable prefix + private part)                           */
/* ------------------------------------------------------------------------ */
/* Solution derivatives (osqp_amd_adjoint / osqp_amd_tangent): one polish-mode KKT instance per solved problem, built by the first
 * call after a solve and dropped by the next solve, update or warm start; the device side (hipsens) and the host buffers stay
 * until cleanup.  Allocated by the first call: a workspace that never asks has none of it. */
typedef struct {
  LinSysSolver *ls;       /* the instance: [P + d I, Ared'; Ared, -d I] (NULL: none alive) */
  csc *Ared;
  OSQPPolish pol;         /* its active rows (row maps of its own; polish's stay polish's) */
  hipsens *dev;           /* O(nnz) kernels and their device arrays (csrc/kkt_sens.h) */
  c_int dev_device;       /* ... and the device they live on: the instance's */
  c_int built, solves;    /* instances built / linear solves since setup */
  c_int *act;             /* [m] -1 / +1 / 0 */
  c_float *yact, *rnu;    /* [m] y on the active rows, 0 elsewhere; rnu scattered to the rows */
  c_float *rhs, *sol, *res, *tmp;   /* [n + m] */
} sens_state;

typedef struct {
  enum linsys_solver_type type;
  c_int (*solve)(LinSysSolver *self, c_float *b);
  void  (*free)(LinSysSolver *self);
  c_int (*update_matrices)(LinSysSolver *self, const csc *P, const csc *A);
  c_int (*update_rho_vec)(LinSysSolver *self, const c_float *rho_vec);
  c_int nthreads;
  /* private */
  hipeng *eng;            /* device engine (owned)                                */
  hipeng *aux;            /* workspace view only: lazily created solve() engine   */
  OSQPWorkspace *owner;   /* non-NULL when this is a workspace's solver           */
  c_int n, m, polish;
  c_float sigma;
  c_float *rho_tmp;       /* polish: constant 1/delta vector                      */
  csc *rawP, *rawA;       /* workspace view: unscaled problem as last given by the caller */
  c_float *rawq, *rawl, *rawu;
  hipeng_scalars sc;      /* last residual scalars                                */
  c_int sc_iter;          /* iteration they belong to (-1 = stale)                */
  hipeng_scalars early;   /* scalars that came back with a window's own wait (hipeng_run_admm_check) */
  c_int early_iter;       /* iteration they belong to (-1 = none): refresh_info takes them once */
  c_int host_syncs;
  c_int forced_warned;    /* the pcg_forced warning has been printed for this workspace */
  osqp_amd_options opt;   /* this instance's engine options (copied from the defaults at creation) */
  sens_state *sens;       /* workspace view: solution derivatives (NULL until the first call) */
  c_int sens_ready;       /* an osqp_solve has completed and no data, rho or iterate was changed since */
  c_int pol_info[4];      /* workspace view: run_polish's last instance, as osqp_amd_polish_info reports it */
  hipver *ver;            /* workspace view: the device side of osqp_amd_verify (csrc/verify.h; NULL until the first call) */
  c_int ver_stale;        /* VER_P .. VER_U: parts of the raw problem changed since that side copied them (ver_mark) */
  c_int ver_calls;        /* osqp_amd_verify calls served */
} hip_pcg_solver;

#define PCG(work) ((hip_pcg_solver *)((work)->linsys_solver))

/* the parts of the raw problem osqp_amd_verify keeps on the device (the bits of hipver_upload) and their one writer */
enum { VER_P = 1, VER_A = 2, VER_Q = 4, VER_L = 8, VER_U = 16, VER_ALL = 31 };
static void ver_mark(OSQPWorkspace *w, c_int parts) { PCG(w)->ver_stale |= parts; }

static c_int pcg_solve(LinSysSolver *self, c_float *b) {
  hip_pcg_solver *s = (hip_pcg_solver *)self;
  hipeng *e = s->eng;
  if (s->owner) {   /* never disturb the workspace's resident iterates */
    if (!s->aux) {
      const OSQPWorkspace *w = s->owner;
      hipeng_params prm;
      fill_params(&prm, &s->opt, w->settings->sigma, w->settings->alpha, w->data->n);
      if (hipeng_create(&s->aux, w->data->P, w->data->A, NULL, NULL, NULL, w->rho_vec, &prm,
                        (int)s->opt.device)) return 1;
    }
    e = s->aux;
  }
  if (hipeng_kkt_solve(e, b)) return 1;
  if (s->polish) {   /* return [x ; nu] with nu = (A x - b2)/delta  (qdldl_interface.c:354-356) */
    /* kkt_solve wrote z~ = A x into b[n..]; the caller's b2 is kept in rho_tmp[m..2m) */
    for (c_int i = 0; i < s->m; i++) b[s->n + i] = (b[s->n + i] - s->rho_tmp[s->m + i]) / s->sigma;
  }
  return 0;
}

static c_int pcg_solve_polish(LinSysSolver *self, c_float *b) {
  hip_pcg_solver *s = (hip_pcg_solver *)self;
  for (c_int i = 0; i < s->m; i++) s->rho_tmp[s->m + i] = b[s->n + i];
  return pcg_solve(self, b);
}

static void sens_drop_instance(sens_state *ss) {
  if (!ss) return;
  if (ss->ls) ss->ls->free(ss->ls);
  csc_spfree(ss->Ared);
  ss->ls = NULL; ss->Ared = NULL;
}
static void sens_free(sens_state *ss) {
  if (!ss) return;
  sens_drop_instance(ss);
  hipsens_destroy(ss->dev);
  c_free(ss->pol.Alow_to_A); c_free(ss->pol.Aupp_to_A); c_free(ss->pol.A_to_Alow); c_free(ss->pol.A_to_Aupp);
  c_free(ss->act); c_free(ss->yact); c_free(ss->rnu);
  c_free(ss->rhs); c_free(ss->sol); c_free(ss->res); c_free(ss->tmp);
  c_free(ss);
}

static void pcg_free(LinSysSolver *self) {
  hip_pcg_solver *s = (hip_pcg_solver *)self;
  if (!s) return;
  sens_free(s->sens);
  hipver_destroy(s->ver);
  hipeng_destroy(s->eng);
  hipeng_destroy(s->aux);
  c_free(s->rho_tmp);
  csc_spfree(s->rawP); csc_spfree(s->rawA);
  c_free(s->rawq); c_free(s->rawl); c_free(s->rawu);
  c_free(s);
}

static c_int pcg_update_matrices(LinSysSolver *self, const csc *P, const csc *A) {
  hip_pcg_solver *s = (hip_pcg_solver *)self;
  if (hipeng_upload_matrices(s->eng, P, A)) return 1;
  if (s->aux && hipeng_upload_matrices(s->aux, P, A)) return 1;
  s->sc_iter = -1;
  return 0;
}

static c_int pcg_update_rho_vec(LinSysSolver *self, const c_float *rho_vec) {
  hip_pcg_solver *s = (hip_pcg_solver *)self;
  if (hipeng_upload_rho(s->eng, rho_vec)) return 1;
  if (s->aux && hipeng_upload_rho(s->aux, rho_vec)) return 1;
  return 0;
}

static hip_pcg_solver *pcg_alloc(c_int n, c_int m, c_float sigma, c_int polish) {
  hip_pcg_solver *s = (hip_pcg_solver *)c_calloc(1, sizeof(hip_pcg_solver));
  if (!s) return NULL;
  s->type = HIP_PCG_SOLVER; s->nthreads = 1;
  s->solve = polish ? pcg_solve_polish : pcg_solve;
  s->free = pcg_free;
  s->update_matrices = pcg_update_matrices; s->update_rho_vec = pcg_update_rho_vec;
  s->n = n; s->m = m; s->sigma = sigma; s->polish = polish; s->sc_iter = -1; s->early_iter = -1;
  opt_init();
  s->opt = g_opt;
  return s;
}

/* Stand-alone plugin constructor (lin_sys/direct/qdldl/qdldl_interface.c:177-323
 * is the CPU counterpart).  polish != 0: sigma carries delta, rho_vec is NULL,
 * and the (2,2) block is -delta I  =>  reduced system with rho = 1/delta. */
c_int init_linsys_solver_hip_pcg(LinSysSolver **sp, const csc *P, const csc *A,
                                 c_float sigma, const c_float *rho_vec, c_int polish) {
  if (!sp || !P || !A) return OSQP_LINSYS_SOLVER_INIT_ERROR;
  *sp = NULL;
  hip_pcg_solver *s = pcg_alloc(P->n, A->m, sigma, polish);
  if (!s) return OSQP_LINSYS_SOLVER_INIT_ERROR;
  const c_float *rv = rho_vec;
  if (polish) {
    s->rho_tmp = (c_float *)c_malloc((size_t)(2 * A->m + 1) * sizeof(c_float));
    if (!s->rho_tmp) { c_free(s); return OSQP_LINSYS_SOLVER_INIT_ERROR; }
    for (c_int i = 0; i < A->m; i++) s->rho_tmp[i] = 1.0 / sigma;
    rv = s->rho_tmp;
  }
  hipeng_params prm;
  fill_params(&prm, &s->opt, sigma, 1.0, P->n);
  if (polish) { prm.pcg_eps_rel = HMIN(prm.pcg_eps_rel, 1e-12); }
  if (hipeng_create(&s->eng, P, A, NULL, NULL, NULL, rv, &prm, (int)s->opt.device)) {
    c_free(s->rho_tmp); c_free(s);
    return OSQP_LINSYS_SOLVER_INIT_ERROR;
  }
  *sp = (LinSysSolver *)s;
  return 0;
}

c_int load_linsys_solver(enum linsys_solver_type t)   { (void)t; return 0; }
c_int unload_linsys_solver(enum linsys_solver_type t) { (void)t; return 0; }

/* Every id is served by the HIP PCG plugin: this library carries no CPU
 * factorisation (lin_sys.c:56-75 is the reference dispatch). */
c_int init_linsys_solver(LinSysSolver **s, const csc *P, const csc *A, c_float sigma,
                         const c_float *rho_vec, enum linsys_solver_type t, c_int polish) {
  (void)t;
  return init_linsys_solver_hip_pcg(s, P, A, sigma, rho_vec, polish);
}

/* ------------------------------------------------------------------------ */
/* small host helpers                                                         */
/* ------------------------------------------------------------------------ */
static c_float *dup_vec(const c_float *a, c_int n) {
  c_float *b = (c_float *)c_malloc((size_t)(n > 0 ? n : 1) * sizeof(c_float));
  if (b && n > 0) memcpy(b, a, (size_t)n * sizeof(c_float));
  return b;
}
static c_float *zero_vec(c_int n) { return (c_float *)c_calloc((size_t)(n > 0 ? n : 1), sizeof(c_float)); }

static csc *dup_csc(const csc *A) { return copy_csc_mat(A); }
static void free_csc(csc *A) { csc_spfree(A); }

static c_float absmax(const c_float *v, c_int n) {
  c_float b = 0.0;
  for (c_int k = 0; k < n; k++) { c_float a = fabs(v[k]); if (a > b) b = a; }
  return b;
}

/* ------------------------------------------------------------------------ */
/* status strings (src/auxil.c:651-679)                                       */
/* ------------------------------------------------------------------------ */
static void put_status(OSQPInfo *info, c_int v) {
  static const struct { c_int v; const char *s; } T[] = {
    {OSQP_SOLVED, "solved"}, {OSQP_SOLVED_INACCURATE, "solved inaccurate"},
    {OSQP_PRIMAL_INFEASIBLE, "primal infeasible"},
    {OSQP_PRIMAL_INFEASIBLE_INACCURATE, "primal infeasible inaccurate"},
    {OSQP_UNSOLVED, "unsolved"}, {OSQP_DUAL_INFEASIBLE, "dual infeasible"},
    {OSQP_DUAL_INFEASIBLE_INACCURATE, "dual infeasible inaccurate"},
    {OSQP_MAX_ITER_REACHED, "maximum iterations reached"},
    {OSQP_TIME_LIMIT_REACHED, "run time limit reached"},
    {OSQP_SIGINT, "interrupted"}, {OSQP_NON_CVX, "problem non convex"}};
  info->status_val = v;
  for (size_t k = 0; k < sizeof(T) / sizeof(T[0]); k++)
    if (T[k].v == v) { snprintf(info->status, sizeof(info->status), "%s", T[k].s); return; }
}

static c_int solution_exists(const OSQPInfo *info) {
  c_int v = info->status_val;
  return !(v == OSQP_PRIMAL_INFEASIBLE || v == OSQP_PRIMAL_INFEASIBLE_INACCURATE ||
           v == OSQP_DUAL_INFEASIBLE || v == OSQP_DUAL_INFEASIBLE_INACCURATE || v == OSQP_NON_CVX);
}

static void info_reset(OSQPInfo *info) {   /* src/auxil.c:632-649 */
  info->solve_time = 0.0; info->polish_time = 0.0;
  put_status(info, OSQP_UNSOLVED);
  info->rho_updates = 0;
}

/* ------------------------------------------------------------------------ */
/* defaults and validation                                                    */
/* ------------------------------------------------------------------------ */
void osqp_set_default_settings(OSQPSettings *s) {   /* src/osqp.c:24-71 */
  s->rho = RHO; s->sigma = SIGMA; s->scaling = SCALING;
  s->adaptive_rho = ADAPTIVE_RHO; s->adaptive_rho_interval = ADAPTIVE_RHO_INTERVAL;
  s->adaptive_rho_tolerance = ADAPTIVE_RHO_TOLERANCE; s->adaptive_rho_fraction = ADAPTIVE_RHO_FRACTION;
  s->max_iter = MAX_ITER; s->eps_abs = EPS_ABS; s->eps_rel = EPS_REL;
  s->eps_prim_inf = EPS_PRIM_INF; s->eps_dual_inf = EPS_DUAL_INF; s->alpha = ALPHA;
  s->linsys_solver = HIP_PCG_SOLVER;
  s->delta = DELTA; s->polish = POLISH; s->polish_refine_iter = POLISH_REFINE_ITER;
  s->verbose = VERBOSE; s->scaled_termination = SCALED_TERMINATION;
  s->check_termination = CHECK_TERMINATION; s->warm_start = WARM_START; s->time_limit = TIME_LIMIT;
}

#define FAIL(msg) do { fprintf(stderr, "ERROR in %s: %s\n", __func__, msg); return 1; } while (0)

static c_int check_data(const OSQPData *d) {   /* src/auxil.c:791-879 */
  if (!d) FAIL("Missing data");
  if (!d->P) FAIL("Missing matrix P");
  if (!d->A) FAIL("Missing matrix A");
  if (!d->q) FAIL("Missing vector q");
  if (d->n <= 0 || d->m < 0) FAIL("n must be positive and m nonnegative");
  if (d->P->m != d->n) FAIL("P does not have dimension n x n");
  if (d->P->m != d->P->n) FAIL("P is not square");
  for (c_int j = 0; j < d->n; j++)
    for (c_int k = d->P->p[j]; k < d->P->p[j + 1]; k++)
      if (d->P->i[k] > j) FAIL("P is not upper triangular");
  if (d->A->m != d->m || d->A->n != d->n) FAIL("A does not have dimension m x n");
  for (c_int i = 0; i < d->m; i++)
    if (d->l[i] > d->u[i]) FAIL("Lower bound is greater than upper bound");
  return 0;
}

static c_int check_settings(const OSQPSettings *s) {   /* src/auxil.c:893-1065 */
  if (!s) FAIL("Missing settings!");
  if (s->scaling < 0) FAIL("scaling must be nonnegative");
  if (s->adaptive_rho != 0 && s->adaptive_rho != 1) FAIL("adaptive_rho must be either 0 or 1");
  if (s->adaptive_rho_interval < 0) FAIL("adaptive_rho_interval must be nonnegative");
  if (s->adaptive_rho_fraction <= 0) FAIL("adaptive_rho_fraction must be positive");
  if (s->adaptive_rho_tolerance < 1.0) FAIL("adaptive_rho_tolerance must be >= 1");
  if (s->polish_refine_iter < 0) FAIL("polish_refine_iter must be nonnegative");
  if (s->rho <= 0.0) FAIL("rho must be positive");
  if (s->sigma <= 0.0) FAIL("sigma must be positive");
  if (s->delta <= 0.0) FAIL("delta must be positive");
  if (s->max_iter <= 0) FAIL("max_iter must be positive");
  if (s->eps_abs < 0.0) FAIL("eps_abs must be nonnegative");
  if (s->eps_rel < 0.0) FAIL("eps_rel must be nonnegative");
  if (s->eps_rel == 0.0 && s->eps_abs == 0.0) FAIL("at least one of eps_abs and eps_rel must be positive");
  if (s->eps_prim_inf <= 0.0) FAIL("eps_prim_inf must be positive");
  if (s->eps_dual_inf <= 0.0) FAIL("eps_dual_inf must be positive");
  if (s->alpha <= 0.0 || s->alpha >= 2.0) FAIL("alpha must be strictly between 0 and 2");
  if (s->linsys_solver != QDLDL_SOLVER && s->linsys_solver != MKL_PARDISO_SOLVER &&
      s->linsys_solver != HIP_PCG_SOLVER) FAIL("linsys_solver not recognized");
  if (s->verbose != 0 && s->verbose != 1) FAIL("verbose must be either 0 or 1");
  if (s->scaled_termination != 0 && s->scaled_termination != 1) FAIL("scaled_termination must be either 0 or 1");
  if (s->check_termination < 0) FAIL("check_termination must be nonnegative");
  if (s->warm_start != 0 && s->warm_start != 1) FAIL("warm_start must be either 0 or 1");
  if (s->time_limit < 0.0) FAIL("time_limit must be nonnegative");
  return 0;
}

/* ------------------------------------------------------------------------ */
/* Ruiz equilibration runs on the device (hipeng_ruiz_scale); the host keeps   */
/* the mirrors the API exposes (work->data, work->scaling)                     */
/* ------------------------------------------------------------------------ */
#define PCG_OF(w) ((hip_pcg_solver *)((w)->linsys_solver))
static c_int rescale_on_device(OSQPWorkspace *w);

/* ------------------------------------------------------------------------ */
/* rho by constraint class (src/auxil.c:76-142)                               */
/* ------------------------------------------------------------------------ */
static c_int row_class(c_float l, c_float u) {
  if (l < -BOUND_INF && u > BOUND_INF) return -1;
  if (u - l < RHO_TOL) return 1;
  return 0;
}
static c_float rho_of_class(c_int cls, c_float rho) {
  return cls == -1 ? RHO_MIN : (cls == 1 ? RHO_EQ_OVER_RHO_INEQ * rho : rho);
}

static void init_rho_vec(OSQPWorkspace *w) {
  w->settings->rho = HMIN(HMAX(w->settings->rho, RHO_MIN), RHO_MAX);
  for (c_int i = 0; i < w->data->m; i++) {
    w->constr_type[i] = row_class(w->data->l[i], w->data->u[i]);
    w->rho_vec[i] = rho_of_class(w->constr_type[i], w->settings->rho);
    w->rho_inv_vec[i] = 1. / w->rho_vec[i];
  }
}

static c_int reclassify_rows(OSQPWorkspace *w) {
  c_int changed = 0;
  for (c_int i = 0; i < w->data->m; i++) {
    c_int cls = row_class(w->data->l[i], w->data->u[i]);
    if (cls == w->constr_type[i]) continue;
    w->constr_type[i] = cls;
    w->rho_vec[i] = rho_of_class(cls, w->settings->rho);
    w->rho_inv_vec[i] = 1. / w->rho_vec[i];
    changed = 1;
  }
  if (changed) return w->linsys_solver->update_rho_vec(w->linsys_solver, w->rho_vec);
  return 0;
}

/* The device holds the raw problem; equilibrate it there and refresh the host mirrors
 * (scaled P, A, q, l, u and D, E, c) -- scale_data of src/scaling.c:44-156. */
static c_int rescale_on_device(OSQPWorkspace *w) {
  hip_pcg_solver *s = PCG_OF(w);
  const c_int n = w->data->n, m = w->data->m;
  if (hipeng_ruiz_scale(s->eng, w->settings->scaling, w->scaling->D, w->scaling->E, &w->scaling->c,
                        w->data->q, w->data->l, w->data->u, w->data->P->x, w->data->A->x)) return 1;
  w->scaling->cinv = 1. / w->scaling->c;
  for (c_int j = 0; j < n; j++) w->scaling->Dinv[j] = (c_float)1.0 / w->scaling->D[j];
  for (c_int i = 0; i < m; i++) w->scaling->Einv[i] = (c_float)1.0 / w->scaling->E[i];
  return 0;
}

/* ------------------------------------------------------------------------ */
/* setup / cleanup                                                            */
/* ------------------------------------------------------------------------ */
static c_int setup_fail(c_int code, const char *msg) {
  fprintf(stderr, "ERROR in osqp_setup: %s\n", msg);
  return code;
}

void cold_start(OSQPWorkspace *w) {   /* src/auxil.c:155-159 */
  memset(w->x, 0, (size_t)w->data->n * sizeof(c_float));
  if (w->data->m) {
    memset(w->z, 0, (size_t)w->data->m * sizeof(c_float));
    memset(w->y, 0, (size_t)w->data->m * sizeof(c_float));
  }
  if (w->linsys_solver && PCG(w)->eng) hipeng_cold_start(PCG(w)->eng);
}

c_int osqp_setup(OSQPWorkspace **workp, const OSQPData *data, const OSQPSettings *settings) {
  if (check_data(data)) return setup_fail(OSQP_DATA_VALIDATION_ERROR, "Data validation returned failure");
  if (check_settings(settings)) return setup_fail(OSQP_SETTINGS_VALIDATION_ERROR, "Settings validation returned failure");
  OSQPWorkspace *w = (OSQPWorkspace *)c_calloc(1, sizeof(OSQPWorkspace));
  if (!w) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  *workp = w;   /* set early: cleanup after a failed setup must work (osqp.c:88-90) */
  const c_int n = data->n, m = data->m;
  w->timer = (OSQPTimer *)c_malloc(sizeof(OSQPTimer));
  if (!w->timer) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  tic(w->timer);

  w->data = (OSQPData *)c_calloc(1, sizeof(OSQPData));
  if (!w->data) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  w->data->n = n; w->data->m = m;
  w->data->P = dup_csc(data->P); w->data->A = dup_csc(data->A);
  w->data->q = dup_vec(data->q, n); w->data->l = dup_vec(data->l, m); w->data->u = dup_vec(data->u, m);
  w->rho_vec = zero_vec(m); w->rho_inv_vec = zero_vec(m);
  w->constr_type = (c_int *)c_calloc((size_t)(m > 0 ? m : 1), sizeof(c_int));
  w->x = zero_vec(n); w->z = zero_vec(m); w->xz_tilde = zero_vec(n + m);
  w->x_prev = zero_vec(n); w->z_prev = zero_vec(m); w->y = zero_vec(m);
  w->Ax = zero_vec(m); w->Px = zero_vec(n); w->Aty = zero_vec(n);
  w->delta_y = zero_vec(m); w->Atdelta_y = zero_vec(n);
  w->delta_x = zero_vec(n); w->Pdelta_x = zero_vec(n); w->Adelta_x = zero_vec(m);
  w->settings = (OSQPSettings *)c_malloc(sizeof(OSQPSettings));
  w->solution = (OSQPSolution *)c_calloc(1, sizeof(OSQPSolution));
  w->info = (OSQPInfo *)c_calloc(1, sizeof(OSQPInfo));
  w->pol = (OSQPPolish *)c_calloc(1, sizeof(OSQPPolish));
  if (!w->data->P || !w->data->A || !w->data->q || !w->data->l || !w->data->u || !w->rho_vec ||
      !w->rho_inv_vec || !w->constr_type || !w->x || !w->z || !w->xz_tilde || !w->x_prev ||
      !w->z_prev || !w->y || !w->Ax || !w->Px || !w->Aty || !w->delta_y || !w->Atdelta_y ||
      !w->delta_x || !w->Pdelta_x || !w->Adelta_x || !w->settings || !w->solution || !w->info || !w->pol)
    return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  *w->settings = *settings;
  w->solution->x = zero_vec(n); w->solution->y = zero_vec(m);
  size_t mm = (size_t)(m > 0 ? m : 1);
  w->pol->Alow_to_A = (c_int *)c_malloc(mm * sizeof(c_int)); w->pol->Aupp_to_A = (c_int *)c_malloc(mm * sizeof(c_int));
  w->pol->A_to_Alow = (c_int *)c_malloc(mm * sizeof(c_int)); w->pol->A_to_Aupp = (c_int *)c_malloc(mm * sizeof(c_int));
  w->pol->x = zero_vec(n); w->pol->z = zero_vec(m); w->pol->y = zero_vec(m);
  if (!w->solution->x || !w->solution->y || !w->pol->Alow_to_A || !w->pol->Aupp_to_A ||
      !w->pol->A_to_Alow || !w->pol->A_to_Aupp || !w->pol->x || !w->pol->z || !w->pol->y)
    return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");

  if (settings->scaling) {
    w->scaling = (OSQPScaling *)c_calloc(1, sizeof(OSQPScaling));
    if (!w->scaling) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
    w->scaling->D = zero_vec(n); w->scaling->Dinv = zero_vec(n);
    w->scaling->E = zero_vec(m); w->scaling->Einv = zero_vec(m);
    w->D_temp = zero_vec(n); w->D_temp_A = zero_vec(n); w->E_temp = zero_vec(m);
    if (!w->scaling->D || !w->scaling->Dinv || !w->scaling->E || !w->scaling->Einv ||
        !w->D_temp || !w->D_temp_A || !w->E_temp)
      return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  }

  /* device engine = the workspace's linear-system plugin; it is created on the RAW problem and
   * equilibrates it in place on the GPU (scale_data, src/scaling.c:44-156) */
  hip_pcg_solver *s = pcg_alloc(n, m, w->settings->sigma, 0);
  if (!s) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  s->owner = w;
  w->linsys_solver = (LinSysSolver *)s;
  if (settings->scaling) {
    s->rawP = dup_csc(data->P); s->rawA = dup_csc(data->A);
    s->rawq = dup_vec(data->q, n); s->rawl = dup_vec(data->l, m); s->rawu = dup_vec(data->u, m);
    if (!s->rawP || !s->rawA || !s->rawq || !s->rawl || !s->rawu)
      return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
  }
  hipeng_params prm;
  fill_params(&prm, &s->opt, w->settings->sigma, w->settings->alpha, n);
  int rc = hipeng_create(&s->eng, w->data->P, w->data->A, w->data->q, w->data->l, w->data->u,
                         NULL, &prm, (int)s->opt.device);
  if (rc == HIPENG_ERR_NO_DEVICE)
    return setup_fail(OSQP_LINSYS_SOLVER_LOAD_ERROR, "no HIP device: the HIP PCG solver cannot be loaded");
  if (rc) return setup_fail(OSQP_LINSYS_SOLVER_INIT_ERROR, "HIP engine initialisation failed");
  if (settings->scaling && rescale_on_device(w))
    return setup_fail(OSQP_LINSYS_SOLVER_INIT_ERROR, "HIP engine initialisation failed");
  init_rho_vec(w);
  if (hipeng_upload_rho(s->eng, w->rho_vec))
    return setup_fail(OSQP_LINSYS_SOLVER_INIT_ERROR, "HIP engine initialisation failed");
  /* Convexity probe.  The reference rejects a KKT matrix whose LDL^T factor has fewer than n
   * positive pivots (qdldl_interface.c:93-99, OSQP_NONCVX_ERROR), i.e. a reduced matrix
   * P + sigma I + A' rho A that is not positive definite.  An iterative solver has no inertia;
   * the equivalent signal is negative curvature p'Kp <= 0 met by CG.  A short CG run on a
   * fixed pseudo-random right-hand side is a best-effort version of that test (up to 300 iterations; it
   * ends as soon as the solve converges, and during it ANY loss of positivity in the recurrence counts --
   * no restart at the rounding floor, hipeng_params.no_restart). */
  {
    c_int probe = HMIN(HMAX(2 * n, 8), 300);
    hipeng_params pp = prm;
    pp.pcg_max_iter = probe; pp.no_restart = 1;
    c_float *rhs = (c_float *)c_malloc((size_t)(n + m + 1) * sizeof(c_float));
    unsigned long long lcg = 88172645463325252ULL;
    if (!rhs) return setup_fail(OSQP_MEM_ALLOC_ERROR, "Memory allocation failed");
    for (c_int k = 0; k < n + m; k++) {
      lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
      rhs[k] = (c_float)((lcg >> 11) & 0xFFFFF) / 1048576.0 - 0.5;
    }
    hipeng_stats hs;
    int bad = hipeng_set_params(s->eng, &pp) || hipeng_kkt_solve_unrefined(s->eng, rhs) || hipeng_get_stats(s->eng, &hs);
    c_free(rhs);
    if (bad) return setup_fail(OSQP_LINSYS_SOLVER_INIT_ERROR, "HIP engine initialisation failed");
    if (hs.neg_curvature > 0)
      return setup_fail(OSQP_NONCVX_ERROR, "KKT matrix factorization.\nThe problem seems to be non-convex");
    hipeng_set_params(s->eng, &prm);
    hipeng_cold_start(s->eng);
    hipeng_reset_stats(s->eng);
  }

  w->info->status_polish = 0;
  put_status(w->info, OSQP_UNSOLVED);
  w->info->setup_time = toc(w->timer);
  w->first_run = 1; w->clear_update_time = 0; w->rho_update_from_solve = 0;
  w->info->rho_updates = 0;
  w->info->rho_estimate = w->settings->rho;
  w->summary_printed = 0;
  if (w->settings->verbose)
    printf("osqp_amd (HIP/gfx950): variables n = %lld, constraints m = %lld, nnz(P)+nnz(A) = %lld; "
           "linear system solver = hip pcg\n", (long long)n, (long long)m,
           (long long)(w->data->P->p[n] + w->data->A->p[n]));
  return 0;
}

c_int osqp_cleanup(OSQPWorkspace *w) {   /* src/osqp.c:659-757 */
  if (!w) return 0;
  if (w->data) {
    free_csc(w->data->P); free_csc(w->data->A);
    c_free(w->data->q); c_free(w->data->l); c_free(w->data->u); c_free(w->data);
  }
  if (w->scaling) {
    c_free(w->scaling->D); c_free(w->scaling->Dinv); c_free(w->scaling->E); c_free(w->scaling->Einv);
    c_free(w->scaling);
  }
  c_free(w->D_temp); c_free(w->D_temp_A); c_free(w->E_temp);
  if (w->linsys_solver && w->linsys_solver->free) w->linsys_solver->free(w->linsys_solver);
  if (w->pol) {
    c_free(w->pol->Alow_to_A); c_free(w->pol->Aupp_to_A); c_free(w->pol->A_to_Alow); c_free(w->pol->A_to_Aupp);
    c_free(w->pol->x); c_free(w->pol->z); c_free(w->pol->y); c_free(w->pol);
  }
  c_free(w->rho_vec); c_free(w->rho_inv_vec); c_free(w->constr_type);
  c_free(w->x); c_free(w->z); c_free(w->xz_tilde); c_free(w->x_prev); c_free(w->z_prev); c_free(w->y);
  c_free(w->Ax); c_free(w->Px); c_free(w->Aty); c_free(w->delta_y); c_free(w->Atdelta_y);
  c_free(w->delta_x); c_free(w->Pdelta_x); c_free(w->Adelta_x);
  c_free(w->settings);
  if (w->solution) { c_free(w->solution->x); c_free(w->solution->y); c_free(w->solution); }
  c_free(w->info); c_free(w->timer); c_free(w);
  return 0;
}

/* ------------------------------------------------------------------------ */
/* info from device scalars (src/auxil.c:227-359, 564-629)                    */
/* ------------------------------------------------------------------------ */
static c_int use_unscaled(const OSQPWorkspace *w) {
  return w->settings->scaling && !w->settings->scaled_termination;
}

static c_int refresh_info(OSQPWorkspace *w, c_int iter, c_int with_obj) {
  hip_pcg_solver *s = PCG(w);
  if (s->early_iter == iter) s->sc = s->early;      /* the window's own wait brought them (hipeng_run_admm_check): used once */
  else {
    if (hipeng_residuals(s->eng, &s->sc)) return 1;
    s->host_syncs++;
  }
  s->early_iter = -1;
  s->sc_iter = iter;
  w->info->iter = iter;
  if (with_obj) w->info->obj_val = s->sc.obj_scaled * (w->settings->scaling ? w->scaling->cinv : 1.0);
  if (w->data->m == 0) w->info->pri_res = 0.;
  else w->info->pri_res = use_unscaled(w) ? s->sc.pri_res_u : s->sc.pri_res_s;
  w->info->dua_res = use_unscaled(w) ? w->scaling->cinv * s->sc.dua_res_u : s->sc.dua_res_s;
  w->info->solve_time = toc(w->timer);
  w->summary_printed = 0;
  return 0;
}

/* status decision on the reduced scalars (src/auxil.c:681-786) */
static c_int decide_termination(OSQPWorkspace *w, c_int approximate) {
  hip_pcg_solver *s = PCG(w);
  hipeng_scalars *sc = &s->sc;
  const OSQPSettings *st = w->settings;
  const c_int un = use_unscaled(w);
  c_float eps_abs = st->eps_abs, eps_rel = st->eps_rel;
  c_float eps_pinf = st->eps_prim_inf, eps_dinf = st->eps_dual_inf;
  c_int prim_ok = 0, dual_ok = 0, pinf = 0, dinf = 0;

  if (w->info->pri_res > OSQP_INFTY || w->info->dua_res > OSQP_INFTY) {
    put_status(w->info, OSQP_NON_CVX);
    w->info->obj_val = OSQP_NAN;
    return 1;
  }
  if (approximate) { eps_abs *= 10; eps_rel *= 10; eps_pinf *= 10; eps_dinf *= 10; }

  /* candidates for the second-stage (SpMV) certificates */
  c_int need_cert = 0, pinf_cand = 0, dinf_cand = 0;
  c_float ndy = un ? sc->dy_norm_u : sc->dy_norm_s;
  c_float ndx = un ? sc->dx_norm_u : sc->dx_norm_s;
  c_float cs = un ? w->scaling->c : 1.0;

  if (w->data->m == 0) prim_ok = 1;
  else {
    c_float eps_prim = eps_abs + eps_rel * (un ? HMAX(sc->z_u, sc->Ax_u) : HMAX(sc->z_s, sc->Ax_s));
    if (w->info->pri_res < eps_prim) prim_ok = 1;
    else if (ndy > OSQP_DIVISION_TOL && sc->dy_lhs < eps_pinf * ndy) { pinf_cand = 1; need_cert = 1; }
  }
  {
    c_float nrm = un ? w->scaling->cinv * HMAX(HMAX(sc->q_u, sc->Aty_u), sc->Px_u)
                     : HMAX(HMAX(sc->q_s, sc->Aty_s), sc->Px_s);
    c_float eps_dual = eps_abs + eps_rel * nrm;
    if (w->info->dua_res < eps_dual) dual_ok = 1;
    else if (ndx > OSQP_DIVISION_TOL && sc->q_dx < cs * eps_dinf * ndx) { dinf_cand = 1; need_cert = 1; }
  }
  if (need_cert && !(prim_ok && dual_ok)) {
    if (hipeng_certificates(s->eng, eps_dinf * ndx, (int)un, sc)) return 0;
    s->host_syncs++;
    if (pinf_cand) pinf = (un ? sc->Atdy_u : sc->Atdy_s) < eps_pinf * ndy;
    if (dinf_cand) dinf = ((un ? sc->Pdx_u : sc->Pdx_s) < cs * eps_dinf * ndx) && (sc->Adx_viol == 0.0);
  }

  if (prim_ok && dual_ok) {
    put_status(w->info, approximate ? OSQP_SOLVED_INACCURATE : OSQP_SOLVED);
    return 1;
  }
  if (pinf) {
    put_status(w->info, approximate ? OSQP_PRIMAL_INFEASIBLE_INACCURATE : OSQP_PRIMAL_INFEASIBLE);
    w->info->obj_val = OSQP_INFTY;
    return 1;
  }
  if (dinf) {
    put_status(w->info, approximate ? OSQP_DUAL_INFEASIBLE_INACCURATE : OSQP_DUAL_INFEASIBLE);
    w->info->obj_val = -OSQP_INFTY;
    return 1;
  }
  return 0;
}

/* src/auxil.c:13-52 on the scaled norms */
static c_float estimate_rho(const OSQPWorkspace *w) {
  const hipeng_scalars *sc = &PCG(w)->sc;
  c_float pri = (w->data->m ? sc->pri_res_s : 0.0) / (HMAX(sc->z_s, sc->Ax_s) + OSQP_DIVISION_TOL);
  c_float dua = sc->dua_res_s / (HMAX(HMAX(sc->q_s, sc->Aty_s), sc->Px_s) + OSQP_DIVISION_TOL);
  c_float r = w->settings->rho * sqrt(pri / dua);
  return HMIN(HMAX(r, RHO_MIN), RHO_MAX);
}

static c_int maybe_adapt_rho(OSQPWorkspace *w) {   /* src/auxil.c:54-74 */
  c_float r = estimate_rho(w);
  c_int rc = 0;
  w->info->rho_estimate = r;
  if (r > w->settings->rho * w->settings->adaptive_rho_tolerance ||
      r < w->settings->rho / w->settings->adaptive_rho_tolerance) {
    rc = osqp_update_rho(w, r);
    w->info->rho_updates += 1;
  }
  return rc;
}

static void print_line(const OSQPWorkspace *w) {
  printf("%4lld  %12.4e  %9.2e  %9.2e  %9.2e  %9.2es\n", (long long)w->info->iter, w->info->obj_val,
         w->info->pri_res, w->info->dua_res, w->settings->rho,
         w->info->solve_time + (w->first_run ? w->info->setup_time : w->info->update_time));
}

/* src/auxil.c:524-562 + src/scaling.c:177-192 */
static c_int extract_solution(OSQPWorkspace *w) {
  hip_pcg_solver *s = PCG(w);
  const c_int n = w->data->n, m = w->data->m;
  const c_int v = w->info->status_val;
  const c_int pinf = (v == OSQP_PRIMAL_INFEASIBLE || v == OSQP_PRIMAL_INFEASIBLE_INACCURATE);
  if (hipeng_download(s->eng, w->x, w->y, w->z, w->delta_x, w->delta_y, (int)pinf)) return 1;
  s->host_syncs++;
  if (solution_exists(w->info)) {
    memcpy(w->solution->x, w->x, (size_t)n * sizeof(c_float));
    if (m) memcpy(w->solution->y, w->y, (size_t)m * sizeof(c_float));
    if (w->settings->scaling) {
      for (c_int j = 0; j < n; j++) w->solution->x[j] = w->solution->x[j] * w->scaling->D[j];
      for (c_int i = 0; i < m; i++) w->solution->y[i] = w->solution->y[i] * w->scaling->E[i];
      for (c_int i = 0; i < m; i++) w->solution->y[i] *= w->scaling->cinv;
    }
  } else {
    for (c_int j = 0; j < n; j++) w->solution->x[j] = OSQP_NAN;
    for (c_int i = 0; i < m; i++) w->solution->y[i] = OSQP_NAN;
    if (pinf) {   /* certificate: E.dy (auxil.c:757-760), normalised (auxil.c:545-549) */
      if (use_unscaled(w)) for (c_int i = 0; i < m; i++) w->delta_y[i] = w->delta_y[i] * w->scaling->E[i];
      c_float nv = absmax(w->delta_y, m);
      for (c_int i = 0; i < m; i++) w->delta_y[i] *= 1. / nv;
    }
    if (v == OSQP_DUAL_INFEASIBLE || v == OSQP_DUAL_INFEASIBLE_INACCURATE) {
      if (use_unscaled(w)) for (c_int j = 0; j < n; j++) w->delta_x[j] = w->delta_x[j] * w->scaling->D[j];
      c_float nv = absmax(w->delta_x, n);
      for (c_int j = 0; j < n; j++) w->delta_x[j] *= 1. / nv;
    }
    cold_start(w);
  }
  return 0;
}

static c_int run_polish(OSQPWorkspace *w);

/* the solved point is gone (a new solve starts, or data, rho or the iterates change): so is the KKT instance of its derivatives */
static void sens_invalidate(OSQPWorkspace *w) {
  hip_pcg_solver *s = PCG(w);
  if (!s) return;
  s->sens_ready = 0;
  sens_drop_instance(s->sens);
}

/* ------------------------------------------------------------------------ */
/* osqp_solve (src/osqp.c:288-654)                                            */
/* ------------------------------------------------------------------------ */
c_int osqp_solve(OSQPWorkspace *w) {
  if (!w) { fprintf(stderr, "ERROR in osqp_solve: Workspace not initialized\n"); return OSQP_WORKSPACE_NOT_INIT_ERROR; }
  hip_pcg_solver *s = PCG(w);
  OSQPSettings *st = w->settings;
  c_int exitflag = 0, iter = 0, can_check = 0, can_print = 0;
  const c_int with_obj = st->verbose;

  sens_invalidate(w);
  if (w->clear_update_time == 1) w->info->update_time = 0.0;
  w->rho_update_from_solve = 1;
  tic(w->timer);
  if (st->verbose) printf("iter   objective    pri res    dua res    rho        time\n");

  hipeng_params prm;
  fill_params(&prm, &s->opt, st->sigma, st->alpha, w->data->n);
  /* opt-in inexact mode (not parity-exact): the linear solves are only as accurate as the ADMM
   * iterate needs -- PCG stops at lambda * sqrt(||r_prim|| * ||r_dual||) (scaled residuals of the
   * last evaluation), the rule of Schubiger, Banjac, Lygeros (JPDC 144, 2020) cited by the
   * reference (docs/citing/index.rst:45-59); until the first evaluation a loose relative one */
  /* A direct factorisation is exact whatever eps_abs/eps_rel ask for; an indirect solve that stops at eps_pcg * ||b||
   * leaves a floor under the ADMM residuals and a distance to the direct solver's iterates.  Measured on config 2
   * (tools/pcg_tol_sweep.py, eps = 1e-4, against the recorded run of the CPU direct solver): x, y deviate by 1.3 ... 5 x eps_pcg,
   * the residuals by 3e-6 / 9e-5 / 5e-4 relative at eps_pcg = 1e-9 / 1e-8 / 1e-7, iteration counts stay equal throughout.
   * The stop is therefore tied to the request: 1e-5 * min(eps_abs, eps_rel), never looser than the option pcg_eps_rel
   * (default 1e-9) -- x, y 250 times inside the 1e-6 bar of the parity tests, residuals 30 times inside theirs (round 1
   * used 1e-6 * eps: 2.4 more PCG iterations per solve at config 2 for digits nothing looks at). */
  {
    const c_float e = HMIN(st->eps_abs > 0 ? st->eps_abs : st->eps_rel, st->eps_rel > 0 ? st->eps_rel : st->eps_abs);
    const double factor = g_pcg_eps_factor;
    prm.pcg_eps_rel = s->opt.pcg_eps_rel;
    if (e > 0) prm.pcg_eps_rel = HMAX(1e-13, HMIN(prm.pcg_eps_rel, factor * e));
    /* Equality rows carry rho_eq = 1e3 rho (constants.h:70): ||b|| is then dominated by their terms and a stop
     * relative to ||b|| leaves the rest of x~ far less accurate (configs 3 and 5: x, y within 1e-4 of the direct
     * solve at 1e-10, within 1e-6 at 1e-12).  Such problems get a stop 1e3 times tighter. */
    /* ... unless the engine has eliminated a slack-like variable through that row (engine_aux_kernels.h, k_elim_refresh): the row then
     * enters the reduced system with rho~ = rho (P_yy + sigma) / (P_yy + sigma + rho a^2), not with 1e3 rho. */
    for (c_int i = 0; i < w->data->m; i++)
      if (w->constr_type[i] == 1 && !hipeng_row_eliminated(s->eng, i)) { prm.pcg_eps_rel = HMAX(1e-13, 1e-3 * prm.pcg_eps_rel); break; }
  }
  const c_int adaptive_pcg = s->opt.pcg_adaptive;
  const c_float strict_rel = prm.pcg_eps_rel;
  if (adaptive_pcg) prm.pcg_eps_rel = 1e-3;
  if (hipeng_set_params(s->eng, &prm)) { exitflag = 1; goto done; }

  c_int rho_interval = st->adaptive_rho_interval;
  if (st->adaptive_rho && !rho_interval)
    rho_interval = st->check_termination ? ADAPTIVE_RHO_MULTIPLE_TERMINATION * st->check_termination
                                         : ADAPTIVE_RHO_FIXED;

  if (!st->warm_start) cold_start(w);
  s->sc_iter = -1;
  s->early_iter = -1;

  while (iter < st->max_iter) {
    /* next iteration count at which the reference would look at the iterates */
    c_int next = st->max_iter;
    if (st->check_termination) next = HMIN(next, (iter / st->check_termination + 1) * st->check_termination);
    if (st->adaptive_rho && rho_interval) next = HMIN(next, (iter / rho_interval + 1) * rho_interval);
    if (st->verbose) next = HMIN(next, iter == 0 ? 1 : (iter / PRINT_INTERVAL + 1) * PRINT_INTERVAL);
    next = HMIN(next, iter + (st->time_limit ? 8 : 128));
    /* a window that ends where the residuals are looked at (a check, a printed line, a rho-interval check, the last iteration)
     * takes them behind its own iterations: one wait instead of two */
    {
      const c_int will_check = st->check_termination && (next % st->check_termination == 0);
      const c_int will_print = st->verbose && ((next % PRINT_INTERVAL == 0) || (next == 1));
      const c_int will_rho = st->adaptive_rho && rho_interval && (next % rho_interval == 0);
      int have = 0;
      s->early_iter = -1;
      if (will_check || will_print || will_rho || next == st->max_iter) {
        if (hipeng_run_admm_check(s->eng, next - iter, &s->early, &have)) { exitflag = 1; goto done; }
      } else if (hipeng_run_admm(s->eng, next - iter)) { exitflag = 1; goto done; }
      s->host_syncs++;
      if (have) s->early_iter = next;
    }
    iter = next;

    if (st->time_limit) {
      c_float t = (w->first_run ? w->info->setup_time : w->info->update_time) + toc(w->timer);
      if (t >= st->time_limit) {
        put_status(w->info, OSQP_TIME_LIMIT_REACHED);
        if (st->verbose) printf("run time limit reached\n");
        can_print = 0; can_check = 0;
        break;
      }
    }
    can_check = st->check_termination && (iter % st->check_termination == 0);
    can_print = st->verbose && ((iter % PRINT_INTERVAL == 0) || (iter == 1));
    if (can_check || can_print) {
      if (refresh_info(w, iter, with_obj)) { exitflag = 1; goto done; }
      if (can_print) { print_line(w); w->summary_printed = 1; }
      if (can_check && decide_termination(w, 0)) break;
    }
    if (adaptive_pcg && s->sc_iter == iter) {
      const c_float lam = 0.15;
      prm.pcg_eps_rel = strict_rel;
      prm.pcg_eps_abs = lam * sqrt(HMAX(s->sc.pri_res_s, 1e-300) * HMAX(s->sc.dua_res_s, 1e-300));
      if (hipeng_set_params(s->eng, &prm)) { exitflag = 1; goto done; }
    }
    if (st->adaptive_rho && rho_interval && (iter % rho_interval == 0)) {
      if (!can_check && !can_print && refresh_info(w, iter, with_obj)) { exitflag = 1; goto done; }
      if (maybe_adapt_rho(w)) { fprintf(stderr, "ERROR in osqp_solve: Failed rho update\n"); exitflag = 1; goto done; }
    }
  }

  if (!can_check) {
    /* On a time limit the reference breaks at the TOP of iteration k and reports k - 1 = the iterations it completed
     * (osqp.c:404, 545).  Here the limit is polled after a window, so `iter` iterations are complete and x, y and the
     * residuals belong to iterate `iter`: that is the count reported. */
    if (!can_print && refresh_info(w, iter, with_obj)) { exitflag = 1; goto done; }
    if (st->verbose && !w->summary_printed) { print_line(w); w->summary_printed = 1; }
    decide_termination(w, 0);
  }
  if (!with_obj && solution_exists(w->info)) {
    if (s->sc_iter != iter && refresh_info(w, iter, 0)) { exitflag = 1; goto done; }
    w->info->obj_val = s->sc.obj_scaled * (st->scaling ? w->scaling->cinv : 1.0);
  }
  if (st->verbose && !w->summary_printed) { print_line(w); w->summary_printed = 1; }

  if (w->info->status_val == OSQP_UNSOLVED) {
    if (!decide_termination(w, 1)) put_status(w->info, OSQP_MAX_ITER_REACHED);
  }
  if (w->info->status_val == OSQP_TIME_LIMIT_REACHED) {
    if (!decide_termination(w, 1)) put_status(w->info, OSQP_TIME_LIMIT_REACHED);
  }
  w->info->rho_estimate = estimate_rho(w);
  w->info->solve_time = toc(w->timer);

  /* host mirrors of the iterates + solution (one download per solve) */
  if (extract_solution(w)) { exitflag = 1; goto done; }

  if (st->polish && w->info->status_val == OSQP_SOLVED) run_polish(w);
  s->sens_ready = 1;

  w->info->run_time = (w->first_run ? w->info->setup_time : w->info->update_time) +
                      w->info->solve_time + w->info->polish_time;
  if (w->first_run) w->first_run = 0;
  w->clear_update_time = 1;
  w->rho_update_from_solve = 0;
  if (st->verbose)
    printf("status: %s, iterations: %lld, objective: %.4f, run time: %.2es, rho estimate: %.2e\n",
           w->info->status, (long long)w->info->iter, w->info->obj_val, w->info->run_time,
           w->info->rho_estimate);
  {
    /* An indirect solve that hit its iteration cap (or broke down) was accepted as it stood.  OSQPInfo is ABI and has no
     * field for it, so: one line on stderr per workspace, whatever `verbose` says (every solve when verbose);
     * osqp_amd_get_stats(work, &st) -> st.pcg_forced has the count.  The reference's direct solve has no such state. */
    hipeng_stats hs;
    if (!hipeng_get_stats(s->eng, &hs) && hs.pcg_forced > 0 && (st->verbose || !s->forced_warned)) {
      s->forced_warned = 1;
      fprintf(stderr, "osqp_amd warning: %lld linear solve(s) of this workspace so far stopped at the PCG iteration cap or on a breakdown "
                      "before reaching the requested accuracy; the iterates were accepted as they stood (osqp_amd_get_stats: "
                      "pcg_forced; OSQP_AMD_PCG_MAX_ITER raises the cap)\n", (long long)hs.pcg_forced);
    }
  }
done:
  return exitflag;
}

/* ------------------------------------------------------------------------ */
/* data updates (src/osqp.c:765-1332)                                         */
/* ------------------------------------------------------------------------ */
static void upd_begin(OSQPWorkspace *w) {
  if (w->clear_update_time == 1) { w->clear_update_time = 0; w->info->update_time = 0.0; }
  tic(w->timer);
}
static void upd_end(OSQPWorkspace *w) { w->info->update_time += toc(w->timer); }
#define NEED_WORK(w) do { if (!(w)) { fprintf(stderr, "ERROR in %s: Workspace not initialized\n", __func__); \
                                      return OSQP_WORKSPACE_NOT_INIT_ERROR; } } while (0)

c_int osqp_update_lin_cost(OSQPWorkspace *w, const c_float *q_new) {
  NEED_WORK(w);
  upd_begin(w);
  sens_invalidate(w);
  ver_mark(w, VER_Q);
  const c_int n = w->data->n;
  memcpy(w->data->q, q_new, (size_t)n * sizeof(c_float));
  if (w->settings->scaling) {
    memcpy(PCG(w)->rawq, q_new, (size_t)n * sizeof(c_float));
    for (c_int j = 0; j < n; j++) w->data->q[j] = w->data->q[j] * w->scaling->D[j];
    for (c_int j = 0; j < n; j++) w->data->q[j] *= w->scaling->c;
  }
  if (hipeng_upload_q(PCG(w)->eng, w->data->q)) return 1;
  info_reset(w->info);
  upd_end(w);
  return 0;
}

static c_int push_bounds(OSQPWorkspace *w) {
  sens_invalidate(w);
  if (hipeng_upload_bounds(PCG(w)->eng, w->data->l, w->data->u)) return 1;
  info_reset(w->info);
  return reclassify_rows(w);
}

c_int osqp_update_bounds(OSQPWorkspace *w, const c_float *l_new, const c_float *u_new) {
  NEED_WORK(w);
  upd_begin(w);
  const c_int m = w->data->m;
  for (c_int i = 0; i < m; i++)
    if (l_new[i] > u_new[i]) { fprintf(stderr, "ERROR in osqp_update_bounds: lower bound must be lower than or equal to upper bound\n"); return 1; }
  ver_mark(w, VER_L | VER_U);
  memcpy(w->data->l, l_new, (size_t)m * sizeof(c_float));
  memcpy(w->data->u, u_new, (size_t)m * sizeof(c_float));
  if (w->settings->scaling) { memcpy(PCG(w)->rawl, l_new, (size_t)m * sizeof(c_float)); memcpy(PCG(w)->rawu, u_new, (size_t)m * sizeof(c_float)); }
  if (w->settings->scaling)
    for (c_int i = 0; i < m; i++) { w->data->l[i] = w->data->l[i] * w->scaling->E[i]; w->data->u[i] = w->data->u[i] * w->scaling->E[i]; }
  c_int rc = push_bounds(w);
  upd_end(w);
  return rc;
}

c_int osqp_update_lower_bound(OSQPWorkspace *w, const c_float *l_new) {
  NEED_WORK(w);
  upd_begin(w);
  const c_int m = w->data->m;
  ver_mark(w, VER_L);
  memcpy(w->data->l, l_new, (size_t)m * sizeof(c_float));
  if (w->settings->scaling) memcpy(PCG(w)->rawl, l_new, (size_t)m * sizeof(c_float));
  if (w->settings->scaling) for (c_int i = 0; i < m; i++) w->data->l[i] = w->data->l[i] * w->scaling->E[i];
  for (c_int i = 0; i < m; i++)
    if (w->data->l[i] > w->data->u[i]) { fprintf(stderr, "ERROR in osqp_update_lower_bound: upper bound must be greater than or equal to lower bound\n"); return 1; }
  c_int rc = push_bounds(w);
  upd_end(w);
  return rc;
}

c_int osqp_update_upper_bound(OSQPWorkspace *w, const c_float *u_new) {
  NEED_WORK(w);
  upd_begin(w);
  const c_int m = w->data->m;
  ver_mark(w, VER_U);
  memcpy(w->data->u, u_new, (size_t)m * sizeof(c_float));
  if (w->settings->scaling) memcpy(PCG(w)->rawu, u_new, (size_t)m * sizeof(c_float));
  if (w->settings->scaling) for (c_int i = 0; i < m; i++) w->data->u[i] = w->data->u[i] * w->scaling->E[i];
  for (c_int i = 0; i < m; i++)
    if (w->data->u[i] < w->data->l[i]) { fprintf(stderr, "ERROR in osqp_update_upper_bound: lower bound must be lower than or equal to upper bound\n"); return 1; }
  c_int rc = push_bounds(w);
  upd_end(w);
  return rc;
}

static c_int warm(OSQPWorkspace *w, const c_float *x, const c_float *y) {
  const c_int n = w->data->n, m = w->data->m;
  sens_invalidate(w);
  if (!w->settings->warm_start) w->settings->warm_start = 1;
  if (x) {
    memcpy(w->x, x, (size_t)n * sizeof(c_float));
    if (w->settings->scaling) for (c_int j = 0; j < n; j++) w->x[j] = w->x[j] * w->scaling->Dinv[j];
  }
  if (y) {
    memcpy(w->y, y, (size_t)m * sizeof(c_float));
    if (w->settings->scaling) {
      for (c_int i = 0; i < m; i++) w->y[i] = w->y[i] * w->scaling->Einv[i];
      for (c_int i = 0; i < m; i++) w->y[i] *= w->scaling->c;
    }
  }
  /* z = A x is evaluated on the device (osqp.c:960-963) */
  return hipeng_set_iterates(PCG(w)->eng, x ? w->x : NULL, y ? w->y : NULL) ? 1 : 0;
}
c_int osqp_warm_start(OSQPWorkspace *w, const c_float *x, const c_float *y) { NEED_WORK(w); return warm(w, x, y); }
c_int osqp_warm_start_x(OSQPWorkspace *w, const c_float *x) { NEED_WORK(w); return warm(w, x, NULL); }
c_int osqp_warm_start_y(OSQPWorkspace *w, const c_float *y) { NEED_WORK(w); return warm(w, NULL, y); }

static c_int patch(OSQPWorkspace *w, const c_float *Px, const c_int *Pi, c_int Pn, int doP,
                   const c_float *Ax, const c_int *Ai, c_int An, int doA) {
  hip_pcg_solver *s = PCG(w);
  const c_int nnzP = w->data->P->p[w->data->P->n], nnzA = w->data->A->p[w->data->A->n];
  upd_begin(w);
  sens_invalidate(w);
  if (doP && Pi && Pn > nnzP) { fprintf(stderr, "ERROR: new number of elements greater than elements in P\n"); return 1; }
  if (doA && Ai && An > nnzA) { fprintf(stderr, "ERROR: new number of elements greater than elements in A\n"); return doP ? 2 : 1; }
  /* the reference trusts the index arrays; an index outside the matrix would write past its values */
  if (doP && Pi) for (c_int k = 0; k < Pn; k++) if (Pi[k] < 0 || Pi[k] >= nnzP) { fprintf(stderr, "ERROR: index %lld outside P\n", (long long)Pi[k]); return 1; }
  if (doA && Ai) for (c_int k = 0; k < An; k++) if (Ai[k] < 0 || Ai[k] >= nnzA) { fprintf(stderr, "ERROR: index %lld outside A\n", (long long)Ai[k]); return doP ? 2 : 1; }
  /* The reference unscales, patches and re-equilibrates from scratch (osqp.c:1046-1067).  Here
   * the unscaled problem is kept as given, patched, uploaded and re-equilibrated on the GPU. */
  csc *P = w->settings->scaling ? s->rawP : w->data->P;
  csc *A = w->settings->scaling ? s->rawA : w->data->A;
  ver_mark(w, (doP ? VER_P : 0) | (doA ? VER_A : 0));
  if (doP) {
    if (Pi) for (c_int k = 0; k < Pn; k++) P->x[Pi[k]] = Px[k];
    else    for (c_int k = 0; k < nnzP; k++) P->x[k] = Px[k];
  }
  if (doA) {
    if (Ai) for (c_int k = 0; k < An; k++) A->x[Ai[k]] = Ax[k];
    else    for (c_int k = 0; k < nnzA; k++) A->x[k] = Ax[k];
  }
  c_int rc;
  if (w->settings->scaling) {
    if (hipeng_upload_matrices(s->eng, P, A) || hipeng_upload_q(s->eng, s->rawq) ||
        hipeng_upload_bounds(s->eng, s->rawl, s->rawu) || rescale_on_device(w)) return 1;
    rc = hipeng_matrices_changed(s->eng) ? 1 : 0;
    if (s->aux && hipeng_upload_matrices(s->aux, w->data->P, w->data->A)) rc = 1;
    s->sc_iter = -1;
    /* constraint classes follow the rescaled bounds (set_rho_vec semantics are unchanged:
     * classes depend on l, u only through the 1e26 / RHO_TOL tests) */
  } else {
    rc = w->linsys_solver->update_matrices(w->linsys_solver, w->data->P, w->data->A);
  }
  info_reset(w->info);
  upd_end(w);
  return rc;
}

c_int osqp_update_P(OSQPWorkspace *w, const c_float *Px, const c_int *Pi, c_int Pn) {
  NEED_WORK(w); return patch(w, Px, Pi, Pn, 1, NULL, NULL, 0, 0);
}
c_int osqp_update_A(OSQPWorkspace *w, const c_float *Ax, const c_int *Ai, c_int An) {
  NEED_WORK(w); return patch(w, NULL, NULL, 0, 0, Ax, Ai, An, 1);
}
c_int osqp_update_P_A(OSQPWorkspace *w, const c_float *Px, const c_int *Pi, c_int Pn,
                      const c_float *Ax, const c_int *Ai, c_int An) {
  NEED_WORK(w); return patch(w, Px, Pi, Pn, 1, Ax, Ai, An, 1);
}

c_int osqp_update_rho(OSQPWorkspace *w, c_float rho_new) {   /* src/osqp.c:1281-1332 */
  NEED_WORK(w);
  if (rho_new <= 0) { fprintf(stderr, "ERROR in osqp_update_rho: rho must be positive\n"); return 1; }
  double t0 = 0;
  sens_invalidate(w);
  if (!w->rho_update_from_solve) {
    if (w->clear_update_time == 1) { w->clear_update_time = 0; w->info->update_time = 0.0; }
    t0 = now_s();
  }
  w->settings->rho = HMIN(HMAX(rho_new, RHO_MIN), RHO_MAX);
  for (c_int i = 0; i < w->data->m; i++) {
    if (w->constr_type[i] == 0) { w->rho_vec[i] = w->settings->rho; w->rho_inv_vec[i] = 1. / w->settings->rho; }
    else if (w->constr_type[i] == 1) { w->rho_vec[i] = RHO_EQ_OVER_RHO_INEQ * w->settings->rho; w->rho_inv_vec[i] = 1. / w->rho_vec[i]; }
  }
  c_int rc = w->linsys_solver->update_rho_vec(w->linsys_solver, w->rho_vec);
  if (!w->rho_update_from_solve) w->info->update_time += now_s() - t0;
  return rc;
}

/* ------------------------------------------------------------------------ */
/* settings setters (src/osqp.c:1339-1617)                                    */
/* ------------------------------------------------------------------------ */
#define SETTER(name, type, field, cond, msg)                               \
  c_int name(OSQPWorkspace *w, type v) {                                   \
    NEED_WORK(w);                                                          \
    if (!(cond)) { fprintf(stderr, "ERROR in %s: %s\n", __func__, msg); return 1; } \
    w->settings->field = v;                                                \
    return 0;                                                              \
  }
SETTER(osqp_update_max_iter, c_int, max_iter, v > 0, "max_iter must be positive")
SETTER(osqp_update_eps_abs, c_float, eps_abs, v >= 0., "eps_abs must be nonnegative")
SETTER(osqp_update_eps_rel, c_float, eps_rel, v >= 0., "eps_rel must be nonnegative")
SETTER(osqp_update_eps_prim_inf, c_float, eps_prim_inf, v >= 0., "eps_prim_inf must be nonnegative")
SETTER(osqp_update_eps_dual_inf, c_float, eps_dual_inf, v >= 0., "eps_dual_inf must be nonnegative")
SETTER(osqp_update_alpha, c_float, alpha, (v > 0. && v < 2.), "alpha must be between 0 and 2")
SETTER(osqp_update_warm_start, c_int, warm_start, (v == 0 || v == 1), "warm_start should be either 0 or 1")
SETTER(osqp_update_scaled_termination, c_int, scaled_termination, (v == 0 || v == 1), "scaled_termination should be either 0 or 1")
SETTER(osqp_update_check_termination, c_int, check_termination, v >= 0, "check_termination should be nonnegative")
c_int osqp_update_delta(OSQPWorkspace *w, c_float v) {
  NEED_WORK(w);
  if (!(v > 0.)) { fprintf(stderr, "ERROR in %s: %s\n", __func__, "delta must be positive"); return 1; }
  w->settings->delta = v;
  /* a kept KKT instance of the solution derivatives was built with the old delta: the next call builds one with the new */
  if (w->linsys_solver) sens_drop_instance(PCG(w)->sens);
  return 0;
}
SETTER(osqp_update_polish, c_int, polish, (v == 0 || v == 1), "polish should be either 0 or 1")
SETTER(osqp_update_polish_refine_iter, c_int, polish_refine_iter, v >= 0, "polish_refine_iter must be nonnegative")
SETTER(osqp_update_verbose, c_int, verbose, (v == 0 || v == 1), "verbose should be either 0 or 1")
SETTER(osqp_update_time_limit, c_float, time_limit, v >= 0., "time_limit must be nonnegative")

/* The route polish and the solution derivatives (osqp_amd_adjoint / osqp_amd_tangent) share: the active-row guess, Ared, the
 * polish-mode instance and the refined solve. */
/* active-set guess from the (z, y) the workspace holds (polish.c:19-103); p: row maps of m entries each */
static void guess_active_rows(const OSQPWorkspace *w, OSQPPolish *p) {
  const c_int m = w->data->m;
  p->n_low = p->n_upp = 0;
  for (c_int i = 0; i < m; i++) {
    if (w->z[i] - w->data->l[i] < -w->y[i]) { p->Alow_to_A[p->n_low] = i; p->A_to_Alow[i] = p->n_low++; }
    else p->A_to_Alow[i] = -1;
  }
  for (c_int i = 0; i < m; i++) {
    if (w->data->u[i] - w->z[i] < w->y[i]) { p->Aupp_to_A[p->n_upp] = i; p->A_to_Aupp[i] = p->n_upp++; }
    else p->A_to_Aupp[i] = -1;
  }
}

/* the active rows of A, lows first, then upps */
static csc *form_Ared(const OSQPWorkspace *w, const OSQPPolish *p) {
  const c_int n = w->data->n;
  const csc *A = w->data->A;
  const c_int mred = p->n_low + p->n_upp;
  c_int cnt = 0;
  for (c_int k = 0; k < A->p[n]; k++)
    if (p->A_to_Alow[A->i[k]] != -1 || p->A_to_Aupp[A->i[k]] != -1) cnt++;
  csc *Ar = (csc *)c_calloc(1, sizeof(csc));
  if (!Ar) return NULL;
  Ar->m = mred; Ar->n = n; Ar->nz = -1; Ar->nzmax = cnt > 0 ? cnt : 1;
  Ar->p = (c_int *)c_calloc((size_t)n + 1, sizeof(c_int));
  Ar->i = (c_int *)c_calloc((size_t)Ar->nzmax, sizeof(c_int));
  Ar->x = (c_float *)c_calloc((size_t)Ar->nzmax, sizeof(c_float));
  cnt = 0;
  /* a column's lows, then its upps: the reduced row indices ascend within the column whenever A's do (the resident PCG asks for
   * sorted columns and refuses the instance otherwise; in A's own order an upp row ahead of a low row breaks it) */
  for (c_int j = 0; j < n; j++) {
    Ar->p[j] = cnt;
    for (c_int k = A->p[j]; k < A->p[j + 1]; k++) {
      c_int r = A->i[k];
      if (p->A_to_Alow[r] != -1) { Ar->i[cnt] = p->A_to_Alow[r]; Ar->x[cnt++] = A->x[k]; }
    }
    for (c_int k = A->p[j]; k < A->p[j + 1]; k++) {
      c_int r = A->i[k];
      if (p->A_to_Alow[r] == -1 && p->A_to_Aupp[r] != -1) { Ar->i[cnt] = p->A_to_Aupp[r] + p->n_low; Ar->x[cnt++] = A->x[k]; }
    }
  }
  Ar->p[n] = cnt;
  return Ar;
}

/* The reference solves [P + dI, Ar'; Ar, -dI] with d = settings->delta (1e-6) by a direct factorisation and
 * refines against the unregularised KKT matrix (polish.c:134-181, 232-260).  The indirect plugin solves the
 * equivalent reduced system (P + dI + Ar'Ar/d) x = rhs1 + Ar'rhs2/d and recovers nu = (Ar x - rhs2)/d: that
 * difference loses log10(1/d) digits, and cond(K) grows like 1/d, so at d = 1e-6 nothing of nu is left.  The
 * regularisation only has to be small against the KKT matrix for the refinement to contract (error factor
 * ~ d/sigma_min per step), so the solves use d = max(delta, 1e-3) -- nu keeps ~9 digits -- and the refinement
 * runs until the true KKT residual (evaluated on the device) stops falling: same limit point, the solution of
 * the unregularised system, as the reference's 3 steps at 1e-6. */
static c_int kkt_instance(const OSQPWorkspace *w, const csc *Ar, LinSysSolver **ls) {
  const c_float delta = HMAX(w->settings->delta, POLISH_DELTA_MIN);
  return init_linsys_solver(ls, w->data->P, Ar, delta, NULL, w->settings->linsys_solver, 1);
}

/* sol = M^-1 rhs, M = [P, Ar'; Ar, 0] of the instance `ls` (N = n + mred unknowns): its regularised solve, then refinement against
 * M (polish.c:134-181) -- at least polish_refine_iter steps, at most max(polish_refine_iter, POLISH_MAX_REFINE), ended once converged
 * or no longer contracting.  res, tmp: scratch of N.  kkt_res (NULL = skip): the last |rhs - M sol|_inf / max(|rhs|_inf, 1) evaluated;
 * nsolves (NULL = skip): counts the linear solves.  Returns nonzero when a solve or a product failed. */
static c_int kkt_refined_solve(const OSQPWorkspace *w, LinSysSolver *ls, c_int mred, const c_float *rhs, c_float *sol,
                               c_float *res, c_float *tmp, c_float *kkt_res, c_int *nsolves) {
  hipeng *pe = ((hip_pcg_solver *)ls)->eng;      /* the instance's engine holds P and Ared */
  const c_int n = w->data->n, N = n + mred;
  memcpy(sol, rhs, (size_t)N * sizeof(c_float));
  c_int bad = ls->solve(ls, sol);
  if (nsolves) (*nsolves)++;
  c_float prev = OSQP_INFTY;
  const c_int max_ref = HMAX(w->settings->polish_refine_iter, POLISH_MAX_REFINE);
  for (c_int it = 0; !bad && it < max_ref; it++) {   /* polish.c:134-181 */
    /* res = rhs - [P Ar'; Ar 0] sol, SpMVs on the device */
    memcpy(res, rhs, (size_t)N * sizeof(c_float));
    bad = hipeng_spmv(pe, 2, sol, tmp);
    for (c_int j = 0; j < n; j++) res[j] -= tmp[j];
    if (!bad && mred) {
      bad = hipeng_spmv(pe, 1, sol + n, tmp);
      for (c_int j = 0; j < n; j++) res[j] -= tmp[j];
      if (!bad) bad = hipeng_spmv(pe, 0, sol, tmp);
      for (c_int k = 0; k < mred; k++) res[n + k] -= tmp[k];
    }
    if (bad) break;
    const c_float nres = absmax(res, N), scale = HMAX(absmax(rhs, N), 1.0);
    if (kkt_res) *kkt_res = nres / scale;
    /* at least the reference's polish_refine_iter steps; then stop once converged or no longer contracting */
    if (it >= w->settings->polish_refine_iter && (nres <= 1e-14 * scale || nres > 0.5 * prev)) break;
    prev = nres;
    bad = ls->solve(ls, res);
    if (nsolves) (*nsolves)++;
    for (c_int k = 0; k < N; k++) sol[k] += res[k];
  }
  return bad;
}

/* ------------------------------------------------------------------------ */
/* polish (src/polish.c:19-350) through the plugin with polish = 1            */
/* ------------------------------------------------------------------------ */
static c_int run_polish(OSQPWorkspace *w) {
  OSQPPolish *p = w->pol;
  hip_pcg_solver *s = PCG(w);
  const c_int n = w->data->n, m = w->data->m;
  tic(w->timer);
  guess_active_rows(w, p);
  const c_int mred = p->n_low + p->n_upp;
  csc *Ar = form_Ared(w, p);
  if (!Ar) { w->info->status_polish = -1; return -1; }
  p->Ared = Ar;
  LinSysSolver *ls = NULL;
  if (kkt_instance(w, Ar, &ls)) {
    w->info->status_polish = -1; free_csc(Ar); p->Ared = NULL; return 1;
  }
  const c_int N = n + mred;
  c_float *rhs = zero_vec(N), *sol = zero_vec(N), *res = zero_vec(N), *tmp = zero_vec(N);
  for (c_int j = 0; j < n; j++) rhs[j] = -w->data->q[j];
  for (c_int k = 0; k < p->n_low; k++) rhs[n + k] = w->data->l[p->Alow_to_A[k]];
  for (c_int k = 0; k < p->n_upp; k++) rhs[n + p->n_low + k] = w->data->u[p->Aupp_to_A[k]];
  const c_int bad = kkt_refined_solve(w, ls, mred, rhs, sol, res, tmp, NULL, NULL);
  if (bad) { w->info->status_polish = -1; goto cleanup; }
  memcpy(p->x, sol, (size_t)n * sizeof(c_float));
  if (m && hipeng_spmv(s->eng, 0, p->x, p->z)) { w->info->status_polish = -1; goto cleanup; }   /* z = A x on the device */
  for (c_int i = 0; i < m; i++) {
    if (mred == 0) p->y[i] = 0.0;
    else if (p->A_to_Alow[i] != -1) p->y[i] = sol[n + p->A_to_Alow[i]];
    else if (p->A_to_Aupp[i] != -1) p->y[i] = sol[n + p->n_low + p->A_to_Aupp[i]];
    else p->y[i] = 0.0;
  }
  for (c_int i = 0; i < m; i++) {   /* proj.c:16-29 */
    c_float t = p->z[i] + p->y[i];
    p->z[i] = HMIN(HMAX(t, w->data->l[i]), w->data->u[i]);
    p->y[i] = t - p->z[i];
  }
  /* residuals of the polished point, evaluated on the device */
  {
    hipeng_scalars keep = s->sc, sc;
    if (hipeng_set_iterates(s->eng, p->x, p->y) || hipeng_set_z(s->eng, p->z) ||
        hipeng_residuals(s->eng, &sc)) { w->info->status_polish = -1; goto restore; }
    p->obj_val = sc.obj_scaled * (w->settings->scaling ? w->scaling->cinv : 1.0);
    p->pri_res = m == 0 ? 0. : (use_unscaled(w) ? sc.pri_res_u : sc.pri_res_s);
    p->dua_res = use_unscaled(w) ? w->scaling->cinv * sc.dua_res_u : sc.dua_res_s;
    w->info->polish_time = toc(w->timer);
    c_int ok = (p->pri_res < w->info->pri_res && p->dua_res < w->info->dua_res) ||
               (p->pri_res < w->info->pri_res && w->info->dua_res < 1e-10) ||
               (p->dua_res < w->info->dua_res && w->info->pri_res < 1e-10);
    if (ok) {
      w->info->obj_val = p->obj_val; w->info->pri_res = p->pri_res; w->info->dua_res = p->dua_res;
      w->info->status_polish = 1;
      memcpy(w->x, p->x, (size_t)n * sizeof(c_float));
      if (m) { memcpy(w->z, p->z, (size_t)m * sizeof(c_float)); memcpy(w->y, p->y, (size_t)m * sizeof(c_float)); }
      memcpy(w->solution->x, w->x, (size_t)n * sizeof(c_float));
      if (m) memcpy(w->solution->y, w->y, (size_t)m * sizeof(c_float));
      if (w->settings->scaling) {
        for (c_int j = 0; j < n; j++) w->solution->x[j] = w->solution->x[j] * w->scaling->D[j];
        for (c_int i = 0; i < m; i++) { w->solution->y[i] = w->solution->y[i] * w->scaling->E[i]; w->solution->y[i] *= w->scaling->cinv; }
      }
      s->sc = sc;
      goto cleanup;
    }
    w->info->status_polish = -1;
    s->sc = keep;
  }
restore:   /* put the ADMM iterates back on the device */
  hipeng_set_iterates(s->eng, w->x, w->y);
  hipeng_set_z(s->eng, w->z);
cleanup:
  w->info->polish_time = toc(w->timer);
  {   /* what the instance was, for osqp_amd_polish_info: read before it goes */
    long long ri[16];
    hipeng_stats hs;
    hipeng *pe = ((hip_pcg_solver *)ls)->eng;
    const c_int known = !hipeng_resident_info(pe, ri) && !hipeng_get_stats(pe, &hs);
    s->pol_info[0]++;
    s->pol_info[1] = known ? (c_int)ri[9] : -1;
    s->pol_info[2] = mred;
    s->pol_info[3] = known ? (c_int)ri[10] + (c_int)hs.neg_curvature : -1;
  }
  ls->free(ls);
  free_csc(Ar); p->Ared = NULL;
  c_free(rhs); c_free(sol); c_free(res); c_free(tmp);
  return 0;
}

/* ------------------------------------------------------------------------ */
/* binary problem files: the data the reference's     */
/* generators emit as C headers (tests/utils/codegen_utils.py:172-347), as one */
/* little-endian file: magic "OSQPAMD1", int64 n, m, nnzP, nnzA, then          */
/* P.p[n+1] P.i[nnzP] (int64) P.x[nnzP] (f64), A.p A.i A.x, q[n] l[m] u[m].    */
/* ------------------------------------------------------------------------ */
static const char PROBLEM_MAGIC[8] = {'O', 'S', 'Q', 'P', 'A', 'M', 'D', '1'};

c_int osqp_amd_write_problem(const char *path, const OSQPData *d) {
  if (!path || check_data(d)) return 1;
  FILE *f = fopen(path, "wb");
  if (!f) return 2;
  const c_int hdr[4] = {d->n, d->m, d->P->p[d->n], d->A->p[d->n]};
  int ok = fwrite(PROBLEM_MAGIC, 1, 8, f) == 8 && fwrite(hdr, sizeof(c_int), 4, f) == 4;
  const csc *M[2] = {d->P, d->A};
  for (int k = 0; ok && k < 2; k++) {
    const size_t nnz = (size_t)M[k]->p[d->n];
    ok = fwrite(M[k]->p, sizeof(c_int), (size_t)d->n + 1, f) == (size_t)d->n + 1 &&
         fwrite(M[k]->i, sizeof(c_int), nnz, f) == nnz && fwrite(M[k]->x, sizeof(c_float), nnz, f) == nnz;
  }
  ok = ok && fwrite(d->q, sizeof(c_float), (size_t)d->n, f) == (size_t)d->n &&
       fwrite(d->l, sizeof(c_float), (size_t)d->m, f) == (size_t)d->m &&
       fwrite(d->u, sizeof(c_float), (size_t)d->m, f) == (size_t)d->m;
  fclose(f);
  return ok ? 0 : 3;
}

void osqp_amd_free_problem(OSQPData *d) {
  if (!d) return;
  free_csc(d->P); free_csc(d->A);
  c_free(d->q); c_free(d->l); c_free(d->u); c_free(d);
}

c_int osqp_amd_read_problem(const char *path, OSQPData **out) {
  if (!path || !out) return 1;
  *out = NULL;
  FILE *f = fopen(path, "rb");
  if (!f) return 2;
  char magic[8];
  c_int hdr[4];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, PROBLEM_MAGIC, 8) || fread(hdr, sizeof(c_int), 4, f) != 4 ||
      hdr[0] <= 0 || hdr[1] < 0 || hdr[2] < 0 || hdr[3] < 0) { fclose(f); return 3; }
  OSQPData *d = (OSQPData *)c_calloc(1, sizeof(OSQPData));
  if (!d) { fclose(f); return 4; }
  d->n = hdr[0]; d->m = hdr[1];
  int ok = 1;
  for (int k = 0; ok && k < 2; k++) {
    const c_int nnz = hdr[2 + k];
    csc *M = (csc *)c_calloc(1, sizeof(csc));
    if (!M) { ok = 0; break; }
    if (k == 0) d->P = M; else d->A = M;
    M->m = k == 0 ? d->n : d->m; M->n = d->n; M->nz = -1; M->nzmax = nnz > 0 ? nnz : 1;
    M->p = (c_int *)c_malloc(((size_t)d->n + 1) * sizeof(c_int));
    M->i = (c_int *)c_malloc((size_t)M->nzmax * sizeof(c_int));
    M->x = (c_float *)c_malloc((size_t)M->nzmax * sizeof(c_float));
    ok = M->p && M->i && M->x && fread(M->p, sizeof(c_int), (size_t)d->n + 1, f) == (size_t)d->n + 1 &&
         fread(M->i, sizeof(c_int), (size_t)nnz, f) == (size_t)nnz &&
         fread(M->x, sizeof(c_float), (size_t)nnz, f) == (size_t)nnz && M->p[d->n] == nnz;
  }
  d->q = zero_vec(d->n); d->l = zero_vec(d->m); d->u = zero_vec(d->m);
  ok = ok && d->q && d->l && d->u && fread(d->q, sizeof(c_float), (size_t)d->n, f) == (size_t)d->n &&
       fread(d->l, sizeof(c_float), (size_t)d->m, f) == (size_t)d->m &&
       fread(d->u, sizeof(c_float), (size_t)d->m, f) == (size_t)d->m;
  fclose(f);
  if (!ok || check_data(d)) { osqp_amd_free_problem(d); return 3; }
  *out = d;
  return 0;
}

/* ------------------------------------------------------------------------ */
/* engine access for tests / bench                                            */
/* ------------------------------------------------------------------------ */
c_int osqp_amd_get_stats(const OSQPWorkspace *w, osqp_amd_stats *out) {
  if (!w || !w->linsys_solver || !out) return 1;
  hip_pcg_solver *s = PCG(w);
  hipeng_stats hs;
  if (hipeng_get_stats(s->eng, &hs)) return 1;
  out->pcg_iters_total = hs.pcg_iters_total; out->pcg_iters_last = hs.pcg_iters_last;
  out->pcg_forced = hs.pcg_forced; out->graph_launches = hs.graph_launches;
  out->host_syncs = s->host_syncs;
  out->resident = hs.resident;
  return 0;
}

/* ------------------------------------------------------------------------ */
/* derivatives of the solution (include/osqp_amd.h): polish's route with      */
/* another right-hand side, then O(nnz) work on the device (csrc/kkt_sens.h)  */
/* ------------------------------------------------------------------------ */
static void fill_zero(c_float *v, c_int k) { if (v && k > 0) memset(v, 0, (size_t)k * sizeof(c_float)); }
static c_int all_finite(const c_float *v, c_int k) {
  for (c_int q = 0; q < k; q++) if (!isfinite(v[q])) return 0;
  return 1;
}

/* the workspace's state and instance for a derivative call: 0 ready, -1 a failure (status -1), or an OSQP error code to return */
static c_int sens_prepare(OSQPWorkspace *w, const char *who) {
  hip_pcg_solver *s = PCG(w);
  const c_int n = w->data->n, m = w->data->m;
  sens_state *ss = s->sens;
  if (!ss) {
    const size_t mm = (size_t)(m > 0 ? m : 1);
    ss = (sens_state *)c_calloc(1, sizeof(sens_state));
    if (!ss) return -1;
    s->sens = ss;
    ss->pol.Alow_to_A = (c_int *)c_malloc(mm * sizeof(c_int)); ss->pol.Aupp_to_A = (c_int *)c_malloc(mm * sizeof(c_int));
    ss->pol.A_to_Alow = (c_int *)c_malloc(mm * sizeof(c_int)); ss->pol.A_to_Aupp = (c_int *)c_malloc(mm * sizeof(c_int));
    ss->act = (c_int *)c_calloc(mm, sizeof(c_int));
    ss->yact = zero_vec(m); ss->rnu = zero_vec(m);
    ss->rhs = zero_vec(n + m); ss->sol = zero_vec(n + m); ss->res = zero_vec(n + m); ss->tmp = zero_vec(n + m);
    if (!ss->pol.Alow_to_A || !ss->pol.Aupp_to_A || !ss->pol.A_to_Alow || !ss->pol.A_to_Aupp || !ss->act || !ss->yact ||
        !ss->rnu || !ss->rhs || !ss->sol || !ss->res || !ss->tmp) { sens_free(ss); s->sens = NULL; return -1; }
  }
  if (ss->ls) return 0;
  /* one instance per solved problem: the active rows of the point the workspace holds (scaled z, y, l, u), Ared, the instance */
  OSQPPolish *p = &ss->pol;
  guess_active_rows(w, p);
  ss->Ared = form_Ared(w, p);
  if (!ss->Ared) return -1;
  if (kkt_instance(w, ss->Ared, &ss->ls)) { ss->ls = NULL; sens_drop_instance(ss); return -1; }
  /* the kernels run on the instance's stream, so their arrays live on the instance's device */
  const c_int device = ((hip_pcg_solver *)ss->ls)->opt.device;
  if (ss->dev && ss->dev_device != device) { hipsens_destroy(ss->dev); ss->dev = NULL; }
  if (!ss->dev) {
    if (hipsens_create(&ss->dev, n, m, w->data->P->p[n], w->data->A->p[n], (int)device)) {
      fprintf(stderr, "ERROR in %s: device set-up failed\n", who);
      hipsens_destroy(ss->dev); ss->dev = NULL;
      sens_drop_instance(ss);
      return -1;
    }
    ss->dev_device = device;
  }
  for (c_int i = 0; i < m; i++) {
    ss->act[i] = p->A_to_Alow[i] != -1 ? -1 : (p->A_to_Aupp[i] != -1 ? 1 : 0);
    ss->yact[i] = ss->act[i] ? w->y[i] : 0.0;
  }
  const OSQPScaling *sc = w->settings->scaling ? w->scaling : NULL;
  if (hipsens_set_point(ss->dev, ((hip_pcg_solver *)ss->ls)->eng, w->x, ss->yact, ss->act, sc ? sc->D : NULL, sc ? sc->E : NULL,
                        sc ? sc->c : 1.0)) { sens_drop_instance(ss); return -1; }
  ss->built++;
  return 0;
}

/* position of row i among the instance's unknowns behind x (lows first, then upps), -1: inactive */
static c_int sens_slot(const OSQPPolish *p, c_int i) {
  if (p->A_to_Alow[i] != -1) return p->A_to_Alow[i];
  if (p->A_to_Aupp[i] != -1) return p->n_low + p->A_to_Aupp[i];
  return -1;
}

/* the refined solve of ss->rhs into ss->sol; nonzero: a solve failed, met negative curvature or gave a non-finite value */
static c_int sens_solve(const OSQPWorkspace *w, sens_state *ss, c_float *kkt_res) {
  const c_int mred = ss->pol.n_low + ss->pol.n_upp;
  hipeng_stats hs;
  c_float r = 0.0;
  if (kkt_refined_solve(w, ss->ls, mred, ss->rhs, ss->sol, ss->res, ss->tmp, &r, &ss->solves)) return 1;
  if (hipeng_get_stats(((hip_pcg_solver *)ss->ls)->eng, &hs) || hs.neg_curvature > 0) return 1;
  if (!all_finite(ss->sol, w->data->n + mred) || !isfinite(r)) return 1;
  if (kkt_res) *kkt_res = r;
  return 0;
}

#define SENS_ENTRY(w, who)                                                                                       \
  NEED_WORK(w);                                                                                                  \
  if (!(w)->linsys_solver || !PCG(w)->sens_ready) {                                                              \
    fprintf(stderr, "ERROR in %s: no osqp_solve since setup or since the last update or warm start\n", who);     \
    return OSQP_WORKSPACE_NOT_INIT_ERROR;                                                                        \
  }

c_int osqp_amd_adjoint(OSQPWorkspace *w, const c_float *dx, const c_float *dy, c_float *dq, c_float *dl, c_float *du,
                       c_float *dPx, c_float *dAx, c_int *active, c_int *status, c_float *kkt_res) {
  SENS_ENTRY(w, "osqp_amd_adjoint");
  const c_int n = w->data->n, m = w->data->m;
  if (!dx || !dq || !status || (m > 0 && (!dl || !du))) {
    fprintf(stderr, "ERROR in osqp_amd_adjoint: missing argument\n");
    return OSQP_DATA_VALIDATION_ERROR;
  }
  const c_int nnzP = w->data->P->p[n], nnzA = w->data->A->p[n];
  fill_zero(dq, n); fill_zero(dl, m); fill_zero(du, m); fill_zero(dPx, nnzP); fill_zero(dAx, nnzA);
  if (active) for (c_int i = 0; i < m; i++) active[i] = 0;
  if (kkt_res) *kkt_res = 0.0;
  *status = 0;
  if (w->info->status_val != OSQP_SOLVED) return 0;
  *status = -1;
  if (sens_prepare(w, "osqp_amd_adjoint")) return 0;
  sens_state *ss = PCG(w)->sens;
  const OSQPPolish *p = &ss->pol;
  const OSQPScaling *sc = w->settings->scaling ? w->scaling : NULL;
  const c_float cs = sc ? sc->c : 1.0, cinv = 1.0 / cs;
  const c_int mred = p->n_low + p->n_upp;
  /* rhs = [D gx; E gy / c on the active rows] */
  for (c_int j = 0; j < n; j++) ss->rhs[j] = (sc ? sc->D[j] : 1.0) * dx[j];
  for (c_int a = 0; a < mred; a++) {
    const c_int r = a < p->n_low ? p->Alow_to_A[a] : p->Aupp_to_A[a - p->n_low];
    ss->rhs[n + a] = dy ? ((sc ? sc->E[r] : 1.0) * dy[r]) * cinv : 0.0;
  }
  c_float kr = 0.0;
  if (sens_solve(w, ss, &kr)) return 0;
  /* sol = [rx; rnu] of the scaled problem */
  for (c_int i = 0; i < m; i++) { const c_int a = sens_slot(p, i); ss->rnu[i] = a >= 0 ? ss->sol[n + a] : 0.0; }
  if ((dPx || dAx) && hipsens_grad(ss->dev, ((hip_pcg_solver *)ss->ls)->eng, w->data->P, w->data->A, ss->sol, ss->rnu, dPx, dAx)) {
    fill_zero(dPx, nnzP); fill_zero(dAx, nnzA);
    return 0;
  }
  if ((dPx && !all_finite(dPx, nnzP)) || (dAx && !all_finite(dAx, nnzA))) { fill_zero(dPx, nnzP); fill_zero(dAx, nnzA); return 0; }
  for (c_int j = 0; j < n; j++) dq[j] = 0.0 - (cs * (sc ? sc->D[j] : 1.0)) * ss->sol[j];
  for (c_int i = 0; i < m; i++) {
    const c_float v = ss->act[i] ? (sc ? sc->E[i] : 1.0) * ss->rnu[i] : 0.0;
    dl[i] = ss->act[i] < 0 ? v : 0.0;
    du[i] = ss->act[i] > 0 ? v : 0.0;
    if (active) active[i] = ss->act[i];
  }
  if (kkt_res) *kkt_res = kr;
  *status = 1;
  return 0;
}

c_int osqp_amd_tangent(OSQPWorkspace *w, c_int ndir, const c_float *dq, const c_float *dl, const c_float *du,
                       const c_float *dPx, const c_float *dAx, c_float *dx, c_float *dy, c_int *active, c_int *status,
                       c_float *kkt_res) {
  SENS_ENTRY(w, "osqp_amd_tangent");
  const c_int n = w->data->n, m = w->data->m;
  if (!dx || !status || ndir < 1 || ndir > OSQP_AMD_MAX_NDIR) {
    fprintf(stderr, "ERROR in osqp_amd_tangent: %s\n", !dx || !status ? "missing argument" : "ndir must be in [1, 65535]");
    return OSQP_DATA_VALIDATION_ERROR;
  }
  fill_zero(dx, ndir * n); fill_zero(dy, ndir * m); fill_zero(kkt_res, ndir);
  if (active) for (c_int i = 0; i < m; i++) active[i] = 0;
  *status = 0;
  if (w->info->status_val != OSQP_SOLVED) return 0;
  *status = -1;
  if (sens_prepare(w, "osqp_amd_tangent")) return 0;
  sens_state *ss = PCG(w)->sens;
  const OSQPPolish *p = &ss->pol;
  const OSQPScaling *sc = w->settings->scaling ? w->scaling : NULL;
  const c_float cinv = 1.0 / (sc ? sc->c : 1.0);
  const c_int mred = p->n_low + p->n_upp;
  /* the right-hand sides of all directions in one launch: g [ndir][n + m], the row part on all m rows */
  c_float *g = (c_float *)c_malloc((size_t)ndir * (size_t)(n + m) * sizeof(c_float));
  if (!g) return 0;
  c_int bad = hipsens_tan_rhs(ss->dev, ((hip_pcg_solver *)ss->ls)->eng, w->data->P, w->data->A, ndir, dq, dl, du, dPx, dAx, g) ? 1 : 0;
  for (c_int d = 0; !bad && d < ndir; d++) {
    const c_float *gd = g + d * (n + m);
    memcpy(ss->rhs, gd, (size_t)n * sizeof(c_float));
    for (c_int a = 0; a < mred; a++) ss->rhs[n + a] = gd[n + (a < p->n_low ? p->Alow_to_A[a] : p->Aupp_to_A[a - p->n_low])];
    if (!all_finite(ss->rhs, n + mred) || sens_solve(w, ss, kkt_res ? kkt_res + d : NULL)) { bad = 1; break; }
    /* sol = [dx~; dnu~] of the scaled problem */
    for (c_int j = 0; j < n; j++) dx[d * n + j] = (sc ? sc->D[j] : 1.0) * ss->sol[j];
    if (dy) for (c_int i = 0; i < m; i++) {
      const c_int a = sens_slot(p, i);
      dy[d * m + i] = a >= 0 ? ((sc ? sc->E[i] : 1.0) * ss->sol[n + a]) * cinv : 0.0;
    }
  }
  c_free(g);
  if (bad) { fill_zero(dx, ndir * n); fill_zero(dy, ndir * m); fill_zero(kkt_res, ndir); return 0; }
  if (active) for (c_int i = 0; i < m; i++) active[i] = ss->act[i];
  *status = 1;
  return 0;
}

c_int osqp_amd_sens_info(OSQPWorkspace *w, c_int out[4]) {
  NEED_WORK(w);
  if (!w->linsys_solver || !out) return OSQP_DATA_VALIDATION_ERROR;
  const sens_state *ss = PCG(w)->sens;
  out[0] = ss ? ss->built : 0;
  out[1] = ss && ss->ls ? 1 : 0;
  out[2] = ss && ss->ls ? ss->pol.n_low + ss->pol.n_upp : 0;
  out[3] = ss ? ss->solves : 0;
  return 0;
}

/* ------------------------------------------------------------------------ */
/* osqp_amd_verify (include/osqp_amd.h): a point against the raw problem, on   */
/* the device (csrc/verify.h).  Reads the workspace, writes nothing of it.     */
/* ------------------------------------------------------------------------ */
c_int osqp_amd_verify(OSQPWorkspace *w, const c_float *x, const c_float *y, const c_float *dx, const c_float *dy,
                      c_float eps_abs, c_float eps_rel, c_float V[16]) {
  NEED_WORK(w);
  if (!w->linsys_solver || !PCG(w)->eng) {
    fprintf(stderr, "ERROR in osqp_amd_verify: the workspace has no engine\n");
    return OSQP_WORKSPACE_NOT_INIT_ERROR;
  }
  if (!V || !isfinite(eps_abs) || !isfinite(eps_rel)) {
    fprintf(stderr, "ERROR in osqp_amd_verify: %s\n", !V ? "missing argument" : "eps_abs and eps_rel must be finite");
    return OSQP_DATA_VALIDATION_ERROR;
  }
  hip_pcg_solver *s = PCG(w);
  int rc = 0;
  if (!s->ver) {
    rc = hipver_create(&s->ver, w->data->P, w->data->A, (int)s->opt.device);
    if (rc) { hipver_destroy(s->ver); s->ver = NULL; }
    s->ver_stale = VER_ALL;
  }
  /* the raw problem as the caller last gave it: the copies kept beside the scaled data, or the data itself */
  const c_int raw = w->settings->scaling != 0;
  if (!rc && s->ver_stale) {
    rc = hipver_upload(s->ver, s->eng, (int)s->ver_stale, raw ? s->rawP->x : w->data->P->x, raw ? s->rawA->x : w->data->A->x,
                       raw ? s->rawq : w->data->q, raw ? s->rawl : w->data->l, raw ? s->rawu : w->data->u);
    if (!rc) s->ver_stale = 0;
  }
  if (!rc)
    rc = hipver_run(s->ver, s->eng, x ? x : w->solution->x, y ? y : w->solution->y, dx ? dx : w->delta_x, dy ? dy : w->delta_y,
                    eps_abs < 0 ? w->settings->eps_abs : eps_abs, eps_rel < 0 ? w->settings->eps_rel : eps_rel,
                    w->settings->eps_prim_inf, w->settings->eps_dual_inf, V);
  if (rc == HIPENG_ERR_ALLOC) return OSQP_MEM_ALLOC_ERROR;
  if (rc) return HIPENG_ERR_HIP;
  s->ver_calls++;
  return 0;
}

c_int osqp_amd_verify_info(OSQPWorkspace *w, c_int out[4]) {
  NEED_WORK(w);
  if (!w->linsys_solver || !PCG(w)->eng) return OSQP_WORKSPACE_NOT_INIT_ERROR;
  if (!out) return OSQP_DATA_VALIDATION_ERROR;
  out[0] = PCG(w)->ver_calls; out[1] = out[2] = out[3] = 0;
  if (PCG(w)->ver) hipver_uploads(PCG(w)->ver, out + 1);
  return 0;
}

c_int osqp_amd_polish_info(OSQPWorkspace *w, c_int out[4]) {
  NEED_WORK(w);
  if (!w->linsys_solver || !out) return OSQP_DATA_VALIDATION_ERROR;
  const hip_pcg_solver *s = PCG(w);
  out[0] = s->pol_info[0];
  out[1] = s->pol_info[0] ? s->pol_info[1] : -1;
  out[2] = s->pol_info[2];
  out[3] = s->pol_info[3];
  return 0;
}

/* per-workspace engine options (device excluded: the engine lives where it was created) */
c_int osqp_amd_get_workspace_options(const OSQPWorkspace *w, osqp_amd_options *o) {
  if (!w || !w->linsys_solver || !o) return 1;
  *o = PCG(w)->opt;
  return 0;
}
c_int osqp_amd_set_workspace_options(OSQPWorkspace *w, const osqp_amd_options *o) {
  if (!w || !w->linsys_solver || !o) return 1;
  const c_int dev = PCG(w)->opt.device;
  PCG(w)->opt = *o;
  PCG(w)->opt.device = dev;
  return 0;
}

void *osqp_amd_engine(const OSQPWorkspace *w) {
  if (!w || !w->linsys_solver) return NULL;
  return PCG(w)->eng;
}

void *osqp_amd_sens_engine(const OSQPWorkspace *w) {
  if (!w || !w->linsys_solver) return NULL;
  const sens_state *ss = PCG(w)->sens;
  return ss && ss->ls ? ((hip_pcg_solver *)ss->ls)->eng : NULL;
}
