// engine_hooks.h -- included by engine.hip after hipeng_kkt_solve, behind everything else of the engine itself.
// Entry points for tests and measurements, none of them on the solve path: hipeng_spmv / hipeng_spmv_dev, hipeng_time_kernel,
// hipeng_resident_plan / hipeng_resident_plan_lists, hipeng_switch_row / hipeng_switch_values, hipeng_timeline (TIMELINE builds),
// the *_info / *_peek / *_dump hooks and hipeng_kernel_bytes.

// ---- kernel-level entry points for tests and the roofline measurement -------
extern "C" int hipeng_spmv(hipeng *e, int which, const c_float *x, c_float *y) {
  if (!e || !x || !y || which < 0 || which > 2) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n, m = e->m;
  double *in = e->c.pt0, *out = e->c.pt1;   // scratch of n+m doubles each
  HIPCHK(hipMemsetAsync(in, 0, (size_t)std::max(1, n + m) * sizeof(double), e->stream));
  // A x from x in [0, n); A' y (selector 2) from y behind n unused slots, P x (selector 1) from x in [0, n), both through the fused rows of M
  if (which == 1 ? upload_vec(e, in + n, x, m) : upload_vec(e, in, x, n)) return HIPENG_ERR_HIP;
  if (which == 0) launch_spmv(e, e->c.A, in, out, 0);
  else launch_spmv(e, e->c.M, in, out, which == 1 ? 2 : 1);
  HIPCHK(hipMemcpyAsync(y, out, (size_t)(which == 0 ? m : n) * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// Device-to-device SpMV with the engine's matrices (which as in hipeng_spmv), on the engine's stream, no sync:
// the building block of the row-partitioned multi-GPU variant (osqp_amd/rowpart.py), whose vectors live in
// torch tensors.  d_x / d_y are device pointers of n (A x: in, A' y / P x: out) or m doubles.
extern "C" int hipeng_spmv_dev(hipeng *e, int which, const double *d_x, double *d_y) {
  if (!e || !d_x || !d_y || which < 0 || which > 2) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  const int n = e->n, m = e->m;
  if (which == 0) {
    if (m > 0) launch_spmv(e, e->c.A, d_x, d_y, 0);
  } else {
    // the fused row matrix reads y at column ids n + i: stage it behind n unused slots.  x is staged too: k_spmv stages the products of whole
    // rows of [P | A'] (the A' entries gather at column ids up to n + m - 1) before it sums the P part, so the input must be n + m long
    double *in = e->c.pt0;
    if (which == 2 || m > 0) HIPCHK(hipMemcpyAsync(which == 1 ? in + n : in, d_x, (size_t)(which == 1 ? m : n) * sizeof(double), hipMemcpyDeviceToDevice, e->stream));
    launch_spmv(e, e->c.M, in, d_y, which == 1 ? 2 : 1);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

extern "C" int hipeng_time_kernel(hipeng *e, int which, int reps, double *usec) {
  if (!e || !usec || reps <= 0 || which < 0 || which > 8) return HIPENG_ERR_ARG;
  if (which == 8 && !e->resident_available()) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  CuLease lease;
  if (which == 8 && e->one_launch()) lease.take(e->device, e->res_cus, e->one_launch_grid());
  auto one = [&](int it) {
    // the first two kernels of a resident ADMM iteration: right-hand side + start residual, then the whole linear solve
    // (without k_admm_finalize the iterates do not move: every repetition solves the same system from the same start)
    if (which == 8) { launch_init(e, 1, true); launch_resident(e); return; }
    if (which == 5) { launch_init(e, 1); return; }   // first kernel of an ADMM iteration
    if (which == 6) { launch_pcg_iter(e, it, 4); return; }   // one whole PCG iteration (all its launches, in loop order)

    if (which == 7) { hipLaunchKernelGGL(k_fill, dim3(1), dim3(TB), 0, e->stream, e->c.cvec, 0.0, 0); return; }   // empty dependent launch
    if (which == 0) launch_cg_A(e, it, 4);
    else if (which == 3) launch_cg_A(e, it, 4 | 16);
    else if (which == 4) launch_cg_A(e, it, 4 | 32);
    else launch_cg_B(e, it, 4);
  };
  // the launches are captured into one graph so the measurement is not bound by
  // the host's eager launch rate (~3-4 us per launch)
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
  for (int i = 0; i < reps; i++) one(i);
  HIPCHK(hipStreamEndCapture(e->stream, &g));
  HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  HIPCHK(hipGraphDestroy(g));
  HIPCHK(hipGraphLaunch(ge, e->stream));            // warm-up replay
  HIPCHK(hipEventRecord(e->ev0, e->stream));
  HIPCHK(hipGraphLaunch(ge, e->stream));
  HIPCHK(hipEventRecord(e->ev1, e->stream));
  HIPCHK(hipEventSynchronize(e->ev1));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
  HIPCHK(hipGraphExecDestroy(ge));
  *usec = 1e3 * (double)ms / reps;
  if (which == 8) {
    // a resident launch of the timed run may have given up: the number is void then; leave the engine as the run loop would
    State s;
    if (read_state(e, &s)) return HIPENG_ERR_HIP;
    if (s.res_fail) {
      if (resident_gave_up(e, s, false)) return HIPENG_ERR_HIP;
      return HIPENG_ERR_HIP;
    }
  }
  return 0;
}

// For the CPU tests (no device needed): the host side of the resident PCG set-up -- symbolic K, row partition, positions
// in the exchanged vector, register layout -- for a machine of `nwg` CUs.  stats: [0] the problem qualifies, [1] entries of K
// per thread, [2] length of the exchanged vector, [3] nnz(K), [4] workgroups that own rows, [5] most rows per workgroup,
// [6] most entries per workgroup, [7] 448.  Optional outputs (NULL to skip): Kptr (n + 1), Kcol / kdst (cap entries at most:
// column and register slot of every entry of K, row by row), rowpos (n), slotcol (nwg * E * 448: the position held in every
// slot), wg4 (4 ints per workgroup: first row, rows, entries, first position).
extern "C" int hipeng_resident_plan(const csc *P, const csc *A, int nwg, long long stats[8], int *Kptr, int *Kcol, int *kdst, long long cap,
                                    unsigned short *rowpos, unsigned short *slotcol, int *wg4) {
  if (!P || !A || !stats || P->n > 0x7ffffff0LL || A->m > 0x7ffffff0LL) return HIPENG_ERR_ARG;
  hipeng tmp;
  tmp.n = (int)P->n; tmp.m = (int)A->m;
  build_A(&tmp, A); build_M(&tmp, P, A); build_dense(&tmp, P);
  ResPlanOut po;
  const int rc = build_resident(&tmp, nwg, &po);
  for (int k = 0; k < 8; k++) stats[k] = 0;
  if (rc) return rc;
  stats[0] = po.ok; stats[7] = RES_PT;
  if (!po.ok) return 0;
  stats[1] = po.E; stats[2] = po.npad; stats[3] = po.nnzK;
  for (const ResWG &w : po.wg) { if (w.nr) stats[4]++; stats[5] = std::max<long long>(stats[5], w.nr); stats[6] = std::max<long long>(stats[6], w.cnt); }
  if (Kptr) std::copy(po.Kptr.begin(), po.Kptr.end(), Kptr);
  if (po.nnzK <= cap) { if (Kcol) std::copy(po.Kcol.begin(), po.Kcol.end(), Kcol); if (kdst) std::copy(po.kdst.begin(), po.kdst.end(), kdst); }
  else if (Kcol || kdst) return HIPENG_ERR_ARG;
  if (rowpos) std::copy(po.rowpos.begin(), po.rowpos.end(), rowpos);
  if (slotcol) std::copy(po.col.begin(), po.col.end(), slotcol);
  if (wg4) for (size_t g = 0; g < po.wg.size(); g++) { wg4[4 * g] = po.wg[g].r0; wg4[4 * g + 1] = po.wg[g].nr; wg4[4 * g + 2] = po.wg[g].cnt; wg4[4 * g + 3] = po.wg[g].pos; }
  return 0;
}

// The contribution lists of that plan (k_form_K_lists), for the CPU tests: Kcp (nnz(K) + 1 offsets, entries in the order of the
// plan's Kcol), Kcm / Kca (slot in M of a_ki, slot in the CSR copy of A of a_kj; cap terms at most).  Outputs may be NULL.
// Returns the number of terms, -1 when the problem does not qualify for the resident PCG, -2 when it does but the lists are
// switched off or over their budget (OSQP_AMD_FORM_K_LISTS, OSQP_AMD_FORM_K_LIST_MB), or a HIPENG_ERR_* code.
extern "C" long long hipeng_resident_plan_lists(const csc *P, const csc *A, int nwg, int *Kcp, int *Kcm, int *Kca, long long cap) {
  if (!P || !A || P->n > 0x7ffffff0LL || A->m > 0x7ffffff0LL) return HIPENG_ERR_ARG;
  hipeng tmp;
  tmp.n = (int)P->n; tmp.m = (int)A->m;
  build_A(&tmp, A); build_M(&tmp, P, A); build_dense(&tmp, P);
  ResPlanOut po;
  if (const int rc = build_resident(&tmp, nwg, &po)) return rc;
  if (!po.ok) return -1;
  if (!po.lists) return -2;
  const long long terms = (long long)po.Kcm.size();
  if (Kcp) std::copy(po.Kcp.begin(), po.Kcp.end(), Kcp);
  if (terms <= cap) { if (Kcm) std::copy(po.Kcm.begin(), po.Kcm.end(), Kcm); if (Kca) std::copy(po.Kca.begin(), po.Kca.end(), Kca); }
  else if (Kcm || Kca) return HIPENG_ERR_ARG;
  return terms;
}

// The switch table from outside, for the tests and the documentation check (no device, no HIP call).  Row `index` of SW_TABLE: its name,
// kind (SwKind), default as text ("unset" where unset is distinct: the use site works it out), that bit, and the one-line description;
// outputs may be NULL.  Returns the number of rows, whatever the index.
extern "C" int hipeng_switch_row(int index, const char **name, int *kind, char *def_text, int def_cap, int *unset_distinct, const char **what) {
  if (index < 0 || index >= SW_COUNT) return SW_COUNT;
  const SwRow &r = SW_TABLE[index];
  if (name) *name = r.name;
  if (kind) *kind = r.kind;
  if (unset_distinct) *unset_distinct = r.unset_distinct;
  if (what) *what = r.what;
  if (def_text && def_cap > 0) {
    if (r.unset_distinct) snprintf(def_text, (size_t)def_cap, "unset");
    else if (r.kind == SW_TEXT) def_text[0] = 0;
    else if (r.kind == SW_INT_PAIR) snprintf(def_text, (size_t)def_cap, "%d,%d", (int)r.def, (int)r.def2);
    else if (r.kind == SW_DOUBLE) snprintf(def_text, (size_t)def_cap, "%g", r.def);
    else snprintf(def_text, (size_t)def_cap, "%d", (int)r.def);
  }
  return SW_COUNT;
}
// What read_switches() makes of the current environment: two doubles per row, rows at most of them (out[2 i]: the value -- SW_UNSET where
// unset is distinct and the variable is not set, the length of a text; out[2 i + 1]: the second number of a pair, else 0).  Returns the number of rows.
extern "C" int hipeng_switch_values(double *out, int rows) {
  if (!out) return SW_COUNT;
  const Switches sw = read_switches();
  for (int i = 0; i < std::min(rows, SW_COUNT); i++) {
    const SwRow &r = SW_TABLE[i];
    const char *at = reinterpret_cast<const char *>(&sw) + r.field;
    const int *iv = reinterpret_cast<const int *>(at);
    out[2 * i + 1] = r.kind == SW_INT_PAIR ? (double)iv[1] : 0.0;
    out[2 * i] = r.kind == SW_TEXT ? (double)strlen(at) : r.kind == SW_DOUBLE ? *reinterpret_cast<const double *>(at) : (double)iv[0];
  }
  return SW_COUNT;
}

#ifdef OSQP_AMD_TIMELINE
// make TIMELINE=1 builds only: copy out (and reset) the kernel start marks; returns their number
extern "C" long long hipeng_timeline(hipeng *e, unsigned long long *out, long long cap) {
  if (!e || !out) return -1;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return -1;
  unsigned long long cnt = 0;
  if (hipMemcpy(&cnt, e->c.tl, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  const long long k = (long long)std::min<unsigned long long>(std::min<unsigned long long>(cnt, TL_CAP - 2), (unsigned long long)cap);
  if (k > 0 && hipMemcpy(out, e->c.tl + 1, (size_t)k * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemset(e->c.tl, 0, sizeof(unsigned long long)) != hipSuccess) return -1;
  return k;
}
#endif

// 1 if the vector update and the operator apply of k_cg_A run as two launches (A dominated by long rows)
extern "C" int hipeng_is_split(hipeng *e) { return e && e->split ? 1 : 0; }
// For the tests: how the PCG kernels see (P, A) -- host-side fields only, nothing is launched.  out[0] dense blocks of P,
// [1] rows inside them, [2] stream blocks of A, [3] long (one-wavefront) rows of A, [4] huge rows of A, [5] huge rows folded
// into k_cg_B, [6] split, [7] A / [8] M / [9] the matrix k_cg_B streams (Mr when it exists, else M) has 16-bit column ids,
// [10] long rows of the matrix k_cg_B streams, [11] gridA, [12] gridM; the rest 0.
extern "C" int hipeng_pcg_layout(hipeng *e, long long out[16]) {
  if (!e || !out) return HIPENG_ERR_ARG;
  for (int k = 0; k < 16; k++) out[k] = 0;
  const HostMat &B = (!e->dP_blks.empty() || !e->hrows.empty()) ? e->Mr : e->M;
  out[0] = (long long)e->dP_blks.size();
  for (const DenseBlk &d : e->dP_blks) out[1] += d.b;
  out[2] = e->A.nstream; out[3] = e->A.nwave - e->A.nstream; out[4] = (long long)e->A.blk.size() - e->A.nwave;
  out[5] = (long long)e->hrows.size(); out[6] = e->split ? 1 : 0;
  out[7] = e->A.d_col16 != nullptr; out[8] = e->M.d_col16 != nullptr; out[9] = B.d_col16 != nullptr;
  out[10] = B.nwave - B.nstream; out[11] = e->c.gridA; out[12] = e->c.gridM;
  return 0;
}
extern "C" int hipeng_row_eliminated(hipeng *e, c_int i) { return e && !e->ecol.empty() && i >= 0 && i < (c_int)e->ecol.size() && e->ecol[(size_t)i] >= 0 ? 1 : 0; }
extern "C" c_int hipeng_elim_count(hipeng *e) { return e ? e->c.nelim : 0; }
// ---- for the tests: one of the per-row arrays of the elimination on the host (reads only) ----
extern "C" int hipeng_elim_peek(hipeng *e, int which, c_float *out) {
  if (!e || !out || which < 0 || which > 3 || !e->c.nelim) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  const double *src[] = {e->c.rhoe, e->c.ecoef, e->c.edinv, e->c.xte};
  HIPCHK(hipMemcpy(out, src[which], (size_t)e->m * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

// Resident PCG: out[0] structures built, [1] in use, [2] entries of K per thread, [3] workgroups, [4] nnz(K),
// [5] LDS bytes per workgroup, [6] PCG iterations of the most recent linear solve, [7] pipelined phase switched off for this K,
// [8] true-residual checks that failed since create, [9] form: 1 k_pcg_resident, 2 k_pcg_blockres,
// [10] launches that gave up waiting (the third one ends the mode for this engine)
extern "C" int hipeng_resident_info(hipeng *e, long long out[16]) {
  if (!e || !out) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  State s;
  if (read_state(e, &s)) return HIPENG_ERR_HIP;
  out[0] = e->form != FORM_STEPS; out[1] = e->resident_available(); out[2] = e->rc.E; out[3] = e->rc.nwg; out[4] = e->res_nnz; out[5] = (long long)e->res_lds;
  out[6] = std::max(s.iters[0], s.iters[1]); out[7] = s.res_pipe_off; out[8] = s.res_chk_fail; out[9] = e->form; out[10] = e->res_gave_up; out[11] = e->res_slow + s.res_slow;
  out[12] = std::max<long long>(e->res_slow_max, s.res_slow_max); out[13] = e->res_repub + s.res_repub; out[14] = e->res_fails; out[15] = 0;
  if (e->form == FORM_BLOCKRES) { out[2] = 64; out[3] = e->bc.nwg; out[4] = 0; out[5] = 0; }
  if (e->form == FORM_BLOCK_DIRECT) { out[2] = 0; out[3] = e->c.dP.nblk; out[4] = 0; out[5] = 0; out[15] = e->bd.kc; }
  if (e->form == FORM_DENSE_DIRECT) { out[2] = 0; out[3] = e->dd.na; out[4] = (long long)e->dd.nap * e->dd.nap; out[5] = e->dd_chol ? 1 : 0; out[15] = e->dd.nb2; }
  return 0;
}

// How the resident PCG forms K: out[0] 1 k_form_K_lists (contribution lists built at set-up), 0 k_form_K; [1] terms of the
// lists (sum over the rows of A of nnz^2, whether or not they were built), [2] bytes of the list arrays on the device (0: none),
// [3] their budget in bytes (OSQP_AMD_FORM_K_LIST_MB).  All 0 for an engine on another form.
extern "C" int hipeng_form_k_info(hipeng *e, long long out[4]) {
  if (!e || !out) return HIPENG_ERR_ARG;
  const bool res = e->form == FORM_RESIDENT;
  out[0] = res && e->fk_lists; out[1] = res ? e->fk_terms : 0; out[2] = res ? e->fk_bytes : 0; out[3] = res ? e->fk_budget : 0;
  return 0;
}

// k_pcg_resident since create: out[0] vector trips of its launches (start-up product, iterations, predicted / wasted trip, check),
// [1] launches that ran a solve, [2] predicted last trips whose products served the true-residual check, [3] predicted last trips
// that were not the last, [4] predicted trips switched off for the current K, [5] the switch (OSQP_AMD_RESIDENT_PREDICT), [6] solves /
// [7] misses minus hits of the current window of RES_PRED_WINDOW solves.
extern "C" int hipeng_resident_trips(hipeng *e, long long out[8]) {
  if (!e || !out) return HIPENG_ERR_ARG;
  HIPCHK(hipSetDevice(e->device));
  State s;
  if (read_state(e, &s)) return HIPENG_ERR_HIP;
  out[0] = s.res_trips; out[1] = s.res_solves; out[2] = s.res_pred_hit; out[3] = s.res_pred_miss;
  out[4] = s.res_pred_off; out[5] = e->form == FORM_RESIDENT ? e->rc.predict : 0; out[6] = s.res_pred_win[0]; out[7] = s.res_pred_win[2] - s.res_pred_win[1];
  return 0;
}

// Resident PCG, for the tests: what the start-up of the last launch summed.  Returns gridM (or a negative code); part_bb receives
// min(gridM, cap) partials of ||b||^2 as the last k_pcg_init left them, *tol2 State::tol2 as the last launch stored it.
extern "C" long long hipeng_resident_start_peek(hipeng *e, double *part_bb, long long cap, double *tol2) {
  if (!e || e->form != FORM_RESIDENT || !part_bb || !tol2 || cap < 0) return HIPENG_ERR_ARG;
  if (hipSetDevice(e->device) != hipSuccess) return HIPENG_ERR_HIP;
  State s;
  if (read_state(e, &s)) return HIPENG_ERR_HIP;       // (synchronises the stream)
  const long long cnt = std::min<long long>(e->c.gridM, cap);
  if (cnt > 0 && hipMemcpy(part_bb, e->c.part_bb, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return HIPENG_ERR_HIP;
  *tol2 = s.tol2;
  return e->c.gridM;
}

// Resident PCG, for the tests: the rows of K as the resident kernel holds them.  row/col/val receive nnz(K) triplets
// (row by row, columns ascending; values read from the slots the threads load them from); returns the count or a negative code.
extern "C" long long hipeng_resident_dump(hipeng *e, int *row, int *col, double *val, long long cap) {
  if (!e || e->form != FORM_RESIDENT || !row || !col || !val) return HIPENG_ERR_ARG;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return HIPENG_ERR_HIP;
  const ResCtx &rc = e->rc;
  const size_t slots = (size_t)rc.nwg * rc.E * RES_PT;
  const long long nnz = e->res_nnz;
  if (nnz > cap) return HIPENG_ERR_ARG;
  std::vector<double> v(slots); std::vector<int> krp(e->n + 1), kcj((size_t)nnz), kdst((size_t)nnz);
  if (hipMemcpy(v.data(), rc.val, slots * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(krp.data(), rc.krp, krp.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(kcj.data(), rc.kcj, kcj.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(kdst.data(), rc.kdst, kdst.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return HIPENG_ERR_HIP;
  long long k = 0;
  for (int i = 0; i < e->n; i++)
    for (int q = krp[i]; q < krp[i + 1]; q++) { row[k] = i; col[k] = kcj[q]; val[k] = v[kdst[q]]; k++; }
  return k;
}

extern "C" int hipeng_kernel_bytes(hipeng *e, int which, double *bytes) {
  if (!e || !bytes) return HIPENG_ERR_ARG;
  const double n = e->n, m = e->m;
  const double nnzA = (double)e->A.val.size();
  const double nnzPtriu = (double)e->P_toM_up.size();
  // device layout: fp64 values + int32 indices (12 B per stored entry), one
  // int32 row pointer per row, fp64 vectors; gathers counted once per vector
  // k_cg_A: A stream; u,w,p,s,r,Minv,x read + p,s,r,x,u written (12n); rho read, t written (2m)
  if (which == 0)      *bytes = nnzA * 12 + (m + 1) * 4 + 8 * (12 * n + 2 * m);
  // k_cg_B: [P|A'] stream; [u|t] and r read, w written.  P is counted as its stored upper
  // triangle (each stored entry serves both triangles) although the fused row
  // matrix M holds both, so the figure does not reward the expanded layout.
  else if (which == 1) *bytes = (nnzA + nnzPtriu) * 12 + (n + 1) * 4 + 8 * ((n + m) + 2 * n);
  else                 *bytes = 0;
  return 0;
}
