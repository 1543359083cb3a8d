// sfx_shard.inc -- heads sharded across ranks (included by sfx.hip; SURVEY.md §8e, config C4).
//
// Rank g owns global heads [off, off + T) of Tg; the reward weights w (Tg rows), the env and
// the replay are replicated, so every rank sees the same minibatch.  The only cross-rank data
// are GPI maxima, exchanged by the caller with all-reduce(MAX) between these calls:
//
//   sfx_shard_begin                      forward S / S1 of the local heads (+ LMS on w)
//   for r in rounds:
//     sfx_shard_td_maxima(r, X)          X[i][b][a] = max over local heads of q (guess roles)
//       all_reduce(X, MAX)
//     sfx_shard_td_update(r, X)          TD target from X, backward + Adam, post-update forward
//   sfx_shard_ver_maxima(r_last, Y)      maxima with the post-update heads
//     all_reduce(Y, MAX)
//   sfx_shard_verify(X, Y, flag)         first policy whose next actions were guessed wrong
//   (flag < Tg: more rounds, each fixes >= 1 more policy)
//   sfx_shard_select(r_last, task, key)  this rank's best (q, t, a) for the env action
//     all_reduce(key, MAX)               -> (c, a) with the reference's tie-breaking
//   sfx_shard_finish                     slot flip, step / target-sync bookkeeping
//
// The speculation is the single-GPU one (DESIGN.md §4) with the GPI reduction split across
// ranks; max is exact and order-free, so every rank derives identical next actions and flags.

namespace {

int shard_fail_inactive(sfx_handle* h) {
  if (!h->spend.active) SFX_FAIL(SFX_E_STATE, "sfx_shard_*: no step begun (sfx_shard_begin)");
  return SFX_OK;
}

// ---- the sharded all-task env step as one stream of launches (the native runner's "sharded"
// schedule): every collective is coll_max on h->stream, so with RCCL the whole step, all-reduces
// included, is captured into one graph.  p: the step's staged inputs (runner_pending).
//
// Maxima buffers (sortable int32): xb[0], xb[1] = [Tg][B][A] body ++ [Tg][A] selection table.
// Round r's TD target reads xb[r & 1]; its post-update forward fills xb[(r + 1) & 1] = the maxima
// round r + 1 would use, which are also round r's verification maxima.  With shard_fused (d | 16)
// those maxima come out of the ψ output layer's forward tiles (q_accumulate): round 0's from the
// step's forward of S1 (which also keeps the pre-step part xge), later rounds' from the
// post-update forward; otherwise from k_qmax launches.

bool shard_fused(const sfx_handle* h, int B) {
  return h->shard_qa && 16 % h->d == 0 && can_fuse_tdg(h) && h->A <= 32 && (long)h->Tg * h->d <= QA_WMAX &&
         can_fuse_v0(h, B + 1);
}

int shard_qmax(sfx_handle* h, int B, int guess, int* X) {
  const int TA = h->T * h->A;
  QmaxArgs Q{};
  Q.M = B;
  Q.Tg = h->Tg;
  Q.off = h->off;
  Q.guess = guess;
  Q.rows = TA >= 256 ? 1 : std::min(B, 256 / TA);
  Q.pol0 = 0;
  Q.tsel = -1;
  Q.X = X;
  const double by = 4.0 * (double)h->Tg * B * (TA * h->d + h->A) + 4.0 * h->Tg * h->d;
  if (wide_gpi(h))
    launch(h, K_VER, by, SFX_WIDE(k_qmaxw), dim3(B, cdiv(h->Tg, WPC)), dim3(256), h->G, Q);
  else
    launch(h, K_VER, by, k_qmax, dim3(h->Tg, cdiv(B, Q.rows)), dim3(256), h->G, Q);
  LAUNCHCHK();
  return SFX_OK;
}

size_t shard_body(const sfx_handle* h, int B) { return (size_t)h->Tg * B * h->A; }

// LMS on w[lms_task] and the forwards of the step's states; fused: round 0's maxima (xb[0]) and
// the pre-step part (xge) -- both SORT_EMPTY-filled by the step's gate -- or, without a minibatch,
// the selection table; then round 0's all-reduce
int shard_begin_body(sfx_handle* h, const sfx_handle::Pending& p, int lms_task, const float* lms_phi,
                     const float* lms_r, float lms_alpha) {
  FwdExtra ex = lms_extra(lms_task, lms_phi, lms_r, lms_alpha);
  const bool fused = shard_fused(h, p.B);
  if (fused && !p.update) {
    ex.qa_role = R_A;
    ex.qa_M = 0;
    ex.qa_sel = h->xb[0];
    ex.qa_row = 0;
    ex.qa_task = p.task;
    ex.qa_use_gpi = p.sel_use_gpi;
  } else if (fused) {
    ex.qa_role = R_S1;
    ex.qa_M = p.B;
    ex.qa_all = h->xb[0];
    ex.qa_ge = h->xge;
  } else if (p.update && p.pre) {
    return SFX_OK;  // look-ahead: the step before forwarded this minibatch (runner_ahead_ok)
  }
  RC(step_fwd(h, p, ex));
  return fused ? coll_max(h, h->xb[0], p.update ? shard_body(h, p.B) : (size_t)h->Tg * h->A) : SFX_OK;
}

// speculative round r: (unfused: GPI maxima of every global policy over this rank's heads ->
// all-reduce) -> TD targets, backward + Adam of the local heads, post-update forward of
// S1 ++ s_next (fused: which accumulates the next round's maxima, all-reduced right after;
// final rounds also fill the selection table)
int shard_round_body(sfx_handle* h, const sfx_handle::Pending& p, int r, bool final) {
  const bool fused = shard_fused(h, p.B);
  const size_t body = shard_body(h, p.B), tail = (size_t)h->Tg * h->A;
  int* xr = fused ? h->xb[r & 1] : h->xb[0];
  int* xn = h->xb[(r + 1) & 1];
  if (!fused) {
    RC(shard_qmax(h, p.B, r == 0 ? R_S1 : POST_ROLE, xr));
    RC(coll_max(h, xr, body));
  }
  TdgSpec td;
  td.use_gpi = 1;
  td.xmax = xr;
  td.poloff = h->off;
  td.next = spec_buf(h, r);  // local policies' next actions: round r+1 compares against them
  td.next_stride = MMAX;
  td.prev = r > 0 ? spec_buf(h, r - 1) : nullptr;
  td.skip = h->skip_rounds;
  // a skipped head's post-update forward is skipped too: unfused, its rows of the round's role
  // already hold what it would write; fused, its terms of the next round's maxima are replayed from
  // the copy its last computed round stored (FwdArgs::qh)
  const bool skip_fwd = h->skip_rounds && (!fused || h->qh);
  FwdExtra vx;
  if (fused) {
    td.xi_src = h->xge;
    td.xi_dst = xn;
    td.xi_copy = (int)body;
    td.xi_n = (int)(body + (final ? tail : 0));
    vx.qa_role = POST_ROLE;
    vx.qa_M = p.B;
    vx.qa_lt = xn;
    vx.qa_sel = final ? xn + body : nullptr;
    vx.qa_row = p.B;
    vx.qa_task = p.task;
    vx.qa_use_gpi = p.sel_use_gpi;
    if (skip_fwd) {
      vx.qh = h->qh;
      vx.qhs = h->qhs;
    }
  }
  // the look-ahead with unfused maxima only (DESIGN.md §4)
  bool v0 = false;
  RC(round_body(h, p, r, final, td, vx, p.s_next, skip_fwd, !fused, nullptr, &v0));
  if (!v0) return run_fwd(h, {{R_A, P_NEW, 1, 0, h->T}}, 1, p.s_next, nullptr);
  return fused ? coll_max(h, xn, body + (final ? tail : 0)) : SFX_OK;
}

// after the last round r_last (< 0: no update this step): verification against the post-update
// maxima, the env action from the selection table, and (runner steps, pub) the publication
int shard_final_body(sfx_handle* h, const sfx_handle::Pending& p, int r_last, HostResult* pub, const long long* dctr) {
  const bool upd = p.update && r_last >= 0;
  const bool fused = shard_fused(h, p.B);
  const size_t body = upd ? shard_body(h, p.B) : 0;
  const int *X, *Y;
  if (fused) {  // everything already accumulated and all-reduced by the rounds (or the begin)
    X = upd ? h->xb[r_last & 1] : nullptr;
    Y = upd ? h->xb[(r_last + 1) & 1] : h->xb[0];
  } else {
    X = upd ? h->xb[0] : nullptr;
    int* Yw = h->xb[1];
    if (upd) RC(shard_qmax(h, p.B, POST_ROLE, Yw));
    SselArgs S{};
    if (!upd || !can_fuse_v0(h, p.B + 1)) {
      S.role = R_A;
      S.row = 0;
    } else {
      S.role = POST_ROLE;
      S.row = p.B;
    }
    S.task = p.task;
    S.use_gpi = p.sel_use_gpi;
    S.off = h->off;
    S.Tg = h->Tg;
    S.q = Yw + body;
    launch(h, K_VER, 4.0 * h->T * h->O + 4.0 * h->Tg * h->A, k_ssel, dim3(cdiv(h->Tg * h->A, 256)), dim3(256), h->G,
           S);
    LAUNCHCHK();
    RC(coll_max(h, Yw, body + (size_t)h->Tg * h->A));
    Y = Yw;
  }
  SfinArgs F{};
  F.X = X;
  F.Y = Y;
  F.q = Y + body;
  F.Tg = h->Tg;
  F.M = p.B;
  F.A = h->A;
  F.flag = &h->dout->flag;
  F.sel = h->dout->sel;
  F.pub = pub;
  F.nonfin = h->G.nonfin;
  F.stall = pub ? h->dstall : nullptr;
  F.dctr = dctr;
  F.cancel = h->dcancel;
  launch(h, K_VER, 4.0 * (2.0 * body + (double)h->Tg * h->A), k_sfinish, dim3(1), dim3(1024), F);
  LAUNCHCHK();
  return SFX_OK;
}

// The sharded step p as the runner launches it, launch_step_all's twin: the begin, `rounds` device
// rounds (0: no minibatch in this step) and the finish
int shard_step_all(sfx_handle* h, const sfx_handle::Pending& p, int lms_task, const float* lms_phi, const float* lms_r,
                   float lms_alpha, int rounds, HostResult* pub, const long long* dctr) {
  RC(shard_begin_body(h, p, lms_task, lms_phi, lms_r, lms_alpha));
  for (int r = 0; r < rounds; ++r) RC(shard_round_body(h, p, r, r == rounds - 1));
  return shard_final_body(h, p, rounds - 1, pub, dctr);
}

// xb[2], xge of the sharded step (sized for T_glob, max_batch); xge follows xb[0] in one block so
// the gate's fill covers both
int shard_buffers(sfx_handle* h) {
  const size_t nb = (size_t)h->Tg * h->Mmax * h->A, nx = nb + (size_t)h->Tg * h->A;
  for (int*& p : h->xb) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  h->xge = nullptr;
  if (h->qh) (void)hipFree(h->qh);
  h->qh = nullptr;
  h->qhs = nullptr;
  HIPCHK(hipMalloc((void**)&h->xb[0], sizeof(int) * (nx + nb)));
  HIPCHK(hipMalloc((void**)&h->xb[1], sizeof(int) * nx));
  h->xge = h->xb[0] + nx;
  // each local head's own terms of the post-update maxima (q_accumulate), replayed by the rounds
  // that skip the head: [T][Tg][Mmax][A] ++ the selection row [T][A]
  const size_t nq = (size_t)h->T * h->Tg * h->Mmax * h->A;
  HIPCHK(hipMalloc((void**)&h->qh, sizeof(int) * (nq + (size_t)h->T * h->A)));
  h->qhs = h->qh + nq;
  return SFX_OK;
}

}  // namespace

extern "C" {

int sfx_shard_setup(sfx_t h, int T_glob, int head_offset) {
  RC(settle(h));
  if (!h || T_glob < h->T || head_offset < 0 || head_offset + h->T > T_glob)
    SFX_FAIL(SFX_E_ARG, "sfx_shard_setup: need 0 <= head_offset, head_offset + T <= T_glob");
  if ((long)T_glob * h->A > QMAX) SFX_FAIL(SFX_E_ARG, "sfx_shard_setup: T_glob * A exceeds kernel limits");
  HIPCHK(hipStreamSynchronize(h->stream));
  const size_t bytes = sizeof(float) * (size_t)T_glob * h->dpad;
  float* nw[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    if (hipMalloc((void**)&nw[i], bytes) != hipSuccess || hipMemset(nw[i], 0, bytes) != hipSuccess) {
      for (float* p : nw)
        if (p) (void)hipFree(p);
      SFX_FAIL(SFX_E_HIP, "sfx_shard_setup: hipMalloc failed");
    }
  }
  // keep what was loaded before the setup: the local rows land at their global index
  // (first setup: local rows 0..T-1 -> global rows head_offset..; a repeated setup keeps the
  // global rows it can)
  const bool first = h->Tg == h->T && h->off == 0;
  const size_t old_bytes = sizeof(float) * (size_t)std::min(h->Tg, first ? h->T : T_glob) * h->dpad;
  const size_t at = first ? (size_t)head_offset * h->dpad : 0;
  {
    const float* src[3] = {h->w, h->wm, h->wv};
    for (int i = 0; i < 3; ++i)
      if (hipMemcpy(nw[i] + at, src[i], old_bytes, hipMemcpyDeviceToDevice) != hipSuccess) {
        for (float* p : nw) (void)hipFree(p);
        SFX_FAIL(SFX_E_HIP, "sfx_shard_setup: copy of the loaded w rows failed");
      }
  }
  (void)hipFree(h->w);
  (void)hipFree(h->wm);
  (void)hipFree(h->wv);
  h->w = nw[0];
  h->wm = nw[1];
  h->wv = nw[2];
  h->G.w = h->w;
  h->G.wm = h->wm;
  h->G.wv = h->wv;
  h->Tg = T_glob;
  h->off = head_offset;
  if (h->spec_rounds_auto) h->spec_rounds = auto_spec_rounds(T_glob);
  clear_graphs(h);
  return SFX_OK;
}

int sfx_shard_begin(sfx_t h, const float* S, const int64_t* a, const float* phi, const float* S1, const float* gamma,
                    int B, int lms_task, const float* lms_phi, const float* lms_r, float lms_alpha,
                    const float* s_next) {
  RC(settle(h));
  if (!h) SFX_FAIL(SFX_E_ARG, "null handle");
  if (h->spend.active) SFX_FAIL(SFX_E_STATE, "sfx_shard_begin: previous step not finished");
  if (B < 0 || B > h->Mmax || (B > 0 && (!S || !a || !phi || !S1 || !gamma)) || !s_next)
    SFX_FAIL(SFX_E_ARG, "sfx_shard_begin: bad minibatch / next state");
  if (lms_task >= h->Tg || (lms_task >= 0 && (!lms_phi || !lms_r))) SFX_FAIL(SFX_E_ARG, "bad LMS args");
  auto& P = h->spend;
  P = sfx_handle::Pending();
  P.active = true;
  P.update = B > 0;
  P.B = B;
  P.S = S;
  P.S1 = S1;
  P.phi = phi;
  P.gamma = gamma;
  P.a = a;
  P.s_next = s_next;
  unsigned ab;
  std::memcpy(&ab, &lms_alpha, 4);
  const GraphKey key = make_key(10, {B, lms_task, (int)ab}, h->mask, {S, S1, s_next, lms_phi, lms_r});
  return run_graph(h, key, [&]() -> int { return step_fwd(h, P, lms_extra(lms_task, lms_phi, lms_r, lms_alpha)); });
}

int sfx_shard_td_maxima(sfx_t h, int round, int32_t* X) {
  RC(settle(h));
  if (!h || round < 0 || !X) SFX_FAIL(SFX_E_ARG, "bad args");
  RC(shard_fail_inactive(h));
  if (h->spend.B == 0) SFX_FAIL(SFX_E_STATE, "no minibatch in this step");
  const int guess = round == 0 ? R_S1 : POST_ROLE;
  const GraphKey key = make_key(11, {h->spend.B, guess}, h->mask, {X});
  return run_graph(h, key, [&]() -> int { return shard_qmax(h, h->spend.B, guess, X); });
}

int sfx_shard_td_update(sfx_t h, int round, const int32_t* X) {
  RC(settle(h));
  if (!h || round < 0 || !X) SFX_FAIL(SFX_E_ARG, "bad args");
  RC(shard_fail_inactive(h));
  const auto& P = h->spend;
  if (P.B == 0) SFX_FAIL(SFX_E_STATE, "no minibatch in this step");
  const GraphKey key =
      make_key(12, {P.B, round == 0 ? 1 : 0, POST_ROLE}, h->mask, {X, P.S, P.a, P.phi, P.S1, P.gamma, P.s_next});
  return run_graph(h, key, [&]() -> int {
    TdgSpec td;
    td.use_gpi = 1;
    td.xmax = X;
    td.poloff = h->off;
    bool v0 = false;  // no next / prev actions, no skipping, no look-ahead: the caller drives the rounds
    RC(round_body(h, P, round, false, td, FwdExtra(), P.s_next, false, false, nullptr, &v0));
    return v0 ? SFX_OK : run_fwd(h, {{R_A, P_NEW, 1, 0, h->T}}, 1, P.s_next, nullptr);
  });
}

int sfx_shard_ver_maxima(sfx_t h, int round, int32_t* Y) {
  RC(settle(h));
  if (!h || round < 0 || !Y) SFX_FAIL(SFX_E_ARG, "bad args");
  RC(shard_fail_inactive(h));
  if (h->spend.B == 0) SFX_FAIL(SFX_E_STATE, "no minibatch in this step");
  const GraphKey key = make_key(13, {h->spend.B, POST_ROLE}, h->mask, {Y});
  return run_graph(h, key, [&]() -> int { return shard_qmax(h, h->spend.B, POST_ROLE, Y); });
}

int sfx_shard_verify(sfx_t h, const int32_t* X, const int32_t* Y, int* flag) {
  RC(settle(h));
  if (!h || !X || !Y || !flag) SFX_FAIL(SFX_E_ARG, "bad args");
  RC(shard_fail_inactive(h));
  const GraphKey key = make_key(14, {h->spend.B}, 0, {X, Y, flag});
  return run_graph(h, key, [&]() -> int {
    hipLaunchKernelGGL(k_sverify, dim3(1), dim3(256), 0, h->stream, X, Y, h->Tg, h->spend.B, h->A, flag);
    LAUNCHCHK();
    return SFX_OK;
  });
}

int sfx_shard_select(sfx_t h, int round, int task, int use_gpi, long long* key_out) {
  RC(settle(h));
  if (!h || !key_out || task < 0 || task >= h->Tg) SFX_FAIL(SFX_E_ARG, "bad args");
  RC(shard_fail_inactive(h));
  KeyArgs K{};
  if (h->spend.B == 0 || round < 0) {  // online heads on s_next (computed by sfx_shard_begin)
    K.role = R_A;
    K.row = 0;
  } else if (can_fuse_v0(h, h->spend.B + 1)) {
    K.role = POST_ROLE;
    K.row = h->spend.B;
  } else {
    K.role = R_A;
    K.row = 0;
  }
  K.task = task;
  K.use_gpi = use_gpi ? 1 : 0;
  K.off = h->off;
  K.key = key_out;
  const GraphKey key = make_key(15, {K.role, K.row, task, K.use_gpi}, 0, {key_out});
  return run_graph(h, key, [&]() -> int {
    hipLaunchKernelGGL(k_skey, dim3(1), dim3(256), 0, h->stream, h->G, K);
    LAUNCHCHK();
    return SFX_OK;
  });
}

int sfx_shard_finish(sfx_t h, int rounds_run) {
  RC(settle(h));
  if (!h) SFX_FAIL(SFX_E_ARG, "null handle");
  RC(shard_fail_inactive(h));
  const bool update = h->spend.B > 0;
  h->spend.active = false;
  if (update) {
    h->steps_spec += 1;
    h->rounds_total += rounds_run;
    if (rounds_run > h->spec_rounds) h->steps_fallback += 1;
    h->mask ^= h->all_bits();
    for (int t = 0; t < h->T; ++t) {
      after_update(h, t);
      RC(maybe_sync_target(h, t));
    }
  }
  return SFX_OK;
}

}  // extern "C"
