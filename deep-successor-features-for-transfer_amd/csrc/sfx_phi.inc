// sfx_phi.inc -- learned φ (features/deep_phi.py DeepSF_PHI.update_successor, SURVEY §8f rank 4)
// on a handle (included by sfx.hip).  Kernels and the math: sfx_phi.h.

struct sfx_phi_state {
  int n_in = 0, hid = 0, n_mid = 0, P = 0;
  float* p = nullptr;     // [P] the φ net (torch packing)
  float* acts = nullptr;  // [n_mid + 2][Mmax][hid] (+ the input block)
  float* phis = nullptr;  // [Mmax][d]
  float lr = 1e-3f;
  bool wide = false;      // hid > 128: sfx_phiw.h's kernels
  // TSF-DQN with a learned φ (sfx_tsf_phi_update) and the wide net's backward
  float *tphi = nullptr, *tt = nullptr, *usum = nullptr;  // [Mmax][d] φ̃, t, u + u'
  float* gbuf = nullptr;  // [2][Mmax][max(hid, d)] the layers' output gradients (ping-pong)
};

namespace {

void phi_free(sfx_phi_state* s) {
  if (!s) return;
  for (float* q : {s->p, s->acts, s->phis, s->tphi, s->tt, s->usum, s->gbuf})
    if (q) (void)hipFree(q);
  delete s;
}

PhiArgs phi_args(sfx_handle* h, int pol, int B) {
  sfx_phi_state* s = h->phi;
  PhiArgs A{};
  A.n_in = s->n_in;
  A.hid = s->hid;
  A.n_mid = s->n_mid;
  A.d = h->d;
  A.B = B;
  A.n_s = h->n_s;
  A.O = h->O;
  A.lastOff = h->actOff[h->NL - 1];
  A.pol = pol;
  A.p = s->p;
  A.acts = s->acts;
  A.phis = s->phis;
  A.w = h->w + (size_t)pol * h->dpad;
  A.dzlast = h->dz + (size_t)pol * h->actSize + A.lastOff;
  A.hp = AdamHP{s->lr, 0.0, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.cancel = h->dcancel;
  return A;
}

// Buffers that only some updates need, allocated at their first use (outside any capture): gbuf for a
// wide net's backward and for sfx_tsf_phi_update, tphi / tt / usum for sfx_tsf_phi_update alone.
int phi_lazy_buffers(sfx_handle* h, bool tsf) {
  sfx_phi_state* s = h->phi;
  const size_t bd = (size_t)h->Mmax * h->d, gs = (size_t)2 * h->Mmax * std::max(s->hid, h->d);
  float** ptrs[4] = {&s->gbuf, &s->tphi, &s->tt, &s->usum};
  const size_t sizes[4] = {gs, bd, bd, bd};
  for (int i = 0; i < (tsf ? 4 : 1); ++i) {
    if (*ptrs[i]) continue;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (hipMalloc((void**)ptrs[i], sizeof(float) * sizes[i]) != hipSuccess ||
        hipMemset(*ptrs[i], 0, sizeof(float) * sizes[i]) != hipSuccess)
      SFX_FAIL(SFX_E_HIP, "learned φ: hipMalloc failed");
  }
  return SFX_OK;
}

int phi_setup_common(sfx_handle* h, int n_in, int hid, int n_mid, float lr) {
  HIPCHK(hipStreamSynchronize(h->stream));
  if (h->phi) phi_free(h->phi);
  h->phi = nullptr;
  clear_graphs(h);  // captured updates carry the freed buffers
  auto* s = new sfx_phi_state();
  s->n_in = n_in;
  s->hid = hid;
  s->n_mid = n_mid;
  s->lr = lr;
  s->wide = hid > PHI_HID;
  s->P = hid * (n_in + 1) + n_mid * hid * (hid + 1) + h->d * (hid + 1);
  // the layer-0 input block [Mmax][n_in] sits in the last slot of acts: a slot holds max(hid, n_in) per row
  const size_t sizes[3] = {(size_t)s->P, (size_t)(n_mid + 2) * h->Mmax * std::max(hid, n_in), (size_t)h->Mmax * h->d};
  float** ptrs[3] = {&s->p, &s->acts, &s->phis};
  for (int i = 0; i < 3; ++i)
    if (hipMalloc((void**)ptrs[i], sizeof(float) * sizes[i]) != hipSuccess ||
        hipMemset(*ptrs[i], 0, sizeof(float) * sizes[i]) != hipSuccess) {
      phi_free(s);
      SFX_FAIL(SFX_E_HIP, "sfx_phi_setup: hipMalloc failed");
    }
  h->phi = s;
  return SFX_OK;
}

}  // namespace

void phi_release(sfx_handle* h) {
  phi_free(h->phi);
  h->phi = nullptr;
}

extern "C" {

int sfx_phi_setup(sfx_t h, int width_mul, int n_mid, float lr) {
  RC(settle(h));
  if (!h || width_mul < 1 || n_mid < 0 || !(lr > 0.f)) SFX_FAIL(SFX_E_ARG, "bad args");
  touch(h);
  const int n_in = 2 * h->n_s + 1, hid = width_mul * n_in;
  if (n_in > PHI_IN || hid > PHI_HID || h->d > PHI_IN || n_mid + 2 > PHI_L || h->Mmax > PHI_B || h->Tg != h->T)
    SFX_FAIL(SFX_E_ARG, "sfx_phi_setup: needs 2 n_s + 1 <= 64, hidden <= 128, d <= 64, max_batch <= 64, unsharded");
  return phi_setup_common(h, n_in, hid, n_mid, lr);
}

int sfx_phi_setup_dims(sfx_t h, int hid, int n_mid, float lr) {
  RC(settle(h));
  if (!h || hid < 1 || n_mid < 0 || !(lr > 0.f)) SFX_FAIL(SFX_E_ARG, "bad args");
  touch(h);
  const int n_in = 2 * h->n_s + 1;
  if (n_in > PHI_IN || hid > PHIW_HID || h->d > PHI_IN || n_mid + 2 > PHI_L || h->Mmax > PHI_B || h->Tg != h->T)
    SFX_FAIL(SFX_E_ARG,
             "sfx_phi_setup_dims: needs 2 n_s + 1 <= 64, hidden <= 2048, d <= 64, max_batch <= 64, unsharded");
  return phi_setup_common(h, n_in, hid, n_mid, lr);
}

int sfx_phi_numel(sfx_t h) { return h && h->phi ? h->phi->P : SFX_E_ARG; }

int sfx_phi_load(sfx_t h, const float* params_host) {
  RC(settle(h));
  if (!h || !h->phi || !params_host) SFX_FAIL(SFX_E_ARG, "sfx_phi_load: call sfx_phi_setup first");
  HIPCHK(hipStreamSynchronize(h->stream));
  touch(h);
  HIPCHK(hipMemcpy(h->phi->p, params_host, sizeof(float) * h->phi->P, hipMemcpyHostToDevice));
  return SFX_OK;
}

int sfx_phi_get(sfx_t h, float* params_host) {
  RC(settle(h));
  if (!h || !h->phi || !params_host) SFX_FAIL(SFX_E_ARG, "sfx_phi_get: call sfx_phi_setup first");
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(params_host, h->phi->p, sizeof(float) * h->phi->P, hipMemcpyDeviceToHost));
  return SFX_OK;
}

}  // extern "C"

namespace {

// ---- the wide net (sfx_phiw.h): one launch per layer and pass ----
PhiwLayer phiw_layer(sfx_handle* h, int l, int B, int clamp) {
  sfx_phi_state* s = h->phi;
  const int L = s->n_mid + 2;
  PhiwLayer A{};
  A.K = l == 0 ? s->n_in : s->hid;
  A.N = l == L - 1 ? h->d : s->hid;
  size_t off = 0;
  for (int j = 0; j < l; ++j) off += (size_t)(j == L - 1 ? h->d : s->hid) * ((j == 0 ? s->n_in : s->hid) + 1);
  A.W = s->p + off;
  A.X = l == 0 ? s->acts + (size_t)(L - 1) * B * s->hid : s->acts + (size_t)(l - 1) * B * s->hid;
  A.Y = l == L - 1 ? s->phis : s->acts + (size_t)l * B * s->hid;
  const size_t gs = (size_t)h->Mmax * std::max(s->hid, h->d);
  A.G = s->gbuf + (size_t)((L - 1 - l) & 1) * gs;
  A.GX = s->gbuf + (size_t)((L - l) & 1) * gs;
  A.B = B;
  A.relu = l < L - 1;
  A.clamp = clamp;
  A.hp = AdamHP{s->lr, 0.0, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.cancel = h->dcancel;
  return A;
}

// out: where the last layer's φ [B][d] goes (nullptr: the state's phis)
int phiw_forward(sfx_handle* h, int B, const float* S, const int64_t* a, const float* S1, float* out = nullptr) {
  sfx_phi_state* s = h->phi;
  const int L = s->n_mid + 2, MT = cdiv(B, 16);
  launch(h, K_TSF, 4.0 * 2.0 * B * s->n_in, k_phiw_in, dim3(cdiv(B * s->n_in, 256)), dim3(256),
         s->acts + (size_t)(L - 1) * B * s->hid, S, a, S1, B, h->n_s);
  LAUNCHCHK();
  for (int l = 0; l < L; ++l) {
    PhiwLayer A = phiw_layer(h, l, B, 0);
    if (out && l == L - 1) A.Y = out;
    const double bytes = 4.0 * ((double)A.N * (A.K + 1) + (double)B * (A.K + A.N));
    const dim3 grid(cdiv(A.N, 16));
    switch (MT) {
      case 1: launch(h, K_TSF, bytes, k_phiw_fwd<1>, grid, dim3(64 * PHIW_S), A); break;
      case 2: launch(h, K_TSF, bytes, k_phiw_fwd<2>, grid, dim3(64 * PHIW_S), A); break;
      case 3: launch(h, K_TSF, bytes, k_phiw_fwd<3>, grid, dim3(64 * PHIW_S), A); break;
      default: launch(h, K_TSF, bytes, k_phiw_fwd<4>, grid, dim3(64 * PHIW_S), A); break;
    }
    LAUNCHCHK();
  }
  return SFX_OK;
}

// from the output gradient dφ in gbuf's first half: per layer dX (W before its step), then dW + step
int phiw_backward(sfx_handle* h, int B, int clamp) {
  sfx_phi_state* s = h->phi;
  const int L = s->n_mid + 2, MT = cdiv(B, 16);
  for (int l = L - 1; l >= 0; --l) {
    const PhiwLayer A = phiw_layer(h, l, B, clamp);
    const double wb = 4.0 * (double)A.N * A.K, ab = 4.0 * (double)B * (A.K + A.N);
    if (l > 0) {
      const dim3 grid(cdiv(A.K, 16));
      switch (MT) {
        case 1: launch(h, K_TSF, wb + ab, k_phiw_dx<1>, grid, dim3(64 * PHIW_S), A); break;
        case 2: launch(h, K_TSF, wb + ab, k_phiw_dx<2>, grid, dim3(64 * PHIW_S), A); break;
        case 3: launch(h, K_TSF, wb + ab, k_phiw_dx<3>, grid, dim3(64 * PHIW_S), A); break;
        default: launch(h, K_TSF, wb + ab, k_phiw_dx<4>, grid, dim3(64 * PHIW_S), A); break;
      }
      LAUNCHCHK();
    }
    const dim3 gw(cdiv(A.N, 16), cdiv(A.K, 256));
    switch (MT) {
      case 1: launch(h, K_TSF, 2.0 * wb + ab, k_phiw_dw<1>, gw, dim3(256), A); break;
      case 2: launch(h, K_TSF, 2.0 * wb + ab, k_phiw_dw<2>, gw, dim3(256), A); break;
      case 3: launch(h, K_TSF, 2.0 * wb + ab, k_phiw_dw<3>, gw, dim3(256), A); break;
      default: launch(h, K_TSF, 2.0 * wb + ab, k_phiw_dw<4>, gw, dim3(256), A); break;
    }
    LAUNCHCHK();
  }
  return SFX_OK;
}

// DeepSF_PHI.update_successor (transform = 0) / TSFDQN_PHI.update_deep_models (transform = 1) of one head:
// launches only (update_body's shape), shared by sfx_phi_update, sfx_tsf_phi_update and the runner's learned-φ
// steps, so all three produce the same bits.  The buffers of phi_lazy_buffers must exist already (it allocates:
// never inside a capture).  Under a runner gate every commit honours the step's cancel word: the ψ launches
// through Geo::cancel, the φ kernels through PhiArgs / TsfPhiArgs / PhiwLayer::cancel.
int phi_update_body(sfx_handle* h, int transform, int policy, const float* S, const int64_t* a, const float* r,
                    const float* S1, const float* gamma, int B, int use_gpi, float* bias, float* lambda, float* losses,
                    int64_t* next) {
  sfx_phi_state* s = h->phi;
  PhiArgs A = phi_args(h, policy, B);
  A.S = S;
  A.S1 = S1;
  A.a = a;
  A.r = r;
  A.wb = bias;
  A.lam = lambda;
  A.losses = losses;
  TsfPhiArgs Q{};
  Q.B = B;
  Q.d = h->d;
  Q.n_s = h->n_s;
  Q.O = h->O;
  Q.transform = transform;
  Q.clamp = transform;
  Q.S = S;
  Q.S1 = S1;
  Q.a = a;
  Q.r = r;
  if (transform) {
    Q.g = h->tsf->g + (size_t)policy * h->tsf->Pg;
    Q.hp = h->tsf->hp;
  }
  Q.phis = s->phis;
  Q.tphi = transform ? s->tphi : s->phis;
  Q.tt = s->tt;
  Q.usum = s->usum;
  Q.dzlast = A.dzlast;
  Q.gtop = s->gbuf;
  Q.w = A.w;
  Q.wb = bias;
  Q.lam = lambda;
  Q.losses = losses;
  Q.hpa = A.hp;
  Q.cancel = h->dcancel;
  const double P = s->P, Bd = B, bd = Bd * h->d;
  if (s->wide) {
    RC(phiw_forward(h, B, S, a, S1));
  } else {
    launch(h, K_TSF, 4.0 * (P + Bd * (s->n_in + (s->n_mid + 1.0) * s->hid + h->d)), k_phi_fwd, dim3(1), dim3(256), A);
    LAUNCHCHK();
  }
  if (transform) {
    launch(h, K_TSF, 4.0 * (2.0 * Bd * h->n_s + 4.0 * bd + h->tsf->Pg + h->tsf->Ph), k_tsfphi_fwd, dim3(1), dim3(256),
           Q);
    LAUNCHCHK();
  }
  // the ψ update with φ (φ̃) as the features: λ-scaled output gradient, fresh Adam, psi_loss into losses[1]
  if (use_gpi)
    RC(run_fwd(h, {{R_S, P_ONLINE, 1, policy, 1}, {R_S1T, P_TARGET, 2, policy, 1}, {R_S1, P_ONLINE, 2, 0, h->T}}, B,
               S, S1));
  else
    RC(run_fwd(h, {{R_S, P_ONLINE, 1, policy, 1}, {R_S1T, P_TARGET, 2, policy, 1}, {R_S1, P_ONLINE, 2, policy, 1}},
               B, S, S1));
  // a freshly built Adam (features/deep_phi.py:163-175, agents/tsfdqn_phi.py:249 make one per update):
  // zero moments in the head's read slot and step 0, which the backward bumps to 1 (its bias corrections).
  // No cancel guard on this reset: every learned-φ update starts from zero moments and step 0, so a
  // cancelled runner step that zeroed them leaves exactly what its re-issue (and any later φ update of
  // the head) would write first anyway.  It is a kernel (k_phi_fresh), not three hipMemsetAsync: as memset
  // nodes of the runner's step graphs -- launched behind a step that is still running, their gates giving
  // up -- the resets did not stay in order with the kernels around them (measured: non-finite heads after
  // the first cancelled step with memset nodes, bit-exact runs with the kernel), and every other schedule's
  // step graph is kernel nodes only.
  const size_t ro = ((size_t)h->slot(policy) * h->T + policy) * h->P;
  touch(h);
  launch(h, K_TSF, 8.0 * h->P, k_phi_fresh, dim3(cdiv(h->P, 256)), dim3(256), h->am + ro, h->av + ro, h->P,
         h->step + policy);
  LAUNCHCHK();
  TdgSpec td;
  td.use_gpi = use_gpi;
  td.a = a;
  td.gamma = gamma;
  td.next = next;
  td.next_stride = B;
  td.dz_scale = lambda;
  RC(run_bwd(h, policy, 1, B, S, Q.tphi, nullptr, losses, td));
  if (!s->wide && !transform) {
    launch(h, K_TSF, 4.0 * (3.0 * P + Bd * ((s->n_mid + 1.0) * s->hid + s->n_in + 2.0 * h->d + h->O)), k_phi_bwd,
           dim3(1), dim3(256), A);
    LAUNCHCHK();
    return SFX_OK;
  }
  launch(h, K_TSF, 4.0 * (Bd * h->O + 6.0 * bd + (transform ? 2.0 * (h->tsf->Pg + h->tsf->Ph) : 0.0)), k_tsfphi_bwd,
         dim3(1), dim3(256), Q);
  LAUNCHCHK();
  if (s->wide) {
    RC(phiw_backward(h, B, transform));
  } else {
    launch(h, K_TSF, 4.0 * (3.0 * P + Bd * ((s->n_mid + 1.0) * s->hid + s->n_in + h->d)), k_phi_bwd_top, dim3(1),
           dim3(256), A, (const float*)s->gbuf);
    LAUNCHCHK();
  }
  return SFX_OK;
}

// What the runner's learned-φ schedules need of the handle (sfx_runner_config): SFX_E_STATE naming the missing
// piece, else the update's lazily allocated buffers are made now, outside any capture.
int phi_runner_prepare(sfx_handle* h, bool tsf) {
  if (h->Tg != h->T) SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the learned-φ schedules need an unsharded handle");
  if (!h->phi)
    SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the learned-φ schedules need a φ net (sfx_phi_setup or sfx_phi_setup_dims)");
  if (tsf && (!h->tsf || h->tsf->G != h->d || h->tsf->K != 0))
    SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the tsf_phi schedule needs sfx_tsf_setup(G = d, K = 0) (g_i, h plain Linear)");
  if (h->T > 64 || h->A > 256)
    SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the biased selection of the learned-φ schedules needs T <= 64 and A <= 256");
  if (tsf || h->phi->wide) RC(phi_lazy_buffers(h, tsf));
  return SFX_OK;
}

// still so at a step's capture?  (a φ or TSF setup made after sfx_runner_config replaces the state and its buffers)
bool phi_runner_ready(const sfx_handle* h, bool tsf) {
  const sfx_phi_state* s = h->phi;
  if (!s || h->Tg != h->T || ((tsf || s->wide) && !s->gbuf)) return false;
  return !tsf || (s->tphi && s->tt && s->usum && h->tsf && h->tsf->G == h->d && h->tsf->K == 0);
}

int phi_update_impl(sfx_handle* h, int op, int transform, int policy, const float* S, const int64_t* a, const float* r,
                    const float* S1, const float* gamma, int B, int use_gpi, float* bias, float* lambda, float* losses,
                    int64_t* next) {
  if (transform || h->phi->wide) RC(phi_lazy_buffers(h, transform != 0));
  const GraphKey key =
      make_key(op, {policy, B, use_gpi ? 1 : 0}, h->mask, {S, a, r, S1, gamma, bias, lambda, losses, next});
  RC(run_graph(h, key, [&]() -> int {
    return phi_update_body(h, transform, policy, S, a, r, S1, gamma, B, use_gpi, bias, lambda, losses, next);
  }));
  h->mask ^= 1ull << policy;
  after_update(h, policy);
  return maybe_sync_target(h, policy);
}

}  // namespace

extern "C" {

int sfx_phi_update(sfx_t h, int policy, const float* S, const int64_t* a, const float* r, const float* S1,
                   const float* gamma, int B, int use_gpi, float* bias, float* lambda, float* losses, int64_t* next) {
  RC(settle(h));
  if (!h || !h->phi) SFX_FAIL(SFX_E_ARG, "sfx_phi_update: call sfx_phi_setup first");
  if (!valid_head(h, policy) || B < 1 || B > h->Mmax || !S || !a || !r || !S1 || !gamma || !bias || !lambda || !losses)
    SFX_FAIL(SFX_E_ARG, "bad args");
  return phi_update_impl(h, 30, 0, policy, S, a, r, S1, gamma, B, use_gpi, bias, lambda, losses, next);
}

int sfx_tsf_phi_update(sfx_t h, int policy, const float* S, const int64_t* a, const float* r, const float* S1,
                       const float* gamma, int B, int use_gpi, float* bias, float* lambda, float* losses,
                       int64_t* next) {
  RC(settle(h));
  if (!h) SFX_FAIL(SFX_E_ARG, "bad args");
  if (!h->phi) SFX_FAIL(SFX_E_ARG, "sfx_tsf_phi_update: call sfx_phi_setup or sfx_phi_setup_dims first");
  if (!h->tsf) SFX_FAIL(SFX_E_ARG, "sfx_tsf_phi_update: call sfx_tsf_setup(G = d, K = 0) first");
  if (h->tsf->G != h->d || h->tsf->K != 0)
    SFX_FAIL(SFX_E_ARG, "sfx_tsf_phi_update: needs sfx_tsf_setup with G = d and K = 0 (g_i, h plain Linear)");
  if (!valid_head(h, policy) || B < 1 || B > h->Mmax || !S || !a || !r || !S1 || !gamma || !bias || !lambda || !losses)
    SFX_FAIL(SFX_E_ARG, "bad args");
  return phi_update_impl(h, 31, 1, policy, S, a, r, S1, gamma, B, use_gpi, bias, lambda, losses, next);
}

}  // extern "C"

// ---- the learned-φ agents' test phase (kernels and the math: sfx_phitest.h) ------------------

namespace {

// what every test-phase call needs: an unsharded handle and a φ setup; the TSF ones also g_t / h as plain
// Linears (sfx_tsf_setup(G = d, K = 0)) and shapes one workgroup of k_tsfphi_test_* holds
int phi_test_ok(sfx_handle* h, bool tsf, const char* name) {
  if (!h) SFX_FAIL(SFX_E_ARG, std::string(name) + ": null handle");
  if (h->Tg != h->T) SFX_FAIL(SFX_E_ARG, std::string(name) + ": needs an unsharded handle");
  if (!h->phi) SFX_FAIL(SFX_E_ARG, std::string(name) + ": call sfx_phi_setup or sfx_phi_setup_dims first");
  if (!tsf) return SFX_OK;
  if (!h->tsf) SFX_FAIL(SFX_E_ARG, std::string(name) + ": call sfx_tsf_setup(G = d, K = 0) first");
  if (h->tsf->G != h->d || h->tsf->K != 0)
    SFX_FAIL(SFX_E_ARG, std::string(name) + ": needs sfx_tsf_setup with G = d and K = 0 (g_i, h plain Linear)");
  const long long Td = (long long)h->T * h->d;
  if (h->d > PHIT_D || h->A > PHIT_A || h->A * h->d > PHIT_AD || Td > PHIT_TD || h->A * Td > PHIT_ATD)
    SFX_FAIL(SFX_E_ARG, std::string(name) + ": needs d <= 64, A <= 64, A d <= 1024, T d <= 1024, A T d <= 4096");
  return SFX_OK;
}

// φ of B rows into out [B][d]: one row of a wide net through the one-row kernels, anything else through the
// update's forward
int phi_features_impl(sfx_handle* h, const float* S, const int64_t* a, const float* S1, int B, float* out) {
  sfx_phi_state* s = h->phi;
  if (!s->wide) {
    PhiArgs A = phi_args(h, 0, B);
    A.S = S;
    A.S1 = S1;
    A.a = a;
    A.phis = out;
    launch(h, K_TSF, 4.0 * (s->P + (double)B * (s->n_in + (s->n_mid + 1.0) * s->hid + h->d)), k_phi_fwd, dim3(1),
           dim3(256), A);
    LAUNCHCHK();
    return SFX_OK;
  }
  if (B > 1) {
    RC(phi_lazy_buffers(h, false));
    return phiw_forward(h, B, S, a, S1, out);
  }
  const int L = s->n_mid + 2;
  size_t off = 0;
  for (int l = 0; l < L; ++l) {
    Phi1Args A{};
    A.K = l == 0 ? s->n_in : s->hid;
    A.N = l == L - 1 ? h->d : s->hid;
    A.W = s->p + off;
    off += (size_t)A.N * (A.K + 1);
    A.X = l == 0 ? nullptr : s->acts + (size_t)(l - 1) * s->hid;
    A.Y = l == L - 1 ? out : s->acts + (size_t)l * s->hid;
    A.s = S;
    A.s1 = S1;
    A.a = a;
    A.n_s = h->n_s;
    A.relu = l < L - 1;
    launch(h, K_TSF, 4.0 * ((double)A.N * (A.K + 2) + A.K), k_phi1_fwd, dim3(cdiv(A.N, PHI1_R)),
           dim3(64 * PHI1_R * PHI1_S), A);
    LAUNCHCHK();
  }
  return SFX_OK;
}

PhiTestArgs phi_test_args(sfx_handle* h) {
  PhiTestArgs A{};
  A.T = h->T;
  A.A = h->A;
  A.d = h->d;
  A.n_s = h->n_s;
  A.lastOff = h->actOff[h->NL - 1];
  A.actSize = h->actSize;
  A.phi = h->phi->phis;
  A.hpa = AdamHP{h->phi->lr, 0.0, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  return A;
}

}  // namespace

extern "C" {

int sfx_phi_features(sfx_t h, const float* S, const int64_t* a, const float* S1, int B, float* phi) {
  RC(settle(h));
  RC(phi_test_ok(h, false, "sfx_phi_features"));
  if (!S || !a || !S1 || !phi) SFX_FAIL(SFX_E_ARG, "sfx_phi_features: null argument");
  if (B < 1 || B > h->Mmax) SFX_FAIL(SFX_E_ARG, "sfx_phi_features: B must be in [1, max_batch]");
  return phi_features_impl(h, S, a, S1, B, phi);
}

int sfx_tsf_phi_test_action(sfx_t h, const float* s, const float* omega_w, const float* omega_b, const float* w,
                            const float* wb, int64_t* a_out) {
  RC(settle(h));
  RC(phi_test_ok(h, true, "sfx_tsf_phi_test_action"));
  if (!s || !omega_w || !omega_b || !w || !wb || !a_out) SFX_FAIL(SFX_E_ARG, "sfx_tsf_phi_test_action: null argument");
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}}, 1, s, nullptr));
  PhiTestArgs A = phi_test_args(h);
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.oW = const_cast<float*>(omega_w);
  A.ob = const_cast<float*>(omega_b);
  A.w = const_cast<float*>(w);
  A.wb = const_cast<float*>(wb);
  A.act_out = a_out;
  launch(h, K_GPI, 4.0 * ((double)h->T * h->O + (double)h->d * (h->T * h->d + 2.0)), k_tsfphi_test_act, dim3(1),
         dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_tsf_phi_test_update(sfx_t h, const float* s, const int64_t* a, float r, const float* s1, float gamma,
                            float* omega_w, float* omega_b, float* w, float* wb, float* lambda, float* losses) {
  RC(settle(h));
  RC(phi_test_ok(h, true, "sfx_tsf_phi_test_update"));
  if (!s || !a || !s1 || !omega_w || !omega_b || !w || !wb || !lambda || !losses)
    SFX_FAIL(SFX_E_ARG, "sfx_tsf_phi_test_update: null argument");
  sfx_tsf_state* ts = h->tsf;
  RC(phi_features_impl(h, s, a, s1, 1, h->phi->phis));
  // ψ_t(s) of the online heads and ψ⁻_t(s1) of the target heads, one forward for both
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}, {R_G, P_TARGET, 2, 0, h->T}}, 1, s, s1));
  PhiTestArgs A = phi_test_args(h);
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.psi1 = h->act + (size_t)R_G * h->T * h->actSize;
  A.s = s;
  A.s1 = s1;
  A.g = ts->g;
  A.Pg = ts->Pg;
  A.hp = ts->hp;
  A.oW = omega_w;
  A.ob = omega_b;
  A.w = w;
  A.wb = wb;
  A.lam = lambda;
  A.r = r;
  A.gamma = gamma;
  A.losses = losses;
  launch(h, K_TSF, 4.0 * (2.0 * h->T * h->O + (double)h->T * ts->Pg + ts->Ph + 2.0 * h->d * (h->T * h->d + 2.0)),
         k_tsfphi_test_step, dim3(1), dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_phi_test_update(sfx_t h, const float* s, const int64_t* a, float r, const float* s1, float* w, float* wb,
                        float* loss) {
  RC(settle(h));
  RC(phi_test_ok(h, false, "sfx_phi_test_update"));
  if (!s || !a || !s1 || !w || !wb || !loss) SFX_FAIL(SFX_E_ARG, "sfx_phi_test_update: null argument");
  RC(phi_features_impl(h, s, a, s1, 1, h->phi->phis));
  PhiTestArgs A = phi_test_args(h);
  A.w = w;
  A.wb = wb;
  A.r = r;
  A.losses = loss;
  launch(h, K_TSF, 4.0 * 3.0 * h->d, k_phi_test_step, dim3(1), dim3(64), A);
  LAUNCHCHK();
  return SFX_OK;
}

}  // extern "C"

// ---- SF-φ's test tasks in lockstep: E rows per launch set ------------------------------------

namespace {

int phi_rows_ok(sfx_handle* h, int E, const char* name) {
  RC(phi_test_ok(h, false, name));
  if (E < 1 || E > PHIE || E > h->Mmax)
    SFX_FAIL(SFX_E_ARG, std::string(name) + ": E must be in [1, min(" + std::to_string(PHIE) + ", max_batch)]");
  return SFX_OK;
}

// φ of E rows into out [E][d], row e bit for bit phi_features_impl's one-row result
int phi_rows_impl(sfx_handle* h, const float* S, const int64_t* a, const float* S1, int E, float* out) {
  sfx_phi_state* s = h->phi;
  if (!s->wide) {
    PhiArgs A = phi_args(h, 0, 1);
    A.S = S;
    A.S1 = S1;
    A.a = a;
    A.phis = out;
    launch(h, K_TSF, 4.0 * E * (s->P + (double)s->n_in + h->d), k_phiE_narrow, dim3(E), dim3(256), A);
    LAUNCHCHK();
    return SFX_OK;
  }
  const int L = s->n_mid + 2;
  size_t off = 0;
  for (int l = 0; l < L; ++l) {
    PhiEArgs A{};
    A.K = l == 0 ? s->n_in : s->hid;
    A.N = l == L - 1 ? h->d : s->hid;
    A.W = s->p + off;
    off += (size_t)A.N * (A.K + 1);
    A.X = l == 0 ? nullptr : s->acts + (size_t)(l - 1) * E * s->hid;
    A.Y = l == L - 1 ? out : s->acts + (size_t)l * E * s->hid;
    A.S = S;
    A.S1 = S1;
    A.a = a;
    A.n_s = h->n_s;
    A.relu = l < L - 1;
    A.E = E;
    const double bytes = 4.0 * ((double)A.N * (A.K + 1) + (double)E * (A.K + A.N));
    const dim3 grid(cdiv(A.N, PHI1_R)), block(64 * PHI1_R * PHI1_S);
    // k_phi1_fwd's test for 16-byte words (its x, s->acts + (l - 1) hid, is aligned when K = hid is a multiple
    // of 4, as this one): then the rows go through LDS, PHIE_LDS of them per launch; else the scalar-load kernel
    const bool vec = A.X && (A.K & 3) == 0 && A.K <= PHIW_HID && (((uintptr_t)A.W | (uintptr_t)A.X) & 15) == 0;
    if (vec) {
      const dim3 gl(cdiv(A.N, PHI1_R * PHIE_G));
      for (int e0 = 0; e0 < E; e0 += PHIE_LDS) {
        PhiEArgs C = A;
        C.E = std::min(PHIE_LDS, E - e0);
        C.X = A.X + (size_t)e0 * A.K;
        C.Y = A.Y + (size_t)e0 * A.N;
        const double by = 4.0 * ((double)A.N * (A.K + 1) + (double)C.E * (A.K + A.N));
        if (C.E == 1)
          launch(h, K_TSF, by, k_phiE_fwd_lds<1>, gl, block, C);
        else if (C.E == 2)
          launch(h, K_TSF, by, k_phiE_fwd_lds<2>, gl, block, C);
        else if (C.E <= 4)
          launch(h, K_TSF, by, k_phiE_fwd_lds<4>, gl, block, C);
        else
          launch(h, K_TSF, by, k_phiE_fwd_lds<PHIE_LDS>, gl, block, C);
        LAUNCHCHK();
      }
      continue;
    }
    if (E == 1)
      launch(h, K_TSF, bytes, k_phiE_fwd<1>, grid, block, A);
    else if (E == 2)
      launch(h, K_TSF, bytes, k_phiE_fwd<2>, grid, block, A);
    else if (E <= 4)
      launch(h, K_TSF, bytes, k_phiE_fwd<4>, grid, block, A);
    else if (E <= 8)
      launch(h, K_TSF, bytes, k_phiE_fwd<8>, grid, block, A);
    else
      launch(h, K_TSF, bytes, k_phiE_fwd<PHIE>, grid, block, A);
    LAUNCHCHK();
  }
  return SFX_OK;
}

// ---- the learned-φ SF agent's test phase in the runner (sfx_runner_phi_test_phase, sfx_runner.inc) ----

// the handle's part of the phase's preconditions (the E-row calls' own, phi_rows_ok, with the phase's name and
// status codes; E is checked by the entry point); the phase needs no buffer of the φ state beyond those of the φ
// setup, so nothing is allocated.  The kernels' shape bounds need no refusal of their own: a φ setup takes
// 2 n_s + 1 <= 64 only (k_phi_test_intake's LDS holds n_s <= PHI_TEST_NS = 32), and the phase runs under schedule 5
// only, which sfx_runner_config grants at T <= 64 and A <= 256 (gpi_pick's 256 head / action maxima in LDS).
int phi_test_phase_ready(sfx_handle* h) {
  const std::string F = "sfx_runner_phi_test_phase: ";
  if (h->Tg != h->T) SFX_FAIL(SFX_E_STATE, F + "needs an unsharded handle");
  if (!h->phi) SFX_FAIL(SFX_E_STATE, F + "needs a φ net (sfx_phi_setup or sfx_phi_setup_dims)");
  return SFX_OK;
}

// what a captured lockstep step carries of the φ state: a new φ setup frees them (and clears the graphs)
void phi_test_phase_ptrs(sfx_handle* h, const void** p) {
  p[0] = h->phi->p;
  p[1] = h->phi->acts;
  p[2] = h->phi->phis;
}

// One lockstep step's launches on h->stream, a linear chain: intake; φ(S ⊕ a ⊕ S1) of the E rows into the φ
// state's phis (dead rows ride along: the same launches every step); ψ(S1) of every online head -> R_G, as
// sfx_phi_test_actions (a role nothing reads afterwards); the row kernel; the publication.
int phi_test_phase_body(sfx_handle* h, int E, int horizon, float* W, int w_stride, float* Wb, const unsigned char* stage,
                        unsigned char* blk, float* loss, int64_t* sel, TestResult* res) {
  const PhiTestDevLayout D = phi_test_dev_layout(h->n_s);
  PhiTestIntakeArgs I{};
  I.stage = stage;
  I.E = E;
  I.n_s = h->n_s;
  I.horizon = horizon;
  I.hdr = reinterpret_cast<PhiTestDevHdr*>(blk + D.hdr);
  I.live = reinterpret_cast<int*>(blk + D.live);
  I.a = reinterpret_cast<int64_t*>(blk + D.a);
  I.r = reinterpret_cast<float*>(blk + D.r);
  I.S = reinterpret_cast<float*>(blk + D.S);
  I.S1 = reinterpret_cast<float*>(blk + D.S1);
  hipLaunchKernelGGL(k_phi_test_intake, dim3(1), dim3(256), 0, h->stream, I);
  LAUNCHCHK();
  RC(phi_rows_impl(h, I.S, I.a, I.S1, E, h->phi->phis));
  RC(run_fwd(h, {{R_G, P_ONLINE, 1, 0, h->T}}, E, I.S1, nullptr));
  GpiArgs g = gpi_args(R_G, 0, 0, W, nullptr, nullptr, nullptr, nullptr, sel, 0, 1, E);
  g.w_stride = w_stride;
  g.sel_stride = 2;
  PhiTestArgs A = phi_test_args(h);
  A.w = W;
  PhiTestRowArgs X{};
  X.hdr = I.hdr;
  X.live = I.live;
  X.r = I.r;
  X.loss = loss;
  X.E = E;
  X.horizon = horizon;
  X.w_stride = w_stride;
  launch(h, K_GPI, 4.0 * E * ((double)h->T * h->O + 4.0 * h->d + 5.0), k_phi_test_row, dim3(E), dim3(256), h->G, g, Wb, A,
         X);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_test_publish, dim3(1), dim3(128), 0, h->stream, (const int64_t*)sel, E,
                     (const long long*)&I.hdr->seq, res);
  LAUNCHCHK();
  return SFX_OK;
}

}  // namespace

extern "C" {

int sfx_phi_features_rows(sfx_t h, const float* S, const int64_t* a, const float* S1, int E, float* phi) {
  RC(settle(h));
  RC(phi_rows_ok(h, E, "sfx_phi_features_rows"));
  if (!S || !a || !S1 || !phi) SFX_FAIL(SFX_E_ARG, "sfx_phi_features_rows: null argument");
  return phi_rows_impl(h, S, a, S1, E, phi);
}

int sfx_phi_test_actions(sfx_t h, const float* S, int E, const float* W, int w_stride, const float* Wb, float* q,
                         int64_t* out) {
  RC(settle(h));
  RC(phi_rows_ok(h, E, "sfx_phi_test_actions"));
  if (!S || !W || !Wb || !out) SFX_FAIL(SFX_E_ARG, "sfx_phi_test_actions: null argument");
  if (w_stride < h->d) SFX_FAIL(SFX_E_ARG, "sfx_phi_test_actions: w_stride must be at least d");
  RC(run_fwd(h, {{R_G, P_ONLINE, 1, 0, h->T}}, E, S, nullptr));
  GpiArgs g = gpi_args(R_G, 0, 0, W, nullptr, q, nullptr, nullptr, out, 0, 1, E);
  g.w_stride = w_stride;
  g.sel_stride = 2;
  launch(h, K_GPI, 4.0 * E * ((double)h->T * h->O + h->d + 1.0 + (q ? h->T * h->A : 0)), k_phi_test_act, dim3(E),
         dim3(256), h->G, g, Wb);
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_phi_test_updates(sfx_t h, int E, const float* S, const int64_t* a, const float* r, const float* S1, float* W,
                         int w_stride, float* Wb, float* loss) {
  RC(settle(h));
  RC(phi_rows_ok(h, E, "sfx_phi_test_updates"));
  if (!S || !a || !r || !S1 || !W || !Wb || !loss) SFX_FAIL(SFX_E_ARG, "sfx_phi_test_updates: null argument");
  if (w_stride < h->d) SFX_FAIL(SFX_E_ARG, "sfx_phi_test_updates: w_stride must be at least d");
  RC(phi_rows_impl(h, S, a, S1, E, h->phi->phis));
  PhiTestArgs A = phi_test_args(h);
  A.w = W;
  A.wb = Wb;
  A.losses = loss;
  launch(h, K_TSF, 4.0 * E * (3.0 * h->d + 4.0), k_phi_test_steps, dim3(E), dim3(64), A, r, w_stride);
  LAUNCHCHK();
  return SFX_OK;
}

}  // extern "C"
