// sfx_pre.inc -- C ABI of the φ pre-training handle (include/sfx.h sfx_pre_*; kernels: sfx_pre.h).
// Included at the end of sfx.hip.  A handle of its own: the reference pre-trains before any task is
// added to the agent (sfdqn_phi.py:987), so nothing here touches an sfx_t.

struct sfx_pre_handle {
  PreGeo G{};
  int Ptorch = 0, Pint = 0;
  hipStream_t stream = nullptr;
  AdamHP hp_phi{1e-3, 0.0, 0.9, 0.999, 1e-8};
  AdamHP hp_w{1e-3, 0.0, 0.9, 0.999, 1e-8};
  float *p = nullptr, *m = nullptr, *v = nullptr, *w = nullptr, *wm = nullptr, *wv = nullptr;
  float *act = nullptr, *dz = nullptr, *dzt = nullptr, *phi = nullptr, *dy = nullptr;
  int* step = nullptr;
  AdamC* adamc = nullptr;
};

namespace {

template <class T>
int pre_alloc(T** out, size_t n) {
  HIPCHK(hipMalloc(reinterpret_cast<void**>(out), n * sizeof(T)));
  HIPCHK(hipMemset(*out, 0, n * sizeof(T)));
  return SFX_OK;
}

// torch packing (per Linear: W [N][K], b [N]) <-> the padded device layout
void pre_pack(const PreGeo& G, const float* src, std::vector<float>& dst) {
  for (int l = 0; l < G.NL; ++l) {
    for (int o = 0; o < G.N[l]; ++o)
      std::memcpy(&dst[G.offW[l] + (size_t)o * G.Kp[l]], src + (size_t)o * G.K[l], sizeof(float) * G.K[l]);
    src += (size_t)G.N[l] * G.K[l];
    std::memcpy(&dst[G.offB[l]], src, sizeof(float) * G.N[l]);
    src += G.N[l];
  }
}
void pre_unpack(const PreGeo& G, const std::vector<float>& src, float* dst) {
  for (int l = 0; l < G.NL; ++l) {
    for (int o = 0; o < G.N[l]; ++o)
      std::memcpy(dst + (size_t)o * G.K[l], &src[G.offW[l] + (size_t)o * G.Kp[l]], sizeof(float) * G.K[l]);
    dst += (size_t)G.N[l] * G.K[l];
    std::memcpy(dst, &src[G.offB[l]], sizeof(float) * G.N[l]);
    dst += G.N[l];
  }
}

int pre_put(sfx_pre_handle* h, float* dev, const float* host) {
  std::vector<float> buf(h->Pint, 0.f);
  pre_pack(h->G, host, buf);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dev, buf.data(), sizeof(float) * h->Pint, hipMemcpyHostToDevice));
  return SFX_OK;
}
int pre_fetch(sfx_pre_handle* h, const float* dev, float* host) {
  std::vector<float> buf(h->Pint);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(buf.data(), dev, sizeof(float) * h->Pint, hipMemcpyDeviceToHost));
  pre_unpack(h->G, buf, host);
  return SFX_OK;
}

PreArgs pre_args(sfx_pre_handle* h, int task, const float* S, const int64_t* a, const float* r, const float* S1, int B,
                 float* out) {
  PreArgs A{};
  A.G = h->G;
  A.p = h->p, A.m = h->m, A.v = h->v, A.w = h->w, A.wm = h->wm, A.wv = h->wv;
  A.step = h->step, A.adamc = h->adamc, A.act = h->act, A.dz = h->dz, A.dzt = h->dzt, A.phi = h->phi, A.dy = h->dy;
  A.S = S, A.S1 = S1, A.r = r, A.a = a, A.out = out, A.B = B, A.task = task;
  A.hp_phi = h->hp_phi, A.hp_w = h->hp_w;
  return A;
}

}  // namespace

int sfx_pre_create(sfx_pre_t* out, int n_s, int d, int T, const int* hidden_host, int n_hidden, int max_batch) {
  if (!out) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: null argument (out)");
  *out = nullptr;
  if (n_s < 1 || 2 * n_s + 1 > PRE_IN) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit n_in = 2 n_s + 1 <= 64 (n_s >= 1)");
  if (n_hidden < 1 || n_hidden > PRE_NL - 1) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit 1 to 4 hidden layers");
  if (!hidden_host) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: null argument (hidden_host)");
  for (int i = 0; i < n_hidden; ++i)
    if (hidden_host[i] < 1 || hidden_host[i] > PRE_HID)
      SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit hidden width 1 to 256");
  if (d < 1 || d > PRE_D) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit 1 <= d <= 64");
  if (max_batch < 1 || max_batch > PRE_B) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit 1 <= max_batch <= 64");
  if (T < 1) SFX_FAIL(SFX_E_ARG, "sfx_pre_create: limit T >= 1");
  auto* h = new sfx_pre_handle();
  PreGeo& G = h->G;
  G.n_s = n_s, G.n_in = 2 * n_s + 1, G.d = d, G.T = T, G.NL = n_hidden + 1, G.Mmax = max_batch, G.dp = align4(d);
  int off = 0, offA = 0, offZ = 0, offZt = 0, tile = 0;
  for (int l = 0; l < G.NL; ++l) {
    G.K[l] = l == 0 ? G.n_in : hidden_host[l - 1];
    G.N[l] = l == G.NL - 1 ? d : hidden_host[l];
    G.Kp[l] = align4(G.K[l]);
    G.offW[l] = off, off += G.N[l] * G.Kp[l];
    G.offB[l] = off, off += align4(G.N[l]);
    G.offA[l] = offA, offA += max_batch * G.Kp[l];
    G.offZ[l] = offZ, offZ += max_batch * G.N[l];
    G.offZt[l] = offZt, offZt += PRE_B * G.N[l];
    G.tile0[l] = tile, tile += cdiv(G.N[l], 16);
    h->Ptorch += G.N[l] * (G.K[l] + 1);
  }
  G.tile0[G.NL] = G.ntile = tile;
  h->Pint = off;
  int rc = SFX_OK;
  auto take = [&](int r) { rc = rc ? rc : r; };
  take(pre_alloc(&h->p, off)), take(pre_alloc(&h->m, off)), take(pre_alloc(&h->v, off));
  take(pre_alloc(&h->w, (size_t)T * G.dp)), take(pre_alloc(&h->wm, (size_t)T * G.dp));
  take(pre_alloc(&h->wv, (size_t)T * G.dp));
  take(pre_alloc(&h->act, offA)), take(pre_alloc(&h->dz, offZ)), take(pre_alloc(&h->dzt, offZt)), take(pre_alloc(&h->phi, (size_t)max_batch * d));
  take(pre_alloc(&h->dy, max_batch)), take(pre_alloc(&h->step, 1 + T)), take(pre_alloc(&h->adamc, 2));
  if (rc) {
    const std::string keep = g_err;
    sfx_pre_destroy(h);
    g_err = keep;
    return rc;
  }
  *out = h;
  return SFX_OK;
}

int sfx_pre_destroy(sfx_pre_t h) {
  if (!h) return SFX_OK;
  (void)hipStreamSynchronize(h->stream);
  for (void* q : {(void*)h->p, (void*)h->m, (void*)h->v, (void*)h->w, (void*)h->wm, (void*)h->wv, (void*)h->act,
                  (void*)h->dz, (void*)h->dzt, (void*)h->phi, (void*)h->dy, (void*)h->step, (void*)h->adamc})
    if (q) (void)hipFree(q);
  delete h;
  return SFX_OK;
}

int sfx_pre_set_stream(sfx_pre_t h, void* stream) {
  if (!h) SFX_FAIL(SFX_E_ARG, "sfx_pre_set_stream: null handle");
  h->stream = static_cast<hipStream_t>(stream);
  return SFX_OK;
}

int sfx_pre_numel(sfx_pre_t h) { return h ? h->Ptorch : 0; }

int sfx_pre_set_adam(sfx_pre_t h, double lr_phi, double wd_phi, double lr_w, double wd_w, double beta1, double beta2,
                     double eps) {
  if (!h) SFX_FAIL(SFX_E_ARG, "sfx_pre_set_adam: null handle");
  h->hp_phi = AdamHP{lr_phi, wd_phi, beta1, beta2, eps};
  h->hp_w = AdamHP{lr_w, wd_w, beta1, beta2, eps};
  return SFX_OK;
}

int sfx_pre_load(sfx_pre_t h, const float* params_host) {
  if (!h || !params_host) SFX_FAIL(SFX_E_ARG, "sfx_pre_load: null argument");
  return pre_put(h, h->p, params_host);
}

int sfx_pre_get(sfx_pre_t h, float* params_host) {
  if (!h || !params_host) SFX_FAIL(SFX_E_ARG, "sfx_pre_get: null argument");
  return pre_fetch(h, h->p, params_host);
}

int sfx_pre_load_adam(sfx_pre_t h, const float* m_host, const float* v_host, int step) {
  if (!h || !m_host || !v_host) SFX_FAIL(SFX_E_ARG, "sfx_pre_load_adam: null argument");
  if (step < 0) SFX_FAIL(SFX_E_ARG, "sfx_pre_load_adam: limit step >= 0");
  RC(pre_put(h, h->m, m_host));
  RC(pre_put(h, h->v, v_host));
  HIPCHK(hipMemcpy(h->step, &step, sizeof(int), hipMemcpyHostToDevice));
  return SFX_OK;
}

int sfx_pre_get_adam(sfx_pre_t h, float* m_host, float* v_host, int* step) {
  if (!h || !m_host || !v_host || !step) SFX_FAIL(SFX_E_ARG, "sfx_pre_get_adam: null argument");
  RC(pre_fetch(h, h->m, m_host));
  RC(pre_fetch(h, h->v, v_host));
  HIPCHK(hipMemcpy(step, h->step, sizeof(int), hipMemcpyDeviceToHost));
  return SFX_OK;
}

int sfx_pre_load_w(sfx_pre_t h, int t, const float* w_host, const float* m_host, const float* v_host, int step) {
  if (!h || !w_host || !m_host || !v_host) SFX_FAIL(SFX_E_ARG, "sfx_pre_load_w: null argument");
  if (t < 0 || t >= h->G.T) SFX_FAIL(SFX_E_ARG, "sfx_pre_load_w: limit 0 <= t < T");
  if (step < 0) SFX_FAIL(SFX_E_ARG, "sfx_pre_load_w: limit step >= 0");
  const size_t o = (size_t)t * h->G.dp, n = sizeof(float) * h->G.d;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->w + o, w_host, n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->wm + o, m_host, n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->wv + o, v_host, n, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->step + 1 + t, &step, sizeof(int), hipMemcpyHostToDevice));
  return SFX_OK;
}

int sfx_pre_get_w(sfx_pre_t h, int t, float* w_host, float* m_host, float* v_host, int* step) {
  if (!h || !w_host || !m_host || !v_host || !step) SFX_FAIL(SFX_E_ARG, "sfx_pre_get_w: null argument");
  if (t < 0 || t >= h->G.T) SFX_FAIL(SFX_E_ARG, "sfx_pre_get_w: limit 0 <= t < T");
  const size_t o = (size_t)t * h->G.dp, n = sizeof(float) * h->G.d;
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(w_host, h->w + o, n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(m_host, h->wm + o, n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(v_host, h->wv + o, n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(step, h->step + 1 + t, sizeof(int), hipMemcpyDeviceToHost));
  return SFX_OK;
}

#define PRE_BY_TILES(B, ...)     \
  switch (cdiv((B), 16)) {       \
    case 1: { constexpr int MT = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int MT = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int MT = 3; __VA_ARGS__; } break; \
    default: { constexpr int MT = 4; __VA_ARGS__; } break; \
  }

int sfx_pre_update(sfx_pre_t h, int task, const float* S, const int64_t* a, const float* r, const float* S1, int B,
                   float* loss) {
  if (!h) SFX_FAIL(SFX_E_ARG, "sfx_pre_update: null handle");
  if (!S || !a || !r || !S1 || !loss) SFX_FAIL(SFX_E_ARG, "sfx_pre_update: null argument");
  if (task < 0 || task >= h->G.T) SFX_FAIL(SFX_E_ARG, "sfx_pre_update: limit 0 <= task < T");
  if (B < 1 || B > h->G.Mmax) SFX_FAIL(SFX_E_ARG, "sfx_pre_update: limit 1 <= B <= max_batch");
  const PreArgs A = pre_args(h, task, S, a, r, S1, B, loss);
  PRE_BY_TILES(B, (k_pre_fwd<MT, true><<<2, 64 * PRE_WAVES, 0, h->stream>>>(A)));
  LAUNCHCHK();
  PRE_BY_TILES(B, (k_pre_step<MT><<<h->G.ntile + 1, 256, 0, h->stream>>>(A)));
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_pre_features(sfx_pre_t h, const float* S, const int64_t* a, const float* S1, int B, float* phi) {
  if (!h) SFX_FAIL(SFX_E_ARG, "sfx_pre_features: null handle");
  if (!S || !a || !S1 || !phi) SFX_FAIL(SFX_E_ARG, "sfx_pre_features: null argument");
  if (B < 1 || B > h->G.Mmax) SFX_FAIL(SFX_E_ARG, "sfx_pre_features: limit 1 <= B <= max_batch");
  const PreArgs A = pre_args(h, 0, S, a, nullptr, S1, B, phi);
  PRE_BY_TILES(B, (k_pre_fwd<MT, false><<<1, 64 * PRE_WAVES, 0, h->stream>>>(A)));
  LAUNCHCHK();
  return SFX_OK;
}

namespace {

// k_pre_rows on `stream` (the runner: the ψ handle's, inside its captured step graph).  No allocation, no
// scratch of the handle; cancel: a runner gate's cancel word or null.
int pre_rows_body(sfx_pre_handle* h, hipStream_t stream, const float* S, const int64_t* a, const float* S1, int M,
                  float* phi, const int* cancel) {
  PreRowsArgs A{};
  A.G = h->G;
  A.p = h->p, A.S = S, A.S1 = S1, A.a = a, A.phi = phi, A.M = M, A.cancel = cancel;
  k_pre_rows<<<cdiv(M, 16), 64 * PRE_WAVES, 0, stream>>>(A);
  LAUNCHCHK();
  return SFX_OK;
}
void pre_dims(const sfx_pre_handle* h, int* n_s, int* d) { *n_s = h->G.n_s, *d = h->G.d; }

}  // namespace

int sfx_pre_features_rows(sfx_pre_t h, const float* S, const int64_t* a, const float* S1, int M, float* phi) {
  if (!h) SFX_FAIL(SFX_E_ARG, "sfx_pre_features_rows: null handle");
  if (!S || !a || !S1 || !phi) SFX_FAIL(SFX_E_ARG, "sfx_pre_features_rows: null argument");
  if (M < 1 || M > PRE_ROWS_MAX) SFX_FAIL(SFX_E_ARG, "sfx_pre_features_rows: limit 1 <= M <= 65536");
  return pre_rows_body(h, h->stream, S, a, S1, M, phi, nullptr);
}

#undef PRE_BY_TILES
