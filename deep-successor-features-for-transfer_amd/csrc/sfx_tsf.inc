// sfx_tsf.inc -- TSF-DQN update (tsfdqn.py:588-709, tsfdqn_nf.py) on a handle (included by
// sfx.hip).  Kernels: sfx_tsf.h.  The ψ part reuses the SF-DQN path with φ̃ as the features.

struct sfx_tsf_state {
  int G = 0, K = 0, Pg = 0, Ph = 0;
  float beta = 1.f;
  AdamHP hpg{1e-3, 0.0, 0.9, 0.999, 1e-8}, hph{1e-3, 0.0, 0.9, 0.999, 1e-8};
  bool freeze_flows = false;  // sfx_tsf_freeze_flows
  float *g = nullptr, *gm = nullptr, *gv = nullptr, *hp = nullptr, *hm = nullptr, *hv = nullptr;
  float *zs = nullptr, *ts = nullptr, *gfeat = nullptr, *tphi = nullptr, *part = nullptr, *snap = nullptr;
  float* gch = nullptr;   // [T][K][tsf_fst(NP)] the flows in the chain layout (TsfArgs::gch)
  float* bimg = nullptr;  // the backward's staging image of W_l, W_h (TsfArgs::bimg)
  float* tgf = nullptr;  // [rows][T][2][G] g features of the test-task path (sfx_tsf_test_update(s))
  int tgf_rows = 0;
  std::vector<char> g_loaded;  // task t's g_t was loaded (sfx_tsf_load_g / _g_state); h_loaded: sfx_tsf_load_h
  bool h_loaded = false;
  // The TSF forward, backward and the flows' sums ride along in ψ launches on the step stream
  // (k_fwd_tsf / k_bwd_tsf) when their LDS carve and the grid fit, else they run as their own
  // launches there.  (Round 3's side-stream fork of the TSF kernels lost its A/B to riding along
  // and was removed in round 5: DESIGN.md §3.)
};

namespace {

void tsf_free(sfx_tsf_state* s) {
  if (!s) return;
  for (float* p : {s->g, s->gm, s->gv, s->hp, s->hm, s->hv, s->zs, s->ts, s->gfeat, s->tphi, s->part, s->snap, s->tgf,
                   s->gch, s->bimg})
    if (p) (void)hipFree(p);
  delete s;
}

TsfArgs tsf_args(sfx_handle* h, int pol, int B, const float* S, const float* S1, const float* phi, const float* r,
                 const int64_t* a, float* losses) {
  sfx_tsf_state* s = h->tsf;
  TsfArgs A{};
  A.pol = pol;
  A.B = B;
  A.n_s = h->n_s;
  A.G = s->G;
  A.K = s->K;
  A.d = h->d;
  A.Pg = s->Pg;
  A.Ph = s->Ph;
  A.O = h->O;
  A.lastOff = h->actOff[h->NL - 1];
  A.beta = s->beta;
  A.S = S;
  A.S1 = S1;
  A.phi = phi;
  A.r = r;
  A.a = a;
  A.g = s->g;
  A.gch = s->gch;
  A.gm = s->gm;
  A.gv = s->gv;
  A.hp = s->hp;
  A.hm = s->hm;
  A.hv = s->hv;
  A.zs = s->zs;
  A.ts = s->ts;
  A.gfeat = s->gfeat;
  A.tphi = s->tphi;
  A.part = s->part;
  A.snap = s->snap;
  A.np = tsf_np(h->n_s);
  A.scratch = s->snap + ((s->Pg + s->Ph + h->d + 63) & ~63);
  A.bimg = s->bimg;
  A.nflow = s->K > 0 ? cdiv(2 * B, TSF_FR) : 0;
  A.nh = cdiv(s->Ph, 256);
  A.nlin = cdiv(s->G, TSF_QS);
  A.losses = losses;
  A.dzlast = h->dz + (size_t)pol * h->actSize + A.lastOff;
  A.step = h->step + pol;
  A.cancel = h->dcancel;
  const size_t wr = (size_t)(h->off + pol) * h->dpad;  // w has T_glob rows when the heads are sharded
  A.w = h->w + wr;
  A.wm = h->wm + wr;
  A.wv = h->wv + wr;
  A.hpw = h->hp_w;
  A.hpg = s->hpg;
  A.hph = s->hph;
  A.hpf = s->hpg;
  if (s->freeze_flows) A.hpf.lr = A.hpf.wd = 0.0;
  return A;
}

}  // namespace

namespace {

// the flow kernels for NP = tsf_np(n_s) (register width of a flow row)
struct TsfKernels {
  void (*fwd)(TsfArgs, const float*);
  void (*bwd)(TsfArgs, const float*);
  void (*ride[2])(Geo, BwdArgs, TsfArgs, const float*, int, int);          // fp32 / bf16 ψ tiles
  void (*fride[2][3])(Geo, FwdArgs, TsfArgs, const float*, int, int, int);  // [fp32 / bf16][1 / 2 / 3 column tiles]
};
template <int NP>
constexpr TsfKernels tsf_kernels_of() {
  return {k_tsf_fwd<NP>, k_tsf_bwd<NP>, {k_bwd_tsf<NP, false>, k_bwd_tsf<NP, true>},
          {{k_fwd_tsf<NP, false, 1>, k_fwd_tsf<NP, false, 2>, k_fwd_tsf<NP, false, 3>},
           {k_fwd_tsf<NP, true, 1>, k_fwd_tsf<NP, true, 2>, k_fwd_tsf<NP, true, 3>}}};
}
TsfKernels tsf_kernels(int np) {
  switch (np) {
    case 4: return tsf_kernels_of<4>();
    case 8: return tsf_kernels_of<8>();
    case 16: return tsf_kernels_of<16>();
    default: return tsf_kernels_of<32>();
  }
}

// xmax (sharded heads): the all-reduced GPI maxima [B][A] of this policy replace the local GPI
// (the forward of every head on S1 was run by sfx_shard_tsf_maxima).
// algorithmic bytes of the TSF forward: g_i and h read, the 2B rows in, φ̃ / g features / flow states out
double tsf_fwd_bytes(const sfx_handle* h, int B) {
  const sfx_tsf_state* ts = h->tsf;
  const double rows = 2.0 * B, acts = rows * ts->G + B * (double)h->d + (ts->K + 1.0) * rows * h->n_s + ts->K * rows;
  return 4.0 * (ts->Pg + ts->Ph + rows * h->n_s + B * (double)h->d + acts);
}

// The TSF forward of `policy` for the minibatch (S, S1, φ) -- φ̃, the flow states, g features and
// the pre-step snapshot of g_i, h, w_i -- beside the ψ forward `fwd` (a run_fwd call taking the
// FwdExtra): riding in its first (layer-0+1) launch when the LDS carve fits there, else as its own
// launch before it (or after it, when that launch could not take riders).
int tsf_fwd_with(sfx_handle* h, int policy, int B, const float* S, const float* S1, const float* phi,
                 const std::function<int(const FwdExtra&)>& fwd, const float* xc, int mode) {
  const sfx_tsf_state* ts = h->tsf;
  TsfArgs A = tsf_args(h, policy, B, S, S1, phi, nullptr, nullptr, nullptr);
  A.fwd_mode = mode;
  const double fwd_by = tsf_fwd_bytes(h, B);
  const int fgrid = cdiv(B, TSF_PB);
  const float* gfl = ts->g + (size_t)policy * ts->Pg;
  auto fwd_alone = [&]() -> int {
    launch(h, K_TSF, fwd_by, tsf_kernels(A.np).fwd, dim3(fgrid), dim3(256), A, gfl);
    LAUNCHCHK();
    return SFX_OK;
  };
  const bool fride = tsf_fwd_lds(ts->K, A.np, ts->G, h->d).total <= TSFXF_SM;
  bool rode = false;
  FwdExtra fx;
  fx.xc = xc;
  if (fride)
    fx.ride_l0 = [&](const FwdArgs& F0, dim3 grid, double by) -> bool {
      // the two halves' LDS side by side holds this launch to one workgroup per CU: three column
      // tiles per workgroup where two would leave workgroups for a second round (the TSF look-ahead
      // select's 544 tiles: 272 + 4 workgroups -> 204 + 4)
      FwdArgs F = F0;
      if (F.tpw == 2 && (long)grid.x * grid.y * grid.z + fgrid > h->ncu) {
        F.tpw = 3;
        grid.x = cdiv(F.ntN, 3);
      }
      launch(h, K_FWD, by + fwd_by, tsf_kernels(A.np).fride[h->bf16 ? 1 : 0][F.tpw - 1],
             dim3(fgrid + grid.x * grid.y * grid.z), dim3(64 * FWD_WAVES), h->G, F, A, gfl, fgrid, (int)grid.x, (int)grid.y);
      rode = true;
      return true;
    };
  else
    RC(fwd_alone());
  RC(fwd(fx));
  if (fride && !rode) RC(fwd_alone());
  return SFX_OK;
}

// the forward's tail (mode 2) as riders of the selection launch, when its LDS carve fits there
bool tsf_tail_rider(sfx_handle* h, int policy, int B, const float* S, const float* S1, const float* phi, TsfTail* out) {
  const sfx_tsf_state* ts = h->tsf;
  if (!ts) return false;
  TsfArgs A = tsf_args(h, policy, B, S, S1, phi, nullptr, nullptr, nullptr);
  if (tsf_tail_lds(A.np, ts->G, h->d).total > TSFXF_SM) return false;
  A.fwd_mode = 2;
  out->A = A;
  out->gfl = ts->g + (size_t)policy * ts->Pg;
  out->nblk = cdiv(B, TSF_PB);
  out->bytes = 0.0;  // counted with the forward (tsf_fwd_bytes)
  return true;
}

int tsf_body(sfx_handle* h, int policy, const float* S, const int64_t* a, const float* r, const float* phi,
             const float* S1, const float* gamma, int B, int use_gpi, float* losses, int64_t* next,
             const int* xmax, bool pre) {
  const TsfArgs A = tsf_args(h, policy, B, S, S1, phi, r, a, losses);
  // algorithmic bytes of the backward: the ψ output gradient read, g_i, h (+ moments)
  // read-modify-written (the forward's: tsf_fwd_bytes)
  const sfx_tsf_state* ts = h->tsf;
  const double rows = 2.0 * B, acts = rows * ts->G + B * (double)h->d + (ts->K + 1.0) * rows * h->n_s + ts->K * rows;
  const double bwd_by = 24.0 * (ts->Pg + ts->Ph + h->d) + 4.0 * (acts + B * (double)h->O + rows * h->n_s);
  const float* sfl = ts->snap;
  // the ψ forward of the minibatch; pre: the previous step's look-ahead select computed it and
  // the TSF forward (select_ahead_body)
  auto psi_fwd = [&](const FwdExtra& fx) -> int {
    if (xmax) return run_fwd(h, {{R_S, P_ONLINE, 1, policy, 1}, {R_S1T, P_TARGET, 2, policy, 1}}, B, S, S1, fx);
    if (use_gpi)
      return run_fwd(h, {{R_S, P_ONLINE, 1, policy, 1}, {R_S1T, P_TARGET, 2, policy, 1}, {R_S1, P_ONLINE, 2, 0, h->T}},
                     B, S, S1, fx);
    return run_fwd(h, {{R_S, P_ONLINE, 1, policy, 1}, {R_S1T, P_TARGET, 2, policy, 1}, {R_S1, P_ONLINE, 2, policy, 1}},
                   B, S, S1, fx);
  };
  if (!pre)  // riding along in the ψ forward's first launch (its workgroups first in the grid)
    RC(tsf_fwd_with(h, policy, B, S, S1, phi, psi_fwd, nullptr));
  TdgSpec td;
  td.use_gpi = use_gpi;
  td.a = a;
  td.gamma = gamma;
  td.next = next;
  td.next_stride = B;
  td.xmax = xmax;
  td.poloff = -policy;  // xmax holds this policy's rows only
  const int nbwd = A.nflow + A.nh + A.nlin + 1;
  const double flow_by = 4.0 * (2.0 * B + 6.0) * ts->K * (2 * h->n_s + 1);
  auto bwd_alone = [&]() -> int {
    launch(h, K_TSF, bwd_by, tsf_kernels(A.np).bwd, dim3(nbwd), dim3(256), A, sfl);
    LAUNCHCHK();
    return SFX_OK;
  };
  auto flow_alone = [&]() -> int {
    if (ts->K > 0) {
      launch(h, K_TSF, flow_by, k_tsf_flow, dim3(ts->K), dim3(256), A);
      LAUNCHCHK();
    }
    return SFX_OK;
  };
  BwdExtra bx;
  // ride along: the TSF backward in the first ψ backward launch after the loss tail (the ψ
  // output gradient, l1 and the Adam step are final there), the flows' sums in the next one
  int rode = 0;
  const bool ride = tsf_bwd_lds(ts->K, A.np, ts->G, h->d, B).total <= TSFX_SM;
  if (ride) {
    bx.ride = [&](int li, int tail_at, const BwdArgs& BA, int ntile, double by) -> bool {
      int mode = 0, ntsf = 0;
      double tb = 0.0;
      if (rode == 0 && li == tail_at + 1) {
        mode = 1, ntsf = nbwd, tb = bwd_by;
      } else if (rode == 1 && ts->K > 0 && li == tail_at + 2) {
        mode = 2, ntsf = ts->K, tb = flow_by;
      }
      if (!mode || ntsf + ntile > h->ncu) return false;
      launch(h, K_BWD, by + tb, tsf_kernels(A.np).ride[h->bf16 ? 1 : 0], dim3(ntsf + ntile), dim3(256), h->G, BA, A,
             sfl, mode, ntsf);
      rode = mode;
      return true;
    };
  }
  RC(run_bwd(h, policy, 1, B, S, ts->tphi, nullptr, losses, td, bx));  // ψ with φ̃; l1 into losses
  // what did not ride a ψ launch runs after them
  if (rode == 0) RC(bwd_alone());
  if (rode <= 1) RC(flow_alone());
  return SFX_OK;
}

}  // namespace

// TsfArgs::gch of head t from its packed flows (after a host write of g_t)
int tsf_pack_chain(sfx_handle* h, int t) {
  const sfx_tsf_state* ts = h->tsf;
  if (ts->K == 0) return SFX_OK;
  const int np = tsf_np(h->n_s);
  hipLaunchKernelGGL(k_tsf_gch, dim3(ts->K), dim3(64), 0, h->stream, ts->g + (size_t)t * ts->Pg,
                     ts->gch + (size_t)t * ts->K * tsf_fst(np), h->n_s, np);
  LAUNCHCHK();
  return SFX_OK;
}

void tsf_release(sfx_handle* h) {
  tsf_free(h->tsf);
  h->tsf = nullptr;
}

extern "C" {

int sfx_tsf_setup(sfx_t h, int G, int K, float beta, double lr_g, double wd_g, double lr_h, double wd_h) {
  RC(settle(h));
  if (!h || G < 1 || K < 0) SFX_FAIL(SFX_E_ARG, "bad args");
  touch(h);
  const int n_s = h->n_s, d = h->d, B = h->Mmax;
  const long fs = 2L * n_s + 1, nfl = K * fs, nlin = (long)G * n_s + G;
  const long np = tsf_np(n_s), fr = TSF_FR;
  const long g4 = (G + 3) & ~3;
  if (n_s > TSF_NS || B > 64 || d > 256 || G > 256 || (long)d * g4 > TSF_LDS || 2L * B * G > TSF_LDS ||
      (long)B * d > TSF_LDS / 2 || nfl + nlin > TSF_LDS / 2 || 2L * TSF_PB * g4 > TSF_LDS / 2 || g4 * np > TSF_LDS / 2 ||
      (long)G * ((d + 3) & ~3) > TSF_LDS || (long)TSF_FR * g4 > 2048 ||
      (long)TSF_PB * d > 1024 ||
      (K > 0 && (K * tsf_fst((int)np) > TSF_FA || fr * K > TSF_TS || fr * G > 2048 || fr * d > 2048)) ||
      tsf_bwd_lds(K, (int)np, G, d, B).total > TSF_SM || tsf_fwd_lds(K, (int)np, G, d).total > TSF_FWD_SM)
    SFX_FAIL(SFX_E_ARG, "TSF geometry exceeds kernel limits (n_s<=32, batch<=64, d*G<=8192, ...; see sfx_tsf.h)");
  HIPCHK(hipStreamSynchronize(h->stream));
  tsf_free(h->tsf);
  h->tsf = nullptr;
  sfx_tsf_state* s = new sfx_tsf_state();
  s->G = G;
  s->K = K;
  s->Pg = (int)(nfl + nlin);
  s->Ph = d * G + d;
  s->beta = beta;
  s->g_loaded.assign(h->T, 0);
  s->hpg = AdamHP{lr_g, wd_g, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  s->hph = AdamHP{lr_h, wd_h, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  const int T = h->T, R2 = 2 * B;
  const size_t sizes[14] = {(size_t)T * s->Pg, (size_t)T * s->Pg, (size_t)T * s->Pg, (size_t)s->Ph,
                            (size_t)T * s->Ph, (size_t)T * s->Ph, (size_t)(K + 1) * R2 * np, (size_t)std::max(K, 1) * ((R2 + TSF_FR - 1) / TSF_FR * TSF_FR),
                            (size_t)R2 * G, (size_t)B * d, (size_t)std::max(K, 1) * R2 * tsf_pst((int)np),
                            (size_t)((s->Pg + s->Ph + d + 63) & ~63) + TSF_SCR,
                            (size_t)T * std::max(K, 1) * tsf_fst((int)np),
                            (size_t)np * g4 + (size_t)G * ((d + 3) & ~3)};
  float** ptrs[14] = {&s->g,  &s->gm,    &s->gv,   &s->hp,   &s->hm,   &s->hv,  &s->zs,
                      &s->ts, &s->gfeat, &s->tphi, &s->part, &s->snap, &s->gch, &s->bimg};
  for (int i = 0; i < 14; ++i) {
    const size_t bytes = sizeof(float) * ((sizes[i] + 63) & ~(size_t)63);
    if (hipMalloc((void**)ptrs[i], bytes) != hipSuccess || hipMemset(*ptrs[i], 0, bytes) != hipSuccess) {
      tsf_free(s);
      SFX_FAIL(SFX_E_HIP, "sfx_tsf_setup: hipMalloc failed");
    }
  }
  h->tsf = s;
  clear_graphs(h);
  return SFX_OK;
}

int sfx_tsf_freeze_flows(sfx_t h, int freeze) {
  RC(settle(h));
  if (!h || !h->tsf) SFX_FAIL(SFX_E_ARG, "sfx_tsf_freeze_flows: call sfx_tsf_setup first");
  if (h->tsf->freeze_flows != (freeze != 0)) {
    HIPCHK(hipStreamSynchronize(h->stream));
    h->tsf->freeze_flows = freeze != 0;
    clear_graphs(h);  // the captured updates carry the flows' Adam hyper-parameters
  }
  return SFX_OK;
}

int sfx_tsf_load_g(sfx_t h, int t, const float* g_host) {
  RC(settle(h));
  if (!h || !h->tsf || !valid_head(h, t) || !g_host) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  touch(h);
  HIPCHK(hipMemcpyAsync(h->tsf->g + (size_t)t * h->tsf->Pg, g_host, sizeof(float) * h->tsf->Pg,
                        hipMemcpyHostToDevice, h->stream));
  RC(tsf_pack_chain(h, t));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tsf->g_loaded[t] = 1;
  return SFX_OK;
}

int sfx_tsf_get_g(sfx_t h, int t, float* g_host, float* gm_host, float* gv_host) {
  RC(settle(h));
  if (!h || !h->tsf || !valid_head(h, t)) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  const size_t o = (size_t)t * h->tsf->Pg, n = sizeof(float) * h->tsf->Pg;
  if (g_host) HIPCHK(hipMemcpyAsync(g_host, h->tsf->g + o, n, hipMemcpyDeviceToHost, h->stream));
  if (gm_host) HIPCHK(hipMemcpyAsync(gm_host, h->tsf->gm + o, n, hipMemcpyDeviceToHost, h->stream));
  if (gv_host) HIPCHK(hipMemcpyAsync(gv_host, h->tsf->gv + o, n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SFX_OK;
}

// g_t with its Adam moments (checkpoint resume)
int sfx_tsf_load_g_state(sfx_t h, int t, const float* g_host, const float* gm_host, const float* gv_host) {
  RC(settle(h));
  if (!h || !h->tsf || !valid_head(h, t) || !g_host || !gm_host || !gv_host)
    SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  const size_t o = (size_t)t * h->tsf->Pg, n = sizeof(float) * h->tsf->Pg;
  touch(h);
  HIPCHK(hipMemcpyAsync(h->tsf->g + o, g_host, n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tsf->gm + o, gm_host, n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tsf->gv + o, gv_host, n, hipMemcpyHostToDevice, h->stream));
  RC(tsf_pack_chain(h, t));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tsf->g_loaded[t] = 1;
  return SFX_OK;
}

// task t's Adam moments of the shared h (each task's optimizer keeps its own, tsfdqn.py:255-270)
int sfx_tsf_get_h_state(sfx_t h, int t, float* hm_host, float* hv_host) {
  RC(settle(h));
  if (!h || !h->tsf || !valid_head(h, t)) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  const size_t o = (size_t)t * h->tsf->Ph, n = sizeof(float) * h->tsf->Ph;
  if (hm_host) HIPCHK(hipMemcpyAsync(hm_host, h->tsf->hm + o, n, hipMemcpyDeviceToHost, h->stream));
  if (hv_host) HIPCHK(hipMemcpyAsync(hv_host, h->tsf->hv + o, n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SFX_OK;
}

int sfx_tsf_load_h_state(sfx_t h, int t, const float* hm_host, const float* hv_host) {
  RC(settle(h));
  if (!h || !h->tsf || !valid_head(h, t) || !hm_host || !hv_host) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  const size_t o = (size_t)t * h->tsf->Ph, n = sizeof(float) * h->tsf->Ph;
  touch(h);
  HIPCHK(hipMemcpyAsync(h->tsf->hm + o, hm_host, n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->tsf->hv + o, hv_host, n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SFX_OK;
}

int sfx_tsf_load_h(sfx_t h, const float* h_host) {
  RC(settle(h));
  if (!h || !h->tsf || !h_host) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  touch(h);
  HIPCHK(hipMemcpyAsync(h->tsf->hp, h_host, sizeof(float) * h->tsf->Ph, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->tsf->h_loaded = true;
  return SFX_OK;
}

int sfx_tsf_get_h(sfx_t h, float* h_host) {
  RC(settle(h));
  if (!h || !h->tsf || !h_host) SFX_FAIL(SFX_E_ARG, "bad args (sfx_tsf_setup first)");
  HIPCHK(hipMemcpyAsync(h_host, h->tsf->hp, sizeof(float) * h->tsf->Ph, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return SFX_OK;
}

int sfx_tsf_update(sfx_t h, int policy, const float* S, const int64_t* a, const float* r, const float* phi,
                   const float* S1, const float* gamma, int B, int use_gpi, float* losses, int64_t* next) {
  RC(settle(h));
  if (!h || !h->tsf) SFX_FAIL(SFX_E_ARG, "sfx_tsf_update: call sfx_tsf_setup first");
  if (!valid_head(h, policy) || !S || !a || !r || !phi || !S1 || !gamma || !losses) SFX_FAIL(SFX_E_ARG, "bad args");
  if (B < 1 || B > h->Mmax) SFX_FAIL(SFX_E_ARG, "batch exceeds max_batch");
  use_gpi = use_gpi ? 1 : 0;
  const GraphKey key = make_key(20, {policy, use_gpi, B}, h->mask, {S, a, r, phi, S1, gamma, losses, next});
  RC(run_graph(h, key, [&]() -> int { return tsf_body(h, policy, S, a, r, phi, S1, gamma, B, use_gpi, losses, next); }));
  h->mask ^= 1ull << policy;
  after_update(h, policy);
  return maybe_sync_target(h, policy);
}

// ---- TSF-DQN with the heads sharded across ranks (BASELINE config C5; DESIGN.md §7) ----
// The active policy i lives on one rank (its owner); w (T_glob rows) and h are replicated.
//   sfx_shard_tsf_maxima(i, S1, X)   every rank: X[b][a] = max over its heads of ψ_t(s1_b)[a]·w_i
//     all_reduce(X, MAX)             (use_gpi = 0: the owner alone, own head, no all-reduce)
//   sfx_shard_tsf_update(i, ..., X)  the owner: TSFDQN.update_successor with next actions argmax_a X
//   sfx_shard_tsf_shared(i, buf, 0)  the owner packs h and w_i; broadcast from the owner;
//   sfx_shard_tsf_shared(i, buf, 1)  the others unpack (h's Adam moments are per task: owner-local)
//   sfx_shard_tsf_select(s, task, key)  this rank's best (q, t, a) for the env action
//     all_reduce(key, MAX)
int sfx_shard_tsf_maxima(sfx_t h, int policy, const float* S1, int B, int own_only, int32_t* X) {
  RC(settle(h));
  if (!h || !h->tsf || !S1 || !X || policy < 0 || policy >= h->Tg || B < 1 || B > h->Mmax)
    SFX_FAIL(SFX_E_ARG, "bad args (sfx_shard_setup and sfx_tsf_setup first)");
  const int loc = policy - h->off;
  if (own_only && (loc < 0 || loc >= h->T)) SFX_FAIL(SFX_E_ARG, "own_only on a rank that does not own the policy");
  const GraphKey key = make_key(22, {policy, B, own_only ? 1 : 0}, h->mask, {S1, X});
  return run_graph(h, key, [&]() -> int {
    if (own_only)
      RC(run_fwd(h, {{R_S1, P_ONLINE, 1, loc, 1}}, B, S1, nullptr));
    else
      RC(run_fwd(h, {{R_S1, P_ONLINE, 1, 0, h->T}}, B, S1, nullptr));
    const int TA = (own_only ? 1 : h->T) * h->A;
    QmaxArgs Q{};
    Q.M = B;
    Q.Tg = h->Tg;
    Q.off = h->off;
    Q.guess = R_S1;
    Q.rows = TA >= 256 ? 1 : std::min(B, 256 / TA);
    Q.pol0 = policy;
    Q.tsel = own_only ? loc : -1;
    Q.X = X;
    launch(h, K_VER, 4.0 * B * ((double)TA * h->d + h->A) + 4.0 * h->d, k_qmax, dim3(1, cdiv(B, Q.rows)), dim3(256),
           h->G, Q);
    LAUNCHCHK();
    return SFX_OK;
  });
}

int sfx_shard_tsf_update(sfx_t h, int policy, const float* S, const int64_t* a, const float* r, const float* phi,
                         const float* S1, const float* gamma, int B, const int32_t* X, float* losses) {
  RC(settle(h));
  if (!h || !h->tsf) SFX_FAIL(SFX_E_ARG, "sfx_shard_tsf_update: call sfx_tsf_setup first");
  const int loc = policy - h->off;
  if (loc < 0 || loc >= h->T) SFX_FAIL(SFX_E_ARG, "sfx_shard_tsf_update: this rank does not own the policy");
  if (!S || !a || !r || !phi || !S1 || !gamma || !X || !losses) SFX_FAIL(SFX_E_ARG, "bad args");
  if (B < 1 || B > h->Mmax) SFX_FAIL(SFX_E_ARG, "batch exceeds max_batch");
  const GraphKey key = make_key(23, {loc, B}, h->mask, {S, a, r, phi, S1, gamma, X, losses});
  RC(run_graph(h, key, [&]() -> int { return tsf_body(h, loc, S, a, r, phi, S1, gamma, B, 1, losses, nullptr, X); }));
  h->mask ^= 1ull << loc;
  after_update(h, loc);
  return maybe_sync_target(h, loc);
}

int sfx_shard_tsf_shared(sfx_t h, int policy, float* buf, int unpack) {
  RC(settle(h));
  if (!h || !h->tsf || !buf || policy < 0 || policy >= h->Tg) SFX_FAIL(SFX_E_ARG, "bad args");
  const size_t nh = sizeof(float) * h->tsf->Ph, nw = sizeof(float) * h->d;
  float* w = h->w + (size_t)policy * h->dpad;
  if (unpack) {
    touch(h);
    HIPCHK(hipMemcpyAsync(h->tsf->hp, buf, nh, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(w, buf + h->tsf->Ph, nw, hipMemcpyDeviceToDevice, h->stream));
  } else {
    HIPCHK(hipMemcpyAsync(buf, h->tsf->hp, nh, hipMemcpyDeviceToDevice, h->stream));
    touch(h);
    HIPCHK(hipMemcpyAsync(buf + h->tsf->Ph, w, nw, hipMemcpyDeviceToDevice, h->stream));
  }
  return SFX_OK;
}

int sfx_shard_tsf_select(sfx_t h, const float* s, int task, int use_gpi, long long* key_out) {
  RC(settle(h));
  if (!h || !s || !key_out || task < 0 || task >= h->Tg) SFX_FAIL(SFX_E_ARG, "bad args");
  use_gpi = use_gpi ? 1 : 0;
  const GraphKey key = make_key(24, {task, use_gpi}, h->mask, {s, key_out});
  return run_graph(h, key, [&]() -> int {
    RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}}, 1, s, nullptr));
    KeyArgs K{};
    K.role = R_A;
    K.row = 0;
    K.task = task;
    K.use_gpi = use_gpi;
    K.off = h->off;
    K.key = key_out;
    hipLaunchKernelGGL(k_skey, dim3(1), dim3(256), 0, h->stream, h->G, K);
    LAUNCHCHK();
    return SFX_OK;
  });
}

}  // extern "C"

// ---- the sharded TSF step of the native runner (schedule "sharded_tsf"; BASELINE config C5) ----
// One env step of TSF-DQN's train_agent (tsfdqn_nf.py:598-612) with the heads split over the ranks,
// every collective enqueued on the step stream (captured with the step's graph under RCCL):
//   gate -> [minibatch] forward of S1 through this rank's heads -> k_qmax: the active policy's GPI
//   maxima over them -> all-reduce(MAX) -> the owner of the active task: TSFDQN.update_successor
//   with next actions argmax_a of the maxima (tsf_body, xmax) -> h ++ w_task from the owner (one
//   all-reduce over raw bits, k_tsx_*) -> forward of s_next through this rank's (post-update) heads
//   -> k_ssel: this rank's slice of the q table with the NEW w_task -> all-reduce(MAX) ->
//   k_sfinish: the env action, published.  use_gpi = 0 (own-ψ next actions): the owner's update
//   alone, no maxima.  (The table cannot ride in the h / w_task all-reduce: the other ranks'
//   slices need the updated w_task first.)
namespace {

int shard_tsf_buffers(sfx_handle* h) {
  if (!h->tsf) SFX_FAIL(SFX_E_STATE, "sharded_tsf: call sfx_tsf_setup first");
  for (int*& p : {std::ref(h->tsx), std::ref(h->tsz)}) {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  HIPCHK(hipMalloc((void**)&h->tsx, sizeof(int) * (size_t)h->Mmax * h->A));
  HIPCHK(hipMalloc((void**)&h->tsz, sizeof(int) * ((size_t)h->tsf->Ph + h->d + (size_t)h->Tg * h->A)));
  return SFX_OK;
}

// pre: the previous step's look-ahead (select_ahead_body) forwarded this minibatch -- ψ(S1) of this
// rank's heads and, on the owner, ψ(S), ψ⁻(S1) and the TSF forward of the active head; ahead: this
// step's selection forwards the next one's
int shard_tsf_body(sfx_runner* R, bool have, bool pre, bool ahead) {
  sfx_handle* h = R->h;
  const auto at = [&](size_t off) { return reinterpret_cast<const float*>(R->dst + off); };
  const int loc = own_loc(R), B = R->B;  // (runner_body launched the step's gate)
  if (have) {
    const float* S1 = at(R->lay.s1);
    if (R->upd_use_gpi) {
      if (!pre) RC(run_fwd(h, {{R_S1, P_ONLINE, 1, 0, h->T}}, B, S1, nullptr));
      QmaxArgs Q{};
      Q.M = B;
      Q.Tg = h->Tg;
      Q.off = h->off;
      Q.guess = R_S1;
      const int TA = h->T * h->A;
      Q.rows = TA >= 256 ? 1 : std::min(B, 256 / TA);
      Q.pol0 = R->task;
      Q.tsel = -1;
      Q.X = h->tsx;
      launch(h, K_VER, 4.0 * B * ((double)TA * h->d + h->A) + 4.0 * h->d, k_qmax, dim3(1, cdiv(B, Q.rows)), dim3(256),
             h->G, Q);
      LAUNCHCHK();
      RC(coll_max(h, h->tsx, (size_t)B * h->A));
    }
    if (loc >= 0)
      RC(tsf_body(h, loc, at(R->lay.s), reinterpret_cast<const int64_t*>(R->dst + R->lay.a), at(R->lay.rb),
                  at(R->lay.phi), S1, at(R->lay.gamma), B, R->upd_use_gpi, R->dloss, nullptr,
                  R->upd_use_gpi ? h->tsx : nullptr, pre));
  }
  // h and w_task from the owner to every rank (the next step's maxima and the env action below
  // read w_task; the owner of a later active task reads h)
  const int nsh = h->tsf->Ph + h->d;
  TsxArgs X{};
  X.nsh = nsh;
  X.Ph = h->tsf->Ph;
  X.own = loc >= 0 ? 1 : 0;
  X.hp = h->tsf->hp;
  X.w = h->w + (size_t)R->task * h->dpad;
  X.z = h->tsz;
  X.cancel = h->dcancel;
  launch(h, K_VER, 4.0 * 2.0 * nsh, k_tsx_pack, dim3(cdiv(nsh, 256)), dim3(256), X);
  LAUNCHCHK();
  RC(coll_max(h, h->tsz, (size_t)nsh));
  launch(h, K_VER, 4.0 * 2.0 * nsh, k_tsx_unpack, dim3(cdiv(nsh, 256)), dim3(256), X);
  LAUNCHCHK();
  // the env action for s_next (SF.GPI with w_task over every head, tsfdqn.py get_Q_values): this
  // rank's slice of the q table, all-reduced, picked and published by k_sfinish
  int* q = h->tsz + nsh;
  const std::function<int()> pick = [&]() -> int {
    SselArgs S{};
    S.role = R_A;
    S.row = 0;
    S.task = R->task;
    S.use_gpi = R->sel_use_gpi;
    S.off = h->off;
    S.Tg = h->Tg;
    S.q = q;
    launch(h, K_VER, 4.0 * h->T * h->O + 4.0 * h->Tg * h->A, k_ssel, dim3(cdiv(h->Tg * h->A, 256)), dim3(256), h->G,
           S);
    LAUNCHCHK();
    RC(coll_max(h, q, (size_t)h->Tg * h->A));
    SfinArgs F{};
    F.X = nullptr;  // no speculation: flag = T_glob
    F.Y = nullptr;
    F.q = q;
    F.Tg = h->Tg;
    F.M = 0;
    F.A = h->A;
    F.flag = &h->dout->flag;
    F.sel = h->dout->sel;
    F.pub = R->res;
    F.nonfin = h->G.nonfin;
    F.stall = nullptr;
    F.dctr = R->dctr;
    F.cancel = h->dcancel;
    launch(h, K_VER, 4.0 * h->Tg * h->A, k_sfinish, dim3(1), dim3(1024), F);
    LAUNCHCHK();
    return SFX_OK;
  };
  // the selection sees the post-update heads: the owner's update flips its slot
  const unsigned long long saved = h->mask;
  if (have && loc >= 0) h->mask ^= 1ull << loc;
  int rc;
  if (ahead)
    rc = select_ahead_body(h, at(R->lay.snext), at(R->lay.ax), at(R->lay.axphi), B, loc, R->sel_use_gpi, nullptr,
                           nullptr, &pick);
  else {
    rc = run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}}, 1, at(R->lay.snext), nullptr);
    if (rc == SFX_OK) rc = pick();
  }
  h->mask = saved;
  return rc;
}

}  // namespace

// ---- TSF test tasks (SURVEY §8f rank 1; kernels and math: sfx_tsf.h k_tsf_test_*) ------------

namespace {

TsfTestArgs tsf_test_args(sfx_handle* h) {
  TsfTestArgs A{};
  A.T = h->T;
  A.n_s = h->n_s;
  A.G = h->tsf->G;
  A.K = h->tsf->K;
  A.A = h->A;
  A.d = h->d;
  A.O = h->O;
  A.Pg = h->tsf->Pg;
  A.lastOff = h->actOff[h->NL - 1];
  A.actSize = h->actSize;
  A.g = h->tsf->g;
  A.hp = h->tsf->hp;
  return A;
}

int tsf_test_ok(sfx_handle* h) {
  if (!h || !h->tsf) SFX_FAIL(SFX_E_ARG, "sfx_tsf_test_*: call sfx_tsf_setup first");
  if (h->Tg != h->T || h->T > 64 || h->d > 256 || h->tsf->G > 512 || h->A > 256)
    SFX_FAIL(SFX_E_ARG, "sfx_tsf_test_*: needs an unsharded handle, T <= 64, d <= 256, G <= 512, A <= 256");
  return SFX_OK;
}

// ---- the TSF agent's test phase in the runner (sfx_runner_tsf_test_phase, sfx_runner.inc) ----

// the handle's part of the phase's preconditions; sizes the g-feature scratch for E rows (never inside a capture)
int tsf_test_phase_ready(sfx_handle* h, int E) {
  if (!h->tsf) SFX_FAIL(SFX_E_STATE, "sfx_runner_tsf_test_phase: call sfx_tsf_setup first (and load every g_t and h)");
  sfx_tsf_state* ts = h->tsf;
  if (h->Tg != h->T) SFX_FAIL(SFX_E_STATE, "sfx_runner_tsf_test_phase: needs an unsharded handle");
  if (h->T > 64 || h->d > 256 || ts->G > 512 || h->A > 256)
    SFX_FAIL(SFX_E_ARG, "sfx_runner_tsf_test_phase: needs T <= 64, d <= 256, G <= 512, A <= 256");
  for (int t = 0; t < h->T; ++t)
    if (!ts->g_loaded[t])
      SFX_FAIL(SFX_E_STATE, "sfx_runner_tsf_test_phase: g of task " + std::to_string(t) + " was never loaded (sfx_tsf_load_g)");
  if (!ts->h_loaded) SFX_FAIL(SFX_E_STATE, "sfx_runner_tsf_test_phase: h was never loaded (sfx_tsf_load_h)");
  if (E > h->Mmax)
    SFX_FAIL(SFX_E_ARG, "sfx_runner_tsf_test_phase: E = " + std::to_string(E) + " test tasks, needs 1 <= E <= min(" +
                            std::to_string(TEST_EMAX) + ", max_batch = " + std::to_string(h->Mmax) + ")");
  if (ts->tgf_rows < E) {
    HIPCHK(hipStreamSynchronize(h->stream));
    if (ts->tgf) HIPCHK(hipFree(ts->tgf));
    ts->tgf = nullptr;
    ts->tgf_rows = 0;
    HIPCHK(hipMalloc((void**)&ts->tgf, sizeof(float) * 2 * (size_t)E * h->T * ts->G));
    ts->tgf_rows = E;
  }
  return SFX_OK;
}

const void* tsf_test_phase_tgf(sfx_handle* h) { return h->tsf ? h->tsf->tgf : nullptr; }

// One lockstep step's launches on h->stream, a linear chain: intake; ψ(S) -> R_A, ψ(S1) -> R_V (online) and
// ψ⁻(S1) -> R_G in one forward (none of them a role the look-ahead carries: R_NS* and the minibatch copy
// R_S*); the g features of S / S1; the row kernel; the publication.
int tsf_test_phase_body(sfx_runner* R, int E, int horizon, float* W, int w_stride, float* Om, int o_stride, float* mom,
                        int mom_stride) {
  sfx_handle* h = R->h;
  sfx_tsf_state* ts = h->tsf;
  const sfx_runner::TestPhaseBufs& tb = R->tp[sfx_runner::TP_TSF];
  const TestStageLayout L = tsf_test_stage_layout(h->n_s, h->d);
  const TsfTestDevLayout D = tsf_test_dev_layout(h->n_s, h->d);
  uint8_t* blk = tb.blk;
  TsfTestIntakeArgs I{};
  I.stage = tb.st;
  I.off_phi = L.phi;
  I.off_s1 = L.s1;
  I.E = E;
  I.d = h->d;
  I.n_s = h->n_s;
  I.horizon = horizon;
  I.hdr = reinterpret_cast<TsfTestDevHdr*>(blk + D.hdr);
  I.live = reinterpret_cast<int*>(blk + D.live);
  I.a = reinterpret_cast<int64_t*>(blk + D.a);
  I.a1x = reinterpret_cast<int*>(blk + D.a1x);
  I.rowp = reinterpret_cast<float*>(blk + D.rowp);
  I.phi = reinterpret_cast<float*>(blk + D.phi);
  I.S = reinterpret_cast<float*>(blk + D.S);
  I.S1 = reinterpret_cast<float*>(blk + D.S1);
  I.dseq = R->tdseq;
  hipLaunchKernelGGL(k_tsf_test_intake, dim3(1), dim3(256), 0, h->stream, I);
  LAUNCHCHK();
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}, {R_V, P_ONLINE, 2, 0, h->T}, {R_G, P_TARGET, 2, 0, h->T}}, E, I.S, I.S1));
  TsfTestArgs A = tsf_test_args(h);
  A.s = I.S;
  A.s1 = I.S1;
  A.gfeat = ts->tgf;
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.psi1 = h->act + (size_t)R_G * h->T * h->actSize;
  A.phi = I.phi;
  A.a = I.a;
  A.w = W;
  A.omega = Om;
  A.mom = mom;
  A.w_stride = w_stride;
  A.o_stride = o_stride;
  A.mom_stride = mom_stride;
  A.rowp = I.rowp;
  A.step = 1;  // per row from rowp
  A.hpw = AdamHP{0.0, 0.0, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.hpo = A.hpw;
  launch(h, K_TSF, 4.0 * E * ((double)h->T * ts->Pg + 2.0 * h->T * ts->G), k_tsf_test_g, dim3(h->T, E), dim3(64), A);
  LAUNCHCHK();
  TsfTestRowArgs X{};
  X.hdr = I.hdr;
  X.live = I.live;
  X.a1x = I.a1x;
  X.psi_s1 = h->act + (size_t)R_V * h->T * h->actSize;
  X.loss = tb.loss;
  X.sel = R->tsel;
  X.E = E;
  X.horizon = horizon;
  launch(h, K_TSF, 4.0 * E * (3.0 * h->T * h->O + 2.0 * h->T * ts->G + ts->Ph + 6.0 * (h->d + h->T)), k_tsf_test_row,
         dim3(E), dim3(256), A, X);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_test_publish, dim3(1), dim3(128), 0, h->stream, (const int64_t*)R->tsel, E,
                     (const long long*)R->tdseq, R->tres);
  LAUNCHCHK();
  return SFX_OK;
}

}  // namespace

extern "C" {

int sfx_tsf_test_action(sfx_t h, const float* s, const float* w, const float* omega, int64_t* a_out) {
  RC(settle(h));
  RC(tsf_test_ok(h));
  if (!s || !w || !omega || !a_out) SFX_FAIL(SFX_E_ARG, "null argument");
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}}, 1, s, nullptr));
  TsfTestArgs A = tsf_test_args(h);
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.w = const_cast<float*>(w);
  A.omega = const_cast<float*>(omega);
  A.act_out = a_out;
  launch(h, K_GPI, 4.0 * ((double)h->T * h->O + h->d + h->T), k_tsf_test_act, dim3(1), dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_tsf_test_update(sfx_t h, const float* s, const float* s1, const int64_t* a, const int64_t* a1, float r,
                        const float* phi, float* w, float* omega, float* adam_state, int step, float gamma,
                        float beta, float lasso, float lr_w, float wd_w, float lr_omega, float wd_omega,
                        float* losses) {
  RC(settle(h));
  RC(tsf_test_ok(h));
  if (!s || !s1 || !a || !a1 || !phi || !w || !omega || !adam_state || !losses || step < 1)
    SFX_FAIL(SFX_E_ARG, "bad args");
  sfx_tsf_state* ts = h->tsf;
  if (!ts->tgf) {
    HIPCHK(hipMalloc((void**)&ts->tgf, sizeof(float) * 2 * (size_t)h->T * ts->G));
    ts->tgf_rows = 1;
  }
  // ψ_t(s) of the online heads and ψ⁻_t(s1) of the target heads, one forward for both
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}, {R_G, P_TARGET, 2, 0, h->T}}, 1, s, s1));
  TsfTestArgs A = tsf_test_args(h);
  A.s = s;
  A.s1 = s1;
  A.gfeat = ts->tgf;
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.psi1 = h->act + (size_t)R_G * h->T * h->actSize;
  A.phi = phi;
  A.a = a;
  A.a1 = a1;
  A.r = r;
  A.gamma = gamma;
  A.beta = beta;
  A.lasso = lasso;
  A.w = w;
  A.omega = omega;
  A.mom = adam_state;
  A.step = step;
  A.hpw = AdamHP{lr_w, wd_w, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.hpo = AdamHP{lr_omega, wd_omega, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.losses = losses;
  launch(h, K_TSF, 4.0 * ((double)h->T * ts->Pg + 2.0 * h->T * ts->G), k_tsf_test_g, dim3(h->T), dim3(64), A);
  LAUNCHCHK();
  launch(h, K_TSF, 4.0 * (2.0 * h->T * h->O + 2.0 * h->T * ts->G + ts->Ph + 6.0 * (h->d + h->T)), k_tsf_test_step,
         dim3(1), dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

// Lockstep test phase (agents/tsfdqn_sequential.py:392-433 for E test tasks at once): one launch
// set chooses the E greedy actions, one launch set fits the E reward models; row e of every
// launch is test task e (TsfTestArgs::rowp and the row strides, sfx_tsf.h tsf_test_row).
int sfx_tsf_test_actions(sfx_t h, const float* S, int E, const float* W, int w_stride, const float* Omega,
                         int o_stride, int64_t* a_out) {
  RC(settle(h));
  RC(tsf_test_ok(h));
  if (!S || !W || !Omega || !a_out || E < 1 || w_stride < h->d || o_stride < h->T) SFX_FAIL(SFX_E_ARG, "bad args");
  if (E > h->Mmax) SFX_FAIL(SFX_E_ARG, "sfx_tsf_test_actions: E exceeds max_batch");
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}}, E, S, nullptr));
  TsfTestArgs A = tsf_test_args(h);
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.w = const_cast<float*>(W);
  A.omega = const_cast<float*>(Omega);
  A.w_stride = w_stride;
  A.o_stride = o_stride;
  A.act_out = a_out;
  launch(h, K_GPI, 4.0 * E * ((double)h->T * h->O + h->d + h->T), k_tsf_test_act, dim3(E), dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

int sfx_tsf_test_updates(sfx_t h, int E, const float* S, const float* S1, const int64_t* a, const int64_t* a1,
                         const float* phi, float* W, int w_stride, float* Omega, int o_stride, float* adam_state,
                         int mom_stride, const float* rowp, float gamma, float beta, float lasso, float* losses) {
  RC(settle(h));
  RC(tsf_test_ok(h));
  if (!S || !S1 || !a || !a1 || !phi || !W || !Omega || !adam_state || !rowp || !losses || E < 1 ||
      w_stride < h->d || o_stride < h->T || mom_stride < 2 * (h->d + h->T))
    SFX_FAIL(SFX_E_ARG, "bad args");
  if (E > h->Mmax) SFX_FAIL(SFX_E_ARG, "sfx_tsf_test_updates: E exceeds max_batch");
  sfx_tsf_state* ts = h->tsf;
  if (ts->tgf_rows < E) {
    if (ts->tgf) HIPCHK(hipFree(ts->tgf));
    ts->tgf = nullptr;
    HIPCHK(hipMalloc((void**)&ts->tgf, sizeof(float) * 2 * (size_t)E * h->T * ts->G));
    ts->tgf_rows = E;
  }
  RC(run_fwd(h, {{R_A, P_ONLINE, 1, 0, h->T}, {R_G, P_TARGET, 2, 0, h->T}}, E, S, S1));
  TsfTestArgs A = tsf_test_args(h);
  A.s = S;
  A.s1 = S1;
  A.gfeat = ts->tgf;
  A.psi = h->act + (size_t)R_A * h->T * h->actSize;
  A.psi1 = h->act + (size_t)R_G * h->T * h->actSize;
  A.phi = phi;
  A.a = a;
  A.a1 = a1;
  A.gamma = gamma;
  A.beta = beta;
  A.lasso = lasso;
  A.w = W;
  A.omega = Omega;
  A.mom = adam_state;
  A.w_stride = w_stride;
  A.o_stride = o_stride;
  A.mom_stride = mom_stride;
  A.rowp = rowp;
  A.step = 1;  // per row from rowp
  A.hpw = AdamHP{0.0, 0.0, h->hp_psi.b1, h->hp_psi.b2, h->hp_psi.eps};
  A.hpo = A.hpw;
  A.losses = losses;
  launch(h, K_TSF, 4.0 * E * ((double)h->T * ts->Pg + 2.0 * h->T * ts->G), k_tsf_test_g, dim3(h->T, E), dim3(64), A);
  LAUNCHCHK();
  launch(h, K_TSF, 4.0 * E * (2.0 * h->T * h->O + 2.0 * h->T * ts->G + ts->Ph + 6.0 * (h->d + h->T)),
         k_tsf_test_step, dim3(E), dim3(256), A);
  LAUNCHCHK();
  return SFX_OK;
}

}  // extern "C"
