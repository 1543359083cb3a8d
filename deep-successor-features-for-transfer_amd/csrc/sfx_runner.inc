// sfx_runner.inc -- native env-step loop of SF-DQN / TSF-DQN (included by sfx.hip).
//
// One env step is one iteration of Agent.next_sample (agents/agent.py:195-261) with one of
// the reference's training schedules (sfx_runner_config):
//   all    (default) agents/sfdqn.py:39-60 (main_sfdqn_torch.py): GPI action for the current
//          state (computed by the previous step's graph), ε-greedy, env transition, LMS reward
//          fit (features/successor.py:146-167), replay append + uniform minibatch
//          (agents/buffer.py:34-82), every head's ψ update in the reference's order;
//   active sfdqn.py:462-471 / agents/sfdqn_sequential.py:63-76: only the active task's head is
//          updated (l1 + l2, Adam-trained w), no LMS;
//   tsf    tsfdqn.py:566-580 / tsfdqn_nf.py:598-612: TSFDQN.update_successor of the active task.
//   phi    agents/sfdqn_phi.py:80-109 over features/deep_phi.py: GPI with the active task's biased reward
//          model (q = ψ·w + b), ε-greedy, env transition, append (the env's φ is not used), replay,
//          DeepSF_PHI.update_successor of the active head (phi_update_body, sfx_phi.inc);
//   tsf_phi agents/tsfdqn_phi.py:80-103 over features/deep_tsf_phi.py: the same loop with
//          TSFDQN_PHI.update_deep_models (φ̃ = φ ⊙ t, g_i and h plain Linears).
//          Both step the φ net, w_i, its bias, λ_i (and g_i, h) in place, so every one of their kernels
//          honours the gate's cancel word; no look-ahead and no device replay yet.
// sfx_runner_featurizer (active and tsf): a frozen pre-trained φ net (sfx_pre_t); each step with an update
// recomputes its minibatch's φ rows from (s, a, s1) with k_pre_rows between the gate and the update -- the
// main phase of sfdqn_phi.py / tsfdqn_phi.py.  The staged φ rows and the env's φ are then never read.
// The env and the replay ring stay on the host (north_star); the device work of a step is one
// hipGraph: k_gate -> the step's update -> the action for the next state -> publish.
//
// Pipelining: right after releasing step j, the host launches ONE graph holding steps j+1 ..
// j+span (span <= 8, fewer before a target sync or the end of the run); each step's k_gate
// waits on the device until the host has written that step's inputs.  The host therefore never
// pays a graph launch or a host->device copy on the critical path: it spins on step j's
// published result, runs the env and the replay, writes the inputs and bumps `go`.
// Steps whose speculation failed on the device (flag < T) finish with host-driven rounds on a
// side stream while the next graph's gate keeps waiting; a step that ends with a target-net
// sync (every target_update_ev updates) is not pipelined, so the copy lands in stream order.

namespace {

// Staging record of one step: the minibatch [s .. rb], then the tail the host writes every
// step [snext .. tr_meta] (with device replay only the tail crosses PCIe).
enum { RUN_ALL = 0, RUN_ACTIVE = 1, RUN_TSF = 2, RUN_SHARD = 3, RUN_SHARD_TSF = 4, RUN_PHI = 5, RUN_TSF_PHI = 6 };
constexpr int RUN_SCHEDULES = 8;  // graph-key factor: room for every schedule above

struct RunnerLayout {
  size_t s, s1, phi, a, gamma, snext, phi1, r1, rb, bytes;
  size_t tr_s, tr_s1, tr_phi, tr_meta;  // this step's transition (device replay)
  size_t ax;     // look-ahead: the next step's minibatch states [S | S1] (2 B n_s floats)
  size_t axphi;  // look-ahead, TSF: the next step's minibatch φ rows (B d floats), the last field
  // end of what a step hands over (look-ahead: with the block of its schedule)
  size_t end(bool ahead, int schedule) const {
    return !ahead ? ax : schedule == RUN_TSF || schedule == RUN_SHARD_TSF ? bytes : axphi;
  }
};


RunnerLayout runner_layout(int B, int n_s, int d) {
  RunnerLayout L{};
  size_t off = 0;
  auto take = [&](size_t n) {
    const size_t o = off;
    off += (n + 15) / 16 * 16;
    return o;
  };
  L.s = take(sizeof(float) * B * n_s);
  L.s1 = take(sizeof(float) * B * n_s);
  L.phi = take(sizeof(float) * B * d);
  L.a = take(sizeof(int64_t) * B);
  L.gamma = take(sizeof(float) * B);
  L.rb = take(sizeof(float) * B);
  L.snext = take(sizeof(float) * n_s);
  L.phi1 = take(sizeof(float) * d);
  L.r1 = take(sizeof(float));
  L.tr_s = take(sizeof(float) * n_s);
  L.tr_s1 = take(sizeof(float) * n_s);
  L.tr_phi = take(sizeof(float) * d);
  L.tr_meta = take(sizeof(ReplayMeta));
  L.ax = take(sizeof(float) * 2 * B * n_s);  // pushed / copied only by look-ahead steps
  L.axphi = take(sizeof(float) * B * d);      // (TSF look-ahead steps only)
  L.bytes = off;
  return L;
}

}  // namespace

struct sfx_pre_handle;  // sfx_pre.inc
namespace {
int pre_rows_body(sfx_pre_handle* p, hipStream_t stream, const float* S, const int64_t* a, const float* S1, int M,
                  float* phi, const int* cancel);
void pre_dims(const sfx_pre_handle* p, int* n_s, int* d);
const char* const RUN_NAMES[] = {"all", "active", "tsf", "sharded", "sharded_tsf", "phi", "tsf_phi"};
}  // namespace

struct sfx_runner {
  sfx_handle* h = nullptr;
  // sfx_runner_featurizer: the frozen φ net whose forward of the staged minibatch replaces the staged φ rows
  // (active and TSF schedules); caller-owned
  sfx_pre_handle* feat = nullptr;
  int B = 32, cap = 0, ep_len = 500, sel_use_gpi = 1, pipeline = 1;
  int schedule = RUN_ALL, upd_use_gpi = 1;  // sfx_runner_config
  float gamma = 0.9f, eps = 0.1f, alpha_w = 1e-3f, p_end = 0.f;
  float* dloss = nullptr;  // device [DLOSS_N]: losses of the active-task update (read back by sfx_runner_phi_losses only)
  static constexpr int DLOSS_N = 16;
  float *phi_bias = nullptr, *phi_lam = nullptr;  // sfx_runner_phi_scalars: caller-owned device [T] each
  std::mt19937_64 rng;
  sfx_env_reset_fn env_reset = nullptr;
  sfx_env_step_fn env_step = nullptr;
  void* env_ctx = nullptr;
  // replay ring (host)
  std::vector<float> rs, rs1, rphi, rr, rgam;
  std::vector<int64_t> ra;
  long rsize = 0, ridx = 0;
  // device-resident replay (sfx_runner_device_replay): the ring in HBM, the host ring above
  // kept as its mirror (prefill, records)
  int dev_replay = 0;
  bool dring_dirty = true;  // host ring changed outside device-replay steps: upload before a run
  float *drs = nullptr, *drs1 = nullptr, *drphi = nullptr, *drr = nullptr, *drg = nullptr;
  long long* dra = nullptr;
  // staging: host-coherent inputs of the next step and their device twin
  RunnerLayout lay{};
  uint8_t* hst = nullptr;
  uint8_t* dst = nullptr;
  long long* go = nullptr;        // host-coherent: last step whose inputs are ready
  HostResult* res = nullptr;      // host-coherent: published results, a ring (RES_RING); err in slot 0
  HostResult* cur() const { return res + (inflight_seq & (RES_RING - 1)); }  // the in-flight step's
  long long* dctr = nullptr;      // device: last step a gate opened
  // push staging (pull -- host-coherent memory read across PCIe -- only when the fine-grained
  // allocation fails): the host copies the staged inputs into
  // fine-grained device memory through the BAR and bumps a go word there, so the gate polls and
  // copies from HBM instead of across PCIe (tools/pingpong.hip: copy 2.6 -> 0.8 µs for 6.9 KB)
  uint8_t* dpush = nullptr;
  long long* dgo = nullptr;
  hipStream_t side = nullptr;
  long long seq = 0;              // last step handed to the device
  // env state
  int task = 0, steps_in_ep = 0;
  std::vector<float> s, s1, phi;
  long long sel_c = 0, sel_a = 0;
  std::vector<long long> gpi_counters;
  // in-flight step / pre-launched graph
  bool inflight = false, inflight_have = false, inflight_lms = false;
  long long inflight_seq = 0;
  unsigned long long inflight_mask = 0;
  int pre_n = 0;          // steps whose graph is already launched behind the in-flight one
  bool pre_have = false;
  int span_max = 8;       // steps per pre-launched graph (DESIGN.md §10 v5.3: 16 measured no better)
  long long gate_timeout = 500000000LL;  // gate wait bound, 100 MHz ticks (sfx_runner_gate_timeout)
  double wait_bound = 10.0;  // host wait on a published result, s (sfx_runner_wait_timeout)
  bool broken = false;       // a drain after a timed-out step did not finish: every call fails
  std::string broken_why;
  long long retried = 0;  // steps issued again after their gate gave up on a slow host (in flight or queued)
  long long recomputed = 0;  // steps recomputed before host rounds (later steps ran over their buffers)
  // look-ahead (DESIGN.md §4, §5; host replay; SFX_AHEAD=0: off): step E's final round (all-task) or
  // its select (active / TSF) also forwards step E+1's minibatch, so step E+1 starts at its TD launch.  Minibatch indices come
  // from their own stream (irng), drawn ahead of time into `plans`: a step's plan is known when the
  // graph of the steps before it is launched.  A plan is "dirty" when it samples the slot its own
  // step's transition is appended to (that S1 row is unknown a step early): such a step runs its own
  // forward, and a pre-launched span ends before it.
  struct MbPlan {
    long long step;    // env step (env_steps at its iteration)
    long size, slot;   // replay size when it samples, slot of its step's transition
    bool dirty;        // samples `slot`
    bool early;        // drawn before its step's iteration (so the step before could forward it)
    std::vector<long> idx;
  };
  struct StepFlags {
    bool pre, ahead;
    int par;  // copy of the minibatch roles (Geo::mb / R_NS)
  };
  bool ahead_on = true;         // SFX_AHEAD
  bool ahead = false;           // this run's steps look ahead (runner_run decides)
  bool chain = false;           // the last issued step forwarded the next step's minibatch
  bool round_posted = false;    // the host round just launched posts its verdict (round_wait)
  unsigned long long chain_gen = 0;  // sfx_handle::gen when `chain` was set: a call on the handle in
                                     // between (weights, roles, engine launches) drops the chain
  std::mt19937_64 irng;
  std::deque<MbPlan> plans;
  std::deque<StepFlags> preq;   // flags of the pre-launched steps
  StepFlags inflight_fl{false, false, 0};
  long long pre_steps = 0, dirty_steps = 0;
  long long cur_step = 0;       // env step of the current iteration (its transition is in the ring)
  // stats
  long long env_steps = 0, prelaunched = 0, host_rounds = 0;
  long long nonfinite_steps = 0;  // steps whose published result carried the non-finite TD flag
  double wait_us = 0.0;
  // record (tests)
  int rec_cap = 0, rec_n = 0;
  std::vector<uint8_t> rec_stage;
  std::vector<long long> rec_meta;  // task, have, c, a_greedy, a_taken, terminal

  // native test phases (sfx_runner_test_env / sfx_runner_*test_phase): the test tasks' callbacks (null: the
  // built-in synthetic test tasks, one generator each in trng), the exploration schedule's own stream, and
  // what the three kinds of phase share: the host-coherent result, the device selections, the sequence word
  // (the φ phase keeps its own in its device block's header) and the launch-set counter
  unsigned long long seed = 0;
  sfx_env_reset_fn tenv_reset = nullptr;
  sfx_env_step_fn tenv_step = nullptr;
  void* tenv_ctx = nullptr;
  std::vector<std::mt19937_64> trng;
  std::mt19937_64 xrng;
  TestResult* tres = nullptr;
  int64_t* tsel = nullptr;
  long long* tdseq = nullptr;
  long long tseq = 0;
  // a kind's own buffers, allocated by its first phase (the step graphs are keyed on their addresses): the
  // host-coherent staging record (TestStageLayout), the device block (SF: the state rows [TEST_EMAX][n_s]; TSF:
  // TsfTestDevLayout; φ: PhiTestDevLayout) and the loss block [horizon][E] (TSF: [horizon][E][3])
  enum { TP_SF = 0, TP_TSF = 1, TP_PHI = 2 };
  struct TestPhaseBufs {
    uint8_t* st = nullptr;
    uint8_t* blk = nullptr;
    float* loss = nullptr;
    size_t loss_n = 0;
  } tp[3];

  float uni() { return std::uniform_real_distribution<float>(0.f, 1.f)(rng); }
  // host-written cancel word next to the go word the gates poll (push: device memory through
  // the BAR; pull: host-coherent memory)
  int* hcancel_word() const { return reinterpret_cast<int*>((dpush ? dgo : go) + 4); }
  int* hold_word() const { return reinterpret_cast<int*>((dpush ? dgo : go) + 5); }  // gate_wait
};

namespace {

int shard_tsf_body(sfx_runner* R, bool have, bool pre, bool ahead);  // sfx_tsf.inc
int tsf_test_phase_ready(sfx_handle* h, int E);
int tsf_test_phase_body(sfx_runner* R, int E, int horizon, float* W, int w_stride, float* Om, int o_stride, float* mom,
                        int mom_stride);
const void* tsf_test_phase_tgf(sfx_handle* h);
int phi_test_phase_ready(sfx_handle* h);  // sfx_phi.inc
void phi_test_phase_ptrs(sfx_handle* h, const void** p);
int phi_test_phase_body(sfx_handle* h, int E, int horizon, float* W, int w_stride, float* Wb, const unsigned char* stage,
                        unsigned char* blk, float* loss, int64_t* sel, TestResult* res);
int shard_tsf_buffers(sfx_handle* h);

bool sharded_sched(const sfx_runner* R) { return R->schedule == RUN_SHARD || R->schedule == RUN_SHARD_TSF; }
bool phi_sched(int schedule) { return schedule == RUN_PHI || schedule == RUN_TSF_PHI; }
// the local head of the active task on this rank (sharded TSF: -1 when another rank owns it)
int own_loc(const sfx_runner* R) {
  if (R->schedule != RUN_SHARD_TSF) return R->task;
  const int loc = R->task - R->h->off;
  return loc >= 0 && loc < R->h->T ? loc : -1;
}
// slot bits a step with an update flips: every head (all-task schedules) or the active one
unsigned long long step_bits(const sfx_runner* R) {
  if (R->schedule == RUN_ALL || R->schedule == RUN_SHARD) return R->h->all_bits();
  const int loc = own_loc(R);
  return loc >= 0 ? 1ull << loc : 0ull;
}

// marks the handle as driven by the runner: its launches do not bump sfx_handle::gen
struct RunnerScope {
  sfx_handle* h;
  explicit RunnerScope(sfx_handle* hh) : h(hh) { ++h->in_runner; }
  ~RunnerScope() { --h->in_runner; }
  RunnerScope(const RunnerScope&) = delete;
  RunnerScope& operator=(const RunnerScope&) = delete;
};

// Points the handle at a step's host rounds and puts it back on every exit: the side stream (the
// next step may already wait at its gate on the step stream), the step's slot mask and role copy,
// the rounds' collectives on their own communicator (sharded), and a cancel word that stays zero
// -- the next step's gate, spinning meanwhile, may write dcancel (when the host is slower than its
// bound), but these rounds belong to a step that runs.
struct RoundsTarget {
  sfx_handle* h;
  const hipStream_t stream;
  const unsigned long long mask;
  const int* const cancel;
  const int mb;
  const bool rounds_comm;
  RoundsTarget(sfx_runner* R, unsigned long long m, int par)
      : h(R->h), stream(h->stream), mask(h->mask), cancel(h->G.cancel), mb(h->G.mb), rounds_comm(h->rounds_comm) {
    h->stream = R->side;
    h->mask = m;
    h->G.mb = par ? R_NS : 0;
    h->G.cancel = h->dcancel + 1;
    h->rounds_comm = R->schedule == RUN_SHARD;
  }
  ~RoundsTarget() {
    h->stream = stream;
    h->mask = mask;
    h->G.cancel = cancel;
    h->G.mb = mb;
    h->rounds_comm = rounds_comm;
  }
  RoundsTarget(const RoundsTarget&) = delete;
  RoundsTarget& operator=(const RoundsTarget&) = delete;
};

int synth_reset(sfx_runner* R, float* s0) {
  std::normal_distribution<float> nd(0.f, 1.f);
  for (int k = 0; k < R->h->n_s; ++k) s0[k] = nd(R->rng);
  return 0;
}

// tasks/reacher.py-shaped synthetic task: s' ~ N(0,1), φ ~ U[0,1), r = φ·onehot(task)
int synth_step(sfx_runner* R, int task, float* s1, float* phi, float* r, int* terminal) {
  synth_reset(R, s1);
  const int d = R->h->d;
  for (int k = 0; k < d; ++k) phi[k] = R->uni();
  *r = phi[task % d];
  *terminal = R->p_end > 0.f && R->uni() < R->p_end ? 1 : 0;
  return 0;
}

int env_reset(sfx_runner* R, float* s0) {
  if (R->env_reset) {
    if (R->env_reset(R->env_ctx, R->task, s0)) SFX_FAIL(SFX_E_STATE, "env reset callback failed");
    return SFX_OK;
  }
  return synth_reset(R, s0);
}

int env_step(sfx_runner* R, int a, float* s1, float* phi, float* r, int* terminal) {
  if (R->env_step) {
    if (R->env_step(R->env_ctx, R->task, a, s1, phi, r, terminal)) SFX_FAIL(SFX_E_STATE, "env step callback failed");
    return SFX_OK;
  }
  return synth_step(R, R->task, s1, phi, r, terminal);
}

void replay_append(sfx_runner* R, const float* s, int64_t a, float r, const float* phi, const float* s1, float g) {
  const int n_s = R->h->n_s, d = R->h->d;
  const long i = R->ridx;
  std::memcpy(&R->rs[(size_t)i * n_s], s, sizeof(float) * n_s);
  std::memcpy(&R->rs1[(size_t)i * n_s], s1, sizeof(float) * n_s);
  std::memcpy(&R->rphi[(size_t)i * d], phi, sizeof(float) * d);
  R->rr[i] = r;
  R->ra[i] = a;
  R->rgam[i] = g;
  R->rsize = std::min<long>(R->rsize + 1, R->cap);
  R->ridx = (i + 1) % R->cap;
}

// The minibatch plan of env step `step` >= E (E = env_steps of the current iteration, after its
// transition was appended; look-ahead mode): drawn from irng in step order, with the replay size
// and the slot of that step's transition as they will be when every step in between appends one
// transition.  Plans drawn before the ring changed otherwise (prefill) are dropped and drawn again.
const sfx_runner::MbPlan& plan_of(sfx_runner* R, long long step) {
  const long long E = R->cur_step;
  auto predict = [&](long long st, long& size, long& slot) {
    const long long dd = st - E;
    size = (long)std::min<long long>((long long)R->rsize + dd, R->cap);
    slot = (long)(((long long)R->ridx - 1 + dd + 2LL * R->cap) % R->cap);
  };
  while (!R->plans.empty() && R->plans.front().step < E) R->plans.pop_front();
  if (!R->plans.empty()) {
    long size, slot;
    predict(R->plans.front().step, size, slot);
    if (R->plans.front().step != E || R->plans.front().size != size || R->plans.front().slot != slot)
      R->plans.clear();
  }
  while (R->plans.empty() || R->plans.back().step < step) {
    sfx_runner::MbPlan pl;
    pl.step = R->plans.empty() ? E : R->plans.back().step + 1;
    pl.early = pl.step > E;
    predict(pl.step, pl.size, pl.slot);
    std::uniform_int_distribution<long> ui(0, std::max(1L, pl.size) - 1);
    pl.idx.resize(R->B);
    pl.dirty = false;
    for (int b = 0; b < R->B; ++b) {
      pl.idx[b] = ui(R->irng);
      pl.dirty = pl.dirty || pl.idx[b] == pl.slot;
    }
    R->plans.push_back(std::move(pl));
  }
  return R->plans[(size_t)(step - R->plans.front().step)];
}

// rows idx of the host ring into [S | S1] at dst (the look-ahead block; TSF: and the φ rows)
void stage_ahead(sfx_runner* R, const std::vector<long>& idx) {
  const int n_s = R->h->n_s, d = R->h->d, B = R->B;
  float* S = reinterpret_cast<float*>(R->hst + R->lay.ax);
  float* S1 = S + (size_t)B * n_s;
  float* PHI = reinterpret_cast<float*>(R->hst + R->lay.axphi);
  for (int b = 0; b < B; ++b) {
    std::memcpy(S + (size_t)b * n_s, &R->rs[(size_t)idx[b] * n_s], sizeof(float) * n_s);
    std::memcpy(S1 + (size_t)b * n_s, &R->rs1[(size_t)idx[b] * n_s], sizeof(float) * n_s);
    if (R->schedule == RUN_TSF || R->schedule == RUN_SHARD_TSF)
      std::memcpy(PHI + (size_t)b * d, &R->rphi[(size_t)idx[b] * d], sizeof(float) * d);
  }
}

// uniform minibatch into the host staging (agents/buffer.py:52-64); look-ahead mode: the rows of
// this step's plan
void replay_sample(sfx_runner* R) {
  const int n_s = R->h->n_s, d = R->h->d, B = R->B;
  std::uniform_int_distribution<long> ui(0, R->rsize - 1);
  const std::vector<long>* pidx = R->ahead ? &plan_of(R, R->cur_step).idx : nullptr;
  float* S = reinterpret_cast<float*>(R->hst + R->lay.s);
  float* S1 = reinterpret_cast<float*>(R->hst + R->lay.s1);
  float* PHI = reinterpret_cast<float*>(R->hst + R->lay.phi);
  int64_t* Aa = reinterpret_cast<int64_t*>(R->hst + R->lay.a);
  float* GA = reinterpret_cast<float*>(R->hst + R->lay.gamma);
  float* RB = reinterpret_cast<float*>(R->hst + R->lay.rb);
  for (int b = 0; b < B; ++b) {
    // the same index stream with look-ahead on or off while plans are consumed in order (one run,
    // or runs back to back); a prefill between runs, or plans drawn for steps that never sample,
    // use up draws the look-ahead-off path does not make, so the two streams part there
    const long i = pidx ? (*pidx)[b] : ui(R->irng);
    std::memcpy(S + (size_t)b * n_s, &R->rs[(size_t)i * n_s], sizeof(float) * n_s);
    std::memcpy(S1 + (size_t)b * n_s, &R->rs1[(size_t)i * n_s], sizeof(float) * n_s);
    std::memcpy(PHI + (size_t)b * d, &R->rphi[(size_t)i * d], sizeof(float) * d);
    Aa[b] = R->ra[i];
    GA[b] = R->rgam[i];
    RB[b] = R->rr[i];
  }
}

// the device replay's minibatch of a step, drawn from the host mirror (records only)
void replay_sample_keyed(sfx_runner* R, unsigned long long key) {
  const int n_s = R->h->n_s, d = R->h->d, B = R->B;
  float* S = reinterpret_cast<float*>(R->hst + R->lay.s);
  float* S1 = reinterpret_cast<float*>(R->hst + R->lay.s1);
  float* PHI = reinterpret_cast<float*>(R->hst + R->lay.phi);
  int64_t* Aa = reinterpret_cast<int64_t*>(R->hst + R->lay.a);
  float* GA = reinterpret_cast<float*>(R->hst + R->lay.gamma);
  float* RB = reinterpret_cast<float*>(R->hst + R->lay.rb);
  for (int b = 0; b < B; ++b) {
    const long i = (long)replay_index(key, b, R->rsize);
    std::memcpy(S + (size_t)b * n_s, &R->rs[(size_t)i * n_s], sizeof(float) * n_s);
    std::memcpy(S1 + (size_t)b * n_s, &R->rs1[(size_t)i * n_s], sizeof(float) * n_s);
    std::memcpy(PHI + (size_t)b * d, &R->rphi[(size_t)i * d], sizeof(float) * d);
    Aa[b] = R->ra[i];
    GA[b] = R->rgam[i];
    RB[b] = R->rr[i];
  }
}

int replay_upload(sfx_runner* R) {
  const size_t cap = (size_t)R->cap, n_s = R->h->n_s, d = R->h->d;
  const struct {
    void* dst;
    const void* src;
    size_t bytes;
  } cp[6] = {{R->drs, R->rs.data(), 4 * cap * n_s},  {R->drs1, R->rs1.data(), 4 * cap * n_s},
             {R->drphi, R->rphi.data(), 4 * cap * d}, {R->drr, R->rr.data(), 4 * cap},
             {R->drg, R->rgam.data(), 4 * cap},       {R->dra, R->ra.data(), 8 * cap}};
  for (const auto& c : cp) HIPCHK(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyHostToDevice, R->h->stream));
  HIPCHK(hipStreamSynchronize(R->h->stream));
  R->dring_dirty = false;
  return SFX_OK;
}

sfx_handle::Pending runner_pending(sfx_runner* R, bool have, bool pre = false, bool ahead = false) {
  sfx_handle::Pending p;
  p.pre = have && pre;
  p.ax = have && ahead ? reinterpret_cast<const float*>(R->dst + R->lay.ax) : nullptr;
  p.aM = p.ax ? R->B : 0;
  p.active = true;
  p.update = have;
  p.sel = true;
  p.B = have ? R->B : 0;
  p.use_gpi = 1;  // features/deep.py: next actions by GPI over all heads
  p.task = R->task;
  p.sel_use_gpi = R->sel_use_gpi;
  p.S = reinterpret_cast<const float*>(R->dst + R->lay.s);
  p.S1 = reinterpret_cast<const float*>(R->dst + R->lay.s1);
  p.phi = reinterpret_cast<const float*>(R->dst + R->lay.phi);
  p.a = reinterpret_cast<const int64_t*>(R->dst + R->lay.a);
  p.gamma = reinterpret_cast<const float*>(R->dst + R->lay.gamma);
  p.s_next = reinterpret_cast<const float*>(R->dst + R->lay.snext);
  p.losses = nullptr;
  return p;
}

GateArgs runner_gate(sfx_runner* R, bool ahead = false) {
  GateArgs g{};
  g.src = reinterpret_cast<const uint4*>(R->dpush ? R->dpush : R->hst);
  g.dst = reinterpret_cast<uint4*>(R->dst);
  g.n16 = (int)(R->lay.end(ahead, R->schedule) / 16);
  g.go = R->dpush ? R->dgo : R->go;
  g.dctr = R->dctr;
  g.timeout = R->gate_timeout;  // ticks of the 100 MHz clock (default 5 s)
  g.err = &R->res->err;
  g.hcancel = R->hcancel_word();
  g.hold = R->hold_word();
  g.hard = std::max(R->gate_timeout, 2000000000LL);  // a held wait: at least 20 s
  g.cancel = R->h->dcancel;
  g.rearm0 = &R->h->dout->done;
  g.rearm1 = R->h->selk ? &R->h->selk->done : nullptr;
  if (R->schedule == RUN_SHARD && shard_fused(R->h, R->B) && R->h->xb[0]) {  // round 0's maxima, pre-step part
    g.clr = R->h->xb[0];
    g.nclr = (int)(2 * shard_body(R->h, R->h->Mmax) + (size_t)R->h->Tg * R->h->A);
  }
  return g;
}

// pre: the step's flag reset and LMS move into its gate (no step-start forward)
int runner_launch_gate(sfx_runner* R, bool ahead = false, bool pre = false, bool lms = false) {
  sfx_handle* h = R->h;
  if (!R->dev_replay) {
    GateArgs g = runner_gate(R, ahead);
    if (pre) {
      const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
      g.flag = &h->dout->flag;
      g.flag_value = h->T;
      if (lms) {
        g.lms_w = h->w + (size_t)R->task * h->dpad;
        g.lms_phi = reinterpret_cast<const float*>(src + R->lay.phi1);
        g.lms_r = reinterpret_cast<const float*>(src + R->lay.r1);
        g.lms_alpha = R->alpha_w;
        g.lms_d = h->d;
      }
    }
    hipLaunchKernelGGL(k_gate, dim3(1), dim3(256), 0, h->stream, g);
    LAUNCHCHK();
    return SFX_OK;
  }
  const RunnerLayout& L = R->lay;
  ReplayGateArgs A{};
  A.g = runner_gate(R);
  A.tail0 = (int)(L.snext / 16);
  A.g.n16 = (int)((L.ax - L.snext) / 16);  // the tail up to the look-ahead block (no look-ahead here)
  A.n_s = h->n_s;
  A.d = h->d;
  A.B = R->B;
  A.off_s = (int)L.s;
  A.off_s1 = (int)L.s1;
  A.off_phi = (int)L.phi;
  A.off_a = (int)L.a;
  A.off_g = (int)L.gamma;
  A.off_rb = (int)L.rb;
  A.tr_s = (int)(L.tr_s - L.snext);
  A.tr_s1 = (int)(L.tr_s1 - L.snext);
  A.tr_phi = (int)(L.tr_phi - L.snext);
  A.tr_meta = (int)(L.tr_meta - L.snext);
  A.rs = R->drs;
  A.rs1 = R->drs1;
  A.rphi = R->drphi;
  A.rr = R->drr;
  A.rg = R->drg;
  A.ra = R->dra;
  hipLaunchKernelGGL(k_gate_replay, dim3(1), dim3(256), 0, h->stream, A);
  LAUNCHCHK();
  return SFX_OK;
}

// The device work of one step on h->stream, with h->mask as its slot mask:
//   all          gate -> the speculative all-task step (its last k_ver publishes) -> [publish]
//   active / tsf gate -> the active head's update -> action for s_next -> publish
int runner_body(sfx_runner* R, bool have, bool lms, sfx_runner::StepFlags fl = {false, false, 0}) {
  sfx_handle* h = R->h;
  const auto at = [&](size_t off) { return reinterpret_cast<const float*>(R->dst + off); };
  const bool pre = have && fl.pre, ahead = have && fl.ahead;
  RC(runner_launch_gate(R, ahead, pre, lms));
  if (R->schedule == RUN_SHARD_TSF) return shard_tsf_body(R, have, pre, ahead);
  const SelPub pub{R->res, (const long long*)R->dctr, (const int*)&h->dout->flag, (const int*)h->dcancel,
                   (const int*)h->G.nonfin};
  // the all-task step with the heads sharded over the ranks; k_sfinish publishes
  // (pre: the step before forwarded this minibatch and this step's gate ran the LMS)
  if (R->schedule == RUN_SHARD)
    return shard_step_all(h, runner_pending(R, have, pre, ahead), lms && !pre ? R->task : -1, at(R->lay.phi1),
                          at(R->lay.r1), R->alpha_w, have ? h->spec_rounds : 0, R->res, R->dctr);
  if (R->schedule != RUN_ALL) {
    const int64_t* a = reinterpret_cast<const int64_t*>(R->dst + R->lay.a);
    const bool phis = phi_sched(R->schedule);
    if (phis && !phi_runner_ready(h, R->schedule == RUN_TSF_PHI))
      SFX_FAIL(SFX_E_STATE, "runner: the φ / TSF setup changed after sfx_runner_config; configure the schedule again");
    if (have && phis) {  // the staged φ rows are not read: φ comes from the net
      RC(phi_update_body(h, R->schedule == RUN_TSF_PHI ? 1 : 0, R->task, at(R->lay.s), a, at(R->lay.rb), at(R->lay.s1),
                         at(R->lay.gamma), R->B, R->upd_use_gpi, R->phi_bias + R->task, R->phi_lam + R->task, R->dloss,
                         nullptr));
    } else if (have) {  // pre: the previous step's select forwarded this minibatch (select_ahead_body)
      // frozen featurizer: the minibatch's φ rows from its (s, a, s1), over the staged ones the gate copied
      if (R->feat)
        RC(pre_rows_body(R->feat, h->stream, at(R->lay.s), a, at(R->lay.s1), R->B,
                         reinterpret_cast<float*>(R->dst + R->lay.phi), h->dcancel));
      if (R->schedule == RUN_TSF)
        RC(tsf_body(h, R->task, at(R->lay.s), a, at(R->lay.rb), at(R->lay.phi), at(R->lay.s1), at(R->lay.gamma), R->B,
                    R->upd_use_gpi, R->dloss, nullptr, nullptr, pre));
      else
        RC(update_body(h, R->task, at(R->lay.s), a, at(R->lay.rb), at(R->lay.phi), at(R->lay.s1), at(R->lay.gamma),
                       R->B, R->upd_use_gpi, R->dloss, nullptr, pre));
    }
    // the action for s_next sees the post-update heads: the update flips the task's slot
    const unsigned long long saved = h->mask;
    if (have) h->mask ^= 1ull << R->task;
    const int rc = ahead ? select_ahead_body(h, at(R->lay.snext), at(R->lay.ax),
                                             R->schedule == RUN_TSF ? at(R->lay.axphi) : nullptr, R->B, R->task,
                                             R->sel_use_gpi, h->dout->sel, &pub)
                         : select_body(h, at(R->lay.snext), R->task, R->sel_use_gpi, nullptr, h->dout->sel, &pub,
                                       phis ? R->phi_bias + R->task : nullptr);
    h->mask = saved;
    return rc;
  }
  const sfx_handle::Pending p = runner_pending(R, have, pre, ahead);
  h->pub_res = R->res;
  h->pub_dctr = R->dctr;
  h->pub_folded = false;
  const int rc = launch_step_all(h, p, lms && !pre ? R->task : -1, at(R->lay.phi1), at(R->lay.r1), R->alpha_w,
                                 h->spec_rounds);
  const bool folded = h->pub_folded;
  h->pub_res = nullptr;
  h->pub_dctr = nullptr;
  h->pub_folded = false;
  RC(rc);
  // no final k_ver with action selection in this step: publish on its own
  return folded ? SFX_OK : run_publish(h, h->dout->sel, pub);
}

// Launch ONE graph holding `nsteps` consecutive steps (up to span_max when the runner
// pre-launches: one graph boundary per nsteps steps), step s with h->mask flipped s times --
// the flips runner_issue makes after each step.  Every step still opens with its own gate.
// Look-ahead runs: flags of the steps of such a graph -- the first step's `pre` is fl0.pre (later
// steps are pre: a span never holds a dirty step or a target sync after its first), every step
// with an update looks ahead, role copies alternate from fl0.par.
int runner_launch(sfx_runner* R, bool have, bool lms, int nsteps = 1, bool launch_it = true,
                  sfx_runner::StepFlags fl0 = {false, false, 0}) {
  sfx_handle* h = R->h;
  unsigned alpha_bits;
  std::memcpy(&alpha_bits, &R->alpha_w, 4);
  const unsigned long long bits = step_bits(R);
  if (sharded_sched(R) && !coll_capturable(h)) {  // host transport: eager, one step
    if (!launch_it) return SFX_OK;
    if (nsteps != 1) SFX_FAIL(SFX_E_STATE, "runner: host-transport steps are launched one at a time");
    return runner_body(R, have, lms);
  }
  const GraphKey key =
      make_key(6, {have ? R->B : 0, lms ? R->task : -1, R->task, R->sel_use_gpi, (int)alpha_bits,
                   h->spec_rounds * RUN_SCHEDULES + R->schedule,
                   R->dev_replay + 2 * R->upd_use_gpi + 4 * nsteps + 128 * fl0.pre + 256 * fl0.ahead + 512 * fl0.par},
               h->mask, {R->dst, R->hst, R->go, R->res, phi_sched(R->schedule) ? R->phi_bias : nullptr,
                         phi_sched(R->schedule) ? R->phi_lam : nullptr, R->feat});
  return run_graph(h, key, [&]() -> int {
    const unsigned long long m0 = h->mask;
    int rc = SFX_OK;
    for (int st = 0; st < nsteps && rc == SFX_OK; ++st) {
      h->mask = (st & 1) ? m0 ^ bits : m0;
      sfx_runner::StepFlags fl{st == 0 ? fl0.pre : fl0.ahead, fl0.ahead, fl0.ahead ? (fl0.par + st) & 1 : 0};
      h->G.mb = fl.par ? R_NS : 0;
      rc = runner_body(R, have, lms, fl);
    }
    h->mask = m0;
    h->G.mb = 0;
    return rc;
  }, launch_it);
}

// Stop every step still queued behind the host: their gates cancel them (nothing of them
// commits), the streams drain, and the hand-off counters restart from the host's sequence.
// restore: the in-flight step did not commit either (cancelled at its gate), so the slot mask
// returns to what it was before that step was issued.
// Wait (bounded) until everything queued on `s` has run; false when it has not after `seconds`.
bool stream_drain(hipStream_t s, double seconds) {
  const auto t0 = std::chrono::steady_clock::now();
  for (long spins = 0;; ++spins) {
    const hipError_t e = hipStreamQuery(s);
    if (e != hipErrorNotReady) return true;  // done (or failed: nothing left to wait for)
    if ((spins & 255) == 0 &&
        std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds)
      return false;
  }
}

void runner_abort(sfx_runner* R, bool restore) {
  sfx_handle* h = R->h;
  volatile int* hc = R->hcancel_word();
  *hc = 1;
  __builtin_ia32_sfence();
  // the gates of queued steps see the cancel word and their launches run without committing; a
  // queue that still does not drain (a collective waiting for a dead peer) leaves the runner
  // unusable instead of hanging the caller
  const double bound = std::max(30.0, R->wait_bound);
  if (!stream_drain(h->stream, bound) || (R->side && !stream_drain(R->side, bound))) {
    R->broken = true;
    R->broken_why = "runner: the device queue did not drain after a cancelled step (runner unusable)";
    return;
  }
  *hc = 0;
  __builtin_ia32_sfence();
  const long long seq = R->seq;
  (void)hipMemsetAsync(h->dcancel, 0, sizeof(int), h->stream);
  (void)hipMemcpyAsync(R->dctr, &seq, sizeof(seq), hipMemcpyHostToDevice, h->stream);
  (void)hipStreamSynchronize(h->stream);
  R->res->err = 0;
  for (int i = 0; i < RES_RING; ++i) {  // the drained steps' publications: below every later seq
    R->res[i].cancelled = 0;
    __atomic_store_n(&R->res[i].seq, seq, __ATOMIC_RELEASE);
  }
  if (restore && R->inflight) h->mask = R->inflight_mask;
  R->inflight = false;
  R->pre_n = 0;
  R->preq.clear();
  R->chain = false;  // the drained launches ran over both copies of the minibatch roles
}

int runner_issue(sfx_runner* R, bool have, bool lms, const sfx_runner::StepFlags* retry = nullptr);

// Host rounds of a step run on the side stream while the next step's gate may be waiting: raise
// the hold word first (gate_wait), flushed before err is read; a gate that gave up before that
// lets its step's launches run -- cancel and drain everything queued before the rounds touch the
// transient buffers (the steps are issued again when their turn comes).
void runner_hold(sfx_runner* R, int on) {
  volatile int* hw = R->hold_word();
  *hw = on;
  __builtin_ia32_sfence();
  if (R->dpush) (void)*hw;  // a read through the BAR completes the posted write
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

// Returns true when queued steps were cancelled and drained: their launches ran (committing
// nothing) and overwrote the transient buffers -- activations of every role, the speculative next
// actions -- that the host rounds would read.
bool runner_hold_for_rounds(sfx_runner* R) {
  runner_hold(R, 1);
  if (__atomic_load_n(&R->res->err, __ATOMIC_SEQ_CST)) {
    R->retried += R->pre_n;  // issued again when their turn comes
    runner_abort(R, false);
    return true;
  }
  return false;
}

// Spin (bounded: sfx_runner_wait_timeout, 10 s by default) until the in-flight step has
// published its result.  Past the bound: cancel the queued steps and drain (bounded); a queue
// that does not drain -- a sharded step's collective waiting for a peer that is gone -- gets
// RCCL's asynchronous error read and both communicators aborted (comm_abort), which ends the
// waiting RCCL kernels; then the error returns (bench.py falls back instead of hanging).
int runner_wait(sfx_runner* R) {
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  while (__atomic_load_n(&R->cur()->seq, __ATOMIC_ACQUIRE) < R->inflight_seq) {
    if ((++spins & 1023) == 0) {
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > R->wait_bound) {
        sfx_handle* h = R->h;
        char msg[160];
        std::snprintf(msg, sizeof(msg), "runner: device step %lld did not complete within %.3g s", R->inflight_seq,
                      R->wait_bound);
        std::string why = msg;
        volatile int* hc = R->hcancel_word();
        *hc = 1;
        __builtin_ia32_sfence();
        const bool drained = stream_drain(h->stream, R->wait_bound) && (!R->side || stream_drain(R->side, R->wait_bound));
        {  // what the step was waiting for: the hand-off words as the host sees them
          const long long go = __atomic_load_n(R->dpush ? R->dgo : R->go, __ATOMIC_ACQUIRE);
          long long dc = -1;
          if (drained) (void)hipMemcpy(&dc, R->dctr, sizeof(dc), hipMemcpyDeviceToHost);
          char d[200];
          std::snprintf(d, sizeof(d), " [go %lld, last gate opened %lld%s, result seq %lld, gate err %d, hold %d, %d queued]",
                        go, dc, drained ? "" : " (queue not drained)", __atomic_load_n(&R->cur()->seq, __ATOMIC_ACQUIRE),
                        R->res->err, *R->hold_word(), R->pre_n);
          why += d;
        }
        if (!drained && (h->comm || h->comm_rounds)) why += "; RCCL async error" + comm_abort(h) + "; communicators aborted";
        runner_abort(R, true);
        if (R->broken)
          why += "; " + R->broken_why;
        else if (h->comm_dead)
          clear_graphs(h);  // the captured steps hold all-reduce nodes of the aborted communicators
        SFX_FAIL(SFX_E_STATE, why.c_str());
      }
    }
  }
  R->wait_us += 1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return SFX_OK;
}

// One host round r of the in-flight step (on the side stream) and the copy of its verdict to the
// host, as ONE graph launch: captured once per (round parity, role copy, look-ahead, slot mask) --
// everything a round bakes into its launches -- instead of a dozen eager launches, which put the
// runtime's per-launch host cost on the critical path of every step that needs host rounds.
template <class F>
// A host round (op 40: the all-task round; 41: the sharded one).  The all-task round's final
// k_ver posts its verdict to hout itself (R->round_posted; round_wait polls that word) unless a
// selection follows it; otherwise hout is a copy after the round.
int host_round_graph(sfx_runner* R, int op, int r, F round, bool launch_it = true) {
  sfx_handle* h = R->h;
  bool recorded = false, posted = false;
  const auto body = [&]() -> int {
    h->post_hout = op == 40;
    h->hout_posted = false;
    const int rc = round();
    h->post_hout = false;
    RC(rc);
    recorded = true;
    posted = h->hout_posted;
    if (posted) return SFX_OK;
    return hipMemcpyAsync(h->hout, h->dout, sizeof(StepOut), hipMemcpyDeviceToHost, h->stream) == hipSuccess
               ? SFX_OK
               : SFX_E_HIP;
  };
  if (launch_it) h->hout->posted = 0;  // the round before was waited for: nothing writes hout now
  R->round_posted = false;
  if (!coll_capturable(h)) {  // the host transport synchronises inside its collectives
    if (!launch_it) return SFX_OK;
    RC(body());
    R->round_posted = posted;
    return SFX_OK;
  }
  const GraphKey key = make_key(op, {r & 1, R->inflight_fl.ahead ? 1 : 0, R->inflight_fl.par, h->spec_rounds, R->B},
                                h->mask, {R->dst, h->dout, h->hout});
  RC(run_graph(h, key, body, launch_it));
  if (recorded) {
    if (h->use_graphs && !h->prof) h->graph_posts[key] = posted;
  } else {
    const auto it = h->graph_posts.find(key);
    posted = it != h->graph_posts.end() && it->second;
  }
  R->round_posted = launch_it && posted;
  return SFX_OK;
}

// Wait for the host round just launched on h->stream: its posted verdict, or the stream.
int round_wait(sfx_runner* R) {
  sfx_handle* h = R->h;
  if (R->round_posted && wait_posted(h)) return SFX_OK;
  return hipStreamSynchronize(h->stream) == hipSuccess ? SFX_OK : SFX_E_HIP;
}

// Host round r of the step p on h->stream (launch_it false: its capture alone), the round of the
// runner's schedule: all-task, or sharded with the round's finish
int host_round(sfx_runner* R, const sfx_handle::Pending& p, int r, bool launch_it = true) {
  sfx_handle* h = R->h;
  if (R->schedule != RUN_SHARD)
    return host_round_graph(R, 40, r, [&]() -> int { return launch_round(h, p, r, true); }, launch_it);
  return host_round_graph(R, 41, r, [&]() -> int {
    RC(shard_round_body(h, p, r, true));
    return shard_final_body(h, p, r, nullptr, nullptr);
  }, launch_it);
}

// Instantiate the host-round graphs a run may need (sfx_runner_warm): both slot masks, both round
// parities, both role copies, with and without the look-ahead -- so the first step that needs host
// rounds does not pay a capture on its critical path.
int warm_host_rounds(sfx_runner* R, unsigned long long bits, bool ahd) {
  sfx_handle* h = R->h;
  if (R->schedule != RUN_ALL && R->schedule != RUN_SHARD) return SFX_OK;
  const unsigned long long m0 = h->mask;
  const sfx_runner::StepFlags fl0 = R->inflight_fl;
  int rc = SFX_OK;
  const RoundsTarget target(R, m0, 0);
  for (int pm = 0; pm < 2 && rc == SFX_OK; ++pm)
    for (int ah = 0; ah < (ahd ? 2 : 1) && rc == SFX_OK; ++ah)
      for (int par = 0; par < (ah ? 2 : 1) && rc == SFX_OK; ++par)
        for (int r = h->spec_rounds; r < h->spec_rounds + 2 && rc == SFX_OK; ++r) {
          h->mask = pm ? m0 ^ bits : m0;
          R->inflight_fl = sfx_runner::StepFlags{false, ah != 0, par};
          h->G.mb = par ? R_NS : 0;
          rc = host_round(R, runner_pending(R, true, false, ah != 0), r, false);
        }
  R->inflight_fl = fl0;
  return rc;
}

// The hold word raised for a step's host rounds (runner_hold_for_rounds) and dropped on every exit.
struct RoundsHold {
  sfx_runner* R;
  const bool drained;
  explicit RoundsHold(sfx_runner* r) : R(r), drained(runner_hold_for_rounds(r)) {}
  ~RoundsHold() { runner_hold(R, 0); }
  RoundsHold(const RoundsHold&) = delete;
  RoundsHold& operator=(const RoundsHold&) = delete;
};

// Finish the in-flight all-task step (RUN_ALL, RUN_SHARD) from the verdict `flag` its device rounds
// published: account the speculation and, when it left policies unverified, run host rounds on the
// side stream until none is (on every rank alike, sharded: the flag comes from all-reduced maxima),
// then take the selection (*c, *a) from the last round.  The two schedules differ in recompute()
// and host_round() alone (and in the refusal below).
int runner_host_rounds(sfx_runner* R, int flag, long long* c, long long* a) {
  sfx_handle* h = R->h;
  const bool shard = R->schedule == RUN_SHARD;
  const int Tn = shard ? h->Tg : h->T;
  int first, r = h->spec_rounds;
  RC(spec_verdict(h, flag, Tn, r, &first));
  h->steps_spec += 1;
  if (first == Tn) {
    h->rounds_total += r;
    return SFX_OK;
  }
  h->steps_fallback += 1;
  h->policies_rerun += Tn - first;
  R->host_rounds += 1;
  // the step's own forward is recomputed in full (after a drain), its final rounds look ahead
  const sfx_handle::Pending p = runner_pending(R, true, false, R->inflight_fl.ahead);
  // The step's forward and device rounds again, from the pre-step slot (nothing of them committed
  // there; this step's LMS has, so none here); sharded: round 0's maxima refilled as the gate fills them
  const auto recompute = [&]() -> int {
    if (!shard) return launch_step_all(h, p, -1, nullptr, nullptr, 0.f, h->spec_rounds);
    const GateArgs g = runner_gate(R);
    if (g.clr && hipMemsetD32Async((hipDeviceptr_t)g.clr, SORT_EMPTY, (size_t)g.nclr, h->stream) != hipSuccess)
      return SFX_E_HIP;
    return shard_step_all(h, p, -1, nullptr, nullptr, 0.f, h->spec_rounds, nullptr, nullptr);
  };
  const RoundsHold hold(R);  // before the handle leaves the step stream: a drain works on that one
  if (shard && hold.drained && coll_active(h))  // a recompute would repeat its collectives on this rank only
    SFX_FAIL(SFX_E_STATE, "runner: a sharded step needing host rounds found later steps cancelled at their gates");
  const RoundsTarget target(R, R->inflight_mask, R->inflight_fl.par);
  const int rc = [&]() -> int {
    if (hold.drained) {
      // cancelled steps ran over this step's transient buffers (activations, maxima, next actions):
      // recompute it with the Adam step counters back at their pre-step values (round 0 bumps them)
      int e = hipMemcpyAsync(h->step, h->host_step.data(), sizeof(int) * h->T, hipMemcpyHostToDevice, h->stream) == hipSuccess
                  ? recompute()
                  : SFX_E_HIP;
      if (e == SFX_OK && (hipMemcpyAsync(h->hout, h->dout, sizeof(StepOut), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
                          hipStreamSynchronize(h->stream) != hipSuccess))
        e = SFX_E_HIP;
      if (e == SFX_OK) e = spec_verdict(h, h->hout->flag, Tn, r, &first);
      R->recomputed += 1;
      RC(e);
    }
    while (first < Tn) {  // each round fixes >= 1 head
      if (r > Tn + 1) SFX_FAIL(SFX_E_STATE, "speculation did not converge");
      RC(host_round(R, p, r));
      RC(round_wait(R));  // the sharded round posts no verdict: the wait is for the stream
      ++r;
      RC(spec_verdict(h, h->hout->flag, Tn, r, &first));
    }
    return SFX_OK;
  }();
  if (rc) {
    if (g_err.empty()) g_err = "runner: host round failed";
    return rc;
  }
  *c = h->hout->sel[0];
  *a = h->hout->sel[1];
  h->rounds_total += r;
  return SFX_OK;
}

// account head t's optimizer step exactly like sfx_step_finish
int runner_account(sfx_runner* R, int t) {
  after_update(R->h, t);
  RC(maybe_sync_target(R->h, t));  // only reached with nothing pre-launched (see runner_run)
  if (R->h->since_target[t] == 0) R->chain = false;  // the look-ahead forwarded the old target head
  return SFX_OK;
}

// Wait for the in-flight step's result; finish a failed speculation with host rounds;
// account the optimizer step (after_update / target sync) exactly like sfx_step_finish.
// A step cancelled at its gate (the host released it after the gate's bound) committed nothing:
// the queue behind it is dropped and the step runs again from the same staged inputs.
int runner_complete(sfx_runner* R) {
  sfx_handle* h = R->h;
  if (R->broken) SFX_FAIL(SFX_E_STATE, R->broken_why.c_str());
  if (!R->inflight) return SFX_OK;
  for (int attempt = 0;; ++attempt) {
    RC(runner_wait(R));
    if (!R->cur()->cancelled) break;
    if (sharded_sched(R) && coll_active(R->h)) {  // a re-issued step would repeat its collectives on this rank only
      char msg[256];
      std::snprintf(msg, sizeof(msg),
                    "runner: sharded step %lld cancelled at its gate (gate timeout flag %d, %d steps queued, %lld env "
                    "steps done)",
                    R->inflight_seq, R->res->err, R->pre_n, R->env_steps);
      runner_abort(R, true);
      SFX_FAIL(SFX_E_STATE, msg);
    }
    const bool have = R->inflight_have, lms = R->inflight_lms;
    const sfx_runner::StepFlags fl = R->inflight_fl;
    runner_abort(R, true);
    if (attempt > 0) SFX_FAIL(SFX_E_STATE, "runner: step cancelled at its gate twice");
    R->retried += 1;
    RC(runner_issue(R, have, lms, &fl));
  }
  R->inflight = false;
  const bool later_cancelled = R->res->err != 0;  // a gate queued behind this step gave up
  const HostResult* res = R->cur();
  if (res->nonfinite) {  // SURVEY §5: a TD error came out non-finite (NaN / Inf φ, γ or ψ): stop loudly
    R->nonfinite_steps += 1;
    char msg[200];
    std::snprintf(msg, sizeof(msg),
                  "runner: non-finite TD error at env step %lld (NaN/Inf in the transition or the heads; "
                  "sfx_nonfinite resets the flag)", R->env_steps + 1);
    runner_abort(R, false);
    SFX_FAIL(SFX_E_STATE, msg);
  }
  long long c = res->sel0, a = res->sel1;
  if (R->inflight_have && (R->schedule == RUN_ALL || R->schedule == RUN_SHARD)) {
    RC(runner_host_rounds(R, res->flag, &c, &a));
    for (int t = 0; t < h->T; ++t) RC(runner_account(R, t));
  } else if (R->inflight_have && own_loc(R) >= 0) {  // sharded TSF: only the owner of the active task updated
    RC(runner_account(R, own_loc(R)));
  }
  R->sel_c = c;
  R->sel_a = a;
  if (later_cancelled) {  // those steps are issued again when their turn comes
    R->retried += R->pre_n;
    runner_abort(R, false);
  }
  return SFX_OK;
}

// Hand the staged inputs of the next step to the device.
void runner_release(sfx_runner* R, bool ahead = false) {
  R->seq += 1;
  if (R->dpush) {  // write-combined stores through the BAR, fenced before and after the go word
    const size_t from = R->dev_replay ? R->lay.snext : 0;  // device replay: the gate reads only the tail
    const size_t to = R->lay.end(ahead, R->schedule);      // the look-ahead block only when used
    std::memcpy(R->dpush + from, R->hst + from, to - from);
    __builtin_ia32_sfence();
    __atomic_store_n(R->dgo, R->seq, __ATOMIC_RELEASE);
    __builtin_ia32_sfence();
    return;
  }
  __atomic_store_n(R->go, R->seq, __ATOMIC_RELEASE);
}

// Hand step seq + 1 to the device: its pre-launched graph, or a graph launched now (set_task, the
// first step of a run, after a sync or an abort).
// retry: a step issued again after its gate cancelled it -- its staging (with the look-ahead block)
// is still in place; it runs its own forward.
int runner_issue(sfx_runner* R, bool have, bool lms, const sfx_runner::StepFlags* retry) {
  sfx_handle* h = R->h;
  sfx_runner::StepFlags fl{false, false, 0};
  if (R->pre_n > 0) {
    if (R->pre_have != have) SFX_FAIL(SFX_E_STATE, "runner: pre-launched step of the wrong kind");
    if (R->preq.empty()) SFX_FAIL(SFX_E_STATE, "runner: pre-launched step without flags");
    fl = R->preq.front();
  } else if (retry) {
    fl = *retry;
    fl.pre = false;
    fl.par = fl.ahead ? (int)((R->seq + 1) & 1) : 0;
  } else if (R->ahead && have) {
    const sfx_runner::MbPlan& pl = plan_of(R, R->cur_step);
    fl.pre = R->chain && pl.early && !pl.dirty;
    fl.ahead = true;
    fl.par = (int)((R->seq + 1) & 1);
  }
  if (fl.ahead && !retry) stage_ahead(R, plan_of(R, R->cur_step + 1).idx);
  runner_release(R, fl.ahead);
  R->inflight_mask = h->mask;
  if (R->pre_n > 0) {
    R->pre_n -= 1;
    R->preq.pop_front();
  } else {
    RC(runner_launch(R, have, lms, 1, true, fl));
  }
  R->inflight_fl = fl;
  R->chain = fl.ahead;
  R->chain_gen = h->gen;
  if (fl.pre) R->pre_steps += 1;
  if (fl.ahead && !fl.pre && have && R->ahead) R->dirty_steps += 1;
  if (have) h->mask ^= step_bits(R);
  R->inflight = true;
  R->inflight_have = have;
  R->inflight_lms = lms;
  R->inflight_seq = R->seq;
  return SFX_OK;
}

// Launch ONE graph of the next `span` steps behind the in-flight one (their gates wait for the
// host) and queue their flags (see runner_launch)
int runner_prelaunch(sfx_runner* R, bool next_have, bool lms, int span, sfx_runner::StepFlags fl0) {
  RC(runner_launch(R, next_have, lms, span, true, fl0));
  R->pre_n = span;
  R->pre_have = next_have;
  R->prelaunched += span;
  for (int st = 0; st < span; ++st)
    R->preq.push_back({st == 0 ? fl0.pre : fl0.ahead, fl0.ahead, fl0.ahead ? (fl0.par + st) & 1 : 0});
  return SFX_OK;
}

int runner_select_initial(sfx_runner* R) {
  // selection for the first state of an episode: a graph with no update and no LMS
  float* sn = reinterpret_cast<float*>(R->hst + R->lay.snext);
  std::memcpy(sn, R->s.data(), sizeof(float) * R->h->n_s);
  ReplayMeta* m = reinterpret_cast<ReplayMeta*>(R->hst + R->lay.tr_meta);
  m->slot = -1;  // no transition to append
  m->have = 0;
  RC(runner_issue(R, false, false));
  return runner_complete(R);
}

// The side stream runs host rounds while the next step's gate spins on `main`, so the two must
// never feed the same hardware queue: AQL packets of one queue run in order, and the rounds
// would wait behind the gate until it gives up.  Once GPU_MAX_HW_QUEUES queues are in use the
// runtime gives a new stream the least-used existing queue, which may be main's.  (A
// high-priority stream would get a queue of its own, but measured: the extra queue level slows
// the forked TSF graphs by 40 %.)  So probe: a bounded spin on main that only a kernel on the
// candidate stream can end; a candidate that queues behind it is kept aside while the next one
// is created (so the runtime does not hand out the same queue again) and dropped afterwards.
// When no candidate passes (e.g. under a profiler that serialises every dispatch) the last one
// is kept and *independent = false: the runner then never pre-launches.
int create_side_stream(hipStream_t main, hipStream_t* out, bool* independent) {
  *out = nullptr;
  *independent = false;
  int* words = nullptr;  // [0] the word k_qset sets, [1] what k_qwait saw
  if (hipMalloc((void**)&words, 2 * sizeof(int)) != hipSuccess) SFX_FAIL(SFX_E_HIP, "hipMalloc(queue probe) failed");
  std::vector<hipStream_t> shared;
  int rc = SFX_OK, seen = 0;
  for (int attempt = 0; attempt < 8 && rc == SFX_OK && !*independent; ++attempt) {
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      rc = SFX_E_HIP;
      g_err = "hipStreamCreate failed";
      break;
    }
    seen = 0;
    if (hipMemsetAsync(words, 0, 2 * sizeof(int), main) != hipSuccess || hipStreamSynchronize(main) != hipSuccess) {
      rc = SFX_E_HIP;
      g_err = "runner: queue probe failed";
    } else {
      hipLaunchKernelGGL(k_qwait, dim3(1), dim3(64), 0, main, (const int*)words, words + 1, 5000000LL);  // 50 ms
      hipLaunchKernelGGL(k_qset, dim3(1), dim3(64), 0, s, words);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
          hipStreamSynchronize(main) != hipSuccess ||
          hipMemcpy(&seen, words + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
        rc = SFX_E_HIP;
        g_err = "runner: queue probe failed";
      }
    }
    if (rc == SFX_OK && seen) {
      *out = s;
      *independent = true;
    } else {
      shared.push_back(s);
    }
  }
  if (rc == SFX_OK && !*independent && !shared.empty()) {
    *out = shared.back();
    shared.pop_back();
  }
  for (hipStream_t s : shared) (void)hipStreamDestroy(s);
  (void)hipFree(words);
  return rc;
}

}  // namespace

extern "C" {

int sfx_runner_create(sfx_runner_t* out, sfx_t h, int batch, int capacity, float gamma, float epsilon, float alpha_w,
                      int episode_len, int sel_use_gpi, unsigned long long seed, sfx_env_reset_fn reset_fn,
                      sfx_env_step_fn step_fn, void* env_ctx) {
  if (!out || !h) SFX_FAIL(SFX_E_ARG, "null argument");
  RC(settle(h));
  *out = nullptr;
  if (batch < 1 || batch > h->Mmax || capacity < batch || episode_len < 1 || (!reset_fn) != (!step_fn))
    SFX_FAIL(SFX_E_ARG, "bad runner configuration (1 <= batch <= max_batch <= capacity; both env callbacks or none)");
  sfx_runner* R = new sfx_runner();
  R->h = h;
  R->B = batch;
  R->cap = capacity;
  R->gamma = gamma;
  R->eps = epsilon;
  R->alpha_w = alpha_w;
  R->ep_len = episode_len;
  R->sel_use_gpi = sel_use_gpi ? 1 : 0;
  R->rng.seed(seed);
  R->irng.seed(seed ^ 0x5DEECE66DULL);
  R->seed = seed;
  R->xrng.seed(test_stream_seed(seed, -1));
  const char* eah = std::getenv("SFX_AHEAD");
  R->ahead_on = !(eah && eah[0] == '0');
  R->env_reset = reset_fn;
  R->env_step = step_fn;
  R->env_ctx = env_ctx;
  const char* ep = std::getenv("SFX_RUNNER_PIPELINE");
  R->pipeline = !(ep && ep[0] == '0');
  const int n_s = h->n_s, d = h->d;
  R->rs.assign((size_t)capacity * n_s, 0.f);
  R->rs1.assign((size_t)capacity * n_s, 0.f);
  R->rphi.assign((size_t)capacity * d, 0.f);
  R->rr.assign(capacity, 0.f);
  R->rgam.assign(capacity, 0.f);
  R->ra.assign(capacity, 0);
  R->s.assign(n_s, 0.f);
  R->s1.assign(n_s, 0.f);
  R->phi.assign(d, 0.f);
  R->gpi_counters.assign((size_t)h->T * h->T, 0);
  R->lay = runner_layout(batch, n_s, d);
  int rc = SFX_OK;
  auto fail = [&](const char* m) {
    g_err = m;
    rc = SFX_E_HIP;
  };
  if (hipHostMalloc((void**)&R->hst, R->lay.bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    fail("hipHostMalloc(staging) failed");
  if (!rc && hipHostMalloc((void**)&R->go, 64, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    fail("hipHostMalloc(go) failed");
  if (!rc && hipHostMalloc((void**)&R->res, sizeof(HostResult) * RES_RING, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
    fail("hipHostMalloc(result) failed");
  if (!rc && hipMalloc((void**)&R->dst, R->lay.bytes) != hipSuccess) fail("hipMalloc(staging) failed");
  if (!rc && hipMalloc((void**)&R->dctr, 64) != hipSuccess) fail("hipMalloc(counter) failed");
  if (!rc && (hipMalloc((void**)&R->dloss, sizeof(float) * sfx_runner::DLOSS_N) != hipSuccess ||
              hipMemset(R->dloss, 0, sizeof(float) * sfx_runner::DLOSS_N) != hipSuccess))
    fail("hipMalloc(losses) failed");
  if (!rc) {
    if (hipExtMallocWithFlags((void**)&R->dpush, R->lay.bytes, hipDeviceMallocFinegrained) != hipSuccess ||
        hipExtMallocWithFlags((void**)&R->dgo, 64, hipDeviceMallocFinegrained) != hipSuccess ||
        hipMemset(R->dgo, 0, 64) != hipSuccess || hipMemset(R->dpush, 0, R->lay.bytes) != hipSuccess) {
      if (R->dpush) (void)hipFree(R->dpush);
      if (R->dgo) (void)hipFree(R->dgo);
      R->dpush = nullptr;  // pull staging
      R->dgo = nullptr;
      (void)hipGetLastError();
    }
  }
  if (!rc && R->pipeline) {
    bool indep = false;
    rc = create_side_stream(h->stream, &R->side, &indep);
    if (!rc && !indep) R->pipeline = false;  // host rounds would queue behind a pre-launched gate
  } else if (!rc && hipStreamCreateWithFlags(&R->side, hipStreamNonBlocking) != hipSuccess) {
    fail("hipStreamCreate failed");
  }
  if (!rc) {
    std::memset(R->hst, 0, R->lay.bytes);
    std::memset(R->go, 0, 64);  // go, the cancel and hold words
    std::memset(R->res, 0, sizeof(HostResult) * RES_RING);
    if (hipMemset(R->dctr, 0, 64) != hipSuccess || hipMemset(R->dst, 0, R->lay.bytes) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess)
      fail("hipMemset failed");
  }
  if (rc) {
    sfx_runner_destroy(R);
    return rc;
  }
  *out = R;
  return SFX_OK;
}

int sfx_runner_destroy(sfx_runner_t R) {
  if (!R) return SFX_OK;
  if (R->inflight) (void)runner_complete(R);
  if (R->h) (void)hipStreamSynchronize(R->h->stream);
  if (R->side) (void)hipStreamDestroy(R->side);
  if (R->hst) (void)hipHostFree(R->hst);
  if (R->go) (void)hipHostFree(R->go);
  if (R->res) (void)hipHostFree(R->res);
  if (R->dst) (void)hipFree(R->dst);
  if (R->dctr) (void)hipFree(R->dctr);
  if (R->dloss) (void)hipFree(R->dloss);
  if (R->dpush) (void)hipFree(R->dpush);
  if (R->dgo) (void)hipFree(R->dgo);
  if (R->tres) (void)hipHostFree(R->tres);
  for (void* p : {(void*)R->tsel, (void*)R->tdseq})
    if (p) (void)hipFree(p);
  for (const sfx_runner::TestPhaseBufs& b : R->tp) {
    if (b.st) (void)hipHostFree(b.st);
    if (b.blk) (void)hipFree(b.blk);
    if (b.loss) (void)hipFree(b.loss);
  }
  for (void* p : {(void*)R->drs, (void*)R->drs1, (void*)R->drphi, (void*)R->drr, (void*)R->drg, (void*)R->dra})
    if (p) (void)hipFree(p);
  delete R;
  return SFX_OK;
}

int sfx_runner_layout(sfx_runner_t R, int64_t* offsets_host) {
  if (!R || !offsets_host) SFX_FAIL(SFX_E_ARG, "null argument");
  const RunnerLayout& L = R->lay;
  const size_t v[10] = {L.s, L.s1, L.phi, L.a, L.gamma, L.snext, L.phi1, L.r1, L.rb, L.bytes};
  for (int i = 0; i < 10; ++i) offsets_host[i] = (int64_t)v[i];
  return SFX_OK;
}

int sfx_runner_config(sfx_runner_t R, int schedule, int use_gpi, float p_end) {
  if (!R || schedule < RUN_ALL || schedule > RUN_TSF_PHI || p_end < 0.f || p_end > 1.f) SFX_FAIL(SFX_E_ARG, "bad args");
  if (R->feat && schedule != RUN_ACTIVE && schedule != RUN_TSF)
    SFX_FAIL(SFX_E_STATE, std::string("sfx_runner_config: a featurizer is set (sfx_runner_featurizer), which runs with the "
                                      "active and tsf schedules only, not with schedule ") +
                              std::to_string(schedule) + " (" + RUN_NAMES[schedule] + "); clear it first");
  if ((schedule == RUN_TSF || schedule == RUN_SHARD_TSF) && !R->h->tsf)
    SFX_FAIL(SFX_E_STATE, "sfx_runner_config: tsf schedule needs sfx_tsf_setup");
  if ((schedule == RUN_SHARD || schedule == RUN_SHARD_TSF) && R->h->comm_world < 1)
    SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the sharded schedule needs a communicator (sfx_comm_init / sfx_set_comm*)");
  if (schedule == RUN_SHARD && !use_gpi)
    SFX_FAIL(SFX_E_ARG, "sfx_runner_config: the sharded schedule is features/deep.py's all-task update (GPI next actions)");
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_config: a step is pre-launched");
  if (phi_sched(schedule)) {
    if (!R->phi_bias || !R->phi_lam)
      SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the learned-φ schedules need the per-task scalars (sfx_runner_phi_scalars)");
    if (R->dev_replay)
      SFX_FAIL(SFX_E_STATE, "sfx_runner_config: the learned-φ schedules do not run with device replay (switch it off first)");
    RC(phi_runner_prepare(R->h, schedule == RUN_TSF_PHI));  // allocates: here, never inside a capture
  }
  if (schedule == RUN_SHARD || schedule == RUN_SHARD_TSF) {
    RC(schedule == RUN_SHARD ? shard_buffers(R->h) : shard_tsf_buffers(R->h));
    R->gpi_counters.assign((size_t)R->h->Tg * R->h->Tg, 0);
    clear_graphs(R->h);
  } else if (R->gpi_counters.size() != (size_t)R->h->T * R->h->T) {
    R->gpi_counters.assign((size_t)R->h->T * R->h->T, 0);
  }
  R->schedule = schedule;
  R->upd_use_gpi = use_gpi ? 1 : 0;
  R->p_end = p_end;
  return SFX_OK;
}

int sfx_runner_device_replay(sfx_runner_t R, int enable) {
  if (!R) SFX_FAIL(SFX_E_ARG, "null runner");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_device_replay: a step is pre-launched");
  if (enable && phi_sched(R->schedule))
    SFX_FAIL(SFX_E_STATE, "sfx_runner_device_replay: the learned-φ schedules (phi, tsf_phi) keep the replay on the host");
  if (enable && R->feat)
    SFX_FAIL(SFX_E_STATE, "sfx_runner_device_replay: a featurizer is set (sfx_runner_featurizer), which keeps the replay "
                          "on the host; clear it first");
  if (enable && !R->drs) {
    if (R->lay.ax - R->lay.snext > (size_t)REPLAY_TAIL_MAX)
      SFX_FAIL(SFX_E_ARG, "sfx_runner_device_replay: state / feature sizes exceed the gate's staging");
    const size_t cap = (size_t)R->cap, n_s = R->h->n_s, d = R->h->d;
    void** p[6] = {(void**)&R->drs, (void**)&R->drs1, (void**)&R->drphi, (void**)&R->drr, (void**)&R->drg,
                   (void**)&R->dra};
    const size_t bytes[6] = {4 * cap * n_s, 4 * cap * n_s, 4 * cap * d, 4 * cap, 4 * cap, 8 * cap};
    for (int i = 0; i < 6; ++i)
      if (hipMalloc(p[i], bytes[i]) != hipSuccess) SFX_FAIL(SFX_E_HIP, "sfx_runner_device_replay: hipMalloc failed");
  }
  R->dev_replay = enable ? 1 : 0;
  R->dring_dirty = true;
  return SFX_OK;
}

int sfx_runner_featurizer(sfx_runner_t R, sfx_pre_t p) {
  if (!R) SFX_FAIL(SFX_E_ARG, "sfx_runner_featurizer: null runner");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_featurizer: a step is pre-launched");
  if (p) {
    int n_s = 0, d = 0;
    pre_dims(p, &n_s, &d);
    if (n_s != R->h->n_s || d != R->h->d)
      SFX_FAIL(SFX_E_ARG, "sfx_runner_featurizer: the featurizer's n_s = " + std::to_string(n_s) + ", d = " +
                              std::to_string(d) + " differ from the handle's n_s = " + std::to_string(R->h->n_s) +
                              ", d = " + std::to_string(R->h->d));
    if (R->schedule != RUN_ACTIVE && R->schedule != RUN_TSF)
      SFX_FAIL(SFX_E_STATE, std::string("sfx_runner_featurizer: a featurizer runs with the active and tsf schedules only, "
                                        "not with schedule ") +
                                std::to_string(R->schedule) + " (" + RUN_NAMES[R->schedule] + ")");
    if (R->dev_replay)
      SFX_FAIL(SFX_E_STATE, "sfx_runner_featurizer: a featurizer keeps the replay on the host (device replay is on; "
                            "switch it off first)");
    clear_graphs(R->h);  // the step graphs hold the net's geometry and pointers: none may outlive a handle's address
  }
  if (p != R->feat) R->chain = false;
  R->feat = p;
  return SFX_OK;
}

int sfx_runner_set_task(sfx_runner_t R, int task) {
  if (!R || task < 0 || task >= (sharded_sched(R) ? R->h->Tg : R->h->T)) SFX_FAIL(SFX_E_ARG, "bad task");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  R->task = task;
  R->steps_in_ep = 0;
  RC(env_reset(R, R->s.data()));
  return runner_select_initial(R);
}

int sfx_runner_prefill(sfx_runner_t R, int n) {
  if (!R || n < 0) SFX_FAIL(SFX_E_ARG, "bad args");
  RunnerScope scope(R->h);
  std::uniform_int_distribution<int> ua(0, R->h->A - 1);
  std::vector<float> s0(R->h->n_s);
  for (int i = 0; i < n; ++i) {
    RC(env_reset(R, s0.data()));
    const int a = ua(R->rng);
    float r = 0.f;
    int term = 0;
    RC(env_step(R, a, R->s1.data(), R->phi.data(), &r, &term));
    replay_append(R, s0.data(), a, r, R->phi.data(), R->s1.data(), R->gamma);
  }
  R->dring_dirty = true;
  return SFX_OK;
}

int runner_run(sfx_runner* R, int n);

// Look-ahead applies with the host replay to the all-task schedule when the fused post-update
// forward holds the extra rows, and to the active-task and TSF schedules (their select forwards the
// next minibatch; TSF: with its kernels on the step stream) (SFX_AHEAD=0: off)
bool runner_ahead_ok(const sfx_runner* R) {
  if (!R->ahead_on || R->dev_replay || phi_sched(R->schedule)) return false;  // learned φ: no look-ahead yet
  // frozen featurizer: the active schedule's look-ahead block holds states only and stays; the TSF one carries
  // the next minibatch's φ rows from the host, which are not the net's
  if (R->feat && R->schedule != RUN_ACTIVE) return false;
  if (R->schedule == RUN_ALL) return can_fuse_ahead(R->h, R->B + 1, R->B);
  // the sharded all-task step whose maxima come from k_qmax launches (the fused maxima accumulate
  // round 0's GPI terms in the step's own S1 forward)
  if (R->schedule == RUN_SHARD) return !shard_fused(R->h, R->B) && can_fuse_ahead(R->h, R->B + 1, R->B);
  return R->schedule == RUN_ACTIVE || ((R->schedule == RUN_TSF || R->schedule == RUN_SHARD_TSF) && R->h->tsf);
}

// On any failure (an env callback, a launch, the device) the steps queued behind the host are
// cancelled before the error returns: the heads hold the last completed step, and the runner
// can run again.
int sfx_runner_run(sfx_runner_t R, int n) {
  if (!R || n < 0) SFX_FAIL(SFX_E_ARG, "bad args");
  RunnerScope scope(R->h);
  const int rc = runner_run(R, n);
  if (rc) {
    const std::string e = g_err;
    runner_abort(R, true);
    g_err = e;
  }
  return rc;
}

int runner_run(sfx_runner* R, int n) {
  sfx_handle* h = R->h;
  if (R->broken) SFX_FAIL(SFX_E_STATE, R->broken_why.c_str());
  if (sharded_sched(R) && h->comm_dead) SFX_FAIL(SFX_E_STATE, h->comm_err.c_str());
  const int n_s = h->n_s, d = h->d;
  std::uniform_int_distribution<int> ua(0, h->A - 1);
  if (R->dev_replay && R->dring_dirty) {
    RC(runner_complete(R));
    RC(replay_upload(R));
  }
  const bool shard = R->schedule == RUN_SHARD, shard_any = sharded_sched(R);
  const bool ahead = runner_ahead_ok(R);
  if (R->chain_gen != h->gen) R->chain = false;  // the handle was used in between (ADVICE r4)
  if (ahead != R->ahead) {
    R->chain = false;
    R->plans.clear();
  }
  R->ahead = ahead;
  // sharded steps with collectives: with the host rounds' own communicator (comm_rounds, split off
  // by sfx_comm_init / sfx_set_comm) the steps pipeline like the all-task schedule -- the rounds'
  // all-reduces (side stream) and the pre-launched steps' (step stream) use different
  // communicators, each in the same order on every rank.  Without it (host transport) the next
  // step's graph goes out only once this step is complete -- never while a step may still need
  // host rounds -- and waits at its gate while the host runs the env and the replay.
  const bool shard_coll = shard_any && coll_active(h) && !h->comm_rounds;
  const int Tc = shard_any ? h->Tg : h->T;  // GPI tasks are global indices in the sharded schedules
  for (int i = 0; i < n; ++i) {
    RC(runner_complete(R));  // the greedy action for R->s
    if (shard_coll && R->pipeline && !h->prof && h->use_graphs && coll_capturable(h) && R->pre_n == 0) {
      const bool next_have = std::min<long>(R->rsize + 1, R->cap) >= R->B;
      RC(runner_prelaunch(R, next_have, true, 1, {false, false, 0}));
    }
    const long long c = R->sel_c;
    // SF.GPI(..., update_counters=self.use_gpi) (agents/sfdqn.py:41): counted only with GPI selection
    if (R->sel_use_gpi)
      R->gpi_counters[(size_t)R->task * Tc + (size_t)std::max<long long>(0, std::min<long long>(c, Tc - 1))] += 1;
    int a = (int)R->sel_a;
    if (R->uni() <= R->eps) a = ua(R->rng);  // ε-greedy (agents/agent.py:144-157)
    float r = 0.f;
    int term = 0;
    RC(env_step(R, a, R->s1.data(), R->phi.data(), &r, &term));
    const float g = term ? 0.f : R->gamma;
    const long slot = R->ridx;
    replay_append(R, R->s.data(), a, r, R->phi.data(), R->s1.data(), g);
    R->cur_step = R->env_steps;
    const bool have = R->rsize >= R->B;
    if (R->dev_replay) {  // hand over the transition; the gate appends and samples on the device
      ReplayMeta* m = reinterpret_cast<ReplayMeta*>(R->hst + R->lay.tr_meta);
      m->a = a;
      m->slot = slot;
      m->size = R->rsize;
      m->key = R->rng();
      m->r = r;
      m->gamma = g;
      m->have = have ? 1 : 0;
      std::memcpy(R->hst + R->lay.tr_s, R->s.data(), sizeof(float) * n_s);
      std::memcpy(R->hst + R->lay.tr_s1, R->s1.data(), sizeof(float) * n_s);
      std::memcpy(R->hst + R->lay.tr_phi, R->phi.data(), sizeof(float) * d);
      if (have && R->rec_n < R->rec_cap) replay_sample_keyed(R, m->key);
    } else {
      R->dring_dirty = true;
      if (have) replay_sample(R);
    }
    R->steps_in_ep += 1;
    float* sn = reinterpret_cast<float*>(R->hst + R->lay.snext);
    if (term || R->steps_in_ep >= R->ep_len) {  // new episode (agents/agent.py:211-220, 248-249)
      RC(env_reset(R, sn));
      R->steps_in_ep = 0;
    } else {
      std::memcpy(sn, R->s1.data(), sizeof(float) * n_s);
    }
    std::memcpy(R->hst + R->lay.phi1, R->phi.data(), sizeof(float) * d);
    std::memcpy(R->hst + R->lay.r1, &r, sizeof(float));
    if (R->rec_n < R->rec_cap) {
      std::memcpy(&R->rec_stage[(size_t)R->rec_n * R->lay.bytes], R->hst, R->lay.bytes);
      long long* m = &R->rec_meta[(size_t)R->rec_n * 6];
      m[0] = R->task;
      m[1] = have;
      m[2] = c;
      m[3] = R->sel_a;
      m[4] = a;
      m[5] = term;
      R->rec_n += 1;
    }
    std::memcpy(R->s.data(), sn, sizeof(float) * n_s);
    RC(runner_issue(R, have, R->schedule == RUN_ALL || shard));
    R->env_steps += 1;
    // pre-launch the next step's graph behind this one (its gate waits for the host)
    if (!shard_coll && R->pipeline && !h->prof && h->use_graphs && i + 1 < n && R->pre_n == 0) {
      // no pre-launch across a target sync (its copy must land between two steps): none after
      // this step, and a graph of `span` steps only when none of its first span - 1 ends with one
      const int upd = have ? 1 : 0;
      long left = 1L << 40;  // updates until the first head's next sync
      const auto chk = [&](int t) { left = std::min<long>(left, (long)h->target_update_ev - h->since_target[t]); };
      if (R->schedule == RUN_SHARD_TSF) {
        if (own_loc(R) >= 0) chk(own_loc(R));  // only the owner's head syncs
      } else if (R->schedule != RUN_ALL && !shard)
        chk(R->task);
      else
        for (int t = 0; t < h->T; ++t) chk(t);
      const bool sync_due = have && left <= 1;
      if (!sync_due) {
        const bool next_have = std::min<long>(R->rsize + 1, R->cap) >= R->B;
        const int span_max = R->span_max;
        // look-ahead: the span's first step starts at its TD launch when this step forwards its
        // (clean) minibatch; the span ends before a dirty step, which runs its own forward
        sfx_runner::StepFlags fl0{false, false, 0};
        const bool ahd = R->ahead && next_have;
        if (ahd) {
          fl0.par = (int)((R->seq + 1) & 1);
          const sfx_runner::MbPlan& p1 = plan_of(R, R->cur_step + 1);
          fl0.pre = R->chain && p1.early && !p1.dirty;
          fl0.ahead = true;
        }
        int span = 1;
        while (span < span_max && next_have && i + span + 1 < n && upd + span < left &&
               (!ahd || !plan_of(R, R->cur_step + 1 + span).dirty))
          ++span;
        RC(runner_prelaunch(R, next_have, R->schedule == RUN_ALL || shard, span, fl0));
      }
    }
  }
  return runner_complete(R);
}

// ---- native test phase (agents/sfdqn.py:105-120 over test_agent :139-166) ----

int sfx_runner_test_env(sfx_runner_t R, sfx_env_reset_fn reset_fn, sfx_env_step_fn step_fn, void* ctx) {
  if (!R) SFX_FAIL(SFX_E_ARG, "sfx_runner_test_env: null runner");
  if ((!reset_fn) != (!step_fn)) SFX_FAIL(SFX_E_ARG, "sfx_runner_test_env: both test env callbacks or none");
  R->tenv_reset = reset_fn;
  R->tenv_step = step_fn;
  R->tenv_ctx = reset_fn ? ctx : nullptr;
  return SFX_OK;
}

namespace {

using TestPhaseBufs = sfx_runner::TestPhaseBufs;

// A kind's buffers and what the kinds share; allocated here, never inside a capture.  A larger loss block
// replaces the old one: the graphs keyed on that one are never replayed again.
int test_phase_buffers(sfx_runner* R, int kind, const std::string& F, size_t st_bytes, size_t blk_bytes, size_t loss_need) {
  if (!R->tres) {
    if (hipHostMalloc((void**)&R->tres, sizeof(TestResult), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
      SFX_FAIL(SFX_E_HIP, "sfx_runner_test_phase: hipHostMalloc(result) failed");
    std::memset(R->tres, 0, sizeof(TestResult));
  }
  if (!R->tsel) {
    HIPCHK(hipMalloc((void**)&R->tsel, sizeof(int64_t) * 2 * TEST_EMAX));
    HIPCHK(hipMemset(R->tsel, 0, sizeof(int64_t) * 2 * TEST_EMAX));
  }
  if (!R->tdseq) {
    HIPCHK(hipMalloc((void**)&R->tdseq, 64));
    HIPCHK(hipMemset(R->tdseq, 0, 64));
  }
  TestPhaseBufs& b = R->tp[kind];
  if (!b.st) {
    if (hipHostMalloc((void**)&b.st, st_bytes, hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess)
      SFX_FAIL(SFX_E_HIP, F + "hipHostMalloc(staging) failed");
    std::memset(b.st, 0, st_bytes);
  }
  if (!b.blk) {
    HIPCHK(hipMalloc((void**)&b.blk, blk_bytes));
    HIPCHK(hipMemset(b.blk, 0, blk_bytes));
  }
  if (b.loss_n < loss_need) {
    HIPCHK(hipStreamSynchronize(R->h->stream));
    if (b.loss) (void)hipFree(b.loss);
    b.loss = nullptr;
    b.loss_n = 0;
    HIPCHK(hipMalloc((void**)&b.loss, sizeof(float) * loss_need));
    b.loss_n = loss_need;
  }
  return SFX_OK;
}

// One lockstep step's launch set of the SF phase on h->stream: intake; when `full`, the forward of all heads
// on the E rows chunked by max_batch (sfx_test_actions' launches), the GPI selection with per-row W, and
// the publication.  The phase's trailing launch (the last transitions' updates) is the intake alone.
int test_step_body(sfx_runner* R, int E, int horizon, float* W, int w_stride, bool full) {
  sfx_handle* h = R->h;
  const TestPhaseBufs& b = R->tp[sfx_runner::TP_SF];
  const TestStageLayout L = test_stage_layout(h->n_s, h->d);
  float* S = reinterpret_cast<float*>(b.blk);
  TestIntakeArgs A{};
  A.stage = b.st;
  A.off_phi = L.phi;
  A.off_s1 = L.s1;
  A.E = E;
  A.d = h->d;
  A.n_s = h->n_s;
  A.w_stride = w_stride;
  A.horizon = horizon;
  A.W = W;
  A.S = S;
  A.loss = b.loss;
  A.dseq = R->tdseq;
  hipLaunchKernelGGL(k_test_intake, dim3(1), dim3(256), 0, h->stream, A);
  LAUNCHCHK();
  if (!full) return SFX_OK;
  for (int row0 = 0; row0 < E; row0 += h->Mmax) {
    const int m = E - row0 < h->Mmax ? E - row0 : h->Mmax;
    RC(run_fwd(h, {{R_G, P_ONLINE, 1, 0, h->T}}, m, S + (size_t)row0 * h->n_s, nullptr));
    GpiArgs g = gpi_args(R_G, 0, row0, W, nullptr, nullptr, nullptr, nullptr, R->tsel, 0, 1, m);
    g.w_stride = w_stride;
    g.sel_stride = 2;
    RC(run_gpi(h, g));
  }
  hipLaunchKernelGGL(k_test_publish, dim3(1), dim3(128), 0, h->stream, (const int64_t*)R->tsel, E,
                     (const long long*)R->tdseq, R->tres);
  LAUNCHCHK();
  return SFX_OK;
}

// cached per (E, w_stride, W, horizon's loss block): at most two graphs a phase (full / trailing)
int test_step_launch(sfx_runner* R, int E, int horizon, float* W, int w_stride, bool full) {
  sfx_handle* h = R->h;
  const TestPhaseBufs& b = R->tp[sfx_runner::TP_SF];
  const GraphKey key = make_key(27, {E, w_stride, horizon, full ? 1 : 0}, h->mask,
                                {W, b.st, R->tres, b.blk, R->tsel, b.loss, R->tdseq});
  return run_graph(h, key, [&]() -> int { return test_step_body(R, E, horizon, W, w_stride, full); });
}

// cached per (E, strides, horizon, the caller's blocks, the phase's buffers): one graph a phase
int tsf_test_step_launch(sfx_runner* R, int E, int horizon, float* W, int w_stride, float* Om, int o_stride, float* mom,
                         int mom_stride) {
  sfx_handle* h = R->h;
  const TestPhaseBufs& b = R->tp[sfx_runner::TP_TSF];
  const GraphKey key = make_key(28, {E, w_stride, o_stride, mom_stride, horizon}, h->mask,
                                {W, Om, mom, b.st, R->tres, b.blk, b.loss, R->tsel, R->tdseq, tsf_test_phase_tgf(h)});
  return run_graph(h, key, [&]() -> int {
    return tsf_test_phase_body(R, E, horizon, W, w_stride, Om, o_stride, mom, mom_stride);
  });
}

// cached per (E, w_stride, horizon, the caller's W and Wb, the phase's buffers, the φ state's): one graph a phase
int phi_test_step_launch(sfx_runner* R, int E, int horizon, float* W, int w_stride, float* Wb) {
  sfx_handle* h = R->h;
  const TestPhaseBufs& b = R->tp[sfx_runner::TP_PHI];
  const void* ps[3];
  phi_test_phase_ptrs(h, ps);
  const GraphKey key =
      make_key(29, {E, w_stride, horizon}, h->mask, {W, Wb, b.st, R->tres, b.blk, b.loss, R->tsel, ps[0], ps[1], ps[2]});
  return run_graph(h, key, [&]() -> int {
    return phi_test_phase_body(h, E, horizon, W, w_stride, Wb, b.st, b.blk, b.loss, R->tsel, R->tres);
  });
}

// Wait (bounded by sfx_runner_wait_timeout) for launch set `seq` to publish its selections.
int test_wait(sfx_runner* R, long long seq) {
  const auto t0 = std::chrono::steady_clock::now();
  long spins = 0;
  while (__atomic_load_n(&R->tres->seq, __ATOMIC_ACQUIRE) < seq) {
    if ((++spins & 1023) == 0) {
      const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (el > R->wait_bound) {
        char msg[160];
        std::snprintf(msg, sizeof(msg), "sfx_runner_test_phase: lockstep launch %lld did not publish within %.3g s", seq,
                      R->wait_bound);
        (void)stream_drain(R->h->stream, std::max(30.0, R->wait_bound));
        SFX_FAIL(SFX_E_STATE, msg);
      }
    }
  }
  return SFX_OK;
}

int test_env_reset(sfx_runner* R, int e, float* s0) {
  if (R->tenv_reset) {
    if (R->tenv_reset(R->tenv_ctx, e, s0)) SFX_FAIL(SFX_E_STATE, "sfx_runner_test_phase: test env reset callback failed");
    return SFX_OK;
  }
  std::normal_distribution<float> nd(0.f, 1.f);
  for (int k = 0; k < R->h->n_s; ++k) s0[k] = nd(R->trng[e]);
  return SFX_OK;
}

// built-in synthetic test task e: the training synthetic task's shape (synth_step) on its own generator
int test_env_step(sfx_runner* R, int e, int a, float* s1, float* phi, float* r, int* terminal) {
  if (R->tenv_step) {
    if (R->tenv_step(R->tenv_ctx, e, a, s1, phi, r, terminal))
      SFX_FAIL(SFX_E_STATE, "sfx_runner_test_phase: test env step callback failed");
    return SFX_OK;
  }
  std::mt19937_64& g = R->trng[e];
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  const int d = R->h->d;
  for (int k = 0; k < R->h->n_s; ++k) s1[k] = nd(g);
  for (int k = 0; k < d; ++k) phi[k] = u01(g);
  *r = phi[e % d];
  *terminal = 0;  // never ends, like tasks/reacher.py:112
  return SFX_OK;
}

// what tells the three kinds of phase apart for lockstep_phase_run
struct LockstepSpec {
  int kind;                             // sfx_runner::TP_*
  std::string F;                        // the entry point's name, in front of its messages
  TestStageLayout L;                    // the kind's staging record
  size_t blk_bytes;                     // its device block
  int draws;                            // schedule entries per step: 1; TSF 2 (a, then a1, which the device reports)
  int comps;                            // loss components per row-step: 1; TSF 3
  bool trailing_intake;                 // SF: the last record's launch is the intake alone, which publishes nothing
  float neg_lr = 0.f, wd = 0.f;         // SF: the header's SGD constants
  const sfx_tsf_test_hp* hp = nullptr;  // TSF: the phase's hyperparameters
  long long* opt_steps = nullptr;       // TSF: [E] in/out
};

// The lockstep loop of every kind: draw the schedule, seed the built-in tasks, reset, launch the first record
// (every row's s0); then per step wait for the publication, step every live row's env on the published (or
// scheduled) action, stage the transitions and launch.  launch(full): one step's launch set; full is false only
// for a trailing intake.  Afterwards the loss block comes back and is summed per row in step order.
int lockstep_phase_run(sfx_runner* R, const LockstepSpec& sp, int E, int horizon, float test_epsilon, const int* explore,
                       double* returns, double* loss, long long* steps, long long* actions,
                       const std::function<int(bool full)>& launch) {
  sfx_handle* h = R->h;
  std::vector<int> drawn;
  if (!explore) {
    drawn.resize((size_t)E * horizon * sp.draws);
    draw_test_schedule(R->xrng, E, horizon * sp.draws, test_epsilon, h->A, drawn.data());
    explore = drawn.data();
  }
  if (!R->tenv_step)
    for (int e = (int)R->trng.size(); e < E; ++e) R->trng.emplace_back(test_stream_seed(R->seed, e));
  RC(test_phase_buffers(R, sp.kind, sp.F, sp.L.bytes, sp.blk_bytes, (size_t)E * horizon * sp.comps));
  const TestPhaseBufs& b = R->tp[sp.kind];
  TestPhaseHost P;
  std::vector<double> ret_tmp(E);
  std::vector<long long> steps_tmp(E);
  P.begin(sp.L, sp.draws, E, horizon, h->n_s, h->d, b.st, explore, returns ? returns : ret_tmp.data(),
          steps ? steps : steps_tmp.data(), actions);
  if (sp.hp) {
    TsfTestRowHP rhp;
    rhp.lr_w = (float)sp.hp->lr_w;
    rhp.wd_w = (float)sp.hp->wd_w;
    rhp.wd_omega = (float)sp.hp->wd_omega;
    rhp.lr_omega = sp.hp->lr_omega;
    rhp.lr_omega_decay = sp.hp->lr_omega_decay;
    P.begin_tsf(rhp, sp.hp->gamma, sp.hp->beta, sp.hp->lasso, sp.opt_steps);
  }
  // 0 <= v < A, or the phase stops: a published selection the host is about to act on or to report
  const auto published = [&](int e, int k, long long* v) -> int {
    *v = R->tres->sel[2 * e + k];
    if (*v < 0 || *v >= h->A) SFX_FAIL(SFX_E_STATE, sp.F + "corrupt published action");
    return SFX_OK;
  };
  // TSF: the a1 the device chose for the rows of the record just published (step j)
  const auto collect_a1 = [&](int j) -> int {
    for (int e = 0; e < E; ++e) {
      if (!P.in_record(e)) continue;
      long long a1;
      RC(published(e, 0, &a1));
      P.took_a1(e, j, a1);
    }
    return SFX_OK;
  };
  for (int e = 0; e < E; ++e) RC(test_env_reset(R, e, P.s1_row(e)));
  P.header(++R->tseq, 0, 0, sp.neg_lr, sp.wd);
  RC(launch(true));
  int last_j = -1;
  for (int j = 0; j < horizon; ++j) {
    RC(test_wait(R, R->tseq));
    if (sp.draws == 2 && j > 0) RC(collect_a1(j - 1));
    for (int e = 0; e < E; ++e) {
      if (!P.is_live(e)) {
        P.idle(e);
        continue;
      }
      long long greedy;
      RC(published(e, 1, &greedy));
      const int a = P.action(e, j, greedy);
      float r = 0.f;
      int term = 0;
      RC(test_env_step(R, e, a, P.s1_row(e), P.phi_row(e), &r, &term));  // no φ column: the callback's φ is not used
      P.took(e, j, a, r, term);
    }
    const bool last = P.end_step() == 0 || j + 1 == horizon;
    P.header(++R->tseq, j, 1, sp.neg_lr, sp.wd);
    RC(launch(!(last && sp.trailing_intake)));
    last_j = j;
    if (last) break;
  }
  if (!sp.trailing_intake) {  // the last record was launched like the others; a trailing intake is not waited for
    RC(test_wait(R, R->tseq));
    if (sp.draws == 2) RC(collect_a1(last_j));
  }
  std::vector<float> lh((size_t)E * horizon * sp.comps);
  HIPCHK(hipMemcpyAsync(lh.data(), b.loss, sizeof(float) * lh.size(), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (loss)
    for (int e = 0; e < E; ++e)
      for (int c = 0; c < sp.comps; ++c) {
        double acc = 0.0;  // accum_loss += loss.item() (and its siblings), in step order
        for (long long j = 0; j < P.steps[e]; ++j) acc += (double)lh[((size_t)j * E + e) * sp.comps + c];
        loss[(size_t)e * sp.comps + c] = acc;
      }
  return SFX_OK;
}

// ---- the entry points' refusals; each entry point calls them in its own order ----

// the caller has found E out of range; max_batch is named when it bounds E as well
int refuse_E(const std::string& F, int E, int emax, int max_batch) {
  const std::string lim = max_batch > 0 ? "min(" + std::to_string(emax) + ", max_batch = " + std::to_string(max_batch) + ")"
                                        : std::to_string(emax);
  SFX_FAIL(SFX_E_ARG, F + "E = " + std::to_string(E) + " test tasks, needs 1 <= E <= " + lim);
}
int need_horizon(const std::string& F, int horizon) {
  if (horizon < 1) SFX_FAIL(SFX_E_ARG, F + "horizon = " + std::to_string(horizon) + ", needs horizon >= 1");
  return SFX_OK;
}
int need_stride(const std::string& F, const char* name, int stride, const char* of, int least) {
  if (stride < least)
    SFX_FAIL(SFX_E_ARG, F + name + " = " + std::to_string(stride) + ", needs " + name + " >= " + of + " = " +
                            std::to_string(least));
  return SFX_OK;
}
int need_epsilon(const std::string& F, float test_epsilon) {
  if (!(test_epsilon >= 0.f && test_epsilon <= 1.f)) SFX_FAIL(SFX_E_ARG, F + "test_epsilon needs to be in [0, 1]");
  return SFX_OK;
}
// checked before the first step: a phase never stops after it has moved an env or a row
int need_explore(const std::string& F, const int* explore, size_t n, int A) {
  if (explore)
    for (size_t i = 0; i < n; ++i)
      if (explore[i] >= A) SFX_FAIL(SFX_E_ARG, F + "explore_host holds an action >= A = " + std::to_string(A));
  return SFX_OK;
}
int need_sound(sfx_runner* R) {
  if (R->broken) SFX_FAIL(SFX_E_STATE, R->broken_why.c_str());
  return SFX_OK;
}
int need_no_featurizer(const std::string& F, sfx_runner* R) {
  if (R->feat) SFX_FAIL(SFX_E_STATE, F + "a featurizer is set (sfx_runner_featurizer); clear it first");
  return SFX_OK;
}
// whose: "the SF agent's test phase runs with the all and active schedules only"
int need_schedule(const std::string& F, sfx_runner* R, bool ok, const char* whose) {
  if (!ok)
    SFX_FAIL(SFX_E_STATE,
             F + whose + ", not with schedule " + std::to_string(R->schedule) + " (" + RUN_NAMES[R->schedule] + ")");
  return SFX_OK;
}
// after the refusals, inside the entry point's RunnerScope: nothing of a training step in flight or pre-launched
int phase_prologue(const std::string& F, sfx_runner* R) {
  RC(settle(R->h));
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, F + "a step is pre-launched");
  return SFX_OK;
}
// a failed phase leaves nothing queued: the staging and the caller's rows are free again on return
int phase_drained(sfx_runner* R, int rc) {
  if (rc) {
    const std::string e = g_err;
    (void)stream_drain(R->h->stream, std::max(30.0, R->wait_bound));
    g_err = e;
  }
  return rc;
}

}  // namespace

// ---- the SF agent's test phase (agents/sfdqn.py:105-120 over test_agent :139-166) ----

int sfx_runner_test_phase(sfx_runner_t R, int E, int horizon, float test_epsilon, double lr, double wd, float* W_dev,
                          int w_stride, const int* explore_host, double* returns_host, double* loss_host,
                          long long* steps_host, long long* actions_host) {
  const std::string F = "sfx_runner_test_phase: ";
  if (!R) SFX_FAIL(SFX_E_ARG, F + "null runner");
  sfx_handle* h = R->h;
  if (E < 1 || E > TEST_EMAX) return refuse_E(F, E, TEST_EMAX, 0);
  RC(need_horizon(F, horizon));
  if (!W_dev) SFX_FAIL(SFX_E_ARG, F + "W_dev is null");
  RC(need_stride(F, "w_stride", w_stride, "d", h->d));
  RC(need_epsilon(F, test_epsilon));
  RC(need_explore(F, explore_host, (size_t)E * horizon, h->A));
  RC(need_sound(R));
  if (h->Tg != h->T) SFX_FAIL(SFX_E_STATE, F + "needs an unsharded handle");
  RC(need_schedule(F, R, R->schedule == RUN_ALL || R->schedule == RUN_ACTIVE,
                   "the SF agent's test phase runs with the all and active schedules only"));
  RC(need_no_featurizer(F, R));
  RunnerScope scope(h);
  RC(phase_prologue(F, R));
  LockstepSpec sp{sfx_runner::TP_SF, F, test_stage_layout(h->n_s, h->d), sizeof(float) * TEST_EMAX * h->n_s, 1, 1, true};
  sp.neg_lr = (float)(-lr);
  sp.wd = (float)wd;
  return phase_drained(R, lockstep_phase_run(R, sp, E, horizon, test_epsilon, explore_host, returns_host, loss_host,
                                             steps_host, actions_host, [&](bool full) -> int {
                                               return test_step_launch(R, E, horizon, W_dev, w_stride, full);
                                             }));
}

// ---- the TSF agent's test phase (agents/tsfdqn_sequential.py:363-369 over test_agent :392-433) ----

float sfx_tsf_test_lr_omega(double lr_omega, double decay, long long epoch) {
  return tsf_test_lr_omega(lr_omega, decay, epoch);
}

int sfx_runner_tsf_test_phase(sfx_runner_t R, int E, int horizon, float test_epsilon, const sfx_tsf_test_hp* hp,
                              float* W_dev, int w_stride, float* Omega_dev, int o_stride, float* adam_state_dev,
                              int mom_stride, long long* opt_steps_host, const int* explore_host, double* returns_host,
                              double* losses_host, long long* steps_host, long long* actions_host) {
  const std::string F = "sfx_runner_tsf_test_phase: ";
  if (!R) SFX_FAIL(SFX_E_ARG, F + "null runner");
  sfx_handle* h = R->h;
  if (E < 1 || E > TEST_EMAX) return refuse_E(F, E, TEST_EMAX, h->Mmax);  // E <= max_batch: tsf_test_phase_ready
  if (!hp || !W_dev || !Omega_dev || !adam_state_dev || !opt_steps_host)
    SFX_FAIL(SFX_E_ARG, F + "hp, W_dev, Omega_dev, adam_state_dev and opt_steps_host need to be non-null");
  RC(need_horizon(F, horizon));
  RC(need_stride(F, "w_stride", w_stride, "d", h->d));
  RC(need_stride(F, "o_stride", o_stride, "T", h->T));
  RC(need_stride(F, "mom_stride", mom_stride, "2(d + T)", 2 * (h->d + h->T)));
  RC(need_epsilon(F, test_epsilon));
  for (int e = 0; e < E; ++e)
    if (opt_steps_host[e] < 0 || opt_steps_host[e] + horizon >= (1LL << 24))
      SFX_FAIL(SFX_E_ARG, F + "opt_steps_host[" + std::to_string(e) + "] = " + std::to_string(opt_steps_host[e]) +
                              ", needs opt_steps >= 0 and opt_steps + horizon < 2^24");
  RC(need_explore(F, explore_host, (size_t)E * horizon * 2, h->A));
  RC(need_sound(R));
  if (!h->tsf) SFX_FAIL(SFX_E_STATE, F + "call sfx_tsf_setup first (and load every g_t and h)");
  RC(need_schedule(F, R, R->schedule == RUN_TSF, "the TSF agent's test phase runs with the tsf schedule only"));
  RC(need_no_featurizer(F, R));
  RunnerScope scope(h);
  RC(phase_prologue(F, R));
  RC(tsf_test_phase_ready(h, E));
  LockstepSpec sp{sfx_runner::TP_TSF, F, tsf_test_stage_layout(h->n_s, h->d), tsf_test_dev_layout(h->n_s, h->d).bytes, 2, 3,
                  false};
  sp.hp = hp;
  sp.opt_steps = opt_steps_host;
  return phase_drained(R, lockstep_phase_run(R, sp, E, horizon, test_epsilon, explore_host, returns_host, losses_host,
                                             steps_host, actions_host, [&](bool) -> int {
                                               return tsf_test_step_launch(R, E, horizon, W_dev, w_stride, Omega_dev,
                                                                           o_stride, adam_state_dev, mom_stride);
                                             }));
}

// ---- the learned-φ SF agent's test phase (agents/sfdqn_phi.py:211-212 over test_agent :234-261) ----

int sfx_runner_phi_test_phase(sfx_runner_t R, int E, int horizon, float test_epsilon, float* W_dev, int w_stride,
                              float* Wb_dev, const int* explore_host, double* returns_host, double* loss_host,
                              long long* steps_host, long long* actions_host) {
  const std::string F = "sfx_runner_phi_test_phase: ";
  if (!R) SFX_FAIL(SFX_E_ARG, F + "null runner");
  sfx_handle* h = R->h;
  if (E < 1 || E > PHI_TEST_EMAX || E > h->Mmax) return refuse_E(F, E, PHI_TEST_EMAX, h->Mmax);
  RC(need_horizon(F, horizon));
  if (!W_dev || !Wb_dev) SFX_FAIL(SFX_E_ARG, F + "W_dev and Wb_dev need to be non-null");
  RC(need_stride(F, "w_stride", w_stride, "d", h->d));
  RC(need_epsilon(F, test_epsilon));
  RC(need_explore(F, explore_host, (size_t)E * horizon, h->A));
  RC(need_sound(R));
  RC(phi_test_phase_ready(h));  // an unsharded handle with a φ net
  RC(need_no_featurizer(F, R));
  RC(need_schedule(F, R, R->schedule == RUN_PHI, "the learned-φ SF agent's test phase runs with the phi schedule only"));
  RunnerScope scope(h);
  RC(phase_prologue(F, R));
  const LockstepSpec sp{sfx_runner::TP_PHI, F, phi_test_stage_layout(h->n_s), phi_test_dev_layout(h->n_s).bytes, 1, 1,
                        false};
  return phase_drained(R, lockstep_phase_run(R, sp, E, horizon, test_epsilon, explore_host, returns_host, loss_host,
                                             steps_host, actions_host, [&](bool) -> int {
                                               return phi_test_step_launch(R, E, horizon, W_dev, w_stride, Wb_dev);
                                             }));
}

int sfx_runner_action(sfx_runner_t R, int64_t* out_host) {
  if (!R || !out_host) SFX_FAIL(SFX_E_ARG, "null argument");
  RC(runner_complete(R));
  out_host[0] = R->sel_c;
  out_host[1] = R->sel_a;
  out_host[2] = R->task;
  return SFX_OK;
}

int sfx_runner_stats(sfx_runner_t R, long long* env_steps, long long* prelaunched, long long* host_round_steps,
                     double* wait_us) {
  if (!R) SFX_FAIL(SFX_E_ARG, "null runner");
  if (env_steps) *env_steps = R->env_steps;
  if (prelaunched) *prelaunched = R->prelaunched;
  if (host_round_steps) *host_round_steps = R->host_rounds;
  if (wait_us) *wait_us = R->wait_us;
  return SFX_OK;
}

int sfx_runner_warm(sfx_runner_t R) {
  if (!R) SFX_FAIL(SFX_E_ARG, "null runner");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  sfx_handle* h = R->h;
  if (!h->use_graphs || h->prof) return SFX_OK;
  const unsigned long long bits = step_bits(R);
  const unsigned long long m0 = h->mask;
  const int span_max =
      (R->schedule == RUN_SHARD && coll_active(h)) || (R->schedule == RUN_SHARD_TSF && !coll_capturable(h)) ? 1
                                                                                                          : R->span_max;
  const bool lms = R->schedule == RUN_ALL || R->schedule == RUN_SHARD;
  int rc = SFX_OK;
  const bool ahd = runner_ahead_ok(R);
  for (int par = 0; par < 2 && rc == SFX_OK; ++par) {
    h->mask = par ? m0 ^ bits : m0;
    for (int n = 1; n <= span_max && rc == SFX_OK; ++n) {
      if (!ahd) {
        rc = runner_launch(R, true, lms, n, false);
        continue;
      }
      for (int v = 0; v < 4 && rc == SFX_OK; ++v)  // (first step's pre, role copy of the first step)
        rc = runner_launch(R, true, lms, n, false, sfx_runner::StepFlags{(v & 1) != 0, true, v >> 1});
    }
  }
  h->mask = m0;
  if (rc == SFX_OK && R->pipeline) rc = warm_host_rounds(R, bits, ahd);
  return rc;
}

int sfx_runner_wait_timeout(sfx_runner_t R, double seconds) {
  if (!R || !(seconds > 0.0) || seconds > 600.0) SFX_FAIL(SFX_E_ARG, "wait timeout must be in (0, 600] s");
  R->wait_bound = seconds;
  return SFX_OK;
}

int sfx_runner_gate_timeout(sfx_runner_t R, double seconds) {
  if (!R || !(seconds > 0.0) || seconds > 600.0) SFX_FAIL(SFX_E_ARG, "gate timeout must be in (0, 600] s");
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_gate_timeout: a step is pre-launched");
  R->gate_timeout = std::max(1LL, (long long)(seconds * 1e8));
  clear_graphs(R->h);  // the bound is baked into the captured gates
  return SFX_OK;
}

int sfx_runner_ahead_stats(sfx_runner_t R, long long* pre_steps, long long* own_forward_steps) {
  if (!R) SFX_FAIL(SFX_E_ARG, "null runner");
  if (pre_steps) *pre_steps = R->pre_steps;
  if (own_forward_steps) *own_forward_steps = R->dirty_steps;
  return SFX_OK;
}

int sfx_runner_phi_scalars(sfx_runner_t R, float* bias_dev, float* lambda_dev) {
  if (!R || !bias_dev || !lambda_dev) SFX_FAIL(SFX_E_ARG, "sfx_runner_phi_scalars: null argument");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_phi_scalars: a step is pre-launched");
  R->phi_bias = bias_dev;
  R->phi_lam = lambda_dev;
  return SFX_OK;
}

int sfx_runner_phi_losses(sfx_runner_t R, float* out_host) {
  static_assert(sfx_runner::DLOSS_N >= 4, "the runner's loss buffer holds (loss, psi_loss, phi_loss, lambda)");
  if (!R || !out_host) SFX_FAIL(SFX_E_ARG, "sfx_runner_phi_losses: null argument");
  if (!phi_sched(R->schedule)) SFX_FAIL(SFX_E_STATE, "sfx_runner_phi_losses: the schedule is not phi or tsf_phi");
  RunnerScope scope(R->h);
  RC(runner_complete(R));
  // between runs nothing is queued behind the completed step (a queued step's gate would hold the stream)
  if (R->pre_n) SFX_FAIL(SFX_E_STATE, "sfx_runner_phi_losses: a step is pre-launched");
  HIPCHK(hipStreamSynchronize(R->h->stream));
  HIPCHK(hipMemcpy(out_host, R->dloss, sizeof(float) * 4, hipMemcpyDeviceToHost));
  return SFX_OK;
}

int sfx_runner_retried(sfx_runner_t R, long long* retried) {
  if (!R || !retried) SFX_FAIL(SFX_E_ARG, "null argument");
  *retried = R->retried;
  return SFX_OK;
}

int sfx_runner_nonfinite(sfx_runner_t R, long long* steps) {
  if (!R || !steps) SFX_FAIL(SFX_E_ARG, "bad args");
  *steps = R->nonfinite_steps;
  return SFX_OK;
}

int sfx_runner_recomputed(sfx_runner_t R, long long* recomputed) {
  if (!R || !recomputed) SFX_FAIL(SFX_E_ARG, "null argument");
  *recomputed = R->recomputed;
  return SFX_OK;
}

int sfx_runner_gpi_counters(sfx_runner_t R, long long* out_host) {
  if (!R || !out_host) SFX_FAIL(SFX_E_ARG, "null argument");
  std::memcpy(out_host, R->gpi_counters.data(), sizeof(long long) * R->gpi_counters.size());
  return SFX_OK;
}

int sfx_runner_record(sfx_runner_t R, int capacity) {
  if (!R || capacity < 0) SFX_FAIL(SFX_E_ARG, "bad args");
  R->rec_cap = capacity;
  R->rec_n = 0;
  R->rec_stage.assign((size_t)capacity * R->lay.bytes, 0);
  R->rec_meta.assign((size_t)capacity * 6, 0);
  return SFX_OK;
}

int sfx_runner_get_record(sfx_runner_t R, int i, void* stage_host, int64_t* meta_host) {
  if (!R || i < 0 || i >= R->rec_n) SFX_FAIL(SFX_E_ARG, "no such record");
  if (stage_host) std::memcpy(stage_host, &R->rec_stage[(size_t)i * R->lay.bytes], R->lay.bytes);
  if (meta_host)
    for (int k = 0; k < 6; ++k) meta_host[k] = R->rec_meta[(size_t)i * 6 + k];
  return SFX_OK;
}

int sfx_runner_recorded(sfx_runner_t R) { return R ? R->rec_n : 0; }

}  // extern "C"
