// sfx_test_host.h -- the host half of the native test phase (sfx_runner_test_phase, sfx_runner.inc)
// that needs no device: the staging record's layout, the test-phase random streams, the exploration
// schedule and the per-row bookkeeping of E lockstep episodes (agents/sfdqn.py:139-166).  Plain C++,
// so tools/hostsan/test_phase_hostsan.cpp drives it under the host sanitizers without a GPU.  The TSF agent's
// phase (sfx_runner_tsf_test_phase) has its own layout and bookkeeping below (tools/hostsan/tsf_test_phase_hostsan.cpp),
// and so has the learned-φ SF agent's (sfx_runner_phi_test_phase; tools/hostsan/phi_test_phase_hostsan.cpp).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <random>
#include <vector>

namespace sfx {

constexpr int TEST_EMAX = 64;       // test tasks of one phase
constexpr int TEST_PHI_LDS = 8192;  // φ floats k_test_intake stages in LDS (larger E·d: read from the staging)

// Staging record of one lockstep step (host-coherent, written by the host before each launch):
//   TestStageHdr | live[TEST_EMAX] (int) | r[TEST_EMAX] | φ [TEST_EMAX][d] | s1 [TEST_EMAX][n_s]
// live[e]: row e took the env step this record describes (the phase's first record: every row, its
// s0 in s1).  Rows are d / n_s floats apart whatever E is, so the offsets hold for every phase.
struct TestStageHdr {
  long long seq;     // sequence number of this launch set (published back by k_test_publish)
  int step, update;  // lockstep step the transitions belong to; update 0: no mapper step (first record)
  float neg_lr, wd;  // the SGD step's constants, narrowed as sfx_test_reward_updates narrows them
  int pad0_, pad1_;
};
static_assert(sizeof(TestStageHdr) == 32, "TestStageHdr: two 16-byte words");

struct TestStageLayout {
  int live, r, phi, s1;  // byte offsets, multiples of 16
  size_t bytes;
};

inline TestStageLayout test_stage_layout(int n_s, int d) {
  TestStageLayout L{};
  const auto up16 = [](size_t n) { return (n + 15) / 16 * 16; };
  L.live = (int)sizeof(TestStageHdr);
  L.r = L.live + 4 * TEST_EMAX;
  L.phi = L.r + 4 * TEST_EMAX;
  L.s1 = L.phi + (int)up16(sizeof(float) * TEST_EMAX * (size_t)d);
  L.bytes = (size_t)L.s1 + up16(sizeof(float) * TEST_EMAX * (size_t)n_s);
  return L;
}

// Seeds of the test phase's own generators, from (runner seed, a fixed test-phase constant, e):
// e >= 0 the built-in synthetic test task e, e = -1 the exploration schedule's stream.  splitmix64
// finaliser, so neighbouring seeds and tasks give unrelated streams; none is the training stream's.
inline unsigned long long test_stream_seed(unsigned long long seed, int e) {
  unsigned long long x = seed ^ 0x7E57FA5EC0FFEE11ull;
  x += (unsigned long long)(long long)(e + 2) * 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The exploration schedule of E sequential test episodes in the reference's order
// (SFDQN.get_test_action, agents/sfdqn.py:125-137): task-major, per step one uniform and, when it is
// <= epsilon, one randrange(n_actions).  out[e * horizon + j] = the explored action, or -1 (greedy).
template <class Rng>
inline void draw_test_schedule(Rng& g, int E, int horizon, float epsilon, int n_actions, int* out) {
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  std::uniform_int_distribution<int> ua(0, n_actions - 1);
  for (int e = 0; e < E; ++e)
    for (int j = 0; j < horizon; ++j) out[(size_t)e * horizon + j] = u01(g) <= epsilon ? ua(g) : -1;
}

// Bookkeeping of one phase: which rows still run, their returns / step counts / actions, and the
// writes into the staging record.  Per lockstep step j the loop calls, for every row, either
// took() (a live row's transition, written by the env callback into s1_row / phi_row) or idle(),
// then header() and, after the launch, end_step().
struct TestPhaseHost {
  int E = 0, horizon = 0, n_s = 0, d = 0;
  TestStageLayout L{};
  uint8_t* st = nullptr;
  const int* explore = nullptr;  // [E * horizon]
  double* ret = nullptr;         // [E]
  long long* steps = nullptr;    // [E]
  long long* actions = nullptr;  // [E * horizon] or null
  std::vector<char> live, done;

  int* live_w() const { return reinterpret_cast<int*>(st + L.live); }
  float* r_w() const { return reinterpret_cast<float*>(st + L.r); }
  float* phi_row(int e) const { return reinterpret_cast<float*>(st + L.phi) + (size_t)e * d; }
  float* s1_row(int e) const { return reinterpret_cast<float*>(st + L.s1) + (size_t)e * n_s; }

  void begin(int E_, int horizon_, int n_s_, int d_, uint8_t* staging, const int* explore_, double* ret_,
             long long* steps_, long long* actions_) {
    E = E_, horizon = horizon_, n_s = n_s_, d = d_;
    L = test_stage_layout(n_s, d);
    st = staging, explore = explore_, ret = ret_, steps = steps_, actions = actions_;
    live.assign(E, 1);
    done.assign(E, 0);
    for (int e = 0; e < E; ++e) {
      ret[e] = 0.0;
      steps[e] = 0;
      live_w()[e] = 1;  // the first record carries every row's s0
      r_w()[e] = 0.f;
    }
    for (int e = E; e < TEST_EMAX; ++e) live_w()[e] = 0;
    if (actions)
      for (size_t i = 0; i < (size_t)E * horizon; ++i) actions[i] = -1;
  }
  void header(long long seq, int step, int update, float neg_lr, float wd) const {
    TestStageHdr hd{seq, step, update, neg_lr, wd, 0, 0};
    std::memcpy(st, &hd, sizeof(hd));
  }
  bool is_live(int e) const { return live[e] != 0; }
  // the action row e takes at step j: the schedule's when it explores, else the greedy one
  int action(int e, int j, long long greedy) const {
    const int x = explore[(size_t)e * horizon + j];
    return x >= 0 ? x : (int)greedy;
  }
  void took(int e, int j, int a, float r, int terminal) {
    if (actions) actions[(size_t)e * horizon + j] = a;
    ret[e] += (double)r;  // the callback's float32 reward, added in double
    steps[e] += 1;
    live_w()[e] = 1;
    r_w()[e] = r;
    done[e] = terminal ? 1 : 0;
  }
  void idle(int e) const { live_w()[e] = 0; }
  // rows whose callback reported done got this step's update and stop (the reference's break);
  // returns the number of rows still running
  int end_step() {
    int n = 0;
    for (int e = 0; e < E; ++e) {
      if (done[e]) live[e] = 0;
      n += live[e] ? 1 : 0;
    }
    return n;
  }
};

// -------------------------------------------------------------------------------------
// The TSF agent's test phase (sfx_runner_tsf_test_phase; agents/tsfdqn_sequential.py:392-433): per
// lockstep step a row chooses a at s, steps its env, chooses a1 at s1 and takes one
// update_test_reward_mapper step on its own (w, ω) with its own Adam state and ω-lr schedule.
// -------------------------------------------------------------------------------------

// Staging record of one lockstep step of the TSF phase (host-coherent):
//   TestStageHdr | hp[4] = γ, β, λ, 0 | live[TEST_EMAX] (int) | r[TEST_EMAX] | a[TEST_EMAX] (int: the
//   action taken at s) | a1x[TEST_EMAX] (int: the explored a1, or -1 = greedy) | rowp [TEST_EMAX][6]
//   (sfx_tsf_test_updates' layout: r, lr_w, wd_w, lr_ω, wd_ω, Adam step) | φ [TEST_EMAX][d] |
//   s1 [TEST_EMAX][n_s]
// The header's neg_lr / wd are not used (0).  Everything in front of φ is TSF_TEST_PRE bytes whatever
// the shape is.
constexpr int TSF_TEST_PRE = (int)sizeof(TestStageHdr) + 16 + 4 * 4 * TEST_EMAX + 4 * 6 * TEST_EMAX;

struct TsfTestStageLayout {
  int hp, live, r, a, a1x, rowp, phi, s1;  // byte offsets, multiples of 16
  size_t bytes;
};

inline TsfTestStageLayout tsf_test_stage_layout(int n_s, int d) {
  TsfTestStageLayout L{};
  const auto up16 = [](size_t n) { return (n + 15) / 16 * 16; };
  L.hp = (int)sizeof(TestStageHdr);
  L.live = L.hp + 16;
  L.r = L.live + 4 * TEST_EMAX;
  L.a = L.r + 4 * TEST_EMAX;
  L.a1x = L.a + 4 * TEST_EMAX;
  L.rowp = L.a1x + 4 * TEST_EMAX;
  L.phi = L.rowp + 4 * 6 * TEST_EMAX;
  L.s1 = L.phi + (int)up16(sizeof(float) * TEST_EMAX * (size_t)d);
  L.bytes = (size_t)L.s1 + up16(sizeof(float) * TEST_EMAX * (size_t)n_s);
  return L;
}
static_assert(TSF_TEST_PRE % 16 == 0, "TSF_TEST_PRE: whole 16-byte words");

// lr of ω's parameter group at scheduler epoch `epoch`: LambdaLR over (1 - decay) ** epoch
// (agents/tsfdqn_sequential.py:344-348), narrowed as the row's float32 rowp entry is.
inline float tsf_test_lr_omega(double lr_omega, double decay, long long epoch) {
  return (float)(lr_omega * std::pow(1.0 - decay, (double)epoch));
}

// The exploration schedule of E sequential TSF test episodes in the reference's order
// (get_test_action at s, then at s1: agents/tsfdqn_sequential.py:377-381, :404-407): task-major, per
// step for a and then for a1 one uniform and, when it is <= epsilon, one randrange(n_actions).
// out[(e * horizon + j) * 2 + {0, 1}] = the explored a / a1, or -1 (greedy).
template <class Rng>
inline void draw_tsf_test_schedule(Rng& g, int E, int horizon, float epsilon, int n_actions, int* out) {
  draw_test_schedule(g, E, 2 * horizon, epsilon, n_actions, out);  // the same draws, two per step
}

// hyperparameters of a TSF phase as the rows' rowp entries carry them
struct TsfTestRowHP {
  float lr_w = 0.f, wd_w = 0.f, wd_omega = 0.f;
  double lr_omega = 0.0, lr_omega_decay = 0.0;
};

// Bookkeeping of one TSF phase; the loop is TestPhaseHost's with two additions: took() also writes
// the row's a, explored a1 and rowp (from its own optimizer step count, which it advances), and
// took_a1() records the a1 the device chose once the step's launch has published.
struct TsfTestPhaseHost {
  int E = 0, horizon = 0, n_s = 0, d = 0;
  TsfTestStageLayout L{};
  uint8_t* st = nullptr;
  const int* explore = nullptr;    // [E * horizon * 2]
  double* ret = nullptr;           // [E]
  long long* steps = nullptr;      // [E]
  long long* actions = nullptr;    // [E * horizon * 2] or null
  long long* opt_steps = nullptr;  // [E] in/out
  TsfTestRowHP hp;
  std::vector<char> live, done;

  int* live_w() const { return reinterpret_cast<int*>(st + L.live); }
  float* r_w() const { return reinterpret_cast<float*>(st + L.r); }
  int* a_w() const { return reinterpret_cast<int*>(st + L.a); }
  int* a1x_w() const { return reinterpret_cast<int*>(st + L.a1x); }
  float* rowp_row(int e) const { return reinterpret_cast<float*>(st + L.rowp) + (size_t)e * 6; }
  float* phi_row(int e) const { return reinterpret_cast<float*>(st + L.phi) + (size_t)e * d; }
  float* s1_row(int e) const { return reinterpret_cast<float*>(st + L.s1) + (size_t)e * n_s; }

  void begin(int E_, int horizon_, int n_s_, int d_, uint8_t* staging, const int* explore_, const TsfTestRowHP& hp_,
             float gamma, float beta, float lasso, long long* opt_steps_, double* ret_, long long* steps_,
             long long* actions_) {
    E = E_, horizon = horizon_, n_s = n_s_, d = d_;
    L = tsf_test_stage_layout(n_s, d);
    st = staging, explore = explore_, ret = ret_, steps = steps_, actions = actions_, opt_steps = opt_steps_;
    hp = hp_;
    const float g[4] = {gamma, beta, lasso, 0.f};
    std::memcpy(st + L.hp, g, sizeof(g));
    live.assign(E, 1);
    done.assign(E, 0);
    for (int e = 0; e < TEST_EMAX; ++e) {
      live_w()[e] = e < E ? 1 : 0;  // the first record carries every row's s0
      r_w()[e] = 0.f;
      a_w()[e] = 0;
      a1x_w()[e] = -1;
      for (int k = 0; k < 6; ++k) rowp_row(e)[k] = k == 5 ? 1.f : 0.f;
    }
    for (int e = 0; e < E; ++e) {
      ret[e] = 0.0;
      steps[e] = 0;
    }
    if (actions)
      for (size_t i = 0; i < (size_t)E * horizon * 2; ++i) actions[i] = -1;
  }
  void header(long long seq, int step, int update) const {
    TestStageHdr hd{seq, step, update, 0.f, 0.f, 0, 0};
    std::memcpy(st, &hd, sizeof(hd));
  }
  bool is_live(int e) const { return live[e] != 0; }
  // row e took the env step the staged record describes (its a1 is published by that record's launch)
  bool in_record(int e) const { return live_w()[e] != 0; }
  int action(int e, int j, long long greedy) const {
    const int x = explore[((size_t)e * horizon + j) * 2];
    return x >= 0 ? x : (int)greedy;
  }
  void took(int e, int j, int a, float r, int terminal) {
    if (actions) actions[((size_t)e * horizon + j) * 2] = a;
    ret[e] += (double)r;  // the callback's float32 reward, added in double
    steps[e] += 1;
    live_w()[e] = 1;
    r_w()[e] = r;
    a_w()[e] = a;
    a1x_w()[e] = explore[((size_t)e * horizon + j) * 2 + 1];
    float* p = rowp_row(e);
    p[0] = r;
    p[1] = hp.lr_w;
    p[2] = hp.wd_w;
    p[3] = tsf_test_lr_omega(hp.lr_omega, hp.lr_omega_decay, opt_steps[e]);
    p[4] = hp.wd_omega;
    p[5] = (float)(opt_steps[e] + 1);  // exact: the entry point bounds it by 2^24
    opt_steps[e] += 1;                 // optim.step() and scheduler.step()
    done[e] = terminal ? 1 : 0;
  }
  void took_a1(int e, int j, long long a1) const {
    if (actions) actions[((size_t)e * horizon + j) * 2 + 1] = a1;
  }
  void idle(int e) const { live_w()[e] = 0; }
  int end_step() {
    int n = 0;
    for (int e = 0; e < E; ++e) {
      if (done[e]) live[e] = 0;
      n += live[e] ? 1 : 0;
    }
    return n;
  }
};

// -------------------------------------------------------------------------------------
// The learned-φ SF agent's test phase (sfx_runner_phi_test_phase; agents/sfdqn_phi.py:234-261): per
// lockstep step a row chooses a at s, steps its env and takes one update_test_reward_mapper step
// (:263-305) on its own biased Linear(d, 1) with φ = phi_net(s ⊕ a ⊕ s1), computed on the device: the
// record carries no φ, and the env callback's φ output goes to a sink nobody reads.
// -------------------------------------------------------------------------------------

constexpr int PHI_TEST_EMAX = 16;  // test tasks of one phase: the E-row φ kernels' PHIE (sfx_phitest.h)
constexpr int PHI_TEST_NS = 32;    // n_s of a φ net's handle is at most 31 (2 n_s + 1 <= 64): k_phi_test_intake's LDS

// Staging record of one lockstep step of the φ phase (host-coherent):
//   TestStageHdr | live[PHI_TEST_EMAX] (int) | r[PHI_TEST_EMAX] | a[PHI_TEST_EMAX] (int: the action
//   taken at s) | s1 [PHI_TEST_EMAX][n_s]
// The header's neg_lr / wd are not used (0).  Everything in front of s1 is PHI_TEST_PRE bytes.
constexpr int PHI_TEST_PRE = (int)sizeof(TestStageHdr) + 3 * 4 * PHI_TEST_EMAX;
static_assert(PHI_TEST_PRE % 16 == 0, "PHI_TEST_PRE: whole 16-byte words");

struct PhiTestStageLayout {
  int live, r, a, s1;  // byte offsets, multiples of 16
  size_t bytes;
};

inline PhiTestStageLayout phi_test_stage_layout(int n_s) {
  PhiTestStageLayout L{};
  const auto up16 = [](size_t n) { return (n + 15) / 16 * 16; };
  L.live = (int)sizeof(TestStageHdr);
  L.r = L.live + 4 * PHI_TEST_EMAX;
  L.a = L.r + 4 * PHI_TEST_EMAX;
  L.s1 = L.a + 4 * PHI_TEST_EMAX;
  L.bytes = (size_t)L.s1 + up16(sizeof(float) * PHI_TEST_EMAX * (size_t)n_s);
  return L;
}

// Bookkeeping of one φ phase: TestPhaseHost's loop, with the action taken written into the record
// (the φ net reads it) and no φ row.  The exploration schedule is the SF agent's (draw_test_schedule:
// agents/sfdqn_phi.py:226-227 draws as agents/sfdqn.py does).
struct PhiTestPhaseHost {
  int E = 0, horizon = 0, n_s = 0;
  PhiTestStageLayout L{};
  uint8_t* st = nullptr;
  const int* explore = nullptr;  // [E * horizon]
  double* ret = nullptr;         // [E]
  long long* steps = nullptr;    // [E]
  long long* actions = nullptr;  // [E * horizon] or null
  std::vector<char> live, done;
  std::vector<float> phi_sink;   // [d]: where the env callback's φ goes

  int* live_w() const { return reinterpret_cast<int*>(st + L.live); }
  float* r_w() const { return reinterpret_cast<float*>(st + L.r); }
  int* a_w() const { return reinterpret_cast<int*>(st + L.a); }
  float* s1_row(int e) const { return reinterpret_cast<float*>(st + L.s1) + (size_t)e * n_s; }
  float* phi_row() { return phi_sink.data(); }

  void begin(int E_, int horizon_, int n_s_, int d_, uint8_t* staging, const int* explore_, double* ret_,
             long long* steps_, long long* actions_) {
    E = E_, horizon = horizon_, n_s = n_s_;
    L = phi_test_stage_layout(n_s);
    st = staging, explore = explore_, ret = ret_, steps = steps_, actions = actions_;
    live.assign(E, 1);
    done.assign(E, 0);
    phi_sink.assign(d_ > 0 ? d_ : 1, 0.f);
    for (int e = 0; e < PHI_TEST_EMAX; ++e) {
      live_w()[e] = e < E ? 1 : 0;  // the first record carries every row's s0
      r_w()[e] = 0.f;
      a_w()[e] = 0;
    }
    for (int e = 0; e < E; ++e) {
      ret[e] = 0.0;
      steps[e] = 0;
    }
    if (actions)
      for (size_t i = 0; i < (size_t)E * horizon; ++i) actions[i] = -1;
  }
  void header(long long seq, int step, int update) const {
    TestStageHdr hd{seq, step, update, 0.f, 0.f, 0, 0};
    std::memcpy(st, &hd, sizeof(hd));
  }
  bool is_live(int e) const { return live[e] != 0; }
  // the action row e takes at step j: the schedule's when it explores, else the published greedy one
  int action(int e, int j, long long greedy) const {
    const int x = explore[(size_t)e * horizon + j];
    return x >= 0 ? x : (int)greedy;
  }
  void took(int e, int j, int a, float r, int terminal) {
    if (actions) actions[(size_t)e * horizon + j] = a;
    ret[e] += (double)r;  // the callback's float32 reward, added in double
    steps[e] += 1;
    live_w()[e] = 1;
    r_w()[e] = r;
    a_w()[e] = a;
    done[e] = terminal ? 1 : 0;
  }
  void idle(int e) const { live_w()[e] = 0; }
  // rows whose callback reported done got this step's update and stop; returns the rows still running
  int end_step() {
    int n = 0;
    for (int e = 0; e < E; ++e) {
      if (done[e]) live[e] = 0;
      n += live[e] ? 1 : 0;
    }
    return n;
  }
};

}  // namespace sfx
