// sfx_test_host.h -- the host half of the native test phases (sfx_runner_test_phase, sfx_runner_tsf_test_phase,
// sfx_runner_phi_test_phase; sfx_runner.inc) that needs no device: the staging record's layout, the test-phase
// random streams, the exploration schedule and the per-row bookkeeping of E lockstep episodes
// (agents/sfdqn.py:139-166, agents/tsfdqn_sequential.py:392-433, agents/sfdqn_phi.py:234-261).  Plain C++, so
// tools/hostsan/lockstep_hostsan.cpp drives it under the host sanitizers without a GPU.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <random>
#include <vector>

namespace sfx {

constexpr int TEST_EMAX = 64;       // test tasks of one SF or TSF phase
constexpr int TEST_PHI_LDS = 8192;  // φ floats k_test_intake stages in LDS (larger E·d: read from the staging)
constexpr int PHI_TEST_EMAX = 16;   // test tasks of one φ phase: the E-row φ kernels' PHIE (sfx_phitest.h)
constexpr int PHI_TEST_NS = 32;     // n_s of a φ net's handle is at most 31 (2 n_s + 1 <= 64): k_phi_test_intake's LDS

// Staging record of one lockstep step (host-coherent, written by the host before each launch): the header,
// then the phase's columns of `emax` rows each, every column starting on a 16-byte word:
//   SF   TestStageHdr | live (int) | r | φ [emax][d] | s1 [emax][n_s]
//   TSF  TestStageHdr | hp[4] = γ, β, λ, 0 | live | r | a (int: the action taken at s) | a1x (int: the explored
//        a1, or -1 = greedy) | rowp [emax][6] (sfx_tsf_test_updates' layout: r, lr_w, wd_w, lr_ω, wd_ω, Adam
//        step) | φ | s1
//   φ    TestStageHdr | live | r | a | s1     (φ is computed on the device: the record carries none)
// live[e]: row e took the env step this record describes (the phase's first record: every row, its s0 in s1).
// Rows are d / n_s floats apart whatever E is, so the offsets hold for every phase of a handle.
struct TestStageHdr {
  long long seq;     // sequence number of this launch set (published back by k_test_publish)
  int step, update;  // lockstep step the transitions belong to; update 0: no mapper step (first record)
  float neg_lr, wd;  // SF: the SGD step's constants, narrowed as sfx_test_reward_updates narrows them; else 0
  int pad0_, pad1_;
};
static_assert(sizeof(TestStageHdr) == 32, "TestStageHdr: two 16-byte words");

struct TestStageLayout {
  int emax;                                // rows of every column
  int hp, live, r, a, a1x, rowp, phi, s1;  // byte offsets, multiples of 16; -1: the phase has no such column
  size_t bytes;
};

constexpr size_t up16(size_t n) { return (n + 15) / 16 * 16; }

namespace detail {
constexpr int stage_col(size_t& at, bool have, size_t bytes) {
  if (!have) return -1;
  const size_t off = at;
  at += up16(bytes);
  return (int)off;
}
constexpr TestStageLayout stage_layout(int emax, bool tsf, bool a, bool phi, int n_s, int d) {
  TestStageLayout L{};
  const size_t col = 4 * (size_t)emax;
  size_t at = sizeof(TestStageHdr);
  L.emax = emax;
  L.hp = stage_col(at, tsf, 16);
  L.live = stage_col(at, true, col);
  L.r = stage_col(at, true, col);
  L.a = stage_col(at, a, col);
  L.a1x = stage_col(at, tsf, col);
  L.rowp = stage_col(at, tsf, 6 * col);
  L.phi = stage_col(at, phi, col * (size_t)d);
  L.s1 = stage_col(at, true, col * (size_t)n_s);
  L.bytes = at;
  return L;
}
}  // namespace detail

constexpr TestStageLayout test_stage_layout(int n_s, int d) {
  return detail::stage_layout(TEST_EMAX, false, false, true, n_s, d);
}
constexpr TestStageLayout tsf_test_stage_layout(int n_s, int d) {
  return detail::stage_layout(TEST_EMAX, true, true, true, n_s, d);
}
constexpr TestStageLayout phi_test_stage_layout(int n_s) {
  return detail::stage_layout(PHI_TEST_EMAX, false, true, false, n_s, 0);
}

// what the intake kernels copy in front of φ (TSF) / s1 (φ phase), whatever the shape is
constexpr int TSF_TEST_PRE = (int)sizeof(TestStageHdr) + 16 + 4 * 4 * TEST_EMAX + 4 * 6 * TEST_EMAX;
constexpr int PHI_TEST_PRE = (int)sizeof(TestStageHdr) + 3 * 4 * PHI_TEST_EMAX;

// The kernels of sfx_testphase.h read the record at these bytes: an edit that moves one fails here.
namespace detail {
constexpr bool same_cols(const TestStageLayout& L, int hp, int live, int r, int a, int a1x, int rowp, int phi, int s1) {
  return L.hp == hp && L.live == live && L.r == r && L.a == a && L.a1x == a1x && L.rowp == rowp && L.phi == phi &&
         L.s1 == s1;
}
}  // namespace detail
static_assert(detail::same_cols(test_stage_layout(3, 5), -1, 32, 288, -1, -1, -1, 544, 544 + 1280), "SF record");
static_assert(test_stage_layout(3, 5).bytes == 544 + 1280 + 768 && test_stage_layout(3, 5).emax == 64, "SF record");
static_assert(detail::same_cols(tsf_test_stage_layout(3, 5), 32, 48, 304, 560, 816, 1072, 2608, 2608 + 1280), "TSF");
static_assert(tsf_test_stage_layout(3, 5).bytes == 2608 + 1280 + 768 && tsf_test_stage_layout(3, 5).emax == 64, "TSF");
static_assert(detail::same_cols(phi_test_stage_layout(3), -1, 32, 96, 160, -1, -1, -1, 224), "φ record");
static_assert(phi_test_stage_layout(3).bytes == 224 + 192 && phi_test_stage_layout(3).emax == 16, "φ record");
static_assert(TSF_TEST_PRE == 2608 && PHI_TEST_PRE == 224, "the intakes' fixed blocks");

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
// (SFDQN.get_test_action, agents/sfdqn.py:125-137; agents/sfdqn_phi.py:226-227 draws alike): task-major, per
// step one uniform and, when it is <= epsilon, one randrange(n_actions).  out[e * horizon + j] = the explored
// action, or -1 (greedy).
template <class Rng>
inline void draw_test_schedule(Rng& g, int E, int horizon, float epsilon, int n_actions, int* out) {
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  std::uniform_int_distribution<int> ua(0, n_actions - 1);
  for (int e = 0; e < E; ++e)
    for (int j = 0; j < horizon; ++j) out[(size_t)e * horizon + j] = u01(g) <= epsilon ? ua(g) : -1;
}

// The TSF agent's (get_test_action at s, then at s1: agents/tsfdqn_sequential.py:377-381, :404-407): the same
// draws, two per step.  out[(e * horizon + j) * 2 + {0, 1}] = the explored a / a1, or -1 (greedy).
template <class Rng>
inline void draw_tsf_test_schedule(Rng& g, int E, int horizon, float epsilon, int n_actions, int* out) {
  draw_test_schedule(g, E, 2 * horizon, epsilon, n_actions, out);
}

// lr of ω's parameter group at scheduler epoch `epoch`: LambdaLR over (1 - decay) ** epoch
// (agents/tsfdqn_sequential.py:344-348), narrowed as the row's float32 rowp entry is.
inline float tsf_test_lr_omega(double lr_omega, double decay, long long epoch) {
  return (float)(lr_omega * std::pow(1.0 - decay, (double)epoch));
}

// hyperparameters of a TSF phase as the rows' rowp entries carry them
struct TsfTestRowHP {
  float lr_w = 0.f, wd_w = 0.f, wd_omega = 0.f;
  double lr_omega = 0.0, lr_omega_decay = 0.0;
};

// Bookkeeping of one phase: which rows still run, their returns / step counts / actions, and the writes into the
// staging record; a column the layout lacks is not written.  Per lockstep step j the loop calls, for every row,
// either took() (a live row's transition, written by the env callback into s1_row / phi_row) or idle(), then
// header() and, after the launch, end_step().  `draws`: schedule entries per step (1; TSF 2: a, then a1).
struct TestPhaseHost {
  int E = 0, horizon = 0, n_s = 0, d = 0, draws = 1;
  TestStageLayout L{};
  uint8_t* st = nullptr;
  const int* explore = nullptr;    // [E * horizon * draws]
  double* ret = nullptr;           // [E]
  long long* steps = nullptr;      // [E]
  long long* actions = nullptr;    // [E * horizon * draws] or null
  long long* opt_steps = nullptr;  // TSF: [E] in/out
  TsfTestRowHP hp;                 // TSF
  std::vector<char> live, done;
  std::vector<float> phi_sink;  // [d]: where the env callback's φ goes when the record carries none

  int* live_w() const { return reinterpret_cast<int*>(st + L.live); }
  float* r_w() const { return reinterpret_cast<float*>(st + L.r); }
  int* a_w() const { return reinterpret_cast<int*>(st + L.a); }
  int* a1x_w() const { return reinterpret_cast<int*>(st + L.a1x); }
  float* rowp_row(int e) const { return reinterpret_cast<float*>(st + L.rowp) + (size_t)e * 6; }
  float* phi_row(int e) { return L.phi < 0 ? phi_sink.data() : reinterpret_cast<float*>(st + L.phi) + (size_t)e * d; }
  float* s1_row(int e) const { return reinterpret_cast<float*>(st + L.s1) + (size_t)e * n_s; }
  size_t at(int e, int j) const { return ((size_t)e * horizon + j) * draws; }

  void begin(const TestStageLayout& L_, int draws_, int E_, int horizon_, int n_s_, int d_, uint8_t* staging,
             const int* explore_, double* ret_, long long* steps_, long long* actions_) {
    E = E_, horizon = horizon_, n_s = n_s_, d = d_, draws = draws_;
    L = L_;
    st = staging, explore = explore_, ret = ret_, steps = steps_, actions = actions_;
    live.assign(E, 1);
    done.assign(E, 0);
    phi_sink.assign(L.phi < 0 ? (d > 0 ? d : 1) : 0, 0.f);
    for (int e = 0; e < L.emax; ++e) {
      live_w()[e] = e < E ? 1 : 0;  // the first record carries every row's s0
      r_w()[e] = 0.f;
      if (L.a >= 0) a_w()[e] = 0;
      if (L.a1x >= 0) a1x_w()[e] = -1;
      if (L.rowp >= 0)
        for (int k = 0; k < 6; ++k) rowp_row(e)[k] = k == 5 ? 1.f : 0.f;
    }
    for (int e = 0; e < E; ++e) {
      ret[e] = 0.0;
      steps[e] = 0;
    }
    if (actions)
      for (size_t i = 0; i < (size_t)E * horizon * draws; ++i) actions[i] = -1;
  }
  // TSF, after begin(): the record's hp column and what took() needs for a row's rowp
  void begin_tsf(const TsfTestRowHP& hp_, float gamma, float beta, float lasso, long long* opt_steps_) {
    hp = hp_;
    opt_steps = opt_steps_;
    const float g[4] = {gamma, beta, lasso, 0.f};
    std::memcpy(st + L.hp, g, sizeof(g));
  }
  void header(long long seq, int step, int update, float neg_lr = 0.f, float wd = 0.f) const {
    TestStageHdr hd{seq, step, update, neg_lr, wd, 0, 0};
    std::memcpy(st, &hd, sizeof(hd));
  }
  bool is_live(int e) const { return live[e] != 0; }
  // TSF: row e took the env step the staged record describes (its a1 is published by that record's launch)
  bool in_record(int e) const { return live_w()[e] != 0; }
  // the action row e takes at step j: the schedule's when it explores, else the published greedy one
  int action(int e, int j, long long greedy) const {
    const int x = explore[at(e, j)];
    return x >= 0 ? x : (int)greedy;
  }
  void took(int e, int j, int a, float r, int terminal) {
    if (actions) actions[at(e, j)] = a;
    ret[e] += (double)r;  // the callback's float32 reward, added in double
    steps[e] += 1;
    live_w()[e] = 1;
    r_w()[e] = r;
    if (L.a >= 0) a_w()[e] = a;
    if (L.a1x >= 0) a1x_w()[e] = explore[at(e, j) + 1];
    if (L.rowp >= 0) {
      float* p = rowp_row(e);
      p[0] = r;
      p[1] = hp.lr_w;
      p[2] = hp.wd_w;
      p[3] = tsf_test_lr_omega(hp.lr_omega, hp.lr_omega_decay, opt_steps[e]);
      p[4] = hp.wd_omega;
      p[5] = (float)(opt_steps[e] + 1);  // exact: the entry point bounds it by 2^24
      opt_steps[e] += 1;                 // optim.step() and scheduler.step()
    }
    done[e] = terminal ? 1 : 0;
  }
  // TSF: the a1 the device chose for row e at step j, once that step's launch has published
  void took_a1(int e, int j, long long a1) const {
    if (actions) actions[at(e, j) + 1] = a1;
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

}  // namespace sfx
