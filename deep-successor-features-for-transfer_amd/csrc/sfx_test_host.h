// sfx_test_host.h -- the host half of the native test phase (sfx_runner_test_phase, sfx_runner.inc)
// that needs no device: the staging record's layout, the test-phase random streams, the exploration
// schedule and the per-row bookkeeping of E lockstep episodes (agents/sfdqn.py:139-166).  Plain C++,
// so tools/hostsan/test_phase_hostsan.cpp drives it under the host sanitizers without a GPU.
#pragma once
#include <stdint.h>

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

}  // namespace sfx
