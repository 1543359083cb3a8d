// Host-only sanitizer run of the native test phase's host half (csrc/sfx_test_host.h): the exploration
// schedule's draws, the staging record's layout and writes, and the live-mask bookkeeping of E lockstep
// episodes -- the loop of test_phase_run (csrc/sfx_runner.inc) with the device replaced by a stand-in
// that reads the staging record the way k_test_intake does and "selects" an action per row.  No GPU,
// no HIP runtime: a CPU program with its own main.  Build and run from the repository root:
//   /opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -o tools/hostsan/test_phase_hostsan tools/hostsan/test_phase_hostsan.cpp
//   tools/hostsan/test_phase_hostsan
// Any heap / stack / UB finding aborts with the sanitizer's report; otherwise it prints "ok".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../deep-successor-features-for-transfer_amd/csrc/sfx_test_host.h"

using namespace sfx;

#define REQUIRE(c)                                                      \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

// what k_test_intake does with a record, on the host: every live row's s1 into the state block, one
// "update" counted per live row when the header asks for it, the loss slot [step][e] written
struct FakeDevice {
  int E, n_s, d, horizon;
  std::vector<float> S, loss;
  std::vector<int> updates;
  long long seq = 0;
  FakeDevice(int E_, int n_s_, int d_, int horizon_)
      : E(E_), n_s(n_s_), d(d_), horizon(horizon_), S((size_t)E_ * n_s_, 0.f), loss((size_t)E_ * horizon_, -1.f),
        updates(E_, 0) {}
  void intake(const uint8_t* st) {
    const TestStageLayout L = test_stage_layout(n_s, d);
    TestStageHdr hd;
    std::memcpy(&hd, st, sizeof(hd));
    const int* live = reinterpret_cast<const int*>(st + L.live);
    const float* r = reinterpret_cast<const float*>(st + L.r);
    const float* phi = reinterpret_cast<const float*>(st + L.phi);
    const float* s1 = reinterpret_cast<const float*>(st + L.s1);
    for (int e = 0; e < E; ++e) {
      if (!live[e]) continue;
      for (int k = 0; k < n_s; ++k) S[(size_t)e * n_s + k] = s1[(size_t)e * n_s + k];
      if (hd.update) {
        REQUIRE(hd.step >= 0 && hd.step < horizon);
        float y = 0.f;
        for (int k = 0; k < d; ++k) y += phi[(size_t)e * d + k];
        loss[(size_t)hd.step * E + e] = (y - r[e]) * (y - r[e]);
        updates[e] += 1;
      }
    }
    seq = hd.seq;
  }
  long long greedy(int e, int A) const {
    const long long v = (long long)(S[(size_t)e * n_s] * 1000.f);  // |s| of a few units: well inside the range
    return (v < 0 ? -v : v) % A;
  }
};

void run_case(int E, int horizon, int n_s, int d, int A, float eps, unsigned long long seed, bool with_ends) {
  std::mt19937_64 xr(test_stream_seed(seed, -1));
  std::vector<int> explore((size_t)E * horizon);
  draw_test_schedule(xr, E, horizon, eps, A, explore.data());
  int n_explore = 0;
  for (int x : explore) {
    REQUIRE(x >= -1 && x < A);
    n_explore += x >= 0;
  }
  if (eps == 0.f) REQUIRE(n_explore == 0);
  if (eps == 1.f) REQUIRE(n_explore == E * horizon);
  // the draws are task-major: the schedule of the first E - 1 tasks is a prefix of E tasks' schedule
  if (E > 1) {
    std::mt19937_64 xr2(test_stream_seed(seed, -1));
    std::vector<int> fewer((size_t)(E - 1) * horizon);
    draw_test_schedule(xr2, E - 1, horizon, eps, A, fewer.data());
    for (size_t i = 0; i < fewer.size(); ++i) REQUIRE(fewer[i] == explore[i]);
  }

  const TestStageLayout L = test_stage_layout(n_s, d);
  REQUIRE(L.live % 16 == 0 && L.r % 16 == 0 && L.phi % 16 == 0 && L.s1 % 16 == 0 && L.bytes % 16 == 0);
  std::vector<uint8_t> staging(L.bytes);  // exactly the record: a write past it is a heap overflow
  std::vector<std::mt19937_64> env;
  for (int e = 0; e < E; ++e) env.emplace_back(test_stream_seed(seed, e));
  std::vector<double> ret(E);
  std::vector<long long> steps(E), actions((size_t)E * horizon);
  std::vector<int> end_at(E, -1);
  if (with_ends)
    for (int e = 0; e < E; e += 2) end_at[e] = (e * 3) % horizon;
  FakeDevice dev(E, n_s, d, horizon);
  TestPhaseHost P;
  P.begin(E, horizon, n_s, d, staging.data(), explore.data(), ret.data(), steps.data(), actions.data());
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
  long long seq = 0;
  P.header(++seq, 0, 0, -0.005f, 0.01f);
  dev.intake(staging.data());
  int launches = 1;
  for (int j = 0; j < horizon; ++j) {
    REQUIRE(dev.seq == seq);
    for (int e = 0; e < E; ++e) {
      if (!P.is_live(e)) {
        P.idle(e);
        continue;
      }
      const int a = P.action(e, j, dev.greedy(e, A));
      REQUIRE(a >= 0 && a < A);
      for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
      for (int k = 0; k < d; ++k) P.phi_row(e)[k] = u01(env[e]);
      P.took(e, j, a, P.phi_row(e)[e % d], end_at[e] == j);
    }
    const bool last = P.end_step() == 0 || j + 1 == horizon;
    P.header(++seq, j, 1, -0.005f, 0.01f);
    dev.intake(staging.data());
    ++launches;
    if (last) break;
  }
  for (int e = 0; e < E; ++e) {
    const long long want = end_at[e] >= 0 ? end_at[e] + 1 : horizon;
    REQUIRE(steps[e] == want);
    REQUIRE(dev.updates[e] == want);  // the ending step's update ran, none after it
    for (int j = 0; j < horizon; ++j) {
      REQUIRE((actions[(size_t)e * horizon + j] >= 0) == (j < want));
      REQUIRE((dev.loss[(size_t)j * E + e] >= 0.f) == (j < want));
    }
  }
  REQUIRE(launches <= horizon + 1);
}

}  // namespace

int main() {
  // distinct streams per task and for the schedule
  REQUIRE(test_stream_seed(1, -1) != test_stream_seed(1, 0) && test_stream_seed(1, 0) != test_stream_seed(1, 1));
  REQUIRE(test_stream_seed(1, 0) != test_stream_seed(2, 0));
  const float epss[3] = {0.f, 0.03f, 1.f};
  for (float eps : epss)
    for (int ends = 0; ends < 2; ++ends) {
      run_case(1, 1, 1, 1, 2, eps, 3, ends != 0);
      run_case(5, 9, 6, 8, 9, eps, 5, ends != 0);
      run_case(17, 12, 6, 20, 9, eps, 7, ends != 0);
      run_case(TEST_EMAX, 7, 17, 8, 7, eps, 11, ends != 0);
      run_case(TEST_EMAX, 3, 3, 255, 3, eps, 13, ends != 0);
    }
  std::printf("ok\n");
  return 0;
}
