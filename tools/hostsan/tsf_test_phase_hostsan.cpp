// Host-only sanitizer run of the TSF test phase's host half (csrc/sfx_test_host.h): the exploration schedule's
// draws, ω's learning-rate schedule, the staging record's layout and writes, and the per-row bookkeeping of E
// lockstep episodes with their own optimizer step counts -- the loop of tsf_test_phase_run (csrc/sfx_runner.inc)
// with the device replaced by a stand-in that reads the staging record the way k_tsf_test_intake does and
// "chooses" a1 and the next greedy action per live row.  No GPU, no HIP runtime: a CPU program with its own
// main.  Build and run from the repository root:
//   /opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -o tools/hostsan/tsf_test_phase_hostsan \
//     tools/hostsan/tsf_test_phase_hostsan.cpp
//   tools/hostsan/tsf_test_phase_hostsan
// Any heap / stack / UB finding aborts with the sanitizer's report; otherwise it prints "ok".
#include <cmath>
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

// what k_tsf_test_intake and k_tsf_test_row do with a record, on the host: a live row's previous S1 row becomes
// its S row and the record's s1 its S1 row; when the header asks for an update, one "update" per live row with
// the row's rowp checked against its own optimizer; a1 and the next greedy action per live row
struct FakeDevice {
  int E, n_s, d, horizon, A;
  std::vector<float> S, S1;
  std::vector<int> updates;
  std::vector<long long> sel;  // [E][2]
  std::vector<float> last_step, last_lr;
  long long seq = 0;
  FakeDevice(int E_, int n_s_, int d_, int horizon_, int A_)
      : E(E_), n_s(n_s_), d(d_), horizon(horizon_), A(A_), S((size_t)E_ * n_s_, 0.f), S1((size_t)E_ * n_s_, 0.f),
        updates(E_, 0), sel((size_t)2 * E_, -1), last_step(E_, 0.f), last_lr(E_, 0.f) {}
  long long greedy(int e) const {
    const long long v = (long long)(S1[(size_t)e * n_s] * 1000.f);
    return (v < 0 ? -v : v) % A;
  }
  void launch(const uint8_t* st) {
    const TsfTestStageLayout L = tsf_test_stage_layout(n_s, d);
    TestStageHdr hd;
    std::memcpy(&hd, st, sizeof(hd));
    const float* hp = reinterpret_cast<const float*>(st + L.hp);
    REQUIRE(hp[0] == 0.9f && hp[1] == 0.5f && hp[2] == 0.05f);
    const int* live = reinterpret_cast<const int*>(st + L.live);
    const float* r = reinterpret_cast<const float*>(st + L.r);
    const int* a = reinterpret_cast<const int*>(st + L.a);
    const int* a1x = reinterpret_cast<const int*>(st + L.a1x);
    const float* rowp = reinterpret_cast<const float*>(st + L.rowp);
    const float* phi = reinterpret_cast<const float*>(st + L.phi);
    const float* s1 = reinterpret_cast<const float*>(st + L.s1);
    for (int e = E; e < TEST_EMAX; ++e) REQUIRE(live[e] == 0);
    for (int e = 0; e < E; ++e) {
      if (!live[e]) continue;
      for (int k = 0; k < n_s; ++k) {
        S[(size_t)e * n_s + k] = S1[(size_t)e * n_s + k];
        S1[(size_t)e * n_s + k] = s1[(size_t)e * n_s + k];
      }
      if (hd.update) {
        REQUIRE(hd.step >= 0 && hd.step < horizon);
        REQUIRE(a[e] >= 0 && a[e] < A && a1x[e] >= -1 && a1x[e] < A);
        const float* p = rowp + (size_t)e * 6;
        REQUIRE(p[0] == r[e] && p[0] == phi[(size_t)e * d + e % d]);
        REQUIRE(p[5] == last_step[e] + 1.f || updates[e] == 0);  // consecutive Adam steps
        REQUIRE(p[3] <= last_lr[e] || updates[e] == 0);          // ω's lr decays
        last_step[e] = p[5];
        last_lr[e] = p[3];
        updates[e] += 1;
        sel[2 * e] = a1x[e] >= 0 ? a1x[e] : greedy(e);
      }
      sel[2 * e + 1] = greedy(e);
    }
    seq = hd.seq;
  }
};

void run_case(int E, int horizon, int n_s, int d, int A, float eps, unsigned long long seed, bool with_ends,
              long long opt0) {
  std::mt19937_64 xr(test_stream_seed(seed, -1));
  std::vector<int> explore((size_t)E * horizon * 2);
  draw_tsf_test_schedule(xr, E, horizon, eps, A, explore.data());
  int n_explore = 0;
  for (int x : explore) {
    REQUIRE(x >= -1 && x < A);
    n_explore += x >= 0;
  }
  if (eps == 0.f) REQUIRE(n_explore == 0);
  if (eps == 1.f) REQUIRE(n_explore == E * horizon * 2);
  // the draws are task-major, a then a1 per step: the SF schedule of 2 * horizon steps is the same stream
  {
    std::mt19937_64 xr2(test_stream_seed(seed, -1));
    std::vector<int> flat((size_t)E * horizon * 2);
    draw_test_schedule(xr2, E, 2 * horizon, eps, A, flat.data());
    REQUIRE(flat == explore);
  }

  const TsfTestStageLayout L = tsf_test_stage_layout(n_s, d);
  for (int off : {L.hp, L.live, L.r, L.a, L.a1x, L.rowp, L.phi, L.s1}) REQUIRE(off % 16 == 0);
  REQUIRE(L.bytes % 16 == 0 && L.phi == TSF_TEST_PRE);
  std::vector<uint8_t> staging(L.bytes);  // exactly the record: a write past it is a heap overflow
  std::vector<std::mt19937_64> env;
  for (int e = 0; e < E; ++e) env.emplace_back(test_stream_seed(seed, e));
  std::vector<double> ret(E);
  std::vector<long long> steps(E), actions((size_t)E * horizon * 2), opt(E);
  for (int e = 0; e < E; ++e) opt[e] = opt0 + e;
  std::vector<int> end_at(E, -1);
  if (with_ends)
    for (int e = 0; e < E; e += 2) end_at[e] = (e * 3) % horizon;
  FakeDevice dev(E, n_s, d, horizon, A);
  TsfTestRowHP hp;
  hp.lr_w = 2e-3f, hp.wd_w = 1e-3f, hp.wd_omega = 1e-4f, hp.lr_omega = 5e-3, hp.lr_omega_decay = 0.01;
  TsfTestPhaseHost P;
  P.begin(E, horizon, n_s, d, staging.data(), explore.data(), hp, 0.9f, 0.5f, 0.05f, opt.data(), ret.data(),
          steps.data(), actions.data());
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
  long long seq = 0;
  P.header(++seq, 0, 0);
  dev.launch(staging.data());
  int launches = 1, last_j = -1;
  const auto collect = [&](int j) {
    for (int e = 0; e < E; ++e)
      if (P.in_record(e)) P.took_a1(e, j, dev.sel[2 * e]);
  };
  for (int j = 0; j < horizon; ++j) {
    REQUIRE(dev.seq == seq);
    if (j > 0) collect(j - 1);
    for (int e = 0; e < E; ++e) {
      if (!P.is_live(e)) {
        P.idle(e);
        continue;
      }
      const int a = P.action(e, j, dev.sel[2 * e + 1]);
      REQUIRE(a >= 0 && a < A);
      for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
      for (int k = 0; k < d; ++k) P.phi_row(e)[k] = u01(env[e]);
      P.took(e, j, a, P.phi_row(e)[e % d], end_at[e] == j);
    }
    const bool last = P.end_step() == 0 || j + 1 == horizon;
    P.header(++seq, j, 1);
    dev.launch(staging.data());
    ++launches;
    last_j = j;
    if (last) break;
  }
  REQUIRE(dev.seq == seq);
  collect(last_j);
  for (int e = 0; e < E; ++e) {
    const long long want = end_at[e] >= 0 ? end_at[e] + 1 : horizon;
    REQUIRE(steps[e] == want);
    REQUIRE(dev.updates[e] == want);  // the ending step's update ran, none after it
    REQUIRE(opt[e] == opt0 + e + want);
    REQUIRE(dev.last_step[e] == (float)(opt0 + e + want));
    for (int j = 0; j < horizon; ++j)
      for (int c = 0; c < 2; ++c) {
        const long long v = actions[((size_t)e * horizon + j) * 2 + c];
        REQUIRE((v >= 0) == (j < want) && v < A);
        const int x = explore[((size_t)e * horizon + j) * 2 + c];
        if (j < want && x >= 0) REQUIRE(v == x);
      }
  }
  REQUIRE(launches <= horizon + 1);
}

}  // namespace

int main() {
  // ω's lr: LambdaLR over (1 - decay) ** epoch, narrowed to float
  REQUIRE(tsf_test_lr_omega(5e-3, 0.0, 1000) == 5e-3f);
  REQUIRE(tsf_test_lr_omega(5e-3, 0.01, 0) == 5e-3f);
  REQUIRE(tsf_test_lr_omega(5e-3, 0.01, 2) == (float)(5e-3 * std::pow(0.99, 2.0)));
  REQUIRE(tsf_test_lr_omega(5e-3, 0.5, 3000) == 0.f);
  const float epss[3] = {0.f, 0.03f, 1.f};
  for (float eps : epss)
    for (int ends = 0; ends < 2; ++ends) {
      run_case(1, 1, 1, 1, 2, eps, 3, ends != 0, 0);
      run_case(5, 9, 6, 8, 9, eps, 5, ends != 0, 37);
      run_case(17, 12, 6, 20, 9, eps, 7, ends != 0, 0);
      run_case(TEST_EMAX, 7, 17, 8, 7, eps, 11, ends != 0, (1LL << 24) - 7 - TEST_EMAX);
      run_case(TEST_EMAX, 3, 3, 255, 3, eps, 13, ends != 0, 5);
    }
  std::printf("ok\n");
  return 0;
}
