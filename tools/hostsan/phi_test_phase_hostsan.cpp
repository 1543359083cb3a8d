// Host-only sanitizer run of the learned-φ SF agent's test phase's host half (csrc/sfx_test_host.h): the
// exploration schedule's draws, the staging record's layout and writes, the live mask and the per-row bookkeeping
// of E lockstep episodes -- the loop of phi_test_phase_run (csrc/sfx_runner.inc) with the device replaced by a
// stand-in that reads the staging record the way k_phi_test_intake does and "chooses" the next greedy action per
// live row as k_phi_test_row does.  No GPU, no HIP runtime: a CPU program with its own main.  Build and run from
// the repository root:
//   /opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -o tools/hostsan/phi_test_phase_hostsan \
//     tools/hostsan/phi_test_phase_hostsan.cpp
//   tools/hostsan/phi_test_phase_hostsan
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

// what k_phi_test_intake and k_phi_test_row do with a record, on the host: the record is copied in 16-byte words
// (the header block and the E rows of s1, no byte past them); a live row's previous S1 row becomes its S row and
// the record's s1 its S1 row (the first record: S = S1 = s0, a = 0); when the header asks for an update, one
// "update" per live row; the next greedy action per live row
struct FakeDevice {
  int E, n_s, horizon, A;
  std::vector<float> S, S1, r;
  std::vector<long long> a;
  std::vector<int> updates, live;
  std::vector<long long> sel;  // [E][2]
  long long seq = 0;
  int step = -1;
  FakeDevice(int E_, int n_s_, int horizon_, int A_)
      : E(E_), n_s(n_s_), horizon(horizon_), A(A_), S((size_t)E_ * n_s_, -7.f), S1((size_t)E_ * n_s_, -7.f), r(E_, 0.f),
        a(E_, -1), updates(E_, 0), live(E_, 0), sel((size_t)2 * E_, -1) {}
  long long greedy(int e) const {
    const long long v = (long long)(S1[(size_t)e * n_s] * 1000.f);
    return (v < 0 ? -v : v) % A;
  }
  void launch(const uint8_t* st, size_t st_bytes) {
    const PhiTestStageLayout L = phi_test_stage_layout(n_s);
    REQUIRE(n_s <= PHI_TEST_NS && E <= PHI_TEST_EMAX);
    const size_t words = (size_t)PHI_TEST_PRE / 16 + ((size_t)E * n_s + 3) / 4;  // the intake's 16-byte loads
    REQUIRE(words * 16 <= st_bytes && words * 16 <= L.bytes);
    std::vector<uint8_t> lds(words * 16);
    std::memcpy(lds.data(), st, lds.size());
    TestStageHdr hd;
    std::memcpy(&hd, lds.data(), sizeof(hd));
    const int* lv = reinterpret_cast<const int*>(lds.data() + L.live);
    const float* rr = reinterpret_cast<const float*>(lds.data() + L.r);
    const int* aa = reinterpret_cast<const int*>(lds.data() + L.a);
    const float* s1 = reinterpret_cast<const float*>(lds.data() + L.s1);
    for (int e = E; e < PHI_TEST_EMAX; ++e) REQUIRE(lv[e] == 0);
    if (!hd.update)
      for (int e = 0; e < E; ++e) REQUIRE(lv[e] == 1);  // the first record carries every row
    for (int e = 0; e < E; ++e) {
      live[e] = lv[e];
      if (!lv[e]) continue;
      for (int k = 0; k < n_s; ++k) {
        const float v = s1[(size_t)e * n_s + k];
        S[(size_t)e * n_s + k] = hd.update ? S1[(size_t)e * n_s + k] : v;
        S1[(size_t)e * n_s + k] = v;
      }
      a[e] = hd.update ? aa[e] : 0;
      r[e] = rr[e];
      if (hd.update) {
        REQUIRE(hd.step >= 0 && hd.step < horizon);
        REQUIRE(aa[e] >= 0 && aa[e] < A);
        REQUIRE(rr[e] == s1[(size_t)e * n_s] * 0.5f);  // the env's r of this very transition
        updates[e] += 1;
      }
      for (int k = 0; k < n_s; ++k) REQUIRE(S[(size_t)e * n_s + k] != -7.f);  // the φ forward reads defined rows
      sel[2 * e] = 0;
      sel[2 * e + 1] = greedy(e);
    }
    seq = hd.seq;
    step = hd.step;
  }
};

// explore_given: the caller's schedule (every third step explores); otherwise the runner's draw
void run_case(int E, int horizon, int n_s, int d, int A, float eps, unsigned long long seed, bool with_ends,
              bool explore_given) {
  std::vector<int> explore((size_t)E * horizon);
  if (explore_given) {
    for (size_t i = 0; i < explore.size(); ++i) explore[i] = i % 3 == 0 ? (int)(i % (size_t)A) : -1;
  } else {
    std::mt19937_64 xr(test_stream_seed(seed, -1));
    draw_test_schedule(xr, E, horizon, eps, A, explore.data());
    int n_explore = 0;
    for (int x : explore) {
      REQUIRE(x >= -1 && x < A);
      n_explore += x >= 0;
    }
    if (eps == 0.f) REQUIRE(n_explore == 0);
    if (eps == 1.f) REQUIRE(n_explore == E * horizon);
  }

  const PhiTestStageLayout L = phi_test_stage_layout(n_s);
  for (int off : {L.live, L.r, L.a, L.s1}) REQUIRE(off % 16 == 0);
  REQUIRE(L.bytes % 16 == 0 && L.s1 == PHI_TEST_PRE);
  std::vector<uint8_t> staging(L.bytes);  // exactly the record: a write past it is a heap overflow
  std::vector<std::mt19937_64> env;
  for (int e = 0; e < E; ++e) env.emplace_back(test_stream_seed(seed, e));
  std::vector<double> ret(E);
  std::vector<long long> steps(E), actions((size_t)E * horizon);
  // rows that end at step 0, in the middle and at the last step
  std::vector<int> end_at(E, -1);
  if (with_ends) {
    end_at[0] = 0;
    if (E > 2) end_at[2] = horizon / 2;
    if (E > 4) end_at[4] = horizon - 1;
    if (E == PHI_TEST_EMAX) end_at[E - 1] = horizon / 3;
  }
  FakeDevice dev(E, n_s, horizon, A);
  PhiTestPhaseHost P;
  P.begin(E, horizon, n_s, d, staging.data(), explore.data(), ret.data(), steps.data(), actions.data());
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
  long long seq = 0;
  P.header(++seq, 0, 0);
  dev.launch(staging.data(), staging.size());
  int launches = 1;
  std::vector<double> want_ret(E, 0.0);
  for (int j = 0; j < horizon; ++j) {
    REQUIRE(dev.seq == seq);
    for (int e = 0; e < E; ++e) {
      if (!P.is_live(e)) {
        P.idle(e);
        continue;
      }
      REQUIRE(dev.live[e]);  // a row that steps was in the record before
      const int a = P.action(e, j, dev.sel[2 * e + 1]);
      REQUIRE(a >= 0 && a < A);
      for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
      for (int k = 0; k < d; ++k) P.phi_row()[k] = u01(env[e]);  // the callback's φ: into the sink
      const float r = P.s1_row(e)[0] * 0.5f;
      want_ret[e] += (double)r;
      P.took(e, j, a, r, end_at[e] == j);
    }
    const bool last = P.end_step() == 0 || j + 1 == horizon;
    P.header(++seq, j, 1);
    dev.launch(staging.data(), staging.size());  // the last record is launched like the others
    ++launches;
    REQUIRE(dev.step == j);
    if (last) break;
  }
  REQUIRE(dev.seq == seq);
  for (int e = 0; e < E; ++e) {
    const long long want = end_at[e] >= 0 ? end_at[e] + 1 : horizon;
    REQUIRE(steps[e] == want);
    REQUIRE(dev.updates[e] == want);  // the ending step's update ran, none after it
    REQUIRE(ret[e] == want_ret[e]);
    for (int j = 0; j < horizon; ++j) {
      const long long v = actions[(size_t)e * horizon + j];
      REQUIRE((v >= 0) == (j < want) && v < A);
      const int x = explore[(size_t)e * horizon + j];
      if (j < want && x >= 0) REQUIRE(v == x);
    }
    if (want > 0) REQUIRE(dev.a[e] == actions[(size_t)e * horizon + want - 1]);  // the widened action of its last step
  }
  REQUIRE(launches <= horizon + 1);
}

}  // namespace

int main() {
  const float epss[3] = {0.f, 0.3f, 1.f};
  for (float eps : epss)
    for (int ends = 0; ends < 2; ++ends)
      for (int given = 0; given < 2; ++given) {
        run_case(1, 1, 1, 1, 2, eps, 3, ends != 0, given != 0);
        run_case(1, 9, 11, 6, 5, eps, 4, ends != 0, given != 0);
        run_case(5, 9, 11, 6, 5, eps, 5, ends != 0, given != 0);
        run_case(9, 12, 6, 12, 9, eps, 7, ends != 0, given != 0);
        run_case(PHI_TEST_EMAX, 7, 31, 8, 7, eps, 11, ends != 0, given != 0);
        run_case(PHI_TEST_EMAX, 3, PHI_TEST_NS, 64, 3, eps, 13, ends != 0, given != 0);
      }
  std::printf("ok\n");
  return 0;
}
