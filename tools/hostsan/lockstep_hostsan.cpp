// Host-only sanitizer run of the native test phases' host half (csrc/sfx_test_host.h): the exploration schedule's
// draws, ω's learning-rate schedule, the three staging records' layouts and writes, and the per-row bookkeeping of
// E lockstep episodes -- the loop of lockstep_phase_run (csrc/sfx_runner.inc) with the device replaced by one
// stand-in per kind of phase, which reads the staging record the way that kind's intake kernel does and "selects"
// per live row.  No GPU, no HIP runtime: a CPU program with its own main.  Build and run from the repository root:
//   /opt/rocm/bin/hipcc -x c++ -O1 -g -std=c++17 -fno-omit-frame-pointer -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -o tools/hostsan/lockstep_hostsan tools/hostsan/lockstep_hostsan.cpp
//   tools/hostsan/lockstep_hostsan
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

enum Kind { SF, TSF, PHI };

long long greedy_of(const std::vector<float>& S, int e, int n_s, int A) {
  const long long v = (long long)(S[(size_t)e * n_s] * 1000.f);  // |s| of a few units: well inside the range
  return (v < 0 ? -v : v) % A;
}

// The three stand-ins share their shape; sel [E][2] is what k_test_publish would post (a1 / c, the next greedy a).
struct FakeDevice {
  int E, n_s, d, horizon, A;
  std::vector<float> S, S1;
  std::vector<int> updates;
  std::vector<long long> sel;
  long long seq = 0;
  FakeDevice(int E_, int n_s_, int d_, int horizon_, int A_, float fill)
      : E(E_), n_s(n_s_), d(d_), horizon(horizon_), A(A_), S((size_t)E_ * n_s_, fill), S1((size_t)E_ * n_s_, fill),
        updates(E_, 0), sel((size_t)2 * E_, -1) {}
};

// what k_test_intake does with a record, on the host: every live row's s1 into the state block, one "update"
// counted per live row when the header asks for it, the loss slot [step][e] written
struct SfDevice : FakeDevice {
  std::vector<float> loss;
  SfDevice(int E_, int n_s_, int d_, int horizon_, int A_)
      : FakeDevice(E_, n_s_, d_, horizon_, A_, 0.f), loss((size_t)E_ * horizon_, -1.f) {}
  void launch(const uint8_t* st) {
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
      sel[2 * e + 1] = greedy_of(S, e, n_s, A);
    }
    seq = hd.seq;
  }
};

// what k_tsf_test_intake and k_tsf_test_row do with a record, on the host: a live row's previous S1 row becomes
// its S row and the record's s1 its S1 row; when the header asks for an update, one "update" per live row with
// the row's rowp checked against its own optimizer; a1 and the next greedy action per live row
struct TsfDevice : FakeDevice {
  std::vector<float> last_step, last_lr;
  TsfDevice(int E_, int n_s_, int d_, int horizon_, int A_)
      : FakeDevice(E_, n_s_, d_, horizon_, A_, 0.f), last_step(E_, 0.f), last_lr(E_, 0.f) {}
  void launch(const uint8_t* st) {
    const TestStageLayout L = tsf_test_stage_layout(n_s, d);
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
        sel[2 * e] = a1x[e] >= 0 ? a1x[e] : greedy_of(S1, e, n_s, A);
      }
      sel[2 * e + 1] = greedy_of(S1, e, n_s, A);
    }
    seq = hd.seq;
  }
};

// what k_phi_test_intake and k_phi_test_row do with a record, on the host: the record is copied in 16-byte words
// (the header block and the E rows of s1, no byte past them); a live row's previous S1 row becomes its S row and
// the record's s1 its S1 row (the first record: S = S1 = s0, a = 0); when the header asks for an update, one
// "update" per live row; the next greedy action per live row
struct PhiDevice : FakeDevice {
  std::vector<float> r;
  std::vector<long long> a;
  std::vector<int> live;
  int step = -1;
  PhiDevice(int E_, int n_s_, int d_, int horizon_, int A_)
      : FakeDevice(E_, n_s_, d_, horizon_, A_, -7.f), r(E_, 0.f), a(E_, -1), live(E_, 0) {}
  void launch(const uint8_t* st, size_t st_bytes) {
    const TestStageLayout L = phi_test_stage_layout(n_s);
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
      sel[2 * e + 1] = greedy_of(S1, e, n_s, A);
    }
    seq = hd.seq;
    step = hd.step;
  }
};

// The literal offsets the kernels read at (the header's static_asserts at one shape; here at every case's).
void check_layout(Kind kind, const TestStageLayout& L, int n_s, int d) {
  const int rows = (int)up16(4 * 64 * (size_t)d);
  for (int off : {L.hp, L.live, L.r, L.a, L.a1x, L.rowp, L.phi, L.s1}) REQUIRE(off == -1 || off % 16 == 0);
  REQUIRE(L.bytes % 16 == 0);
  if (kind == SF) {
    REQUIRE(L.emax == TEST_EMAX && L.live == 32 && L.r == 288 && L.phi == 544 && L.s1 == 544 + rows);
    REQUIRE(L.hp == -1 && L.a == -1 && L.a1x == -1 && L.rowp == -1);
  } else if (kind == TSF) {
    REQUIRE(L.emax == TEST_EMAX && L.hp == 32 && L.live == 48 && L.r == 304 && L.a == 560 && L.a1x == 816);
    REQUIRE(L.rowp == 1072 && L.phi == 2608 && L.phi == TSF_TEST_PRE && L.s1 == 2608 + rows);
  } else {
    REQUIRE(L.emax == PHI_TEST_EMAX && L.live == 32 && L.r == 96 && L.a == 160 && L.s1 == 224 && L.s1 == PHI_TEST_PRE);
    REQUIRE(L.hp == -1 && L.a1x == -1 && L.rowp == -1 && L.phi == -1);
  }
  REQUIRE(L.bytes == (size_t)L.s1 + up16(4 * (size_t)L.emax * n_s));
}

// explore_given: the caller's schedule (every third entry explores); otherwise the runner's draw.  opt0: TSF, the
// first row's optimizer step count.
void run_case(Kind kind, int E, int horizon, int n_s, int d, int A, float eps, unsigned long long seed, bool with_ends,
              long long opt0 = 0, bool explore_given = false) {
  const int draws = kind == TSF ? 2 : 1;
  std::vector<int> explore((size_t)E * horizon * draws);
  if (explore_given) {
    for (size_t i = 0; i < explore.size(); ++i) explore[i] = i % 3 == 0 ? (int)(i % (size_t)A) : -1;
  } else {
    std::mt19937_64 xr(test_stream_seed(seed, -1));
    if (kind == TSF)
      draw_tsf_test_schedule(xr, E, horizon, eps, A, explore.data());
    else
      draw_test_schedule(xr, E, horizon, eps, A, explore.data());
    int n_explore = 0;
    for (int x : explore) {
      REQUIRE(x >= -1 && x < A);
      n_explore += x >= 0;
    }
    if (eps == 0.f) REQUIRE(n_explore == 0);
    if (eps == 1.f) REQUIRE(n_explore == E * horizon * draws);
    std::mt19937_64 xr2(test_stream_seed(seed, -1));
    if (kind == TSF) {  // task-major, a then a1 per step: the SF schedule of 2 * horizon steps is the same stream
      std::vector<int> flat(explore.size());
      draw_test_schedule(xr2, E, 2 * horizon, eps, A, flat.data());
      REQUIRE(flat == explore);
    } else if (E > 1) {  // task-major: the schedule of the first E - 1 tasks is a prefix of E tasks' schedule
      std::vector<int> fewer((size_t)(E - 1) * horizon);
      draw_test_schedule(xr2, E - 1, horizon, eps, A, fewer.data());
      for (size_t i = 0; i < fewer.size(); ++i) REQUIRE(fewer[i] == explore[i]);
    }
  }

  const TestStageLayout L = kind == SF    ? test_stage_layout(n_s, d)
                            : kind == TSF ? tsf_test_stage_layout(n_s, d)
                                          : phi_test_stage_layout(n_s);
  check_layout(kind, L, n_s, d);
  std::vector<uint8_t> staging(L.bytes);  // exactly the record: a write past it is a heap overflow
  std::vector<std::mt19937_64> env;
  for (int e = 0; e < E; ++e) env.emplace_back(test_stream_seed(seed, e));
  std::vector<double> ret(E), want_ret(E, 0.0);
  std::vector<long long> steps(E), actions((size_t)E * horizon * draws), opt(E);
  for (int e = 0; e < E; ++e) opt[e] = opt0 + e;
  std::vector<int> end_at(E, -1);
  if (with_ends && kind == PHI) {  // rows that end at step 0, in the middle and at the last step
    end_at[0] = 0;
    if (E > 2) end_at[2] = horizon / 2;
    if (E > 4) end_at[4] = horizon - 1;
    if (E == PHI_TEST_EMAX) end_at[E - 1] = horizon / 3;
  } else if (with_ends) {
    for (int e = 0; e < E; e += 2) end_at[e] = (e * 3) % horizon;
  }
  SfDevice sf(E, n_s, d, horizon, A);
  TsfDevice tsf(E, n_s, d, horizon, A);
  PhiDevice phi(E, n_s, d, horizon, A);
  FakeDevice& dev = kind == SF ? (FakeDevice&)sf : kind == TSF ? (FakeDevice&)tsf : (FakeDevice&)phi;
  const float neg_lr = kind == SF ? -0.005f : 0.f, wd = kind == SF ? 0.01f : 0.f;
  int launches = 0;
  const auto launch = [&]() {
    if (kind == SF) sf.launch(staging.data());
    if (kind == TSF) tsf.launch(staging.data());
    if (kind == PHI) phi.launch(staging.data(), staging.size());
    ++launches;
  };
  TestPhaseHost P;
  P.begin(L, draws, E, horizon, n_s, d, staging.data(), explore.data(), ret.data(), steps.data(), actions.data());
  if (kind == TSF) {
    TsfTestRowHP hp;
    hp.lr_w = 2e-3f, hp.wd_w = 1e-3f, hp.wd_omega = 1e-4f, hp.lr_omega = 5e-3, hp.lr_omega_decay = 0.01;
    P.begin_tsf(hp, 0.9f, 0.5f, 0.05f, opt.data());
  }
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u01(0.f, 1.f);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
  long long seq = 0;
  P.header(++seq, 0, 0, neg_lr, wd);
  launch();
  int last_j = -1;
  const auto collect = [&](int j) {
    for (int e = 0; e < E; ++e)
      if (P.in_record(e)) P.took_a1(e, j, dev.sel[2 * e]);
  };
  for (int j = 0; j < horizon; ++j) {
    REQUIRE(dev.seq == seq);
    if (kind == TSF && j > 0) collect(j - 1);
    for (int e = 0; e < E; ++e) {
      if (!P.is_live(e)) {
        P.idle(e);
        continue;
      }
      if (kind == PHI) REQUIRE(phi.live[e]);  // a row that steps was in the record before
      const int a = P.action(e, j, dev.sel[2 * e + 1]);
      REQUIRE(a >= 0 && a < A);
      for (int k = 0; k < n_s; ++k) P.s1_row(e)[k] = nd(env[e]);
      for (int k = 0; k < d; ++k) P.phi_row(e)[k] = u01(env[e]);  // no φ column: the callback's φ goes to the sink
      const float r = kind == PHI ? P.s1_row(e)[0] * 0.5f : P.phi_row(e)[e % d];
      want_ret[e] += (double)r;
      P.took(e, j, a, r, end_at[e] == j);
    }
    const bool last = P.end_step() == 0 || j + 1 == horizon;
    P.header(++seq, j, 1, neg_lr, wd);
    launch();  // the last record is launched like the others (the SF phase's: its intake, which is all this one is)
    if (kind == PHI) REQUIRE(phi.step == j);
    last_j = j;
    if (last) break;
  }
  REQUIRE(dev.seq == seq);
  if (kind == TSF) collect(last_j);
  for (int e = 0; e < E; ++e) {
    const long long want = end_at[e] >= 0 ? end_at[e] + 1 : horizon;
    REQUIRE(steps[e] == want);
    REQUIRE(dev.updates[e] == want);  // the ending step's update ran, none after it
    REQUIRE(ret[e] == want_ret[e]);
    if (kind == TSF) {
      REQUIRE(opt[e] == opt0 + e + want);
      REQUIRE(tsf.last_step[e] == (float)(opt0 + e + want));
    }
    for (int j = 0; j < horizon; ++j) {
      for (int c = 0; c < draws; ++c) {
        const long long v = actions[((size_t)e * horizon + j) * draws + c];
        REQUIRE((v >= 0) == (j < want) && v < A);
        const int x = explore[((size_t)e * horizon + j) * draws + c];
        if (j < want && x >= 0) REQUIRE(v == x);
      }
      if (kind == SF) REQUIRE((sf.loss[(size_t)j * E + e] >= 0.f) == (j < want));
    }
    // the widened action of its last step
    if (kind == PHI && want > 0) REQUIRE(phi.a[e] == actions[(size_t)e * horizon + want - 1]);
  }
  REQUIRE(launches <= horizon + 1);
}

}  // namespace

int main() {
  // distinct streams per task and for the schedule
  REQUIRE(test_stream_seed(1, -1) != test_stream_seed(1, 0) && test_stream_seed(1, 0) != test_stream_seed(1, 1));
  REQUIRE(test_stream_seed(1, 0) != test_stream_seed(2, 0));
  // ω's lr: LambdaLR over (1 - decay) ** epoch, narrowed to float
  REQUIRE(tsf_test_lr_omega(5e-3, 0.0, 1000) == 5e-3f);
  REQUIRE(tsf_test_lr_omega(5e-3, 0.01, 0) == 5e-3f);
  REQUIRE(tsf_test_lr_omega(5e-3, 0.01, 2) == (float)(5e-3 * std::pow(0.99, 2.0)));
  REQUIRE(tsf_test_lr_omega(5e-3, 0.5, 3000) == 0.f);
  for (float eps : {0.f, 0.03f, 1.f})
    for (int ends = 0; ends < 2; ++ends)
      for (Kind kind : {SF, TSF}) {
        const bool tsf = kind == TSF;
        run_case(kind, 1, 1, 1, 1, 2, eps, 3, ends != 0, 0);
        run_case(kind, 5, 9, 6, 8, 9, eps, 5, ends != 0, tsf ? 37 : 0);
        run_case(kind, 17, 12, 6, 20, 9, eps, 7, ends != 0, 0);
        run_case(kind, TEST_EMAX, 7, 17, 8, 7, eps, 11, ends != 0, tsf ? (1LL << 24) - 7 - TEST_EMAX : 0);
        run_case(kind, TEST_EMAX, 3, 3, 255, 3, eps, 13, ends != 0, tsf ? 5 : 0);
      }
  for (float eps : {0.f, 0.3f, 1.f})
    for (int ends = 0; ends < 2; ++ends)
      for (int given = 0; given < 2; ++given) {
        run_case(PHI, 1, 1, 1, 1, 2, eps, 3, ends != 0, 0, given != 0);
        run_case(PHI, 1, 9, 11, 6, 5, eps, 4, ends != 0, 0, given != 0);
        run_case(PHI, 5, 9, 11, 6, 5, eps, 5, ends != 0, 0, given != 0);
        run_case(PHI, 9, 12, 6, 12, 9, eps, 7, ends != 0, 0, given != 0);
        run_case(PHI, PHI_TEST_EMAX, 7, 31, 8, 7, eps, 11, ends != 0, 0, given != 0);
        run_case(PHI, PHI_TEST_EMAX, 3, PHI_TEST_NS, 64, 3, eps, 13, ends != 0, 0, given != 0);
      }
  std::printf("ok\n");
  return 0;
}
