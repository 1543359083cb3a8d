// sfx_testphase.h -- device code of the native test phase (sfx_runner_test_phase, sfx_runner.inc).
// Included after every other kernel header, so the code object's layout in front of it is unchanged.
#pragma once
#include "sfx_kernels.h"
#include "sfx_test_host.h"

namespace sfx {

// -------------------------------------------------------------------------------------
// Native test phase (sfx_runner_test_phase): E test episodes of agents/sfdqn.py:139-166 in
// lockstep.  One lockstep step is intake -> ψ forward of the E rows -> k_gpi with per-row W ->
// k_test_publish.  Nothing here waits for the host: the launch set is issued after the host has
// written the staging record, and the host waits (bounded) for the published sequence word.
// The staging record (TestStageHdr | live | r | φ | s1) is laid out in sfx_test_host.h.
// -------------------------------------------------------------------------------------
constexpr int TEST_PRE16 = (int)((sizeof(TestStageHdr) + 8 * TEST_EMAX) / 16);  // header + live + r, 16-byte words

struct TestIntakeArgs {
  const unsigned char* stage;  // host-coherent staging record
  int off_phi, off_s1;         // byte offsets of φ and s1 in it (multiples of 16)
  int E, d, n_s, w_stride, horizon, pad_;
  float* W;            // [E] rows w_stride floats apart, updated in place
  float* S;            // device state block [E][n_s]
  float* loss;         // device [horizon][E]
  long long* dseq;     // device: the header's seq, for k_test_publish
};

// (a) of a lockstep step: s1 of every live row into the device state block, the reward-mapper step
// of SFDQN.update_test_reward_mapper on its W row (sf_test_mapper_row: k_sf_test_mapper's
// arithmetic), the pre-step loss into loss[step][e].  One workgroup; lane e owns row e's W.
__global__ __launch_bounds__(256) void k_test_intake(TestIntakeArgs A) {
  __shared__ __attribute__((aligned(16))) uint4 s_pre[TEST_PRE16];
  __shared__ __attribute__((aligned(16))) float s_phi[TEST_PHI_LDS];
  const int tid = threadIdx.x;
  const uint4* src = reinterpret_cast<const uint4*>(A.stage);
  if (tid < TEST_PRE16) s_pre[tid] = src[tid];
  const int nphi = A.E * A.d;
  const bool phi_lds = nphi <= TEST_PHI_LDS;
  const float* gphi = reinterpret_cast<const float*>(A.stage + A.off_phi);
  if (phi_lds) {
    const uint4* p16 = reinterpret_cast<const uint4*>(gphi);
    uint4* l16 = reinterpret_cast<uint4*>(s_phi);
    for (int i = tid; i < (nphi + 3) / 4; i += 256) l16[i] = p16[i];
  }
  __syncthreads();
  const TestStageHdr& H = *reinterpret_cast<const TestStageHdr*>(s_pre);
  const int* live = reinterpret_cast<const int*>(s_pre) + sizeof(TestStageHdr) / 4;
  const float* r = reinterpret_cast<const float*>(live + TEST_EMAX);
  const float* gs1 = reinterpret_cast<const float*>(A.stage + A.off_s1);
  const FDiv fn = fdiv(A.n_s);
  for (int i = tid; i < A.E * A.n_s; i += 256) {
    const int e = i / fn;
    if (live[e]) A.S[i] = gs1[i];
  }
  if (tid < A.E && H.update && live[tid] && H.step >= 0 && H.step < A.horizon) {
    const float* f = (phi_lds ? s_phi : gphi) + (size_t)tid * A.d;
    A.loss[(size_t)H.step * A.E + tid] =
        sf_test_mapper_row(A.d, f, r[tid], A.W + (long long)tid * A.w_stride, H.neg_lr, H.wd);
  }
  if (tid == 0) __hip_atomic_store(A.dseq, H.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (c)'s tail: the E selections (c_e, a_e) k_gpi left in sel [E][2] to host-coherent memory, the
// sequence word last (system release), as publish_result posts a training step's.
struct TestResult {
  long long sel[2 * TEST_EMAX];
  long long seq, pad_;
};
__global__ __launch_bounds__(128) void k_test_publish(const int64_t* sel, int E, const long long* dseq, TestResult* out) {
  const int tid = threadIdx.x;
  if (tid < 2 * E) {
    const long long v = __hip_atomic_load(sel + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&out->sel[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  __threadfence_system();
  __syncthreads();
  if (tid == 0) {
    const long long seq = __hip_atomic_load(dseq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&out->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// -------------------------------------------------------------------------------------
// The TSF agent's test phase (sfx_runner_tsf_test_phase): E episodes of
// agents/tsfdqn_sequential.py:392-433 in lockstep.  One lockstep step is k_tsf_test_intake -> one ψ
// forward of the E rows (ψ(S), ψ(S1) online, ψ⁻(S1)) -> k_tsf_test_g -> k_tsf_test_row ->
// k_test_publish, a linear chain; the staging record is tsf_test_stage_layout's (sfx_test_host.h).
// -------------------------------------------------------------------------------------

// what the intake leaves on the device for the row kernel
struct TsfTestDevHdr {
  int step, update;
  float gamma, beta, lasso;
  int pad_[3];
};

// The phase's device block, one allocation: byte offsets of its parts (multiples of 16)
struct TsfTestDevLayout {
  int hdr, live, a, a1x, rowp, phi, S, S1;
  size_t bytes;
};
inline TsfTestDevLayout tsf_test_dev_layout(int n_s, int d) {
  TsfTestDevLayout L{};
  const auto up16 = [](size_t n) { return (n + 15) / 16 * 16; };
  L.hdr = 0;
  L.live = (int)sizeof(TsfTestDevHdr);
  L.a = L.live + 4 * TEST_EMAX;
  L.a1x = L.a + 8 * TEST_EMAX;
  L.rowp = L.a1x + 4 * TEST_EMAX;
  L.phi = L.rowp + 4 * 6 * TEST_EMAX;
  L.S = L.phi + (int)up16(sizeof(float) * TEST_EMAX * (size_t)d);
  L.S1 = L.S + (int)up16(sizeof(float) * TEST_EMAX * (size_t)n_s);
  L.bytes = (size_t)L.S1 + up16(sizeof(float) * TEST_EMAX * (size_t)n_s);
  return L;
}

struct TsfTestIntakeArgs {
  const unsigned char* stage;  // host-coherent staging record (tsf_test_stage_layout)
  int off_phi, off_s1;         // byte offsets of φ and s1 in it (multiples of 16)
  int E, d, n_s, horizon;
  TsfTestDevHdr* hdr;
  int* live;         // [E]
  int64_t* a;        // [E] the actions taken at s (k_tsf_test_step's type)
  int* a1x;          // [E] explored a1 or -1
  float* rowp;       // [E][6]
  float* phi;        // [E][d]
  float* S;          // [E][n_s]: a live row's previous S1 row
  float* S1;         // [E][n_s]: its new s1
  long long* dseq;   // device: the header's seq, for k_test_publish
};

// (a) of a TSF lockstep step, one workgroup: for every live row the previous S1 row becomes its S row
// and the record's s1 its S1 row; φ, a, the explored a1 and rowp go to the device block, the live
// mask and the header's step / update / (γ, β, λ) too, the header's seq to the device word.  A row
// that is not live keeps everything it had.
__global__ __launch_bounds__(256) void k_tsf_test_intake(TsfTestIntakeArgs A) {
  constexpr int PRE16 = TSF_TEST_PRE / 16;
  __shared__ __attribute__((aligned(16))) uint4 s_pre[PRE16];
  const int tid = threadIdx.x;
  SFX_CHK(A.E >= 1 && A.E <= TEST_EMAX, A.E, TEST_EMAX, 0);
  const uint4* src = reinterpret_cast<const uint4*>(A.stage);
  if (tid < PRE16) s_pre[tid] = src[tid];
  __syncthreads();
  const TestStageHdr& H = *reinterpret_cast<const TestStageHdr*>(s_pre);
  const float* hp = reinterpret_cast<const float*>(s_pre) + sizeof(TestStageHdr) / 4;
  const int* live = reinterpret_cast<const int*>(hp + 4);
  const int* a = live + 2 * TEST_EMAX;
  const int* a1x = a + TEST_EMAX;
  const float* rowp = reinterpret_cast<const float*>(a1x + TEST_EMAX);
  const float* gphi = reinterpret_cast<const float*>(A.stage + A.off_phi);
  const float* gs1 = reinterpret_cast<const float*>(A.stage + A.off_s1);
  const FDiv fn = fdiv(A.n_s), fd = fdiv(A.d);
  for (int i = tid; i < A.E * A.n_s; i += 256) {
    const int e = i / fn;
    SFX_CHK(e >= 0 && e < A.E, e, A.E, i);
    if (live[e]) {
      A.S[i] = A.S1[i];
      A.S1[i] = gs1[i];
    }
  }
  for (int i = tid; i < A.E * A.d; i += 256) {
    const int e = i / fd;
    SFX_CHK(e >= 0 && e < A.E, e, A.E, i);
    if (live[e]) A.phi[i] = gphi[i];
  }
  for (int i = tid; i < A.E * 6; i += 256)
    if (live[i / 6]) A.rowp[i] = rowp[i];
  if (tid < A.E) {
    A.live[tid] = live[tid];
    if (live[tid]) {
      A.a[tid] = a[tid];
      A.a1x[tid] = a1x[tid];
    }
  }
  if (tid == 0) {
    SFX_CHK(!H.update || (H.step >= 0 && H.step < A.horizon), H.step, A.horizon, H.update);
    TsfTestDevHdr d{H.step, H.update, hp[0], hp[1], hp[2], {0, 0, 0}};
    *A.hdr = d;
    __hip_atomic_store(A.dseq, H.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct TsfTestRowArgs {
  const TsfTestDevHdr* hdr;
  const int* live;     // [E]
  const int* a1x;      // [E] explored a1 or -1
  const float* psi_s1; // ψ_t(s1) of the online heads: an activation role, as TsfTestArgs::psi
  float* loss;         // [horizon][E][3]: loss, l2, l1 of each step's update
  int64_t* sel;        // [E][2]: the step's a1, the next step's greedy action
  int E, horizon;
};

// (c) of a TSF lockstep step, one workgroup per row; a row that is not live returns at once.  When
// the header asks for an update: a1 = the explored one, or the greedy action at s1 under the row's
// (w, ω) as they stand (tsf_test_greedy: k_tsf_test_act's arithmetic), then one
// update_test_reward_mapper step with it (tsf_test_step_body: k_tsf_test_step's arithmetic, its losses
// into loss[step][e]).  Then, for every live row, the greedy action at s1 under the updated (w, ω):
// the action the row takes next unless it explores.  A0: sfx_tsf_test_updates' arguments (psi = ψ(S),
// psi1 = ψ⁻(S1) of the E rows; gamma / beta / lasso / losses come from the device header).
__global__ __launch_bounds__(256) void k_tsf_test_row(TsfTestArgs A0, TsfTestRowArgs X) {
  const int e = blockIdx.x, tid = threadIdx.x;
  SFX_CHK(e < X.E && X.E <= TEST_EMAX, e, X.E, 0);
  if (!X.live[e]) return;
  __shared__ float s_on[64];
  __shared__ float s_q[256];
  __shared__ int s_a1;
  const TsfTestDevHdr H = *X.hdr;
  A0.gamma = H.gamma;
  A0.beta = H.beta;
  A0.lasso = H.lasso;
  const int step = H.update && H.step >= 0 && H.step < X.horizon ? H.step : 0;
  A0.losses = X.loss + (size_t)step * X.E * 3;
  const TsfTestArgs A = tsf_test_row(A0, e);
  TsfTestArgs Ag = A;  // the greedy choice at s1
  Ag.psi = X.psi_s1 + (long long)e * A.O;
  if (H.update) {
    SFX_CHK(H.step >= 0 && H.step < X.horizon, H.step, X.horizon, e);
    const int x = X.a1x[e];
    const int g = x >= 0 ? x : tsf_test_greedy(Ag, s_on, s_q);  // x is the workgroup's: a uniform branch
    if (tid == 0) {
      s_a1 = g;
      X.sel[2 * e] = g;
    }
    __syncthreads();
    const int a = (int)*A.a, a1 = s_a1;
    SFX_CHK(a >= 0 && a < A.A && a1 >= 0 && a1 < A.A, a, a1, A.A);
    tsf_test_step_body(A, a, a1);
    __threadfence_block();  // the row's stores of w and ω: visible to the whole workgroup
    __syncthreads();
  }
  const int best = tsf_test_greedy(Ag, s_on, s_q);
  if (tid == 0) X.sel[2 * e + 1] = best;
}

// -------------------------------------------------------------------------------------
// The learned-φ SF agent's test phase (sfx_runner_phi_test_phase): E episodes of
// agents/sfdqn_phi.py:234-261 in lockstep.  One lockstep step is k_phi_test_intake -> the φ forward of
// the E rows (phi_rows_impl: φ(S ⊕ a ⊕ S1) into the φ state's phis) -> the ψ forward of every online
// head on the E S1 rows -> k_phi_test_row -> k_test_publish, a linear chain; the staging record is
// phi_test_stage_layout's (sfx_test_host.h).
// -------------------------------------------------------------------------------------
static_assert(PHI_TEST_EMAX == PHIE, "the φ phase steps as many rows as one launch of the E-row φ kernels takes");
static_assert(PHI_IN <= 2 * PHI_TEST_NS + 1, "every n_s a φ setup takes (2 n_s + 1 <= PHI_IN) fits k_phi_test_intake's LDS");

// what the intake leaves on the device for the row kernel and the publication
struct PhiTestDevHdr {
  long long seq;  // the record's sequence number: k_test_publish's dseq
  int step, update;
};
static_assert(sizeof(PhiTestDevHdr) == 16, "PhiTestDevHdr: one 16-byte word");

// The phase's device block, one allocation: byte offsets of its parts (multiples of 16)
struct PhiTestDevLayout {
  int hdr, live, a, r, S, S1;
  size_t bytes;
};
inline PhiTestDevLayout phi_test_dev_layout(int n_s) {
  PhiTestDevLayout L{};
  const auto up16 = [](size_t n) { return (n + 15) / 16 * 16; };
  L.hdr = 0;
  L.live = (int)sizeof(PhiTestDevHdr);
  L.a = L.live + 4 * PHI_TEST_EMAX;
  L.r = L.a + 8 * PHI_TEST_EMAX;
  L.S = L.r + 4 * PHI_TEST_EMAX;
  L.S1 = L.S + (int)up16(sizeof(float) * PHI_TEST_EMAX * (size_t)n_s);
  L.bytes = (size_t)L.S1 + up16(sizeof(float) * PHI_TEST_EMAX * (size_t)n_s);
  return L;
}

struct PhiTestIntakeArgs {
  const unsigned char* stage;  // host-coherent staging record (phi_test_stage_layout)
  int E, n_s, horizon, pad_;
  PhiTestDevHdr* hdr;
  int* live;    // [E]
  int64_t* a;   // [E] the actions taken at s, as the φ kernels read them
  float* r;     // [E]
  float* S;     // [E][n_s]: a live row's previous S1 row
  float* S1;    // [E][n_s]: its new s1
};

// (a) of a φ lockstep step, one workgroup.  The whole record (at most PHI_TEST_PRE + 2 KB) comes through
// LDS in 16-byte words.  For every live row the previous S1 row becomes its S row and the record's s1
// its S1 row; its action (widened) and r go to the device block, the live mask and the header too.  The
// phase's first record (update 0) carries the initial states: S = S1 = s0 and a = 0, so the φ forward
// of that launch reads defined rows.  A row that is not live keeps everything it had.
__global__ __launch_bounds__(256) void k_phi_test_intake(PhiTestIntakeArgs A) {
  constexpr int PRE16 = PHI_TEST_PRE / 16;
  __shared__ __attribute__((aligned(16))) uint4 s_rec[PRE16 + PHI_TEST_EMAX * PHI_TEST_NS / 4];
  const int tid = threadIdx.x;
  SFX_CHK(A.E >= 1 && A.E <= PHI_TEST_EMAX && A.n_s <= PHI_TEST_NS, A.E, A.n_s, 0);
  if (A.E < 1 || A.E > PHI_TEST_EMAX || A.n_s < 1 || A.n_s > PHI_TEST_NS) return;  // refused by the host already
  const int nrow = A.E * A.n_s;
  const uint4* src = reinterpret_cast<const uint4*>(A.stage);
  for (int i = tid; i < PRE16 + (nrow + 3) / 4; i += 256) s_rec[i] = src[i];
  __syncthreads();
  const TestStageHdr& H = *reinterpret_cast<const TestStageHdr*>(s_rec);
  const int* live = reinterpret_cast<const int*>(s_rec) + sizeof(TestStageHdr) / 4;
  const float* r = reinterpret_cast<const float*>(live + PHI_TEST_EMAX);
  const int* a = live + 2 * PHI_TEST_EMAX;
  const float* s1 = reinterpret_cast<const float*>(s_rec + PRE16);
  const FDiv fn = fdiv(A.n_s);
  for (int i = tid; i < nrow; i += 256) {
    const int e = i / fn;
    SFX_CHK(e >= 0 && e < A.E, e, A.E, i);
    if (live[e]) {
      const float v = s1[i];
      A.S[i] = H.update ? A.S1[i] : v;
      A.S1[i] = v;
    }
  }
  if (tid < A.E) {
    A.live[tid] = live[tid];
    if (live[tid]) {
      A.a[tid] = H.update ? a[tid] : 0;
      A.r[tid] = r[tid];
    }
  }
  if (tid == 0) {
    SFX_CHK(!H.update || (H.step >= 0 && H.step < A.horizon), H.step, A.horizon, H.update);
    A.hdr->step = H.step;
    A.hdr->update = H.update;
    __hip_atomic_store(&A.hdr->seq, H.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct PhiTestRowArgs {
  const PhiTestDevHdr* hdr;
  const int* live;  // [E]
  const float* r;   // [E]
  float* loss;      // [horizon][E]: the pre-step loss of each step's update
  int E, horizon, w_stride, pad_;
};

// (c) of a φ lockstep step, one workgroup per row; a row that is not live returns at once.  When the
// header asks for an update: one update_test_reward_mapper step on the row's (w, b) with φ_e
// (phi_test_step_row: k_phi_test_steps' arithmetic), its loss into loss[step][e].  Then, whatever the
// flag, the biased GPI selection at S1 under the updated (w, b) (phi_test_act_row: k_phi_test_act's
// arithmetic) into sel[e] = (c, a): the action the row takes next unless it explores.  G / g:
// sfx_phi_test_actions' arguments (ψ(S1) of the E rows in g.role); A: sfx_phi_test_updates'.
__global__ __launch_bounds__(256) void k_phi_test_row(Geo G, GpiArgs g, float* Wb, PhiTestArgs A, PhiTestRowArgs X) {
  const int e = blockIdx.x;
  SFX_CHK(e < X.E && X.E <= PHI_TEST_EMAX, e, X.E, 0);
  if (!X.live[e]) return;
  const int update = X.hdr->update, hstep = X.hdr->step;
  if (update) {  // the header is the grid's: a uniform branch
    SFX_CHK(hstep >= 0 && hstep < X.horizon, hstep, X.horizon, e);
    const int step = hstep >= 0 && hstep < X.horizon ? hstep : 0;
    A.w += (long long)e * X.w_stride;
    A.wb = Wb + e;
    A.phi += (long long)e * A.d;
    A.r = X.r[e];
    A.losses = X.loss + (size_t)step * X.E + e;
    phi_test_step_row(A);
    __threadfence_block();  // the row's stores of w and b: visible to the whole workgroup
    __syncthreads();
  }
  phi_test_act_row(G, g, Wb, e);
}

}  // namespace sfx
