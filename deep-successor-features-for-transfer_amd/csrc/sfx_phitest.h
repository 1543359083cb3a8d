// sfx_phitest.h -- the test phase of the learned-φ agents: agents/tsfdqn_phi.py TSFDQN_PHI.get_test_action
// (:381-397) and update_target_models (:434-505), agents/sfdqn_phi.py SFDQN_PHI.update_test_reward_mapper
// (:263-305).  Device side; the entry points are in sfx_phi.inc.
//
// A test step is ONE transition: φ = phi_net(s ⊕ a ⊕ s1) is a one-row pass through the φ net.
//
//   k_phi1_fwd  one Linear (+ ReLU) of the wide φ net (hid > 128) for one row: y[o] = act(W[o]·x + b[o]),
//               a GEMV.  At hid 2048 a hidden layer is 16 MB of weights for 4 M FMAs: bytes and latency,
//               no arithmetic, so the shape is the one that keeps the most loads in flight -- PHI1_S waves stream
//               each row of W (consecutive lanes consecutive 16-byte words, every load of a 1024-float trip
//               issued before the first use), PHI1_R rows per workgroup: 2 × 2 waves, 1024 workgroups of
//               256 threads on a 2048-wide layer, 4 per CU, 16 KB in flight each.  Rows that are not
//               16-byte aligned (an odd K: layer 0's K = 2 n_s + 1 always, hid 131) take coalesced scalar
//               loads.  Layer 0 reads its input straight from s, a, s1.  Reduction: an fmaf chain per lane
//               in k order, a xor butterfly across the wave, the waves of a row added in wave order
//               through LDS -- no atomics, the same bits every run.
//               (k_phiw_fwd<1> at B = 1 is 128 workgroups of 16-row MFMA tiles with one row in use.)
//               Measured: the 5 launches of a 2048-wide net take 35.1 µs, 1.44 TB/s of weight
//               bytes, 1.24× faster than k_phiw_in + 5 × k_phiw_fwd<1> at B = 2; ≈5 µs of each launch are the
//               boundary and the first operands' round trip, which a dependent chain pays per layer.
//
// TSF-φ (Ω = agent.omegas, Linear(T d, d): W [d][T d], β [d]; the test task's w = Linear(d, 1): w [d], b_w;
// λ its loss coefficient; flat(ψ)[a][t d + k] = ψ_t[a][k]):
//
//   k_tsfphi_test_act   q_a = w·Ω(flat(ψ(s))[a]) + b_w, the first argmax.
//   k_tsfphi_test_step  x_a = flat(ψ(s))[a], y_a = flat(ψ⁻(s1))[a], c = concat_t g_t(s), c1 = concat_t g_t(s1)
//       σ = Ω(c), σ1 = Ω(c1), aff = h(σ) + h(σ1), φ̃ = φ ⊙ aff
//       P_a = Ω(x_a), N_a = Ω(y_a), e_a = P_a - (φ̃ + γ N_a)
//       psi_loss = Σ_a |e_a|² / (A d), ρ = w·φ̃ + b_w - r, phi_loss = ρ², loss = phi_loss + λ psi_loss
//       δ_a = 2 λ e_a / (A d), f = 2ρ w - Σ_a δ_a, κ = f ⊙ φ, η = W_hᵀ κ
//       ∂W = Σ_a δ_a (x_a - γ y_a)ᵀ + η (c + c1)ᵀ, ∂β = (1 - γ) Σ_a δ_a + 2η
//       ∂w = 2ρ φ̃, ∂b_w = 2ρ, ∂λ = psi_loss
//     every gradient clamped to ±1e10 (:495-497), one step of a freshly built Adam (:452; descent on
//     W, β, w, b_w, ascent on λ), λ clamped to [1e-2, 1e6] (:502).  ψ, ψ⁻, g_t, h and the φ net are read only.
//   k_phi_test_step     SF-φ: ρ = w·φ + b_w - r, loss = ρ², ∂w = 2ρ φ, ∂b_w = 2ρ, the same clamp and step.
//
// SF-φ's test tasks in lockstep (agents/sfdqn_phi.py:211-212 over test_agent :234-261; sfx/lockstep.py
// test_tasks_lockstep_phi): E <= PHIE rows per launch, every row bit for bit what the one-row call gives.
//   k_phiE_fwd        k_phi1_fwd for E rows: the same split of k over lanes and waves, the same fmaf chain,
//                     butterfly and wave-order add, E accumulators per lane.  A trip's words of W are loaded
//                     once and held in registers.  Rows in 16-byte words: k_phiE_fwd_lds, the E <= 8 input rows
//                     staged once per workgroup in LDS (64 KB at E = 8, K = 2048), two row groups of W per
//                     workgroup.  Scalar loads (layer 0, an odd hid): k_phiE_fwd, the rows read from L2 per use.
//                     k_phiE_narrow: the narrow net, a workgroup per row.
//                     Measured (hid 2048): 30.9 / 37.6 / 51.9 / 81.5 µs at E = 1 / 2 / 4 / 8,
//                     3.4× faster than 8 one-row chains, 1.8× slower than the MFMA forward at B = 8 (whose
//                     sums differ in the last bits).
//   k_phi_test_steps  k_phi_test_step for E rows, one wave per row, r read from the device.
//   k_phi_test_act    the E greedy actions under q = fl(ψ·w + b_w): the bias added after the dot product.
//
// One workgroup each: the step is 2 (A + 1) products of the d × T d matrix and one pass over it, 588 entries
// at the reference's T = 4, d = 12, A = 9 -- launch latency, not work.  Limits (LDS): d <= 64, A <= 64,
// A d <= 1024, T d <= 1024, A T d <= 4096 (x_a and y_a of every action are held, 32 KB).
#pragma once

namespace sfx {

constexpr int PHI1_R = 2, PHI1_S = 2;  // rows of W per workgroup, waves per row
constexpr int PHIE = 16;               // test tasks (input rows) per launch of the lockstep kernels
constexpr int PHIT_D = 64, PHIT_A = 64, PHIT_AD = 1024, PHIT_TD = 1024, PHIT_ATD = 4096;

struct Phi1Args {
  const float* W;   // [N][K], bias [N] right after
  const float* X;   // [K] the layer's input; nullptr: layer 0, x = s ⊕ a ⊕ s1
  float* Y;         // [N]
  const float* s;   // [n_s]
  const float* s1;
  const int64_t* a;
  int K, N, n_s, relu;
};

__device__ __forceinline__ float phi1_x(const Phi1Args& A, int k) {
  if (A.X) return A.X[k];
  return k < A.n_s ? A.s[k] : (k == A.n_s ? (float)*A.a : A.s1[k - A.n_s - 1]);
}

__global__ __launch_bounds__(64 * PHI1_R * PHI1_S) void k_phi1_fwd(Phi1Args A) {
  __shared__ float part[PHI1_R][PHI1_S];
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, rr = wv / PHI1_S, q = wv - rr * PHI1_S;
  const int K = A.K, N = A.N;
  const int o = blockIdx.x * PHI1_R + rr;
  float acc = 0.f;
  if (o < N) {
    const float* wrow = A.W + (long long)o * K;
    // the row and x in 16-byte words when both are aligned (every row: K a multiple of 4)
    const bool vec = A.X && phiw_vec(A.W, K, 4) && phiw_vec(A.X, K, 4);
    if (vec) {
      const int K4 = K >> 2, q4 = (K4 + PHI1_S - 1) / PHI1_S;  // words of the row, of a wave's share
      const int beg = q * q4, end = min(K4, beg + q4);
      const float4* w4 = reinterpret_cast<const float4*>(wrow);
      const float4* x4 = reinterpret_cast<const float4*>(A.X);
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int b = beg; b < end; b += 256) {
        float4 w[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = b + 64 * u + l;
          w[u] = i < end ? w4[i] : z4;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = b + 64 * u + l;
          x[u] = i < end ? x4[i] : z4;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          acc = __builtin_fmaf(w[u].x, x[u].x, acc);
          acc = __builtin_fmaf(w[u].y, x[u].y, acc);
          acc = __builtin_fmaf(w[u].z, x[u].z, acc);
          acc = __builtin_fmaf(w[u].w, x[u].w, acc);
        }
      }
    } else {
      const int kq = (K + PHI1_S - 1) / PHI1_S;
      const int beg = q * kq, end = min(K, beg + kq);
      for (int b = beg; b < end; b += 256) {
        float w[4], x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = b + 64 * u + l;
          w[u] = k < end ? wrow[k] : 0.f;
          x[u] = k < end ? phi1_x(A, k) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_fmaf(w[u], x[u], acc);
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, m, 64));
  if (l == 0) part[rr][q] = acc;
  __syncthreads();
  if (q == 0 && l == 0 && o < N) {
    float v = part[rr][0];
#pragma unroll
    for (int j = 1; j < PHI1_S; ++j) v = __fadd_rn(v, part[rr][j]);
    v = __fadd_rn(v, A.W[(long long)N * K + o]);
    A.Y[o] = A.relu ? fmaxf(v, 0.f) : v;
  }
}

struct PhiTestArgs {
  int T, A, d, n_s, lastOff, Pg;
  long long actSize;
  const float* psi;    // ψ_t(s): row 0 of an activation role, head stride actSize, at lastOff
  const float* psi1;   // ψ⁻_t(s1)
  const float* s;      // [n_s]
  const float* s1;
  const float* g;      // [T][Pg] g_t: W [d][n_s], b [d] (sfx_tsf_setup with K = 0)
  const float* hp;     // h: W [d][d], b [d]
  const float* phi;    // [d] φ of the transition
  float* oW;           // Ω: W [d][T d]
  float* ob;           // β [d]
  float* w;            // [d]
  float* wb;           // b_w
  float* lam;          // λ
  float r, gamma;
  float* losses;       // [3]: loss, psi_loss, phi_loss ([1] for k_phi_test_step)
  int64_t* act_out;
  AdamHP hpa;
};

__device__ __forceinline__ float phit_clamp(float g) { return fminf(fmaxf(g, -1e10f), 1e10f); }

// flat(ψ)[a][t d + k] of every action into LDS
__device__ __forceinline__ void phit_flat(const PhiTestArgs& A, const float* psi, float* dst) {
  const int Td = A.T * A.d;
  for (int i = threadIdx.x; i < A.A * Td; i += 256) {
    const int a = i / Td, j = i - a * Td, t = j / A.d, k = j - t * A.d;
    dst[i] = psi[(long long)t * A.actSize + A.lastOff + a * A.d + k];
  }
}

// Ω(v) row k: Σ_j W[k][j] v[j] + β[k], j ascending
__device__ __forceinline__ float phit_omega(const PhiTestArgs& A, int k, const float* v) {
  const int Td = A.T * A.d;
  const float* row = A.oW + (long long)k * Td;
  float acc = 0.f;
  for (int j = 0; j < Td; ++j) acc = __builtin_fmaf(row[j], v[j], acc);
  return __fadd_rn(acc, A.ob[k]);
}

__global__ __launch_bounds__(256) void k_tsfphi_test_act(PhiTestArgs A) {
  __shared__ float s_x[PHIT_ATD], s_P[PHIT_AD], s_q[PHIT_A];
  const int tid = threadIdx.x, d = A.d, Td = A.T * d;
  phit_flat(A, A.psi, s_x);
  __syncthreads();
  for (int i = tid; i < A.A * d; i += 256) {
    const int a = i / d, k = i - a * d;
    s_P[i] = phit_omega(A, k, s_x + a * Td);
  }
  __syncthreads();
  for (int a = tid; a < A.A; a += 256) {
    float q = 0.f;
    for (int k = 0; k < d; ++k) q = __builtin_fmaf(s_P[a * d + k], A.w[k], q);
    s_q[a] = __fadd_rn(q, *A.wb);
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int a = 1; a < A.A; ++a)
      if (s_q[a] > s_q[best]) best = a;
    *A.act_out = best;
  }
}

__global__ __launch_bounds__(256) void k_tsfphi_test_step(PhiTestArgs A) {
  __shared__ float s_x[PHIT_ATD], s_y[PHIT_ATD];          // x_a (then x_a - γ y_a), y_a
  __shared__ float s_P[PHIT_AD], s_N[PHIT_AD];  // P_a, N_a; then e_a, δ_a
  __shared__ float s_c[2][PHIT_TD], s_cs[PHIT_TD];
  __shared__ float s_sig[2][PHIT_D], s_w[PHIT_D], s_phi[PHIT_D], s_tphi[PHIT_D], s_sd[PHIT_D], s_kap[PHIT_D],
      s_eta[PHIT_D], s_pa[PHIT_A];
  __shared__ float s_rho, s_psi;
  const int tid = threadIdx.x, T = A.T, d = A.d, Td = T * d, nA = A.A;
  const float* Wh = A.hp;
  const float* bh = A.hp + d * d;
  const float gamma = A.gamma, wb = *A.wb, lam = *A.lam;
  const AdamC c1 = adam_consts(A.hpa, 1);
  phit_flat(A, A.psi, s_x);
  phit_flat(A, A.psi1, s_y);
  // c = concat_t g_t(s), c1 = concat_t g_t(s1)
  for (int i = tid; i < 2 * Td; i += 256) {
    const int which = i / Td, j = i - which * Td, t = j / d, k = j - t * d;
    const float* gp = A.g + (long long)t * A.Pg;
    const float* x = which ? A.s1 : A.s;
    float acc = 0.f;
    for (int q = 0; q < A.n_s; ++q) acc = __builtin_fmaf(gp[k * A.n_s + q], x[q], acc);
    s_c[which][j] = __fadd_rn(acc, gp[d * A.n_s + k]);
  }
  if (tid < d) {
    s_w[tid] = A.w[tid];
    s_phi[tid] = A.phi[tid];
  }
  __syncthreads();
  for (int j = tid; j < Td; j += 256) s_cs[j] = __fadd_rn(s_c[0][j], s_c[1][j]);
  // P_a, N_a, σ, σ1: 2 (A + 1) d rows of Ω
  for (int i = tid; i < 2 * (nA + 1) * d; i += 256) {
    const int which = i / ((nA + 1) * d), ii = i - which * (nA + 1) * d, a = ii / d, k = ii - a * d;
    if (a < nA)
      (which ? s_N : s_P)[a * d + k] = phit_omega(A, k, (which ? s_y : s_x) + a * Td);
    else
      s_sig[which][k] = phit_omega(A, k, s_c[which]);
  }
  __syncthreads();
  if (tid < d) {
    float h0 = 0.f, h1 = 0.f;
    for (int m = 0; m < d; ++m) {
      h0 = __builtin_fmaf(Wh[tid * d + m], s_sig[0][m], h0);
      h1 = __builtin_fmaf(Wh[tid * d + m], s_sig[1][m], h1);
    }
    const float aff = __fadd_rn(__fadd_rn(h0, bh[tid]), __fadd_rn(h1, bh[tid]));
    s_tphi[tid] = __fmul_rn(s_phi[tid], aff);
  }
  __syncthreads();
  // e_a into s_P; x_a - γ y_a into s_x (P_a, N_a are done with x_a, y_a)
  for (int i = tid; i < nA * d; i += 256) {
    const int k = i % d;
    s_P[i] = __fsub_rn(s_P[i], __fadd_rn(s_tphi[k], __fmul_rn(gamma, s_N[i])));
  }
  for (int i = tid; i < nA * Td; i += 256) s_x[i] = __builtin_fmaf(-gamma, s_y[i], s_x[i]);
  __syncthreads();
  if (tid < nA) {
    float se = 0.f;
    for (int k = 0; k < d; ++k) se = __builtin_fmaf(s_P[tid * d + k], s_P[tid * d + k], se);
    s_pa[tid] = se;
  }
  __syncthreads();
  const float nAd = (float)(nA * d);
  if (tid == 0) {
    float se = 0.f, rf = 0.f;
    for (int a = 0; a < nA; ++a) se = __fadd_rn(se, s_pa[a]);
    for (int k = 0; k < d; ++k) rf = __builtin_fmaf(s_tphi[k], s_w[k], rf);
    const float psi_loss = __fdiv_rn(se, nAd);
    const float rho = __fsub_rn(__fadd_rn(rf, wb), A.r);
    const float phi_loss = __fmul_rn(rho, rho);
    s_rho = rho;
    s_psi = psi_loss;
    A.losses[0] = __fadd_rn(phi_loss, __fmul_rn(lam, psi_loss));  // λ before its step
    A.losses[1] = psi_loss;
    A.losses[2] = phi_loss;
  }
  // δ_a into s_N
  const float cf = __fdiv_rn(__fmul_rn(2.f, lam), nAd);
  for (int i = tid; i < nA * d; i += 256) s_N[i] = __fmul_rn(cf, s_P[i]);
  __syncthreads();
  const float rho2 = __fmul_rn(2.f, s_rho);
  if (tid < d) {
    float sd = 0.f;
    for (int a = 0; a < nA; ++a) sd = __fadd_rn(sd, s_N[a * d + tid]);
    s_sd[tid] = sd;
    s_kap[tid] = __fmul_rn(__fsub_rn(__fmul_rn(rho2, s_w[tid]), sd), s_phi[tid]);
  }
  __syncthreads();
  if (tid < d) {
    float acc = 0.f;
    for (int k = 0; k < d; ++k) acc = __builtin_fmaf(Wh[k * d + tid], s_kap[k], acc);
    s_eta[tid] = acc;
  }
  __syncthreads();
  // the steps: Ω's weight (every read of it above is behind the barriers), β, w, b_w, λ
  for (int i = tid; i < d * Td; i += 256) {
    const int k = i / Td, j = i - k * Td;
    float g = 0.f;
    for (int a = 0; a < nA; ++a) g = __builtin_fmaf(s_N[a * d + k], s_x[a * Td + j], g);
    g = __builtin_fmaf(s_eta[k], s_cs[j], g);
    A.oW[i] = fresh_adam(A.oW[i], phit_clamp(g), c1);
  }
  if (tid < d) {
    const float gb = __builtin_fmaf(__fsub_rn(1.f, gamma), s_sd[tid], __fmul_rn(2.f, s_eta[tid]));
    A.ob[tid] = fresh_adam(A.ob[tid], phit_clamp(gb), c1);
    A.w[tid] = fresh_adam(s_w[tid], phit_clamp(__fmul_rn(rho2, s_tphi[tid])), c1);
  }
  if (tid == 64) {
    *A.wb = fresh_adam(wb, phit_clamp(rho2), c1);
    *A.lam = fminf(fmaxf(fresh_adam(lam, phit_clamp(s_psi), c1, true), 1e-2f), 1e6f);
  }
}

// SFDQN_PHI.update_test_reward_mapper after φ: one wave (the body of k_phi_test_step and k_phi_test_steps)
__device__ __forceinline__ void phi_test_step_row(const PhiTestArgs& A) {
  __shared__ float s_rho;
  const int tid = threadIdx.x, d = A.d;
  const AdamC c1 = adam_consts(A.hpa, 1);
  const float wb = *A.wb;
  const float wk = tid < d ? A.w[tid] : 0.f, pk = tid < d ? A.phi[tid] : 0.f;
  if (tid == 0) {
    float rf = 0.f;
    for (int k = 0; k < d; ++k) rf = __builtin_fmaf(A.phi[k], A.w[k], rf);
    const float rho = __fsub_rn(__fadd_rn(rf, wb), A.r);
    s_rho = rho;
    A.losses[0] = __fmul_rn(rho, rho);
  }
  __syncthreads();
  const float rho2 = __fmul_rn(2.f, s_rho);
  if (tid < d) A.w[tid] = fresh_adam(wk, phit_clamp(__fmul_rn(rho2, pk)), c1);
  if (tid == 0) *A.wb = fresh_adam(wb, phit_clamp(rho2), c1);
}

__global__ __launch_bounds__(64) void k_phi_test_step(PhiTestArgs A) { phi_test_step_row(A); }

// ---- E test tasks in lockstep (sfx.lockstep.test_tasks_lockstep_phi) ---------------------------

// E rows of one Linear (+ ReLU) of the wide φ net; Y[e][o] is bit for bit what k_phi1_fwd writes for row e
struct PhiEArgs {
  const float* W;   // [N][K], bias [N] right after
  const float* X;   // [E][K] the layer's input; nullptr: layer 0, x_e = S[e] ⊕ a[e] ⊕ S1[e]
  float* Y;         // [E][N]
  const float* S;   // [E][n_s]
  const float* S1;
  const int64_t* a; // [E]
  int K, N, n_s, relu, E;
};

__device__ __forceinline__ float phiE_x(const PhiEArgs& A, int e, int k) {
  if (A.X) return A.X[(long long)e * A.K + k];
  const long long r = (long long)e * A.n_s;
  return k < A.n_s ? A.S[r + k] : (k == A.n_s ? (float)A.a[e] : A.S1[r + k - A.n_s - 1]);
}

// k_phi1_fwd's scalar-load path for E rows (a row of W or x that is not in 16-byte words: layer 0 always, an
// odd hid; phi_rows_impl sends every other layer to k_phiE_fwd_lds).  The input rows are read per use.
// EB: the accumulators a lane holds, E <= EB; the slots past E recompute row E - 1 and are dropped
template <int EB>
__global__ __launch_bounds__(64 * PHI1_R * PHI1_S) void k_phiE_fwd(PhiEArgs A) {
  __shared__ float part[PHI1_R][PHI1_S][EB];
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, rr = wv / PHI1_S, q = wv - rr * PHI1_S;
  const int K = A.K, N = A.N, E = A.E;
  const int o = blockIdx.x * PHI1_R + rr;
  float acc[EB];
#pragma unroll
  for (int e = 0; e < EB; ++e) acc[e] = 0.f;
  if (o < N) {
    const float* wrow = A.W + (long long)o * K;
    const int kq = (K + PHI1_S - 1) / PHI1_S;
    const int beg = q * kq, end = min(K, beg + kq);
    for (int b = beg; b < end; b += 256) {
      float w[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = b + 64 * u + l;
        w[u] = k < end ? wrow[k] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < EB; ++e) {
        const int er = min(e, E - 1);
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = b + 64 * u + l;
          x[u] = k < end ? phiE_x(A, er, k) : 0.f;
        }
        float v = acc[e];
#pragma unroll
        for (int u = 0; u < 4; ++u) v = __builtin_fmaf(w[u], x[u], v);
        acc[e] = v;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EB; ++e) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[e] = __fadd_rn(acc[e], __shfl_xor(acc[e], m, 64));
    if (l == 0) part[rr][q][e] = acc[e];
  }
  __syncthreads();
  if (q == 0 && l < E && o < N) {  // lane e finishes row e
    float v = part[rr][0][l];
#pragma unroll
    for (int j = 1; j < PHI1_S; ++j) v = __fadd_rn(v, part[rr][j][l]);
    v = __fadd_rn(v, A.W[(long long)N * K + o]);
    A.Y[(long long)l * N + o] = A.relu ? fmaxf(v, 0.f) : v;
  }
}

// k_phiE_fwd's 16-byte-word path with the E <= EB <= PHIE_LDS input rows staged once per workgroup in LDS
// (K <= PHIW_HID: 8 KB a row) and PHIE_G row groups of W per workgroup, so the rows are fetched from L2 once per
// 2 PHIE_G rows of W instead of once per wave.  The first trip's words of W of every row group are requested
// before the staging, so they are in flight while it runs.  Per row of W the same lanes, waves and fmaf order.
constexpr int PHIE_G = 2, PHIE_LDS = 8;

template <int EB>  // 2 waves per SIMD: the grid is 2 workgroups per CU on a 2048-wide layer, and 64 KB of LDS allow no more
__global__ __launch_bounds__(64 * PHI1_R * PHI1_S, 2) void k_phiE_fwd_lds(PhiEArgs A) {
  static_assert(EB <= PHIE_LDS, "LDS holds PHIE_LDS rows");
  __shared__ float4 xs[EB * (PHIW_HID / 4)];
  __shared__ float part[PHIE_G][PHI1_R][PHI1_S][EB];
  const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63, rr = wv / PHI1_S, q = wv - rr * PHI1_S;
  const int K = A.K, N = A.N, E = A.E;
  const int K4 = K >> 2, q4 = (K4 + PHI1_S - 1) / PHI1_S;
  const int beg = q * q4, end = min(K4, beg + q4);
  const float4* x4 = reinterpret_cast<const float4*>(A.X);
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 w0[PHIE_G][4];
#pragma unroll
  for (int g = 0; g < PHIE_G; ++g) {
    const int o = (blockIdx.x * PHIE_G + g) * PHI1_R + rr;
    const float4* w4 = reinterpret_cast<const float4*>(A.W + (long long)min(o, N - 1) * K);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = beg + 64 * u + l;
      w0[g][u] = (o < N && i < end) ? w4[i] : z4;
    }
  }
  for (int i = tid; i < E * K4; i += 64 * PHI1_R * PHI1_S) xs[i] = x4[i];
  __syncthreads();
  float acc[PHIE_G][EB];
#pragma unroll
  for (int g = 0; g < PHIE_G; ++g) {
#pragma unroll
    for (int e = 0; e < EB; ++e) acc[g][e] = 0.f;
    const int o = (blockIdx.x * PHIE_G + g) * PHI1_R + rr;
    if (o < N) {
      const float4* w4 = reinterpret_cast<const float4*>(A.W + (long long)o * K);
      for (int b = beg; b < end; b += 256) {
        float4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = b + 64 * u + l;
          w[u] = b == beg ? w0[g][u] : (i < end ? w4[i] : z4);
        }
#pragma unroll
        for (int e = 0; e < EB; ++e) {
          const float4* xe = xs + min(e, E - 1) * K4;
          float4 x[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int i = b + 64 * u + l;
            x[u] = i < end ? xe[i] : z4;
          }
          float v = acc[g][e];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v = __builtin_fmaf(w[u].x, x[u].x, v);
            v = __builtin_fmaf(w[u].y, x[u].y, v);
            v = __builtin_fmaf(w[u].z, x[u].z, v);
            v = __builtin_fmaf(w[u].w, x[u].w, v);
          }
          acc[g][e] = v;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EB; ++e) {
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) acc[g][e] = __fadd_rn(acc[g][e], __shfl_xor(acc[g][e], m, 64));
      if (l == 0) part[g][rr][q][e] = acc[g][e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < PHIE_G; ++g) {
    const int o = (blockIdx.x * PHIE_G + g) * PHI1_R + rr;
    if (q == 0 && l < E && o < N) {  // lane e finishes row e
      float v = part[g][rr][0][l];
#pragma unroll
      for (int j = 1; j < PHI1_S; ++j) v = __fadd_rn(v, part[g][rr][j][l]);
      v = __fadd_rn(v, A.W[(long long)N * K + o]);
      A.Y[(long long)l * N + o] = A.relu ? fmaxf(v, 0.f) : v;
    }
  }
}

// A narrow net (hid <= PHI_HID): k_phi_fwd's computation of one row (the fmaf chain over k, the bias, the
// ReLU), one workgroup per row, the activations in LDS only.
__global__ __launch_bounds__(256) void k_phiE_narrow(PhiArgs A) {
  __shared__ float sx[PHI_HID], sy[PHI_HID];
  const int tid = threadIdx.x, e = blockIdx.x, n_s = A.n_s, L = A.n_mid + 2;
  for (int k = tid; k < A.n_in; k += 256)
    sx[k] = k < n_s ? A.S[(long long)e * n_s + k]
                    : (k == n_s ? (float)A.a[e] : A.S1[(long long)e * n_s + (k - n_s - 1)]);
  __syncthreads();
  float* x = sx;
  float* y = sy;
  for (int l = 0; l < L; ++l) {
    const int K = phi_layer_in(A, l), N = phi_layer_out(A, l);
    const float* W = A.p + phi_layer_off(A, l);
    const float* bias = W + (long long)N * K;
    for (int o = tid; o < N; o += 256) {
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = __builtin_fmaf(x[k], W[(long long)o * K + k], acc);
      acc = __fadd_rn(acc, bias[o]);
      if (l == L - 1)
        A.phis[(long long)e * N + o] = acc;
      else
        y[o] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    float* t = x;
    x = y;
    y = t;
  }
}

// E updates of k_phi_test_step in one launch, one wave (workgroup) per row: row e's w at w + e w_stride, its
// bias at wb + e, φ_e at phi + e d, r_e read from the device, loss_e to losses + e.
__global__ __launch_bounds__(64) void k_phi_test_steps(PhiTestArgs A, const float* r, int w_stride) {
  const int e = blockIdx.x;
  A.w += (long long)e * w_stride;
  A.wb += e;
  A.phi += (long long)e * A.d;
  A.r = r[e];
  A.losses += e;
  phi_test_step_row(A);
}

// SFDQN_PHI.get_test_action's greedy branch for E test tasks (agents/sfdqn_phi.py:223-232 over
// features/deep_phi.py GPI_w): k_gpi's row with the reward model's bias added AFTER the dot product,
// q[e,t,a] = fl(ψ_t(S[e])[a,:]·W[e,:] + Wb[e]), then the first-index argmaxes.  One workgroup per row.
// phi_test_act_row is the whole 256-thread workgroup's body for row b; k_phi_test_act and the native test
// phase's row kernel (k_phi_test_row, sfx_testphase.h) both call it.
__device__ __forceinline__ void phi_test_act_row(const Geo& G, const GpiArgs& A, const float* Wb, const int b) {
  __shared__ float s_q[QMAX];
  __shared__ float s_w[DMAX];
  __shared__ float s_mt[256], s_ma[256];
  const int tid = threadIdx.x;
  const int T = G.T, Aa = G.A, d = G.d, O = G.O, NLm = G.lastOff, TA = T * Aa;
  const long long ob = (long long)(A.row0 + b);
  const int lb = A.rowoff + b;
  const float* wr = A.w + ob * A.w_stride;
  const float wb = Wb[ob];
  int64_t* so = A.sel_out + ob * A.sel_stride;
  for (int k = tid; k < d; k += 256) s_w[k] = wr[k];
  __syncthreads();
  for (int idx = tid; idx < TA; idx += 256) {
    const int t = idx / Aa, a = idx - t * Aa;
    const float* p = G.actp(A.role, t, NLm) + (size_t)lb * O + a * d;
    float q = 0.f;
#pragma unroll 8
    for (int k = 0; k < d; ++k) q = __builtin_fmaf(p[k], s_w[k], q);
    q = __fadd_rn(q, wb);
    s_q[idx] = q;
    if (A.q_out) A.q_out[(ob * T + t) * Aa + a] = q;
  }
  __syncthreads();
  gpi_pick(A, s_q, s_mt, s_ma, T, Aa, ob, so, 256);
}

__global__ __launch_bounds__(256) void k_phi_test_act(Geo G, GpiArgs A, const float* Wb) {
  phi_test_act_row(G, A, Wb, blockIdx.x);
}

}  // namespace sfx
