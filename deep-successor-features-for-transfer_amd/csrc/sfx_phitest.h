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
// One workgroup each: the step is 2 (A + 1) products of the d × T d matrix and one pass over it, 588 entries
// at the reference's T = 4, d = 12, A = 9 -- launch latency, not work.  Limits (LDS): d <= 64, A <= 64,
// A d <= 1024, T d <= 1024, A T d <= 4096 (x_a and y_a of every action are held, 32 KB).
#pragma once

namespace sfx {

constexpr int PHI1_R = 2, PHI1_S = 2;  // rows of W per workgroup, waves per row
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

// SFDQN_PHI.update_test_reward_mapper after φ: one wave
__global__ __launch_bounds__(64) void k_phi_test_step(PhiTestArgs A) {
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

}  // namespace sfx
