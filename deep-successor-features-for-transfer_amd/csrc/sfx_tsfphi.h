// sfx_tsfphi.h -- TSF-DQN with a learned φ: agents/tsfdqn_phi.py TSFDQN_PHI.update_deep_models
// (:180-288) over features/deep_tsf_phi.py DeepSF_TSF_PHI, the library of main_tsfdqn_phi_torch.py.
// Device side of the transform around the φ net; the φ net itself is sfx_phi.h (hid <= 128) or
// sfx_phiw.h (wider), the ψ part the SF-DQN kernels with φ̃ as the features.
//
//   x_b = s_b ⊕ a_b ⊕ s1_b, φ_b = phi_net(x_b), u_b = g_i(s_b), u'_b = g_i(s1_b)   (g_i, h: Linear)
//   t_b = h(u_b) + h(u'_b), φ̃_b = φ_b ⊙ t_b
//   y_b = φ̃_b + γ_b ψ⁻_i(s1_b)[a'_b], psi_loss = MSE(ψ_i(s), merged), e_b = w_i·φ̃_b + b_i - r_b,
//   phi_loss = mean e², loss = phi_loss + λ_i psi_loss
//   dφ̃_b = -λ_i ∂psi_loss/∂ψ_i(s_b)[a_b] + (2/B) e_b w_i, dφ_b = dφ̃_b ⊙ t_b, dt_b = dφ̃_b ⊙ φ_b
//   dW_h = Σ_b dt_b ⊗ (u_b + u'_b), db_h = 2 Σ_b dt_b, du_b = W_hᵀ dt_b
//   dW_g = Σ_b du_b ⊗ (s_b + s1_b), db_g = 2 Σ_b du_b
//   dw_i = Σ_b (2/B) e_b φ̃_b, db_i = Σ_b (2/B) e_b, dλ_i = psi_loss (ascent)
//
// k_tsfphi_fwd runs after the φ net's forward (u, u', t, φ̃; h evaluated twice, then added, as the
// reference does); k_tsfphi_bwd after the ψ backward: the head (e, dφ̃, the steps of w_i, b_i, λ_i,
// the losses), dφ as the φ net's output gradient, and the steps of g_i and h.  One workgroup each:
// d <= 64, n_s <= 31, B <= 64.  With transform = 0 k_tsfphi_bwd is the head of DeepSF_PHI's update
// alone (φ̃ = φ, t = 1; sfx_phi_update on a wide net).
//
// The optimiser is a freshly built Adam (:249) after grad.clamp_(-1, 1) (:268-270).  These kernels and
// sfx_phiw.h's dW epilogue clamp literally.  The ψ heads' Adam epilogue (the headline kernel) is left
// alone and does not clamp: a fresh Adam's step is lr·g/(|g| + ε), for |g| >= 1 that is ±lr to within
// one ulp of the step with or without the clamp (ε = 1e-8 is below half an ulp of |g| >= 1), and for
// |g| < 1 the clamp is the identity.
//
// k_tsfphi_bwd steps w_i, its bias, λ_i, g_i and h in place: it reads TsfPhiArgs::cancel first and a runner
// step cancelled at its gate commits none of them (step_cancelled, sfx_kernels.h); dφ and the losses are
// transient and written either way.
#pragma once

namespace sfx {

struct TsfPhiArgs {
  int B, d, n_s, O, transform, clamp;
  const float* S;       // [B][n_s]
  const float* S1;
  const int64_t* a;
  const float* r;       // [B]
  float* g;             // g_i: W [d][n_s], b [d]
  float* hp;            // h: W [d][d], b [d]
  const float* phis;    // [B][d] φ
  float* tphi;          // [B][d] φ̃ (= phis when transform = 0)
  float* tt;            // [B][d] t
  float* usum;          // [B][d] u + u'
  const float* dzlast;  // [B][O] the ψ output gradient of the policy (λ-scaled), nonzero at a_b only
  float* gtop;          // [B][d] dφ, the φ net's output gradient
  float* w;             // [d] w_i
  float* wb;            // w_i's bias
  float* lam;           // λ_i
  float* losses;        // [4]: loss, psi_loss (written by the ψ tail), phi_loss, λ_i after
  AdamHP hpa;
  const int* cancel;    // runner steps: 1 when the step's gate cancelled it (no commit); 0 otherwise
};

__device__ __forceinline__ float tsfphi_clamp(float g, int on) { return on ? fminf(fmaxf(g, -1.f), 1.f) : g; }

__global__ __launch_bounds__(256) void k_tsfphi_fwd(TsfPhiArgs A) {
  __shared__ float su[2][PHI_B * PHI_IN];
  const int tid = threadIdx.x, B = A.B, d = A.d, n_s = A.n_s;
  const float* Wg = A.g;
  const float* bg = A.g + d * n_s;
  const float* Wh = A.hp;
  const float* bh = A.hp + d * d;
  for (int j = tid; j < 2 * B * d; j += 256) {
    const int q = j / (B * d), jj = j - q * B * d, b = jj / d, m = jj - b * d;
    const float* s = (q ? A.S1 : A.S) + (long long)b * n_s;
    float acc = 0.f;
    for (int k = 0; k < n_s; ++k) acc = __builtin_fmaf(s[k], Wg[m * n_s + k], acc);
    su[q][b * d + m] = __fadd_rn(acc, bg[m]);
  }
  __syncthreads();
  for (int j = tid; j < B * d; j += 256) {
    const int b = j / d, o = j - b * d;
    float h0 = 0.f, h1 = 0.f;
    for (int m = 0; m < d; ++m) {
      h0 = __builtin_fmaf(su[0][b * d + m], Wh[o * d + m], h0);
      h1 = __builtin_fmaf(su[1][b * d + m], Wh[o * d + m], h1);
    }
    const float t = __fadd_rn(__fadd_rn(h0, bh[o]), __fadd_rn(h1, bh[o]));
    A.tt[j] = t;
    A.usum[j] = __fadd_rn(su[0][j], su[1][j]);
    A.tphi[j] = __fmul_rn(A.phis[j], t);
  }
}

__global__ __launch_bounds__(256) void k_tsfphi_bwd(TsfPhiArgs A) {
  __shared__ float sa[PHI_B * PHI_IN], sb[PHI_B * PHI_IN];
  __shared__ float s_w[PHI_IN], s_e[PHI_B];
  const int tid = threadIdx.x, B = A.B, d = A.d, n_s = A.n_s;
  const AdamC c1 = adam_consts(A.hpa, 1);
  const int cx = step_cancelled(A.cancel);
  if (tid < d) s_w[tid] = A.w[tid];
  __syncthreads();
  const float wb = *A.wb;
  // r_fit_b - r_b with w_i before its step
  for (int b = tid; b < B; b += 256) {
    float rf = 0.f;
    for (int k = 0; k < d; ++k) rf = __builtin_fmaf(A.tphi[(long long)b * d + k], s_w[k], rf);
    s_e[b] = __fsub_rn(__fadd_rn(rf, wb), A.r[b]);
  }
  __syncthreads();
  const float nrm = (float)(2.0 / (double)B);
  // dφ̃ = -dz[b][a_b][:] (λ-scaled ∂psi_loss/∂ψ; ∂/∂y is its negative) + (2/B) e_b w
  for (int j = tid; j < B * d; j += 256) {
    const int b = j / d, k = j - b * d;
    const int ab = (int)A.a[b];
    const float dz = A.dzlast[(long long)b * A.O + ab * d + k];
    const float dp = __fadd_rn(-dz, __fmul_rn(__fmul_rn(nrm, s_e[b]), s_w[k]));
    if (A.transform) {
      A.gtop[j] = __fmul_rn(dp, A.tt[j]);
      sb[j] = __fmul_rn(dp, A.phis[j]);  // dt
    } else {
      A.gtop[j] = dp;
    }
  }
  // w_i, its bias (gradients Σ_b (2/B) e_b φ̃_b, Σ_b (2/B) e_b), phi_loss, λ_i
  if (tid < d) {
    float g = 0.f;
    for (int b = 0; b < B; ++b) g = __builtin_fmaf(__fmul_rn(nrm, s_e[b]), A.tphi[(long long)b * d + tid], g);
    if (!cx) A.w[tid] = fresh_adam(s_w[tid], tsfphi_clamp(g, A.clamp), c1);
  }
  if (tid == 64) {
    float gb = 0.f, sse = 0.f;
    for (int b = 0; b < B; ++b) {
      gb = __fadd_rn(gb, __fmul_rn(nrm, s_e[b]));
      sse = __builtin_fmaf(s_e[b], s_e[b], sse);
    }
    if (!cx) *A.wb = fresh_adam(wb, tsfphi_clamp(gb, A.clamp), c1);
    const float phi_loss = (float)((double)sse / (double)B);
    const float psi_loss = A.losses[1];
    const float lam = *A.lam;
    A.losses[0] = __fadd_rn(phi_loss, __fmul_rn(lam, psi_loss));
    A.losses[2] = phi_loss;
    const float ln = fminf(fmaxf(fresh_adam(lam, tsfphi_clamp(psi_loss, A.clamp), c1, true), 1e-2f), 1e6f);
    if (!cx) *A.lam = ln;
    A.losses[3] = ln;
  }
  if (!A.transform || cx) return;  // cancelled: g_i and h keep their values (cx is uniform)
  __syncthreads();
  float* Wg = A.g;
  float* bg = A.g + d * n_s;
  float* Wh = A.hp;
  float* bh = A.hp + d * d;
  // du_b = W_hᵀ dt_b, W_h before its step
  for (int j = tid; j < B * d; j += 256) {
    const int b = j / d, m = j - b * d;
    float acc = 0.f;
    for (int o = 0; o < d; ++o) acc = __builtin_fmaf(sb[b * d + o], Wh[o * d + m], acc);
    sa[j] = acc;
  }
  __syncthreads();
  for (int j = tid; j < d * d; j += 256) {
    const int o = j / d, m = j - o * d;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = __builtin_fmaf(sb[b * d + o], A.usum[(long long)b * d + m], acc);
    Wh[j] = fresh_adam(Wh[j], tsfphi_clamp(acc, A.clamp), c1);
  }
  for (int j = tid; j < d * n_s; j += 256) {
    const int m = j / n_s, k = j - m * n_s;
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
      acc = __builtin_fmaf(sa[b * d + m], __fadd_rn(A.S[(long long)b * n_s + k], A.S1[(long long)b * n_s + k]), acc);
    Wg[j] = fresh_adam(Wg[j], tsfphi_clamp(acc, A.clamp), c1);
  }
  for (int o = tid; o < d; o += 256) {
    float acc = 0.f, accu = 0.f;
    for (int b = 0; b < B; ++b) {
      acc = __fadd_rn(acc, sb[b * d + o]);
      accu = __fadd_rn(accu, sa[b * d + o]);
    }
    bh[o] = fresh_adam(bh[o], tsfphi_clamp(__fmul_rn(2.f, acc), A.clamp), c1);
    bg[o] = fresh_adam(bg[o], tsfphi_clamp(__fmul_rn(2.f, accu), A.clamp), c1);
  }
}

}  // namespace sfx
