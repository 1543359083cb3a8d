// sfx_phiw.h -- the wide φ net (hidden width 129..2048): main_tsfdqn_phi_torch.py's phi_model_lambda
// is Linear(2 n_s + 1, 2048) + ReLU, 3 × (Linear(2048, 2048) + ReLU), Linear(2048, d): 12.6 M fp32
// parameters, ≈50 MB, updated at B = 32.  The update is a weight-streaming problem: every pass
// reads each layer's W once, so the kernels are many-workgroup, one launch per layer and pass
// (sfx_phi.h's one-workgroup scalar loops serve hid <= 128 and stay as they are).
//
// All products run on v_mfma_f32_16x16x4_f32 (exact f32, an fmaf chain); lane l of a wave supplies
// A[i = l & 15][kk = l >> 4] and B[kk = l >> 4][j = l & 15] and holds D[i = 4 (l >> 4) + r][j = l & 15].
// Batch rows pad to 16-row tiles (MT of them, B <= 64), out-of-range rows / columns load as zero and
// are never stored.  X of a layer has row stride K, Y and G row stride N (acts [l][B][hid], φ [B][d]).
//
//   k_phiw_fwd  Y[b][o] = act(Σ_k X[b][k] W[o][k] + bias[o]).  One workgroup per 16 rows of W; its
//               16 waves split k, each lane loads 4 consecutive k of its row as one dwordx4 (the 4 MFMAs
//               of a load take k = base + 4 (l >> 4) + c, a fixed permutation of the k order); the
//               waves' partial tiles are summed through LDS in a fixed order.
//   k_phiw_dx   GX[b][k] = [X[b][k] > 0] Σ_o G[b][o] W[o][k], W before its update.  One workgroup per
//               16 columns of W (64-B runs of every row; the neighbouring workgroup takes the other half
//               of the line), its 16 waves split o, summed through LDS in a fixed order.
//   k_phiw_dw   dW[o][k] = Σ_b G[b][o] X[b][k], db[o] = Σ_b G[b][o], then the fresh-Adam step in the
//               epilogue (gradient clamped to [-1, 1] first when asked): a wave owns a 16 × 64 tile of W,
//               read and written once, 256-B runs per row.
// The kernels are latency bound, not byte bound (B <= 64 rows of work per weight): what counts is the
// number of waves with loads in flight, hence the 16-wave split (2048 waves on a 2048 × 2048 layer)
// and trips that issue all their loads before the first MFMA.
// No floating-point atomics and a fixed reduction order everywhere: two runs from the same state
// give the same bits.  Bytes per update at hid 2048, n_mid 3: forward P·4, dX (P - first layer)·4,
// dW 2·P·4 -- four passes over ≈50 MB.
// k_phiw_dw is the one kernel here that writes persistent state (W and the bias, in place): a runner step
// cancelled at its gate (PhiwLayer::cancel, step_cancelled in sfx_kernels.h) leaves before it loads anything.
#pragma once

namespace sfx {

constexpr int PHIW_HID = 2048;

struct PhiwLayer {
  float* W;        // [N][K], bias [N] right after
  const float* X;  // [B][K] the layer's input (post-activation output of the layer below)
  float* Y;        // forward: [B][N]
  const float* G;  // backward: [B][N] gradient at the layer's (pre-activation) output
  float* GX;       // dX: [B][K] gradient at the pre-activation output of the layer below
  int K, N, B, relu, clamp;
  AdamHP hp;
  const int* cancel;  // runner steps: 1 when the step's gate cancelled it (k_phiw_dw commits nothing)
};

__device__ __forceinline__ bool phiw_vec(const void* p, int stride, int n) {
  return ((unsigned long long)p & (unsigned long long)(4 * n - 1)) == 0 && (stride & (n - 1)) == 0;
}

// 4 consecutive floats of a row from k (k a multiple of 4), zero from K on
__device__ __forceinline__ float4 phiw_ld4(const float* row, int k, int K, bool vec) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (vec) {
    if (k < K) v = *reinterpret_cast<const float4*>(row + k);
  } else {
    if (k < K) v.x = row[k];
    if (k + 1 < K) v.y = row[k + 1];
    if (k + 2 < K) v.z = row[k + 2];
    if (k + 3 < K) v.w = row[k + 3];
  }
  return v;
}

// the layer-0 input s ⊕ a ⊕ s1, kept for dW
__global__ __launch_bounds__(256) void k_phiw_in(float* x, const float* S, const int64_t* a, const float* S1, int B,
                                                 int n_s) {
  const int n_in = 2 * n_s + 1;
  for (int j = blockIdx.x * 256 + threadIdx.x; j < B * n_in; j += gridDim.x * 256) {
    const int b = j / n_in, k = j - b * n_in;
    x[j] = k < n_s ? S[(long long)b * n_s + k] : (k == n_s ? (float)a[b] : S1[(long long)b * n_s + (k - n_s - 1)]);
  }
}

// The reduction of a forward / dX tile is split over the PHIW_S waves of a workgroup (each streams
// its share of W with every load of a trip in flight); their partial tiles meet in LDS in a fixed
// order: wave w + S/2 into wave w, then waves 0 .. S/2 - 1 summed in wave order by the epilogue.
constexpr int PHIW_S = 16;

template <int NT>
__device__ __forceinline__ void phiw_fold(floatx4 (&acc)[NT], float (*red)[NT * 4][64], int w, int l) {
  if (w >= PHIW_S / 2) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w - PHIW_S / 2][t * 4 + r][l] = acc[t][r];
  }
  __syncthreads();
  if (w < PHIW_S / 2) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] = __fadd_rn(acc[t][r], red[w][t * 4 + r][l]);
  }
  __syncthreads();
  if (w < PHIW_S / 2) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[w][t * 4 + r][l] = acc[t][r];
  }
  __syncthreads();
}

template <int NT>
__device__ __forceinline__ float phiw_sum(float (*red)[NT * 4][64], int tr, int ll) {
  float v = red[0][tr][ll];
#pragma unroll
  for (int q = 1; q < PHIW_S / 2; ++q) v = __fadd_rn(v, red[q][tr][ll]);
  return v;
}

template <int MT>
__global__ __launch_bounds__(64 * PHIW_S) void k_phiw_fwd(PhiwLayer A) {
  __shared__ float red[PHIW_S / 2][MT * 4][64];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int K = A.K, N = A.N, B = A.B;
  const int o = blockIdx.x * 16 + c;
  const bool vw = phiw_vec(A.W, K, 4), vx = phiw_vec(A.X, K, 4);
  const int kq = ((K + 16 * PHIW_S - 1) / (16 * PHIW_S)) * 16;  // a wave's k range, a multiple of 16
  const int kbeg = w * kq, kend = min(K, kbeg + kq);
  const float* wrow = A.W + (long long)min(o, N - 1) * K;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  // 4 chunks of 16 k per trip, every load of a trip issued before its first use
  for (int kb = kbeg; kb < kend; kb += 64) {
    float4 a[4], x[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = kb + 16 * u + 4 * g;
      a[u] = o < N ? phiw_ld4(wrow, k, kend, vw) : z4;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int b = 16 * t + c;
        x[u][t] = b < B ? phiw_ld4(A.X + (long long)b * K, k, kend, vx) : z4;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc[t] = mfma4(a[u].x, x[u][t].x, acc[t]);
        acc[t] = mfma4(a[u].y, x[u][t].y, acc[t]);
        acc[t] = mfma4(a[u].z, x[u][t].z, acc[t]);
        acc[t] = mfma4(a[u].w, x[u][t].w, acc[t]);
      }
  }
  phiw_fold<MT>(acc, red, w, l);
  const float* bias = A.W + (long long)N * K;
  for (int idx = tid; idx < MT * 4 * 64; idx += 64 * PHIW_S) {
    const int tr = idx >> 6, ll = idx & 63, t = tr >> 2, r = tr & 3;
    const int oo = blockIdx.x * 16 + 4 * (ll >> 4) + r, b = 16 * t + (ll & 15);
    if (oo < N && b < B) {
      float v = __fadd_rn(phiw_sum<MT>(red, tr, ll), bias[oo]);
      if (A.relu) v = fmaxf(v, 0.f);
      A.Y[(long long)b * N + oo] = v;
    }
  }
}

template <int MT>
__global__ __launch_bounds__(64 * PHIW_S) void k_phiw_dx(PhiwLayer A) {
  __shared__ float red[PHIW_S / 2][MT * 4][64];
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int K = A.K, N = A.N, B = A.B;
  const int k0 = blockIdx.x * 16, k = k0 + c;
  const int oq = ((N + 4 * PHIW_S - 1) / (4 * PHIW_S)) * 4;  // a wave's o range, a multiple of 4
  const int obeg = w * oq, oend = min(N, obeg + oq);
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  // 8 groups of 4 rows per trip, every load of a trip issued before its first use
  for (int ob = obeg; ob < oend; ob += 32) {
    float a[8], gv[8][MT];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int o = ob + 4 * u + g;
      const bool in = o < oend;
      a[u] = (in && k < K) ? A.W[(long long)o * K + k] : 0.f;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int b = 16 * t + c;
        gv[u][t] = (in && b < B) ? A.G[(long long)b * N + o] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t] = mfma4(a[u], gv[u][t], acc[t]);
  }
  phiw_fold<MT>(acc, red, w, l);
  for (int idx = tid; idx < MT * 4 * 64; idx += 64 * PHIW_S) {
    const int tr = idx >> 6, ll = idx & 63, t = tr >> 2, r = tr & 3;
    const int kk = k0 + 4 * (ll >> 4) + r, b = 16 * t + (ll & 15);
    if (kk < K && b < B) {
      const float v = phiw_sum<MT>(red, tr, ll);
      const long long j = (long long)b * K + kk;
      A.GX[j] = A.X[j] > 0.f ? v : 0.f;  // ReLU of the layer below
    }
  }
}

template <int MT>
__global__ __launch_bounds__(256) void k_phiw_dw(PhiwLayer A) {
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, g = l >> 4, c = l & 15;
  const int K = A.K, N = A.N, B = A.B;
  const int o0 = blockIdx.x * 16, k0 = (blockIdx.y * 4 + w) * 64;
  if (step_cancelled(A.cancel)) return;  // uniform: the tile's only output is the stepped W / bias
  const AdamC c1 = adam_consts(A.hp, 1);
  const float* __restrict__ G = A.G;
  const float* __restrict__ X = A.X;
  if (k0 < K) {
    float wv[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + 4 * g + r, k = k0 + 16 * e + c;
        wv[e][r] = (o < N && k < K) ? A.W[(long long)o * K + k] : 0.f;
      }
    // every load of the tile's B <= 16 MT rows issued before the first MFMA
    float a[4 * MT], x[4 * MT][4];
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q) {
      const int b = 4 * q + g;
      a[q] = (b < B && o0 + c < N) ? G[(long long)b * N + o0 + c] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 16 * e + c;
        x[q][e] = (b < B && k < K) ? X[(long long)b * K + k] : 0.f;
      }
    }
    floatx4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = mfma4(a[q], x[q][e], acc[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + 4 * g + r, k = k0 + 16 * e + c;
        if (o < N && k < K) {
          float gg = acc[e][r];
          if (A.clamp) gg = fminf(fmaxf(gg, -1.f), 1.f);
          A.W[(long long)o * K + k] = fresh_adam(wv[e][r], gg, c1);
        }
      }
  }
  if (blockIdx.y == 0 && tid < 16 && o0 + tid < N) {
    const int o = o0 + tid;
    float* bias = A.W + (long long)N * K;
    float gg = 0.f;
    for (int b = 0; b < B; ++b) gg = __fadd_rn(gg, G[(long long)b * N + o]);
    if (A.clamp) gg = fminf(fmaxf(gg, -1.f), 1.f);
    bias[o] = fresh_adam(bias[o], gg, c1);
  }
}

}  // namespace sfx
