// sfx_pre.h -- pre-training of the reward features φ: sfdqn_phi.py PhiFunction (:90-123) and the
// minibatch update inside SFDQN.pre_train (:851-867; tsfdqn_phi.py:1087-1103 is the same).  Device side.
//
// One update of task t on B rows (x_b = s_b ⊕ float(a_b) ⊕ s1_b, n_in = 2 n_s + 1):
//   A_0 = x, A_{l+1} = relu(A_l W_lᵀ + b_l), φ = A_L W_Lᵀ + b_L, ŷ_b = w_t·φ_b, loss = mean_b (r_b - ŷ_b)²
//   dŷ_b = 2 (ŷ_b - r_b) / B, dw_t = Σ_b dŷ_b φ_b, dZ_L = dŷ ⊗ w_t, dZ_{l-1} = [A_l > 0] ⊙ (dZ_l W_l),
//   dW_l = dZ_lᵀ A_l, db_l = Σ_b dZ_l; one Adam step (adam_consts / adam_apply, sfx_kernels.h) on the net
//   with its persistent moments and step count, one on w_t with those of row t.
//
// The hazard: dZ_{l-1} reads W_l, so W_l may not be stepped before every dZ below it exists.  The launches are
// cut there, and the parameters are stepped in place (one slot):
//   k_pre_fwd   one workgroup, 16 waves.  The forward (every A_l kept), ŷ, the loss, dŷ and the whole dZ chain
//               -- every read of a weight by another layer's work happens here, before any step.  An update
//               launches a second workgroup that only computes the two AdamC and bumps the two step counts.
//   k_pre_step  one workgroup per 16-row tile of every W_l (its 4 waves take 64 columns each; the last one
//               sums the bias gradient) plus one for w_t: dW from the kept dZ_l and A_l, then Adam on the
//               tile's own rows.  It reads no weight but the ones it steps.
// The forward alone (TRAIN = false) is sfx_pre_features; k_pre_rows is the same forward, one workgroup per 16-row
// tile with the activations in LDS and no scratch of the handle (sfx_pre_features_rows, the runner's featurizer).
//
// Products run on v_mfma_f32_16x16x4_f32 with the operand layout of sfx_phiw.h: lane l supplies A[l & 15][l >> 4]
// and B[l >> 4][l & 15] and holds D[4 (l >> 4) + r][l & 15].  A wave owns whole output tiles and walks the
// reduction index alone, or shares it with other waves in slices fixed by the layer's geometry whose partial tiles
// meet in LDS in slice order; an output element's operation sequence depends on its own row and column only: row b
// of a B-row forward equals the one-row forward bit for bit, and two runs give the same bits.  No atomics.
// Internally every row of W_l and A_l is padded to a multiple of 4 floats (pads zero, never stepped), so all
// operand loads of the forward are aligned dwordx4 whatever n_in is.
#pragma once

namespace sfx {

constexpr int PRE_IN = 64, PRE_HID = 256, PRE_D = 64, PRE_B = 64;
constexpr int PRE_NL = 5;      // Linear layers: up to 4 hidden + the output layer
constexpr int PRE_WAVES = 16;  // k_pre_fwd's workgroup

struct PreGeo {
  int n_s, n_in, d, T, NL, Mmax, dp, ntile;
  int K[PRE_NL], Kp[PRE_NL], N[PRE_NL];
  int offW[PRE_NL], offB[PRE_NL];  // into p / m / v: W_l [N][Kp], b_l [N]
  int offA[PRE_NL];                // into act: A_l [Mmax][Kp_l], the input of Linear l
  int offZ[PRE_NL];                // into dz: dZ_l [Mmax][N_l], the gradient at Linear l's output
  int offZt[PRE_NL];               // into dzt: the same dZ_l transposed, [N_l][PRE_B], for the dZ chain's reads
  int tile0[PRE_NL + 1];           // k_pre_step: first workgroup of layer l
};

struct PreArgs {
  PreGeo G;
  float *p, *m, *v;    // the φ net and its Adam moments, padded layout
  float *w, *wm, *wv;  // [T][dp] reward rows and their moments
  int* step;           // [1 + T]: the net's Adam step count, then each row's
  AdamC* adamc;        // [2]: this update's constants for the net and for row `task`
  float *act, *dz, *dzt;
  float* phi;          // [Mmax][d] φ of the update's rows
  float* dy;           // [Mmax] dŷ
  const float *S, *S1, *r;
  const int64_t* a;
  float* out;          // update: the loss scalar; features: φ [B][d]
  int B, task;
  AdamHP hp_phi, hp_w;
};

__device__ __forceinline__ float4 pre_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// A layer has at most 16 output tiles (widths <= 256) and the workgroup 16 waves: wave -> (tile, slice), the
// slices of a tile splitting the reduction index.  S depends on the layer's geometry only, never on B, so an
// element's operation sequence is the same in every call.  Slices >= 1 park their partial tiles in LDS (at most
// PRE_SLOTS of them), slice 0 adds them in slice order and writes the tile.
constexpr int PRE_SLOTS = 8;
__device__ __forceinline__ int pre_slices(int ntile, int trips) {
  return max(1, min(min(PRE_WAVES / ntile, 1 + PRE_SLOTS / ntile), trips));
}

template <int MT>
__device__ __forceinline__ void pre_fold(floatx4 (&acc)[MT], float (*red)[MT * 4][64], int S, int tile, int slice,
                                         bool active, int lane) {
  if (S == 1) return;  // uniform over the workgroup
  if (active && slice > 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[tile * (S - 1) + slice - 1][t * 4 + r][lane] = acc[t][r];
  }
  __syncthreads();
  if (active && slice == 0) {
    for (int q = 1; q < S; ++q)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = __fadd_rn(acc[t][r], red[tile * (S - 1) + q - 1][t * 4 + r][lane]);
  }
  __syncthreads();  // red is free for the next layer
}

// Y[b][o] = act(Σ_k X[b][k] W[o][k] + bias[o]) for o < N; columns N .. ycols - 1 (the row pad) are written as zero.
// xs / ys: the row strides of X and Y in floats (multiples of 4); X and Y may live in global memory or in LDS.
template <int MT>
__device__ __forceinline__ void pre_fwd_layer(const float* W, const float* bias, const float* X, int xs, float* Y,
                                              int ys, int ycols, int Kp, int N, int B, bool relu, int wave, int lane,
                                              float (*red)[MT * 4][64]) {
  constexpr int CH = MT <= 2 ? 4 : 2;  // chunks of 16 k per trip: every load of a trip issued before its first use
  const int g = lane >> 4, c = lane & 15;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int ntile = (ycols + 15) >> 4, S = pre_slices(ntile, (Kp + 31) >> 5);
  const int ct = wave / S, slice = wave - ct * S;
  const bool active = ct < ntile;
  const int kq = (((Kp + 15) >> 4) + S - 1) / S * 16;  // a slice's k range, a multiple of 16 (Kp: one of 4)
  const int kbeg = slice * kq, kend = min(Kp, kbeg + kq);
  const int o = ct * 16 + c;
  const float* wrow = W + (long long)min(o, N - 1) * Kp;
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    for (int kb = kbeg; kb < kend; kb += 16 * CH) {
      float4 a[CH], x[CH][MT];
#pragma unroll
      for (int u = 0; u < CH; ++u) {
        const int k = kb + 16 * u + 4 * g;
        a[u] = (o < N && k < kend) ? pre_ld4(wrow + k) : z4;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int b = 16 * t + c;
          x[u][t] = (b < B && k < kend) ? pre_ld4(X + (long long)b * xs + k) : z4;
        }
      }
#pragma unroll
      for (int u = 0; u < CH; ++u)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          acc[t] = mfma4(a[u].x, x[u][t].x, acc[t]);
          acc[t] = mfma4(a[u].y, x[u][t].y, acc[t]);
          acc[t] = mfma4(a[u].z, x[u][t].z, acc[t]);
          acc[t] = mfma4(a[u].w, x[u][t].w, acc[t]);
        }
    }
  }
  pre_fold<MT>(acc, red, S, ct, slice, active, lane);
  if (active && slice == 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oo = ct * 16 + 4 * g + r, b = 16 * t + c;
        if (b < B && oo < ycols) {
          float v = 0.f;
          if (oo < N) {
            v = __fadd_rn(acc[t][r], bias[oo]);
            if (relu) v = fmaxf(v, 0.f);
          }
          Y[(long long)b * ys + oo] = v;
        }
      }
  }
}

// GX[b][k] = [X[b][k] > 0] Σ_o G[b][o] W[o][k]: X [B][Kp] the layer's input (the ReLU output of the layer below).
// G is read from its transposed copy Gt [N][PRE_B] -- a lane group's 16 rows b are one 64-byte run there, and 16
// different cache lines in the row-major dZ that k_pre_step reads (measured: 40 of the launch's 68 µs) -- and
// GX is written both ways (GXt null for dZ_0, which no chain reads).
template <int MT>
__device__ __forceinline__ void pre_dx_layer(const float* W, const float* Gt, const float* X, float* GX, float* GXt,
                                             int K, int Kp, int N, int B, int wave, int lane,
                                             float (*red)[MT * 4][64]) {
  const int g = lane >> 4, c = lane & 15;
  const int ntile = (K + 15) >> 4, S = pre_slices(ntile, (N + 31) >> 5);
  const int ct = wave / S, slice = wave - ct * S;
  const bool active = ct < ntile;
  const int oq = (((N + 3) >> 2) + S - 1) / S * 4;  // a slice's o range, a multiple of 4
  const int obeg = slice * oq, oend = min(N, obeg + oq);
  const int k = ct * 16 + c;
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    // 8 groups of 4 rows of W per trip, every load of a trip issued before its first use
    for (int ob = obeg; ob < oend; ob += 32) {
      float a[8], gv[8][MT];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int o = ob + 4 * u + g;
        const bool in = o < oend;
        a[u] = (in && k < K) ? W[(long long)o * Kp + k] : 0.f;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int b = 16 * t + c;
          gv[u][t] = (in && b < B) ? Gt[o * PRE_B + b] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = mfma4(a[u], gv[u][t], acc[t]);
    }
  }
  pre_fold<MT>(acc, red, S, ct, slice, active, lane);
  if (active && slice == 0) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = ct * 16 + 4 * g + r, b = 16 * t + c;
        if (kk < K && b < B) {
          const float v = X[(long long)b * Kp + kk] > 0.f ? acc[t][r] : 0.f;
          GX[(long long)b * K + kk] = v;
          if (GXt) GXt[kk * PRE_B + b] = v;
        }
      }
  }
}

template <int MT, bool TRAIN>
__global__ __launch_bounds__(64 * PRE_WAVES) void k_pre_fwd(PreArgs A) {
  __shared__ float s_sq[PRE_B], s_dy[PRE_B];
  __shared__ float red[PRE_SLOTS][MT * 4][64];
  const PreGeo& G = A.G;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, B = A.B, NL = G.NL, d = G.d;
  if (TRAIN && blockIdx.x == 1) {
    // The update's second workgroup: the Adam constants (four double-precision pow) and the step counts, off
    // the forward's critical path.  Both steps use this update's gradients; every other row's count stays.
    if (tid < 2) {
      const int i = tid ? 1 + A.task : 0, st = A.step[i] + 1;
      A.adamc[tid] = adam_consts(tid ? A.hp_w : A.hp_phi, st);
      A.step[i] = st;
    }
    return;
  }
  {
    float* x0 = A.act + G.offA[0];
    const int Kp0 = G.Kp[0], n_s = G.n_s;
    for (int j = tid; j < B * Kp0; j += 64 * PRE_WAVES) {
      const int b = j / Kp0, k = j - b * Kp0;
      float v = 0.f;
      if (k < n_s) v = A.S[(long long)b * n_s + k];
      else if (k == n_s) v = (float)A.a[b];
      else if (k < G.n_in) v = A.S1[(long long)b * n_s + (k - n_s - 1)];
      x0[j] = v;
    }
  }
  __syncthreads();
  for (int l = 0; l < NL; ++l) {
    const bool last = l == NL - 1;
    float* Y = last ? (TRAIN ? A.phi : A.out) : A.act + G.offA[l + 1];
    const int ys = last ? d : G.Kp[l + 1];
    pre_fwd_layer<MT>(A.p + G.offW[l], A.p + G.offB[l], A.act + G.offA[l], G.Kp[l], Y, ys, ys, G.Kp[l], G.N[l], B, !last,
                      wave, lane, red);
    __syncthreads();
  }
  if constexpr (TRAIN) {
    const float* w = A.w + (long long)A.task * G.dp;
    float* dzL = A.dz + G.offZ[NL - 1];
    if (tid < B) {
      float yh = 0.f;
      for (int j = 0; j < d; ++j) yh = __builtin_fmaf(w[j], A.phi[(long long)tid * d + j], yh);
      const float diff = __fsub_rn(yh, A.r[tid]);
      const float dy = __fmul_rn(__fdiv_rn(2.f, (float)B), diff);
      A.dy[tid] = dy;
      s_dy[tid] = dy;
      s_sq[tid] = __fmul_rn(diff, diff);
    }
    __syncthreads();
    for (int j = tid; j < B * d; j += 64 * PRE_WAVES) {
      const int b = j / d;
      const float v = __fmul_rn(s_dy[b], w[j - b * d]);
      dzL[j] = v;
      A.dzt[G.offZt[NL - 1] + (j - b * d) * PRE_B + b] = v;
    }
    __syncthreads();  // dZ_L is complete before the chain reads it
    if (tid == 0) {
      float s = 0.f;
      for (int b = 0; b < B; ++b) s = __fadd_rn(s, s_sq[b]);
      *A.out = __fdiv_rn(s, (float)B);
    }
    for (int l = NL - 1; l >= 1; --l) {
      pre_dx_layer<MT>(A.p + G.offW[l], A.dzt + G.offZt[l], A.act + G.offA[l], A.dz + G.offZ[l - 1],
                       l > 1 ? A.dzt + G.offZt[l - 1] : nullptr, G.K[l], G.Kp[l], G.N[l], B, wave, lane, red);
      __syncthreads();
    }
  }
}

// The forward alone on M rows, one workgroup per 16-row tile, every activation of the tile in LDS (two buffers,
// ping-pong between layers): it reads the net's parameters and the rows' (s, a, s1) and writes φ, nothing else --
// no handle scratch, so it may run on any stream, also inside another handle's captured graph, and M is not
// bounded by max_batch.  Each layer is pre_fwd_layer<1> itself (same MFMA, operand layout, pre_slices split and
// fold order), so row b of an M-row call equals sfx_pre_features of that row at B = 1 bit for bit.
//
// LDS row stride: lane (c = l & 15, g = l >> 4) reads row c at k + 4 g as one ds_read_b128, whose 16-lane groups
// hold 8 rows at one g and 8 at g + 1 (banks: dword address mod 64, 4 per lane).  A stride of Kp = 64 / 128 / 256
// floats puts the 8 rows of one g on the same 4 banks (8-way); stride / 4 ≡ 2 (mod 4) spreads one g over the even
// 16-byte slots and the other over the odd ones: conflict-free.  PRE_LS = 264 is that for every Kp <= 256.
constexpr int PRE_LS = 264;
constexpr int PRE_ROWS_MAX = 65536;  // sfx_pre_features_rows' M limit (4096 workgroups)

struct PreRowsArgs {
  PreGeo G;
  const float* p;
  const float *S, *S1;
  const int64_t* a;
  float* phi;         // [M][d]
  int M;
  const int* cancel;  // runner steps: the gate's cancel word (a cancelled step writes nothing); null otherwise
};

__global__ __launch_bounds__(64 * PRE_WAVES) void k_pre_rows(PreRowsArgs A) {
  __shared__ __attribute__((aligned(16))) float xa[2][16 * PRE_LS];
  __shared__ float red[PRE_SLOTS][4][64];
  if (A.cancel && step_cancelled(A.cancel)) return;  // uniform over the grid
  const PreGeo& G = A.G;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, NL = G.NL, d = G.d;
  const long long row0 = 16LL * blockIdx.x;
  const int B = (int)min(16LL, (long long)A.M - row0);
  {
    const int Kp0 = G.Kp[0], n_s = G.n_s;
    for (int j = tid; j < B * Kp0; j += 64 * PRE_WAVES) {
      const int b = j / Kp0, k = j - b * Kp0;
      float v = 0.f;
      if (k < n_s) v = A.S[(row0 + b) * n_s + k];
      else if (k == n_s) v = (float)A.a[row0 + b];
      else if (k < G.n_in) v = A.S1[(row0 + b) * n_s + (k - n_s - 1)];
      xa[0][b * PRE_LS + k] = v;
    }
  }
  __syncthreads();
  // hidden layers LDS -> LDS, the output layer LDS -> global: two call sites, so every access keeps its address space
  for (int l = 0; l < NL - 1; ++l) {
    pre_fwd_layer<1>(A.p + G.offW[l], A.p + G.offB[l], xa[l & 1], PRE_LS, xa[(l + 1) & 1], PRE_LS, G.Kp[l + 1], G.Kp[l],
                     G.N[l], B, true, wave, lane, red);
    __syncthreads();
  }
  const int l = NL - 1;
  pre_fwd_layer<1>(A.p + G.offW[l], A.p + G.offB[l], xa[l & 1], PRE_LS, A.phi + row0 * d, d, d, G.Kp[l], G.N[l], B, false,
                   wave, lane, red);
}

template <int MT>
__global__ __launch_bounds__(256) void k_pre_step(PreArgs A) {
  const PreGeo& G = A.G;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15, B = A.B;
  const int blk = blockIdx.x;
  if (blk >= G.ntile) {  // the reward row of the task
    const int d = G.d;
    if (tid < d) {
      float gw = 0.f;
      for (int b = 0; b < B; ++b) gw = __builtin_fmaf(A.dy[b], A.phi[(long long)b * d + tid], gw);
      const long long j = (long long)A.task * G.dp + tid;
      adam_el(A.w + j, A.wm + j, A.wv + j, gw, A.adamc[1]);
    }
    return;
  }
  int l = 0;
  while (l + 1 < G.NL && blk >= G.tile0[l + 1]) ++l;
  const int K = G.K[l], Kp = G.Kp[l], N = G.N[l];
  const int o0 = (blk - G.tile0[l]) * 16, k0 = wave * 64;
  const float* __restrict__ Gz = A.dz + G.offZ[l];
  const float* __restrict__ X = A.act + G.offA[l];
  const AdamC ac = A.adamc[0];
  if (k0 < K) {
    // every load of the tile's B <= 16 MT rows issued before the first MFMA
    float a[4 * MT], x[4 * MT][4];
#pragma unroll
    for (int q = 0; q < 4 * MT; ++q) {
      const int b = 4 * q + g;
      a[q] = (b < B && o0 + c < N) ? Gz[(long long)b * N + o0 + c] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 16 * e + c;
        x[q][e] = (b < B && k < K) ? X[(long long)b * Kp + k] : 0.f;
      }
    }
    // the tile's parameters and moments too: loads behind the epilogue's stores could not be hoisted
    float pw[4][4], pm[4][4], pv[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + 4 * g + r, k = k0 + 16 * e + c;
        const bool in = o < N && k < K;
        const long long j = G.offW[l] + (long long)min(o, N - 1) * Kp + min(k, K - 1);
        pw[e][r] = in ? A.p[j] : 0.f;
        pm[e][r] = in ? A.m[j] : 0.f;
        pv[e][r] = in ? A.v[j] : 0.f;
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
          const long long j = G.offW[l] + (long long)o * Kp + k;
          adam_apply(pw[e][r], pm[e][r], pv[e][r], acc[e][r], ac);
          A.p[j] = pw[e][r];
          A.m[j] = pm[e][r];
          A.v[j] = pv[e][r];
        }
      }
  }
  if (wave == 3 && lane < 16 && o0 + lane < N) {
    const int o = o0 + lane;
    float gb = 0.f;
    for (int b = 0; b < B; ++b) gb = __fadd_rn(gb, Gz[(long long)b * N + o]);
    const long long j = G.offB[l] + o;
    adam_el(A.p + j, A.m + j, A.v + j, gb, ac);
  }
}

}  // namespace sfx
