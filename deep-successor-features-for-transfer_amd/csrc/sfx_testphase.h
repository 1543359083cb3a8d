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

}  // namespace sfx
