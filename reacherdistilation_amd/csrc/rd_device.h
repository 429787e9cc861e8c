// Device primitives shared by the translation units (distill, student_mlp, student_lstm, ppo,
// rd_gemm, rd_xgmi): each exists once, here.  Everything is __device__ __forceinline__, so a
// kernel's ISA is what it was with a local copy (scripts/isa/same_isa.py is the gate).
#pragma once
#include <hip/hip_runtime.h>

namespace rd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x4_f32 (exact f32 products, 8 passes); see fence_begin for its SrcC hazard
__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Memory that is private to one wave (a per-wave LDS scratch): LDS instructions of one wave
// execute in issue order, so staging needs only a compiler-level barrier, not s_barrier.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tanh(z) = 1 - 2/(2^y + 1) with y = 2 log2(e) z: v_exp_f32 + v_add + v_rcp_f32 + v_fma.
// tanh_pre takes y (distill's forward weight images are pre-scaled by kTanhScale, so a layer's
// accumulator already is y); tanh_fast takes z.
constexpr float kTanhScale = 2.8853900817779268f;
__device__ __forceinline__ float tanh_pre(float y) {
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(y) + 1.0f), 1.0f);
}
__device__ __forceinline__ float tanh_fast(float z) { return tanh_pre(z * kTanhScale); }

// SrcC fence around a group of f32 MFMAs whose accumulators are G[0..Q): the accumulators pass
// through an empty asm before and after the group (so its MFMAs stay between them, and no load --
// the asm clobbers memory -- moves into the group), and each result is read by a VALU before the
// closing asm, so the compiler waits for every MFMA of the group to complete first.
// Needed wherever the compiler would otherwise issue a load into a register that an in-flight
// 8-pass v_mfma_f32_16x16x4_f32 still reads as SrcC: ROCm 7.2 protects that WAR for the XDL
// (bf16) MFMAs but emits such loads 0-9 wait states after the f32 form (it renames a chain's
// accumulators, D = v[20:23], C = v[22:25]), and a load returning there is lost for the lanes of
// the MFMA's last row group (rows 12-15 = lanes 48-63) while the MFMA still reads (DESIGN.md §3:
// found statically with scripts/isa/hazards.py class LDSRC, confirmed by
// profiles/r03_srcc_probe_*.txt).  The rollout has its own four-operand form (distill_forward.h).
template <int Q>
__device__ __forceinline__ void fence_begin(f32x4 (&G)[Q]) {
#pragma unroll
    for (int t = 0; t < Q; ++t) asm volatile("" : "+v"(G[t])::"memory");
}
template <int Q>
__device__ __forceinline__ void fence_end(f32x4 (&G)[Q]) {
#pragma unroll
    for (int t = 0; t < Q; ++t) G[t][3] = __builtin_amdgcn_fmed3f(G[t][3], G[t][3], G[t][3]);
#pragma unroll
    for (int t = 0; t < Q; ++t) asm volatile("" : "+v"(G[t])::"memory");
}

// TF1 ApplyAdam (training_ops.cc; mlp_train.py:73-80) of one parameter with gradient g, from the
// running powers b1p = beta1^t, b2p = beta2^t: alpha = adam_alpha(lr, b1p, b2p); m = adam_m(g, m, b1);
// v = adam_v(g, v, b2); w -= adam_delta(m, v, alpha, eps).  Values in, value out, so that every
// caller keeps its own loads, stores and their order: one function updating m, v, w through
// references changed the schedule of three of the four reduce kernels (scripts/isa/same_isa.py).
__device__ __forceinline__ float adam_alpha(float lr, float b1p, float b2p) {
    return lr * sqrtf(1.0f - b2p) / (1.0f - b1p);
}
__device__ __forceinline__ float adam_m(float g, float m, float b1) { return m + (g - m) * (1.0f - b1); }
__device__ __forceinline__ float adam_v(float g, float v, float b2) { return v + (g * g - v) * (1.0f - b2); }
__device__ __forceinline__ float adam_delta(float m, float v, float alpha, float eps) {
    return (m * alpha) / (sqrtf(v) + eps);
}

}  // namespace rd
