// distill.hip, part 2a: one net's exact-f32 forward on a 16-env tile and what it needs -- the SrcC
// fence of a group of four f32 MFMAs, tanh4, the cross-lane sums, the store helpers, load_net and
// mlp_forward.  Included by distill_forward.h, and by teacher_f32.h for the teacher inside the two
// students' evaluation and envs kernels (one definition, three translation units).  Expects
// distill_layout.h, rd_device.h's f32x4, mfma, ld4, kTanhScale, tanh_pre, and kFenceAll (true
// only in distill.hip's -DRD_MFMA_SRCC_FENCE diagnostic build).
#pragma once

template <bool FENCE>
__device__ __forceinline__ void fence_begin(f32x4 (&acc)[4]) {   // the group's MFMAs read acc: they follow
    if constexpr (FENCE || kFenceAll)
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])::"memory");
}
template <bool FENCE>
__device__ __forceinline__ void fence_end(f32x4 (&acc)[4]) {   // every MFMA of the group precedes it
    if constexpr (FENCE || kFenceAll) {
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) acc[fb][3] = __builtin_amdgcn_fmed3f(acc[fb][3], acc[fb][3], acc[fb][3]);
        asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3])::"memory");
    }
}

// rd::tanh_pre on the four rows of an accumulator (the forward images carry kTanhScale; the backward
// needs only tanh's output, W2^T for dH1 keeps the unscaled weights), as scalar VALU.  No packed-f32 forms: a
// v_pk_add/fma_f32 whose sources a later load overwrites before anything reads its result can
// lose lanes 48-63 (PKWAR), and in an MFMA gap a packed op costs more issue than
// the two scalar ones (MI355X_MICROARCH.md: +22 cycles for v_pk_fma_f32).  The rollout kernels
// contain no v_pk_*_f32 at all (tests/test_product_hygiene.py).
__device__ __forceinline__ f32x4 tanh4(f32x4 y) {
    return f32x4{tanh_pre(y[0]), tanh_pre(y[1]), tanh_pre(y[2]), tanh_pre(y[3])};
}

// x + x from the partner row (lane ^ 16) / half (lane ^ 32): v_permlane16/32_swap (VALU,
// no LDS round trip).  Every lane gets the bitwise-identical sum.
__device__ __forceinline__ float xsum16(float x) {
    const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(p[0]) + __uint_as_float(p[1]);
}
__device__ __forceinline__ float xsum32(float x) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(p[0]) + __uint_as_float(p[1]);
}

// (a + b) + (c + d) per component as scalar adds (a vector add would be v_pk_add_f32)
__device__ __forceinline__ f32x4 sum4(f32x4 a, f32x4 b, f32x4 c, f32x4 d) {
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (a[i] + b[i]) + (c[i] + d[i]);
    return r;
}

// Global stores, plain or non-temporal (NT).  The bf16-student kernels (c5) write the rollout's
// partial row NT (__builtin_nontemporal_store): the rows no longer wait dirty in the writer's L2
// for the end-of-kernel writeback, c5 -0.5 us per step; the f32-student kernels keep plain stores
// (neutral at c4, -0.25 us at c3, +0.25 at c2's 64 workgroups; DESIGN.md §3,
// profiles/r03k_nt_stores.txt, profiles/r03y_sched_nt.txt).  An inline-asm NT store that chose per
// launch made the first rollout of a process differ in one gradient entry and is gone
// (profiles/r03x_nt_asm_rejected.txt; no wait-state pair explains it, profiles/r04_r03x_isa.txt).
// NT state, reduce+Adam and all-kernel row stores measured no gain
// (profiles/r04_removed_diagnostic_variants.diff).
template <bool NT, class T>
__device__ __forceinline__ void gst(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
template <class T>
__device__ __forceinline__ void put(T* p, T v) { *p = v; }

// global net = params[P] | mu[11] | sd[11]  ->  LDS image (+ W2^T if `transposed`); the
// forward images of W1, b1, W2, b2 carry the tanh scale (kTanhScale)
__device__ void load_net(float* L, const float* g, bool transposed, int nthreads) {
    const float* mu = g + P_TOT;
    const float* sd = g + P_TOT + OBD;
    for (int i = threadIdx.x; i < 12 * HID; i += nthreads) {
        const int k = i >> 6, f = i & 63;
        L[N_W1 + k * HID + (f & 15) * 4 + (f >> 4)] = kTanhScale * (k < OBD ? g[P_W1 + i] : g[P_B1 + f]);
    }
    for (int i = threadIdx.x; i < HID * HID; i += nthreads) {
        const int k = i >> 6, f = i & 63;
        L[N_W2 + k * HID + (f & 15) * 4 + (f >> 4)] = kTanhScale * g[P_W2 + i];
    }
    if (transposed)   // k fastest across lanes: the LDS writes spread over the banks
        for (int i = threadIdx.x; i < HID * HID; i += nthreads) {
            const int f = i >> 6, k = i & 63;
            L[N_W2T + f * HID + (k & 15) * 4 + (k >> 4)] = g[P_W2 + k * HID + f];
        }
    for (int i = threadIdx.x; i < HID; i += nthreads) L[N_B2 + i] = kTanhScale * g[P_B2 + i];
    for (int i = threadIdx.x; i < HID * ACD; i += nthreads) L[N_W3 + i] = g[P_W3 + i];
    if (threadIdx.x < ACD) {
        L[N_B3 + threadIdx.x] = g[P_B3 + threadIdx.x];
        L[N_LS + threadIdx.x] = g[P_LS + threadIdx.x];
    }
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;
        L[N_MU + k] = k < OBD ? mu[k] : 0.0f;
        L[N_RS + k] = k < OBD ? 1.0f / sd[k] : 1.0f;
    }
}

// MlpPolicy forward of the 16-env tile whose raw observations are rows ob[0..15] of the
// wave's obs scratch (row stride SOS, component 11 = 1).  Lane (j, g):
// H1, H2 = hidden activations, features 16 fb + 4 g + r of env j; (m0, m1) = action mean
// of env j (identical in the four k-groups).
template <bool FENCE = false>
__device__ __forceinline__ void mlp_forward(const float* L, const float* ob, int j, int g, f32x4 (&H1)[4],
                                            f32x4 (&H2)[4], float& m0, float& m1) {
    f32x4 acc[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // layer 1: K = 12 (11 filtered inputs + the bias input), k-step s covers inputs 4s+g
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        const float z = fminf(fmaxf((ob[j * SOS + k] - L[N_MU + k]) * L[N_RS + k], -5.0f), 5.0f);
        const f32x4 w = ld4(L + N_W1 + k * HID + 4 * j);
        fence_begin<FENCE>(acc);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) acc[fb] = mfma(w[fb], z, acc[fb]);
        fence_end<FENCE>(acc);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
        H1[fb] = tanh4(acc[fb]);
    // layer 2: K = 64; k-step (kb, r) uses features 16 kb + 4 g + r = this lane's H1[kb][r]
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = ld4(L + N_B2 + 16 * fb + 4 * g);
    // A operands prefetched one k-step ahead (LDS latency vs 4 MFMAs of 32 cycles)
    f32x4 wn = ld4(L + N_W2 + (4 * g) * HID + 4 * j);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 w = wn;
            if (kb * 4 + r < 15) {
                const int kn = (r == 3) ? 16 * (kb + 1) + 4 * g : 16 * kb + 4 * g + r + 1;
                wn = ld4(L + N_W2 + kn * HID + 4 * j);
            }
            fence_begin<FENCE>(acc);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) acc[fb] = mfma(w[fb], H1[kb][r], acc[fb]);
            fence_end<FENCE>(acc);
        }
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const f32x4 wa = ld4(L + N_W3 + (16 * fb + 4 * g) * 2);       // W3[f][0..1], f = 16fb+4g+0,1
        const f32x4 wb = ld4(L + N_W3 + (16 * fb + 4 * g) * 2 + 4);   // f = 16fb+4g+2,3
        H2[fb] = tanh4(acc[fb]);
        p0 = fmaf(H2[fb][0], wa[0], p0); p1 = fmaf(H2[fb][0], wa[1], p1);
        p0 = fmaf(H2[fb][1], wa[2], p0); p1 = fmaf(H2[fb][1], wa[3], p1);
        p0 = fmaf(H2[fb][2], wb[0], p0); p1 = fmaf(H2[fb][2], wb[1], p1);
        p0 = fmaf(H2[fb][3], wb[2], p0); p1 = fmaf(H2[fb][3], wb[3], p1);
    }
    p0 = xsum32(xsum16(p0));
    p1 = xsum32(xsum16(p1));
    m0 = p0 + L[N_B3];
    m1 = p1 + L[N_B3 + 1];
}
