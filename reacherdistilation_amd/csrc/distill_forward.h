// distill.hip, part 2 of 5: a net's forward on a 16-env tile -- exact f32 (load_net and mlp_forward
// in distill_forward_f32.h, which student_mlp.hip shares; mlp_forward_pair), f32 split into bf16 pieces (split1 ... mlp_forward_split), bf16 (load_net_bf16,
// mlp_forward_bf16) -- the image packers (pack_param, pack_net_kernel, copy_images) and the rollout's
// SrcC fences.  Expects distill_layout.h and rd_device.h's f32x4, mfma, ld4, kTanhScale, tanh_pre.
#pragma once

// SrcC fence around a group of four f32 MFMAs (FENCE): what it does and why it is needed is at
// rd::fence_begin (rd_device.h).  The consumer-side-env-step kernels (bf16 student) fence their
// teacher's f32 MFMAs; -DRD_MFMA_SRCC_FENCE fences every group (diagnostic builds).
// One asm with four operands, not rd::fence_begin<4>'s four asms: kPairFence (below) is tuned to
// the schedule this form yields.
#ifdef RD_MFMA_SRCC_FENCE
constexpr bool kFenceAll = true;
#else
constexpr bool kFenceAll = false;
#endif
#include "distill_forward_f32.h"

// Teacher and student forwards of one tile, interleaved layer by layer: 8 independent
// accumulator chains per layer, and one net's tanh can issue behind the other's MFMAs.
// Returns the student's hidden activations (needed by the backward) and both means.
// FENCE: every MFMA group SrcC-fenced; LAST: only layer 2's last k-step, whose results the
// tanh / W3 epilogue follows (hipcc hoists the W3 loads into that step's in-flight SrcC
// registers, hazards.py scan_ldsrc; layer 1's end is interlocked by its own tanh reads)
constexpr unsigned kPairFence = 0x8a00u;   // layer-2 k-steps 9, 11, 15 (below)
template <bool FENCE = false, unsigned FM = FENCE ? 0xffffu : 0u>
__device__ __forceinline__ void mlp_forward_pair(const float* LT, const float* LS, const float* ob, int j, int g,
                                                 f32x4 (&H1)[4], f32x4 (&H2)[4], float& mt0, float& mt1,
                                                 float& ms0, float& ms1) {
    f32x4 at[4], as[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) at[fb] = as[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        const float x = ob[j * SOS + k];
        const float zt = fminf(fmaxf((x - LT[N_MU + k]) * LT[N_RS + k], -5.0f), 5.0f);
        const float zs = fminf(fmaxf((x - LS[N_MU + k]) * LS[N_RS + k], -5.0f), 5.0f);
        const f32x4 wt = ld4(LT + N_W1 + k * HID + 4 * j);
        const f32x4 ws = ld4(LS + N_W1 + k * HID + 4 * j);
        fence_begin<FENCE>(at);
        fence_begin<FENCE>(as);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            at[fb] = mfma(wt[fb], zt, at[fb]);
            as[fb] = mfma(ws[fb], zs, as[fb]);
        }
        fence_end<FENCE>(at);
        fence_end<FENCE>(as);
    }
    f32x4 T1[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        T1[fb] = tanh4(at[fb]);
        H1[fb] = tanh4(as[fb]);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        at[fb] = ld4(LT + N_B2 + 16 * fb + 4 * g);
        as[fb] = ld4(LS + N_B2 + 16 * fb + 4 * g);
    }
    f32x4 wtn = ld4(LT + N_W2 + (4 * g) * HID + 4 * j);
    f32x4 wsn = ld4(LS + N_W2 + (4 * g) * HID + 4 * j);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const f32x4 wt = wtn, ws = wsn;
            if (kb * 4 + r < 15) {
                const int kn = (r == 3) ? 16 * (kb + 1) + 4 * g : 16 * kb + 4 * g + r + 1;
                wtn = ld4(LT + N_W2 + kn * HID + 4 * j);
                wsn = ld4(LS + N_W2 + kn * HID + 4 * j);
            }
            if (FENCE || ((FM >> (kb * 4 + r)) & 1u)) {
                fence_begin<true>(at);
                fence_begin<true>(as);
            }
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                at[fb] = mfma(wt[fb], T1[kb][r], at[fb]);
                as[fb] = mfma(ws[fb], H1[kb][r], as[fb]);
            }
            if (FENCE || ((FM >> (kb * 4 + r)) & 1u)) {
                fence_end<true>(at);
                fence_end<true>(as);
            }
        }
    float pt0 = 0.0f, pt1 = 0.0f, ps0 = 0.0f, ps1 = 0.0f;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const f32x4 ta = ld4(LT + N_W3 + (16 * fb + 4 * g) * 2), tb = ld4(LT + N_W3 + (16 * fb + 4 * g) * 2 + 4);
        const f32x4 sa = ld4(LS + N_W3 + (16 * fb + 4 * g) * 2), sb = ld4(LS + N_W3 + (16 * fb + 4 * g) * 2 + 4);
        f32x4 t2;
        t2 = tanh4(at[fb]);
        H2[fb] = tanh4(as[fb]);
        pt0 = fmaf(t2[0], ta[0], pt0); pt1 = fmaf(t2[0], ta[1], pt1);
        pt0 = fmaf(t2[1], ta[2], pt0); pt1 = fmaf(t2[1], ta[3], pt1);
        pt0 = fmaf(t2[2], tb[0], pt0); pt1 = fmaf(t2[2], tb[1], pt1);
        pt0 = fmaf(t2[3], tb[2], pt0); pt1 = fmaf(t2[3], tb[3], pt1);
        ps0 = fmaf(H2[fb][0], sa[0], ps0); ps1 = fmaf(H2[fb][0], sa[1], ps1);
        ps0 = fmaf(H2[fb][1], sa[2], ps0); ps1 = fmaf(H2[fb][1], sa[3], ps1);
        ps0 = fmaf(H2[fb][2], sb[0], ps0); ps1 = fmaf(H2[fb][2], sb[1], ps1);
        ps0 = fmaf(H2[fb][3], sb[2], ps0); ps1 = fmaf(H2[fb][3], sb[3], ps1);
    }
    mt0 = xsum32(xsum16(pt0)) + LT[N_B3];
    mt1 = xsum32(xsum16(pt1)) + LT[N_B3 + 1];
    ms0 = xsum32(xsum16(ps0)) + LS[N_B3];
    ms1 = xsum32(xsum16(ps1)) + LS[N_B3 + 1];
}

// ---------------------------------------------------------------- bf16 student (RDD_DTYPE_BF16)
// v_mfma_f32_16x16x32_bf16 (lane l: A[row l&15][k 8(l>>4)+jj], B[k 8(l>>4)+jj][col l&15],
// jj = 0..7) for the layers and dH1, v_mfma_f32_16x16x16_bf16 (k = 4(l>>4)+jj, jj = 0..3)
// where K is the tile's 16 envs (dW2, dW1).  C/D layout as the f32 forms.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma_k32(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_k16(s16x4 a, s16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ unsigned short bf16_bits(float x) { return __builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }
__device__ __forceinline__ s16x4 pack4(float a, float b, float c, float d) {
    return s16x4{(short)bf16_bits(a), (short)bf16_bits(b), (short)bf16_bits(c), (short)bf16_bits(d)};
}
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
    return bf16x8{(__bf16)lo[0], (__bf16)lo[1], (__bf16)lo[2], (__bf16)lo[3],
                  (__bf16)hi[0], (__bf16)hi[1], (__bf16)hi[2], (__bf16)hi[3]};
}
__device__ __forceinline__ bf16x8 ldbf8(const float* base, int half) {
    return *reinterpret_cast<const bf16x8*>(reinterpret_cast<const unsigned short*>(base) + half);
}

__device__ __forceinline__ int kperm(int s, int g, int jj) { return 32 * s + 4 * g + (jj & 3) + 16 * (jj >> 2); }

__device__ void load_net_bf16(float* L, const float* g, int nthreads) {
    unsigned short* w1 = reinterpret_cast<unsigned short*>(L + NB_W1);
    unsigned short* w2f = reinterpret_cast<unsigned short*>(L + NB_W2F);
    unsigned short* w2b = reinterpret_cast<unsigned short*>(L + NB_W2B);
    for (int x = threadIdx.x; x < 4 * 4 * 16 * 8; x += nthreads) {
        const int jj = x & 7, i = (x >> 3) & 15, fb = (x >> 7) & 3, gg = x >> 9;
        const int k = 8 * gg + jj;
        w1[x] = bf16_bits(k < OBD ? g[P_W1 + k * HID + 16 * fb + i] : 0.0f);
    }
    for (int x = threadIdx.x; x < 2 * 4 * 4 * 16 * 8; x += nthreads) {
        const int jj = x & 7, i = (x >> 3) & 15, b = (x >> 7) & 3, gg = (x >> 9) & 3, s = x >> 11;
        const int kp = kperm(s, gg, jj);
        w2f[x] = bf16_bits(g[P_W2 + kp * HID + 16 * b + i]);
        w2b[x] = bf16_bits(g[P_W2 + (16 * b + i) * HID + kp]);
    }
    for (int x = threadIdx.x; x < HID; x += nthreads) {
        L[NB_B1 + x] = g[P_B1 + x];
        L[NB_B2 + x] = g[P_B2 + x];
    }
    for (int x = threadIdx.x; x < HID * ACD; x += nthreads) L[NB_W3 + x] = bf16_round(g[P_W3 + x]);
    if (threadIdx.x < ACD) {
        L[NB_B3 + threadIdx.x] = g[P_B3 + threadIdx.x];
        L[NB_LS + threadIdx.x] = g[P_LS + threadIdx.x];
    }
    if (threadIdx.x < 12) {
        const int k = threadIdx.x;
        L[NB_MU + k] = k < OBD ? g[P_TOT + k] : 0.0f;
        L[NB_RS + k] = k < OBD ? 1.0f / g[P_TOT + OBD + k] : 1.0f;
    }
}

// ---------------------------------------------------------------- f32 on bf16 MFMAs (split images)
// gfx950 runs f32 MFMAs at 1/16 of the bf16 rate, and beside them VALU work serialises on
// the SIMD's issue.  With rdd_config.f32_split the hidden-layer products
// (K = 64: both nets' layer 2 and the student's dH1 = W2 dZ2) run as f32 EMULATED on
// v_mfma_f32_16x16x32_bf16: each operand is split exactly into three bf16 pieces
//   x = x0 + x1 + x2,  x0 = x truncated to bf16, x1 = (x - x0) truncated, x2 = the rest,
// (x2 has at most 8 significant bits, so the split loses nothing) and a K = 32 step sums
// the six partial products of order >= 2^-16 (x2y0, x1y1, x0y2, x1y0, x0y1, x0y0, smallest
// first), each exact in the MFMA, into the f32 accumulator.  The dropped terms are below
// 2^-24 of |x||y|: f32 accuracy (scripts/micro/split_layer.hip: max error 1.5e-7 of
// sum|terms| vs 1.3e-7 for the exact f32 MFMA form; 1.54x its throughput).  Weight pieces
// are prepacked (pack_param); activation pieces are made per tile (split8).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void split1(float x, unsigned short (&h)[3]) {
    const uint32_t u = __float_as_uint(x);
    const float r = x - __uint_as_float(u & 0xffff0000u);
    const uint32_t ur = __float_as_uint(r);
    const float l = r - __uint_as_float(ur & 0xffff0000u);
    h[0] = (unsigned short)(u >> 16);
    h[1] = (unsigned short)(ur >> 16);
    h[2] = (unsigned short)(__float_as_uint(l) >> 16);
}

// split1's arithmetic as bit patterns whose high halves are the three pieces
__device__ __forceinline__ void split_bits(float x, uint32_t& u0, uint32_t& u1, uint32_t& u2) {
    u0 = __float_as_uint(x);
    const float r = x - __uint_as_float(u0 & 0xffff0000u);
    u1 = __float_as_uint(r);
    u2 = __float_as_uint(r - __uint_as_float(u1 & 0xffff0000u));
}

// lo = features k-slots jj 0..3, hi = jj 4..7 (the B operand order of the permuted images)
__device__ __forceinline__ void split8(f32x4 lo, f32x4 hi, bf16x8 (&p)[3]) {
    const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    uint32_t u0[8], u1[8], u2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) split_bits(x[i], u0[i], u1[i], u2[i]);   // scalar: no packed-f32 ops
    u32x4 q0, q1, q2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // high halves of two words -> one packed pair
        q0[i] = __builtin_amdgcn_perm(u0[2 * i + 1], u0[2 * i], 0x07060302u);
        q1[i] = __builtin_amdgcn_perm(u1[2 * i + 1], u1[2 * i], 0x07060302u);
        q2[i] = __builtin_amdgcn_perm(u2[2 * i + 1], u2[2 * i], 0x07060302u);
    }
    p[0] = __builtin_bit_cast(bf16x8, q0);
    p[1] = __builtin_bit_cast(bf16x8, q1);
    p[2] = __builtin_bit_cast(bf16x8, q2);
}

// one bf16 pair (lo = high half of a, hi = high half of b)
__device__ __forceinline__ uint32_t pair_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// acc += W . X over one K = 32 step from split pieces w[3] (A) and x[3] (B)
__device__ __forceinline__ f32x4 mfma_split(const bf16x8 (&w)[3], const bf16x8 (&x)[3], f32x4 c) {
    c = mfma_k32(w[2], x[0], c);
    c = mfma_k32(w[1], x[1], c);
    c = mfma_k32(w[0], x[2], c);
    c = mfma_k32(w[1], x[0], c);
    c = mfma_k32(w[0], x[1], c);
    return mfma_k32(w[0], x[0], c);
}

// dW2 += H1^T dZ2 over a tile's 16 envs as f32 emulated on v_mfma_f32_32x32x16_bf16 (f32_split, f32
// student): K = the tile's 16 envs (lane half h = lane >> 5 carries envs 8h .. 8h + 7), the 64 x 64
// gradient as 2 x 2 blocks of 32 x 32 (C/D: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 h).
// x[mb][e] = H1[32 mb + (lane & 31)][env 8h + e], y[nb][e] = dZ2[32 nb + (lane & 31)][env 8h + e],
// each split into its three bf16 pieces (split8); per block the six products of order >= 2^-16,
// smallest first (mfma_split): 24 MFMAs of 32 cycles that hold the SIMD's VALU issue for 8 each,
// where the round-5 16x16x32 form took 48 of 16 holding it for 8 (c4 75.2 -> 74.3 us per step,
// c3 28.1 -> 27.8, profiles/r06p_dw2_32x32_ab.jsonl) --
// half the held issue for the same MFMA time, and 17 % fewer VALU (no piece re-pairing).
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x16 mfma_32k16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ void dw2_split32(const float (&x)[2][8], const float (&y)[2][8], f32x16 (&g)[2][2]) {
    bf16x8 xp[2][3], yp[2][3];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        split8(f32x4{x[b][0], x[b][1], x[b][2], x[b][3]}, f32x4{x[b][4], x[b][5], x[b][6], x[b][7]}, xp[b]);
        split8(f32x4{y[b][0], y[b][1], y[b][2], y[b][3]}, f32x4{y[b][4], y[b][5], y[b][6], y[b][7]}, yp[b]);
    }
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x16 c = g[mb][nb];
            c = mfma_32k16(xp[mb][2], yp[nb][0], c);
            c = mfma_32k16(xp[mb][1], yp[nb][1], c);
            c = mfma_32k16(xp[mb][0], yp[nb][2], c);
            c = mfma_32k16(xp[mb][1], yp[nb][0], c);
            c = mfma_32k16(xp[mb][0], yp[nb][1], c);
            g[mb][nb] = mfma_32k16(xp[mb][0], yp[nb][0], c);
        }
}

__device__ __forceinline__ void ld_pieces(const float* L, int base, int o, bf16x8 (&w)[3]) {
    const unsigned short* h = reinterpret_cast<const unsigned short*>(L + base);
#pragma unroll
    for (int q = 0; q < 3; ++q) w[q] = *reinterpret_cast<const bf16x8*>(h + q * SP_PIECE + o);
}

// Layer 1 of a split image's net on v_mfma_f32_16x16x32_bf16 (f32 emulated by three-piece splits):
// lane group g's inputs 4s + g (s < 3; input 11 is the bias input 1) as three pieces each, a
// K = 32 step carrying two pieces of each input (slots 2s, 2s + 1), the six products of order
// >= 2^-16 in three MFMAs per output block: w0z2 + w2z0, w0z1 + w1z1, w0z0 + w1z0.  12 bf16
// MFMAs instead of 12 f32 ones, which hold the SIMD's VALU issue for 32 cycles each and read
// their SrcC for 8 passes (the hazard the consumer-side-step kernels had to fence).
__device__ __forceinline__ void layer1_split(const float* L, const float* ob, int j, int g, f32x4 (&acc)[4]) {
    u32x4 b[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int k = 4 * s + g;
        const float z = fminf(fmaxf((ob[j * SOS + k] - L[NX_MU + k]) * L[NX_RS + k], -5.0f), 5.0f);
        uint32_t z0, z1, z2;
        split_bits(z, z0, z1, z2);
        b[0][s] = pair_hi(z2, z0);
        b[1][s] = pair_hi(z1, z1);
        b[2][s] = pair_hi(z0, z0);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        b[q][3] = 0u;
        const bf16x8 bq = __builtin_bit_cast(bf16x8, b[q]);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
            acc[fb] = mfma_k32(ldbf8(L + NX_W1S, ((((q ? 1 : 0) * 4 + g) * 4 + fb) * 16 + j) * 8), bq, acc[fb]);
    }
}

// Teacher and student forwards of one tile with split images (both nets, interleaved):
// layer 1 (layer1_split) and layer 2 on split bf16 MFMAs.  Layer 2 runs in three scheduling
// regions: the first K step's splits | its MFMAs with the second step's splits in their gaps
// (per output block its six piece loads, then 12 x (one MFMA, three VALU)) | the second
// step's MFMAs (c4 80.9 -> 79.7 us per step, profiles/r03y_sched_nt.txt; 3 VALU per MFMA
// -0.25 us vs 2, profiles/r03ze_ps_per.txt).
__device__ __forceinline__ void mlp_forward_pair_split(const float* LT, const float* LS, const float* ob, int j, int g,
                                                       f32x4 (&H1)[4], f32x4 (&H2)[4], float& mt0, float& mt1,
                                                       float& ms0, float& ms1) {
    f32x4 at[4], as[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) at[fb] = as[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    layer1_split(LT, ob, j, g, at);
    layer1_split(LS, ob, j, g, as);
    f32x4 T1[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        T1[fb] = tanh4(at[fb]);
        H1[fb] = tanh4(as[fb]);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        at[fb] = ld4(LT + NX_B2 + 16 * fb + 4 * g);
        as[fb] = ld4(LS + NX_B2 + 16 * fb + 4 * g);
    }
    {   // three regions: split s0 | s0 MFMAs + split s1 | s1 MFMAs
        bf16x8 tp[2][3], sp[2][3];
        __builtin_amdgcn_sched_barrier(0);
        split8(T1[0], T1[1], tp[0]);
        split8(H1[0], H1[1], sp[0]);
        __builtin_amdgcn_sched_barrier(0);
        split8(T1[2], T1[3], tp[1]);
        split8(H1[2], H1[3], sp[1]);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const int o = (((0 * 4 + g) * 4 + fb) * 16 + j) * 8;
            bf16x8 wt[3], ws[3];
            ld_pieces(LT, NX_W2F, o, wt);
            ld_pieces(LS, NX_W2F, o, ws);
            at[fb] = mfma_split(wt, tp[0], at[fb]);
            as[fb] = mfma_split(ws, sp[0], as[fb]);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 6, 2);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            if (fb < 3) __builtin_amdgcn_sched_group_barrier(0x100, 6, 2);
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 2);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 2);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const int o = (((1 * 4 + g) * 4 + fb) * 16 + j) * 8;
            bf16x8 wt[3], ws[3];
            ld_pieces(LT, NX_W2F, o, wt);
            ld_pieces(LS, NX_W2F, o, ws);
            at[fb] = mfma_split(wt, tp[1], at[fb]);
            as[fb] = mfma_split(ws, sp[1], as[fb]);
        }
    }
    float pt0 = 0.0f, pt1 = 0.0f, ps0 = 0.0f, ps1 = 0.0f;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const f32x4 ta = ld4(LT + NX_W3 + (16 * fb + 4 * g) * 2), tb = ld4(LT + NX_W3 + (16 * fb + 4 * g) * 2 + 4);
        const f32x4 sa = ld4(LS + NX_W3 + (16 * fb + 4 * g) * 2), sb = ld4(LS + NX_W3 + (16 * fb + 4 * g) * 2 + 4);
        f32x4 t2;
        t2 = tanh4(at[fb]);
        H2[fb] = tanh4(as[fb]);
        pt0 = fmaf(t2[0], ta[0], pt0); pt1 = fmaf(t2[0], ta[1], pt1);
        pt0 = fmaf(t2[1], ta[2], pt0); pt1 = fmaf(t2[1], ta[3], pt1);
        pt0 = fmaf(t2[2], tb[0], pt0); pt1 = fmaf(t2[2], tb[1], pt1);
        pt0 = fmaf(t2[3], tb[2], pt0); pt1 = fmaf(t2[3], tb[3], pt1);
        ps0 = fmaf(H2[fb][0], sa[0], ps0); ps1 = fmaf(H2[fb][0], sa[1], ps1);
        ps0 = fmaf(H2[fb][1], sa[2], ps0); ps1 = fmaf(H2[fb][1], sa[3], ps1);
        ps0 = fmaf(H2[fb][2], sb[0], ps0); ps1 = fmaf(H2[fb][2], sb[1], ps1);
        ps0 = fmaf(H2[fb][3], sb[2], ps0); ps1 = fmaf(H2[fb][3], sb[3], ps1);
    }
    mt0 = xsum32(xsum16(pt0)) + LT[NX_B3];
    mt1 = xsum32(xsum16(pt1)) + LT[NX_B3 + 1];
    ms0 = xsum32(xsum16(ps0)) + LS[NX_B3];
    ms1 = xsum32(xsum16(ps1)) + LS[NX_B3 + 1];
}

// One net's forward with a split image (the teacher beside the bf16 student; HO: also
// return the hidden activations).
template <bool HO>
__device__ __forceinline__ void mlp_forward_split_t(const float* L, const float* ob, int j, int g, f32x4 (&H1)[4],
                                                    f32x4 (&H2)[4], float& m0, float& m1) {
    f32x4 acc[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = f32x4{0.f, 0.f, 0.f, 0.f};
    layer1_split(L, ob, j, g, acc);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
        H1[fb] = tanh4(acc[fb]);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = ld4(L + NX_B2 + 16 * fb + 4 * g);
    {   // three regions, as the pair's layer 2 (c5 37.2-37.6 -> 36.6 us per step, profiles/r03za_tsched.txt)
        bf16x8 hp[2][3];
        __builtin_amdgcn_sched_barrier(0);
        split8(H1[0], H1[1], hp[0]);
        __builtin_amdgcn_sched_barrier(0);
        split8(H1[2], H1[3], hp[1]);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            bf16x8 w[3];
            ld_pieces(L, NX_W2F, (((0 * 4 + g) * 4 + fb) * 16 + j) * 8, w);
            acc[fb] = mfma_split(w, hp[0], acc[fb]);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 3, 3);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            if (fb < 3) __builtin_amdgcn_sched_group_barrier(0x100, 3, 3);
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 3);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 3);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            bf16x8 w[3];
            ld_pieces(L, NX_W2F, (((1 * 4 + g) * 4 + fb) * 16 + j) * 8, w);
            acc[fb] = mfma_split(w, hp[1], acc[fb]);
        }
    }
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const f32x4 wa = ld4(L + NX_W3 + (16 * fb + 4 * g) * 2);
        const f32x4 wb = ld4(L + NX_W3 + (16 * fb + 4 * g) * 2 + 4);
        f32x4 h2;
        h2 = tanh4(acc[fb]);
        if constexpr (HO) H2[fb] = h2;
        p0 = fmaf(h2[0], wa[0], p0); p1 = fmaf(h2[0], wa[1], p1);
        p0 = fmaf(h2[1], wa[2], p0); p1 = fmaf(h2[1], wa[3], p1);
        p0 = fmaf(h2[2], wb[0], p0); p1 = fmaf(h2[2], wb[1], p1);
        p0 = fmaf(h2[3], wb[2], p0); p1 = fmaf(h2[3], wb[3], p1);
    }
    m0 = xsum32(xsum16(p0)) + L[NX_B3];
    m1 = xsum32(xsum16(p1)) + L[NX_B3 + 1];
}
__device__ __forceinline__ void mlp_forward_split(const float* L, const float* ob, int j, int g, float& m0, float& m1) {
    f32x4 h1[4], h2[4];
    mlp_forward_split_t<false>(L, ob, j, g, h1, h2, m0, m1);
}

// ---------------------------------------------------------------- prepacked LDS images
// The rollout's LDS images (teacher NET floats, student NET_S floats) are kept ready in
// HBM: pack_param() writes one parameter's value into every image slot it occupies.  The
// images are built once by pack_net_kernel (rdd_set_teacher / rdd_set_student) and the
// student's is refreshed by reduce_adam_kernel as it updates each parameter, so a rollout's
// prologue is a plain 16-B copy instead of a gather with index arithmetic.
// image kinds: IMG_F32 (N_* layout), IMG_SPLIT (NX_*), IMG_BF16 (NB_*, student only)
constexpr int IMG_F32 = 0, IMG_SPLIT = 1, IMG_BF16 = 2;

__device__ __forceinline__ void pack_param(float* img, int p, float v, bool student, int kind) {
    if (kind == IMG_SPLIT) {
        unsigned short* h = reinterpret_cast<unsigned short*>(img);
        unsigned short q[3];
        if (p < P_W2) {   // W1 rows 0..10, b1 as row 11
            const int k = p < P_B1 ? p >> 6 : OBD, f = p < P_B1 ? p & 63 : p - P_B1;
            // layer1_split's A operands: slots 2s, 2s + 1 of lane group k & 3
            split1(kTanhScale * v, q);
            const int o = 2 * NX_W1S + (((k & 3) * 4 + (f >> 4)) * 16 + (f & 15)) * 8 + 2 * (k >> 2);
            constexpr int V1 = 4 * 4 * 16 * 8;   // the (0,1) pairing follows the (0,2) one
            put(h + (o), q[0]); put(h + (o + 1), q[2]);
            put(h + (o + V1), q[0]); put(h + (o + V1 + 1), q[1]);
        } else if (p < P_B2) {
            const int k = (p - P_W2) >> 6, f = (p - P_W2) & 63;
            {   // forward: k is the permuted K index (as NB_W2F), pieces of the scaled weight
                const int s = k >> 5, r = k & 31, gg = (r & 15) >> 2, jj = (r & 3) + 4 * (r >> 4);
                const int o = 2 * NX_W2F + (((s * 4 + gg) * 4 + (f >> 4)) * 16 + (f & 15)) * 8 + jj;
                split1(kTanhScale * v, q);
                put(h + (o), q[0]); put(h + (o + SP_PIECE), q[1]); put(h + (o + 2 * SP_PIECE), q[2]);
            }
            if (student) {   // dH1: f is the permuted K index (as NB_W2B), unscaled
                const int s = f >> 5, r = f & 31, gg = (r & 15) >> 2, jj = (r & 3) + 4 * (r >> 4);
                const int o = 2 * NX_W2B + (((s * 4 + gg) * 4 + (k >> 4)) * 16 + (k & 15)) * 8 + jj;
                split1(v, q);
                put(h + (o), q[0]); put(h + (o + SP_PIECE), q[1]); put(h + (o + 2 * SP_PIECE), q[2]);
            }
        } else if (p < P_W3) {
            put(img + (NX_B2 + (p - P_B2)), kTanhScale * v);
        } else if (p < P_B3) {
            put(img + (NX_W3 + (p - P_W3)), v);
        } else if (p < P_LS) {
            put(img + (NX_B3 + (p - P_B3)), v);
        } else if (p < P_TOT) {
            put(img + (NX_LS + (p - P_LS)), v);
        }
        return;
    }
    if (kind == IMG_F32) {
        if (p < P_B1) {
            const int k = p >> 6, f = p & 63;
            put(img + (N_W1 + k * HID + (f & 15) * 4 + (f >> 4)), kTanhScale * v);
        } else if (p < P_W2) {
            const int f = p - P_B1;
            put(img + (N_W1 + OBD * HID + (f & 15) * 4 + (f >> 4)), kTanhScale * v);
        } else if (p < P_B2) {
            const int k = (p - P_W2) >> 6, f = (p - P_W2) & 63;
            put(img + (N_W2 + k * HID + (f & 15) * 4 + (f >> 4)), kTanhScale * v);
            if (student) put(img + (N_W2T + f * HID + (k & 15) * 4 + (k >> 4)), v);
        } else if (p < P_W3) {
            put(img + (N_B2 + (p - P_B2)), kTanhScale * v);
        } else if (p < P_B3) {
            put(img + (N_W3 + (p - P_W3)), v);
        } else if (p < P_LS) {
            put(img + (N_B3 + (p - P_B3)), v);
        } else if (p < P_TOT) {
            put(img + (N_LS + (p - P_LS)), v);
        }
        return;
    }
    unsigned short* h = reinterpret_cast<unsigned short*>(img);
    if (p < P_B1) {
        const int k = p >> 6, f = p & 63;   // k = 8gg + jj
        put(h + (2 * NB_W1 + (((k >> 3) * 4 + (f >> 4)) * 16 + (f & 15)) * 8 + (k & 7)), bf16_bits(v));
    } else if (p < P_W2) {
        put(img + (NB_B1 + (p - P_B1)), v);
    } else if (p < P_B2) {
        const int k = (p - P_W2) >> 6, f = (p - P_W2) & 63;
        // forward image: k (H1 feature) is the permuted K index, f the output row
        {
            const int s = k >> 5, r = k & 31, gg = (r & 15) >> 2, jj = (r & 3) + 4 * (r >> 4);
            put(h + (2 * NB_W2F + (((s * 4 + gg) * 4 + (f >> 4)) * 16 + (f & 15)) * 8 + jj), bf16_bits(v));
        }
        // dH1 image: f (dZ2 feature) is the permuted K index, k the output row
        {
            const int s = f >> 5, r = f & 31, gg = (r & 15) >> 2, jj = (r & 3) + 4 * (r >> 4);
            put(h + (2 * NB_W2B + (((s * 4 + gg) * 4 + (k >> 4)) * 16 + (k & 15)) * 8 + jj), bf16_bits(v));
        }
    } else if (p < P_W3) {
        put(img + (NB_B2 + (p - P_B2)), v);
    } else if (p < P_B3) {
        put(img + (NB_W3 + (p - P_W3)), bf16_round(v));
    } else if (p < P_LS) {
        put(img + (NB_B3 + (p - P_B3)), v);
    } else if (p < P_TOT) {
        put(img + (NB_LS + (p - P_LS)), v);
    }
}

// net = params[P] | mu[11] | sd[11] -> image (every slot, including zero padding and filter)
__global__ __launch_bounds__(256) void pack_net_kernel(const float* net, float* img, int img_floats, int student,
                                                       int kind) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    // phase 1 (one launch): zero the image, then the filter words, then every parameter
    for (int i = x; i < img_floats; i += gridDim.x * 256) img[i] = 0.0f;
    __syncthreads();   // (single-block launch: see rdd host code)
    if (x < 12) {
        const int mu = kind == IMG_BF16 ? NB_MU : kind == IMG_SPLIT ? NX_MU : N_MU;
        const int rs = kind == IMG_BF16 ? NB_RS : kind == IMG_SPLIT ? NX_RS : N_RS;
        img[mu + x] = x < OBD ? net[P_TOT + x] : 0.0f;
        img[rs + x] = x < OBD ? 1.0f / net[P_TOT + OBD + x] : 1.0f;
    }
    for (int p = x; p < P_TOT; p += gridDim.x * 256) pack_param(img, p, net[p], student != 0, kind);
}

// Both rollout images (contiguous in LDS: teacher then student) by LDS-DMA: every 16-B piece is
// one global_load_lds_dwordx4 (wave-uniform LDS base + lane x 16 B, per-lane global address), so
// the copy needs no staging VGPRs and no ds_write pass.  `between` runs while they are in flight
// (the producers' first observations); every wave then drains its DMA (vmcnt(0)) before the
// caller's __syncthreads publishes the image.  Round 4 measured it 0.2-0.3 us per step faster
// than the register-staged copy (profiles/r04c_imgdma_ab.txt) but reverted it: its first rollout
// in a process differed in lanes-48-63 dW3 entries.  Round 5 found that signature's cause on the
// compute side -- the SLP-packed dW3 accumulators at the tile loop's latch (PKWAR, DESIGN.md §3;
// distill.hip is now built without SLP) -- and re-landed the fill; the register-staged form is
// in profiles/r04_removed_diagnostic_variants.diff.
template <int V4A, int V4B, int NT, class F>
__device__ __forceinline__ void copy_images(float* L, const float* ta, const float* sb, F&& between) {
    constexpr int TOT = V4A + V4B, PER = (TOT + NT - 1) / NT;
    const int wbase = threadIdx.x & ~63;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int x = threadIdx.x + u * NT;
        if (x < TOT)
            __builtin_amdgcn_global_load_lds(x < V4A ? ta + 4 * x : sb + 4 * (x - V4A), L + 4 * (wbase + u * NT), 16, 0, 0);
    }
    between();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's image pieces have landed in LDS
}

// kTanhScale * x as four scalar multiplies: a vector multiply would be a v_pk_mul_f32, and packed-f32
// ops are kept out of the rollout's hot loops (PKWAR)
__device__ __forceinline__ f32x4 scale4(f32x4 x) {
    return f32x4{kTanhScale * x[0], kTanhScale * x[1], kTanhScale * x[2], kTanhScale * x[3]};
}

// bf16-student forward of a 16-env tile (same outputs/layouts as mlp_forward).
__device__ __forceinline__ void mlp_forward_bf16(const float* L, const float* ob, int j, int g, f32x4 (&H1)[4],
                                                 f32x4 (&H2)[4], float& m0, float& m1) {
    f32x4 acc[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = ld4(L + NB_B1 + 16 * fb + 4 * g);
    // layer 1: one K = 32 step, lane group g supplies inputs 8g .. 8g+7 (zero past input 10)
    bf16x8 zb;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int k = 8 * g + jj;
        const int kc = k < OBD ? k : 0;
        const float z = fminf(fmaxf((ob[j * SOS + kc] - L[NB_MU + kc]) * L[NB_RS + kc], -5.0f), 5.0f);
        zb[jj] = (__bf16)(k < OBD ? z : 0.0f);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = mfma_k32(ldbf8(L + NB_W1, ((g * 4 + fb) * 16 + j) * 8), zb, acc[fb]);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
        H1[fb] = tanh4(scale4(acc[fb]));
    // layer 2: two K = 32 steps over the permuted feature order kperm
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) acc[fb] = ld4(L + NB_B2 + 16 * fb + 4 * g);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bf16x8 hb = pack8(H1[2 * s], H1[2 * s + 1]);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
            acc[fb] = mfma_k32(ldbf8(L + NB_W2F, (((s * 4 + g) * 4 + fb) * 16 + j) * 8), hb, acc[fb]);
    }
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const f32x4 wa = ld4(L + NB_W3 + (16 * fb + 4 * g) * 2);
        const f32x4 wb = ld4(L + NB_W3 + (16 * fb + 4 * g) * 2 + 4);
        H2[fb] = tanh4(scale4(acc[fb]));
        p0 = fmaf(H2[fb][0], wa[0], p0); p1 = fmaf(H2[fb][0], wa[1], p1);
        p0 = fmaf(H2[fb][1], wa[2], p0); p1 = fmaf(H2[fb][1], wa[3], p1);
        p0 = fmaf(H2[fb][2], wb[0], p0); p1 = fmaf(H2[fb][2], wb[1], p1);
        p0 = fmaf(H2[fb][3], wb[2], p0); p1 = fmaf(H2[fb][3], wb[3], p1);
    }
    m0 = xsum32(xsum16(p0)) + L[NB_B3];
    m1 = xsum32(xsum16(p1)) + L[NB_B3 + 1];
}
