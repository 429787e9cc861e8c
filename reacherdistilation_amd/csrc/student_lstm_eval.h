// student_lstm.hip's whole-episode evaluation (rdl_evaluate, include/reacher_student_lstm.h): one
// rollout launch rolls n evaluation envs through E consecutive 50-step episodes under the LSTM
// student's mean action (DESIGN.md §3 "Evaluation of the LSTM student"): the query loop of
// lstm_train.train without the optimiser steps.  Included inside student_lstm.hip's anonymous
// namespace after head_layer; expects rd_device.h, rd_physics.h and the file's constants.
//
// A workgroup (8 waves, two per SIMD) owns a block of 16 envs -- one MFMA row tile -- for the whole
// launch:
//  * lanes 0..15 of wave 0 keep the envs: state, return and the carried reward in registers
//    (rd::env_reset, rd::observe<true>, rd::env_step<true>: rd_reset / rd_step's functions);
//  * wave 7 (one unit block of its own, below) runs the teacher, tch::mlp_forward<true> on the
//    load_net image (forward_kernel's, kept in LDS for the launch);
//  * the x rows of an episode's last T records (inputs_kernel's arithmetic, formed once per record)
//    stay in an LDS ring, c and h in LDS; a record before the episode's first is the zero row's
//    x = [0 | bp];
//  * per window position the eight waves share the 13 blocks of 16 units (a SIMD's second wave
//    issues MFMAs while the first evaluates its cells: a block's 20 exp / tanh per lane cost about
//    as much issue time as its 256 MFMAs).  A wave forms the four gates of its block -- Zx (k < 43,
//    one chain, the Zx GEMM's order and epilogue) and the recurrent half as the two chains k < 112 /
//    k >= 112 of lstm_rec_fwd_kernel -- with the weights streamed from L2 out of an image packed once
//    per call (lstm_eval_pack_kernel: every B operand of a lane for four k steps is one 16-byte
//    load, a wave's load one contiguous KB), then the cell at its points (lstm_rec_fwd_kernel's
//    epilogue);
//  * head T-1 runs as head_fwd_kernel's five head_layer calls on the final h, over eight waves.
// No env depends on another (an MFMA row, a lane): no grid barrier, no hand-off between workgroups.
// Every operation is the stepwise forward's in its order, so the outputs are bitwise those of
// rd_reset, then 50 x { rdd_forward, the window, rdl_forward, rd_step }, whatever the grid.
#pragma once

// The 2x64 MlpPolicy's layouts and exact-f32 forward: the definitions distill.hip compiles, in a
// namespace of their own (student_mlp_eval.h does the same in its translation unit).
namespace tch {
using rd::f32x4, rd::mfma, rd::ld4, rd::kTanhScale, rd::tanh_pre;
constexpr bool kFenceAll = false;   // the all-fenced diagnostic build is distill.hip's; mlp_forward<true> is fenced
#include "distill_layout.h"
#include "distill_forward_f32.h"
}  // namespace tch

constexpr int EV_ROWS = 16;                          // envs per workgroup: one MFMA row tile
constexpr int EV_MAX_T = RDL_EVAL_MAX_STEPS;         // the history ring's rows per env
constexpr int EV_REC = rd::kObsDim + 1 + 4 + 4 + 1;  // dataset.py's record: ob | reward | t_pdflat | s_pdflat | stepped_with
constexpr int EV_UB = (U + 15) / 16;                 // 13 blocks of 16 units (the last holds 8)
// k steps of a (unit block, gate) in groups of four: 3 of Zx (k < 43; the rest zero), 7 of the
// recurrent chain k < 112, 6 of the chain k >= 112 (k >= 200 zero)
constexpr int EV_GX = 3, EV_GLO = LSTM_KH / 16, EV_GHI = (U - LSTM_KH + 15) / 16, EV_G = EV_GX + EV_GLO + EV_GHI;
constexpr int EV_IMG = EV_UB * EV_G * 4 * 64 * 4;    // the packed image: [ub][group][gate][lane][4 k steps], 212,992 floats
constexpr int EV_WAVES = 8, EV_THREADS = 64 * EV_WAVES;
constexpr int EV_PF = 3;                             // groups of B operands in flight ahead of the MFMAs
constexpr int EV_XS = 52, EV_HS = U + 4;             // LDS row strides of x and h / c (64 distinct banks per A-operand read)
static_assert(EV_MAX_T >= 16 && XI + 1 <= 4 * 4 * EV_GX && LSTM_KH % 16 == 0 && EV_G == 16 && tch::OBD == rd::kObsDim,
              "evaluation tiling");

// image[ub][g][y][lane = (gq, i)][e] = the weight of gate y, unit 16 ub + i at k = 4 (4 g' + e) + gq of
// its chain: Wl[k] (g < 3, k < 43), Wr[k] (k < 112), Wr[112 + k] (k < 88); zero past the matrix
__global__ __launch_bounds__(256) void lstm_eval_pack_kernel(const float* __restrict__ P, float* __restrict__ img) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= EV_IMG) return;
    const int e = x & 3, lane = (x >> 2) & 63, y = (x >> 8) & 3, g = (x >> 10) & 15, ub = x >> 14;
    const int i = lane & 15, gq = lane >> 4, u = 16 * ub + i;
    int row;   // of Wl [243][800], -1: zero
    if (g < EV_GX) {
        const int k = 4 * (4 * g + e) + gq;
        row = k < XI ? k : -1;
    } else if (g < EV_GX + EV_GLO) {
        row = XI + 4 * (4 * (g - EV_GX) + e) + gq;
    } else {
        const int k = LSTM_KH + 4 * (4 * (g - EV_GX - EV_GLO) + e) + gq;
        row = k < U ? XI + k : -1;
    }
    img[x] = row >= 0 && u < U ? P[OFF_WL + (int64_t)row * G4 + y * U + u] : 0.0f;
}

struct LsEvalArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* P;          // the student's flat parameters
    const float* img;        // lstm_eval_pack_kernel's image of Wl [EV_IMG]
    const float* draws;      // [E][n][6] or null (Philox)
    const float* state0;     // [2][n][U] = (c, h) or null (zeros)
    float* returns;          // [E][n]
    float* final_dist;       // [E][n] or null
    float* records;          // [E][n][50][EV_REC] or null
    float* state_out;        // [2][n][U] or null
    int episodes, first_episode, T;
};

__global__ __launch_bounds__(EV_THREADS) void student_lstm_evaluate_kernel(LsEvalArgs a) {
    __shared__ __attribute__((aligned(16))) float LT[tch::NET];                  // the teacher (load_net)
    __shared__ __attribute__((aligned(16))) float SO[EV_ROWS * tch::SOS];        // raw obs rows (component 11 = 1)
    __shared__ __attribute__((aligned(16))) float TO[2][EV_ROWS][4];             // the teacher's pdflat, by step parity
    __shared__ __attribute__((aligned(16))) float Xr[EV_MAX_T][EV_ROWS][EV_XS];  // x rows of records j, slot j % T
    __shared__ __attribute__((aligned(16))) float Xz[EV_XS];                     // the zero record's x row [0 | bp | 0]
    __shared__ __attribute__((aligned(16))) float Hb[2][EV_ROWS][EV_HS];         // h, read / written by position parity
    __shared__ __attribute__((aligned(16))) float Cst[EV_ROWS][EV_HS];           // c
    __shared__ __attribute__((aligned(16))) float X1[HF_ROWS][L1];
    __shared__ __attribute__((aligned(16))) float X2[HF_ROWS][L2];
    __shared__ __attribute__((aligned(16))) float X3[HF_ROWS][L3];
    __shared__ __attribute__((aligned(16))) float X4[HF_ROWS][L4];
    __shared__ __attribute__((aligned(16))) float X5[HF_ROWS][8];
    static_assert(EV_ROWS == HF_ROWS, "head_layer's tile");
    const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, gq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // in an SGPR: the weight addresses are scalar + lane
    const int T = a.T;
    const float* P = a.P;
    const float* Ph0 = P + OFF_H + (int64_t)(T - 1) * HSZ;   // head T-1: the only one a query evaluates
    const rdg::f32x4* img4 = reinterpret_cast<const rdg::f32x4*>(a.img);
    tch::load_net(LT, a.tnet, false, EV_THREADS);   // published by the first step's barriers
    // this thread's point of the dense32 part of x: row tid / 32, column 11 + tid % 32
    const int dr = tid >> 5, dc = tid & 31;
    static_assert(EV_THREADS == EV_ROWS * 32, "a dense32 point per thread");
    float wp[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wp[q] = P[OFF_WP + q * 32 + dc];
    const float bpc = P[OFF_BP + dc];
    for (int x = tid; x < EV_MAX_T * EV_ROWS * EV_XS; x += EV_THREADS) (&Xr[0][0][0])[x] = 0.0f;
    if (tid < EV_XS) Xz[tid] = 0.0f;
    __syncthreads();
    if (tid < 32) {   // inputs_kernel's arithmetic on a zero prev: bias first, then four fmaf
        float v = bpc;
#pragma unroll
        for (int q = 0; q < 4; ++q) v = fmaf(0.0f, wp[q], v);
        Xz[11 + tid] = v;
    }
    const bool phys = wave == 0 && lane < EV_ROWS;   // the env of this lane
    const int64_t n = a.n, nblk = (n + EV_ROWS - 1) / EV_ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * EV_ROWS;
        const bool valid = phys && row0 + lane < n;
        const int64_t env = row0 + (valid ? lane : 0);   // a ragged block's spare lanes repeat its env 0
        __syncthreads();   // the previous block's last reads of c and h
        for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {   // the call's initial state
            const int r = x / U, u = x - r * U;
            const int64_t er = row0 + r < n ? row0 + r : row0;
            Cst[r][u] = a.state0 ? a.state0[er * U + u] : 0.0f;
            Hb[0][r][u] = a.state0 ? a.state0[(n + er) * U + u] : 0.0f;
        }
        int hp = 0;   // Hb[hp] holds the current h
        rd::State st;
        float carry = 0.0f;   // the reward this env's previous step returned
        for (int e = 0; e < a.episodes; ++e) {
            float ret = 0.0f;
            if (phys) {
                float d[6];
                if (a.draws) {
                    const float* p = a.draws + ((int64_t)e * n + env) * 6;
#pragma unroll
                    for (int k = 0; k < 6; ++k) d[k] = p[k];
                } else {
                    rd::philox_draw(a.seed, (uint64_t)(a.env_base + env), (uint32_t)(a.first_episode + e), d);
                }
                rd::env_reset(st, d);
            }
            float* rec = a.records && valid ? a.records + ((int64_t)e * n + env) * (rd::kEpisodeSteps * EV_REC) : nullptr;
            for (int s = 0; s < rd::kEpisodeSteps; ++s) {
                const int slot = s % T;
                if (phys) {   // record s: ob_s | the carried reward
                    float ob[rd::kObsDim];
                    rd::observe<true>(st, ob);
#pragma unroll
                    for (int k = 0; k < rd::kObsDim; ++k) {
                        SO[lane * tch::SOS + k] = ob[k];
                        Xr[slot][lane][k] = ob[k];
                    }
                    SO[lane * tch::SOS + tch::OBD] = 1.0f;
                    if (rec) {
                        float* r = rec + s * EV_REC;
#pragma unroll
                        for (int k = 0; k < rd::kObsDim; ++k) r[k] = ob[k];
                        r[rd::kObsDim] = carry;
                        r[EV_REC - 1] = 1.0f;
                    }
                }
                {   // prev . Wp + bp of record s: prev = T_{s-1}, zero at s = 0
                    float v = bpc;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v = fmaf(s ? TO[(s - 1) & 1][dr][q] : 0.0f, wp[q], v);
                    Xr[slot][dr][11 + dc] = v;
                }
                __syncthreads();
                if (wave == EV_WAVES - 1) {   // T_s
                    rd::f32x4 A1[4], A2[4];
                    float m0, m1;
                    tch::mlp_forward<true>(LT, SO, i, gq, A1, A2, m0, m1);
                    if (gq == 0) {
                        float* o = TO[s & 1][i];
                        o[0] = m0; o[1] = m1; o[2] = LT[tch::N_LS]; o[3] = LT[tch::N_LS + 1];
                    }
                }
                // the query: positions p = 0 .. T-1 hold records s - (T-1) + p, from the carried (c, h)
                for (int p = 0; p < T; ++p) {
                    const int j = s - (T - 1) + p;
                    const float* xrow = j < 0 ? Xz : &Xr[j % T][i][0];
                    const float* hrow = &Hb[hp][i][0];
                    for (int it = 0; it < (EV_UB + EV_WAVES - 1) / EV_WAVES; ++it) {
                        const int ub = wave + EV_WAVES * it;
                        if (ub >= EV_UB) break;   // (wave-uniform)
                        const int u = 16 * ub + i;
                        const bool uv = u < U;
                        // the block's image: a scalar base (opaque here, so that its 64 load addresses are
                        // formed where they are used, not once per launch and kept in registers) + the lane
                        uint32_t here = 0;
                        asm volatile("" : "+s"(here));
                        const rdg::f32x4* wb = img4 + (int64_t)ub * (EV_G * 4 * 64) + here;
                        const uint32_t ln = (uint32_t)lane;
                        // group g's operands: the four gates' B (one 16-byte load each) and this lane's
                        // A values x[i][k] / h[i][k], k = 4 (4 g' + e) + gq (zero past U: the B rows are zero
                        // there, the LDS pad is not)
                        rdg::f32x4 b[EV_PF][4];
                        float av[EV_PF][4];
                        auto fetch = [&](int g) {
#pragma unroll
                            for (int y = 0; y < 4; ++y) b[g % EV_PF][y] = wb[(g * 4 + y) * 64 + ln];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int q = 4 * (g < EV_GX ? g : g - EV_GX) + e;
                                av[g % EV_PF][e] = g < EV_GX ? xrow[4 * q + gq] : 4 * q < U ? hrow[4 * q + gq] : 0.0f;
                            }
                        };
#pragma unroll
                        for (int g = 0; g < EV_PF; ++g) fetch(g);
                        float bias[4];
#pragma unroll
                        for (int y = 0; y < 4; ++y) bias[y] = uv ? P[OFF_BL + y * U + u] : 0.0f;
                        rdg::f32x4 zx[4], lo[4], hi[4];
#pragma unroll
                        for (int y = 0; y < 4; ++y) zx[y] = lo[y] = hi[y] = rdg::f32x4{0.f, 0.f, 0.f, 0.f};
                        // a group: four k steps of the four gates' chains, its operands in registers
                        // and the loads of group g + EV_PF issued before its MFMAs start (SrcC fence)
                        auto group = [&](int g, rdg::f32x4 (&acc)[4]) {
                            rdg::f32x4 cur[4];
                            float ca[4];
#pragma unroll
                            for (int y = 0; y < 4; ++y) {
                                cur[y] = b[g % EV_PF][y];
                                ca[y] = av[g % EV_PF][y];
                            }
                            if (g + EV_PF < EV_G) fetch(g + EV_PF);
                            fence_begin(acc);
#pragma unroll
                            for (int k = 0; k < 4; ++k)
#pragma unroll
                                for (int y = 0; y < 4; ++y)
                                    acc[y] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[k], cur[y][k], acc[y], 0, 0, 0);
                            fence_end(acc);
                        };
#pragma unroll
                        for (int g = 0; g < EV_G; ++g) {
                            if (g < EV_GX) group(g, zx);
                            else if (g < EV_GX + EV_GLO) group(g, lo);
                            else group(g, hi);
                        }
                        // TF1 LSTMCell at rows 4 gq + r of unit u (lstm_rec_fwd_kernel's epilogue; Zx = acc + bias
                        // is the Zx GEMM's)
                        if (uv) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int row = 4 * gq + r;
                                float z[4];
#pragma unroll
                                for (int y = 0; y < 4; ++y) {
                                    const float zxv = zx[y][r] + bias[y];
                                    z[y] = ((lo[y][r] + hi[y][r]) + 0.0f) + zxv;
                                }
                                const float gi = sigm(z[0]), gj = tanhf(z[1]), gf = sigm(z[2] + 1.0f), go = sigm(z[3]);
                                const float c = fmaf(gf, Cst[row][u], gi * gj);
                                Cst[row][u] = c;
                                Hb[hp ^ 1][row][u] = go * tanhf(c);
                            }
                        }
                    }
                    hp ^= 1;
                    __syncthreads();
                }
                // head T-1 on the final h (head_fwd_kernel's layers; nothing stored to global: R = 0)
                const float (*X0)[EV_HS] = Hb[hp];
                uint32_t hoff = 0;   // (opaque, as the image's base: the layers' addresses are formed here)
                asm volatile("" : "+s"(hoff));
                const float* Ph = Ph0 + hoff;
                head_layer<U, H1, true, EV_WAVES>(X0, X1, Ph + OFF_W1, Ph + OFF_B1, nullptr, 0, 0, 0);
                head_layer<H1, H2, true, EV_WAVES>(X1, X2, Ph + OFF_W2, Ph + OFF_B2, nullptr, 0, 0, 0);
                head_layer<H2, H3, true, EV_WAVES>(X2, X3, Ph + OFF_W3, Ph + OFF_B3, nullptr, 0, 0, 0);
                head_layer<H3, H4, true, EV_WAVES>(X3, X4, Ph + OFF_W4, Ph + OFF_B4, nullptr, 0, 0, 0);
                head_layer<H4, 4, false, EV_WAVES>(X4, X5, Ph + OFF_W5, Ph + OFF_B5, nullptr, 0, 0, 0);
                // the next step's first writes (SO, the ring's slot, TO's other parity) follow every
                // read of them: the barriers above
                if (phys) {
                    float sp[4], tp[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        sp[c] = X5[lane][c];
                        tp[c] = TO[s & 1][lane][c];
                    }
                    if (rec) {
                        float* r = rec + s * EV_REC + rd::kObsDim + 1;
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            r[c] = tp[c];
                            r[4 + c] = sp[c];
                        }
                    }
                    carry = rd::env_step<true>(st, sp[0], sp[1]);
                    ret += carry;
                }
            }
            if (valid) {
                a.returns[(int64_t)e * n + env] = ret;
                if (a.final_dist) a.final_dist[(int64_t)e * n + env] = rd::tip_distance(st);
            }
        }
        if (a.state_out)   // (c, h) after the call's last query (the last position ends with a barrier)
            for (int x = tid; x < EV_ROWS * U; x += EV_THREADS) {
                const int r = x / U, u = x - r * U;
                if (row0 + r < n) {
                    a.state_out[(row0 + r) * U + u] = Cst[r][u];
                    a.state_out[(n + row0 + r) * U + u] = Hb[hp][r][u];
                }
            }
    }
}
