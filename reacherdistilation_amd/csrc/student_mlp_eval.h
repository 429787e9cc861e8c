// student_mlp.hip's whole-episode evaluation (rdm_evaluate, include/reacher_student_mlp.h): one
// launch rolls n evaluation envs through E consecutive 50-step episodes under the reference
// student's mean action (DESIGN.md §3 "Evaluation of the reference student").  Included inside
// student_mlp.hip's anonymous namespace after fwd_layer; expects rd_device.h and rd_physics.h.
//
// A workgroup owns a block of ROWS envs (64, or 16 for a small batch) for the whole launch:
//  * wave 0 keeps the envs, one per lane: state, return and the carried reward in registers
//    (rd::env_reset, rd::observe<true>, rd::env_step<true>: rd_reset / rd_step's functions);
//  * waves 0..7 run the student's layers on the block exactly as student_mlp_kernel's forward does
//    (fwd_layer on the trainer's weight image, the activations in LDS between the layers);
//  * waves 8.. (one per 16-env tile) run the teacher, mlp_forward<true> on the load_net image
//    (forward_kernel's, kept in LDS for the launch).  T_s is needed only by step s + 1's row and by
//    the records, so it runs beside the student's largest layer (128 x 128).
// Every env's chain depends on no other env (an MFMA row, a lane), and every function is the
// stepwise path's, so the outputs are bitwise those of rd_reset, then 50 x { rdd_forward,
// rdm_forward on the assembled row, rd_step }, whatever ROWS and the grid.
#pragma once

#include "teacher_f32.h"   // namespace tch: the teacher's layouts, load_net and mlp_forward

constexpr int EREC = rd::kObsDim + 1 + 4 + 4 + 1;   // dataset.py's record: ob | reward | t_pdflat | s_pdflat | stepped_with
static_assert(RDM_IN == rd::kObsDim + RDM_OUT + 1 && tch::OBD == rd::kObsDim, "row = ob | prev pdflat | prev reward");

template <int ROWS>
struct ELay {
    static constexpr int TW = ROWS / 16;                           // teacher waves: one per 16-env tile
    static constexpr int THREADS = 64 * (WAVES + TW);
    static constexpr int O_NET = Lay<ROWS>::O_D4;                  // after the forward's buffers X0 .. X4, D5
    static constexpr int O_SO = O_NET + tch::NET;                  // [ROWS][SOS] raw obs (component 11 = 1)
    static constexpr int O_TO = O_SO + ROWS * tch::SOS;            // [ROWS][4] the teacher's pdflat
    static constexpr int LDS_FLOATS = O_TO + ROWS * RDM_OUT;       // 30,172 floats = 118 KiB at 64 rows
    static_assert(O_NET % 4 == 0 && O_SO % 4 == 0 && THREADS <= 1024 && LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
};

struct SmEvalArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* img;        // the student's weight image [IMG]
    const float* draws;      // [E][n][6] or null (Philox)
    float* returns;          // [E][n]
    float* final_dist;       // [E][n] or null
    float* records;          // [E][n][50][EREC] or null
    int episodes, first_episode;
};

template <int ROWS, bool BF>
__global__ __launch_bounds__(ELay<ROWS>::THREADS) void student_mlp_evaluate_kernel(SmEvalArgs a) {
    using LY = Lay<ROWS>;
    using EL = ELay<ROWS>;
    constexpr int RB = LY::RB;
    __shared__ __attribute__((aligned(16))) float lds[EL::LDS_FLOATS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    float* X0 = lds + LY::O_X0;
    float* X1 = lds + LY::O_X1;
    float* X2 = lds + LY::O_X2;
    float* X3 = lds + LY::O_X3;
    float* X4 = lds + LY::O_X4;
    float* D5 = lds + LY::O_D5;
    float* LT = lds + EL::O_NET;
    float* SO = lds + EL::O_SO;
    float* TO = lds + EL::O_TO;
    tch::load_net(LT, a.tnet, false, EL::THREADS);   // published by the first step's barriers
    const bool student = wave < WAVES;               // wave-uniform
    const bool phys = wave == 0 && lane < ROWS;      // the env of this lane
    const int64_t n = a.n, nblk = (n + ROWS - 1) / ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * ROWS;
        const bool valid = phys && row0 + lane < n;
        const int64_t env = row0 + (valid ? lane : 0);   // a ragged block's spare lanes repeat its env 0
        rd::State st;
        float carry = 0.0f;   // the reward this env's previous step returned
        for (int e = 0; e < a.episodes; ++e) {
            float ret = 0.0f, prev_field = 0.0f, tp[RDM_OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
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
            float* rec = a.records && valid ? a.records + ((int64_t)e * n + env) * (rd::kEpisodeSteps * EREC) : nullptr;
            for (int s = 0; s < rd::kEpisodeSteps; ++s) {
                if (phys) {   // row s = ob | T_{s-1} | record s-1's reward field (zeros at s = 0)
                    float ob[rd::kObsDim];
                    rd::observe<true>(st, ob);
#pragma unroll
                    for (int k = 0; k < rd::kObsDim; ++k) {
                        SO[lane * tch::SOS + k] = ob[k];
                        X0[lane * S_X0 + pk(k)] = ob[k];
                    }
                    SO[lane * tch::SOS + tch::OBD] = 1.0f;
#pragma unroll
                    for (int c = 0; c < RDM_OUT; ++c) X0[lane * S_X0 + pk(rd::kObsDim + c)] = s ? tp[c] : 0.0f;
                    X0[lane * S_X0 + pk(RDM_IN - 1)] = s ? prev_field : 0.0f;
                    if (rec) {
                        float* r = rec + s * EREC;
#pragma unroll
                        for (int k = 0; k < rd::kObsDim; ++k) r[k] = ob[k];
                        r[rd::kObsDim] = carry;
                        r[EREC - 1] = 1.0f;
                    }
                    prev_field = carry;
                }
                __syncthreads();
                if (student) fwd<BF, RB, 0, S_X0, S_X1>(X0, X1, a.img, wave, i, g);
                __syncthreads();
                if (student) fwd<BF, RB, 1, S_X1, S_X2>(X1, X2, a.img, wave, i, g);
                __syncthreads();
                if (student) {
                    fwd<BF, RB, 2, S_X2, S_X3>(X2, X3, a.img, wave, i, g);
                } else {   // the teacher on tile wave - 8, beside the student's largest layer
                    const int t = wave - WAVES;
                    f32x4 H1[4], H2[4];
                    float m0, m1;
                    tch::mlp_forward<true>(LT, SO + t * 16 * tch::SOS, i, g, H1, H2, m0, m1);
                    if (g == 0) {
                        float* o = TO + (t * 16 + i) * RDM_OUT;
                        o[0] = m0; o[1] = m1; o[2] = LT[tch::N_LS]; o[3] = LT[tch::N_LS + 1];
                    }
                }
                __syncthreads();
                if (student) fwd<BF, RB, 3, S_X3, S_X4>(X3, X4, a.img, wave, i, g);
                __syncthreads();
                if (student) fwd<BF, RB, 4, S_X4, S_D5>(X4, D5, a.img, wave, i, g);
                __syncthreads();
                // the next step's first writes (X0, SO) follow every read of them: X0's before the
                // second barrier above, SO's before the fourth
                if (phys) {
                    float sp[RDM_OUT];
#pragma unroll
                    for (int c = 0; c < RDM_OUT; ++c) {
                        sp[c] = D5[lane * S_D5 + pk(c)];
                        tp[c] = TO[lane * RDM_OUT + c];
                    }
                    if (rec) {
                        float* r = rec + s * EREC + rd::kObsDim + 1;
#pragma unroll
                        for (int c = 0; c < RDM_OUT; ++c) {
                            r[c] = tp[c];
                            r[RDM_OUT + c] = sp[c];
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
    }
}
