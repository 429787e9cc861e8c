// One closed-loop step of the reference MLP student on a block of ROWS envs: what
// student_mlp_evaluate_kernel (student_mlp_eval.h) and student_mlp_envs_kernel (student_mlp_envs.h)
// both run, once.  Included inside student_mlp.hip's anonymous namespace after student_mlp_layers.h
// (fwd); expects rd_device.h, rd_physics.h and student_mlp_layout.h's Lay<ROWS>.
//
// A workgroup owns a block of ROWS envs (64, or 16 for a small batch) for the whole launch:
//  * wave 0 keeps the envs, one per lane (rd::observe<true>, rd::env_step<true>: rd_step's functions);
//  * waves 0..7 run the student's layers on the block exactly as student_mlp_kernel's forward does
//    (fwd on the trainer's weight image, the activations in LDS between the layers);
//  * waves 8.. (one per 16-env tile) run the teacher, mlp_forward<true> on the load_net image
//    (forward_kernel's, kept in LDS for the launch).  T_s is needed only by step s + 1's row and by
//    the records, so it runs beside the student's largest layer (128 x 128).
// The two kernels call qs_row, qs_layers and qs_outputs in this order, with the barriers where
// qs_layers has them; what differs between them is a template argument here (whether the student
// acts, layer 1's SrcC fence) or stays in the kernel (where the row and the outputs are written).
// The block's LDS is passed as its base; every buffer is a constant offset from it (Lay, ELay).
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

// Row s of this lane's env = ob | T_{s-1} | record s-1's reward field (zeros at s = 0): the raw obs
// into the teacher's rows SO and, when the student acts, the row into X0.  The stores to SO and X0
// alternate, as the evaluation kernel had them: with all of SO first (the envs kernel's order) hipcc
// lays the 64-env evaluation instances out anew and the bf16 one runs 1 % slower at 262,144 envs
// (profiles/student_mlp_split_timing.txt)
template <int ROWS, bool STUDENT_ACTS>
__device__ __forceinline__ void qs_row(float* lds, int lane, const rd::State& st, int s, const float (&tp)[RDM_OUT],
                                       float prev_field, float (&row)[RDM_IN]) {
    float* X0 = lds + Lay<ROWS>::O_X0;
    float* SO = lds + ELay<ROWS>::O_SO;
    rd::observe<true>(st, row);
#pragma unroll
    for (int c = 0; c < RDM_OUT; ++c) row[rd::kObsDim + c] = s ? tp[c] : 0.0f;
    row[RDM_IN - 1] = s ? prev_field : 0.0f;
#pragma unroll
    for (int c = 0; c < rd::kObsDim; ++c) {
        SO[lane * tch::SOS + c] = row[c];
        if constexpr (STUDENT_ACTS) X0[lane * S_X0 + pk(c)] = row[c];
    }
    SO[lane * tch::SOS + tch::OBD] = 1.0f;
    if constexpr (STUDENT_ACTS) {
#pragma unroll
        for (int c = rd::kObsDim; c < RDM_IN; ++c) X0[lane * S_X0 + pk(c)] = row[c];
    }
}

// The step's layers behind the rows' barrier: the student's five (STUDENT_ACTS; a barrier behind
// each) and the teacher on tile wave - 8 beside layer 2.  STUDENT_ACTS = false: the student's waves
// run no layer and the step has two barriers instead of six.  FENCE1: layer 1's SrcC fence.
// The next step's first writes (X0, SO) follow every read of them: X0's before the second barrier,
// SO's before the teacher's.
template <int ROWS, bool STUDENT_ACTS, bool BF, bool FENCE1>
__device__ __forceinline__ void qs_layers(float* lds, const float* img, int wave, int i, int g) {
    using LY = Lay<ROWS>;
    using EL = ELay<ROWS>;
    constexpr int RB = LY::RB;
    float* X0 = lds + LY::O_X0;
    float* X1 = lds + LY::O_X1;
    float* X2 = lds + LY::O_X2;
    float* X3 = lds + LY::O_X3;
    float* X4 = lds + LY::O_X4;
    float* D5 = lds + LY::O_D5;
    float* LT = lds + EL::O_NET;
    float* SO = lds + EL::O_SO;
    float* TO = lds + EL::O_TO;
    const bool student = wave < WAVES;   // wave-uniform
    __syncthreads();
    if constexpr (STUDENT_ACTS) {
        if (student) fwd<BF, RB, 0, S_X0, S_X1>(X0, X1, img, wave, i, g);
        __syncthreads();
        if (student) fwd<BF, RB, 1, S_X1, S_X2, FENCE1>(X1, X2, img, wave, i, g);
        __syncthreads();
    }
    if (student) {
        if constexpr (STUDENT_ACTS) fwd<BF, RB, 2, S_X2, S_X3>(X2, X3, img, wave, i, g);
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
    if constexpr (STUDENT_ACTS) {
        if (student) fwd<BF, RB, 3, S_X3, S_X4>(X3, X4, img, wave, i, g);
        __syncthreads();
        if (student) fwd<BF, RB, 4, S_X4, S_D5>(X4, D5, img, wave, i, g);
        __syncthreads();
    }
}

// Step s's two pdflats at this lane's env: tp = T_s, sp = the student's row of D5 (no STUDENT_ACTS:
// zeros, the teacher steps)
template <int ROWS, bool STUDENT_ACTS>
__device__ __forceinline__ void qs_outputs(const float* lds, int lane, float (&sp)[RDM_OUT], float (&tp)[RDM_OUT]) {
    const float* D5 = lds + Lay<ROWS>::O_D5;
    const float* TO = lds + ELay<ROWS>::O_TO;
#pragma unroll
    for (int c = 0; c < RDM_OUT; ++c) {
        sp[c] = STUDENT_ACTS ? D5[lane * S_D5 + pk(c)] : 0.0f;
        tp[c] = TO[lane * RDM_OUT + c];
    }
}
