// student_mlp.hip's persistent envs (rdm_envs_*, rdm_step_envs, include/reacher_student_mlp.h):
// one launch takes the handle's n envs through K lockstep env steps under the teacher's or the
// reference student's mean action and writes the K n training rows and their teacher targets,
// which the training launch (student_mlp_kernel<true>) then reads as any caller's rows (DESIGN.md
// §3 "On-policy distillation of the reference student").  Included inside student_mlp.hip's
// anonymous namespace after student_mlp_eval.h: tch::, ELay and EREC's row layout are its.
//
// It is student_mlp_evaluate_kernel with the envs kept between launches.  A workgroup owns a block
// of ROWS envs (64, or 16 for a small batch) for the launch:
//  * wave 0 keeps the envs, one per lane.  State, carried reward, the previous record's reward
//    field, the teacher's previous pdflat and the clock (step 0..49, episode) are loaded from the
//    handle's device arrays at entry and written back at exit; between, they are registers;
//  * waves 0..7 run the student's layers (fwd_layer on the trainer's weight image);
//  * waves 8.. (one per 16-env tile) run the teacher, mlp_forward<true> on the load_net image,
//    beside the student's layer 2.
// STUDENT_ACTS = false (the driver's phase 1: the teacher steps the envs): the student's waves run
// no layer, s_pdflat is written as 0, and a step has two barriers instead of six.
// After an env's step 49 it resets from Philox(seed, env_base + i, episode + 1), inside the step
// as rd_step does, so the state at exit is rd_get_state's after the same steps.  The clock is the
// device's: no host-side count enters the arguments, and a captured launch replays the next steps.
// Every env's chain depends on no other env and every function is the stepwise path's in its
// order, so the outputs are bitwise those of K x { rdd_forward (teacher), rdm_forward on the
// assembled row, rd_step }, whatever ROWS, the grid and the split of the steps over launches.
#pragma once

constexpr int ENV_AUX = 2 + RDM_OUT;   // per env, SoA rows: carried reward | prev reward field | prev T[4]

struct SmEnvsArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* img;        // the student's weight image [IMG]
    float* state;            // [8][n] SoA (rd_get_state's layout)
    float* aux;              // [ENV_AUX][n]
    int32_t* clock;          // [2][n]: step of the episode, episode
    float* x;                // [K][n][16] the undropped rows
    float* t_pdflat;         // [K][n][4]
    float* s_pdflat;         // [K][n][4] or null
    float* reward;           // [K][n] or null
    int steps;               // K
};

// episode 0 of every env; clocks, carried reward and previous fields to 0 (rd_reset's arithmetic)
__global__ __launch_bounds__(256) void student_mlp_envs_reset_kernel(SmEnvsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    float d[6];
    rd::philox_draw(a.seed, (uint64_t)(a.env_base + i), 0u, d);
    rd::State st;
    rd::env_reset(st, d);
    rd::store_state(a.state, a.n, i, st);
#pragma unroll
    for (int k = 0; k < ENV_AUX; ++k) a.aux[k * a.n + i] = 0.0f;
    a.clock[i] = 0;
    a.clock[a.n + i] = 0;
}

template <int ROWS, bool STUDENT_ACTS, bool BF>
__global__ __launch_bounds__(ELay<ROWS>::THREADS) void student_mlp_envs_kernel(SmEnvsArgs a) {
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
        float carry = 0.0f;        // the reward this env's previous step returned
        float prev_field = 0.0f;   // the previous record's reward field
        float tp[RDM_OUT] = {0.0f, 0.0f, 0.0f, 0.0f};
        int32_t s = 0, episode = 0;
        if (phys) {
            rd::load_state(a.state, n, env, st);
            carry = a.aux[env];
            prev_field = a.aux[n + env];
#pragma unroll
            for (int c = 0; c < RDM_OUT; ++c) tp[c] = a.aux[(2 + c) * n + env];
            s = a.clock[env];
            episode = a.clock[n + env];
        }
        for (int k = 0; k < a.steps; ++k) {
            const int64_t out = (int64_t)k * n + env;   // row of this env's k-th step of the call
            if (phys) {   // row s = ob | T_{s-1} | record s-1's reward field (zeros at s = 0)
                float row[RDM_IN];
                rd::observe<true>(st, row);
#pragma unroll
                for (int c = 0; c < RDM_OUT; ++c) row[rd::kObsDim + c] = s ? tp[c] : 0.0f;
                row[RDM_IN - 1] = s ? prev_field : 0.0f;
#pragma unroll
                for (int c = 0; c < rd::kObsDim; ++c) SO[lane * tch::SOS + c] = row[c];
                SO[lane * tch::SOS + tch::OBD] = 1.0f;
                if (STUDENT_ACTS) {
#pragma unroll
                    for (int c = 0; c < RDM_IN; ++c) X0[lane * S_X0 + pk(c)] = row[c];
                }
                if (valid) {
                    f32x4* xo = reinterpret_cast<f32x4*>(a.x + out * RDM_IN);
#pragma unroll
                    for (int q = 0; q < RDM_IN / 4; ++q)
                        xo[q] = f32x4{row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]};
                }
                prev_field = carry;
            }
            __syncthreads();
            if constexpr (STUDENT_ACTS) {
                if (student) fwd<BF, RB, 0, S_X0, S_X1>(X0, X1, a.img, wave, i, g);
                __syncthreads();
                // fenced: in the 64-env instance hipcc loaded layer 1's next weights into the bias quad its
                // four row blocks' first MFMAs share as SrcC (hazards.py LDSRC).  Fencing every layer
                // scans clean too and costs 2-3 % of the launch (profiles/student_mlp_envs_fence_ab.txt)
                if (student) fwd<BF, RB, 1, S_X1, S_X2, true>(X1, X2, a.img, wave, i, g);
                __syncthreads();
            }
            if (student) {
                if constexpr (STUDENT_ACTS) fwd<BF, RB, 2, S_X2, S_X3>(X2, X3, a.img, wave, i, g);
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
                if (student) fwd<BF, RB, 3, S_X3, S_X4>(X3, X4, a.img, wave, i, g);
                __syncthreads();
                if (student) fwd<BF, RB, 4, S_X4, S_D5>(X4, D5, a.img, wave, i, g);
                __syncthreads();
            }
            // the next step's first writes (X0, SO) follow every read of them: X0's before the
            // second barrier above, SO's before the teacher's barrier
            if (phys) {
                float sp[RDM_OUT];
#pragma unroll
                for (int c = 0; c < RDM_OUT; ++c) {
                    sp[c] = STUDENT_ACTS ? D5[lane * S_D5 + pk(c)] : 0.0f;
                    tp[c] = TO[lane * RDM_OUT + c];
                }
                carry = STUDENT_ACTS ? rd::env_step<true>(st, sp[0], sp[1]) : rd::env_step<true>(st, tp[0], tp[1]);
                if (valid) {
                    *reinterpret_cast<f32x4*>(a.t_pdflat + out * RDM_OUT) = f32x4{tp[0], tp[1], tp[2], tp[3]};
                    if (a.s_pdflat) {
#pragma unroll
                        for (int c = 0; c < RDM_OUT; ++c) a.s_pdflat[out * RDM_OUT + c] = sp[c];
                    }
                    if (a.reward) a.reward[out] = carry;
                }
                if (++s == rd::kEpisodeSteps) {   // TimeLimit: the env resets inside its last step
                    float d[6];
                    s = 0;
                    ++episode;
                    rd::philox_draw(a.seed, (uint64_t)(a.env_base + env), (uint32_t)episode, d);
                    rd::env_reset(st, d);
                }
            }
        }
        if (valid) {
            rd::store_state(a.state, n, env, st);
            a.aux[env] = carry;
            a.aux[n + env] = prev_field;
#pragma unroll
            for (int c = 0; c < RDM_OUT; ++c) a.aux[(2 + c) * n + env] = tp[c];
            a.clock[env] = s;
            a.clock[n + env] = episode;
        }
    }
}
