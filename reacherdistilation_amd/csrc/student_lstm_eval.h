// student_lstm.hip's whole-episode evaluation (rdl_evaluate, include/reacher_student_lstm.h): one
// rollout launch rolls n evaluation envs through E consecutive 50-step episodes under the LSTM
// student's mean action (DESIGN.md §3 "Evaluation of the LSTM student"): the query loop of
// lstm_train.train without the optimiser steps.  Included inside student_lstm.hip's anonymous
// namespace after student_lstm_query.h and student_lstm_query_bf16.h, whose step it runs: the workgroup's layout, the tiling and
// the pieces of a step are there.
//
// This kernel's own: a workgroup owns its block of 16 envs for the whole launch; an env's state,
// return and carried reward stay in registers (lanes 0..15 of wave 0) over the E episodes, each
// begun by rd::env_reset from the caller's draws or Philox; (c, h) starts from state0 or zero and
// is carried over the resets.  The dense part of an x row is formed once per record: the
// parameters are fixed for the call.
// No env depends on another (an MFMA row, a lane): no grid barrier, no hand-off between workgroups.
// Every operation is the stepwise forward's in its order, so the outputs are bitwise those of
// rd_reset, then 50 x { rdd_forward, the window, rdl_forward, rd_step }, whatever the grid.
#pragma once

struct LsEvalArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* P;          // the student's flat parameters
    const float* img;        // lstm_eval_pack_kernel's image of Wl [EV_IMG]; BF16Q: the bf16 image WF
    const float* draws;      // [E][n][6] or null (Philox)
    const float* state0;     // [2][n][U] = (c, h) or null (zeros)
    float* returns;          // [E][n]
    float* final_dist;       // [E][n] or null
    float* records;          // [E][n][50][EV_REC] or null
    float* state_out;        // [2][n][U] or null
    int episodes, first_episode, T;
};

// BF16Q: the positions run on the bf16 cell (student_lstm_query_bf16.h; a.img is then the handle's WF image)
// rdl_evaluate_noisy's instances (student_lstm_noise.hip), told by their argument struct: the student's
// action perturbed (include/reacher_action_noise.h) at Philox episode first_episode + e, with or
// without a draws table; the draws are taken in the env's lane before the step's first barrier
struct LsEvalNoiseArgs : LsEvalArgs {
    int32_t noise_mode;      // RD_NOISE_POLICY or RD_NOISE_FIXED
    float noise_scale;
    uint64_t noise_seed;
};

// rdl_evaluate_faulty's instances (student_lstm_faults.hip): the student reads its observations through
// the sensor faults (include/reacher_obs_faults.h) at Philox episode first_episode + e; its action may
// be perturbed too (noise_mode = RD_NOISE_NONE: the mean acts).  The env's lane masks record s in the
// ring (ls_fault_mask) beside the noise, before the step's first barrier; the record keeps that mask in
// the later windows that hold it.  The teacher's row and the records keep the clean observation
struct LsEvalFaultArgs : LsEvalNoiseArgs {
    int32_t obs_mode;        // RD_OBS_DROPOUT or RD_OBS_MISSING
    float obs_keep;          // keep_prob
    uint64_t obs_seed;
};

// What an instance does follows from its argument struct alone, as the envs kernel's EnvsActs
template <class ARGS>
struct EvalActs {
    static constexpr bool noisy = std::is_base_of_v<LsEvalNoiseArgs, ARGS>;
    static constexpr bool faulty = std::is_base_of_v<LsEvalFaultArgs, ARGS>;
};

// ARGS for a call: the plain instance's arguments, then the fields ARGS adds from the call's settings
template <class ARGS>
ARGS acting_args(const LsEvalArgs& base, const rd::Acting& act) {
    ARGS m{};
    static_cast<LsEvalArgs&>(m) = base;
    if constexpr (EvalActs<ARGS>::noisy) {
        m.noise_mode = act.noise.mode;
        m.noise_scale = act.noise.scale;
        m.noise_seed = act.noise.seed;
    }
    if constexpr (EvalActs<ARGS>::faulty) {
        m.obs_mode = act.faults.mode;
        m.obs_keep = act.faults.keep_prob;
        m.obs_seed = act.faults.seed;
    }
    return m;
}

template <bool BF16Q, class ARGS = LsEvalArgs>
__global__ __launch_bounds__(EV_THREADS) void student_lstm_evaluate_kernel(ARGS a) {
    const LsThread q = ls_prologue(a.tnet, a.P, a.img, a.T);
    const int tid = q.tid, lane = q.lane, T = q.T;
    const bool phys = q.wave == 0 && lane < EV_ROWS;   // the env of this lane
    const int64_t n = a.n, nblk = (n + EV_ROWS - 1) / EV_ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * EV_ROWS;
        const bool valid = phys && row0 + lane < n;
        const int64_t env = row0 + (valid ? lane : 0);   // a ragged block's spare lanes repeat its env 0
        __syncthreads();   // the previous block's last reads of c and h
        ls_state_load(tid, a.state0, n, row0);   // the call's initial state
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
            float* rec0 = a.records && valid ? a.records + ((int64_t)e * n + env) * (rd::kEpisodeSteps * EV_REC) : nullptr;
            for (int s = 0; s < rd::kEpisodeSteps; ++s) {
                const int slot = s % T;
                float* rec = rec0 ? rec0 + s * EV_REC : nullptr;
                if constexpr (EvalActs<ARGS>::noisy) {
                    if (phys && (!EvalActs<ARGS>::faulty || a.noise_mode != 0))   // a faulty call's noise may be off
                        ls_noise_draw(lane, a.noise_seed, (uint64_t)(a.env_base + env), a.first_episode + e, s);
                }
                if (phys) ls_record_head(lane, slot, st, rec, carry, 1.0f);
                if constexpr (EvalActs<ARGS>::faulty) {
                    if (phys)
                        ls_fault_mask(lane, slot, a.obs_mode, a.obs_keep, a.obs_seed, (uint64_t)(a.env_base + env),
                                      a.first_episode + e, s, nullptr);
                }
                // prev . Wp + bp of record s: prev = T_{s-1}, zero at s = 0
                lds::Xr[slot][q.dr][11 + q.dc] = ls_dense(q, s != 0, lds::TO[(s - 1) & 1][q.dr]);
                __syncthreads();
                ls_teacher(q, s);
                hp = ls_positions_of<BF16Q>(q, s, hp);
                ls_head<BF16Q>(q, hp);
                // the next step's first writes (SO, the ring's slot, TO's other parity) follow every
                // read of them: the barriers above
                if (phys) {
                    float sp[4], tp[4];
                    ls_record_tail(lane, s, rec, tp, sp);
                    if constexpr (EvalActs<ARGS>::noisy) {
                        const float xi0 = ls_noise_park()[2 * lane], xi1 = ls_noise_park()[2 * lane + 1];
                        float a0, a1;
                        rd::action_noise_apply(a.noise_mode, a.noise_scale, xi0, xi1, sp[0], sp[1], sp[2], sp[3], a0, a1);
                        carry = rd::env_step<true>(st, a0, a1);
                    } else {
                        carry = rd::env_step<true>(st, sp[0], sp[1]);
                    }
                    ret += carry;
                }
            }
            if (valid) {
                a.returns[(int64_t)e * n + env] = ret;
                if (a.final_dist) a.final_dist[(int64_t)e * n + env] = rd::tip_distance(st);
            }
        }
        if (a.state_out) ls_state_store(tid, a.state_out, n, row0, hp);   // (c, h) after the call's last query
    }
}
