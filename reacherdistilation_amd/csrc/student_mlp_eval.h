// student_mlp.hip's whole-episode evaluation (rdm_evaluate, include/reacher_student_mlp.h): one
// launch rolls n evaluation envs through E consecutive 50-step episodes under the reference
// student's mean action (DESIGN.md §3 "Evaluation of the reference student").  Included inside
// student_mlp.hip's anonymous namespace after student_mlp_query.h: the step (the block's LDS, who
// runs what, the barriers) is its, with the student acting and layer 1 unfenced.
//
// A workgroup owns a block of ROWS envs for the whole launch; wave 0 keeps them, one per lane: state,
// return and the carried reward in registers (rd::env_reset, rd::env_step<true>: rd_reset / rd_step's
// functions).  Every env's chain depends on no other env (an MFMA row, a lane), and every function
// is the stepwise path's, so the outputs are bitwise those of rd_reset, then 50 x { rdd_forward,
// rdm_forward on the assembled row, rd_step }, whatever ROWS and the grid.
#pragma once

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

// rdm_evaluate_noisy's instances (student_mlp_noise.hip), told by their argument struct: the student's
// action perturbed (include/reacher_action_noise.h) at Philox episode first_episode + e, with or
// without a draws table; the draws are taken in the env's lane before the step's first barrier
struct SmEvalNoiseArgs : SmEvalArgs {
    int32_t noise_mode;      // RD_NOISE_POLICY or RD_NOISE_FIXED
    float noise_scale;
    uint64_t noise_seed;
};

// rdm_evaluate_faulty's instances (student_mlp_faults.hip): the student reads its observation through
// the sensor faults (include/reacher_obs_faults.h) at Philox episode first_episode + e; its action may
// be perturbed too (noise_mode = RD_NOISE_NONE: the mean acts).  The env's lane draws the keep bits
// beside the noise and overwrites the observation part of its X0 row; the teacher's row and the
// records keep the clean registers
struct SmEvalFaultArgs : SmEvalNoiseArgs {
    int32_t obs_mode;        // RD_OBS_DROPOUT or RD_OBS_MISSING
    float obs_keep;          // keep_prob
    uint64_t obs_seed;
};

// What an instance does follows from its argument struct alone, as the envs kernel's EnvsActs
template <class ARGS>
struct EvalActs {
    static constexpr bool noisy = std::is_base_of_v<SmEvalNoiseArgs, ARGS>;
    static constexpr bool faulty = std::is_base_of_v<SmEvalFaultArgs, ARGS>;
};

// ARGS for a call: the plain instance's arguments, then the fields ARGS adds from the call's settings
template <class ARGS>
ARGS acting_args(const SmEvalArgs& base, const rd::Acting& act) {
    ARGS m{};
    static_cast<SmEvalArgs&>(m) = base;
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

template <int ROWS, bool BF, class ARGS = SmEvalArgs>
__global__ __launch_bounds__(ELay<ROWS>::THREADS) void student_mlp_evaluate_kernel(ARGS a) {
    // EvalActs::noisy: the step's draws.  The kernel's first locals, as student_mlp_envs_kernel's coin is:
    // declared inside the step loop they move hipcc's register names in the four plain instances
    float xi0 = 0.0f, xi1 = 0.0f;
    __shared__ __attribute__((aligned(16))) float lds[ELay<ROWS>::LDS_FLOATS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    tch::load_net(lds + ELay<ROWS>::O_NET, a.tnet, false, ELay<ROWS>::THREADS);   // published by the first step's barriers
    const bool phys = wave == 0 && lane < ROWS;   // the env of this lane
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
                if (phys) {
                    if constexpr (EvalActs<ARGS>::noisy) {
                        if (!EvalActs<ARGS>::faulty || a.noise_mode != 0)   // a faulty call's noise may be off
                            rd::action_noise_draw(a.noise_seed, (uint64_t)(a.env_base + env), a.first_episode + e, s, xi0, xi1);
                    }
                    float row[RDM_IN];
                    qs_row<ROWS, true>(lds, lane, st, s, tp, prev_field, row);
                    if constexpr (EvalActs<ARGS>::faulty) {
                        const uint32_t keep = rd::obs_fault_keep(a.obs_seed, (uint64_t)(a.env_base + env),
                                                                 a.first_episode + e, s, a.obs_keep);
                        float* X0 = lds + Lay<ROWS>::O_X0;
#pragma unroll
                        for (int c = 0; c < rd::kObsDim; ++c)
                            X0[lane * S_X0 + pk(c)] = rd::obs_fault_see(a.obs_mode, a.obs_keep, keep, c, row[c]);
                    }
                    if (rec) {
                        float* r = rec + s * EREC;
#pragma unroll
                        for (int k = 0; k < rd::kObsDim; ++k) r[k] = row[k];
                        r[rd::kObsDim] = carry;
                        r[EREC - 1] = 1.0f;
                    }
                    prev_field = carry;
                }
                // (the noisy instances run layer 1 fenced, as the envs kernel does: unfenced, the 64-env f32
                // one had the loads into an in-flight MFMA's SrcC that student_mlp_envs.h describes)
                qs_layers<ROWS, true, BF, EvalActs<ARGS>::noisy>(lds, a.img, wave, i, g);
                if (phys) {
                    float sp[RDM_OUT];
                    qs_outputs<ROWS, true>(lds, lane, sp, tp);
                    if (rec) {
                        float* r = rec + s * EREC + rd::kObsDim + 1;
#pragma unroll
                        for (int c = 0; c < RDM_OUT; ++c) {
                            r[c] = tp[c];
                            r[RDM_OUT + c] = sp[c];
                        }
                    }
                    if constexpr (EvalActs<ARGS>::noisy) {
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
    }
}
