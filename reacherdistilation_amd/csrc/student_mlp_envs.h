// student_mlp.hip's persistent envs (rdm_envs_*, rdm_step_envs, include/reacher_student_mlp.h):
// one launch takes the handle's n envs through K lockstep env steps under the teacher's or the
// reference student's mean action and writes the K n training rows and their teacher targets,
// which the training launch (student_mlp_kernel<true>) then reads as any caller's rows (DESIGN.md
// §3 "On-policy distillation of the reference student").  Included inside student_mlp.hip's
// anonymous namespace after student_mlp_query.h: the step (the block's LDS, who runs what, the
// barriers) and the row's layout are its.
//
// It is student_mlp_evaluate_kernel with the envs kept between launches.  A workgroup owns a block
// of ROWS envs (64, or 16 for a small batch) for the launch; wave 0 keeps them, one per lane.
// State, carried reward, the previous record's reward field, the teacher's previous pdflat and the
// clock (step 0..49, episode) are loaded from the handle's device arrays at entry and written back
// at exit; between, they are registers.
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

// the mixed instances' (rdm_envs_set_teacher_share).  A struct of its own: a longer SmEnvsArgs moves
// the kernels' implicit arguments and hipcc then lays the other instances out anew
struct SmEnvsMixArgs : SmEnvsArgs {
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    float* stepped_with;     // [K][n] or null: 1 where the student's action stepped the env, else 0
};

// the noisy instances' (rdm_envs_set_action_noise, rdm_envs_bind_actions), compiled in
// student_mlp_noise.hip.  Again a struct of its own; the instances are told by it (EnvsActs), so the
// kernel's other template parameters, and with them every other instance's name, stay as they are
struct SmEnvsNoiseArgs : SmEnvsMixArgs {
    int32_t noise_mode;      // RD_NOISE_* (include/reacher_action_noise.h)
    float noise_scale;
    uint64_t noise_seed;     // the noise's Philox key
    float* actions;          // [K][n][2] or null: the action that stepped the env
};

// the faulty instances' (rdm_envs_set_obs_faults: sensor faults on the student's observation,
// include/reacher_obs_faults.h), compiled in student_mlp_faults.hip.  Derived from the noisy one, so
// one faulty instance carries beta, the action noise and the faults as run-time arguments
struct SmEnvsFaultArgs : SmEnvsNoiseArgs {
    int32_t obs_mode;        // RD_OBS_* (include/reacher_obs_faults.h)
    float obs_keep;          // keep_prob
    uint64_t obs_seed;       // the mask's Philox key
};

// What an instance does follows from its argument struct alone: each struct above adds its fields to
// the one before, and an instance carries whatever its struct derives from (with the student acting,
// for the mixture: the teacher-acting noisy instance has beta's fields and never reads them)
template <class ARGS>
struct EnvsActs {
    static constexpr bool mixed = std::is_base_of_v<SmEnvsMixArgs, ARGS>;
    static constexpr bool noisy = std::is_base_of_v<SmEnvsNoiseArgs, ARGS>;
    static constexpr bool faulty = std::is_base_of_v<SmEnvsFaultArgs, ARGS>;
};

// ARGS for a call: the plain instance's arguments, then the fields ARGS adds from the handle's settings
template <class ARGS>
ARGS acting_args(const SmEnvsArgs& base, const rd::Acting& act) {
    ARGS m{};
    static_cast<SmEnvsArgs&>(m) = base;
    if constexpr (EnvsActs<ARGS>::mixed) {
        m.beta = act.beta;
        m.coin_seed = act.coin_seed;
        m.stepped_with = act.stepped_with;
    }
    if constexpr (EnvsActs<ARGS>::noisy) {
        m.noise_mode = act.noise.mode;
        m.noise_scale = act.noise.scale;
        m.noise_seed = act.noise.seed;
        m.actions = act.actions;
    }
    if constexpr (EnvsActs<ARGS>::faulty) {
        m.obs_mode = act.faults.mode;
        m.obs_keep = act.faults.keep_prob;
        m.obs_seed = act.faults.seed;
    }
    return m;
}

// episode 0 of every env; clocks, carried reward and previous fields to 0 (rd_reset's arithmetic)
__global__ __launch_bounds__(256) void student_mlp_envs_reset_kernel(SmEnvsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) rd::envs_reset_one<ENV_AUX>(a.state, a.aux, a.clock, a.n, i, a.seed, a.env_base);
}

// The step is student_mlp_query.h's.  Layer 1 runs fenced: in the 64-env instance hipcc loaded its
// next weights into the bias quad its four row blocks' first MFMAs share as SrcC (hazards.py LDSRC).
// Fencing every layer scans clean too and costs 2-3 % of the launch
// (profiles/student_mlp_envs_fence_ab.txt)
// MIXED (with STUDENT_ACTS; DAgger's beta-mixture): the student instance's step, every layer, barrier
// and fence of it, and per env step a coin in the env's lane -- rd::teacher_coin, a function of
// (coin seed, env, episode, step) alone, drawn before the step's first barrier so that it runs beside
// the layers -- that hands the teacher's T_s[0..1] to env_step instead of S_s[0..1].  x, t_pdflat and
// s_pdflat are written as the student instance writes them; the coin goes to stepped_with.
// Acts::noisy (action noise; a student instance is then MIXED too, beta = 0 never firing; a teacher
// instance is not): the two normal draws of this env and step in the env's lane, beside the coin
// (rd::action_noise_draw), and env_step takes rd::action_noise_apply of them and the acting pdflat --
// T_s where the teacher acts, S_s else -- instead of its mean; that action goes to `actions`.
// Nothing else of the step changes.
// Acts::faulty (sensor faults; a student instance, MIXED and noisy too, either of which may be off at
// run time): the env's lane draws this record's keep bits beside the coin and the noise
// (rd::obs_fault_keep, three Philox calls before the step's first barrier) and overwrites the
// observation part of its X0 row with rd::obs_fault_see of them.  Only the student's layer 0 reads X0:
// the teacher's SO row, x and every other output keep the clean registers.
template <int ROWS, bool STUDENT_ACTS, bool BF, class ARGS = SmEnvsArgs>
__global__ __launch_bounds__(ELay<ROWS>::THREADS) void student_mlp_envs_kernel(ARGS a) {
    // MIXED: the teacher steps this lane's env now.  The kernel's first local: declared inside the step
    // loop it moves hipcc's layout of the six instances that never read it
    // (profiles/envs_teacher_share_isa.txt)
    bool coin = false;
    float xi0 = 0.0f, xi1 = 0.0f;   // Acts::noisy: this step's draws, declared here for the same reason
    __shared__ __attribute__((aligned(16))) float lds[ELay<ROWS>::LDS_FLOATS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    tch::load_net(lds + ELay<ROWS>::O_NET, a.tnet, false, ELay<ROWS>::THREADS);   // published by the first step's barriers
    const bool phys = wave == 0 && lane < ROWS;   // the env of this lane
    using Acts = EnvsActs<ARGS>;
    constexpr bool MIXED = STUDENT_ACTS && Acts::mixed;   // the mixture is a student call's
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
            if (phys) {
                if constexpr (MIXED)
                    coin = rd::teacher_coin(a.coin_seed, (uint64_t)(a.env_base + env), episode, s, a.beta);
                if constexpr (Acts::noisy) {
                    if (!Acts::faulty || a.noise_mode != 0)   // a faulty call's noise may be off
                        rd::action_noise_draw(a.noise_seed, (uint64_t)(a.env_base + env), episode, s, xi0, xi1);
                }
                float row[RDM_IN];
                qs_row<ROWS, STUDENT_ACTS>(lds, lane, st, s, tp, prev_field, row);
                if constexpr (Acts::faulty) {
                    static_assert(STUDENT_ACTS, "the faults are on what the student reads");
                    const uint32_t keep = rd::obs_fault_keep(a.obs_seed, (uint64_t)(a.env_base + env), episode, s, a.obs_keep);
                    float* X0 = lds + Lay<ROWS>::O_X0;
#pragma unroll
                    for (int c = 0; c < rd::kObsDim; ++c)
                        X0[lane * S_X0 + pk(c)] = rd::obs_fault_see(a.obs_mode, a.obs_keep, keep, c, row[c]);
                }
                if (valid) {
                    f32x4* xo = reinterpret_cast<f32x4*>(a.x + out * RDM_IN);
#pragma unroll
                    for (int j = 0; j < RDM_IN / 4; ++j)
                        xo[j] = f32x4{row[4 * j], row[4 * j + 1], row[4 * j + 2], row[4 * j + 3]};
                }
                prev_field = carry;
            }
            qs_layers<ROWS, STUDENT_ACTS, BF, true>(lds, a.img, wave, i, g);
            if (phys) {
                float sp[RDM_OUT];
                qs_outputs<ROWS, STUDENT_ACTS>(lds, lane, sp, tp);
                if constexpr (Acts::noisy) {
                    const bool tch_acts = MIXED ? coin : !STUDENT_ACTS;
                    float a0, a1;
                    rd::action_noise_apply(a.noise_mode, a.noise_scale, xi0, xi1, tch_acts ? tp[0] : sp[0],
                                           tch_acts ? tp[1] : sp[1], tch_acts ? tp[2] : sp[2], tch_acts ? tp[3] : sp[3],
                                           a0, a1);
                    carry = rd::env_step<true>(st, a0, a1);
                    if (valid && a.actions) {
                        a.actions[out * 2] = a0;
                        a.actions[out * 2 + 1] = a1;
                    }
                } else if constexpr (MIXED) carry = rd::env_step<true>(st, coin ? tp[0] : sp[0], coin ? tp[1] : sp[1]);
                else carry = STUDENT_ACTS ? rd::env_step<true>(st, sp[0], sp[1]) : rd::env_step<true>(st, tp[0], tp[1]);
                if (valid) {
                    *reinterpret_cast<f32x4*>(a.t_pdflat + out * RDM_OUT) = f32x4{tp[0], tp[1], tp[2], tp[3]};
                    if (a.s_pdflat) {
#pragma unroll
                        for (int c = 0; c < RDM_OUT; ++c) a.s_pdflat[out * RDM_OUT + c] = sp[c];
                    }
                    if (a.reward) a.reward[out] = carry;
                    if constexpr (MIXED) {
                        if (a.stepped_with) a.stepped_with[out] = coin ? 0.0f : 1.0f;
                    }
                }
                rd::env_time_limit(st, s, episode, a.seed, (uint64_t)(a.env_base + env));   // resets inside its last step
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
