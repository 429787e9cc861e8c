// student_lstm.hip's persistent envs (rdl_envs_*, rdl_rollout_envs, rdl_step_envs,
// include/reacher_student_lstm.h): one launch takes the handle's n lockstep envs through K env steps
// under the teacher's or the LSTM student's mean action, writes the K n records and the training
// windows that lie wholly inside an episode, which the training path (rdl_rollout's launches) then
// reads as any caller's windows (DESIGN.md §3 "On-policy distillation of the LSTM student").
// Included inside student_lstm.hip's anonymous namespace after student_lstm_query.h and
// student_lstm_query_bf16.h, whose step it runs: the workgroup's layout, the tiling and the pieces of a step are there.
//
// This kernel's own: the envs are kept between launches.  For its block of 16 envs a workgroup loads
// from the handle's device arrays at entry, and writes back at exit,
//  * the physics state, the reward the last step returned, the clock (step 0..49, episode) and the
//    teacher's last pdflat (lanes 0..15 of wave 0: registers between),
//  * the query state (c, h) (LDS between),
//  * the RAW fields of the ring's T records, ob[11] | prev[4]: they live in the x rows' LDS ring
//    itself, ob in columns 0..10 (the x row's own) and prev in the spare columns EH_PREV.. (the A
//    operands read columns 0..47 only).
// The x rows' dense part (prev . Wp + bp, columns 11..42) is NOT carried: the parameters change
// between calls (an optimiser step, rdl_set_params), so every call re-forms it from the raw prev with
// the Wp, bp it reads, as the stepwise loop forms every window's X at every query (inputs_kernel's
// arithmetic: bias first, then four fmaf).
// STUDENT_ACTS = false (the driver's warm-up: the teacher steps the envs): no cell, no head, (c, h)
// neither read nor written, s_pdflat and stepped_with written as 0; the ring's raw fields are kept
// all the same, for the windows and for a later student call.
// After an env's step 49 it resets from Philox(seed, env_base + i, episode + 1), inside the step as
// rd_step does; the carried reward and (c, h) survive the reset.  The clock is the device's: no
// host-side count enters the arguments, and a captured launch replays the next steps.
// Windows: at an episode step s >= T-1 the query's window is the records s-T+1 .. s of one episode;
// the workgroup writes its 16 windows from the ring (ob, prev, and the records' own t_pdflat: prev of
// the next record, the teacher's output for the last) in the trainer's [T][B][.] layout, window
// index = (qualifying steps of the call so far) n + env, B = LsEnvsArgs::windows.
// Every env's chain depends on no other env and every operation is the stepwise forward's in its
// order, so the outputs are bitwise those of K x { rdd_forward (teacher), the window, rdl_forward,
// rd_step }, whatever the grid and the split of the steps over launches.
#pragma once

constexpr int EH_REC = 16;                    // a ring record in the handle's history: ob[11] | prev[4] | 0
constexpr int ENV_AUX = 1 + 4;                // per env, SoA rows: carried reward | the teacher's last pdflat[4]
static_assert(rd::kObsDim + 4 <= EH_REC, "ring layout");

struct LsEnvsArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;       // teacher net: params | ob mean | ob std
    const float* P;          // the student's flat parameters
    const float* img;        // lstm_eval_pack_kernel's image of Wl [EV_IMG]; BF16Q: the bf16 image WF
    float* state;            // [8][n] SoA (rd_get_state's layout)
    float* aux;              // [ENV_AUX][n]
    int32_t* clock;          // [2][n]: step of the episode, episode
    float* q;                // [2][n][U] = (c, h)
    float* hist;             // [n][T][EH_REC], slot j % T = record j of the open episode
    float* records;          // [K][n][EV_REC]
    float* reward;           // [K][n] or null
    float* ob_w;             // [T][windows][11] or null (no windows written)
    float* prev_w;           // [T][windows][4]
    float* t_w;              // [T][windows][4]
    int64_t windows;         // B: the window buffers' stride and capacity
    int steps, T;            // K
};

// the mixed instances' (rdl_envs_set_teacher_share).  A struct of its own: a longer LsEnvsArgs moves
// the kernels' implicit arguments and hipcc then lays the other instances out anew
struct LsEnvsMixArgs : LsEnvsArgs {
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
};

// the noisy instances' (rdl_envs_set_action_noise, rdl_envs_bind_actions), compiled in
// student_lstm_noise.hip.  Again a struct of its own; the instances are told by it (EnvsActs), so the
// kernel's other template parameters, and with them every other instance's name, stay as they are
struct LsEnvsNoiseArgs : LsEnvsMixArgs {
    int32_t noise_mode;      // RD_NOISE_* (include/reacher_action_noise.h)
    float noise_scale;
    uint64_t noise_seed;     // the noise's Philox key
    float* actions;          // [K][n][2] or null: the action that stepped the env
};

// the faulty instances' (rdl_envs_set_obs_faults: sensor faults on the student's observation,
// include/reacher_obs_faults.h), compiled in student_lstm_faults.hip.  Derived from the noisy one, so
// one faulty instance carries beta, the action noise and the faults as run-time arguments
struct LsEnvsFaultArgs : LsEnvsNoiseArgs {
    int32_t obs_mode;        // RD_OBS_* (include/reacher_obs_faults.h)
    float obs_keep;          // keep_prob
    uint64_t obs_seed;       // the mask's Philox key
};

// What an instance does follows from its argument struct alone: each struct above adds its fields to
// the one before, and an instance carries whatever its struct derives from (with the student acting,
// for the mixture: the teacher-acting noisy instance has beta's fields and never reads them)
template <class ARGS>
struct EnvsActs {
    static constexpr bool mixed = std::is_base_of_v<LsEnvsMixArgs, ARGS>;
    static constexpr bool noisy = std::is_base_of_v<LsEnvsNoiseArgs, ARGS>;
    static constexpr bool faulty = std::is_base_of_v<LsEnvsFaultArgs, ARGS>;
};

// ARGS for a call: the plain instance's arguments, then the fields ARGS adds from the handle's settings
template <class ARGS>
ARGS acting_args(const LsEnvsArgs& base, const rd::Acting& act) {
    ARGS m{};
    static_cast<LsEnvsArgs&>(m) = base;
    if constexpr (EnvsActs<ARGS>::mixed) {
        m.beta = act.beta;
        m.coin_seed = act.coin_seed;
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

// episode 0 of every env; clock and aux to 0 (rd_reset's arithmetic); q and hist are memset by the host
__global__ __launch_bounds__(256) void student_lstm_envs_reset_kernel(LsEnvsArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.n) rd::envs_reset_one<ENV_AUX>(a.state, a.aux, a.clock, a.n, i, a.seed, a.env_base);
}

// BF16Q: the student's positions run on the bf16 cell (student_lstm_query_bf16.h; a.img is then the
// handle's WF image)
// MIXED (with STUDENT_ACTS; DAgger's beta-mixture): the student instance's step, every piece and
// barrier of it -- (c, h) read and replaced, the ring kept, the windows written -- and per env step a
// coin in the env's lane (rd::teacher_coin: a function of (coin seed, env, episode, step) alone, so
// known before the step and drawn before its first barrier) that hands the teacher's T_s[0..1] to
// env_step instead of S_s[0..1]; the record's stepped_with is 1 - coin.
// Acts::noisy (action noise; a student instance is then MIXED too, beta = 0 never firing; the teacher
// instance is not): the two normal draws of this env and step in the env's lane, beside the coin
// (rd::action_noise_draw), and env_step takes rd::action_noise_apply of them and the acting pdflat --
// T_s where the teacher acts, S_s else -- instead of its mean; that action goes to `actions`.
// Nothing else of the step changes: the record, (c, h), the ring and the windows are the plain call's.
// Acts::faulty (sensor faults; a student instance, MIXED and noisy too, either of which may be off at
// run time): columns 0..10 of the ring's x rows hold what the student READS of each record, masked by
// the record's own (episode, step) -- the carried records at entry (the mask is a pure function, so
// the handle's history stays clean and a call after a teacher call, a reset of the setting or a call
// boundary masks them the same), record s in the env's lane beside the coin and the noise
// (ls_fault_mask, before the step's first barrier).  The clean observations live beside the ring
// (ls_fault_clean): the windows' ob_w and the history written back come from there, the teacher's SO
// row and the records from the clean registers.
template <bool STUDENT_ACTS, bool BF16Q, class ARGS = LsEnvsArgs>
__global__ __launch_bounds__(EV_THREADS) void student_lstm_envs_kernel(ARGS a) {
    using Acts = EnvsActs<ARGS>;
    constexpr bool MIXED = STUDENT_ACTS && Acts::mixed;   // the mixture is a student call's
    const LsThread q = ls_prologue<STUDENT_ACTS>(a.tnet, a.P, a.img, a.T);
    const int tid = q.tid, lane = q.lane, T = q.T;
    const bool phys = q.wave == 0 && lane < EV_ROWS;   // the env of this lane
    const bool win = a.ob_w != nullptr;
    const int64_t n = a.n, nblk = (n + EV_ROWS - 1) / EV_ROWS;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t row0 = blk * EV_ROWS;
        const bool valid = phys && row0 + lane < n;
        const int64_t env = row0 + (valid ? lane : 0);   // a ragged block's spare lanes repeat its env 0
        __syncthreads();   // the previous block's last reads and its write-back
        int32_t s = a.clock[row0];   // lockstep: one clock for the block
        if (STUDENT_ACTS) ls_state_load(tid, a.q, n, row0);   // the carried query state
        for (int x = tid; x < EV_ROWS * T * EH_REC; x += EV_THREADS) {   // the ring's raw fields
            const int r = x / (T * EH_REC), y = x - r * (T * EH_REC), slot = y / EH_REC, c = y - slot * EH_REC;
            const int64_t er = row0 + r < n ? row0 + r : row0;
            const float v = a.hist[(er * T + slot) * EH_REC + c];
            if constexpr (Acts::faulty) {
                if (c < rd::kObsDim) ls_fault_clean()[slot][r][c] = v;
            }
            if (c < rd::kObsDim) lds::Xr[slot][r][c] = v;
            else if (c < rd::kObsDim + 4) lds::Xr[slot][r][EH_PREV + c - rd::kObsDim] = v;
        }
        int hp = 0;   // Hb[hp] holds the current h
        rd::State st;
        float carry = 0.0f;   // the reward this env's previous step returned
        float tp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int32_t episode = 0;
        if (phys) {
            rd::load_state(a.state, n, env, st);
            carry = a.aux[env];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                tp[c] = a.aux[(1 + c) * n + env];
                lds::TO[(s + 1) & 1][lane][c] = tp[c];   // T_{s-1}: the next record's prev
            }
            episode = a.clock[n + env];
        }
        __syncthreads();
        if constexpr (Acts::faulty) {
            // the carried records of the open episode, as the student read them: slot's record is the last
            // j <= s - 1 with j % T = slot (none at s = 0, or where that j < 0: a stale slot no window reads)
            static_assert(STUDENT_ACTS && EV_ROWS * EV_MAX_T <= EV_THREADS, "a thread per carried record");
            if (tid < EV_ROWS * T && s > 0) {
                const int r = tid / T, slot = tid - r * T;
                const int j = s - 1 - (((s - 1 - slot) % T + T) % T);
                const int64_t er = row0 + r < n ? row0 + r : row0;
                if (j >= 0)
                    ls_fault_mask(r, slot, a.obs_mode, a.obs_keep, a.obs_seed, (uint64_t)(a.env_base + er),
                                  a.clock[n + er], j, nullptr);
            }
        }
        if (STUDENT_ACTS) {   // the carried records' x rows, from their raw prev and THIS call's Wp, bp
            for (int slot = 0; slot < T; ++slot)
                lds::Xr[slot][q.dr][11 + q.dc] = ls_dense(q, true, &lds::Xr[slot][q.dr][EH_PREV]);
            __syncthreads();
        }
        int64_t wrow = row0;   // this block's first window of the current qualifying step
        for (int k = 0; k < a.steps; ++k) {
            const int slot = s % T;
            float* rec = valid ? a.records + ((int64_t)k * n + env) * EV_REC : nullptr;
            bool coin = false;   // MIXED: the teacher steps this env now
            if (phys) {   // record s, and its raw prev = T_{s-1} (zero at s = 0) into the ring
                if constexpr (MIXED)
                    coin = rd::teacher_coin(a.coin_seed, (uint64_t)(a.env_base + env), episode, s, a.beta);
                if constexpr (Acts::noisy) {
                    if (!Acts::faulty || a.noise_mode != 0)   // a faulty call's noise may be off
                        ls_noise_draw(lane, a.noise_seed, (uint64_t)(a.env_base + env), episode, s);
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) lds::Xr[slot][lane][EH_PREV + c] = s ? lds::TO[(s - 1) & 1][lane][c] : 0.0f;
                if constexpr (MIXED) ls_record_head(lane, slot, st, rec, carry, coin ? 0.0f : 1.0f);
                else ls_record_head(lane, slot, st, rec, carry, STUDENT_ACTS ? 1.0f : 0.0f);
                if constexpr (Acts::faulty)
                    ls_fault_mask(lane, slot, a.obs_mode, a.obs_keep, a.obs_seed, (uint64_t)(a.env_base + env), episode, s,
                                  ls_fault_clean());
            }
            // prev . Wp + bp of record s
            if (STUDENT_ACTS) lds::Xr[slot][q.dr][11 + q.dc] = ls_dense(q, s != 0, lds::TO[(s - 1) & 1][q.dr]);
            __syncthreads();
            ls_teacher(q, s);
            if constexpr (STUDENT_ACTS) hp = ls_positions_of<BF16Q>(q, s, hp);
            else __syncthreads();   // T_s
            // the window of this query, if it lies inside the episode: records s-T+1 .. s from the ring
            // (T_s was published by the barriers above; the ring's next write follows the barriers below)
            if (win && s >= T - 1) {
                for (int x = tid; x < T * EV_ROWS * rd::kObsDim; x += EV_THREADS) {
                    const int p = x / (EV_ROWS * rd::kObsDim), y = x - p * (EV_ROWS * rd::kObsDim);
                    const int r = y / rd::kObsDim, c = y - r * rd::kObsDim;
                    const int64_t w = wrow + r;
                    if constexpr (Acts::faulty) {   // the clean observations
                        if (row0 + r < n && w < a.windows)
                            a.ob_w[((int64_t)p * a.windows + w) * rd::kObsDim + c] = ls_fault_clean()[(s - (T - 1) + p) % T][r][c];
                    } else {
                        if (row0 + r < n && w < a.windows)
                            a.ob_w[((int64_t)p * a.windows + w) * rd::kObsDim + c] = lds::Xr[(s - (T - 1) + p) % T][r][c];
                    }
                }
                for (int x = tid; x < T * EV_ROWS * 4; x += EV_THREADS) {
                    const int p = x / (EV_ROWS * 4), r = (x >> 2) & (EV_ROWS - 1), c = x & 3;
                    const int j = s - (T - 1) + p;
                    const int64_t w = wrow + r;
                    if (row0 + r < n && w < a.windows) {
                        const int64_t o = ((int64_t)p * a.windows + w) * 4 + c;
                        a.prev_w[o] = lds::Xr[j % T][r][EH_PREV + c];
                        a.t_w[o] = p < T - 1 ? lds::Xr[(j + 1) % T][r][EH_PREV + c] : lds::TO[s & 1][r][c];
                    }
                }
                wrow += n;
            }
            if constexpr (STUDENT_ACTS) ls_head<BF16Q>(q, hp);
            if (phys) {
                float sp[4];
                ls_record_tail<STUDENT_ACTS>(lane, s, rec, tp, sp);
                if constexpr (Acts::noisy) {
                    const bool tch_acts = MIXED ? coin : !STUDENT_ACTS;
                    const float xi0 = ls_noise_park()[2 * lane], xi1 = ls_noise_park()[2 * lane + 1];
                    float a0, a1;
                    rd::action_noise_apply(a.noise_mode, a.noise_scale, xi0, xi1, tch_acts ? tp[0] : sp[0],
                                           tch_acts ? tp[1] : sp[1], tch_acts ? tp[2] : sp[2], tch_acts ? tp[3] : sp[3],
                                           a0, a1);
                    carry = rd::env_step<true>(st, a0, a1);
                    if (valid && a.actions) {
                        a.actions[((int64_t)k * n + env) * 2] = a0;
                        a.actions[((int64_t)k * n + env) * 2 + 1] = a1;
                    }
                } else if constexpr (MIXED) carry = rd::env_step<true>(st, coin ? tp[0] : sp[0], coin ? tp[1] : sp[1]);
                else carry = STUDENT_ACTS ? rd::env_step<true>(st, sp[0], sp[1]) : rd::env_step<true>(st, tp[0], tp[1]);
                if (valid && a.reward) a.reward[(int64_t)k * n + env] = carry;
            }
            rd::env_time_limit(st, s, episode, a.seed, (uint64_t)(a.env_base + env), phys);   // resets inside its last step
            // the next step's first writes (SO, the ring's slot, TO's other parity) follow every read of
            // them: the head's barriers, or this one
            if constexpr (!STUDENT_ACTS) __syncthreads();
        }
        // write back: (c, h) after the call's last query, the ring's raw fields, the envs
        if (STUDENT_ACTS) ls_state_store(tid, a.q, n, row0, hp);
        for (int x = tid; x < EV_ROWS * T * EH_REC; x += EV_THREADS) {
            const int r = x / (T * EH_REC), y = x - r * (T * EH_REC), slot = y / EH_REC, c = y - slot * EH_REC;
            if constexpr (Acts::faulty) {   // the clean observations
                if (row0 + r < n)
                    a.hist[((row0 + r) * T + slot) * EH_REC + c] =
                        c < rd::kObsDim ? ls_fault_clean()[slot][r][c] : c < rd::kObsDim + 4 ? lds::Xr[slot][r][EH_PREV + c - rd::kObsDim] : 0.0f;
            } else {
                if (row0 + r < n)
                    a.hist[((row0 + r) * T + slot) * EH_REC + c] =
                        c < rd::kObsDim ? lds::Xr[slot][r][c] : c < rd::kObsDim + 4 ? lds::Xr[slot][r][EH_PREV + c - rd::kObsDim] : 0.0f;
            }
        }
        if (valid) {
            rd::store_state(a.state, n, env, st);
            a.aux[env] = carry;
#pragma unroll
            for (int c = 0; c < 4; ++c) a.aux[(1 + c) * n + env] = tp[c];
            a.clock[env] = s;
            a.clock[n + env] = episode;
        }
    }
}
