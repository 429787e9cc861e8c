// distill.hip, part 4 of 5: the fused rollout + distillation step -- RolloutArgs, the pair
// hand-off (wait_ge / publish), env_step_group and rollout_kernel.  Expects the three parts before
// it (layouts, forwards, ws_index), rd_physics.h, and STAMP / RTSTAMP defined (distill.hip).
#pragma once

struct RolloutArgs {
    int64_t n, env_base;
    uint64_t seed;
    float* state;                          // [8][n]
    const float* tnet;                     // teacher: params[P], mu[11], sd[11] (contiguous); in
                                           // distill_rows_kernel the rows' recorded teacher pdflat [n][4]
    const float* snet;                     // student
    uint32_t* ctl;                         // [0] completed steps, [4..7] snapshot
    float* ws;                             // [RED_GRID][gridDim.x][RED_COLS] (ws_index)
    int loss, act_student, stagger;
    float inv_n_global;
    int gs;                                // envs per group (16, 32 or 64)
    int ksteps;                            // env steps of this launch (rdd_step_accum: accum_steps)
    unsigned long long* dbg;               // RD_STAMPS builds: [grid*WAVES][NSTAMP] stamp sums
    const float* obs_in;                   // observation-batch mode: [n][11] rows, no env step
    const float* timg;                     // prepacked LDS images (pack_net_kernel)
    const float* simg;
};

// Hand-off counters live in LDS; each is written by one wave only.  Acquire/release at
// workgroup scope order the slot data (LDS) around them.  A spin that exceeds SPIN_LIMIT
// raises ctl[8] and returns false: the caller leaves its loop, so the launch always ends.
__device__ __forceinline__ bool wait_ge(const uint32_t* f, uint32_t target, uint32_t* err) {
    for (uint32_t spins = 0;; ++spins) {
        if (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= target) return true;
        if (spins > SPIN_LIMIT) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// wait_ge whose exit the compiler sees as wave-uniform (every lane reads the same counter, so the
// first lane's value is the wave's).  The f32 student's teacher hand-off waits use it: around a
// divergent exit the compiler keeps a second copy of every accumulator that is live across the wait,
// and the f32-split consumer (82 of them) then spills.
__device__ __forceinline__ bool wait_ge_uniform(const uint32_t* f, uint32_t target, uint32_t* err) {
    for (uint32_t spins = 0;; ++spins) {
        const uint32_t v = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_readfirstlane(v) >= target) return true;
        if (spins > SPIN_LIMIT) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

__device__ __forceinline__ void publish(uint32_t* f, uint32_t v) {
    __hip_atomic_store(f, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// env.step of this lane's env with the policy's action, the episode clock (lockstep or
// staggered) and the auto-reset; writes the state back and returns the reward (0 for a lane
// without an env).  met_n counts the stepped envs.
__device__ __forceinline__ float env_step_group(const RolloutArgs& a, uint32_t C, int64_t i, bool valid, float act0,
                                                float act1, rd::State& st, float& met_n) {
    const uint32_t iu = (uint32_t)i;
    const float rew = rd::env_step<false>(st, act0, act1);
    // episode clock of this env (RDD_STAGGER_GROUP envs share an offset)
    const int64_t gid = a.env_base + i;
    const uint32_t u = C + (a.stagger ? (uint32_t)((gid / RDD_STAGGER_GROUP) % rd::kEpisodeSteps) : 0u);
    const bool done_step = (u % rd::kEpisodeSteps) == rd::kEpisodeSteps - 1;
    if (done_step) {
        float dr[6];
        rd::philox_draw(a.seed, (uint64_t)gid, u / rd::kEpisodeSteps + 1, dr);
        rd::env_reset(st, dr);
    }
    if (!valid) return 0.0f;
    rd::store_state(a.state, a.n, iu, st, done_step);
    met_n += 1.0f;
    return rew;
}

// BS: bf16 student (RDD_DTYPE_BF16); SPL: split-bf16 f32 hidden layers; CP: the consumer wave
// steps the envs (else the producer does, from the state it loaded for the observations);
// MD: MD_TEACHER the teacher network is queried; MD_ROWS observation rows with their recorded
// teacher pdflat (a.tnet), no teacher network (no teacher image in LDS); MD_HELPER (f32
// student, one 16-env tile per pair's group, launch_rollout): pairs 0, 1 own the groups and
// pairs 2, 3 run their tiles' teacher forwards on the other two SIMDs
constexpr int MD_TEACHER = 0, MD_ROWS = 1, MD_HELPER = 2;
// KS: a.ksteps env steps in one launch (rdd_step_accum); the K = 1 instances are compiled without
// the step loop.
// TCM (split teacher, K = 1; rdd_config.teacher_tiles): bit t set = the consumer wave runs the
// teacher forward of tile t of every group from the producer's observation rows and hands the
// means back (P_TM, flag [3]); the producer publishes each group's observations (flag [2]) and
// runs the teacher of the other tiles beside the student forwards.  Tile 0 is never the
// consumer's: it needs the group's observations published first.  0: every teacher forward on
// the producer.  0b1010 is config 5's layout (bf16 student, c5 -0.5 us per step).
template <bool BS, bool SPL, bool CP, int MD, bool KS = false, int TCM = 0>
__global__ __launch_bounds__(BLOCK, 2) void rollout_kernel(RolloutArgs a) {
    constexpr bool TGT = MD == MD_ROWS, HLP = MD == MD_HELPER;
    constexpr bool TC = TCM != 0;
    static_assert(TCM == 0 || (MD == MD_TEACHER && !KS && SPL), "teacher on the consumer: split teacher, K = 1");
    static_assert((TCM & ~((1 << GROUP / TILE) - 2)) == 0, "a mask over tiles 1 .. 3; tile 0 stays on the producer");
    // is tile t (t + 1: tn) the consumer's?  0b1010 keeps the odd-tile test config 5 was tuned with
    // (the same tiles for t < 4, and that instance's ISA)
    auto tc_tile = [](int t) { return TCM == 0b1010 ? (t & 1) != 0 : ((TCM >> t) & 1) != 0; };
    auto tc_next = [](int t) { return TCM == 0b1010 ? !(t & 1) : ((TCM >> (t + 1)) & 1) != 0; };
    // TC: the consumer's teacher means of one tile [16][2].  !CP: P_SACT carries actions only in the
    // consumer-side-step kernels (the CP store below), so it is free here
    constexpr int P_TM = CP ? P_ACT : P_SACT;
    static_assert(!HLP || !BS, "helper pairs: f32 student kernels only");
    constexpr int TN = TGT ? 0 : img_t(SPL), SN = img_s(BS, SPL);
    __shared__ __attribute__((aligned(16))) float lds[TN + SN + PAIRS * PSCR];
    float* LT = lds;
    float* LS = lds + TN;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4;
    const int pair = wave & (PAIRS - 1);
    const bool producer = wave < PAIRS;
    uint32_t* flags = reinterpret_cast<uint32_t*>(lds + TN + SN + pair * PSCR + P_FLAGS);
    uint32_t* err = a.ctl + 8;

    RTSTAMP(16);
    STAMP(0);
    const int gs = a.gs;   // envs per group: 64, or 32 / 16 to spread a small batch over more pairs
    // 32-bit group / env indices (n <= 2^31, rdd_create): fewer SGPRs live across the loops
    const uint32_t n32 = (uint32_t)a.n;
    const uint32_t ngroups = (n32 + (uint32_t)gs - 1) / (uint32_t)gs;
    // HLP: the owner pairs 0, 1 take the groups (one each), pairs 2, 3 none (they help).  The
    // layout holds at most one group per owner (launch_rollout): a launch that breaks this ends
    // at once with the hand-off error raised (rdd_counter reports it)
    // KS (K env steps in one launch): the producer re-reads the state its own lanes wrote, so
    // the consumer-side env step (CP), the helper layout and the observation modes stay K = 1
    static_assert(!KS || (!CP && MD == MD_TEACHER), "K-step launches: teacher mode, producer-side env step");
    if constexpr (KS) {
        if (a.obs_in) {
            if (threadIdx.x == 0) __hip_atomic_store(a.ctl + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    if constexpr (HLP) {
        if (ngroups > 2u * gridDim.x) {
            if (threadIdx.x == 0) __hip_atomic_store(a.ctl + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    const bool helper = HLP && pair >= 2;
    const uint32_t gstride = gridDim.x * (HLP ? 2 : PAIRS);
    const uint32_t gfirst = helper ? ngroups : blockIdx.x * (HLP ? 2 : PAIRS) + pair;
    // a producer's first group of envs: its state loads are issued before the image copy so
    // that their HBM latency overlaps the prologue
    rd::State st0{};
    if (producer && !a.obs_in && gfirst < ngroups && lane < gs && gfirst * gs + lane < a.n)
        load_state(a.state, a.n, (uint32_t)(gfirst * gs + lane), st0);
    // HLP with the teacher acting: the helper producer steps its owner's envs (below), so it loads
    // their state here instead of the owner
    const uint32_t og = blockIdx.x * 2 + (pair & 1);   // HLP: the owner group a helper serves
    const bool hstep = helper && producer && !a.obs_in && !a.act_student;
    if constexpr (HLP) {
        if (hstep && og < ngroups && lane < gs && og * gs + lane < a.n)
            load_state(a.state, a.n, (uint32_t)(og * gs + lane), st0);
    }
    static_assert(NET % 4 == 0 && NET_S % 4 == 0, "16-B images");
    // ... and its observations are formed (into obs buffer 0) while the image loads are in flight
    float* PS = lds + TN + SN + pair * PSCR;
    const bool first_obs = producer && gfirst < ngroups;
    auto group_obs = [&](uint32_t k, uint32_t i, bool lvalid, rd::State& st) {
        float ob[OBD];
        if (a.obs_in) {   // observation-batch mode: rows given by the caller
#pragma unroll
            for (int q = 0; q < OBD; ++q) ob[q] = lvalid ? a.obs_in[(size_t)i * OBD + q] : 0.0f;
        } else {
            rd::observe<false>(st, ob);
        }
        float* o = PS + P_SO + lane * SOS;
        st4(o, f32x4{ob[0], ob[1], ob[2], ob[3]});
        st4(o + 4, f32x4{ob[4], ob[5], ob[6], ob[7]});
        st4(o + 8, f32x4{ob[8], ob[9], ob[10], 1.0f});
    };
    copy_images<TN / 4, SN / 4, BLOCK>(LT, a.timg, a.simg, [&] {   // LS = LT + TN
        if (first_obs) {
            const uint32_t i = gfirst * (uint32_t)gs + (uint32_t)lane;
            group_obs(0, i, lane < gs && i < n32, st0);
        }
    });
    using SO = Off<BS ? IMG_BF16 : (SPL ? IMG_SPLIT : IMG_F32)>;
    constexpr int SW3 = SO::W3, SMU = SO::MU, SRS = SO::RS;
    if (threadIdx.x < PAIRS * 4)
        reinterpret_cast<uint32_t*>(lds + TN + SN + (threadIdx.x >> 2) * PSCR + P_FLAGS)[threadIdx.x & 3] = 0u;

    const uint32_t C = a.ctl[0];
    // snapshot of the step words for reduce_adam_kernel, which rewrites ctl[0..3]; ctl[12]
    // tells it whether this launch stepped the envs (the env clock advances only then)
    if (blockIdx.x == 0 && threadIdx.x < 4) a.ctl[4 + threadIdx.x] = a.ctl[threadIdx.x];
    if (blockIdx.x == 0 && threadIdx.x == 4) a.ctl[12] = a.obs_in ? 0u : (KS ? (uint32_t)a.ksteps : 1u);
    __syncthreads();
    STAMP(1);

    if (producer) {
        // ============================================================ producer wave
        // partial sums: dW3 (env j of this lane, features 16x+4g+r), db3, dlogstd, metrics
        f32x4 gw3a[4], gw3b[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) gw3a[x] = gw3b[x] = f32x4{0.f, 0.f, 0.f, 0.f};
        float gb3a = 0, gb3b = 0, gls0 = 0, gls1 = 0, met_l = 0, met_m = 0, met_r = 0, met_n = 0;
        // teacher log-std (TGT: per row, from the recorded pdflat, below)
        const float tl0 = TGT ? 0.0f : a.tnet[P_LS], tl1 = TGT ? 0.0f : a.tnet[P_LS + 1];
        const float sl0 = a.snet[P_LS], sl1 = a.snet[P_LS + 1];
        const float sv0 = __expf(2.0f * sl0), sv1 = __expf(2.0f * sl1);
        const float rtv0 = 1.0f / __expf(2.0f * tl0), rtv1 = 1.0f / __expf(2.0f * tl1);
        uint32_t tiles = 0;
        uint32_t k = 0;
        uint32_t tct = 0;   // TC: teacher tiles taken from the consumer
        bool ok = true;
        // HLP helper (pair 2 + o): the teacher forward of owner o's first tile (its observations
        // were formed in the prologue, before the barrier), means into this pair's P_ACT, flag [0]
        if constexpr (HLP) {
            if (helper && og < ngroups) {
                STAMP(18);
                const float* oobs = lds + TN + SN + (pair & 1) * PSCR + P_SO;
                float m0, m1;
                if constexpr (SPL) {
                    mlp_forward_split(LT, oobs, j, g, m0, m1);
                } else {
                    f32x4 h1[4], h2[4];
                    mlp_forward<true>(LT, oobs, j, g, h1, h2, m0, m1);
                }
                if (g == 0) {
                    PS[P_ACT + 2 * j] = m0;
                    PS[P_ACT + 2 * j + 1] = m1;
                }
                publish(flags, 1u);
                STAMP(19);
                // ... and, with the teacher acting, steps the owner's envs with these means (lane
                // j < 16 holds env j's): the owner's producer skips its env step
                if (hstep && lane < gs) {
                    const uint32_t i = og * (uint32_t)gs + (uint32_t)lane;
                    met_r += env_step_group(a, C, i, i < n32, m0, m1, st0, met_n);
                }
                STAMP(23);
            }
        }
        // K env steps per launch (rdd_step_accum): the images stay in LDS and the gradient
        // partials in registers over all K; a pair that owns one group keeps its envs' state in
        // registers from one step to the next (the rest re-read the state they wrote)
        // (KS: st0 carries it over)
        const uint32_t K = KS ? (uint32_t)a.ksteps : 1u;
        const bool resident = KS && gfirst + gstride >= ngroups;
        for (uint32_t kk = 0;; ++kk) {   // (K = 1: no loop; the K = 1 instances' ISA is that of round 4)
        for (uint32_t grp = gfirst; ok && grp < ngroups; grp += gstride, ++k) {
            STAMP(8);
            const uint32_t Ck = C + kk;   // the episode clock of this env step
            const uint32_t base = grp * (uint32_t)gs;
            const uint32_t i = base + (uint32_t)lane;   // n <= 2^31 (rdd_create)
            const bool lvalid = lane < gs && i < n32;   // this lane has an env
            float* obs = PS + P_SO;
            float* act = PS + P_ACT;
            rd::State st{};   // this lane's env, kept in registers for the env.step after the tiles
            if (k == 0) {
                st = st0;   // observations formed in the prologue
            } else if (resident) {
                if (lvalid) st = st0;   // the state this lane stepped at the previous env step
                group_obs(k, i, lvalid, st);
            } else {
                if (!a.obs_in && lvalid) load_state(a.state, a.n, i, st);
                group_obs(k, i, lvalid, st);
            }
            STAMP(11);
            wave_sync();
            if constexpr (TC) publish(flags + 2, k + 1);   // this group's observation rows are in P_SO
            const int ntile = (int)min((uint32_t)(gs / TILE), (n32 - base + TILE - 1) / TILE);
            for (int t = 0; t < ntile; ++t) {
                const bool tvalid = base + TILE * t + j < a.n;
                const float* obt = obs + TILE * t * SOS;
                f32x4 H1[4], H2[4];
                float mt0, mt1, ms0, ms1;
                float rl0 = tl0, rl1 = tl1, rr0 = rtv0, rr1 = rtv1;   // this row's teacher log-std, 1/var
                STAMP(10);
                if constexpr (TGT) {
                    // the reference's t_pdflat feed (mlp_train.py:146-161): this env's recorded
                    // teacher mean and log-std instead of a teacher query; the student alone runs
                    const uint32_t row = base + TILE * t + j;
                    const f32x4 tq = tvalid ? ld4(a.tnet + (size_t)row * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
                    if constexpr (BS) mlp_forward_bf16(LS, obt, j, g, H1, H2, ms0, ms1);
                    else if constexpr (SPL) mlp_forward_split_t<true>(LS, obt, j, g, H1, H2, ms0, ms1);
                    else mlp_forward(LS, obt, j, g, H1, H2, ms0, ms1);
                    mt0 = tq[0];
                    mt1 = tq[1];
                    rl0 = tq[2];
                    rl1 = tq[3];
                    rr0 = 1.0f / __expf(2.0f * rl0);
                    rr1 = 1.0f / __expf(2.0f * rl1);
                } else if constexpr (HLP) {
                    if (k == 0) {
                        // owner: the student's forward of its tile; the teacher's comes from the
                        // helper pair on another SIMD (gs = 16: one tile, t = 0)
                        if constexpr (SPL) mlp_forward_split_t<true>(LS, obt, j, g, H1, H2, ms0, ms1);
                        else mlp_forward<true>(LS, obt, j, g, H1, H2, ms0, ms1);
                        const float* hp = lds + TN + SN + (pair + 2) * PSCR;
                        if (!(ok = wait_ge(reinterpret_cast<const uint32_t*>(hp + P_FLAGS), 1u, err))) break;
                        mt0 = hp[P_ACT + 2 * j];
                        mt1 = hp[P_ACT + 2 * j + 1];
                    } else {   // later groups (not launched in this layout): both forwards here
                        if constexpr (SPL) mlp_forward_pair_split(LT, LS, obt, j, g, H1, H2, mt0, mt1, ms0, ms1);
                        else mlp_forward_pair<true>(LT, LS, obt, j, g, H1, H2, mt0, mt1, ms0, ms1);
                    }
                } else if constexpr (BS) {
                    if (TC && tc_tile(t)) {   // the consumer ran this tile's teacher forward
                        mlp_forward_bf16(LS, obt, j, g, H1, H2, ms0, ms1);
                        if (!(ok = wait_ge(flags + 3, ++tct, err))) break;
                        mt0 = PS[P_TM + 2 * j];
                        mt1 = PS[P_TM + 2 * j + 1];
                    } else {
                    // CP, KS: in these kernels' schedules the compiler issues loads into the SrcC
                    // registers of the exact teacher's f32 MFMAs: fenced (see fence_begin)
                    if constexpr (SPL) mlp_forward_split(LT, obt, j, g, mt0, mt1);
                    else mlp_forward<CP || KS || TC>(LT, obt, j, g, H1, H2, mt0, mt1);
                    mlp_forward_bf16(LS, obt, j, g, H1, H2, ms0, ms1);
                    }
                } else {
                    // exact f32: unfenced, hipcc issues a W3 load / an A-operand prefetch into the SrcC
                    // registers of an in-flight f32 MFMA of layer 2 (hazards.py scan_ldsrc).  Fencing
                    // k-steps 9, 11 and 15 (kPairFence) leaves no such load in any instance -- the
                    // hygiene test re-checks the built ISA -- at 3 % of the kernel, where fencing all
                    // 16 cost 16 % (c4 exact 110.1 / 113.8 / 128.0 us per step unfenced / kPairFence /
                    // every step, profiles/r06a_*, r06b_*)
                    if constexpr (SPL) {
                        if (TC && tc_tile(t)) {   // as the bf16 student's: the student alone, the means from P_TM
                            mlp_forward_split_t<true>(LS, obt, j, g, H1, H2, ms0, ms1);
                            if (!(ok = wait_ge_uniform(flags + 3, ++tct, err))) break;
                            mt0 = PS[P_TM + 2 * j];
                            mt1 = PS[P_TM + 2 * j + 1];
                        } else {
                            mlp_forward_pair_split(LT, LS, obt, j, g, H1, H2, mt0, mt1, ms0, ms1);
                        }
                    } else {
                        mlp_forward_pair<false, kPairFence>(LT, LS, obt, j, g, H1, H2, mt0, mt1, ms0, ms1);
                    }
                }
                STAMP(12);
                // loss
                const float d0 = ms0 - mt0, d1 = ms1 - mt1;
                float dm0, dm1, dl0 = 0.0f, dl1 = 0.0f, lossv;
                if (a.loss == RDD_LOSS_MSE) {
                    dm0 = d0 * a.inv_n_global;
                    dm1 = d1 * a.inv_n_global;
                    lossv = (d0 * d0 + d1 * d1) * (0.5f * a.inv_n_global);
                } else {
                    dm0 = d0 * rr0;
                    dm1 = d1 * rr1;
                    dl0 = sv0 * rr0 - 1.0f;
                    dl1 = sv1 * rr1 - 1.0f;
                    lossv = (rl0 - sl0 + (sv0 + d0 * d0) * (0.5f * rr0) - 0.5f) +
                            (rl1 - sl1 + (sv1 + d1 * d1) * (0.5f * rr1) - 0.5f);
                }
                if (!tvalid) { dm0 = dm1 = dl0 = dl1 = 0.0f; }
                if (g == 0 && tvalid) {
                    met_l += lossv;
                    met_m += d0 * d0 + d1 * d1;
                    gb3a += dm0; gb3b += dm1; gls0 += dl0; gls1 += dl1;
                    if (!CP) {   // the producer steps the envs itself, after the group's tiles
                        act[(TILE * t + j) * 2] = a.act_student ? ms0 : mt0;
                        act[(TILE * t + j) * 2 + 1] = a.act_student ? ms1 : mt1;
                    }
                }
                // dW3 partials (env j of this lane) and dZ2 = (W3 . dmean) * (1 - H2^2)
                f32x4 dZ[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 wa = ld4(LS + SW3 + (16 * fb + 4 * g) * 2);
                    const f32x4 wb = ld4(LS + SW3 + (16 * fb + 4 * g) * 2 + 4);
                    const float w0[4] = {wa[0], wa[2], wb[0], wb[2]}, w1[4] = {wa[1], wa[3], wb[1], wb[3]};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float h = H2[fb][r];
                        gw3a[fb][r] = fmaf(h, dm0, gw3a[fb][r]);
                        gw3b[fb][r] = fmaf(h, dm1, gw3b[fb][r]);
                        dZ[fb][r] = fmaf(w0[r], dm0, w1[r] * dm1) * fmaf(-h, h, 1.0f);
                    }
                }
                // hand the tile over: H1^T, dZ2^T (env-major rows) into the slot
                STAMP(2);
                if (!(ok = wait_ge(flags + 1, tiles, err))) break;
                STAMP(3);
                float* h1t = PS + P_H1T;
                float* dzt = PS + P_DZT;
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    st4(h1t + j * SAS + 16 * fb + 4 * g, H1[fb]);
                    st4(dzt + j * SAS + 16 * fb + 4 * g, dZ[fb]);
                }
                if (lane < TILE * SOS / 4) st4(PS + P_SOB + 4 * lane, ld4(obt + 4 * lane));
                if (CP && g == 0) {   // the consumer steps these envs: their actions travel with the slot
                    PS[P_SACT + 2 * j] = a.act_student ? ms0 : mt0;
                    PS[P_SACT + 2 * j + 1] = a.act_student ? ms1 : mt1;
                }
                publish(flags, ++tiles);
            }
            if (!ok) break;
            // ---------------------------------------------------------- env.step (one env per lane)
            // !CP: the producer computed this group's actions itself, so it steps the envs at
            // once from the state it holds (the consumer's share is then the gradient tiles
            // only).  CP: the consumer steps them after its last tile of the group, which
            // balances the roles when the producer's forward is the longer one (split / bf16).
            STAMP(4);
            if constexpr (!CP) {
                if (a.obs_in) {   // observation-batch mode: no env to step
                    if (lvalid) met_n += 1.0f;
                } else if (HLP && k == 0 && !a.act_student) {
                    // the helper pair steps these envs (above)
                } else {
                    wave_sync();   // act[] rows were written by the g = 0 lanes of each tile
                    if (lane < gs) met_r += env_step_group(a, Ck, i, lvalid, act[lane * 2], act[lane * 2 + 1], st, met_n);
                }
            }
            if constexpr (KS) st0 = st;
            STAMP(5);
        }
        if (!KS || !ok || kk + 1 >= K) break;
        }
        // ------------------------------------------------------------ this wave's share
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int r = 0; r < 4; ++r)   // sum over the env axis (the 16 lanes of a row)
#pragma unroll
                for (int o = 8; o >= 1; o >>= 1) {
                    gw3a[x][r] += __shfl_xor(gw3a[x][r], o, 16);
                    gw3b[x][r] += __shfl_xor(gw3b[x][r], o, 16);
                }
        gb3a = wave_sum(gb3a); gb3b = wave_sum(gb3b);
        gls0 = wave_sum(gls0); gls1 = wave_sum(gls1);
        met_l = wave_sum(met_l); met_m = wave_sum(met_m);
        met_r = wave_sum(met_r); met_n = wave_sum(met_n);
        STAMP(6);
        __syncthreads();   // (one of the two barriers every wave meets) weights/scratch are free
        STAMP(9);
        float* R = lds + pair * RPAD + RSHIFT;   // pair p fills region p (entries past W2: ridx = p + RSHIFT)
        if (j == 0) {
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = 16 * fb + 4 * g + r;
                    R[P_W3 + 2 * f] = gw3a[fb][r];
                    R[P_W3 + 2 * f + 1] = gw3b[fb][r];
                }
        }
        if (lane == 0) {
            R[P_B3] = gb3a; R[P_B3 + 1] = gb3b; R[P_LS] = gls0; R[P_LS + 1] = gls1;
            R[P_TOT + 1] = met_l; R[P_TOT + 2] = met_m;
            if constexpr (!CP) { R[P_TOT] = met_r; R[P_TOT + 3] = met_n; }
        }
    } else {
        // ============================================================ consumer wave
        // partial sums: dW2, dW1 (+db1 in row 11), db2 (envs 4s+g of feature 16x+j), rewards
        f32x4 gW2[4][4], gW1[4];
        float gb2[4];
        // split mode and the bf16 student: dW2 in 32 x 32 blocks (v_mfma_f32_32x32x16_bf16) and db2 of
        // features 32 nb + (lane & 31) over the envs of this lane half
        constexpr bool D32 = SPL || BS;
        f32x16 gW2s[2][2];
        float gb2s[2] = {0.f, 0.f};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
#pragma unroll
            for (int y = 0; y < 4; ++y) gW2[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
            gW1[x] = f32x4{0.f, 0.f, 0.f, 0.f};
            gb2[x] = 0.0f;
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int r = 0; r < 16; ++r) gW2s[x][y][r] = 0.0f;
        const int c32 = lane & 31, h32 = lane >> 5;   // D32: the 32 x 32 operand / accumulator lane map
        // student filter of input j for the dW1 A operand (lane-constant)
        const float smu = j < 12 ? LS[SMU + j] : 0.0f, srs = j < 12 ? LS[SRS + j] : 0.0f;
        float met_r = 0.0f, met_n = 0.0f;   // CP: reward and env count of the envs this wave steps
        uint32_t tiles = 0;   // tiles taken from the slot (the pair's global tile count)
        bool ok = true;
        // backward of the pair's next tile (tile t of its group): its slot is taken (tiles + 1
        // published), read, freed, and its gradients accumulated
        float act0 = 0.0f, act1 = 0.0f;   // CP: the action of this lane's env (taken from its tile's slot)
        auto bwd_tile = [&](int t) -> bool {
            STAMP(2);
            if (!wait_ge(flags, tiles + 1, err)) return false;
            STAMP(3);
            // read the whole slot, then free it for the producer's next tile
            const float* h1t = PS + P_H1T;
            const float* dzt = PS + P_DZT;
            // dW1 inputs: raw input j of the tile's envs 4g + e (BS) / 4e + g, e < 4
            float xin[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) xin[e] = PS[P_SOB + (BS ? 4 * g + e : 4 * e + g) * SOS + (j < 12 ? j : 0)];
            f32x4 H1[4], dZ[4], acc[4];
            if constexpr (BS) {
                // dW2 operands over the tile's envs 4g..4g+3 (K = 16 envs), rounded to bf16
                // dW2 on v_mfma_f32_32x32x16_bf16 (as dw2_split32's layout, one product per block): K =
                // the tile's 16 envs, lane half h32 carries envs 8h..8h+7, operands rounded to bf16
                bf16x8 xa8[2], yb8[2];
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float xv[8], yv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        xv[e] = h1t[(8 * h32 + e) * SAS + 32 * b + c32];   // H1[32b + c][env 8h+e]
                        yv[e] = dzt[(8 * h32 + e) * SAS + 32 * b + c32];   // dZ2[32b + c][env 8h+e]
                    }
                    gb2s[b] += ((yv[0] + yv[1]) + (yv[2] + yv[3])) + ((yv[4] + yv[5]) + (yv[6] + yv[7]));   // db2 (f32)
                    xa8[b] = pack8(f32x4{xv[0], xv[1], xv[2], xv[3]}, f32x4{xv[4], xv[5], xv[6], xv[7]});
                    yb8[b] = pack8(f32x4{yv[0], yv[1], yv[2], yv[3]}, f32x4{yv[4], yv[5], yv[6], yv[7]});
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    H1[b] = ld4(h1t + j * SAS + 16 * b + 4 * g);   // accumulator layout
                    dZ[b] = ld4(dzt + j * SAS + 16 * b + 4 * g);
                }
                if (CP && (lane >> 4) == t) {
                    act0 = PS[P_SACT + 2 * (lane & 15)];
                    act1 = PS[P_SACT + 2 * (lane & 15) + 1];
                }
                publish(flags + 1, ++tiles);
                STAMP(13);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) gW2s[mb][nb] = mfma_32k16(xa8[mb], yb8[nb], gW2s[mb][nb]);
                // dH1 = W2 . dZ2: two K = 32 steps, dZ2 in accumulator layout = the B operand
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 db = pack8(dZ[2 * s], dZ[2 * s + 1]);
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb)
                        acc[mb] = mfma_k32(ldbf8(LS + NB_W2B, (((s * 4 + g) * 4 + mb) * 16 + j) * 8), db, acc[mb]);
                }
            } else {
                // split: dW2 on split bf16 32x32x16 MFMAs, x32[b][e] / y32[b][e] over envs 8h+e (dw2_split32);
                // exact: f32 MFMAs, x[s][b] / y[s][b] over env 4s+g (k-step s)
                constexpr bool S2 = SPL;
                float x[4][4], y[4][4];     // exact
                float x32[2][8], y32[2][8];   // split: dw2_split32's operands
                if constexpr (S2) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            x32[b][e] = h1t[(8 * h32 + e) * SAS + 32 * b + c32];   // H1[32b + c][env 8h+e]
                            y32[b][e] = dzt[(8 * h32 + e) * SAS + 32 * b + c32];   // dZ2[32b + c][env 8h+e]
                        }
                } else {
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        x[s][b] = h1t[(4 * s + g) * SAS + 16 * b + j];   // H1[16b + j][env 4s+g]
                        y[s][b] = dzt[(4 * s + g) * SAS + 16 * b + j];   // dZ2[16b + j][env 4s+g]
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    H1[b] = ld4(h1t + j * SAS + 16 * b + 4 * g);   // accumulator layout
                    dZ[b] = ld4(dzt + j * SAS + 16 * b + 4 * g);
                }
                if (CP && (lane >> 4) == t) {
                    act0 = PS[P_SACT + 2 * (lane & 15)];
                    act1 = PS[P_SACT + 2 * (lane & 15) + 1];
                }
                publish(flags + 1, ++tiles);
                STAMP(13);
                // db2 partials and dW2 += H1^T dZ2 over the tile's 16 envs (K = env)
                bf16x8 dpre[2][3];   // split: the dH1 operand pieces, made before the dW2 MFMAs
                if constexpr (S2) {
                    if constexpr (!HLP) {   // HLP: the helper pair's consumer takes dW2 and db2
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            gb2s[b] += ((y32[b][0] + y32[b][1]) + (y32[b][2] + y32[b][3])) +
                                       ((y32[b][4] + y32[b][5]) + (y32[b][6] + y32[b][7]));
                    }
                    split8(dZ[0], dZ[1], dpre[0]);
                    split8(dZ[2], dZ[3], dpre[1]);
                    if constexpr (!HLP) dw2_split32(x32, y32, gW2s);
                } else if constexpr (!HLP) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) gb2[b] += y[s][b];
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
                        for (int nb = 0; nb < 4; ++nb) gW2[mb][nb] = mfma(x[s][mb], y[s][nb], gW2[mb][nb]);
                }
                }
                // dH1 = W2 . dZ2 (A = W2^T image)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) acc[mb] = f32x4{0.f, 0.f, 0.f, 0.f};
                if constexpr (S2) {
                    // one scheduling region with the dW2 MFMAs: the splits first, then 72 x (HLP: 48 x) (one
                    // MFMA, three VALU), so the dH1 splits issue in the bf16 MFMAs' gaps (c4 82.5 ->
                    // 80.7 us per step, c3/c2 -1.5 %; profiles/r03v_cons_sched.txt)
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) {
                            bf16x8 w[3];
                            ld_pieces(LS, NX_W2B, (((s * 4 + g) * 4 + mb) * 16 + j) * 8, w);
                            acc[mb] = mfma_split(w, dpre[s], acc[mb]);
                        }
                    }
                    __builtin_amdgcn_sched_group_barrier(0x002, 40, 0);
#pragma unroll
                    for (int i = 0; i < (HLP ? 48 : 72); ++i) {   // 24 dW2 (32x32x16) + 48 dH1 MFMAs
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                    }
                } else {
                // exact f32, k-step (fb, r) = W2^T row 16fb + 4g + r.  Each fb group of 16 MFMAs is
                // SrcC-fenced and its operands are loaded one group ahead, before the previous
                // group's fence: no load issues while an f32 MFMA of this loop is in flight (the
                // one-step-ahead prefetch let the compiler issue W2^T loads into in-flight SrcC
                // registers 4-5 wait states after the MFMA; see fence_begin).
                f32x4 wc[4], wn[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) wc[r] = ld4(LS + N_W2T + (4 * g + r) * HID + 4 * j);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    if (fb < 3) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) wn[r] = ld4(LS + N_W2T + (16 * (fb + 1) + 4 * g + r) * HID + 4 * j);
                    }
                    fence_begin<true>(acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int mb = 0; mb < 4; ++mb) acc[mb] = mfma(wc[r][mb], dZ[fb][r], acc[mb]);
                    fence_end<true>(acc);
#pragma unroll
                    for (int r = 0; r < 4; ++r) wc[r] = wn[r];
                }
                }
            }
            STAMP(14);
            float* sa = PS + P_SA;
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[mb][r] *= fmaf(-H1[mb][r], H1[mb][r], 1.0f);
                st4(sa + j * SAS + 16 * mb + 4 * g, acc[mb]);
            }
            wave_sync();
            // dW1 (+ db1 as input row 11) += z^T dZ1; A = student-filtered inputs of env 4s+g
            if constexpr (BS) {   // K = the tile's 16 envs (4g + jj), operands rounded to bf16
                float zz[4];
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    zz[jj] = j < 12 ? fminf(fmaxf((xin[jj] - smu) * srs, -5.0f), 5.0f) : 0.0f;
                }
                const s16x4 za = pack4(zz[0], zz[1], zz[2], zz[3]);
#pragma unroll
                for (int nb = 0; nb < 4; ++nb) {
                    const float* c = sa + 16 * nb + j;
                    gW1[nb] = mfma_k16(za, pack4(c[(4 * g) * SAS], c[(4 * g + 1) * SAS], c[(4 * g + 2) * SAS],
                                                 c[(4 * g + 3) * SAS]), gW1[nb]);
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float z = j < 12 ? fminf(fmaxf((xin[s] - smu) * srs, -5.0f), 5.0f) : 0.0f;
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) gW1[nb] = mfma(z, sa[(4 * s + g) * SAS + 16 * nb + j], gW1[nb]);
                }
            }
            wave_sync();   // sa is rewritten by the next tile
            STAMP(15);
            return true;
        };
        // after the last tile of a group (envs base ...): CP steps the envs
        auto end_group = [&](uint32_t base, uint32_t Ck) {
            const uint32_t i = base + (uint32_t)lane;
            const bool lvalid = lane < gs && i < n32;
            if constexpr (CP) {
                STAMP(4);
                if (a.obs_in) {
                    if (lvalid) met_n += 1.0f;
                } else if (lane < gs) {   // act[] rows: published with the group's tiles
                    rd::State st{};
                    if (lvalid) load_state(a.state, a.n, i, st);
                    met_r += env_step_group(a, Ck, i, lvalid, act0, act1, st, met_n);
                }
                STAMP(5);
            }
        };
        if constexpr (HLP) {
            // helper pair 2 + o: dW2 = H1^T dZ2 and db2 of owner o's tile, read from the owner's
            // slot beside the owner consumer's dH1 / dW1 (the owner's producer never rewrites the
            // slot: one tile per owner in this layout)
            if (helper && og < ngroups) {
                const float* OP = lds + TN + SN + (pair & 1) * PSCR;
                STAMP(20);
                ok = wait_ge(reinterpret_cast<const uint32_t*>(OP + P_FLAGS), 1u, err);
                STAMP(21);
                if (ok) {
                    const float* h1t = OP + P_H1T;
                    const float* dzt = OP + P_DZT;
                    if constexpr (SPL) {   // as the plain layout's consumer (dw2_split32)
                        float x32[2][8], y32[2][8];
#pragma unroll
                        for (int e = 0; e < 8; ++e)
#pragma unroll
                            for (int b = 0; b < 2; ++b) {
                                x32[b][e] = h1t[(8 * h32 + e) * SAS + 32 * b + c32];
                                y32[b][e] = dzt[(8 * h32 + e) * SAS + 32 * b + c32];
                            }
#pragma unroll
                        for (int b = 0; b < 2; ++b)
                            gb2s[b] += ((y32[b][0] + y32[b][1]) + (y32[b][2] + y32[b][3])) +
                                       ((y32[b][4] + y32[b][5]) + (y32[b][6] + y32[b][7]));
                        dw2_split32(x32, y32, gW2s);
                    } else {
                    float x[4][4], y[4][4];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            x[s][b] = h1t[(4 * s + g) * SAS + 16 * b + j];
                            y[s][b] = dzt[(4 * s + g) * SAS + 16 * b + j];
                        }
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
#pragma unroll
                            for (int b = 0; b < 4; ++b) gb2[b] += y[s][b];
#pragma unroll
                            for (int mb = 0; mb < 4; ++mb) {
                                fence_begin<true>(gW2[mb]);
#pragma unroll
                                for (int nb = 0; nb < 4; ++nb) gW2[mb][nb] = mfma(x[s][mb], y[s][nb], gW2[mb][nb]);
                                fence_end<true>(gW2[mb]);
                            }
                        }
                    }
                }
                STAMP(22);
            }
        }
        uint32_t gi = 0, tcc = 0;   // TC: groups started, teacher tiles published
        for (uint32_t kk = 0;; ++kk) {
        for (uint32_t grp = gfirst; ok && grp < ngroups; grp += gstride, ++gi) {
            const uint32_t base = grp * (uint32_t)gs;
            const int ntile = (int)min((uint32_t)(gs / TILE), (n32 - base + TILE - 1) / TILE);
            if constexpr (TC) {
                if (!(ok = BS ? wait_ge(flags + 2, gi + 1, err) : wait_ge_uniform(flags + 2, gi + 1, err))) break;
            }
            for (int t = 0; ok && t < ntile; ++t) {
                if constexpr (TC) {
                    // the teacher forward of tile t + 1, if it is this wave's, from the producer's observation
                    // rows, before the backward of tile t: its means go to P_TM (a single buffer: one tile
                    // in flight), read by the producer at tile t + 1 before it publishes that tile.
                    // Order (no deadlock, no overwrite).  The producer publishes tile u after: its own
                    // forward of u; flag [3] of u if u is masked; the slot of u - 1 freed.  This wave frees
                    // the slot of u - 1 in bwd_tile(u - 1) and publishes flag [3] of u before bwd_tile(u - 1),
                    // both without waiting for anything past tile u - 1's publication, so by induction
                    // every tile gets published.  P_TM of u may be overwritten only once the producer has
                    // read it, i.e. once tile u is published.  When this wave writes the means of t + 1 it
                    // has passed bwd_tile(t - 1), so tiles <= t - 1 are published: a masked tile <= t - 1
                    // (0b1010, 0b0010, and the previous group's tiles) has been read.  Only when tile t is
                    // masked too (0b1110: t = 1, 2) may its means still be unread: there the forward runs
                    // first, into registers, and the store waits for tile t's publication -- the same
                    // flag bwd_tile(t) waits for next, which the producer raises without needing the
                    // means of t + 1.
                    if (tc_next(t) && t + 1 < ntile) {
                        const float* obt = PS + P_SO + TILE * (t + 1) * SOS;
                        float m0, m1;
                        STAMP(18);   // (the helper layout's stamp slots: MD_HELPER never runs with a mask)
                        mlp_forward_split(LT, obt, j, g, m0, m1);
                        STAMP(19);
                        if constexpr ((TCM & (TCM >> 1)) != 0) {
                            if (tc_tile(t) && !(ok = wait_ge_uniform(flags, tiles + 1, err))) break;
                        }
                        if (g == 0) {
                            PS[P_TM + 2 * j] = m0;
                            PS[P_TM + 2 * j + 1] = m1;
                        }
                        publish(flags + 3, ++tcc);
                    }
                }
                ok = bwd_tile(t);
            }
            if (!ok) break;
            end_group(base, C + kk);
        }
        if (!KS || !ok || kk + 1 >= (uint32_t)a.ksteps) break;
        }
        // ------------------------------------------------------------ this wave's share
#pragma unroll
        for (int x = 0; x < 4; ++x) gb2[x] = xsum32(xsum16(gb2[x]));   // over the k-groups g
#pragma unroll
        for (int x = 0; x < 2; ++x) gb2s[x] = xsum32(gb2s[x]);          // D32: over the two lane halves
        if constexpr (CP) { met_r = wave_sum(met_r); met_n = wave_sum(met_n); }
        STAMP(6);
        __syncthreads();   // (one of the two barriers every wave meets) weights/scratch are free
        STAMP(9);
        float* R = lds + pair * RPAD;   // rows of RROW floats: W1|b1 rows 0..11, W2 rows 12..75
        if constexpr (D32) {   // 32 x 32 blocks: column lane & 31, row (reg & 3) + 8 (reg >> 2) + 4 h
#pragma unroll
            for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        R[(12 + 32 * mb + (r & 3) + 8 * (r >> 2) + 4 * h32) * RROW + 32 * nb + c32] = gW2s[mb][nb][r];
        } else {
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(12 + 16 * mb + 4 * g + r) * RROW + 16 * nb + j] = gW2[mb][nb][r];
        }
        if (g < 3) {   // rows 4g + r < 12: W1 rows 0..10 and b1 as row 11
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(4 * g + r) * RROW + 16 * nb + j] = gW1[nb][r];
        }
        if constexpr (D32) {
            if (h32 == 0) {
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) R[RSHIFT + P_B2 + 32 * nb + c32] = gb2s[nb];
            }
        } else if (g == 0) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) R[RSHIFT + P_B2 + 16 * nb + j] = gb2[nb];
        }
        if (CP && lane == 0) {   // the producer's region entries past W2 hold the other metrics
            R[RSHIFT + P_TOT] = met_r;
            R[RSHIFT + P_TOT + 3] = met_n;
        }
    }

    // Both roles passed exactly one s_barrier above (a wave-level count on gfx950, so the
    // two call sites pair up); this second one publishes the regions.
    __syncthreads();
    static_assert(RED_COLS % 4 == 0, "a 16-B store stays inside one workspace chunk");
#pragma unroll
    for (int u = 0; u < (P_PAD / 4 + BLOCK - 1) / BLOCK; ++u) {
        const int p4 = threadIdx.x + u * BLOCK;
        if (p4 < P_PAD / 4) {
            const int q = ridx(4 * p4);   // 4 | 64: the four entries stay contiguous
            gst<BS>(reinterpret_cast<f32x4*>(a.ws + ws_index(4 * p4, blockIdx.x, gridDim.x)),
                       sum4(ld4(lds + q), ld4(lds + RPAD + q), ld4(lds + 2 * RPAD + q), ld4(lds + 3 * RPAD + q)));
        }
    }
    STAMP(7);
    RTSTAMP(17);
}
