// distill.hip, part 5 of 5: the kernels beside the training step -- rdd_reset's and
// rdd_set_env_state's (reset_state_kernel, check_state_kernel, init_ctl_kernel), the policy query
// (forward_kernel) and the whole-episode evaluation (EvalArgs, evaluate_kernel).
// Expects distill_layout.h, distill_forward.h, rd_device.h and rd_physics.h.
#pragma once

__global__ __launch_bounds__(256) void reset_state_kernel(int64_t n, int64_t env_base, uint64_t seed, float* state) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float d[6];
    rd::philox_draw(seed, (uint64_t)(env_base + i), 0u, d);
    rd::State st;
    rd::env_reset(st, d);
    rd::store_state(state, n, i, st);
}

// rdd_set_env_state's range check: the fused rollout takes its joint trig on the short paths
// (rd_physics.h, kWideRange = false: joint 1 on the hardware within its limit, joint 0 reduced by
// 2 pi below 8192 rad), which an episode's own states never leave; a caller's state outside that
// range (or not finite) raises flag[0]
__global__ __launch_bounds__(256) void check_state_kernel(int64_t n, const float* state, uint32_t* flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float q0 = state[i], q1 = state[n + i];
    if (!(fabsf(q0) < rd::kRolloutMaxQ0) || !(fabsf(q1) <= rd::kRolloutMaxQ1))
        __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the ctl words (distill_reduce.h) at a reset
__global__ __launch_bounds__(256) void init_ctl_kernel(uint32_t* ctl, float b1, float b2) {
    if (threadIdx.x < 2) {
        const int o = 4 * threadIdx.x;   // live words and their snapshot
        ctl[o] = 0u; ctl[o + 1] = 0u; ctl[o + 2] = __float_as_uint(b1); ctl[o + 3] = __float_as_uint(b2);
    }
    if (threadIdx.x >= 8 && threadIdx.x < 16) ctl[threadIdx.x] = threadIdx.x == 12 ? 1u : 0u;
}

// policy query: obs rows -> pdflat of teacher and/or student (one 16-env tile per wave pass)
template <bool BS>
__global__ __launch_bounds__(FBLOCK) void forward_kernel(const float* tnet, const float* snet, const float* obs,
                                                         int64_t n, float* tflat, float* sflat) {
    __shared__ __attribute__((aligned(16))) float lds[NET + NET_S + FWAVES * TILE * SOS];
    load_net(lds, tnet, false, FBLOCK);
    if constexpr (BS) load_net_bf16(lds + NET, snet, FBLOCK);
    else load_net(lds + NET, snet, false, FBLOCK);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    float* ob = lds + NET + NET_S + wave * TILE * SOS;
    const int64_t ntiles = (n + TILE - 1) / TILE;
    for (int64_t t = (int64_t)blockIdx.x * FWAVES + wave; t < ntiles; t += (int64_t)gridDim.x * FWAVES) {
        // raw observations of the tile's 16 envs -> scratch rows (component 11 = 1)
        for (int x = lane; x < TILE * SOS; x += 64) {
            const int e = x / SOS, k = x % SOS;
            const int64_t i = t * TILE + e;
            ob[x] = k == OBD ? 1.0f : (i < n ? obs[i * OBD + k] : 0.0f);
        }
        wave_sync();
        const int64_t i = t * TILE + j;
        f32x4 H1[4], H2[4];
        float m0, m1;
        for (int net = 0; net < 2; ++net) {
            float* out = net ? sflat : tflat;
            if (!out) continue;   // wave-uniform
            const float* L = lds + net * NET;
            float ls0 = L[N_LS], ls1 = L[N_LS + 1];
            if (BS && net == 1) {
                mlp_forward_bf16(L, ob, j, g, H1, H2, m0, m1);
                ls0 = L[NB_LS]; ls1 = L[NB_LS + 1];
            } else {
                // BS: beside the bf16 student's forward hipcc issues an LDS load into the SrcC of
                // one of the teacher's in-flight f32 MFMAs (hazards.py LDSRC): fenced (see fence_begin)
                mlp_forward<BS>(L, ob, j, g, H1, H2, m0, m1);
            }
            if (i < n && g == 0) {
                out[i * 4 + 0] = m0;
                out[i * 4 + 1] = m1;
                out[i * 4 + 2] = ls0;
                out[i * 4 + 3] = ls1;
            }
        }
        wave_sync();
    }
}

// ---------------------------------------------------------------- whole-episode evaluation
// rdd_evaluate: one launch rolls n evaluation envs through E consecutive 50-step episodes under
// one policy's mean action (DESIGN.md §3 "Evaluation").  A wave owns a group of gs envs (64, or 16
// for a small batch) for the whole launch: the state stays in registers (one env per lane), the
// raw observations and the actions pass through a per-wave LDS scratch between the env-per-lane
// physics and the 16-env MFMA tiles of the forward, the weights stay in LDS.  The arithmetic is
// that of the stepwise path -- rd_reset / rd_step's rd::env_reset, rd::observe<true>,
// rd::env_step<true>, and forward_kernel's mlp_forward / mlp_forward_bf16 on the same load_net
// images -- and every env's chain is independent of its tile mates, so returns, final
// distances and records are bitwise those of rdd_forward + rd_step, whatever gs and the grid.
constexpr int EWAVES = 8, EBLOCK = 64 * EWAVES;
constexpr int E_SO = 0;                          // [64][SOS] raw obs (component 11 = 1)
constexpr int E_ACT = E_SO + GROUP * SOS;        // [64][2] the stepping policy's means
constexpr int ESCR = E_ACT + GROUP * 2;
constexpr int EREC = rd::kObsDim + 1 + 4 + 4 + 1;   // dataset.py's record: ob | reward | t_pdflat | s_pdflat | stepped_with
constexpr int E_NS = NETB_S > NET ? NETB_S : NET;   // the student's forward image, f32 (no W2^T) or bf16
constexpr int E_LDS = NET + E_NS + EWAVES * ESCR;
static_assert(ESCR % 4 == 0 && E_NS % 4 == 0 && 2 * E_LDS * 4 <= 160 * 1024, "evaluation LDS: two workgroups per CU");

struct EvalArgs {
    int64_t n, env_base;
    uint64_t seed;
    const float* tnet;
    const float* snet;
    const float* draws;      // [E][n][6] or null (Philox)
    float* returns;          // [E][n]
    float* final_dist;       // [E][n] or null
    float* records;          // [E][n][50][EREC] or null
    int student, episodes, first_episode, gs;
};

// f32 instance: <= 128 VGPRs, so that the two workgroups a CU's LDS holds are resident (4 waves
// per SIMD: one wave's physics issues beside another's MFMAs); the bf16 instance would spill there
template <bool BS>
__global__ __launch_bounds__(EBLOCK, BS ? 2 : 4) void evaluate_kernel(EvalArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[E_LDS];
    const bool run_t = !a.student || a.records, run_s = a.student != 0;
    if (run_t) load_net(lds, a.tnet, false, EBLOCK);
    if (run_s) {
        if constexpr (BS) load_net_bf16(lds + NET, a.snet, EBLOCK);
        else load_net(lds + NET, a.snet, false, EBLOCK);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    float* so = lds + NET + E_NS + wave * ESCR + E_SO;
    float* sact = lds + NET + E_NS + wave * ESCR + E_ACT;
    const float* LT = lds;
    const float* LS = lds + NET;
    const int64_t n = a.n, ngroups = (n + a.gs - 1) / a.gs;
    for (int64_t grp = blockIdx.x + (int64_t)wave * gridDim.x; grp < ngroups; grp += (int64_t)gridDim.x * EWAVES) {
        const int64_t base = grp * a.gs;
        const int cnt = (int)(n - base < a.gs ? n - base : a.gs);   // envs of this group
        const int ntile = (cnt + TILE - 1) / TILE;
        const bool valid = lane < cnt;
        const int64_t i = base + (valid ? lane : 0);
        rd::State st;
        float prev = 0.0f;   // the reward this env's previous step returned (records)
        for (int e = 0; e < a.episodes; ++e) {
            float d[6];
            if (a.draws) {
                const float* p = a.draws + ((int64_t)e * n + i) * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) d[k] = p[k];
            } else {
                rd::philox_draw(a.seed, (uint64_t)(a.env_base + i), (uint32_t)(a.first_episode + e), d);
            }
            rd::env_reset(st, d);
            float ret = 0.0f;
            float* rec = a.records ? a.records + ((int64_t)e * n + i) * (rd::kEpisodeSteps * EREC) : nullptr;
            for (int s = 0; s < rd::kEpisodeSteps; ++s) {
                float ob[rd::kObsDim];
                rd::observe<true>(st, ob);
#pragma unroll
                for (int k = 0; k < rd::kObsDim; ++k) so[lane * SOS + k] = ob[k];
                so[lane * SOS + OBD] = 1.0f;
                wave_sync();
                for (int t = 0; t < ntile; ++t) {   // wave-uniform
                    const float* tob = so + t * TILE * SOS;
                    const bool out = g == 0 && t * TILE + j < cnt;
                    float* trec = rec ? a.records + (((int64_t)e * n + base + t * TILE + (out ? j : 0)) *
                                                     rd::kEpisodeSteps + s) * EREC + rd::kObsDim + 1
                                      : nullptr;
                    f32x4 H1[4], H2[4];
                    float m0 = 0.0f, m1 = 0.0f;
                    if (run_t) {
                        // fenced (see fence_begin): unfenced, hipcc issues the next k-steps' weight loads into
                        // SrcC registers of in-flight f32 MFMAs here (hazards.py LDSRC, 11 sites); the
                        // fence changes the schedule only, not a bit of the result
                        mlp_forward<true>(LT, tob, j, g, H1, H2, m0, m1);
                        if (trec && out) {
                            trec[0] = m0; trec[1] = m1; trec[2] = LT[N_LS]; trec[3] = LT[N_LS + 1];
                        }
                    }
                    if (run_s) {
                        float ls0, ls1;
                        if constexpr (BS) {
                            mlp_forward_bf16(LS, tob, j, g, H1, H2, m0, m1);
                            ls0 = LS[NB_LS]; ls1 = LS[NB_LS + 1];
                        } else {
                            mlp_forward<true>(LS, tob, j, g, H1, H2, m0, m1);
                            ls0 = LS[N_LS]; ls1 = LS[N_LS + 1];
                        }
                        if (trec && out) {
                            trec[4] = m0; trec[5] = m1; trec[6] = ls0; trec[7] = ls1;
                        }
                    } else if (trec && out) {
                        trec[4] = 0.0f; trec[5] = 0.0f; trec[6] = 0.0f; trec[7] = 0.0f;
                    }
                    if (g == 0) {   // the tile's means: env-per-lane again through the scratch
                        sact[(t * TILE + j) * 2] = m0;
                        sact[(t * TILE + j) * 2 + 1] = m1;
                    }
                }
                wave_sync();
                const float a0 = valid ? sact[lane * 2] : 0.0f, a1 = valid ? sact[lane * 2 + 1] : 0.0f;
                if (rec && valid) {
                    float* r = rec + s * EREC;
#pragma unroll
                    for (int k = 0; k < rd::kObsDim; ++k) r[k] = ob[k];
                    r[rd::kObsDim] = prev;
                    r[EREC - 1] = a.student ? 1.0f : 0.0f;
                }
                prev = rd::env_step<true>(st, a0, a1);
                ret += prev;
            }
            if (valid) {
                a.returns[(int64_t)e * n + i] = ret;
                if (a.final_dist) a.final_dist[(int64_t)e * n + i] = rd::tip_distance(st);
            }
        }
    }
}
