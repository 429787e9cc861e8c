// Fused rollout + distillation step for gfx950 (include/reacher_distill.h).
//
// One launch of rollout_kernel runs, for every env, one iteration of the reference's hot
// loop (mlp_train.py:143-204): observation -> teacher MlpPolicy (teacher.py:14-16) ->
// student MlpPolicy -> loss (loss.py:3-13 KL, or action-MSE) -> student backward ->
// env.step(action) with auto-reset; per-workgroup gradient partials go to a workspace.
// reduce_adam_kernel then sums the partials and applies TF1 Adam (mlp_train.py:73-80).
//
// MI355X mapping:
//  * 512-thread workgroups (8 waves = 2 per SIMD, <= 256 VGPR+AGPR each) so that one
//    wave's VALU work (physics, tanh, staging) issues while its SIMD partner's MFMAs run.
//  * a wave owns a GROUP of 64 envs: the physics runs once per env (one env per lane);
//    the networks run on 16-env TILES (4 per group) with v_mfma_f32_16x16x4_f32 in the
//    transposed orientation Z^T[feature x env] = W^T[feature x in] . X^T[in x env]:
//    lane l = (env j = l&15, k-group g = l>>4); a layer's accumulator (features 4g+r in
//    registers, env on the lane) IS the B operand of the next layer (k-step r uses the
//    features {4g + r}), so activations never leave registers in the forward/backward
//    chain.  Layer-1 bias rides in the K padding (input 11 = 1).
//  * weights of both nets live in LDS for the whole launch as [k][j][fb] images (one
//    conflict-free ds_read_b128 feeds the 4 MFMAs of a k-step, prefetched a step ahead);
//    the student also keeps W2^T for dH1 = W2 . dZ2.
//  * weight gradients (sums over envs) are MFMAs with the env as K: H1, dZ2 and dZ1 are
//    transposed through a per-wave LDS scratch (private to the wave: ordered by a
//    wave-level barrier, never s_barrier); accumulators persist across the wave's tiles
//    and are reduced once per workgroup, in a fixed order (deterministic).
//  * exact f32 arithmetic throughout (f32-input MFMA = k-ordered fmaf chain).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "../../include/reacher_distill.h"
#include "rd_comm_impl.h"
#include "rd_common.h"
#include "rd_host.h"
#include "rd_device.h"
#include "rd_physics.h"

namespace {

using rd::f32x4, rd::mfma, rd::ld4, rd::st4, rd::wave_sum, rd::wave_sync, rd::kTanhScale, rd::tanh_pre, rd::load_state;

// Diagnostic build only (-DRD_STAMPS, libreacher_stamps.so): per-wave s_memtime stamps
// of rollout_kernel's phases into a debug buffer nothing else reads.
#ifdef RD_STAMPS
#define STAMP(idx)                                                                      \
    do {                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                              \
        unsigned long long t_;                                                          \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
        __builtin_amdgcn_sched_barrier(0);                                              \
        if (lane == 0 && a.dbg) a.dbg[(blockIdx.x * WAVES + wave) * NSTAMP + (idx)] += t_;   \
    } while (0)
// s_memrealtime (100 MHz) at kernel start/end: with the s_memtime stamps, the shader clock
#define RTSTAMP(idx)                                                                    \
    do {                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                              \
        const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                 \
        __builtin_amdgcn_sched_barrier(0);                                              \
        if (lane == 0 && a.dbg) a.dbg[(blockIdx.x * WAVES + wave) * NSTAMP + (idx)] += t_;   \
    } while (0)
#else
#define STAMP(idx) do {} while (0)
#define RTSTAMP(idx) do {} while (0)
#endif

// the device code by concern (DESIGN.md §3 has the map), in the order its definitions depend on
#include "distill_layout.h"
#include "distill_forward.h"
#include "distill_reduce.h"
#include "distill_rollout.h"
#include "distill_eval.h"

}  // namespace

struct rdd_trainer {
    rdd_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    int grid = 0;
    rd::DeviceAllocs mem;      // every device buffer below
    float* state = nullptr;    // [8][n]
    float* tnet = nullptr;     // [P + 22]
    float* snet = nullptr;     // [P + 22]
    float* timg = nullptr;     // [NET]   teacher LDS image
    float* simg = nullptr;     // [NET_S] student LDS image
    float* m = nullptr;
    float* v = nullptr;
    float* grad = nullptr;     // [P] (own or bound)
    float* own_grad = nullptr;
    float* ws = nullptr;       // partials of up to ws_rows workgroups (ws_index layout)
    float* hist = nullptr;     // [hist_len][4]
    uint32_t* ctl = nullptr;   // [16]: step words, snapshot, [8] hand-off timeout flag
    unsigned long long* dbg = nullptr;   // RD_STAMPS builds only
    int last_grid = 0;                   // workgroups of the last rollout (rows of ws to reduce)
    int last_gs = GROUP, last_hlp = 0, last_mode = 0;   // ... its group size, helper layout, 0 env / 1 obs / 2 rows
    int last_tcm = 0;                    // ... and the tiles whose teacher forward the consumer wave ran (mask)
    int tcm = 0;                         // that mask for the f32-split student's K = 1 launches (cfg.teacher_tiles)
    int ws_rows = 0;                     // rows of ws (the device's CU count, or cfg.grid)
    int cus = 0;                         // the device's CU count (rdd_evaluate's grid: no query per launch)
    int gs = GROUP;                      // envs per group of the env rollout
    int accum = 1;                       // rollouts per optimiser step (MSE normalisation)
    rd_comm* comm = nullptr;             // bound RCCL communicator (multi-GPU), not owned
};

namespace {

// Envs per group (one producer/consumer pair steps a group of gs envs, gs/16 tiles at a
// time): 64 fills every lane of the physics and is fastest from one group per pair up
// (measured: c3 = one 64-env group per pair 39.6 us vs 41.9 with 32-env groups); below
// that a pair's tiles run serially while most CUs idle, so small batches use 32- or 16-env
// groups over more pairs (c2, 4,096 envs: 19.1 us per launch vs 35.4 with 64-env groups).
// rdd_config.group_envs = 16|32|64 fixes it (tests: the group size changes only the
// summation order).
int group_envs(int64_t n, int pairs_total, int fixed) {
    if (fixed) return fixed;
    if (n >= (int64_t)GROUP * pairs_total) return 64;
    if (n >= (int64_t)32 * pairs_total) return 32;
    return 16;
}

// LDS image kinds and sizes (floats) of a trainer's teacher and student
int teacher_kind(const rdd_trainer* t) { return t->cfg.f32_split ? IMG_SPLIT : IMG_F32; }
int student_kind(const rdd_trainer* t) {
    return t->cfg.student_dtype == RDD_DTYPE_BF16 ? IMG_BF16 : (t->cfg.f32_split ? IMG_SPLIT : IMG_F32);
}
int image_floats(int kind, bool student) {
    if (kind == IMG_SPLIT) return student ? NETX_S : NETX;
    if (kind == IMG_BF16) return NETB_S;
    return student ? NET_S : NET;
}

// Which wave of a pair steps the envs.  The bf16 student (BASELINE config 5):
// the consumer, after its last tile of a group (the actions travel with each tile's slot):
// this balances the roles, since the producer's forward (f32 teacher + bf16 student) is the
// longer one.  Its MFMAs are all bf16 (XDL: the compiler protects their SrcC) except the
// exact teacher's f32 ones, which are SrcC-fenced.  The f32 student: the producer steps the
// envs it computed the actions for (a consumer-side step there measured c4 -0.8 %, c3 +2.7 %,
// c2 +3.7 % and would need the consumer's f32 MFMAs fenced; profiles/r03h_cp_f32_and_nopack.txt).
int grid_for(int64_t n, int gs, int cap) {
    const int64_t want = ((n + gs - 1) / gs + PAIRS - 1) / PAIRS;   // one group per pair at least
    return (int)(want < cap ? want : cap);
}

// Which tiles of a group take their teacher forward from the consumer wave (rollout_kernel's TCM;
// DESIGN.md §3 "Where a pair's time goes").  The bf16 student's kernel is built with 0b1010 only.
// The f32-split student's K = 1 teacher-mode kernel exists with none, one, two or three of a
// group's four tiles moved; rdd_config.teacher_tiles picks one, -1 the default below.  Tile 1 alone
// is the fastest at every batch size and group size measured (c4 -1.4 us per step, c3 -0.6): the
// consumer runs it while it would wait for the group's first tile; with two or three tiles moved
// the consumer ends last (profiles/r07_teacher_tiles_ab.txt).
constexpr int kTeacherTilesDefault = 0b0010;
bool teacher_tiles_ok(int m) { return m == -1 || m == 0 || m == 0b0010 || m == 0b1010 || m == 0b1110; }

ReduceArgs reduce_args(const rdd_trainer* t, int reduce, int adam, int accum) {
    ReduceArgs a;
    a.ws = t->ws;
    a.nblk = t->last_grid;
    a.grad = t->grad;
    a.params = t->snet;
    a.m = t->m;
    a.v = t->v;
    a.ctl = t->ctl;
    a.hist = t->hist;
    a.hist_len = t->cfg.metrics_len;
    a.reduce = reduce;
    a.adam = adam;
    a.accum = accum;
    a.bump_env = reduce;
    a.bump_opt = adam;
    a.lr = t->cfg.lr;
    a.b1 = t->cfg.beta1;
    a.b2 = t->cfg.beta2;
    a.eps = t->cfg.eps;
    a.simg = t->simg;
    a.img_kind = student_kind(t);
    a.xerr = rd_comm_device_err(t->comm);
    return a;
}

int launch_rollout(rdd_trainer* t, const float* obs_in = nullptr, int64_t n_obs = 0, int64_t n_obs_global = 0,
                   const float* tflat_in = nullptr, int ksteps = 1) {
    RolloutArgs a;
    a.ksteps = ksteps;
    a.n = obs_in ? n_obs : t->cfg.n_envs;
    a.obs_in = obs_in;
    a.timg = t->timg;
    a.simg = t->simg;
    a.env_base = t->cfg.env_base;
    a.seed = t->cfg.seed;
    a.state = t->state;
    a.tnet = tflat_in ? tflat_in : t->tnet;   // rows mode: the recorded teacher outputs
    a.snet = t->snet;
    a.ctl = t->ctl;
    a.ws = t->ws;
    a.loss = t->cfg.loss;
    a.act_student = t->cfg.act_with == RDD_ACT_STUDENT;
    a.stagger = t->cfg.stagger;
    a.dbg = t->dbg;
    // MSE averages over the envs of all ranks and over the accum_steps rollouts of one optimiser step
    a.inv_n_global = obs_in ? 1.0f / (float)n_obs_global : 1.0f / ((float)t->cfg.n_envs_global * (float)t->accum);
    int grid = t->grid;   // <= t->ws_rows, the partial rows the workspace holds
    a.gs = t->gs;
    if (obs_in) {
        a.gs = group_envs(n_obs, t->ws_rows * PAIRS, t->cfg.group_envs);
        grid = grid_for(n_obs, a.gs, t->ws_rows);
    }
    const bool bs = t->cfg.student_dtype == RDD_DTYPE_BF16, spl = t->cfg.f32_split != 0;
    // helper pairs (f32 student): every group one 16-env tile and at most two groups per
    // workgroup -- the batch would leave half the pairs idle or hold one tile each, so pairs 2,
    // 3 run the owners' teacher forwards on the other SIMDs instead (c2: DESIGN.md §3)
    const int64_t ngroups = (a.n + a.gs - 1) / a.gs;
    const bool hlp = !bs && !tflat_in && a.gs == TILE && ngroups <= 2 * (int64_t)t->ws_rows &&
                     t->cfg.group_envs == 0 &&   // a fixed group size keeps the plain layout
                     ksteps == 1;                // K env steps per launch: the plain layout
    if (hlp) grid = (int)((ngroups + 1) / 2);
    t->last_grid = grid;
    t->last_gs = a.gs;
    t->last_hlp = hlp;
    t->last_mode = tflat_in ? 2 : (obs_in ? 1 : 0);
    // the f32-split student's plain K = 1 teacher-mode launch (env or obs): the instance of the trainer's mask
    const int tcm = !bs && spl && !hlp && !tflat_in && ksteps == 1 ? t->tcm : 0;
    t->last_tcm = bs && spl && !tflat_in && ksteps == 1 ? 0b1010 : tcm;
    void (*k)(RolloutArgs) =
        bs ? (spl ? rollout_kernel<true, true, true, MD_TEACHER, false, 0b1010>   // DESIGN.md §3 "c5"
                  : rollout_kernel<true, false, true, MD_TEACHER>)
           : hlp ? (spl ? rollout_kernel<false, true, false, MD_HELPER> : rollout_kernel<false, false, false, MD_HELPER>)
                 : (spl ? (tcm == 0b1110   ? rollout_kernel<false, true, false, MD_TEACHER, false, 0b1110>
                           : tcm == 0b1010 ? rollout_kernel<false, true, false, MD_TEACHER, false, 0b1010>
                           : tcm == 0b0010 ? rollout_kernel<false, true, false, MD_TEACHER, false, 0b0010>
                                           : rollout_kernel<false, true, false, MD_TEACHER>)
                        : rollout_kernel<false, false, false, MD_TEACHER>);
    if (ksteps > 1)   // K steps per launch: the producer steps the envs it reads (no CP)
        k = bs ? (spl ? rollout_kernel<true, true, false, MD_TEACHER, true> : rollout_kernel<true, false, false, MD_TEACHER, true>)
               : (spl ? rollout_kernel<false, true, false, MD_TEACHER, true> : rollout_kernel<false, false, false, MD_TEACHER, true>);
    if (tflat_in)   // the teacher is not run: the bf16 student's kernel does not depend on the teacher's mode
        k = bs ? rollout_kernel<true, false, false, MD_ROWS>
               : (spl ? rollout_kernel<false, true, false, MD_ROWS> : rollout_kernel<false, false, false, MD_ROWS>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), 0, t->stream, a);
    RD_HIP(hipGetLastError(), "rollout_kernel launch");
    return RD_OK;
}

// reduce: partials -> grad (accum: +=) and advance the env clock; adam: TF1 Adam and
// advance the optimiser step
int launch_reduce(rdd_trainer* t, int reduce, int adam, int accum = 0) {
    const ReduceArgs a = reduce_args(t, reduce, adam, accum);
    hipLaunchKernelGGL(reduce_adam_kernel, dim3(RED_GRID), dim3(RED_BLOCK), 0, t->stream, a);
    RD_HIP(hipGetLastError(), "reduce_adam_kernel launch");
    return RD_OK;
}

}  // namespace

extern "C" {

int rdd_param_count(void) { return P_TOT; }

int rdd_set_stream(rdd_trainer* t, void* hip_stream) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_set_stream: null handle");
    t->stream = (hipStream_t)hip_stream;
    return RD_OK;
}

int rdd_create(rdd_trainer** out, const rdd_config* cfg, int device, void* hip_stream) {
    if (!out || !cfg) return rd::set_error(RD_EINVAL, "rdd_create: null argument");
    if (cfg->n_envs <= 0 || cfg->n_envs_global < cfg->n_envs || cfg->env_base < 0 ||
        cfg->n_envs > ((int64_t)1 << 31) || (cfg->loss != RDD_LOSS_MSE && cfg->loss != RDD_LOSS_KL) ||
        (cfg->act_with != RDD_ACT_TEACHER && cfg->act_with != RDD_ACT_STUDENT) || !(cfg->lr > 0) ||
        cfg->grid < 0 || cfg->metrics_len < 0 || (cfg->stagger != 0 && cfg->stagger != 1) ||
        (cfg->student_dtype != RDD_DTYPE_F32 && cfg->student_dtype != RDD_DTYPE_BF16) || cfg->accum_steps < 0 ||
        (cfg->f32_split != 0 && cfg->f32_split != 1) ||
        (cfg->group_envs != 0 && cfg->group_envs != 16 && cfg->group_envs != 32 && cfg->group_envs != 64))
        return rd::set_error(RD_EINVAL, "rdd_create: bad config");
    if (!teacher_tiles_ok(cfg->teacher_tiles))
        return rd::set_error(RD_EINVAL, "rdd_create: teacher_tiles %d is not built (-1 default, 0, 2 = 0b0010, "
                                        "10 = 0b1010, 14 = 0b1110)", (int)cfg->teacher_tiles);
    rd::DeviceGuard g(device);
    RD_HIP(g.err, "rdd_create: hipSetDevice");
    rdd_trainer* t = new (std::nothrow) rdd_trainer();
    if (!t) return rd::set_error(RD_EINVAL, "rdd_create: out of host memory");
    t->cfg = *cfg;
    if (t->cfg.metrics_len == 0) t->cfg.metrics_len = 4096;
    t->accum = cfg->accum_steps > 1 ? cfg->accum_steps : 1;
    t->device = device;
    t->stream = (hipStream_t)hip_stream;
    t->cus = rd::cu_count(device);
    const int cap = cfg->grid > 0 ? cfg->grid : t->cus;
    t->ws_rows = cap;
    t->gs = group_envs(cfg->n_envs, cap * PAIRS, cfg->group_envs);
    t->grid = grid_for(cfg->n_envs, t->gs, cap);
    t->last_grid = t->grid;
    t->last_gs = t->gs;
    t->tcm = cfg->teacher_tiles < 0 ? kTeacherTilesDefault : cfg->teacher_tiles;
    const size_t netf = P_TOT + 2 * OBD;
    rd::DeviceAllocs& mem = t->mem;
    mem.stream = t->stream;
    mem.zeroed(&t->state, (size_t)8 * cfg->n_envs);
    mem.zeroed(&t->tnet, netf);
    mem.zeroed(&t->snet, netf);
    mem.zeroed(&t->timg, image_floats(teacher_kind(t), false));
    mem.zeroed(&t->simg, image_floats(student_kind(t), true));
    mem.zeroed(&t->m, P_TOT);
    mem.zeroed(&t->v, P_TOT);
    mem.zeroed(&t->own_grad, P_TOT);
    t->grad = t->own_grad;
    mem.zeroed(&t->ws, (size_t)t->ws_rows * P_WS);
    mem.zeroed(&t->hist, (size_t)t->cfg.metrics_len * N_MET);
    mem.zeroed(&t->ctl, 16);
#ifdef RD_STAMPS
    mem.zeroed(&t->dbg, (size_t)t->ws_rows * WAVES * NSTAMP);
#endif
    if (mem.err != hipSuccess) {
        const hipError_t e = mem.err;
        rdd_destroy(t);
        return rd::hip_fail(e, "rdd_create: allocation");
    }
    *out = t;
    return RD_OK;
}

int rdd_destroy(rdd_trainer* t) {
    if (!t) return RD_OK;
    rd::DeviceGuard g(t->device);
    t->mem.free_all();
    delete t;
    return RD_OK;
}

static int set_net(rdd_trainer* t, float* dst, const float* params, const float* mu, const float* sd,
                   const char* what) {
    if (!t || !params || !mu || !sd) return rd::set_error(RD_EINVAL, "%s: null argument", what);
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, what);
    if (int rc = rd::upload_net(what, dst, params, P_TOT, mu, sd, OBD, t->stream)) return rc;
    const bool student = dst == t->snet;
    const int kind = student ? student_kind(t) : teacher_kind(t);
    hipLaunchKernelGGL(pack_net_kernel, dim3(1), dim3(256), 0, t->stream, dst, student ? t->simg : t->timg,
                       image_floats(kind, student), student ? 1 : 0, kind);
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

int rdd_set_teacher(rdd_trainer* t, const float* p, const float* mu, const float* sd) {
    return set_net(t, t ? t->tnet : nullptr, p, mu, sd, "rdd_set_teacher");
}

int rdd_set_student(rdd_trainer* t, const float* p, const float* mu, const float* sd) {
    return set_net(t, t ? t->snet : nullptr, p, mu, sd, "rdd_set_student");
}

int rdd_get_student(rdd_trainer* t, float* params) {
    if (!t || !params) return rd::set_error(RD_EINVAL, "rdd_get_student: null argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_get_student");
    RD_HIP(hipMemcpyAsync(params, t->snet, sizeof(float) * P_TOT, hipMemcpyDeviceToDevice, t->stream),
           "rdd_get_student");
    return RD_OK;
}

int rdd_reset(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_reset: null handle");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_reset: hipSetDevice");
    const int64_t n = t->cfg.n_envs;
    hipLaunchKernelGGL(reset_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, n,
                       t->cfg.env_base, t->cfg.seed, t->state);
    hipLaunchKernelGGL(init_ctl_kernel, dim3(1), dim3(64), 0, t->stream, t->ctl, t->cfg.beta1, t->cfg.beta2);
    RD_HIP(hipMemsetAsync(t->m, 0, sizeof(float) * P_TOT, t->stream), "rdd_reset");
    RD_HIP(hipMemsetAsync(t->v, 0, sizeof(float) * P_TOT, t->stream), "rdd_reset");
    RD_HIP(hipGetLastError(), "rdd_reset: launch");
    return RD_OK;
}

int rdd_rollout(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_rollout: null handle");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_rollout: hipSetDevice");
    if (int rc = launch_rollout(t)) return rc;
    return launch_reduce(t, 1, 0);
}

// a bound exchange that failed earlier (reacher_comm.h): no further steps on this trainer
static int comm_ok(const rdd_trainer* t, const char* what) {
    if (rd_comm_failed(t->comm))
        return rd::set_error(RD_ECOMM, "%s: a gradient exchange of this trainer failed (its optimiser step was "
                                       "skipped); destroy the communicator", what);
    return RD_OK;
}

int rdd_rollout_accum(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_rollout_accum: null handle");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_rollout_accum: hipSetDevice");
    if (int rc = launch_rollout(t, nullptr, 0, 0, nullptr, t->accum)) return rc;
    return launch_reduce(t, 1, 0);
}

int rdd_apply(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_apply: null handle");
    if (int rc = comm_ok(t, "rdd_apply")) return rc;
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_apply: hipSetDevice");
    return launch_reduce(t, 0, 1);
}

int rdd_step(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_step: null handle");
    if (int rc = comm_ok(t, "rdd_step")) return rc;
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_step: hipSetDevice");
    if (int rc = launch_rollout(t)) return rc;
    if (!t->comm) return launch_reduce(t, 1, 1);
    // sharded step: the exchange sits between the reduction and Adam, all on one stream
    if (int rc = launch_reduce(t, 1, 0)) return rc;
    if (int rc = rd_comm_allreduce_f32(t->comm, t->grad, P_TOT, t->stream)) return rc;
    return launch_reduce(t, 0, 1);
}

int rdd_step_accum(rdd_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_step_accum: null handle");
    if (int rc = comm_ok(t, "rdd_step_accum")) return rc;
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_step_accum: hipSetDevice");
    if (int rc = launch_rollout(t, nullptr, 0, 0, nullptr, t->accum)) return rc;
    if (!t->comm) return launch_reduce(t, 1, 1);
    if (int rc = launch_reduce(t, 1, 0)) return rc;
    if (int rc = rd_comm_allreduce_f32(t->comm, t->grad, P_TOT, t->stream)) return rc;
    return launch_reduce(t, 0, 1);
}

int rdd_bind_comm(rdd_trainer* t, rd_comm* comm) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_bind_comm: null handle");
    t->comm = comm;
    return RD_OK;
}

int rdd_allreduce_grad(rdd_trainer* t) {
    if (!t || !t->comm) return rd::set_error(RD_EINVAL, "rdd_allreduce_grad: no communicator bound");
    if (int rc = comm_ok(t, "rdd_allreduce_grad")) return rc;
    return rd_comm_allreduce_f32(t->comm, t->grad, P_TOT, t->stream);
}

int rdd_rollout_obs(rdd_trainer* t, const float* obs, int64_t n, int64_t n_global) {
    if (!t || !obs || n <= 0 || n > ((int64_t)1 << 31) || n_global < n)
        return rd::set_error(RD_EINVAL, "rdd_rollout_obs: bad argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_rollout_obs: hipSetDevice");
    if (int rc = launch_rollout(t, obs, n, n_global)) return rc;
    return launch_reduce(t, 1, 0);
}

int rdd_step_obs(rdd_trainer* t, const float* obs, int64_t n) {
    if (!t || !obs || n <= 0 || n > ((int64_t)1 << 31)) return rd::set_error(RD_EINVAL, "rdd_step_obs: bad argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_step_obs: hipSetDevice");
    if (int rc = launch_rollout(t, obs, n, n)) return rc;
    return launch_reduce(t, 1, 1);
}

static int rows_args(rdd_trainer* t, const float* obs, const float* t_pdflat, int64_t n, int64_t n_global,
                     const char* what) {
    if (!t || !obs || !t_pdflat || n <= 0 || n > ((int64_t)1 << 31) || n_global < n)
        return rd::set_error(RD_EINVAL, "%s: bad argument", what);
    if (((uintptr_t)t_pdflat & 15) != 0) return rd::set_error(RD_EINVAL, "%s: t_pdflat must be 16-byte aligned", what);
    return RD_OK;
}

int rdd_rollout_rows(rdd_trainer* t, const float* obs, const float* t_pdflat, int64_t n, int64_t n_global) {
    if (int rc = rows_args(t, obs, t_pdflat, n, n_global, "rdd_rollout_rows")) return rc;
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_rollout_rows: hipSetDevice");
    if (int rc = launch_rollout(t, obs, n, n_global, t_pdflat)) return rc;
    return launch_reduce(t, 1, 0);
}

int rdd_step_rows(rdd_trainer* t, const float* obs, const float* t_pdflat, int64_t n) {
    if (int rc = rows_args(t, obs, t_pdflat, n, n, "rdd_step_rows")) return rc;
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_step_rows: hipSetDevice");
    if (int rc = launch_rollout(t, obs, n, n, t_pdflat)) return rc;
    return launch_reduce(t, 1, 1);
}

int rdd_launch_stage(rdd_trainer* t, int stage) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_launch_stage: null handle");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_launch_stage: hipSetDevice");
    switch (stage) {
        case RDD_STAGE_ROLLOUT: return launch_rollout(t);
        case RDD_STAGE_REDUCE: return launch_reduce(t, 1, 0);
        case RDD_STAGE_APPLY: return launch_reduce(t, 0, 1);
        case RDD_STAGE_REDUCE_APPLY: return launch_reduce(t, 1, 1);
        case RDD_STAGE_REDUCE_ACCUM: return launch_reduce(t, 1, 0, 1);
        case RDD_STAGE_REDUCE_ACCUM_APPLY: return launch_reduce(t, 1, 1, 1);
        default: return rd::set_error(RD_EINVAL, "rdd_launch_stage: bad stage %d", stage);
    }
}

float* rdd_grad_buffer(rdd_trainer* t) { return t ? t->grad : nullptr; }

int rdd_bind_grad_buffer(rdd_trainer* t, float* grad) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_bind_grad_buffer: null handle");
    t->grad = grad ? grad : t->own_grad;
    return RD_OK;
}

int rdd_forward(rdd_trainer* t, const float* obs, int64_t n, float* tflat, float* sflat) {
    if (!t || !obs || n <= 0) return rd::set_error(RD_EINVAL, "rdd_forward: bad argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_forward: hipSetDevice");
    const int64_t ntiles = (n + TILE - 1) / TILE;
    int64_t blocks = (ntiles + FWAVES - 1) / FWAVES;
    if (blocks > 2 * rd::cu_count(t->device)) blocks = 2 * rd::cu_count(t->device);
    if (t->cfg.student_dtype == RDD_DTYPE_BF16)
        hipLaunchKernelGGL(forward_kernel<true>, dim3((unsigned)blocks), dim3(FBLOCK), 0, t->stream, t->tnet, t->snet,
                           obs, n, tflat, sflat);
    else
        hipLaunchKernelGGL(forward_kernel<false>, dim3((unsigned)blocks), dim3(FBLOCK), 0, t->stream, t->tnet,
                           t->snet, obs, n, tflat, sflat);
    RD_HIP(hipGetLastError(), "forward_kernel launch");
    return RD_OK;
}

int rdd_evaluate(rdd_trainer* t, const rdd_eval_config* cfg, float* returns, float* final_dist, float* records) {
    if (!t || !cfg || !returns) return rd::set_error(RD_EINVAL, "rdd_evaluate: null trainer, config or returns");
    if (cfg->n_envs < 1 || cfg->n_envs > ((int64_t)1 << 31))
        return rd::set_error(RD_EINVAL, "rdd_evaluate: n_envs %lld outside 1 .. 2^31", (long long)cfg->n_envs);
    if (cfg->episodes < 1) return rd::set_error(RD_EINVAL, "rdd_evaluate: episodes %d < 1", cfg->episodes);
    if (cfg->policy != RDD_EVAL_TEACHER && cfg->policy != RDD_EVAL_STUDENT)
        return rd::set_error(RD_EINVAL, "rdd_evaluate: unknown policy %d", cfg->policy);
    if (cfg->env_base < 0 || cfg->first_episode < 0 || cfg->grid < 0)
        return rd::set_error(RD_EINVAL, "rdd_evaluate: negative env_base, first_episode or grid");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_evaluate: hipSetDevice");
    EvalArgs a;
    a.n = cfg->n_envs;
    a.env_base = cfg->env_base;
    a.seed = cfg->seed;
    a.tnet = t->tnet;
    a.snet = t->snet;
    a.draws = cfg->draws;
    a.returns = returns;
    a.final_dist = final_dist;
    a.records = records;
    a.student = cfg->policy == RDD_EVAL_STUDENT;
    a.episodes = cfg->episodes;
    a.first_episode = cfg->first_episode;
    // two workgroups fit a CU (LDS); below one 64-env group per resident wave, 16-env groups
    // (one tile per wave and step) spread a small batch over the CUs, as group_envs() does
    const int cap = cfg->grid > 0 ? cfg->grid : 2 * t->cus;
    a.gs = a.n >= (int64_t)GROUP * cap * EWAVES ? GROUP : TILE;
    const int64_t ngroups = (a.n + a.gs - 1) / a.gs;
    const unsigned grid = (unsigned)(ngroups < cap ? ngroups : cap);
    if (t->cfg.student_dtype == RDD_DTYPE_BF16)
        hipLaunchKernelGGL(evaluate_kernel<true>, dim3(grid), dim3(EBLOCK), 0, t->stream, a);
    else
        hipLaunchKernelGGL(evaluate_kernel<false>, dim3(grid), dim3(EBLOCK), 0, t->stream, a);
    RD_HIP(hipGetLastError(), "evaluate_kernel launch");
    return RD_OK;
}

int rdd_get_env_state(rdd_trainer* t, float* state) {
    if (!t || !state) return rd::set_error(RD_EINVAL, "rdd_get_env_state: null argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_get_env_state");
    RD_HIP(hipMemcpyAsync(state, t->state, sizeof(float) * 8 * t->cfg.n_envs, hipMemcpyDeviceToDevice, t->stream),
           "rdd_get_env_state");
    return RD_OK;
}

int rdd_set_env_state(rdd_trainer* t, const float* state) {
    if (!t || !state) return rd::set_error(RD_EINVAL, "rdd_set_env_state: null argument");
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, "rdd_set_env_state");
    // the caller's angles are checked before they replace the trainer's (ctl[14]: this check's flag)
    const int64_t n = t->cfg.n_envs;
    uint32_t bad = 0;
    RD_HIP(hipMemsetAsync(t->ctl + 14, 0, sizeof(uint32_t), t->stream), "rdd_set_env_state");
    hipLaunchKernelGGL(check_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, t->stream, n, state,
                       t->ctl + 14);
    RD_HIP(hipGetLastError(), "rdd_set_env_state: check_state_kernel launch");
    RD_HIP(hipMemcpyAsync(&bad, t->ctl + 14, sizeof(bad), hipMemcpyDeviceToHost, t->stream), "rdd_set_env_state");
    RD_HIP(hipStreamSynchronize(t->stream), "rdd_set_env_state");
    if (bad)
        return rd::set_error(RD_EINVAL,
                             "rdd_set_env_state: a joint angle outside the fused rollout's range (|q0| < %g, |q1| <= %g "
                             "rad, finite); the gym-API env (rd_set_state) takes any state",
                             (double)rd::kRolloutMaxQ0, (double)rd::kRolloutMaxQ1);
    RD_HIP(hipMemcpyAsync(t->state, state, sizeof(float) * 8 * n, hipMemcpyDeviceToDevice, t->stream),
           "rdd_set_env_state");
    return RD_OK;
}

static int read_ctl(rdd_trainer* t, uint32_t (&c)[16], const char* what) {
    rd::DeviceGuard g(t->device);
    RD_HIP(g.err, what);
    RD_HIP(hipMemcpyAsync(c, t->ctl, sizeof(c), hipMemcpyDeviceToHost, t->stream), what);
    RD_HIP(hipStreamSynchronize(t->stream), what);
    if (c[8]) return rd::set_error(RD_EINVAL, "%s: a rollout's producer/consumer hand-off timed out", what);
    if (c[13]) return rd::set_error(RD_ECOMM, "%s: a gradient exchange failed; its optimiser step was skipped", what);
    return RD_OK;
}

int rdd_get_counter(rdd_trainer* t, int64_t* steps) {
    if (!t || !steps) return rd::set_error(RD_EINVAL, "rdd_get_counter: null argument");
    uint32_t c[16];
    if (int rc = read_ctl(t, c, "rdd_get_counter")) return rc;
    *steps = c[0];
    return RD_OK;
}

int rdd_get_counters(rdd_trainer* t, int64_t* env_steps, int64_t* opt_steps) {
    if (!t) return rd::set_error(RD_EINVAL, "rdd_get_counters: null handle");
    uint32_t c[16];
    if (int rc = read_ctl(t, c, "rdd_get_counters")) return rc;
    if (env_steps) *env_steps = c[0];
    if (opt_steps) *opt_steps = c[1];
    return RD_OK;
}

int rdd_read_metrics(rdd_trainer* t, int64_t count, double* out) {
    if (!t || !out || count < 0) return rd::set_error(RD_EINVAL, "rdd_read_metrics: bad argument");
    int64_t steps = 0;   // metrics are kept per optimiser step
    if (int rc = rdd_get_counters(t, nullptr, &steps)) return rc;
    return rd::read_ring("rdd_read_metrics", "steps", t->hist, t->cfg.metrics_len, N_MET, steps, count, out);
}

int rdd_last_layout(const rdd_trainer* t, int32_t out[5]) {
    if (!t || !out) return rd::set_error(RD_EINVAL, "rdd_last_layout: null argument");
    out[0] = t->last_gs;
    out[1] = t->last_grid;
    out[2] = t->last_hlp;
    out[3] = t->last_mode;
    out[4] = t->last_tcm;
    return RD_OK;
}

#ifdef RD_STAMPS
// Diagnostic build only: copy (and zero) the per-wave stamp sums [grid*8][16] to the host.
int rdd_debug_stamps(rdd_trainer* t, unsigned long long* out, int64_t cap) {
    if (!t || !out || !t->dbg) return rd::set_error(RD_EINVAL, "rdd_debug_stamps: bad argument");
    const int64_t cnt = (int64_t)t->ws_rows * WAVES * NSTAMP;
    if (cap < cnt) return rd::set_error(RD_EINVAL, "rdd_debug_stamps: need %lld", (long long)cnt);
    RD_HIP(hipStreamSynchronize(t->stream), "rdd_debug_stamps");
    RD_HIP(hipMemcpy(out, t->dbg, sizeof(unsigned long long) * cnt, hipMemcpyDeviceToHost), "rdd_debug_stamps");
    RD_HIP(hipMemset(t->dbg, 0, sizeof(unsigned long long) * cnt), "rdd_debug_stamps");
    return (int)cnt;
}
#endif

}  // extern "C"
