// The reference's own MLP student (include/reacher_student_mlp.h): forward and one
// distillation training step over a batch of rows, for gfx950.
//
// Graph (reference student_nn.py:51-57): 16 -> 24 tanh -> 128 tanh -> 128 -> 32 tanh -> 4.
// Unlike the 2x64 MlpPolicy path (distill.hip), a 16-row tile cannot keep the whole chain
// plus its 24,380 weight gradients in one wave's registers, so a workgroup of 8 waves
// cooperates on 64-row blocks (16-row blocks for small batches, where 64-row blocks would
// leave CUs idle):
//  * every layer is a small GEMM over the block, v_mfma_f32_16x16x4_f32 in the natural
//    orientation (rows x features): A = the block's activations in LDS ([row][feature],
//    row stride = width + 4 so the 16 rows x 4 k of one A operand hit 64 distinct banks),
//    B = the layer's weights, a padded [in][out] image read through L1/L2 (98 KB, shared
//    by every workgroup on the chip);
//  * all activations of the block stay in LDS (139 KB) between the forward and the
//    backward; the backward reuses dead buffers (dZ1 overwrites H3 after dW3 is taken);
//  * weight gradients dW_l = H_{l-1}^T dZ_l are MFMAs with the 64 rows as K; each wave
//    owns a fixed subset of the 100 16x16 gradient blocks and accumulates them in
//    registers across the workgroup's row blocks; bias gradients are per-thread column
//    sums.  One workspace row per workgroup, summed in a fixed order by the Adam kernel
//    (deterministic, no atomics);
//  * exact f32 products (f32-input MFMA); tanh = 1 - 2 / (2^(2 log2(e) z) + 1);
//  * rdm_create_dtype(.., RDM_DTYPE_BF16, ..): the three wide layers run on v_mfma_f32_16x16x32_bf16
//    instead (student_mlp_bf16.h), in BF = true instances of the same kernels.
//
// One translation unit: the device code is the student_mlp_*.h that student_mlp_device.h includes, in
// the order the kernels stand in the object -- the closed-loop evaluation over whole episodes
// (rdm_evaluate) in student_mlp_eval.h, the persistent envs of the batched on-policy step
// (rdm_step_envs) in student_mlp_envs.h, their common step in student_mlp_query.h -- and
// student_mlp_optim.h.  This file keeps rdm_trainer, the choice of the row block, one launch function
// per kernel family, and the C ABI.  (The closed loop's mixed, noisy and faulty instances -- DAgger's
// beta-mixture, action noise, sensor faults on the student's observation -- are compiled in
// student_mlp_mix.hip, student_mlp_noise.hip and student_mlp_faults.hip: student_mlp_acting.h.)
#include <stdlib.h>

#include <new>

#include "student_mlp_device.h"
// after the ABI header, whose codes it returns
#include "rd_host.h"

namespace {

// PIdx, param_index, store_param, pack_kernel, reduce_adam_kernel, init_ctl_kernel
#include "student_mlp_optim.h"

}  // namespace


struct rdm_trainer {
    rdm_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    int grid = 0;               // workspace rows
    int last_grid = 0;          // workgroups of the last training launch
    rd::DeviceAllocs mem;       // every buffer below but the envs'
    float* params = nullptr;    // [P_REF] f32 master
    float* img = nullptr;       // [IMG_ALL] weight image (forward + backward layouts; f32, then bf16)
    bool bf = false;            // rdm_create_dtype's RDM_DTYPE_BF16: the BF = true instances of every kernel
    float* m = nullptr;
    float* v = nullptr;
    float* grad = nullptr;
    float* own_grad = nullptr;
    float* ws = nullptr;        // [grid][WS_ROW]
    float* hist = nullptr;      // [metrics_len][4]
    uint32_t* ctl = nullptr;    // [8]
    float* tnet = nullptr;      // rdm_evaluate's teacher: params [tch::P_TOT] | ob mean [11] | ob std [11]
    bool has_teacher = false;
    rd::EnvBufs envs;           // the persistent envs (rdm_envs_attach): state [8][n], aux [ENV_AUX][n], clock
    rd::Acting act;             // how the envs calls act (rdm_envs_set_*, rdm_envs_bind_*)
};

namespace {

// 16-row blocks for small batches: they are latency-bound, and four times the workgroups
// run the rows in parallel (measured, scripts/bench_student_mlp.py: the reference's 200-row
// step 21.8 us vs 35.8 us with 64-row blocks, 1,024 rows 27.2 vs 37.4 us).  Every workgroup
// writes a 104 KB partial row, so once the 16-row blocks would occupy more than half of the
// workgroups the 64-row kernel wins (4,096 rows: 51.2 vs 42.4 us).
bool use_small_rows(int64_t n, int grid) {
    return (n + 15) / 16 <= grid / 2;
}

// rdm_evaluate's block of envs, by the same reasoning: a step is a latency chain (physics, five
// layers, six barriers), so 16-env blocks over four times the workgroups are faster while every
// block has a CU of its own.  No partial rows are written here, so the rule holds up to one block
// per workgroup of the grid, not half of them (scripts/bench_evaluate_student_mlp.py,
// profiles/evaluate_student_mlp_fused_vs_stepwise.json "fused_by_block_size", one episode: 4,096
// envs 341 us with 16-env blocks vs 577 us with 64-env blocks; 8,192 envs, two 16-env blocks per
// CU, 673 vs 578 us).
bool eval_small_rows(int64_t n, int grid) {
    return (n + 15) / 16 <= grid;
}

// A launch over n rows (or envs) on at most cap workgroups: 16-row blocks where `small_rows` says
// so, else 64-row blocks; a block of rows per workgroup pass, one workgroup per block up to cap.
// teacher_waves: the closed-loop kernels' workgroup (ELay), else the training kernel's.
struct Blocks {
    bool small;
    unsigned grid, threads;
};
Blocks blocks_of(int64_t n, int cap, bool (*small_rows)(int64_t, int), bool teacher_waves) {
    const bool small = small_rows(n, cap);
    const int rows = small ? 16 : 64;
    const int64_t nblk = (n + rows - 1) / rows;
    return {small, (unsigned)(nblk < cap ? nblk : cap),
            (unsigned)(!teacher_waves ? BLOCK : small ? ELay<16>::THREADS : ELay<64>::THREADS)};
}

// student_mlp_kernel's arguments: the forward reads x and the image only
SmArgs sm_args(const rdm_trainer* t, bool train, const float* x, const float* tgt, float* out, int64_t n,
               int64_t n_global) {
    SmArgs a{};
    a.x = x;
    a.tgt = tgt;
    a.out = out;
    a.n = n;
    a.img = t->img;
    a.keep_prob = 1.0f;
    if (train) {
        a.ws = t->ws;
        a.ctl = t->ctl;
        a.loss = t->cfg.loss;
        a.inv_n_global = 1.0f / (float)n_global;
        a.keep_prob = t->cfg.keep_prob;
        a.seed = t->cfg.seed;
        a.row_base = t->cfg.row_base;
    }
    return a;
}

// One launch of student_mlp_kernel, `what` naming it in the error.  The callers pick the instance
// (the order in which the instances are first named is the order of the kernels in the object).
int launch_rows(rdm_trainer* t, void (*kern)(SmArgs), const Blocks& b, const SmArgs& a, const char* what) {
    hipLaunchKernelGGL(kern, dim3(b.grid), dim3(b.threads), 0, t->stream, a);
    RD_HIP(hipGetLastError(), what);
    return RD_OK;
}

int launch_train(rdm_trainer* t, const float* x, const float* tgt, int64_t n, int64_t n_global) {
    const Blocks b = blocks_of(n, t->grid, use_small_rows, false);
    t->last_grid = (int)b.grid;
    auto* kern = t->bf ? (b.small ? student_mlp_kernel<true, 16, true> : student_mlp_kernel<true, 64, true>)
                       : (b.small ? student_mlp_kernel<true, 16, false> : student_mlp_kernel<true, 64, false>);
    return launch_rows(t, kern, b, sm_args(t, true, x, tgt, nullptr, n, n_global), "student_mlp_kernel launch");
}

int launch_adam(rdm_trainer* t, int reduce, int adam) {
    AdamArgs a;
    a.ws = t->ws;
    a.nblk = t->last_grid;
    a.grad = t->grad;
    a.params = t->params;
    a.img = t->img;
    a.m = t->m;
    a.v = t->v;
    a.ctl = t->ctl;
    a.hist = t->hist;
    a.hist_len = t->cfg.metrics_len;
    a.reduce = reduce;
    a.adam = adam;
    a.lr = t->cfg.lr;
    a.b1 = t->cfg.beta1;
    a.b2 = t->cfg.beta2;
    a.eps = t->cfg.eps;
    auto* kern = t->bf ? reduce_adam_kernel<true> : reduce_adam_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(ADAM_GRID), dim3(ADAM_BLOCK), 0, t->stream, a);
    RD_HIP(hipGetLastError(), "student_mlp reduce_adam_kernel launch");
    return RD_OK;
}

bool bad_rows(const float* x, int64_t n) {
    return !x || n <= 0 || n > ((int64_t)1 << 31) || ((uintptr_t)x & 15) != 0;
}

SmEnvsArgs envs_args(const rdm_trainer* t) {
    SmEnvsArgs a{};
    a.n = t->envs.n;
    a.env_base = t->envs.base;
    a.seed = t->envs.seed;
    a.tnet = t->tnet;
    a.img = t->img;
    a.state = t->envs.state;
    a.aux = t->envs.aux;
    a.clock = t->envs.clock;
    return a;
}

// The argument checks of rdm_envs_act / rdm_rollout_envs / rdm_step_envs, `fn` naming the caller:
// everything that needs no handle first, then what the handle says.
int envs_check(const char* fn, const rdm_trainer* t, int act_with, int steps, const float* x, const float* t_pdflat) {
    if (!t) return rd::set_error(RD_EINVAL, "%s: null trainer", fn);
    if (!x) return rd::set_error(RD_EINVAL, "%s: null x", fn);
    if (!t_pdflat) return rd::set_error(RD_EINVAL, "%s: null t_pdflat", fn);
    if (((uintptr_t)x & 15) != 0) return rd::set_error(RD_EINVAL, "%s: x is not 16-byte aligned", fn);
    if (((uintptr_t)t_pdflat & 15) != 0) return rd::set_error(RD_EINVAL, "%s: t_pdflat is not 16-byte aligned", fn);
    if (steps < 1) return rd::set_error(RD_EINVAL, "%s: steps %d < 1", fn, steps);
    if (act_with != RDM_ACT_TEACHER && act_with != RDM_ACT_STUDENT)
        return rd::set_error(RD_EINVAL, "%s: unknown act_with %d", fn, act_with);
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "%s: no envs attached (rdm_envs_attach)", fn);
    if (t->envs.n > ((int64_t)1 << 31) / steps)
        return rd::set_error(RD_EINVAL, "%s: steps x n_envs = %d x %lld rows > 2^31", fn, steps, (long long)t->envs.n);
    if (!t->has_teacher) return rd::set_error(RD_EINVAL, "%s: no teacher set (rdm_set_teacher)", fn);
    return rd::check_bound_rows(fn, t->act, steps, t->envs.n);
}

// K env steps of every env: a block of envs per workgroup for the whole launch, sized as rdm_evaluate's
int launch_envs(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat, float* reward) {
    SmEnvsArgs a = envs_args(t);
    a.x = x;
    a.t_pdflat = t_pdflat;
    a.s_pdflat = s_pdflat;
    a.reward = reward;
    a.steps = steps;
    const Blocks b = blocks_of(a.n, t->envs.grid > 0 ? t->envs.grid : t->grid, eval_small_rows, true);
    // the teacher-acts instances run no student layer: one arithmetic
    const bool stu = act_with == RDM_ACT_STUDENT;
    auto* kern = stu && t->bf ? (b.small ? student_mlp_envs_kernel<16, true, true> : student_mlp_envs_kernel<64, true, true>)
                 : b.small    ? (stu ? student_mlp_envs_kernel<16, true, false> : student_mlp_envs_kernel<16, false, false>)
                              : (stu ? student_mlp_envs_kernel<64, true, false> : student_mlp_envs_kernel<64, false, false>);
    if (!stu && t->act.stepped_with)   // the teacher stepped every row
        RD_HIP(hipMemsetAsync(t->act.stepped_with, 0, sizeof(float) * (size_t)steps * (size_t)a.n, t->stream),
               "student_mlp_envs_kernel: stepped_with");
    const rd::MlpEnvsLaunch l{&a, &t->act, stu, t->bf, b.small, b.grid, b.threads, t->stream};
    switch (rd::tier_of(t->act, stu)) {
        case rd::Tier::Faulty: RD_HIP(rd::launch_mlp_envs_faulty(l), "student_mlp_envs_kernel (faulty) launch"); break;
        case rd::Tier::Noisy: RD_HIP(rd::launch_mlp_envs_noisy(l), "student_mlp_envs_kernel (noisy) launch"); break;
        case rd::Tier::Mixed: RD_HIP(rd::launch_mlp_envs_mixed(l), "student_mlp_envs_kernel (mixed) launch"); break;
        case rd::Tier::Plain:
            hipLaunchKernelGGL(kern, dim3(b.grid), dim3(b.threads), 0, t->stream, a);
            RD_HIP(hipGetLastError(), "student_mlp_envs_kernel launch");
    }
    return RD_OK;
}

// act, then the training launch on the K n rows just written, as rdm_rollout / rdm_step run it
int envs_train(const char* fn, rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat,
               float* reward, int adam) {
    if (int rc = envs_check(fn, t, act_with, steps, x, t_pdflat)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, fn);
    if (int rc = launch_envs(t, act_with, steps, x, t_pdflat, s_pdflat, reward)) return rc;
    const int64_t rows = (int64_t)steps * t->envs.n;
    if (int rc = launch_train(t, x, t_pdflat, rows, rows)) return rc;
    return launch_adam(t, 1, adam);
}

}  // namespace

extern "C" {

int rdm_param_count(void) { return P_REF; }

int rdm_create(rdm_trainer** out, const rdm_config* cfg, int device, void* hip_stream) {
    return rdm_create_dtype(out, cfg, RDM_DTYPE_F32, device, hip_stream);
}

int rdm_create_dtype(rdm_trainer** out, const rdm_config* cfg, int32_t dtype, int device, void* hip_stream) {
    if (!out || !cfg) return rd::set_error(RD_EINVAL, "rdm_create: null argument");
    if ((cfg->loss != RDM_LOSS_MSE && cfg->loss != RDM_LOSS_KL) || !(cfg->lr > 0) || cfg->grid < 0 ||
        cfg->metrics_len < 0 || !(cfg->keep_prob > 0.0f && cfg->keep_prob <= 1.0f) || cfg->row_base < 0)
        return rd::set_error(RD_EINVAL, "rdm_create: bad config");
    if (dtype != RDM_DTYPE_F32 && dtype != RDM_DTYPE_BF16)
        return rd::set_error(RD_EINVAL, "rdm_create_dtype: unknown dtype %d", (int)dtype);
    rd::DeviceGuard dg(device);
    RD_HIP(dg.err, "rdm_create: hipSetDevice");
    rdm_trainer* t = new (std::nothrow) rdm_trainer();
    if (!t) return rd::set_error(RD_EINVAL, "rdm_create: out of host memory");
    t->cfg = *cfg;
    t->bf = dtype == RDM_DTYPE_BF16;
    if (t->cfg.metrics_len == 0) t->cfg.metrics_len = 4096;
    t->device = device;
    t->stream = (hipStream_t)hip_stream;
    t->grid = cfg->grid > 0 ? cfg->grid : rd::cu_count(device);
    t->last_grid = 0;
    rd::DeviceAllocs& mem = t->mem;
    mem.stream = t->stream;
    mem.zeroed(&t->params, P_REF);
    mem.zeroed(&t->img, IMG_ALL);
    mem.zeroed(&t->m, P_REF);
    mem.zeroed(&t->v, P_REF);
    mem.zeroed(&t->own_grad, P_REF);
    mem.zeroed(&t->ws, (size_t)t->grid * WS_ROW);
    mem.zeroed(&t->hist, (size_t)t->cfg.metrics_len * N_MET);
    mem.zeroed(&t->ctl, 8);
    mem.zeroed(&t->tnet, tch::P_TOT + 2 * tch::OBD);
    t->grad = t->own_grad;
    if (mem.err != hipSuccess) {
        const hipError_t e = mem.err;
        rdm_destroy(t);
        return rd::hip_fail(e, "rdm_create: allocation");
    }
    if (int rc = rdm_reset(t)) {
        rdm_destroy(t);
        return rc;
    }
    *out = t;
    return RD_OK;
}

int rdm_destroy(rdm_trainer* t) {
    if (!t) return RD_OK;
    rd::DeviceGuard dg(t->device);
    t->mem.free_all();
    t->envs.release();
    delete t;
    return RD_OK;
}

int rdm_set_stream(rdm_trainer* t, void* hip_stream) {
    if (!t) return rd::set_error(RD_EINVAL, "rdm_set_stream: null handle");
    t->stream = (hipStream_t)hip_stream;
    return RD_OK;
}

int rdm_set_params(rdm_trainer* t, const float* params) {
    if (!t || !params) return rd::set_error(RD_EINVAL, "rdm_set_params: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_set_params");
    RD_HIP(hipMemcpyAsync(t->params, params, sizeof(float) * P_REF, hipMemcpyDeviceToDevice, t->stream),
           "rdm_set_params");
    auto* kern = t->bf ? pack_kernel<true> : pack_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((P_REF + 255) / 256), dim3(256), 0, t->stream, (const float*)t->params, t->img);
    RD_HIP(hipGetLastError(), "rdm_set_params: pack");
    return RD_OK;
}

int rdm_get_params(rdm_trainer* t, float* params) {
    if (!t || !params) return rd::set_error(RD_EINVAL, "rdm_get_params: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_get_params");
    RD_HIP(hipMemcpyAsync(params, t->params, sizeof(float) * P_REF, hipMemcpyDeviceToDevice, t->stream),
           "rdm_get_params");
    return RD_OK;
}

int rdm_reset(rdm_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdm_reset: null handle");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_reset");
    RD_HIP(hipMemsetAsync(t->m, 0, sizeof(float) * P_REF, t->stream), "rdm_reset");
    RD_HIP(hipMemsetAsync(t->v, 0, sizeof(float) * P_REF, t->stream), "rdm_reset");
    hipLaunchKernelGGL(init_ctl_kernel, dim3(1), dim3(64), 0, t->stream, t->ctl, t->cfg.beta1, t->cfg.beta2);
    RD_HIP(hipGetLastError(), "rdm_reset: launch");
    return RD_OK;
}

int rdm_forward(rdm_trainer* t, const float* x, int64_t n, float* pdflat) {
    if (!t || bad_rows(x, n) || !pdflat) return rd::set_error(RD_EINVAL, "rdm_forward: bad argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_forward");
    const Blocks b = blocks_of(n, t->grid, use_small_rows, false);
    auto* kern = t->bf ? (b.small ? student_mlp_kernel<false, 16, true> : student_mlp_kernel<false, 64, true>)
                       : (b.small ? student_mlp_kernel<false, 16, false> : student_mlp_kernel<false, 64, false>);
    return launch_rows(t, kern, b, sm_args(t, false, x, nullptr, pdflat, n, 0), "student_mlp_kernel (forward) launch");
}

int rdm_rollout(rdm_trainer* t, const float* x, const float* t_pdflat, int64_t n, int64_t n_global) {
    if (!t || bad_rows(x, n) || !t_pdflat || ((uintptr_t)t_pdflat & 15) != 0 || n_global < n)
        return rd::set_error(RD_EINVAL, "rdm_rollout: bad argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_rollout");
    if (int rc = launch_train(t, x, t_pdflat, n, n_global)) return rc;
    return launch_adam(t, 1, 0);
}

int rdm_apply(rdm_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdm_apply: null handle");
    if (t->last_grid == 0) return rd::set_error(RD_EINVAL, "rdm_apply: no rollout yet");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_apply");
    return launch_adam(t, 0, 1);
}

int rdm_step(rdm_trainer* t, const float* x, const float* t_pdflat, int64_t n) {
    if (!t || bad_rows(x, n) || !t_pdflat || ((uintptr_t)t_pdflat & 15) != 0)
        return rd::set_error(RD_EINVAL, "rdm_step: bad argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_step");
    if (int rc = launch_train(t, x, t_pdflat, n, n)) return rc;
    return launch_adam(t, 1, 1);
}

float* rdm_grad_buffer(rdm_trainer* t) { return t ? t->grad : nullptr; }

int rdm_bind_grad_buffer(rdm_trainer* t, float* grad) {
    if (!t) return rd::set_error(RD_EINVAL, "rdm_bind_grad_buffer: null handle");
    t->grad = grad ? grad : t->own_grad;
    return RD_OK;
}

int rdm_get_counter(rdm_trainer* t, int64_t* opt_steps) {
    if (!t || !opt_steps) return rd::set_error(RD_EINVAL, "rdm_get_counter: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_get_counter");
    uint32_t c[8];
    RD_HIP(hipMemcpyAsync(c, t->ctl, sizeof(c), hipMemcpyDeviceToHost, t->stream), "rdm_get_counter");
    RD_HIP(hipStreamSynchronize(t->stream), "rdm_get_counter");
    *opt_steps = c[0];
    return RD_OK;
}

int rdm_read_metrics(rdm_trainer* t, int64_t count, double* out) {
    if (!t || !out || count < 0) return rd::set_error(RD_EINVAL, "rdm_read_metrics: bad argument");
    int64_t steps = 0;
    if (int rc = rdm_get_counter(t, &steps)) return rc;
    return rd::read_ring("rdm_read_metrics", "steps", t->hist, t->cfg.metrics_len, N_MET, steps, count, out);
}

int rdm_set_teacher(rdm_trainer* t, const float* params, const float* ob_mean, const float* ob_std) {
    if (!t || !params || !ob_mean || !ob_std) return rd::set_error(RD_EINVAL, "rdm_set_teacher: null argument");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_set_teacher");
    if (int rc = rd::upload_net("rdm_set_teacher", t->tnet, params, tch::P_TOT, ob_mean, ob_std, tch::OBD, t->stream))
        return rc;
    t->has_teacher = true;
    return RD_OK;
}

}  // extern "C"

namespace {

// rdm_evaluate (nz = of = null), rdm_evaluate_noisy (of = null) and rdm_evaluate_faulty (nz = null: the
// mean acts), `fn` naming the caller; the tier follows from the settings given (rd::tier_of)
int evaluate(const char* fn, rdm_trainer* t, const rdm_eval_config* cfg, const rd_action_noise* nz,
             const rd_obs_faults* of, float* returns, float* final_dist, float* records) {
    if (!t || !cfg || !returns) return rd::set_error(RD_EINVAL, "%s: null trainer, config or returns", fn);
    if (cfg->n_envs < 1 || cfg->n_envs > ((int64_t)1 << 31))
        return rd::set_error(RD_EINVAL, "%s: n_envs %lld outside 1 .. 2^31", fn, (long long)cfg->n_envs);
    if (cfg->episodes < 1) return rd::set_error(RD_EINVAL, "%s: episodes %d < 1", fn, cfg->episodes);
    if (cfg->env_base < 0 || cfg->first_episode < 0 || cfg->grid < 0)
        return rd::set_error(RD_EINVAL, "%s: negative env_base, first_episode or grid", fn);
    if (!t->has_teacher) return rd::set_error(RD_EINVAL, "%s: no teacher set (rdm_set_teacher)", fn);
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, fn);
    SmEvalArgs a;
    a.n = cfg->n_envs;
    a.env_base = cfg->env_base;
    a.seed = cfg->seed;
    a.tnet = t->tnet;
    a.img = t->img;
    a.draws = cfg->draws;
    a.returns = returns;
    a.final_dist = final_dist;
    a.records = records;
    a.episodes = cfg->episodes;
    a.first_episode = cfg->first_episode;
    // a block of envs per workgroup for the whole launch, sized as rdm_forward sizes its row block
    const Blocks b = blocks_of(a.n, cfg->grid > 0 ? cfg->grid : t->grid, eval_small_rows, true);
    auto* kern = t->bf ? (b.small ? student_mlp_evaluate_kernel<16, true> : student_mlp_evaluate_kernel<64, true>)
                       : (b.small ? student_mlp_evaluate_kernel<16, false> : student_mlp_evaluate_kernel<64, false>);
    rd::Acting act;
    if (nz) act.noise = *nz;
    if (of) act.faults = *of;
    const rd::MlpEvalLaunch l{&a, &act, t->bf, b.small, b.grid, b.threads, t->stream};
    switch (rd::tier_of(act, true)) {
        case rd::Tier::Faulty: RD_HIP(rd::launch_mlp_eval_faulty(l), "student_mlp_evaluate_kernel (faulty) launch"); break;
        case rd::Tier::Noisy: RD_HIP(rd::launch_mlp_eval_noisy(l), "student_mlp_evaluate_kernel (noisy) launch"); break;
        default:
            hipLaunchKernelGGL(kern, dim3(b.grid), dim3(b.threads), 0, t->stream, a);
            RD_HIP(hipGetLastError(), "student_mlp_evaluate_kernel launch");
    }
    return RD_OK;
}

}  // namespace

extern "C" {

int rdm_evaluate(rdm_trainer* t, const rdm_eval_config* cfg, float* returns, float* final_dist, float* records) {
    return evaluate("rdm_evaluate", t, cfg, nullptr, nullptr, returns, final_dist, records);
}

int rdm_evaluate_noisy(rdm_trainer* t, const rdm_eval_config* cfg, const rd_action_noise* nz, float* returns,
                       float* final_dist, float* records) {
    if (int rc = rd::check_action_noise("rdm_evaluate_noisy", nz, false)) return rc;
    return evaluate("rdm_evaluate_noisy", t, cfg, nz, nullptr, returns, final_dist, records);
}

int rdm_evaluate_faulty(rdm_trainer* t, const rdm_eval_config* cfg, const rd_obs_faults* of, const rd_action_noise* nz,
                        float* returns, float* final_dist, float* records) {
    if (int rc = rd::check_obs_faults("rdm_evaluate_faulty", of, false)) return rc;
    if (nz) {
        if (int rc = rd::check_action_noise("rdm_evaluate_faulty", nz, true)) return rc;
    }
    return evaluate("rdm_evaluate_faulty", t, cfg, nz, of, returns, final_dist, records);
}

int rdm_envs_reset(rdm_trainer* t) {
    if (!t) return rd::set_error(RD_EINVAL, "rdm_envs_reset: null trainer");
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "rdm_envs_reset: no envs attached (rdm_envs_attach)");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_envs_reset");
    hipLaunchKernelGGL(student_mlp_envs_reset_kernel, dim3((unsigned)((t->envs.n + 255) / 256)), dim3(256), 0, t->stream,
                       envs_args(t));
    RD_HIP(hipGetLastError(), "student_mlp_envs_reset_kernel launch");
    return RD_OK;
}

int rdm_envs_attach(rdm_trainer* t, const rdm_envs_config* cfg) {
    if (int rc = rd::envs_attach_check("rdm_envs_attach", t, cfg)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_envs_attach");
    if (t->envs.state) {   // replace: launches that still read the old envs finish first
        RD_HIP(hipStreamSynchronize(t->stream), "rdm_envs_attach");
        t->envs.release();
    }
    const hipError_t e = rd::envs_alloc(t->envs, *cfg, rd::kStateDim, ENV_AUX);
    if (e != hipSuccess) {
        t->envs.release();
        return rd::hip_fail(e, "rdm_envs_attach: allocation");
    }
    return rdm_envs_reset(t);
}

int rdm_envs_act(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat, float* reward) {
    if (int rc = envs_check("rdm_envs_act", t, act_with, steps, x, t_pdflat)) return rc;
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_envs_act");
    return launch_envs(t, act_with, steps, x, t_pdflat, s_pdflat, reward);
}

int rdm_rollout_envs(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat,
                     float* reward) {
    return envs_train("rdm_rollout_envs", t, act_with, steps, x, t_pdflat, s_pdflat, reward, 0);
}

int rdm_step_envs(rdm_trainer* t, int act_with, int steps, float* x, float* t_pdflat, float* s_pdflat, float* reward) {
    return envs_train("rdm_step_envs", t, act_with, steps, x, t_pdflat, s_pdflat, reward, 1);
}

// how the envs calls act: the checks and the settings are rd_acting.h's
int rdm_envs_set_teacher_share(rdm_trainer* t, float beta, uint64_t coin_seed) {
    return rd::set_teacher_share("rdm_envs_set_teacher_share", rd::acting_of(t), beta, coin_seed);
}

float rdm_envs_teacher_share(const rdm_trainer* t) { return rd::teacher_share(rd::acting_of(t)); }

int rdm_envs_bind_stepped_with(rdm_trainer* t, float* buf, int64_t rows) {
    return rd::bind_stepped_with("rdm_envs_bind_stepped_with", rd::acting_of(t), buf, rows);
}

int rdm_envs_set_action_noise(rdm_trainer* t, const rd_action_noise* nz) {
    return rd::set_action_noise("rdm_envs_set_action_noise", rd::acting_of(t), nz);
}

int rdm_envs_action_noise(const rdm_trainer* t, rd_action_noise* out) {
    return rd::get_action_noise("rdm_envs_action_noise", rd::acting_of(t), out);
}

int rdm_envs_bind_actions(rdm_trainer* t, float* buf, int64_t rows) {
    return rd::bind_actions("rdm_envs_bind_actions", rd::acting_of(t), buf, rows);
}

int rdm_envs_set_obs_faults(rdm_trainer* t, const rd_obs_faults* of) {
    return rd::set_obs_faults("rdm_envs_set_obs_faults", rd::acting_of(t), of);
}

int rdm_envs_obs_faults(const rdm_trainer* t, rd_obs_faults* out) {
    return rd::get_obs_faults("rdm_envs_obs_faults", rd::acting_of(t), out);
}

int rdm_envs_get_state(rdm_trainer* t, float* state, int32_t* step, int32_t* episode) {
    if (!t || !state) return rd::set_error(RD_EINVAL, "rdm_envs_get_state: null trainer or state");
    if (!t->envs.state) return rd::set_error(RD_EINVAL, "rdm_envs_get_state: no envs attached (rdm_envs_attach)");
    rd::DeviceGuard dg(t->device);
    RD_HIP(dg.err, "rdm_envs_get_state");
    return rd::envs_get_state("rdm_envs_get_state", t->envs, rd::kStateDim, t->stream, state, step, episode);
}

}  // extern "C"
