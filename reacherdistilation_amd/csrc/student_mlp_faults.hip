// The reference MLP student's closed loop under sensor faults (include/reacher_obs_faults.h):
// student_mlp_envs_kernel's faulty instances -- the student acting, {16, 64 envs} x {f32, bf16} -- for
// rdm_envs_set_obs_faults, and student_mlp_evaluate_kernel's four for rdm_evaluate_faulty.  The
// kernels, their step and every layer are student_mlp.hip's, from the same headers in the same order
// as student_mlp_noise.hip; only these eight instances are compiled here (student_mlp_faults.h says
// why), behind two launch functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_student_mlp.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_physics.h"
#include "student_mlp_faults.h"

namespace {

using rd::f32x4, rd::mfma, rd::ld4, rd::wave_sum, rd::tanh_fast, rd::fence_begin, rd::fence_end;

#include "student_mlp_layout.h"
#include "student_mlp_layers.h"
#include "student_mlp_query.h"
#include "student_mlp_eval.h"
#include "student_mlp_envs.h"

}  // namespace

namespace rd {

hipError_t launch_mlp_envs_faulty(const MlpEnvsFaultLaunch& l) {
    SmEnvsFaultArgs m{};
    static_cast<SmEnvsArgs&>(m) = *static_cast<const SmEnvsArgs*>(l.args);
    m.beta = l.beta;
    m.coin_seed = l.coin_seed;
    m.stepped_with = l.stepped_with;
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.actions = l.actions;
    m.obs_mode = l.faults.mode;
    m.obs_keep = l.faults.keep_prob;
    m.obs_seed = l.faults.seed;
    auto* kern = l.bf ? (l.small ? student_mlp_envs_kernel<16, true, true, true, SmEnvsFaultArgs>
                                 : student_mlp_envs_kernel<64, true, true, true, SmEnvsFaultArgs>)
                      : (l.small ? student_mlp_envs_kernel<16, true, false, true, SmEnvsFaultArgs>
                                 : student_mlp_envs_kernel<64, true, false, true, SmEnvsFaultArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_mlp_eval_faulty(const MlpEvalFaultLaunch& l) {
    SmEvalFaultArgs m{};
    static_cast<SmEvalArgs&>(m) = *static_cast<const SmEvalArgs*>(l.args);
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.obs_mode = l.faults.mode;
    m.obs_keep = l.faults.keep_prob;
    m.obs_seed = l.faults.seed;
    auto* kern = l.bf ? (l.small ? student_mlp_evaluate_kernel<16, true, SmEvalFaultArgs>
                                 : student_mlp_evaluate_kernel<64, true, SmEvalFaultArgs>)
                      : (l.small ? student_mlp_evaluate_kernel<16, false, SmEvalFaultArgs>
                                 : student_mlp_evaluate_kernel<64, false, SmEvalFaultArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
