// The reference MLP student's closed loop under action noise (include/reacher_action_noise.h):
// student_mlp_envs_kernel's noisy instances -- the student acting, {16, 64 envs} x {f32, bf16}, and the
// teacher acting, {16, 64 envs} -- for rdm_envs_set_action_noise / rdm_envs_bind_actions, and
// student_mlp_evaluate_kernel's four for rdm_evaluate_noisy.  The kernels, their step and every layer
// are student_mlp.hip's, from the same headers in the same order; only these ten instances are
// compiled here (student_mlp_noise.h says why), behind two launch functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_student_mlp.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_physics.h"
#include "student_mlp_noise.h"

namespace {

using rd::f32x4, rd::mfma, rd::ld4, rd::wave_sum, rd::tanh_fast, rd::fence_begin, rd::fence_end;

#include "student_mlp_layout.h"
#include "student_mlp_layers.h"
#include "student_mlp_query.h"
#include "student_mlp_eval.h"
#include "student_mlp_envs.h"

}  // namespace

namespace rd {

hipError_t launch_mlp_envs_noisy(const MlpEnvsNoiseLaunch& l) {
    SmEnvsNoiseArgs m{};
    static_cast<SmEnvsArgs&>(m) = *static_cast<const SmEnvsArgs*>(l.args);
    m.beta = l.beta;
    m.coin_seed = l.coin_seed;
    m.stepped_with = l.stepped_with;
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.actions = l.actions;
    // the teacher-acts instances run no student layer: one arithmetic
    auto* kern = !l.student ? (l.small ? student_mlp_envs_kernel<16, false, false, false, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, false, false, false, SmEnvsNoiseArgs>)
                 : l.bf     ? (l.small ? student_mlp_envs_kernel<16, true, true, true, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, true, true, true, SmEnvsNoiseArgs>)
                            : (l.small ? student_mlp_envs_kernel<16, true, false, true, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, true, false, true, SmEnvsNoiseArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_mlp_eval_noisy(const MlpEvalNoiseLaunch& l) {
    SmEvalNoiseArgs m{};
    static_cast<SmEvalArgs&>(m) = *static_cast<const SmEvalArgs*>(l.args);
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    auto* kern = l.bf ? (l.small ? student_mlp_evaluate_kernel<16, true, SmEvalNoiseArgs>
                                 : student_mlp_evaluate_kernel<64, true, SmEvalNoiseArgs>)
                      : (l.small ? student_mlp_evaluate_kernel<16, false, SmEvalNoiseArgs>
                                 : student_mlp_evaluate_kernel<64, false, SmEvalNoiseArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
