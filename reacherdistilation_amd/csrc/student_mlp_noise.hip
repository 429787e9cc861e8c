// The reference MLP student's closed loop under action noise (include/reacher_action_noise.h):
// student_mlp_envs_kernel's noisy instances -- the student acting, {16, 64 envs} x {f32, bf16}, and the
// teacher acting, {16, 64 envs} -- for rdm_envs_set_action_noise / rdm_envs_bind_actions, and
// student_mlp_evaluate_kernel's four for rdm_evaluate_noisy.  The kernels, their step and every layer
// are student_mlp.hip's; only these ten instances are compiled here (student_mlp_acting.h says why).
#include "student_mlp_device.h"

namespace rd {

hipError_t launch_mlp_envs_noisy(const MlpEnvsLaunch& l) {
    const SmEnvsNoiseArgs m = acting_args<SmEnvsNoiseArgs>(*static_cast<const SmEnvsArgs*>(l.args), *l.act);
    // the teacher-acts instances run no student layer: one arithmetic
    auto* kern = !l.student ? (l.small ? student_mlp_envs_kernel<16, false, false, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, false, false, SmEnvsNoiseArgs>)
                 : l.bf     ? (l.small ? student_mlp_envs_kernel<16, true, true, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, true, true, SmEnvsNoiseArgs>)
                            : (l.small ? student_mlp_envs_kernel<16, true, false, SmEnvsNoiseArgs>
                                       : student_mlp_envs_kernel<64, true, false, SmEnvsNoiseArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_mlp_eval_noisy(const MlpEvalLaunch& l) {
    const SmEvalNoiseArgs m = acting_args<SmEvalNoiseArgs>(*static_cast<const SmEvalArgs*>(l.args), *l.act);
    auto* kern = l.bf ? (l.small ? student_mlp_evaluate_kernel<16, true, SmEvalNoiseArgs>
                                 : student_mlp_evaluate_kernel<64, true, SmEvalNoiseArgs>)
                      : (l.small ? student_mlp_evaluate_kernel<16, false, SmEvalNoiseArgs>
                                 : student_mlp_evaluate_kernel<64, false, SmEvalNoiseArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
