// The reference MLP student's closed loop under sensor faults (include/reacher_obs_faults.h):
// student_mlp_envs_kernel's faulty instances -- the student acting, {16, 64 envs} x {f32, bf16} -- for
// rdm_envs_set_obs_faults, and student_mlp_evaluate_kernel's four for rdm_evaluate_faulty.  The
// kernels, their step and every layer are student_mlp.hip's; only these eight instances are compiled
// here (student_mlp_acting.h says why).
#include "student_mlp_device.h"

namespace rd {

hipError_t launch_mlp_envs_faulty(const MlpEnvsLaunch& l) {
    const SmEnvsFaultArgs m = acting_args<SmEnvsFaultArgs>(*static_cast<const SmEnvsArgs*>(l.args), *l.act);
    auto* kern = l.bf ? (l.small ? student_mlp_envs_kernel<16, true, true, SmEnvsFaultArgs>
                                 : student_mlp_envs_kernel<64, true, true, SmEnvsFaultArgs>)
                      : (l.small ? student_mlp_envs_kernel<16, true, false, SmEnvsFaultArgs>
                                 : student_mlp_envs_kernel<64, true, false, SmEnvsFaultArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_mlp_eval_faulty(const MlpEvalLaunch& l) {
    const SmEvalFaultArgs m = acting_args<SmEvalFaultArgs>(*static_cast<const SmEvalArgs*>(l.args), *l.act);
    auto* kern = l.bf ? (l.small ? student_mlp_evaluate_kernel<16, true, SmEvalFaultArgs>
                                 : student_mlp_evaluate_kernel<64, true, SmEvalFaultArgs>)
                      : (l.small ? student_mlp_evaluate_kernel<16, false, SmEvalFaultArgs>
                                 : student_mlp_evaluate_kernel<64, false, SmEvalFaultArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
