// student_mlp_envs_kernel's mixed instances, {16, 64 envs} x {f32, bf16}: the persistent envs of the
// reference MLP student stepped under DAgger's beta-mixture (rdm_envs_set_teacher_share,
// include/reacher_student_mlp.h).  The kernel, its step and every layer are student_mlp.hip's; only
// these four instances are compiled here (student_mlp_acting.h says why).
#include "student_mlp_device.h"

namespace rd {

hipError_t launch_mlp_envs_mixed(const MlpEnvsLaunch& l) {
    const SmEnvsMixArgs m = acting_args<SmEnvsMixArgs>(*static_cast<const SmEnvsArgs*>(l.args), *l.act);
    auto* kern = l.bf ? (l.small ? student_mlp_envs_kernel<16, true, true, SmEnvsMixArgs>
                                 : student_mlp_envs_kernel<64, true, true, SmEnvsMixArgs>)
                      : (l.small ? student_mlp_envs_kernel<16, true, false, SmEnvsMixArgs>
                                 : student_mlp_envs_kernel<64, true, false, SmEnvsMixArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
