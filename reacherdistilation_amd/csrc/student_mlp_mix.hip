// student_mlp_envs_kernel's mixed instances, {16, 64 envs} x {f32, bf16}: the persistent envs of the
// reference MLP student stepped under DAgger's beta-mixture (rdm_envs_set_teacher_share,
// include/reacher_student_mlp.h).  The kernel, its step and every layer are student_mlp.hip's, from the
// same headers in the same order; only these four instances are compiled here (student_mlp_mix.h says
// why), behind one launch function.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_student_mlp.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_physics.h"
#include "student_mlp_mix.h"

namespace {

using rd::f32x4, rd::mfma, rd::ld4, rd::wave_sum, rd::tanh_fast, rd::fence_begin, rd::fence_end;

#include "student_mlp_layout.h"
#include "student_mlp_layers.h"
#include "student_mlp_query.h"
#include "student_mlp_envs.h"

}  // namespace

namespace rd {

hipError_t launch_mlp_envs_mixed(const MlpEnvsMixLaunch& l) {
    SmEnvsMixArgs m{};
    static_cast<SmEnvsArgs&>(m) = *static_cast<const SmEnvsArgs*>(l.args);
    m.beta = l.beta;
    m.coin_seed = l.coin_seed;
    m.stepped_with = l.stepped_with;
    auto* kern = l.bf ? (l.small ? student_mlp_envs_kernel<16, true, true, true, SmEnvsMixArgs>
                                 : student_mlp_envs_kernel<64, true, true, true, SmEnvsMixArgs>)
                      : (l.small ? student_mlp_envs_kernel<16, true, false, true, SmEnvsMixArgs>
                                 : student_mlp_envs_kernel<64, true, false, true, SmEnvsMixArgs>);
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
