// The LSTM student's closed loop under action noise (include/reacher_action_noise.h):
// student_lstm_envs_kernel's noisy instances -- the student acting on the f32 and on the bf16 query,
// and the teacher acting -- for rdl_envs_set_action_noise / rdl_envs_bind_actions, and
// student_lstm_evaluate_kernel's two for rdl_evaluate_noisy.  The kernels and their step are
// student_lstm.hip's; only these five instances are compiled here (student_lstm_acting.h says why).
#include "student_lstm_device.h"

namespace rd {

hipError_t launch_lstm_envs_noisy(const LstmEnvsLaunch& l) {
    const LsEnvsNoiseArgs m = acting_args<LsEnvsNoiseArgs>(*static_cast<const LsEnvsArgs*>(l.args), *l.act);
    auto* kern = !l.student ? student_lstm_envs_kernel<false, false, LsEnvsNoiseArgs>
                 : l.bf16q  ? student_lstm_envs_kernel<true, true, LsEnvsNoiseArgs>
                            : student_lstm_envs_kernel<true, false, LsEnvsNoiseArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_lstm_eval_noisy(const LstmEvalLaunch& l) {
    const LsEvalNoiseArgs m = acting_args<LsEvalNoiseArgs>(*static_cast<const LsEvalArgs*>(l.args), *l.act);
    auto* kern = l.bf16q ? student_lstm_evaluate_kernel<true, LsEvalNoiseArgs>
                         : student_lstm_evaluate_kernel<false, LsEvalNoiseArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
