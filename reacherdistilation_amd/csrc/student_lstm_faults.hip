// The LSTM student's closed loop under sensor faults (include/reacher_obs_faults.h):
// student_lstm_envs_kernel's faulty instances -- the student acting on the f32 and on the bf16 query --
// for rdl_envs_set_obs_faults, and student_lstm_evaluate_kernel's two for rdl_evaluate_faulty.  The
// kernels and their step are student_lstm.hip's; only these four instances are compiled here
// (student_lstm_acting.h says why).
#include "student_lstm_device.h"

namespace rd {

hipError_t launch_lstm_envs_faulty(const LstmEnvsLaunch& l) {
    const LsEnvsFaultArgs m = acting_args<LsEnvsFaultArgs>(*static_cast<const LsEnvsArgs*>(l.args), *l.act);
    auto* kern = l.bf16q ? student_lstm_envs_kernel<true, true, LsEnvsFaultArgs>
                         : student_lstm_envs_kernel<true, false, LsEnvsFaultArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_lstm_eval_faulty(const LstmEvalLaunch& l) {
    const LsEvalFaultArgs m = acting_args<LsEvalFaultArgs>(*static_cast<const LsEvalArgs*>(l.args), *l.act);
    auto* kern = l.bf16q ? student_lstm_evaluate_kernel<true, LsEvalFaultArgs>
                         : student_lstm_evaluate_kernel<false, LsEvalFaultArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(l.threads), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
