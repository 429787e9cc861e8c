// The LSTM student's closed loop under action noise (include/reacher_action_noise.h):
// student_lstm_envs_kernel's noisy instances -- the student acting on the f32 and on the bf16 query,
// and the teacher acting -- for rdl_envs_set_action_noise / rdl_envs_bind_actions, and
// student_lstm_evaluate_kernel's two for rdl_evaluate_noisy.  The kernels and their step are
// student_lstm.hip's, from the same headers in the same order; only these five instances are compiled
// here (student_lstm_noise.h says why), behind two launch functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_student_lstm.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_gemm.h"
#include "rd_physics.h"
#include "student_lstm_noise.h"

namespace {

#include "student_lstm_layout.h"
#include "student_lstm_step.h"   // LSTM_KH: the query's K split
#include "student_lstm_head.h"   // head_layer
#include "student_lstm_query.h"
#include "student_lstm_bf16.h"
#include "student_lstm_query_bf16.h"
#include "student_lstm_eval.h"
#include "student_lstm_envs.h"

}  // namespace

namespace rd {

hipError_t launch_lstm_envs_noisy(const LstmEnvsNoiseLaunch& l) {
    LsEnvsNoiseArgs m{};
    static_cast<LsEnvsArgs&>(m) = *static_cast<const LsEnvsArgs*>(l.args);
    m.beta = l.beta;
    m.coin_seed = l.coin_seed;
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.actions = l.actions;
    auto* kern = !l.student ? student_lstm_envs_kernel<false, false, false, LsEnvsNoiseArgs>
                 : l.bf16q  ? student_lstm_envs_kernel<true, true, true, LsEnvsNoiseArgs>
                            : student_lstm_envs_kernel<true, false, true, LsEnvsNoiseArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(EV_THREADS), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_lstm_eval_noisy(const LstmEvalNoiseLaunch& l) {
    LsEvalNoiseArgs m{};
    static_cast<LsEvalArgs&>(m) = *static_cast<const LsEvalArgs*>(l.args);
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    auto* kern = l.bf16q ? student_lstm_evaluate_kernel<true, LsEvalNoiseArgs>
                         : student_lstm_evaluate_kernel<false, LsEvalNoiseArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(EV_THREADS), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
