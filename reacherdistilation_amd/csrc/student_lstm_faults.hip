// The LSTM student's closed loop under sensor faults (include/reacher_obs_faults.h):
// student_lstm_envs_kernel's faulty instances -- the student acting on the f32 and on the bf16 query --
// for rdl_envs_set_obs_faults, and student_lstm_evaluate_kernel's two for rdl_evaluate_faulty.  The
// kernels and their step are student_lstm.hip's, from the same headers in the same order as
// student_lstm_noise.hip; only these four instances are compiled here (student_lstm_faults.h says
// why), behind two launch functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_student_lstm.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_gemm.h"
#include "rd_physics.h"
#include "student_lstm_faults.h"

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

hipError_t launch_lstm_envs_faulty(const LstmEnvsFaultLaunch& l) {
    LsEnvsFaultArgs m{};
    static_cast<LsEnvsArgs&>(m) = *static_cast<const LsEnvsArgs*>(l.args);
    m.beta = l.beta;
    m.coin_seed = l.coin_seed;
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.actions = l.actions;
    m.obs_mode = l.faults.mode;
    m.obs_keep = l.faults.keep_prob;
    m.obs_seed = l.faults.seed;
    auto* kern = l.bf16q ? student_lstm_envs_kernel<true, true, true, LsEnvsFaultArgs>
                         : student_lstm_envs_kernel<true, false, true, LsEnvsFaultArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(EV_THREADS), 0, l.stream, m);
    return hipGetLastError();
}

hipError_t launch_lstm_eval_faulty(const LstmEvalFaultLaunch& l) {
    LsEvalFaultArgs m{};
    static_cast<LsEvalArgs&>(m) = *static_cast<const LsEvalArgs*>(l.args);
    m.noise_mode = l.noise.mode;
    m.noise_scale = l.noise.scale;
    m.noise_seed = l.noise.seed;
    m.obs_mode = l.faults.mode;
    m.obs_keep = l.faults.keep_prob;
    m.obs_seed = l.faults.seed;
    auto* kern = l.bf16q ? student_lstm_evaluate_kernel<true, LsEvalFaultArgs>
                         : student_lstm_evaluate_kernel<false, LsEvalFaultArgs>;
    hipLaunchKernelGGL(kern, dim3(l.grid), dim3(EV_THREADS), 0, l.stream, m);
    return hipGetLastError();
}

}  // namespace rd
