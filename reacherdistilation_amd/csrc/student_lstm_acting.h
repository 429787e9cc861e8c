// The launches of the LSTM student's closed-loop instances that live outside student_lstm.hip, one
// function per tier (rd::Tier, rd_acting.h) and kernel family: student_lstm_envs_kernel's and
// student_lstm_evaluate_kernel's noisy instances in student_lstm_noise.hip, their faulty ones in
// student_lstm_faults.hip.  A translation unit per tier for student_mlp_acting.h's reason: the existing
// instances' instruction text is kept as it was (profiles/envs_action_noise_isa.txt,
// envs_obs_faults_isa.txt).  The envs kernel's mixed instances stay in student_lstm.hip, where they
// were first compiled.
#pragma once
#include <hip/hip_runtime.h>

#include "rd_acting.h"

namespace rd {

struct LstmEnvsLaunch {
    const void* args;        // the call's LsEnvsArgs (student_lstm_envs.h), filled as for the plain instance
    const Acting* act;       // the handle's settings: what the tier's argument struct adds
    bool student;            // RDL_ACT_STUDENT (the noisy tier alone has a teacher instance)
    bool bf16q;              // the query on the bf16 cell (rdl_set_query_dtype)
    unsigned grid, threads;
    hipStream_t stream;
};

struct LstmEvalLaunch {
    const void* args;        // the call's LsEvalArgs (student_lstm_eval.h)
    const Acting* act;       // the call's noise (RD_NOISE_NONE: the mean acts) and faults
    bool bf16q;
    unsigned grid, threads;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_lstm_envs_noisy(const LstmEnvsLaunch& l);
hipError_t launch_lstm_envs_faulty(const LstmEnvsLaunch& l);
hipError_t launch_lstm_eval_noisy(const LstmEvalLaunch& l);
hipError_t launch_lstm_eval_faulty(const LstmEvalLaunch& l);

}  // namespace rd
