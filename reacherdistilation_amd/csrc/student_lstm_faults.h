// The launches of the LSTM student's faulty closed-loop instances (sensor faults on the student's
// observation, include/reacher_obs_faults.h): student_lstm_envs_kernel's for rdl_envs_set_obs_faults
// and student_lstm_evaluate_kernel's for rdl_evaluate_faulty.  They live in a translation unit of
// their own, student_lstm_faults.hip, for student_lstm_noise.h's reason: the existing instances'
// instruction text is kept as it was (profiles/envs_obs_faults_isa.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_action_noise.h"
#include "../../include/reacher_obs_faults.h"

namespace rd {

// a student call's (RDL_ACT_STUDENT): the instance carries the coin and the noise too, either of
// which may be off (beta = 0 never fires; RD_NOISE_NONE steps with the mean)
struct LstmEnvsFaultLaunch {
    const void* args;        // the call's LsEnvsArgs (student_lstm_envs.h), filled as for the plain instance
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    rd_action_noise noise;
    float* actions;          // [K][n][2] or null
    rd_obs_faults faults;    // RD_OBS_DROPOUT or RD_OBS_MISSING
    bool bf16q;              // the query on the bf16 cell (rdl_set_query_dtype)
    unsigned grid;
    hipStream_t stream;
};

struct LstmEvalFaultLaunch {
    const void* args;        // the call's LsEvalArgs (student_lstm_eval.h)
    rd_action_noise noise;   // RD_NOISE_NONE: the mean acts
    rd_obs_faults faults;
    bool bf16q;
    unsigned grid;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_lstm_envs_faulty(const LstmEnvsFaultLaunch& l);
hipError_t launch_lstm_eval_faulty(const LstmEvalFaultLaunch& l);

}  // namespace rd
