// The launches of the LSTM student's noisy closed-loop instances (action noise,
// include/reacher_action_noise.h): student_lstm_envs_kernel's for rdl_envs_set_action_noise /
// rdl_envs_bind_actions and student_lstm_evaluate_kernel's for rdl_evaluate_noisy.  They live in a
// translation unit of their own, student_lstm_noise.hip, for student_mlp_mix.h's reason: the existing
// instances' instruction text is kept as it was (profiles/envs_action_noise_isa.txt).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/reacher_action_noise.h"

namespace rd {

struct LstmEnvsNoiseLaunch {
    const void* args;        // the call's LsEnvsArgs (student_lstm_envs.h), filled as for the plain instance
    bool student;            // RDL_ACT_STUDENT: the instance carries the coin (beta = 0 never fires)
    float beta;              // the teacher's share of the env steps
    uint64_t coin_seed;      // the coins' Philox key
    rd_action_noise noise;
    float* actions;          // [K][n][2] or null
    bool bf16q;              // the query on the bf16 cell (rdl_set_query_dtype)
    unsigned grid;
    hipStream_t stream;
};

struct LstmEvalNoiseLaunch {
    const void* args;        // the call's LsEvalArgs (student_lstm_eval.h)
    rd_action_noise noise;
    bool bf16q;
    unsigned grid;
    hipStream_t stream;
};

// the launch's hipGetLastError
hipError_t launch_lstm_envs_noisy(const LstmEnvsNoiseLaunch& l);
hipError_t launch_lstm_eval_noisy(const LstmEvalNoiseLaunch& l);

}  // namespace rd
