// The LSTM student's closed-loop device code -- the evaluation and envs kernels and the headers they
// stand on -- for every translation unit that compiles instances of them: student_lstm.hip and the closed
// loop's tier units (student_lstm_acting.h).  One ordered include block, so that every unit sees the
// same headers in the same order and a new closed-loop header is added here alone.  A unit's object
// carries the instances it names and these headers' non-template kernels; the training path's kernels
// that the closed loop never needs (student_lstm_persist.h, student_lstm_optim.h) are student_lstm.hip's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/reacher_student_lstm.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_gemm.h"
#include "rd_physics.h"
#include "student_lstm_acting.h"

namespace {

// dimensions, strides, flat parameter offsets, sigm
#include "student_lstm_layout.h"
// the per-step forward: inputs_kernel, cell_fwd_kernel, lstm_rec_fwd_kernel
#include "student_lstm_step.h"
// the fused head: head_layer, pack_heads_kernel, head_fwd_kernel, head_bwd_kernel, grad_finish_kernel, the reduces
#include "student_lstm_head.h"

// one closed-loop step of a 16-env block, shared by the two below: tch::, the EV_* tiling,
// lstm_eval_pack_kernel, the block's LDS and the ls_* pieces
#include "student_lstm_query.h"
// the bf16 mixed-precision cell (rdl_create_dtype's RDL_DTYPE_BF16): the Wl images and the three MFMA kernels
#include "student_lstm_bf16.h"
// the step's window positions on the bf16 cell (rdl_set_query_dtype): ls_positions_bf16, ls_positions_of
#include "student_lstm_query_bf16.h"
// the whole-episode evaluation (rdl_evaluate): LsEvalArgs, EvalActs, student_lstm_evaluate_kernel
#include "student_lstm_eval.h"
// the persistent envs (rdl_envs_*, rdl_rollout_envs, rdl_step_envs): LsEnvsArgs, EnvsActs, student_lstm_envs_kernel
#include "student_lstm_envs.h"

}  // namespace
