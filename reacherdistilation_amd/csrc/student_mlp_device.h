// The reference MLP student's device code, for every translation unit that compiles instances of its
// kernels: student_mlp.hip and the closed loop's tier units (student_mlp_acting.h).  One ordered include
// block, so that every unit sees the same headers in the same order and a new device header is added
// here alone.  A unit emits only the instances it names.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/reacher_student_mlp.h"
#include "rd_common.h"
#include "rd_device.h"
#include "rd_physics.h"
#include "student_mlp_acting.h"

namespace {

using rd::f32x4, rd::mfma, rd::ld4, rd::wave_sum, rd::tanh_fast, rd::fence_begin, rd::fence_end;

// dimensions, the flat / workspace / image layouts, pk, the LDS buffers of a row block, Part
#include "student_mlp_layout.h"
// the layer templates, their bf16 siblings (student_mlp_bf16.h) and the fwd / dgrad / wgrad selectors
#include "student_mlp_layers.h"
// the forward and the training step: SmArgs, student_mlp_kernel
#include "student_mlp_train.h"

// one closed-loop step of a block of envs, shared by the two below: tch::, EREC, ELay, the qs_* pieces
#include "student_mlp_query.h"
// the whole-episode evaluation (rdm_evaluate): SmEvalArgs, EvalActs, student_mlp_evaluate_kernel
#include "student_mlp_eval.h"
// the persistent envs (rdm_envs_*, rdm_step_envs): SmEnvsArgs, EnvsActs, student_mlp_envs_kernel
#include "student_mlp_envs.h"

}  // namespace
