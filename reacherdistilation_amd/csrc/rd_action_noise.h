// Host side of the action noise (include/reacher_action_noise.h): the one check of an rd_action_noise
// that every ABI function taking one runs before it reads a handle or calls the device.
#pragma once
#include <math.h>

#include "../../include/reacher_action_noise.h"
#include "rd_common.h"

namespace rd {

// RD_EINVAL naming `fn` and the field: NULL struct; unknown mode (allow_none = false: RD_NOISE_NONE
// too); scale NaN, negative or infinite
inline int check_action_noise(const char* fn, const rd_action_noise* nz, bool allow_none) {
    if (!nz) return set_error(RD_EINVAL, "%s: null rd_action_noise", fn);
    if (nz->mode != RD_NOISE_NONE && nz->mode != RD_NOISE_POLICY && nz->mode != RD_NOISE_FIXED)
        return set_error(RD_EINVAL, "%s: unknown rd_action_noise.mode %d", fn, (int)nz->mode);
    if (!allow_none && nz->mode == RD_NOISE_NONE)
        return set_error(RD_EINVAL, "%s: rd_action_noise.mode = RD_NOISE_NONE (call the plain function)", fn);
    if (!(nz->scale >= 0.0f) || isinf(nz->scale))   // NaN too
        return set_error(RD_EINVAL, "%s: rd_action_noise.scale %g is not a finite value >= 0", fn, (double)nz->scale);
    return RD_OK;
}

}  // namespace rd
