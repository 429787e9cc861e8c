// Host side of the sensor faults (include/reacher_obs_faults.h): the one check of an rd_obs_faults
// that every ABI function taking one runs before it reads a handle or calls the device.
#pragma once
#include "../../include/reacher_obs_faults.h"
#include "rd_common.h"

namespace rd {

// RD_EINVAL naming `fn` and the field: NULL struct; unknown mode (allow_clean = false: RD_OBS_CLEAN
// too); keep_prob NaN, <= 0 or > 1
inline int check_obs_faults(const char* fn, const rd_obs_faults* of, bool allow_clean) {
    if (!of) return set_error(RD_EINVAL, "%s: null rd_obs_faults", fn);
    if (of->mode != RD_OBS_CLEAN && of->mode != RD_OBS_DROPOUT && of->mode != RD_OBS_MISSING)
        return set_error(RD_EINVAL, "%s: unknown rd_obs_faults.mode %d", fn, (int)of->mode);
    if (!allow_clean && of->mode == RD_OBS_CLEAN)
        return set_error(RD_EINVAL, "%s: rd_obs_faults.mode = RD_OBS_CLEAN (call the plain function)", fn);
    if (!(of->keep_prob > 0.0f && of->keep_prob <= 1.0f))   // NaN too
        return set_error(RD_EINVAL, "%s: rd_obs_faults.keep_prob %g is not in (0, 1]", fn, (double)of->keep_prob);
    return RD_OK;
}

}  // namespace rd
