// uv_dose.h -- the lamp model and the dose bookkeeping around TSDFGrid::AccumulateDose (DESIGN.md "UV
// dose"): a tube lamp as point emitters, and the dose of a re-extracted mesh carried over by vertex key.
// Host code only (no engine call); tsdf_amd/uv.py is the same in numpy.
#pragma once

#include <array>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <vector>

#include "disinfect_tsdf.h"

namespace disinfect {

using UVEmitter = tsdf_uv_emitter;

// A tube lamp from p0 to p1 [m] that radiated power_w for dwell_s seconds, as `segments` point
// emitters at the midpoints of its equal segments, each with power_w * dwell_s / segments joules.
inline std::vector<UVEmitter> tube_emitters(const float p0[3], const float p1[3], float power_w, float dwell_s,
                                            int segments) {
  if (segments < 1) throw std::invalid_argument("tube_emitters: segments >= 1");
  std::vector<UVEmitter> out((size_t)segments);
  const double e = (double)power_w * (double)dwell_s / (double)segments;
  for (int i = 0; i < segments; ++i) {
    const double t = ((double)i + 0.5) / (double)segments;
    out[(size_t)i] = UVEmitter{(float)((double)p0[0] + t * ((double)p1[0] - (double)p0[0])),
                               (float)((double)p0[1] + t * ((double)p1[1] - (double)p0[1])),
                               (float)((double)p0[2] + t * ((double)p1[2] - (double)p0[2])), (float)e};
  }
  return out;
}

// The dose of every vertex of a new extraction whose key (gx, gy, gz, axis: tsdf_mesh_out.keys, 4 per
// vertex) existed in the old one; 0 for the rest. old_keys holds 4 * old_dose.size() values.
inline std::vector<float> carry_dose(const std::vector<int32_t>& old_keys, const std::vector<float>& old_dose,
                                     const std::vector<int32_t>& new_keys) {
  if (old_keys.size() != 4 * old_dose.size() || new_keys.size() % 4 != 0)
    throw std::invalid_argument("carry_dose: 4 key values per vertex");
  std::map<std::array<int32_t, 4>, float> seen;
  for (size_t i = 0; i < old_dose.size(); ++i)
    seen[{old_keys[4 * i], old_keys[4 * i + 1], old_keys[4 * i + 2], old_keys[4 * i + 3]}] = old_dose[i];
  std::vector<float> out(new_keys.size() / 4, 0.0f);
  for (size_t i = 0; i < out.size(); ++i) {
    const auto it = seen.find({new_keys[4 * i], new_keys[4 * i + 1], new_keys[4 * i + 2], new_keys[4 * i + 3]});
    if (it != seen.end()) out[i] = it->second;
  }
  return out;
}

}  // namespace disinfect
