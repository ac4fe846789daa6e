// uv_dose.h -- the lamp model and the dose bookkeeping around TSDFGrid::AccumulateDose (DESIGN.md "UV
// dose"): a tube lamp as point emitters, and the dose of a re-extracted mesh carried over by vertex key;
// for the lamp-stop planner (DESIGN.md "Lamp-stop planning"; TSDFGrid::Irradiance / PlanStops) a batch of
// candidate tubes, the missing dose, the vertex areas and the stand-off positions of a distance field.
// Host code only (no engine call); tsdf_amd/uv.py and tsdf_amd/esdf.py are the same in numpy.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <vector>

#include "disinfect_tsdf.h"
#include "tsdf_types.h"

namespace disinfect {

using UVEmitter = tsdf_uv_emitter;

// A tube lamp from p0 to p1 [m] that radiated power_w for dwell_s seconds, as `segments` point
// emitters at the midpoints of its equal segments, each with power_w * dwell_s / segments joules.
inline std::vector<UVEmitter> tube_emitters(const double p0[3], const double p1[3], float power_w, float dwell_s,
                                            int segments) {
  if (segments < 1) throw std::invalid_argument("tube_emitters: segments >= 1");
  std::vector<UVEmitter> out((size_t)segments);
  const double e = (double)power_w * (double)dwell_s / (double)segments;
  for (int i = 0; i < segments; ++i) {
    const double t = ((double)i + 0.5) / (double)segments;
    out[(size_t)i] = UVEmitter{(float)(p0[0] + t * (p1[0] - p0[0])), (float)(p0[1] + t * (p1[1] - p0[1])),
                               (float)(p0[2] + t * (p1[2] - p0[2])), (float)e};
  }
  return out;
}
inline std::vector<UVEmitter> tube_emitters(const float p0[3], const float p1[3], float power_w, float dwell_s,
                                            int segments) {
  const double a[3] = {p0[0], p0[1], p0[2]}, b[3] = {p1[0], p1[1], p1[2]};
  return tube_emitters(a, b, power_w, dwell_s, segments);
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

// ---- the lamp-stop planner's inputs ----
// Candidate lamp placements as tsdf_uv_irradiance takes them: candidate c's emitters are
// emitters[first[c] .. first[c + 1] - 1]; first holds one offset more than there are candidates.
struct LampCandidates {
  std::vector<UVEmitter> emitters;
  std::vector<int32_t> first{0};
  int32_t size() const { return (int32_t)first.size() - 1; }
};

// One tube lamp per centre (3 floats each) [m], all along `axis` (any length, not zero) and `length` metres
// long: tube_emitters(centre - h, centre + h, ...) with h = axis / |axis| * length / 2, in double.
inline LampCandidates tube_candidates(const std::vector<float>& centres, const float axis[3], float length,
                                      float power_w, float dwell_s, int segments) {
  if (centres.size() % 3) throw std::invalid_argument("tube_candidates: 3 floats per centre");
  if (segments < 1) throw std::invalid_argument("tube_candidates: segments >= 1");
  const double a[3] = {axis[0], axis[1], axis[2]};
  const double norm = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  if (!(norm > 0.0)) throw std::invalid_argument("tube_candidates: axis is zero");
  const double half = (double)length / 2;
  double h[3];
  for (int k = 0; k < 3; ++k) h[k] = a[k] / norm * half;
  LampCandidates out;
  for (size_t c = 0; c < centres.size() / 3; ++c) {
    double p0[3], p1[3];
    for (int k = 0; k < 3; ++k) p0[k] = (double)centres[3 * c + k] - h[k], p1[k] = (double)centres[3 * c + k] + h[k];
    const std::vector<UVEmitter> e = tube_emitters(p0, p1, power_w, dwell_s, segments);
    out.emitters.insert(out.emitters.end(), e.begin(), e.end());
    out.first.push_back((int32_t)out.emitters.size());
  }
  return out;
}

// What each vertex still lacks, as PlanStops takes it: max(target - dose, 0) in float where prob >=
// prob_min (the high-touch surface), 0 elsewhere.
inline std::vector<float> plan_need(const std::vector<float>& dose, const std::vector<float>& prob, float target,
                                    float prob_min = 0.5f) {
  if (dose.size() != prob.size()) throw std::invalid_argument("plan_need: one probability per dose");
  std::vector<float> out(dose.size(), 0.0f);
  for (size_t i = 0; i < out.size(); ++i) {
    const float miss = target - dose[i];
    if (prob[i] >= prob_min && miss > 0.0f) out[i] = miss;
  }
  return out;
}

// A third of the area [m^2] of the triangles around each vertex of an indexed mesh (3 floats per vertex,
// 3 indices per triangle), summed in double: first every triangle's first corner in triangle order, then
// the second corners, then the third. Meant for weight = area * prob.
inline std::vector<float> vertex_area(const std::vector<float>& verts, const std::vector<int32_t>& tris) {
  if (verts.size() % 3 || tris.size() % 3) throw std::invalid_argument("vertex_area: 3 values per vertex / triangle");
  const size_t nv = verts.size() / 3, nt = tris.size() / 3;
  std::vector<double> third(nt), acc(nv, 0.0);
  for (size_t t = 0; t < nt; ++t) {
    double p[3][3];
    for (int k = 0; k < 3; ++k) {
      const int32_t v = tris[3 * t + k];
      if (v < 0 || (size_t)v >= nv) throw std::invalid_argument("vertex_area: vertex index out of range");
      for (int a = 0; a < 3; ++a) p[k][a] = verts[3 * (size_t)v + a];
    }
    double e1[3], e2[3];
    for (int a = 0; a < 3; ++a) e1[a] = p[1][a] - p[0][a], e2[a] = p[2][a] - p[0][a];
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2],
                 cz = e1[0] * e2[1] - e1[1] * e2[0];
    third[t] = std::sqrt((cx * cx + cy * cy) + cz * cz) / 6.0;
  }
  for (int k = 0; k < 3; ++k)
    for (size_t t = 0; t < nt; ++t) acc[(size_t)tris[3 * t + k]] += third[t];
  std::vector<float> out(nv);
  for (size_t i = 0; i < nv; ++i) out[i] = (float)acc[i];
  return out;
}

// Where a lamp may stand: the world positions [m], 3 floats each, of the free voxels (state 1) of a distance
// field (d2 and state nz * ny * nx, x fastest; tsdf_types.h DistanceField) whose clearance sqrtf(d2) * voxel
// lies in [lo, hi] and that lie on the lattice origin + stride * k of the box, in box order. Voxel v sits at
// v * voxel. A field built with unknown sites keeps the candidates clear of unobserved space as well.
inline std::vector<float> standoff_candidates(const std::vector<uint16_t>& d2, const std::vector<uint8_t>& state,
                                              const int32_t origin[3], const int32_t dims[3], float voxel, float lo,
                                              float hi, int stride) {
  if (stride < 1) throw std::invalid_argument("standoff_candidates: stride >= 1");
  if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0) throw std::invalid_argument("standoff_candidates: dims");
  const size_t nvox = (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2];
  if (d2.size() != nvox || state.size() != nvox)
    throw std::invalid_argument("standoff_candidates: d2 and state hold one value per voxel of the box");
  std::vector<float> out;
  for (int z = 0; z < dims[2]; z += stride)
    for (int y = 0; y < dims[1]; y += stride)
      for (int x = 0; x < dims[0]; x += stride) {
        const size_t i = ((size_t)z * dims[1] + y) * dims[0] + x;
        const float d = std::sqrt((float)d2[i]) * voxel;
        if (state[i] != 1 || !(d >= lo && d <= hi)) continue;
        const int64_t v[3] = {(int64_t)origin[0] + x, (int64_t)origin[1] + y, (int64_t)origin[2] + z};
        for (int a = 0; a < 3; ++a) out.push_back((float)v[a] * voxel);
      }
  return out;
}

// ---- travel field (tsdf_types.h TravelField; tsdf_amd.esdf's helpers of the same names) ----
// The library's nearest voxel of a world coordinate: round(p / voxel - sample_offset) in float, half away
// from zero; 0 for a NaN.
inline int32_t nearest_voxel(float p, float voxel, float sample_offset = 0.0f) {
  const float f = p / voxel - sample_offset;
  if (!(f == f) || std::fabs(f) < 0.5f) return 0;
  const float r = std::trunc(f + std::copysign(0.5f, f));
  return (int32_t)std::min(std::max((double)r, -2147483648.0), 2147483647.0);
}

// cost / 3 * voxel [m] for every voxel of a travel field: the travel distance from the nearest seed,
// infinity where unreached.
inline std::vector<float> travel_metres(const std::vector<uint32_t>& cost, float voxel) {
  std::vector<float> out(cost.size());
  for (size_t i = 0; i < cost.size(); ++i)
    out[i] = cost[i] == TSDF_TRAVEL_UNREACHED ? INFINITY : ((float)cost[i] / 3.0f) * voxel;
  return out;
}

// The positions (3 floats each, e.g. standoff_candidates' output) whose nearest voxel a travel field (cost
// nz * ny * nx, x fastest, over the box origin / dims) reached, within max_travel metres, in their order;
// travel, when given, receives each kept position's travel distance [m]. A position outside the box is
// unreachable.
inline std::vector<float> reachable_candidates(const std::vector<float>& positions, const std::vector<uint32_t>& cost,
                                               const int32_t origin[3], const int32_t dims[3], float voxel,
                                               float max_travel = INFINITY, float sample_offset = 0.0f,
                                               std::vector<float>* travel = nullptr) {
  if (positions.size() % 3) throw std::invalid_argument("reachable_candidates: 3 floats per position");
  if (dims[0] < 0 || dims[1] < 0 || dims[2] < 0 ||
      cost.size() != (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2])
    throw std::invalid_argument("reachable_candidates: one cost per voxel of the box");
  std::vector<float> out;
  if (travel) travel->clear();
  for (size_t i = 0; i + 2 < positions.size(); i += 3) {
    int64_t v[3];
    bool in = true;
    for (int a = 0; a < 3; ++a) {
      v[a] = (int64_t)nearest_voxel(positions[i + a], voxel, sample_offset) - origin[a];
      in = in && v[a] >= 0 && v[a] < dims[a];
    }
    if (!in) continue;
    const uint32_t c = cost[((size_t)v[2] * dims[1] + (size_t)v[1]) * dims[0] + (size_t)v[0]];
    if (c == TSDF_TRAVEL_UNREACHED) continue;
    const float m = ((float)c / 3.0f) * voxel;
    if (!(m <= max_travel)) continue;
    out.insert(out.end(), positions.begin() + i, positions.begin() + i + 3);
    if (travel) travel->push_back(m);
  }
  return out;
}

// ---- frontiers (tsdf_types.h FrontierSet; tsdf_amd.esdf.frontier_goals) ----
// World positions of a frontier set's clusters, voxel v at v * voxel: per cluster seven floats -- the goal
// (its cheapest voxel to travel to), the centroid (float(sum / size + origin) * voxel, the quotient in double)
// and goal_key / 3 * voxel [m], the travel distance to the goal (0 without a travel field, infinity for a key
// of TSDF_TRAVEL_UNREACHED).
// (Cluster: tsdf_component or the facade's FrontierCluster.)
template <typename Cluster>
std::vector<float> frontier_goals(const std::vector<Cluster>& clusters, const int32_t origin[3], const int32_t dims[3],
                                  float voxel) {
  if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1) throw std::invalid_argument("frontier_goals: dims are positive");
  std::vector<float> out;
  out.reserve(7 * clusters.size());
  for (const Cluster& c : clusters) {
    const int64_t g = c.goal, nx = dims[0], ny = dims[1];
    const int64_t v[3] = {g % nx + origin[0], g / nx % ny + origin[1], g / (nx * ny) + origin[2]};
    for (int a = 0; a < 3; ++a) out.push_back((float)v[a] * voxel);
    const double size = (double)(c.size > 0 ? c.size : 1u);
    for (int a = 0; a < 3; ++a) out.push_back((float)((double)c.sum[a] / size + (double)origin[a]) * voxel);
    out.push_back(c.goal_key == TSDF_TRAVEL_UNREACHED ? INFINITY : ((float)c.goal_key / 3.0f) * voxel);
  }
  return out;
}

// ---- view gain (tsdf_types.h ViewGainResult / NextViews; tsdf_amd.esdf.look_at / view_candidates) ----
// cam_T_world of a camera at `eye` looking at `target`: z forward, x right, y down, x horizontal with respect to
// `up`. An `up` (anti)parallel to the viewing direction is replaced by the world x axis, or the y axis when the
// camera looks along x. Double throughout, one operation at a time in the order of esdf.look_at, then rounded
// to float: the two agree bit for bit.
inline SE3<float> look_at_pose(const double eye[3], const double target[3], const double up_in[3] = nullptr) {
  const double up0[3] = {0.0, 0.0, 1.0};
  const double* up = up_in ? up_in : up0;
  double f[3] = {target[0] - eye[0], target[1] - eye[1], target[2] - eye[2]};
  double n = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  if (!(n > 0.0 && std::isfinite(n))) throw std::invalid_argument("look_at_pose: eye and target coincide (or are not finite)");
  for (int a = 0; a < 3; ++a) f[a] = f[a] / n;
  auto cross = [](const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  double r[3], d[3];
  cross(f, up, r);
  n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (!(n > 1e-9)) {
    const double ex[3] = {1.0, 0.0, 0.0}, ey[3] = {0.0, 1.0, 0.0};
    cross(f, std::fabs(f[0]) < 0.9 ? ex : ey, r);
    n = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  }
  for (int a = 0; a < 3; ++a) r[a] = r[a] / n;
  cross(f, r, d);
  // cam_R_world: rows right, down, forward; its quaternion by the largest of w, x, y, z (Shepperd)
  const double* m[3] = {r, d, f};
  const double tr = m[0][0] + m[1][1] + m[2][2];
  double q[4], s;
  if (tr > 0.0) {
    s = std::sqrt(tr + 1.0) * 2.0;
    q[0] = (m[2][1] - m[1][2]) / s, q[1] = (m[0][2] - m[2][0]) / s, q[2] = (m[1][0] - m[0][1]) / s, q[3] = 0.25 * s;
  } else if (m[0][0] > m[1][1] && m[0][0] > m[2][2]) {
    s = std::sqrt(1.0 + m[0][0] - m[1][1] - m[2][2]) * 2.0;
    q[0] = 0.25 * s, q[1] = (m[0][1] + m[1][0]) / s, q[2] = (m[0][2] + m[2][0]) / s, q[3] = (m[2][1] - m[1][2]) / s;
  } else if (m[1][1] > m[2][2]) {
    s = std::sqrt(1.0 + m[1][1] - m[0][0] - m[2][2]) * 2.0;
    q[0] = (m[0][1] + m[1][0]) / s, q[1] = 0.25 * s, q[2] = (m[1][2] + m[2][1]) / s, q[3] = (m[0][2] - m[2][0]) / s;
  } else {
    s = std::sqrt(1.0 + m[2][2] - m[0][0] - m[1][1]) * 2.0;
    q[0] = (m[0][2] + m[2][0]) / s, q[1] = (m[1][2] + m[2][1]) / s, q[2] = 0.25 * s, q[3] = (m[1][0] - m[0][1]) / s;
  }
  if (q[3] < 0.0)
    for (int a = 0; a < 4; ++a) q[a] = -q[a];
  double t[3];
  for (int a = 0; a < 3; ++a) t[a] = -(m[a][0] * eye[0] + m[a][1] * eye[1] + m[a][2] * eye[2]);
  return SE3<float>((float)q[0], (float)q[1], (float)q[2], (float)q[3], (float)t[0], (float)t[1], (float)t[2]);
}

// Candidate camera poses for a frontier set: at every cluster's goal (frontier_goals), `yaws` poses turned about
// the world z axis, yaw 2 pi k / yaws from the world x axis, looking `pitch` radians above the horizon;
// cluster-major. owner (may be null) receives the index of the cluster each pose belongs to.
template <typename Cluster>
std::vector<SE3<float>> view_candidates(const std::vector<Cluster>& clusters, const int32_t origin[3],
                                        const int32_t dims[3], float voxel, int yaws = 8, float pitch = 0.0f,
                                        std::vector<int32_t>* owner = nullptr) {
  if (yaws < 1) throw std::invalid_argument("view_candidates: yaws >= 1");
  const std::vector<float> goals = frontier_goals(clusters, origin, dims, voxel);
  std::vector<SE3<float>> out;
  out.reserve(clusters.size() * (size_t)yaws);
  if (owner) owner->clear();
  const double pi = 3.141592653589793;
  for (size_t c = 0; c < clusters.size(); ++c) {
    const double e[3] = {(double)goals[7 * c], (double)goals[7 * c + 1], (double)goals[7 * c + 2]};
    for (int k = 0; k < yaws; ++k) {
      const double a = 2.0 * pi * (double)k / (double)yaws;
      const double dirn[3] = {std::cos(a) * std::cos((double)pitch), std::sin(a) * std::cos((double)pitch),
                              std::sin((double)pitch)};
      const double t[3] = {e[0] + dirn[0], e[1] + dirn[1], e[2] + dirn[2]};
      out.push_back(look_at_pose(e, t));
      if (owner) owner->push_back((int32_t)c);
    }
  }
  return out;
}

}  // namespace disinfect
