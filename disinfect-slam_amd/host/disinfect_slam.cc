// disinfect_slam.cc -- DISINFSystem's TSDF half (disinfect_slam/disinfect_slam.cc:3-116).
#include "disinfect_slam.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>

namespace disinfect {

static std::shared_ptr<TSDFSystem> make_tsdf(float voxel_size, float truncation, float max_depth,
                                             const CameraIntrinsics<float>& intrinsics,
                                             const SE3<float>& extrinsics, const tsdf_config* cfg,
                                             int device) {
  if (!cfg) return std::make_shared<TSDFSystem>(voxel_size, truncation, max_depth, intrinsics, extrinsics);
  tsdf_config c = *cfg;
  c.voxel_size = voxel_size;
  c.truncation = truncation;
  return std::make_shared<TSDFSystem>(c, device, max_depth, intrinsics, extrinsics);
}

DISINFSystem::DISINFSystem(float voxel_size, float truncation, float max_depth,
                           const CameraIntrinsics<float>& intrinsics, const SE3<float>& extrinsics,
                           float depth_factor, const tsdf_config* engine_cfg, int device)
    : TSDF_(make_tsdf(voxel_size, truncation, max_depth, intrinsics, extrinsics, engine_cfg, device)),
      camera_pose_manager_(std::make_shared<pose_manager>()),
      depthmap_factor_(depth_factor) {}

void DISINFSystem::feed_rgbd_frame(const Mat& img_rgb, const Mat& img_depth, int64_t timestamp,
                                   const Mat& mask) {
  const SE3<float> posecam_P_world = camera_pose_manager_->query_pose(timestamp);
  TSDF_->IntegrateRaw(posecam_P_world, img_rgb, img_depth, mask, depthmap_factor_);
}

TrackResult DISINFSystem::track_rgbd_frame(const Mat& img_rgb, const Mat& img_depth, int64_t timestamp,
                                           const Mat& mask) {
  if (camera_pose_manager_->size() == 0)
    throw std::logic_error("DISINFSystem::track_rgbd_frame: the first frame needs a registered pose");
  Mat rgb_half, depth_half;
  TSDF_->HalfRGBD(img_rgb, img_depth, mask, depthmap_factor_, &rgb_half, &depth_half);
  // the newest registered pose: the nearest to a time after every timestamp
  const SE3<float> guess = camera_pose_manager_->query_pose(std::numeric_limits<int64_t>::max());
  const TrackResult r = TSDF_->Track(depth_half, guess);
  camera_pose_manager_->register_valid_pose(timestamp, r.pose);
  TSDF_->Integrate(r.pose, rgb_half, depth_half);
  return r;
}

void DISINFSystem::register_camera_pose(int64_t timestamp, const SE3<float>& cam_T_world) {
  camera_pose_manager_->register_valid_pose(timestamp, cam_T_world);
}

SE3<float> DISINFSystem::query_camera_pose(int64_t timestamp) {
  return camera_pose_manager_->query_pose(timestamp);
}

std::vector<VoxelSpatialTSDF> DISINFSystem::query_tsdf(const BoundingCube<float>& volumn) {
  return TSDF_->Query(volumn);
}

TriMesh DISINFSystem::query_mesh(const BoundingCube<float>& volumn) { return TSDF_->QueryMesh(volumn); }

DistanceField DISINFSystem::query_distance_field(const BoundingCube<float>& volumn, int max_dist, int min_weight,
                                                 bool unknown) {
  return TSDF_->DistanceField(volumn, max_dist, min_weight, unknown);
}

TravelField DISINFSystem::query_travel_field(const DistanceField& field, const std::vector<float>& from_world,
                                             float clearance_m, bool unknown_free) {
  if (from_world.size() % 3) throw std::invalid_argument("DISINFSystem::query_travel_field: 3 floats per position");
  const float voxel = TSDF_->voxel_size();
  std::vector<int32_t> seeds(from_world.size());
  for (size_t i = 0; i < seeds.size(); ++i) seeds[i] = nearest_voxel(from_world[i], voxel);
  // sqrt(d2) * voxel >= clearance_m
  const double q = std::max((double)clearance_m, 0.0) / (double)voxel;
  const int clearance2 = (int)std::min(std::ceil(q * q), 65025.0);
  return TSDF_->TravelField(field, seeds, clearance2, unknown_free);
}

void DISINFSystem::enable_free_space(const BoundingCube<float>& volumn) { TSDF_->EnableFreeSpace(volumn); }

DistanceField DISINFSystem::query_free_space(const DistanceField& field, int64_t* promoted) {
  return TSDF_->ApplyFreeSpace(field, promoted);
}

FrontierSet DISINFSystem::query_frontiers(const DistanceField& field, const TravelField* travel, int min_size) {
  return TSDF_->Frontiers(field, travel, min_size);
}

NextViews DISINFSystem::query_next_views(int k, const BoundingCube<float>& volumn, const std::vector<float>& from_world,
                                         const CameraParams& cam, float far, float clearance_m, int min_size, int yaws,
                                         float pitch, int max_dist) {
  const DistanceField field = query_free_space(query_distance_field(volumn, max_dist));
  const TravelField travel = query_travel_field(field, from_world, clearance_m, false);
  const FrontierSet fs = query_frontiers(field, &travel, min_size);
  std::vector<int32_t> owner;
  const std::vector<SE3<float>> views = view_candidates(fs.clusters, fs.origin, fs.dims, TSDF_->voxel_size(), yaws, pitch, &owner);
  NextViews out = TSDF_->NextViewsOf(field, views, cam, k, far);
  out.cluster = owner;
  return out;
}

void DISINFSystem::irradiate(TriMesh& mesh, const std::vector<UVEmitter>& emitters, const tsdf_uv_config* cfg) {
  const size_t nv = mesh.verts.size() / 3;
  if (mesh.normals.empty()) mesh.normals = TSDF_->SurfaceNormals(mesh.verts, 0.5f);
  if (mesh.dose.empty()) mesh.dose.assign(nv, 0.0f);
  if (mesh.normals.size() != mesh.verts.size() || mesh.dose.size() != nv)
    throw std::invalid_argument("DISINFSystem::irradiate: normals / dose do not match the vertices");
  tsdf_uv_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_uv_config_default(TSDF_->engine(), &c);
  c.sample_offset = 0.5f;
  TSDF_->AccumulateDose(mesh.verts, mesh.normals, emitters, &mesh.dose, &c);
}

DISINFSystem::LampPlan DISINFSystem::plan_irradiation(TriMesh& mesh, const std::vector<float>& dose, float target,
                                                      const LampCandidates& candidates, int max_stops, float min_gain,
                                                      float prob_min, const tsdf_uv_config* cfg) {
  const size_t nv = mesh.verts.size() / 3;
  if (mesh.normals.empty()) mesh.normals = TSDF_->SurfaceNormals(mesh.verts, 0.5f);
  if (mesh.normals.size() != mesh.verts.size() || mesh.prob.size() != nv || (!dose.empty() && dose.size() != nv))
    throw std::invalid_argument("DISINFSystem::plan_irradiation: normals / prob / dose do not match the vertices");
  tsdf_uv_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_uv_config_default(TSDF_->engine(), &c);
  c.sample_offset = 0.5f;
  const std::vector<float> E = TSDF_->Irradiance(mesh.verts, mesh.normals, candidates.emitters, candidates.first, &c);
  LampPlan plan;
  plan.need = plan_need(dose.empty() ? std::vector<float>(nv, 0.0f) : dose, mesh.prob, target, prob_min);
  std::vector<float> weight = vertex_area(mesh.verts, mesh.tris);
  for (size_t i = 0; i < nv; ++i) weight[i] = weight[i] * mesh.prob[i];
  plan.stops = TSDF_->PlanStops(E, candidates.size(), &plan.need, weight, max_stops, min_gain, &plan.gains);
  return plan;
}

}  // namespace disinfect
