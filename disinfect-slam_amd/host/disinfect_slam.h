// disinfect_slam.h -- DISINFSystem (disinfect_slam/disinfect_slam.h:22-60) reduced to its TSDF
// half: the pose store the SLAM tracker feeds (pose_manager), the sensor-frame entry point
// feed_rgbd_frame and query_tsdf, over TSDFSystem on the MI355X engine. The ORB-SLAM3 tracker,
// the segmentation network and the renderer are outside this engine: a tracker
// registers its poses with register_camera_pose (what feed_stereo / feed_stereo_IMU do after
// TrackStereo, disinfect_slam.cc:69-100). Without a tracker, track_rgbd_frame takes the pose of each
// frame from the volume itself (frame-to-model ICP, tsdf_track).
#pragma once

#include <memory>

#include "pose_manager.h"
#include "tsdf_module.h"
#include "uv_dose.h"

namespace disinfect {

class DISINFSystem {
 public:
  // disinfect_slam.cc:3-24 builds TSDFSystem(0.05, 0.2, 4, intrinsics, extrinsics) from the camera
  // config and reads DepthMapFactor; here the values are passed in (no YAML reader in the engine)
  DISINFSystem(float voxel_size, float truncation, float max_depth,
               const CameraIntrinsics<float>& intrinsics, const SE3<float>& extrinsics,
               float depth_factor, const tsdf_config* engine_cfg = nullptr, int device = 0);

  // disinfect_slam.cc:31-67: pose at `timestamp` [ms], x0.5 resize of rgb / depth / mask, depth
  // scale, mask -> depth 0, integrate (the resize / scale / mask run on the GPU)
  void feed_rgbd_frame(const Mat& img_rgb, const Mat& img_depth, int64_t timestamp, const Mat& mask = {});
  // feed_rgbd_frame without an outside tracker: the frame's pose comes from the volume. The x0.5
  // resize / depth scale / mask, then frame-to-model ICP of the half-size depth from the newest
  // registered pose (TSDFSystem::Track), register_camera_pose(timestamp, result), integrate. The first
  // frame needs a registered pose (throws std::logic_error without one): it fixes the world frame.
  // A degenerate result registers and integrates at the last good estimate.
  TrackResult track_rgbd_frame(const Mat& img_rgb, const Mat& img_depth, int64_t timestamp, const Mat& mask = {});
  void register_camera_pose(int64_t timestamp, const SE3<float>& cam_T_world);
  SE3<float> query_camera_pose(int64_t timestamp);                              // :108-111
  std::vector<VoxelSpatialTSDF> query_tsdf(const BoundingCube<float>& volumn);  // :113-116
  // the surface in `volumn` as an indexed mesh with colour and high-touch probability: what tsdfCb
  // builds from query_tsdf's voxels on the CPU (ros_offline.cc:286-313), extracted on the GPU
  TriMesh query_mesh(const BoundingCube<float>& volumn);
  // The UV dose [J/m^2] the emitters (e.g. tube_emitters of a lamp pose and dwell time) add to every
  // vertex of a query_mesh result, shadowed by the volume (sample_offset 0.5: the mesh's half-voxel
  // shift; cfg null = the defaults). Fills mesh.normals when empty (the nearest voxel's unit normal) and
  // accumulates into mesh.dose, sized and zeroed when empty. carry_dose (uv_dose.h) moves the dose of an
  // earlier extraction over by mesh.keys.
  void irradiate(TriMesh& mesh, const std::vector<UVEmitter>& emitters, const tsdf_uv_config* cfg = nullptr);
  // Where to hold the lamp next (DESIGN.md "Lamp-stop planning"): the greedy choice of at most max_stops
  // of the candidates (tube_candidates of standoff_candidates, uv_dose.h) against what the high-touch
  // surface of a query_mesh result still lacks -- need = plan_need(dose, mesh.prob, target, prob_min), dose
  // one value per vertex (empty: zeros), weight = vertex_area * mesh.prob. Fills mesh.normals when empty,
  // as irradiate does. stops[r] is the candidate of round r, gains[r] the weighted dose it removed, need
  // what is still missing after the stops. The same inputs give the same plan.
  struct LampPlan {
    std::vector<int32_t> stops;
    std::vector<double> gains;
    std::vector<float> need;
  };
  LampPlan plan_irradiation(TriMesh& mesh, const std::vector<float>& dose, float target,
                            const LampCandidates& candidates, int max_stops = 16, float min_gain = 0.0f,
                            float prob_min = 0.5f, const tsdf_uv_config* cfg = nullptr);
  // The clearance layer a lamp planner asks: squared Euclidean distances [voxels^2] from every voxel whose
  // centre lies in `volumn` to the nearest surface voxel there, saturated at max_dist^2, with the voxels'
  // state (TSDFGrid::DistanceField). unknown: never-observed space is an obstacle as well.
  DistanceField query_distance_field(const BoundingCube<float>& volumn, int max_dist = 255, int min_weight = 1,
                                     bool unknown = false);
  // Whether and how far a lamp travels to reach the voxels of such a field: the travel field
  // (TSDFGrid::TravelField) flooded from the voxel nearest to each world position of from_world (3 floats
  // each, e.g. where the arm is now) through voxels at least clearance_m metres from every surface voxel
  // that are observed free or, with unknown_free, never observed (the optimistic planner: an unobserved
  // gap in a wall leaks). reachable_candidates (uv_dose.h) filters standoff_candidates with it;
  // tsdf().TravelPaths gives the way to a chosen stop.
  TravelField query_travel_field(const DistanceField& field, const std::vector<float>& from_world,
                                 float clearance_m = 0.0f, bool unknown_free = false);
  // Observed free space (DESIGN.md "Observed free space"). Opt-in: once enabled, every frame integrated from
  // then on is also observed into a layer over `volumn` that the system owns -- a bit per voxel, set when a
  // depth frame saw the voxel as free, whether or not its block exists. query_free_space returns a copy of a
  // distance field with its unobserved voxels promoted to free where the layer says so (*promoted: how many),
  // to be handed to query_travel_field(..., unknown_free = false): the field then floods exactly the space the
  // camera saw empty, and a gap in a wall nobody looked through does not leak. The camera centre itself is
  // never marked: start from a position in front of the camera. Without enable_free_space nothing changes.
  void enable_free_space(const BoundingCube<float>& volumn);
  DistanceField query_free_space(const DistanceField& field, int64_t* promoted = nullptr);
  // Where the map ends (DESIGN.md "Frontiers and components"): the observed-free voxels of `field` that touch
  // unobserved space and that `travel` (over the same box; may be null) reached, clustered into 26-connected
  // components of at least min_size voxels. Each cluster carries its size, bounding box, coordinate sums and
  // its goal: the member cheapest to travel to, goal_key / 3 voxels away (frontier_goals in uv_dose.h gives
  // world positions). field should come from query_free_space, over surface sites.
  FrontierSet query_frontiers(const DistanceField& field, const TravelField* travel = nullptr, int min_size = 1);
  // Where to look next (DESIGN.md "View gain"): the distance field over `volumn` (surface sites), promoted by
  // the free layer (enable_free_space first), the travel field from from_world with clearance_m, its frontiers of
  // at least min_size voxels, `yaws` candidate poses of camera `cam` at every cluster's goal (view_candidates in
  // uv_dose.h), and the greedy choice of up to k of them by the unobserved voxels each would add
  // (TSDFSystem::NextViewsOf), rays marched `far` metres.
  NextViews query_next_views(int k, const BoundingCube<float>& volumn, const std::vector<float>& from_world,
                             const CameraParams& cam, float far = 3.0f, float clearance_m = 0.0f, int min_size = 1,
                             int yaws = 8, float pitch = 0.0f, int max_dist = 255);
  TSDFSystem& tsdf() { return *TSDF_; }

 private:
  std::shared_ptr<TSDFSystem> TSDF_;
  std::shared_ptr<pose_manager> camera_pose_manager_;
  float depthmap_factor_;
};

}  // namespace disinfect
