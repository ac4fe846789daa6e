// voxel_tsdf.h -- TSDFGrid (utils/tsdf/voxel_tsdf.cuh:32-124) on the MI355X engine's C ABI.
#pragma once

#include <string>
#include <vector>

#include "disinfect_tsdf.h"
#include "tsdf_types.h"

namespace disinfect {

class TSDFGrid {
 public:
  // voxel_tsdf.cuh:40 TSDFGrid(voxel_size, truncation); engine sizing defaults to the reference's
  // (2^18 blocks, images up to 1920x1080), overridable through cfg.
  TSDFGrid(float voxel_size, float truncation);
  TSDFGrid(const tsdf_config& cfg, int device = 0);
  // one volume spatially sharded over `devices` (one shard per entry; a device may repeat), the
  // exchange inside the library (tsdf_group_*): same results as one volume. FeedRGBD is not
  // available on a sharded volume (integrate the preprocessed frame).
  TSDFGrid(const tsdf_config& cfg, const std::vector<int>& devices);
  ~TSDFGrid();
  TSDFGrid(const TSDFGrid&) = delete;
  TSDFGrid& operator=(const TSDFGrid&) = delete;

  // voxel_tsdf.cu:347-375: rgb CV_8UC3, depth CV_32FC1 [m], ht / lt CV_32FC1 (empty -> ones)
  void Integrate(const Mat& img_rgb, const Mat& img_depth, const Mat& img_ht, const Mat& img_lt,
                 float max_depth, const CameraIntrinsics<float>& intrinsics,
                 const SE3<float>& cam_T_world);

  // DISINFSystem::feed_rgbd_frame's preprocessing + Integrate on the GPU (disinfect_slam.cc:31-67):
  // full-size rgb CV_8UC3, raw depth CV_16UC1, optional mask CV_8UC1 (empty = none), all of even
  // size; intrinsics are those of the half-size image the volume integrates
  void FeedRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor,
                float max_depth, const CameraIntrinsics<float>& intrinsics,
                const SE3<float>& cam_T_world);

  // voxel_tsdf.cu:490-506: renders into CV_8UC4 images (either may be null; the reference writes
  // into GL textures, utils/gl/image.h)
  void RayCast(float max_depth, const CameraParams& virtual_cam, const SE3<float>& cam_T_world,
               Mat* tsdf_rgba = nullptr, Mat* tsdf_normal = nullptr);

  std::vector<VoxelSpatialTSDF> GatherValid();                                  // :399-425
  std::vector<VoxelSpatialTSDF> GatherVoxels(const BoundingCube<float>& volumn);  // :427-454

  // marching-cubes mesh with shared vertices, colour and high-touch probability
  // (tsdf_extract_mesh_indexed; volumn null = every allocated block). Not available on a sharded
  // volume: throws std::runtime_error.
  TriMesh ExtractMesh(const BoundingCube<float>* volumn = nullptr, float missing_tsdf = 0.99f,
                      int min_weight = 0);

  // UV dose on surface points (tsdf_surface_normals / tsdf_uv_dose; 3 floats per point and normal):
  // the nearest voxel's unit normal of each point, and the dose [J/m^2] the emitters add to each
  // receiver, shadowed by the volume (cfg null = the defaults). sample_offset: 0.5 for ExtractMesh's
  // vertices, 0 for RayCastSurface's points. Not available on a sharded volume: std::runtime_error.
  std::vector<float> SurfaceNormals(const std::vector<float>& points, float sample_offset);
  void AccumulateDose(const std::vector<float>& points, const std::vector<float>& normals,
                      const std::vector<tsdf_uv_emitter>& emitters, std::vector<float>* dose,
                      const tsdf_uv_config* cfg = nullptr);

  // Lamp-stop planning (tsdf_uv_irradiance / tsdf_uv_plan). Irradiance: the dose each of C candidates
  // (emitters[first[c] .. first[c + 1] - 1]; first holds C + 1 offsets) alone would add to each receiver, C
  // rows of one float per receiver. Not available on a sharded volume. PlanStops: the greedy choice of at
  // most max_stops rows of such a matrix against the missing dose `need` (updated in place) and the
  // weights (empty: all 1); returns the chosen candidates in order and, through gains, each round's gain.
  // It does not touch the volume.
  std::vector<float> Irradiance(const std::vector<float>& points, const std::vector<float>& normals,
                                const std::vector<tsdf_uv_emitter>& emitters, const std::vector<int32_t>& first,
                                const tsdf_uv_config* cfg = nullptr);
  std::vector<int32_t> PlanStops(const std::vector<float>& irradiance, int32_t candidates, std::vector<float>* need,
                                 const std::vector<float>& weight, int max_stops = 16, float min_gain = 0.0f,
                                 std::vector<double>* gains = nullptr);

  // Exact Euclidean distance field (tsdf_distance_field) over the voxels whose centres lie in `volumn`
  // (voxel v's centre is v * voxel_size): squared distances [voxels^2] to the nearest surface voxel of the
  // box, saturated at max_dist^2; unknown: unobserved voxels are sites too. Pad the cube by max_dist voxels
  // for the volume's own distances. Throws std::invalid_argument on an empty cube or one the call refuses
  // (more than 2048 voxels along an axis or 2^28 in all). Not available on a sharded volume.
  struct DistanceField DistanceField(const BoundingCube<float>& volumn, int max_dist = 255, int min_weight = 1,
                                     bool unknown = false);

  // Travel field (tsdf_travel_field) over a distance field's box: the least travel cost from the seeds (global
  // voxel coordinates, 3 each) through voxels with d2 >= clearance2 that are observed free or, with
  // unknown_free, unobserved. TravelPaths (tsdf_travel_paths): the walk from each target (global voxel
  // coordinates, 3 each) back to a seed as box-local linear indices, target first; empty for a target
  // outside the box or unreached; asks again while a path is longer than max_len. Neither touches the
  // volume. Not available on a sharded volume, like the distance field they start from.
  struct TravelField TravelField(const struct DistanceField& field, const std::vector<int32_t>& seeds,
                                 int clearance2 = 0, bool unknown_free = false);
  std::vector<std::vector<int32_t>> TravelPaths(const struct TravelField& travel, const std::vector<int32_t>& targets,
                                                int max_len = 4096);
  float voxel_size() const { return voxel_size_; }

  // Observed free space (tsdf_free_observe / tsdf_free_apply). MakeFreeLayer: a cleared layer over the voxels
  // whose centres lie in `volumn` (the box DistanceField takes for the same cube). ObserveFree: every voxel of
  // the layer's box that this depth frame (CV_32FC1 [m]) saw as free -- the update's own projection, sdf >=
  // truncation, in front of the camera plane -- gets its bit set, whether or not its block exists. ApplyFree:
  // a copy of the field with state 0 promoted to 1 where the layer's bit is set (the boxes may differ);
  // *promoted the number of voxels changed. Hand the copy to TravelField(..., unknown_free = false). Neither
  // touches the volume. Not available on a sharded volume, like the distance field.
  FreeLayer MakeFreeLayer(const BoundingCube<float>& volumn) const;
  void ObserveFree(FreeLayer& layer, const Mat& img_depth, float max_depth, const CameraIntrinsics<float>& intrinsics,
                   const SE3<float>& cam_T_world);
  struct DistanceField ApplyFree(const FreeLayer& layer, const struct DistanceField& field,
                                 int64_t* promoted = nullptr);

  // Frontiers and components (tsdf_frontier_mark / tsdf_components). Components: the 26-connected components
  // of a mask over a box (nz * ny * nx bytes, members nonzero) as a FrontierSet whose mask is a copy; key
  // (empty, or one uint32 per voxel) chooses each cluster's goal: the member with the least key. Frontiers: the
  // mask of the field's observed-free voxels that touch unobserved space and, with travel, were reached by it,
  // clustered with key = travel->cost, so a cluster's goal is its cheapest voxel to travel to. The field
  // should come from ApplyFree and surface sites. Neither touches the volume. Not available on a sharded
  // volume, like the distance field.
  FrontierSet Components(const std::vector<uint8_t>& mask, const int32_t origin[3], const int32_t dims[3],
                         const std::vector<uint32_t>& key = {}, int min_size = 1);
  FrontierSet Frontiers(const struct DistanceField& field, const struct TravelField* travel = nullptr,
                        int min_size = 1);

  // View gain (tsdf_view_gain): for each candidate cam_T_world, the unobserved voxels (state 0) of the field's
  // box, outside `seen` when given (a layer over the same box), that the view's predicted depth image would mark
  // free. Rays are marched `far` metres in steps of `step` (<= 0: the voxel size) to the first state-2 voxel;
  // a ray that meets none reads miss_depth (< 0: far; 0: no return). margin < 0: the truncation. Host arrays;
  // does not touch the volume. Not available on a sharded volume, like the distance field.
  ViewGainResult ViewGain(const struct DistanceField& field, const std::vector<SE3<float>>& views,
                          const CameraParams& cam, float far, float step = 0.0f, float margin = -1.0f,
                          float miss_depth = -1.0f, const FreeLayer* seen = nullptr, bool want_depth = false);

  // what RayCast sees as float maps (tsdf_raycast_surface). Not available on a sharded volume:
  // throws std::runtime_error, like Track and HalfRGBD.
  SurfaceMaps RayCastSurface(float max_depth, const CameraParams& virtual_cam, const SE3<float>& cam_T_world);
  // the camera pose of a depth frame (CV_32FC1 [m]) by frame-to-model ICP from `guess` (tsdf_track;
  // cfg null = KinectFusion's schedule)
  TrackResult Track(const Mat& img_depth, float max_depth, const CameraIntrinsics<float>& intrinsics,
                    const SE3<float>& guess_cam_T_world, const tsdf_track_config* cfg = nullptr);
  // FeedRGBD's preprocessing alone (tsdf_rgbd_half): the half-size CV_8UC3 rgb and CV_32FC1 depth
  void HalfRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor, Mat* rgb_out,
                Mat* depth_out);

  tsdf_stats Stats(bool clear_status = false);
  tsdf_engine* engine() { return engine_; }  // (NULL for a sharded volume)
  tsdf_group* group() { return group_; }      // (NULL for one engine)
  // block until every integrated frame is in the volume
  void Synchronize();

 private:
  std::vector<VoxelSpatialTSDF> Query(const float* bounds);
  tsdf_engine* engine_ = nullptr;
  tsdf_group* group_ = nullptr;
  float voxel_size_, truncation_;
};

// throws std::runtime_error with the engine's message on a non-zero status
void check_tsdf(int rc, const char* what);

}  // namespace disinfect
