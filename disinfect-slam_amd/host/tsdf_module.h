// tsdf_module.h -- TSDFSystem (modules/tsdf_module.h:16-107): threaded facade over TSDFGrid.
//
// Same contract as the reference: Integrate() is a non-blocking enqueue (it composes
// cam_T_posecam * posecam_T_world and substitutes all-ones ht / lt maps when they are empty,
// tsdf_module.cc:26-38); one worker thread integrates in order; Integrate, Query and Render are
// mutually exclusive (mtx_read_). Differences: the worker waits on a condition variable instead of
// busy-spinning (tsdf_module.cc:51-75), and the queue deep-copies the frames because Mat views
// may borrow caller memory (the reference keeps shallow ref-counted cv::Mat).
#pragma once

#include <condition_variable>
#include <memory>
#include <mutex>
#include <queue>
#include <thread>

#include "voxel_tsdf.h"

namespace disinfect {

struct TSDFSystemInput {
  SE3<float> cam_T_world;
  Mat img_rgb;
  Mat img_depth;
  Mat img_ht;   // raw frames: the mask
  Mat img_lt;
  float depth_factor = 0.0f;  // > 0: a raw sensor frame (FeedRGBD) with depth in sensor units

  TSDFSystemInput(const SE3<float>& cam_T_world, const Mat& img_rgb, const Mat& img_depth,
                  const Mat& img_ht, const Mat& img_lt, float depth_factor = 0.0f)
      : cam_T_world(cam_T_world), img_rgb(img_rgb), img_depth(img_depth), img_ht(img_ht),
        img_lt(img_lt), depth_factor(depth_factor) {}
};

class TSDFSystem {
 public:
  TSDFSystem(float voxel_size, float truncation, float max_depth,
             const CameraIntrinsics<float>& intrinsics,
             const SE3<float>& extrinsics = SE3<float>::Identity());
  // engine sizing / device selection beyond the reference constructor
  TSDFSystem(const tsdf_config& cfg, int device, float max_depth,
             const CameraIntrinsics<float>& intrinsics,
             const SE3<float>& extrinsics = SE3<float>::Identity());
  // one volume spatially sharded over `devices` (TSDFGrid's group constructor): a C++ caller gets a
  // multi-GPU (or multi-shard) volume without Python or a collective library
  TSDFSystem(const tsdf_config& cfg, const std::vector<int>& devices, float max_depth,
             const CameraIntrinsics<float>& intrinsics,
             const SE3<float>& extrinsics = SE3<float>::Identity());
  ~TSDFSystem();

  void Integrate(const SE3<float>& posecam_T_world, const Mat& img_rgb, const Mat& img_depth,
                 const Mat& img_ht = {}, const Mat& img_lt = {});
  // a raw full-size sensor frame (CV_8UC3 rgb, CV_16UC1 depth, optional CV_8UC1 mask): the GPU
  // runs DISINFSystem::feed_rgbd_frame's resize / depth scale / mask before integrating
  void IntegrateRaw(const SE3<float>& posecam_T_world, const Mat& img_rgb, const Mat& img_depth_raw,
                    const Mat& mask, float depth_factor);
  std::vector<VoxelSpatialTSDF> Query(const BoundingCube<float>& volumn);
  TriMesh QueryMesh(const BoundingCube<float>& volumn);  // TSDFGrid::ExtractMesh, under Query's lock
  void Render(const CameraParams& virtual_cam, const SE3<float> cam_T_world, Mat* img_normal);

  // The pose of a depth frame (CV_32FC1 [m], the size the volume integrates) by frame-to-model ICP
  // (TSDFGrid::Track): waits until every queued frame is integrated, then tracks under Query's lock.
  // guess and the result are posecam_T_world, as Integrate takes it.
  TrackResult Track(const Mat& img_depth, const SE3<float>& guess_posecam_T_world,
                    const tsdf_track_config* cfg = nullptr);
  // DISINFSystem::feed_rgbd_frame's preprocessing of a raw sensor frame alone (TSDFGrid::HalfRGBD)
  void HalfRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor, Mat* rgb_out,
                Mat* depth_out);

  // UV dose (TSDFGrid::SurfaceNormals / AccumulateDose): like Track, they wait until every queued frame
  // is integrated and run under Query's lock
  std::vector<float> SurfaceNormals(const std::vector<float>& points, float sample_offset);
  void AccumulateDose(const std::vector<float>& points, const std::vector<float>& normals,
                      const std::vector<tsdf_uv_emitter>& emitters, std::vector<float>* dose,
                      const tsdf_uv_config* cfg = nullptr);
  // lamp-stop planning (TSDFGrid::Irradiance / PlanStops): wait and lock like the dose calls
  std::vector<float> Irradiance(const std::vector<float>& points, const std::vector<float>& normals,
                                const std::vector<tsdf_uv_emitter>& emitters, const std::vector<int32_t>& first,
                                const tsdf_uv_config* cfg = nullptr);
  std::vector<int32_t> PlanStops(const std::vector<float>& irradiance, int32_t candidates, std::vector<float>* need,
                                 const std::vector<float>& weight, int max_stops = 16, float min_gain = 0.0f,
                                 std::vector<double>* gains = nullptr);
  // the distance field of the voxels in `volumn` (TSDFGrid::DistanceField): waits and locks like the dose calls
  struct DistanceField DistanceField(const BoundingCube<float>& volumn, int max_dist = 255, int min_weight = 1,
                                     bool unknown = false);
  // the travel field over a distance field's box and the paths back (TSDFGrid::TravelField / TravelPaths):
  // wait and lock like the distance field
  struct TravelField TravelField(const struct DistanceField& field, const std::vector<int32_t>& seeds,
                                 int clearance2 = 0, bool unknown_free = false);
  std::vector<std::vector<int32_t>> TravelPaths(const struct TravelField& travel, const std::vector<int32_t>& targets,
                                                int max_len = 4096);
  float voxel_size() const { return tsdf_.voxel_size(); }
  // frontiers and components (TSDFGrid::Frontiers / Components), after every queued frame
  FrontierSet Frontiers(const struct DistanceField& field, const struct TravelField* travel = nullptr,
                        int min_size = 1);
  FrontierSet Components(const std::vector<uint8_t>& mask, const int32_t origin[3], const int32_t dims[3],
                         const std::vector<uint32_t>& key = {}, int min_size = 1);
  // view gain (TSDFGrid::ViewGain), after every queued frame; NextViews: the greedy choice of up to k of
  // `views` -- each round the largest gain against what the chosen views will observe wins (ties to the lowest
  // index, stop at gain 0) and its predicted image is committed with ObserveFree (max_depth 2 far; the margin is
  // the truncation, so a gain is exactly what the commit adds)
  ViewGainResult ViewGain(const struct DistanceField& field, const std::vector<SE3<float>>& views, const CameraParams& cam,
                          float far, float step = 0.0f, float margin = -1.0f, float miss_depth = -1.0f,
                          const FreeLayer* seen = nullptr, bool want_depth = false);
  NextViews NextViewsOf(const struct DistanceField& field, const std::vector<SE3<float>>& views, const CameraParams& cam,
                        int k, float far, float step = 0.0f, float miss_depth = -1.0f);
  // Observed free space (TSDFGrid::ObserveFree / ApplyFree). EnableFreeSpace: from the next queued frame on,
  // the worker also observes every frame it integrates into a layer over `volumn` that the system owns (a raw
  // frame's half-size depth is taken from HalfRGBD once more); calling it again starts a cleared layer.
  // ApplyFreeSpace: the field promoted by that layer, after every queued frame (std::logic_error before
  // EnableFreeSpace). FreeSpace: a copy of the layer. Without EnableFreeSpace nothing changes.
  void EnableFreeSpace(const BoundingCube<float>& volumn);
  struct DistanceField ApplyFreeSpace(const struct DistanceField& field, int64_t* promoted = nullptr);
  FreeLayer FreeSpace();
  // the volume replaced by (replace) or extended with n block records (tsdf_import_blocks, host memory;
  // one unsharded volume only), after every queued frame
  void ImportBlocks(const void* records, int64_t n, bool replace);
  // (NULL for a sharded volume; for tsdf_uv_config_default and the like, not for calls beside the worker)
  tsdf_engine* engine() { return tsdf_.engine(); }

  // block until every queued frame has been integrated (not in the reference; used by tests)
  void Flush();
  tsdf_stats Stats();

 private:
  void Run();
  void Enqueue(std::unique_ptr<TSDFSystemInput> in);
  TSDFGrid tsdf_;
  float max_depth_;
  const CameraIntrinsics<float> intrinsics_;
  const SE3<float> cam_T_posecam_;
  std::mutex mtx_queue_;
  std::condition_variable cv_queue_;
  std::condition_variable cv_idle_;
  std::queue<std::unique_ptr<TSDFSystemInput>> inputs_;
  bool busy_ = false;
  std::mutex mtx_read_;
  std::unique_ptr<FreeLayer> free_;  // under mtx_read_; null until EnableFreeSpace
  bool terminate_ = false;
  std::thread t_;
};

}  // namespace disinfect
