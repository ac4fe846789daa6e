// tsdf_module.cc -- TSDFSystem (modules/tsdf_module.cc:5-75) on the MI355X engine.
#include "tsdf_module.h"

#include <cstdio>
#include <stdexcept>

namespace disinfect {

TSDFSystem::TSDFSystem(float voxel_size, float truncation, float max_depth,
                       const CameraIntrinsics<float>& intrinsics, const SE3<float>& extrinsics)
    : tsdf_(voxel_size, truncation),
      max_depth_(max_depth),
      intrinsics_(intrinsics),
      cam_T_posecam_(extrinsics),
      t_(&TSDFSystem::Run, this) {}

TSDFSystem::TSDFSystem(const tsdf_config& cfg, int device, float max_depth,
                       const CameraIntrinsics<float>& intrinsics, const SE3<float>& extrinsics)
    : tsdf_(cfg, device),
      max_depth_(max_depth),
      intrinsics_(intrinsics),
      cam_T_posecam_(extrinsics),
      t_(&TSDFSystem::Run, this) {}

TSDFSystem::TSDFSystem(const tsdf_config& cfg, const std::vector<int>& devices, float max_depth,
                       const CameraIntrinsics<float>& intrinsics, const SE3<float>& extrinsics)
    : tsdf_(cfg, devices),
      max_depth_(max_depth),
      intrinsics_(intrinsics),
      cam_T_posecam_(extrinsics),
      t_(&TSDFSystem::Run, this) {}

TSDFSystem::~TSDFSystem() {
  {
    std::lock_guard<std::mutex> lock(mtx_queue_);
    terminate_ = true;
  }
  cv_queue_.notify_all();
  t_.join();
}

void TSDFSystem::Integrate(const SE3<float>& posecam_T_world, const Mat& img_rgb,
                           const Mat& img_depth, const Mat& img_ht, const Mat& img_lt) {
  std::unique_ptr<TSDFSystemInput> in;
  if (img_ht.empty() || img_lt.empty()) {
    // tsdf_module.cc:29-33 substitutes all-ones maps; the engine reads absent maps as ones
    in = std::make_unique<TSDFSystemInput>(cam_T_posecam_ * posecam_T_world, img_rgb.clone(),
                                           img_depth.clone(), Mat(), Mat());
  } else {
    in = std::make_unique<TSDFSystemInput>(cam_T_posecam_ * posecam_T_world, img_rgb.clone(),
                                           img_depth.clone(), img_ht.clone(), img_lt.clone());
  }
  Enqueue(std::move(in));
}

void TSDFSystem::IntegrateRaw(const SE3<float>& posecam_T_world, const Mat& img_rgb,
                              const Mat& img_depth_raw, const Mat& mask, float depth_factor) {
  if (!(depth_factor > 0.0f)) throw std::invalid_argument("TSDFSystem::IntegrateRaw: depth_factor <= 0");
  Enqueue(std::make_unique<TSDFSystemInput>(cam_T_posecam_ * posecam_T_world, img_rgb.clone(),
                                            img_depth_raw.clone(), mask.empty() ? Mat() : mask.clone(),
                                            Mat(), depth_factor));
}

void TSDFSystem::Enqueue(std::unique_ptr<TSDFSystemInput> in) {
  {
    std::lock_guard<std::mutex> lock(mtx_queue_);
    inputs_.push(std::move(in));
    if (inputs_.size() > 10)  // tsdf_module.cc:62-63
      std::fprintf(stderr, "[TSDF System] Processing cannot catch up (input size: %zu)\n", inputs_.size());
  }
  cv_queue_.notify_one();
}

std::vector<VoxelSpatialTSDF> TSDFSystem::Query(const BoundingCube<float>& volumn) {
  std::lock_guard<std::mutex> lock(mtx_read_);
  return tsdf_.GatherVoxels(volumn);
}

TriMesh TSDFSystem::QueryMesh(const BoundingCube<float>& volumn) {
  std::lock_guard<std::mutex> lock(mtx_read_);
  return tsdf_.ExtractMesh(&volumn);
}

void TSDFSystem::Render(const CameraParams& virtual_cam, const SE3<float> cam_T_world, Mat* img_normal) {
  std::lock_guard<std::mutex> lock(mtx_read_);
  tsdf_.RayCast(max_depth_, virtual_cam, cam_T_world, nullptr, img_normal);
}

TrackResult TSDFSystem::Track(const Mat& img_depth, const SE3<float>& guess_posecam_T_world,
                              const tsdf_track_config* cfg) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  TrackResult r = tsdf_.Track(img_depth, max_depth_, intrinsics_, cam_T_posecam_ * guess_posecam_T_world, cfg);
  r.pose = cam_T_posecam_.Inverse() * r.pose;
  return r;
}

std::vector<float> TSDFSystem::SurfaceNormals(const std::vector<float>& points, float sample_offset) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.SurfaceNormals(points, sample_offset);
}

void TSDFSystem::AccumulateDose(const std::vector<float>& points, const std::vector<float>& normals,
                                const std::vector<tsdf_uv_emitter>& emitters, std::vector<float>* dose,
                                const tsdf_uv_config* cfg) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  tsdf_.AccumulateDose(points, normals, emitters, dose, cfg);
}

std::vector<float> TSDFSystem::Irradiance(const std::vector<float>& points, const std::vector<float>& normals,
                                          const std::vector<tsdf_uv_emitter>& emitters,
                                          const std::vector<int32_t>& first, const tsdf_uv_config* cfg) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.Irradiance(points, normals, emitters, first, cfg);
}

std::vector<int32_t> TSDFSystem::PlanStops(const std::vector<float>& irradiance, int32_t candidates,
                                           std::vector<float>* need, const std::vector<float>& weight, int max_stops,
                                           float min_gain, std::vector<double>* gains) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.PlanStops(irradiance, candidates, need, weight, max_stops, min_gain, gains);
}

struct DistanceField TSDFSystem::DistanceField(const BoundingCube<float>& volumn, int max_dist, int min_weight,
                                               bool unknown) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.DistanceField(volumn, max_dist, min_weight, unknown);
}

struct TravelField TSDFSystem::TravelField(const struct DistanceField& field, const std::vector<int32_t>& seeds,
                                           int clearance2, bool unknown_free) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.TravelField(field, seeds, clearance2, unknown_free);
}

std::vector<std::vector<int32_t>> TSDFSystem::TravelPaths(const struct TravelField& travel,
                                                          const std::vector<int32_t>& targets, int max_len) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.TravelPaths(travel, targets, max_len);
}

FrontierSet TSDFSystem::Frontiers(const struct DistanceField& field, const struct TravelField* travel, int min_size) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.Frontiers(field, travel, min_size);
}

FrontierSet TSDFSystem::Components(const std::vector<uint8_t>& mask, const int32_t origin[3], const int32_t dims[3],
                                   const std::vector<uint32_t>& key, int min_size) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.Components(mask, origin, dims, key, min_size);
}

ViewGainResult TSDFSystem::ViewGain(const struct DistanceField& field, const std::vector<SE3<float>>& views,
                                    const CameraParams& cam, float far, float step, float margin, float miss_depth,
                                    const FreeLayer* seen, bool want_depth) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  return tsdf_.ViewGain(field, views, cam, far, step, margin, miss_depth, seen, want_depth);
}

NextViews TSDFSystem::NextViewsOf(const struct DistanceField& field, const std::vector<SE3<float>>& views,
                                  const CameraParams& cam, int k, float far, float step, float miss_depth) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  NextViews out;
  out.views = views;
  for (int a = 0; a < 3; ++a) out.seen.origin[a] = field.origin[a], out.seen.dims[a] = field.dims[a];
  const int64_t words = tsdf_free_words(field.dims);
  if (words == 0) throw std::invalid_argument("TSDFSystem::NextViewsOf: the field's box is not a layer's");
  out.seen.bits.assign((size_t)words, 0u);
  std::vector<float> depth;  // (the images depend on the state alone: one march serves every round)
  const size_t npix = (size_t)std::max(cam.img_w, 0) * (size_t)std::max(cam.img_h, 0);
  for (int round = 0; round < k && !views.empty(); ++round) {
    ViewGainResult r = tsdf_.ViewGain(field, views, cam, far, step, -1.0f, miss_depth, &out.seen, depth.empty());
    if (depth.empty()) depth.swap(r.depth);
    size_t best = 0;
    for (size_t i = 1; i < r.gain.size(); ++i)
      if (r.gain[i] > r.gain[best]) best = i;  // (the first of the largest)
    if (r.gain[best] <= 0) break;
    const Mat img(cam.img_h, cam.img_w, CV_32FC1, depth.data() + best * npix);
    tsdf_.ObserveFree(out.seen, img, 2.0f * far, cam.intrinsics, views[best]);
    out.chosen.push_back((int32_t)best);
    out.gains.push_back(r.gain[best]);
  }
  return out;
}

void TSDFSystem::EnableFreeSpace(const BoundingCube<float>& volumn) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  free_ = std::make_unique<FreeLayer>(tsdf_.MakeFreeLayer(volumn));
}

struct DistanceField TSDFSystem::ApplyFreeSpace(const struct DistanceField& field, int64_t* promoted) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  if (!free_) throw std::logic_error("TSDFSystem::ApplyFreeSpace: EnableFreeSpace first");
  return tsdf_.ApplyFree(*free_, field, promoted);
}

FreeLayer TSDFSystem::FreeSpace() {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  if (!free_) throw std::logic_error("TSDFSystem::FreeSpace: EnableFreeSpace first");
  return *free_;
}

void TSDFSystem::ImportBlocks(const void* records, int64_t n, bool replace) {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  if (!tsdf_.engine()) throw std::runtime_error("TSDFSystem::ImportBlocks: not available on a sharded volume");
  check_tsdf(tsdf_import_blocks(tsdf_.engine(), records, n, TSDF_MEM_HOST, replace ? 1 : 0), "tsdf_import_blocks");
}

void TSDFSystem::HalfRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor,
                          Mat* rgb_out, Mat* depth_out) {
  std::lock_guard<std::mutex> lock(mtx_read_);
  tsdf_.HalfRGBD(img_rgb, img_depth_raw, mask, depth_factor, rgb_out, depth_out);
}

void TSDFSystem::Flush() {
  std::unique_lock<std::mutex> lock(mtx_queue_);
  cv_idle_.wait(lock, [&] { return inputs_.empty() && !busy_; });
  std::lock_guard<std::mutex> lr(mtx_read_);
  tsdf_.Synchronize();
}

tsdf_stats TSDFSystem::Stats() {
  std::lock_guard<std::mutex> lock(mtx_read_);
  return tsdf_.Stats();
}

void TSDFSystem::Run() {
  while (true) {
    std::unique_ptr<TSDFSystemInput> input;
    {
      std::unique_lock<std::mutex> lock(mtx_queue_);
      cv_queue_.wait(lock, [&] { return terminate_ || !inputs_.empty(); });
      if (terminate_) return;
      input = std::move(inputs_.front());
      inputs_.pop();
      busy_ = true;
    }
    try {
      std::lock_guard<std::mutex> lock(mtx_read_);
      if (input->depth_factor > 0.0f)
        tsdf_.FeedRGBD(input->img_rgb, input->img_depth, input->img_ht, input->depth_factor, max_depth_,
                       intrinsics_, input->cam_T_world);
      else
        tsdf_.Integrate(input->img_rgb, input->img_depth, input->img_ht, input->img_lt, max_depth_,
                        intrinsics_, input->cam_T_world);
      if (free_) {  // the space this frame saw empty (EnableFreeSpace)
        if (input->depth_factor > 0.0f) {
          Mat rgb_half, depth_half;
          tsdf_.HalfRGBD(input->img_rgb, input->img_depth, input->img_ht, input->depth_factor, &rgb_half, &depth_half);
          tsdf_.ObserveFree(*free_, depth_half, max_depth_, intrinsics_, input->cam_T_world);
        } else {
          tsdf_.ObserveFree(*free_, input->img_depth, max_depth_, intrinsics_, input->cam_T_world);
        }
      }
    } catch (const std::exception& ex) {  // never let an engine error kill the worker
      std::fprintf(stderr, "[TSDF System] integrate failed: %s\n", ex.what());
    }
    {
      std::lock_guard<std::mutex> lock(mtx_queue_);
      busy_ = false;
    }
    cv_idle_.notify_all();
  }
}

}  // namespace disinfect
