// voxel_tsdf.cc -- TSDFGrid facade over include/disinfect_tsdf.h.
#include "voxel_tsdf.h"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace disinfect {

void check_tsdf(int rc, const char* what) {
  if (rc != TSDF_OK)
    throw std::runtime_error(std::string(what) + ": " + tsdf_error_string(rc) + " (" +
                             tsdf_last_error() + ")");
}

TSDFGrid::TSDFGrid(float voxel_size, float truncation)
    : voxel_size_(voxel_size), truncation_(truncation) {
  tsdf_config cfg;
  tsdf_config_default(&cfg);
  cfg.voxel_size = voxel_size;
  cfg.truncation = truncation;
  check_tsdf(tsdf_create(&cfg, 0, &engine_), "tsdf_create");
}

TSDFGrid::TSDFGrid(const tsdf_config& cfg, int device)
    : voxel_size_(cfg.voxel_size), truncation_(cfg.truncation) {
  check_tsdf(tsdf_create(&cfg, device, &engine_), "tsdf_create");
}

TSDFGrid::TSDFGrid(const tsdf_config& cfg, const std::vector<int>& devices)
    : voxel_size_(cfg.voxel_size), truncation_(cfg.truncation) {
  check_tsdf(tsdf_group_create(&cfg, devices.data(), (int)devices.size(), &group_), "tsdf_group_create");
}

TSDFGrid::~TSDFGrid() {
  if (engine_) tsdf_destroy(engine_);
  if (group_) tsdf_group_destroy(group_);
}

void TSDFGrid::Synchronize() {
  if (group_)
    check_tsdf(tsdf_group_synchronize(group_), "tsdf_group_synchronize");
  else
    check_tsdf(tsdf_synchronize(engine_), "tsdf_synchronize");
}

static tsdf_pose to_pose(const SE3<float>& T) {
  const Quaternion<float> q = T.GetR();
  const float* t = T.GetT();
  return tsdf_pose{q.x, q.y, q.z, q.w, t[0], t[1], t[2]};
}

void TSDFGrid::Integrate(const Mat& img_rgb, const Mat& img_depth, const Mat& img_ht,
                         const Mat& img_lt, float max_depth,
                         const CameraIntrinsics<float>& intrinsics, const SE3<float>& cam_T_world) {
  // voxel_tsdf.cu:350-353 (asserts in the reference)
  if (img_rgb.type() != CV_8UC3 || img_depth.type() != CV_32FC1 || img_rgb.cols != img_depth.cols ||
      img_rgb.rows != img_depth.rows)
    throw std::invalid_argument("TSDFGrid::Integrate: expects CV_8UC3 rgb and CV_32FC1 depth of equal size");
  const bool sem = !img_ht.empty() && !img_lt.empty();
  if (sem && (img_ht.type() != CV_32FC1 || img_lt.type() != CV_32FC1 || img_ht.total() != img_depth.total() ||
              img_lt.total() != img_depth.total()))
    throw std::invalid_argument("TSDFGrid::Integrate: ht / lt must be CV_32FC1 of the depth size");
  tsdf_frame f;
  f.width = img_depth.cols;
  f.height = img_depth.rows;
  f.rgb = img_rgb.ptr<uint8_t>();
  f.depth = img_depth.ptr<float>();
  f.ht = sem ? img_ht.ptr<float>() : nullptr;
  f.lt = sem ? img_lt.ptr<float>() : nullptr;
  f.mem_kind = TSDF_MEM_HOST;
  const tsdf_intrinsics K{intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy};
  const tsdf_pose P = to_pose(cam_T_world);
  if (group_)
    check_tsdf(tsdf_group_integrate(group_, &f, &K, &P, max_depth), "tsdf_group_integrate");
  else
    check_tsdf(tsdf_integrate(engine_, &f, &K, &P, max_depth), "tsdf_integrate");
}

void TSDFGrid::FeedRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor,
                        float max_depth, const CameraIntrinsics<float>& intrinsics,
                        const SE3<float>& cam_T_world) {
  if (img_rgb.type() != CV_8UC3 || img_depth_raw.type() != CV_16UC1 || img_rgb.cols != img_depth_raw.cols ||
      img_rgb.rows != img_depth_raw.rows ||
      (!mask.empty() && (mask.type() != CV_8UC1 || mask.total() != img_depth_raw.total())))
    throw std::invalid_argument("TSDFGrid::FeedRGBD: expects CV_8UC3 rgb, CV_16UC1 depth, CV_8UC1 mask");
  if (group_) throw std::invalid_argument("TSDFGrid::FeedRGBD: not available on a sharded volume");
  const tsdf_intrinsics K{intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy};
  const tsdf_pose P = to_pose(cam_T_world);
  check_tsdf(tsdf_feed_rgbd_frame(engine_, img_rgb.ptr<uint8_t>(), img_depth_raw.ptr<uint16_t>(),
                                  mask.empty() ? nullptr : mask.ptr<uint8_t>(), img_depth_raw.cols,
                                  img_depth_raw.rows, depth_factor, &K, &P, max_depth, TSDF_MEM_HOST),
             "tsdf_feed_rgbd_frame");
}

void TSDFGrid::RayCast(float max_depth, const CameraParams& cam, const SE3<float>& cam_T_world,
                       Mat* rgba, Mat* normal) {
  if (rgba && (rgba->rows != cam.img_h || rgba->cols != cam.img_w || rgba->type() != CV_8UC4))
    *rgba = Mat(cam.img_h, cam.img_w, CV_8UC4);
  if (normal && (normal->rows != cam.img_h || normal->cols != cam.img_w || normal->type() != CV_8UC4))
    *normal = Mat(cam.img_h, cam.img_w, CV_8UC4);
  const tsdf_intrinsics K{cam.intrinsics.fx, cam.intrinsics.fy, cam.intrinsics.cx, cam.intrinsics.cy};
  const tsdf_pose P = to_pose(cam_T_world);
  if (group_)
    check_tsdf(tsdf_group_raycast(group_, &K, cam.img_w, cam.img_h, &P, max_depth, rgba ? rgba->data : nullptr,
                                  normal ? normal->data : nullptr, TSDF_MEM_HOST),
               "tsdf_group_raycast");
  else
    check_tsdf(tsdf_raycast(engine_, &K, cam.img_w, cam.img_h, &P, max_depth,
                            rgba ? rgba->data : nullptr, normal ? normal->data : nullptr, TSDF_MEM_HOST),
               "tsdf_raycast");
}

std::vector<VoxelSpatialTSDF> TSDFGrid::Query(const float* bounds) {
  int64_t n = 0;
  auto query = [&](tsdf_voxel* o, int64_t cap) {
    return group_ ? tsdf_group_query(group_, bounds, o, cap, &n) : tsdf_query(engine_, bounds, o, cap, &n);
  };
  check_tsdf(query(nullptr, 0), "tsdf_query");
  std::vector<VoxelSpatialTSDF> out((size_t)n);
  if (n) check_tsdf(query(reinterpret_cast<tsdf_voxel*>(out.data()), n), "tsdf_query");
  return out;
}

std::vector<VoxelSpatialTSDF> TSDFGrid::GatherValid() { return Query(nullptr); }

std::vector<VoxelSpatialTSDF> TSDFGrid::GatherVoxels(const BoundingCube<float>& v) {
  const float b[6] = {v.xmin, v.xmax, v.ymin, v.ymax, v.zmin, v.zmax};
  return Query(b);
}

TriMesh TSDFGrid::ExtractMesh(const BoundingCube<float>* v, float missing_tsdf, int min_weight) {
  if (group_) throw std::runtime_error("TSDFGrid::ExtractMesh: not available on a sharded volume");
  float b[6];
  if (v) {
    const float vb[6] = {v->xmin, v->xmax, v->ymin, v->ymax, v->zmin, v->zmax};
    for (int i = 0; i < 6; ++i) b[i] = vb[i];
  }
  int64_t nv = 0, nt = 0;
  check_tsdf(tsdf_extract_mesh_indexed(engine_, v ? b : nullptr, missing_tsdf, min_weight, nullptr, &nv, &nt),
             "tsdf_extract_mesh_indexed");
  TriMesh m;
  m.verts.resize((size_t)nv * 3);
  m.tris.resize((size_t)nt * 3);
  m.rgba.resize((size_t)nv * 4);
  m.prob.resize((size_t)nv);
  m.keys.resize((size_t)nv * 4);
  if (nv == 0 && nt == 0) return m;
  tsdf_mesh_out out{};
  out.positions = m.verts.data();
  out.rgba = m.rgba.data();
  out.prob = m.prob.data();
  out.keys = m.keys.data();
  out.indices = m.tris.data();
  out.vertex_capacity = nv;
  out.triangle_capacity = nt;
  out.mem_kind = TSDF_MEM_HOST;
  check_tsdf(tsdf_extract_mesh_indexed(engine_, v ? b : nullptr, missing_tsdf, min_weight, &out, &nv, &nt),
             "tsdf_extract_mesh_indexed");
  return m;
}

std::vector<float> TSDFGrid::SurfaceNormals(const std::vector<float>& points, float sample_offset) {
  if (group_) throw std::runtime_error("TSDFGrid::SurfaceNormals: not available on a sharded volume");
  if (points.size() % 3) throw std::invalid_argument("TSDFGrid::SurfaceNormals: 3 floats per point");
  std::vector<float> normals(points.size());
  check_tsdf(tsdf_surface_normals(engine_, points.data(), (int64_t)(points.size() / 3), sample_offset, normals.data(),
                                  TSDF_MEM_HOST),
             "tsdf_surface_normals");
  return normals;
}

void TSDFGrid::AccumulateDose(const std::vector<float>& points, const std::vector<float>& normals,
                              const std::vector<tsdf_uv_emitter>& emitters, std::vector<float>* dose,
                              const tsdf_uv_config* cfg) {
  if (group_) throw std::runtime_error("TSDFGrid::AccumulateDose: not available on a sharded volume");
  if (!dose || points.size() % 3 || normals.size() != points.size() || dose->size() * 3 != points.size())
    throw std::invalid_argument("TSDFGrid::AccumulateDose: 3 floats per point and normal, 1 per dose");
  check_tsdf(tsdf_uv_dose(engine_, points.data(), normals.data(), (int64_t)dose->size(), emitters.data(),
                          (int32_t)emitters.size(), cfg, dose->data(), TSDF_MEM_HOST),
             "tsdf_uv_dose");
}

std::vector<float> TSDFGrid::Irradiance(const std::vector<float>& points, const std::vector<float>& normals,
                                        const std::vector<tsdf_uv_emitter>& emitters, const std::vector<int32_t>& first,
                                        const tsdf_uv_config* cfg) {
  if (group_) throw std::runtime_error("TSDFGrid::Irradiance: not available on a sharded volume");
  if (points.size() % 3 || normals.size() != points.size())
    throw std::invalid_argument("TSDFGrid::Irradiance: 3 floats per point and normal");
  if (first.empty() || first.back() < 0 || (size_t)first.back() != emitters.size())
    throw std::invalid_argument("TSDFGrid::Irradiance: first holds one offset more than there are candidates and "
                                "ends at the number of emitters");
  const size_t n = points.size() / 3, C = first.size() - 1;
  std::vector<float> out(C * n);
  check_tsdf(tsdf_uv_irradiance(engine_, points.data(), normals.data(), (int64_t)n, emitters.data(), first.data(),
                                (int32_t)C, cfg, out.data(), TSDF_MEM_HOST),
             "tsdf_uv_irradiance");
  return out;
}

std::vector<int32_t> TSDFGrid::PlanStops(const std::vector<float>& irradiance, int32_t candidates,
                                         std::vector<float>* need, const std::vector<float>& weight, int max_stops,
                                         float min_gain, std::vector<double>* gains) {
  if (group_) throw std::runtime_error("TSDFGrid::PlanStops: not available on a sharded volume");
  if (!need || candidates < 0 || max_stops < 0 || irradiance.size() != (size_t)candidates * need->size() ||
      (!weight.empty() && weight.size() != need->size()))
    throw std::invalid_argument("TSDFGrid::PlanStops: one row of need's length per candidate, one weight per need");
  const tsdf_uv_plan_config c{max_stops, min_gain};
  std::vector<int32_t> stops((size_t)max_stops);
  std::vector<double> g((size_t)max_stops);
  int32_t k = 0;
  check_tsdf(tsdf_uv_plan(engine_, irradiance.data(), candidates, (int64_t)need->size(), need->data(),
                          weight.empty() ? nullptr : weight.data(), &c, stops.data(), g.data(), &k, TSDF_MEM_HOST),
             "tsdf_uv_plan");
  stops.resize((size_t)k);
  g.resize((size_t)k);
  if (gains) *gains = g;
  return stops;
}

namespace {
#define BOX_STR_(x) #x
#define BOX_STR(x) BOX_STR_(x)
static_assert(TSDF_BOX_MAX_VOXELS == 268435456, "the exception text below says 2^28");
// The voxel box of a cube -- the voxels whose centres it holds -- within the box limits (TSDF_BOX_MAX_DIM,
// TSDF_BOX_MAX_VOXELS), or std::invalid_argument in `who`'s name. Returns the number of voxels.
size_t cube_box(const BoundingCube<float>& volumn, float voxel_size, const char* who, int32_t origin[3], int32_t dims[3]) {
  const double lo[3] = {volumn.xmin, volumn.ymin, volumn.zmin}, hi[3] = {volumn.xmax, volumn.ymax, volumn.zmax};
  size_t n = 1;
  for (int a = 0; a < 3; ++a) {
    const double v0 = std::ceil(lo[a] / (double)voxel_size), v1 = std::floor(hi[a] / (double)voxel_size);
    if (!(v0 <= v1) || !(v0 > -1e9) || !(v1 < 1e9) || v1 - v0 >= (double)TSDF_BOX_MAX_DIM)
      throw std::invalid_argument(std::string(who) + ": the cube holds no voxel centre, or more than "
                                  BOX_STR(TSDF_BOX_MAX_DIM) " along an axis");
    origin[a] = (int32_t)v0;
    dims[a] = (int32_t)(v1 - v0) + 1;
    n *= (size_t)dims[a];
  }
  if (n > (size_t)TSDF_BOX_MAX_VOXELS) throw std::invalid_argument(std::string(who) + ": more than 2^28 voxels");
  return n;
}
#undef BOX_STR
#undef BOX_STR_
}  // namespace

struct DistanceField TSDFGrid::DistanceField(const BoundingCube<float>& volumn, int max_dist, int min_weight,
                                             bool unknown) {
  if (group_) throw std::runtime_error("TSDFGrid::DistanceField: not available on a sharded volume");
  struct DistanceField f;
  tsdf_edt_config c;
  tsdf_edt_config_default(&c);
  const size_t n = cube_box(volumn, voxel_size_, "TSDFGrid::DistanceField", f.origin, f.dims);
  for (int a = 0; a < 3; ++a) c.origin[a] = f.origin[a], c.dims[a] = f.dims[a];
  c.max_dist = f.max_dist = max_dist;
  c.min_weight = min_weight;
  c.sites = TSDF_EDT_SURFACE | (unknown ? TSDF_EDT_UNKNOWN : 0);
  f.d2.resize(n);
  f.state.resize(n);
  tsdf_edt_out out{};
  out.d2 = f.d2.data();
  out.state = f.state.data();
  out.mem_kind = TSDF_MEM_HOST;
  check_tsdf(tsdf_distance_field(engine_, &c, &out), "tsdf_distance_field");
  return f;
}

namespace {
// global voxel triples as box-local ones, kept in int32
std::vector<int32_t> box_local(const std::vector<int32_t>& v, const int32_t origin[3], const char* what) {
  if (v.size() % 3) throw std::invalid_argument(std::string(what) + ": three coordinates per voxel");
  std::vector<int32_t> out(v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    const int64_t d = (int64_t)v[i] - origin[i % 3];
    out[i] = (int32_t)std::min<int64_t>(std::max<int64_t>(d, -((int64_t)1 << 30)), (int64_t)1 << 30);
  }
  return out;
}
}  // namespace

struct TravelField TSDFGrid::TravelField(const struct DistanceField& field, const std::vector<int32_t>& seeds,
                                         int clearance2, bool unknown_free) {
  if (group_) throw std::runtime_error("TSDFGrid::TravelField: not available on a sharded volume");
  struct TravelField t;
  tsdf_travel_config c;
  tsdf_travel_config_default(&c);
  size_t n = 1;
  for (int a = 0; a < 3; ++a) {
    t.origin[a] = field.origin[a];
    c.dims[a] = t.dims[a] = field.dims[a];
    n *= (size_t)std::max(field.dims[a], 0);
  }
  if (n == 0 || field.d2.size() != n || field.state.size() != n)
    throw std::invalid_argument("TSDFGrid::TravelField: the field needs d2 and state for every voxel of its box");
  c.clearance2 = clearance2;
  c.unknown_free = unknown_free ? 1 : 0;
  const std::vector<int32_t> s = box_local(seeds, field.origin, "TSDFGrid::TravelField");
  t.cost.resize(n);
  check_tsdf(tsdf_travel_field(engine_, &c, field.d2.data(), field.state.data(), s.empty() ? nullptr : s.data(),
                               (int32_t)(s.size() / 3), t.cost.data(), TSDF_MEM_HOST, &t.seeded, &t.rounds),
             "tsdf_travel_field");
  return t;
}

std::vector<std::vector<int32_t>> TSDFGrid::TravelPaths(const struct TravelField& travel,
                                                        const std::vector<int32_t>& targets, int max_len) {
  if (group_) throw std::runtime_error("TSDFGrid::TravelPaths: not available on a sharded volume");
  const std::vector<int32_t> t = box_local(targets, travel.origin, "TSDFGrid::TravelPaths");
  const int32_t T = (int32_t)(t.size() / 3);
  std::vector<std::vector<int32_t>> out((size_t)T);
  if (T == 0) return out;
  if (travel.dims[0] < 1 || travel.dims[1] < 1 || travel.dims[2] < 1 ||
      travel.cost.size() != (size_t)travel.dims[0] * (size_t)travel.dims[1] * (size_t)travel.dims[2])
    throw std::invalid_argument("TSDFGrid::TravelPaths: one cost per voxel of the box");
  int32_t cap = std::min(std::max(max_len, 1), 1 << 28);
  for (int32_t k0 = 0; k0 < T;) {
    const int32_t n = std::min(T - k0, std::max((1 << 28) / cap, 1));  // (a call takes T * max_len <= 2^28)
    std::vector<int32_t> path((size_t)n * cap), len((size_t)n);
    check_tsdf(tsdf_travel_paths(engine_, travel.dims, travel.cost.data(), TSDF_MEM_HOST, t.data() + 3 * (size_t)k0, n, cap,
                                 path.data(), len.data()),
               "tsdf_travel_paths");
    int32_t longest = 0;
    for (int32_t l : len) {
      if (l < 0) throw std::invalid_argument("TSDFGrid::TravelPaths: a voxel without a predecessor (not a travel field)");
      longest = std::max(longest, l);
    }
    if (longest > cap) {  // (ask again, with fewer targets per call if need be)
      cap = longest;
      continue;
    }
    for (int32_t k = 0; k < n; ++k)
      out[(size_t)(k0 + k)].assign(path.begin() + (size_t)k * cap, path.begin() + (size_t)k * cap + len[(size_t)k]);
    k0 += n;
  }
  return out;
}

FreeLayer TSDFGrid::MakeFreeLayer(const BoundingCube<float>& volumn) const {
  FreeLayer l;  // (DistanceField's box of the same cube)
  cube_box(volumn, voxel_size_, "TSDFGrid::MakeFreeLayer", l.origin, l.dims);
  l.bits.assign((size_t)tsdf_free_words(l.dims), 0u);
  return l;
}

void TSDFGrid::ObserveFree(FreeLayer& layer, const Mat& img_depth, float max_depth,
                           const CameraIntrinsics<float>& intrinsics, const SE3<float>& cam_T_world) {
  if (group_) throw std::runtime_error("TSDFGrid::ObserveFree: not available on a sharded volume");
  if (img_depth.type() != CV_32FC1 || img_depth.empty())
    throw std::invalid_argument("TSDFGrid::ObserveFree: expects a CV_32FC1 depth image");
  if ((int64_t)layer.bits.size() != tsdf_free_words(layer.dims) || layer.bits.empty())
    throw std::invalid_argument("TSDFGrid::ObserveFree: the layer's words do not match its box");
  tsdf_free_box box;
  for (int a = 0; a < 3; ++a) box.origin[a] = layer.origin[a], box.dims[a] = layer.dims[a];
  const tsdf_intrinsics K{intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy};
  const tsdf_pose P = to_pose(cam_T_world);
  check_tsdf(tsdf_free_observe(engine_, &box, layer.bits.data(), img_depth.ptr<float>(), img_depth.cols,
                               img_depth.rows, TSDF_MEM_HOST, &K, &P, max_depth),
             "tsdf_free_observe");
  ++layer.frames;
}

struct DistanceField TSDFGrid::ApplyFree(const FreeLayer& layer, const struct DistanceField& field,
                                         int64_t* promoted) {
  if (group_) throw std::runtime_error("TSDFGrid::ApplyFree: not available on a sharded volume");
  if ((int64_t)layer.bits.size() != tsdf_free_words(layer.dims) || layer.bits.empty())
    throw std::invalid_argument("TSDFGrid::ApplyFree: the layer's words do not match its box");
  size_t n = 1;
  for (int a = 0; a < 3; ++a) n *= (size_t)std::max(field.dims[a], 0);
  if (n == 0 || field.state.size() != n)
    throw std::invalid_argument("TSDFGrid::ApplyFree: the field needs a state for every voxel of its box");
  struct DistanceField out = field;
  tsdf_free_box box;
  for (int a = 0; a < 3; ++a) box.origin[a] = layer.origin[a], box.dims[a] = layer.dims[a];
  int64_t count = 0;
  check_tsdf(tsdf_free_apply(engine_, &box, layer.bits.data(), out.origin, out.dims, out.state.data(), TSDF_MEM_HOST,
                             &count),
             "tsdf_free_apply");
  if (promoted) *promoted = count;
  return out;
}

static_assert(sizeof(FrontierCluster) == sizeof(tsdf_component) && offsetof(FrontierCluster, lo) == offsetof(tsdf_component, lo) &&
                  offsetof(FrontierCluster, hi) == offsetof(tsdf_component, hi) &&
                  offsetof(FrontierCluster, sum) == offsetof(tsdf_component, sum) &&
                  offsetof(FrontierCluster, goal) == offsetof(tsdf_component, goal) &&
                  offsetof(FrontierCluster, goal_key) == offsetof(tsdf_component, goal_key),
              "FrontierCluster is tsdf_component");

FrontierSet TSDFGrid::Components(const std::vector<uint8_t>& mask, const int32_t origin[3], const int32_t dims[3],
                                 const std::vector<uint32_t>& key, int min_size) {
  if (group_) throw std::runtime_error("TSDFGrid::Components: not available on a sharded volume");
  FrontierSet s;
  tsdf_components_config c;
  tsdf_components_config_default(&c);
  size_t n = 1;
  for (int a = 0; a < 3; ++a) {
    s.origin[a] = origin[a];
    c.dims[a] = s.dims[a] = dims[a];
    n *= (size_t)std::max(dims[a], 0);
  }
  if (n == 0 || mask.size() != n || (!key.empty() && key.size() != n))
    throw std::invalid_argument("TSDFGrid::Components: the mask (and the key) need an entry for every voxel of the box");
  c.min_size = min_size;
  s.mask = mask;
  for (uint8_t m : mask) s.marked += m != 0;
  s.label.resize(n);
  // the two-call pattern with a first guess: a table too small asks again with the count it was told
  int32_t count = 0, cap = 4096;
  for (int attempt = 0;; ++attempt) {
    s.clusters.assign((size_t)cap, FrontierCluster{});
    const int rc = tsdf_components(engine_, &c, mask.data(), key.empty() ? nullptr : key.data(), s.label.data(),
                                   TSDF_MEM_HOST, reinterpret_cast<tsdf_component*>(s.clusters.data()), cap, &count,
                                   &s.total);
    if (rc == TSDF_ERR_CAPACITY && attempt == 0) {
      cap = count;
      continue;
    }
    check_tsdf(rc, "tsdf_components");
    break;
  }
  s.clusters.resize((size_t)count);
  return s;
}

FrontierSet TSDFGrid::Frontiers(const struct DistanceField& field, const struct TravelField* travel, int min_size) {
  if (group_) throw std::runtime_error("TSDFGrid::Frontiers: not available on a sharded volume");
  size_t n = 1;
  for (int a = 0; a < 3; ++a) n *= (size_t)std::max(field.dims[a], 0);
  if (n == 0 || field.state.size() != n)
    throw std::invalid_argument("TSDFGrid::Frontiers: the field needs a state for every voxel of its box");
  if (travel) {
    for (int a = 0; a < 3; ++a)
      if (travel->origin[a] != field.origin[a] || travel->dims[a] != field.dims[a])
        throw std::invalid_argument("TSDFGrid::Frontiers: the travel field's box is not the distance field's");
    if (travel->cost.size() != n) throw std::invalid_argument("TSDFGrid::Frontiers: the travel field needs a cost per voxel");
  }
  std::vector<uint8_t> mask(n);
  int64_t marked = 0;
  check_tsdf(tsdf_frontier_mark(engine_, field.dims, field.state.data(), travel ? travel->cost.data() : nullptr,
                                mask.data(), TSDF_MEM_HOST, &marked),
             "tsdf_frontier_mark");
  FrontierSet s = Components(mask, field.origin, field.dims, travel ? travel->cost : std::vector<uint32_t>(), min_size);
  s.marked = marked;
  return s;
}

ViewGainResult TSDFGrid::ViewGain(const struct DistanceField& field, const std::vector<SE3<float>>& views,
                                  const CameraParams& cam, float far, float step, float margin, float miss_depth,
                                  const FreeLayer* seen, bool want_depth) {
  if (group_) throw std::runtime_error("TSDFGrid::ViewGain: not available on a sharded volume");
  size_t n = 1;
  for (int a = 0; a < 3; ++a) n *= (size_t)std::max(field.dims[a], 0);
  if (n == 0 || field.state.size() != n)
    throw std::invalid_argument("TSDFGrid::ViewGain: the field needs a state for every voxel of its box");
  if (seen) {
    for (int a = 0; a < 3; ++a)
      if (seen->origin[a] != field.origin[a] || seen->dims[a] != field.dims[a])
        throw std::invalid_argument("TSDFGrid::ViewGain: the seen layer's box is not the field's");
    if ((int64_t)seen->bits.size() != tsdf_free_words(seen->dims) || seen->bits.empty())
      throw std::invalid_argument("TSDFGrid::ViewGain: the layer's words do not match its box");
  }
  tsdf_view_config c;
  tsdf_view_config_default(engine_, &c);
  for (int a = 0; a < 3; ++a) c.origin[a] = field.origin[a], c.dims[a] = field.dims[a];
  c.width = cam.img_w, c.height = cam.img_h;
  c.K = tsdf_intrinsics{cam.intrinsics.fx, cam.intrinsics.fy, cam.intrinsics.cx, cam.intrinsics.cy};
  c.far = far;
  if (step > 0.0f) c.step = step;
  if (margin >= 0.0f) c.margin = margin;
  c.miss_depth = miss_depth < 0.0f ? far : miss_depth;
  ViewGainResult r;
  r.rows = cam.img_h, r.cols = cam.img_w;
  r.gain.assign(views.size(), 0);
  std::vector<tsdf_pose> poses;
  poses.reserve(views.size());
  for (const SE3<float>& v : views) poses.push_back(to_pose(v));
  if (want_depth) r.depth.resize(views.size() * (size_t)std::max(cam.img_w, 0) * (size_t)std::max(cam.img_h, 0));
  check_tsdf(tsdf_view_gain(engine_, &c, field.state.data(), seen ? seen->bits.data() : nullptr, poses.data(),
                            (int32_t)views.size(), r.gain.data(), want_depth && !r.depth.empty() ? r.depth.data() : nullptr,
                            TSDF_MEM_HOST),
             "tsdf_view_gain");
  return r;
}

SurfaceMaps TSDFGrid::RayCastSurface(float max_depth, const CameraParams& cam, const SE3<float>& cam_T_world) {
  if (group_) throw std::runtime_error("TSDFGrid::RayCastSurface: not available on a sharded volume");
  SurfaceMaps m;
  m.rows = cam.img_h;
  m.cols = cam.img_w;
  const size_t n = (size_t)cam.img_h * cam.img_w;
  m.point.resize(n * 3);
  m.normal.resize(n * 3);
  m.depth.resize(n);
  m.prob.resize(n);
  m.rgbw.resize(n * 4);
  const tsdf_surface_out out{m.point.data(), m.normal.data(), m.depth.data(), m.prob.data(), m.rgbw.data(),
                             TSDF_MEM_HOST};
  const tsdf_intrinsics K{cam.intrinsics.fx, cam.intrinsics.fy, cam.intrinsics.cx, cam.intrinsics.cy};
  const tsdf_pose P = to_pose(cam_T_world);
  check_tsdf(tsdf_raycast_surface(engine_, &K, cam.img_w, cam.img_h, &P, max_depth, &out), "tsdf_raycast_surface");
  return m;
}

TrackResult TSDFGrid::Track(const Mat& img_depth, float max_depth, const CameraIntrinsics<float>& intrinsics,
                            const SE3<float>& guess, const tsdf_track_config* cfg) {
  if (group_) throw std::runtime_error("TSDFGrid::Track: not available on a sharded volume");
  if (img_depth.empty() || img_depth.type() != CV_32FC1)
    throw std::invalid_argument("TSDFGrid::Track: expects a CV_32FC1 depth image");
  const tsdf_intrinsics K{intrinsics.fx, intrinsics.fy, intrinsics.cx, intrinsics.cy};
  const tsdf_pose G = to_pose(guess);
  tsdf_track_result r;
  check_tsdf(tsdf_track(engine_, img_depth.ptr<float>(), img_depth.cols, img_depth.rows, TSDF_MEM_HOST, &K, &G,
                        max_depth, cfg, &r),
             "tsdf_track");
  const tsdf_pose& p = r.cam_T_world;
  TrackResult out;
  out.pose = SE3<float>(p.qx, p.qy, p.qz, p.qw, p.tx, p.ty, p.tz);
  out.degenerate = r.status != TSDF_TRACK_OK;
  out.iterations = r.iterations;
  out.inliers = r.inliers;
  out.rmse = r.rmse;
  return out;
}

void TSDFGrid::HalfRGBD(const Mat& img_rgb, const Mat& img_depth_raw, const Mat& mask, float depth_factor,
                        Mat* rgb_out, Mat* depth_out) {
  if (img_rgb.type() != CV_8UC3 || img_depth_raw.type() != CV_16UC1 || img_rgb.cols != img_depth_raw.cols ||
      img_rgb.rows != img_depth_raw.rows || !rgb_out || !depth_out ||
      (!mask.empty() && (mask.type() != CV_8UC1 || mask.total() != img_depth_raw.total())))
    throw std::invalid_argument("TSDFGrid::HalfRGBD: expects CV_8UC3 rgb, CV_16UC1 depth, CV_8UC1 mask");
  if (group_) throw std::runtime_error("TSDFGrid::HalfRGBD: not available on a sharded volume");
  *rgb_out = Mat(img_rgb.rows / 2, img_rgb.cols / 2, CV_8UC3);
  *depth_out = Mat(img_rgb.rows / 2, img_rgb.cols / 2, CV_32FC1);
  check_tsdf(tsdf_rgbd_half(engine_, img_rgb.ptr<uint8_t>(), img_depth_raw.ptr<uint16_t>(),
                            mask.empty() ? nullptr : mask.ptr<uint8_t>(), img_depth_raw.cols, img_depth_raw.rows,
                            depth_factor, rgb_out->ptr<uint8_t>(), depth_out->ptr<float>(), TSDF_MEM_HOST),
             "tsdf_rgbd_half");
}

tsdf_stats TSDFGrid::Stats(bool clear_status) {
  tsdf_stats s;
  if (group_)
    check_tsdf(tsdf_group_get_stats(group_, &s, clear_status ? 1 : 0), "tsdf_group_get_stats");
  else
    check_tsdf(tsdf_get_stats(engine_, &s, clear_status ? 1 : 0), "tsdf_get_stats");
  return s;
}

}  // namespace disinfect
