// tsdf_host_track.hip -- pose tracking (DESIGN.md "Pose tracking"; kernels in tsdf_track.hip, host
// math in tsdf_track_host.h): tsdf_raycast_surface, tsdf_icp_linearize, tsdf_point_map_normals, tsdf_track.
#include <cmath>
#include <string>

#include "tsdf_host.h"
#include "tsdf_track_host.h"

bool track_refused(const tsdf_engine* e, const char* what) {
  if (e->cfg.shard_count <= 1) return false;
  set_error((std::string(what) + ": not available on a shard engine (shard_count > 1)").c_str());
  return true;
}

namespace {

// the surface maps S (device) of camera (K, W x H, pose): view grid and k_raycast_surface on the
// engine stream (after ENTER)
int surface_launch(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose, float max_depth,
                   const SurfaceOut& S) {
  const FrameParams P = make_params(e, K, W, H, pose, max_depth);
  const float step = e->cfg.truncation / 2;
  ViewGrid V;
  int rc = view_grid_for(e, P, step, kViewBitmapWords, &V);
  if (rc) return rc;
  if (V.n) {
    hipLaunchKernelGGL(k_view_grid, dim3(kOccWords / 256), dim3(256), 0, e->stream, e->D, P, V);
    hipLaunchKernelGGL(k_view_pack, dim3(kViewPackGrid), dim3(256), 0, e->stream, V);
    LAUNCH_OK("k_view_grid");
  }
  const dim3 grid((W + 15) / 16, (H + 15) / 16);
  hipLaunchKernelGGL(k_raycast_surface, grid, dim3(256), V.n ? (size_t)V.nw * 4 : 0, e->stream, e->D, P, step, V, S);
  LAUNCH_OK("k_raycast_surface");
  return TSDF_OK;
}

// tsdf_track's model normals `out` from the device maps of camera (K, W x H, pose): k_surface_normals on
// the engine stream (the kernel reads wt and the size of the camera alone)
int normals_launch(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose, float max_depth,
                   const float* point, const float* normal, float* out) {
  hipLaunchKernelGGL(k_surface_normals, dim3((W + 15) / 16, (H + 15) / 16), dim3(256), 0, e->stream,
                     make_params(e, K, W, H, pose, max_depth), point, normal, out);
  LAUNCH_OK("k_surface_normals");
  return TSDF_OK;
}

// one linearisation of device maps: the two launches and the read of the 29 sums (232 bytes)
int icp_launch(tsdf_engine* e, const float* depth, int W, int H, const tsdf_intrinsics* K, const tsdf_pose* pose,
               const float* point, const float* normal, int Wm, int Hm, const tsdf_intrinsics* Km,
               const tsdf_pose* pose_m, int stride, float max_dist, float max_depth, double* out29) {
  IcpParams I{};
  I.F = make_params(e, K, W, H, pose, max_depth);
  I.M = make_params(e, Km, Wm, Hm, pose_m, max_depth);
  I.depth = depth;
  I.point = point;
  I.normal = normal;
  I.stride = stride;
  I.nsx = (W + stride - 1) / stride;
  I.nsamples = I.nsx * ((H + stride - 1) / stride);
  I.max_dist2 = max_dist * max_dist;
  const int nwg = (I.nsamples + 255) / 256;
  if (int rc = e->tk_part.ensure(((size_t)nwg + 1) * kIcpSums, "icp: hipMalloc tk_part")) return rc;
  double* total = e->tk_part + (e->tk_part.cap - kIcpSums);  // after the sums of as many workgroups as fit
  hipLaunchKernelGGL(k_icp_partial, dim3(nwg), dim3(256), 0, e->stream, I, e->tk_part);
  hipLaunchKernelGGL(k_icp_final, dim3(1), dim3(1024), 0, e->stream, (const double*)e->tk_part, nwg, total);
  LAUNCH_OK("k_icp_partial");
  HIP_OK(hipMemcpyAsync(out29, total, sizeof(double) * kIcpSums, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

}  // namespace

int tsdf_raycast_surface(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                         float max_depth, const tsdf_surface_out* out) {
  TraceRange trace_("tsdf_raycast_surface");
  if (!e || !frame_args_ok(e, K, pose, W, H) || !out || !out->point || !out->normal || !mem_kind_ok(out->mem_kind) ||
      (reinterpret_cast<uintptr_t>(out->rgbw) & 3) != 0) {
    set_error("tsdf_raycast_surface: invalid argument (point and normal are required; rgbw 4-byte aligned)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_raycast_surface")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (out->mem_kind == TSDF_MEM_DEVICE)
    return surface_launch(e, K, W, H, pose, max_depth,
                          SurfaceOut{out->point, out->normal, out->depth, out->prob, reinterpret_cast<uint32_t*>(out->rgbw)});
  // host maps: a staging buffer (sections 16-byte aligned), copied out per map
  const size_t n = (size_t)W * H;
  Sections L;  // (every map has its section, asked for or not)
  const int h_pt = L.add(n * 12), h_nrm = L.add(n * 12), h_dep = L.add(n * 4), h_prob = L.add(n * 4), h_rgbw = L.add(n * 4);
  int rc = track_stage(e, L.total());
  if (rc) return rc;
  uint8_t* b = e->tk_stage;
  const SurfaceOut S{L.at<float>(b, h_pt), L.at<float>(b, h_nrm), out->depth ? L.at<float>(b, h_dep) : nullptr,
                     out->prob ? L.at<float>(b, h_prob) : nullptr, out->rgbw ? L.at<uint32_t>(b, h_rgbw) : nullptr};
  rc = surface_launch(e, K, W, H, pose, max_depth, S);
  if (rc) return rc;
  hipStream_t s = e->stream;
  HIP_OK(hipMemcpyAsync(out->point, S.point, n * 12, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->normal, S.normal, n * 12, hipMemcpyDeviceToHost, s));
  if (out->depth) HIP_OK(hipMemcpyAsync(out->depth, S.depth, n * 4, hipMemcpyDeviceToHost, s));
  if (out->prob) HIP_OK(hipMemcpyAsync(out->prob, S.prob, n * 4, hipMemcpyDeviceToHost, s));
  if (out->rgbw) HIP_OK(hipMemcpyAsync(out->rgbw, S.rgbw, n * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_icp_linearize(tsdf_engine* e, const float* depth, int W, int H, const tsdf_intrinsics* K,
                       const tsdf_pose* pose, const tsdf_icp_model* model, int stride, float max_dist,
                       float max_depth, double* out29, int mem_kind) {
  TraceRange trace_("tsdf_icp_linearize");
  if (!e || !depth || !frame_args_ok(e, K, pose, W, H) || !model || !model->point || !model->normal ||
      !frame_args_ok(e, &model->K, &model->cam_T_world, model->width, model->height) || stride < 1 ||
      !(max_dist >= 0.0f) || !out29 || !mem_kind_ok(mem_kind)) {
    set_error("tsdf_icp_linearize: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_icp_linearize")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const float *d = depth, *pt = model->point, *nr = model->normal;
  if (mem_kind == TSDF_MEM_HOST) {
    const size_t n = (size_t)W * H, nm = (size_t)model->width * model->height;
    Sections L;
    const int h_d = L.add(n * 4), h_pt = L.add(nm * 12), h_nr = L.add(nm * 12);
    int rc = track_stage(e, L.total());
    if (rc) return rc;
    uint8_t* b = e->tk_stage;
    float *sd = L.at<float>(b, h_d), *spt = L.at<float>(b, h_pt), *snr = L.at<float>(b, h_nr);
    HIP_OK(hipMemcpyAsync(sd, depth, n * 4, hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipMemcpyAsync(spt, model->point, nm * 12, hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipMemcpyAsync(snr, model->normal, nm * 12, hipMemcpyHostToDevice, e->stream));
    d = sd, pt = spt, nr = snr;
  }
  return icp_launch(e, d, W, H, K, pose, pt, nr, model->width, model->height, &model->K, &model->cam_T_world, stride,
                    max_dist, max_depth, out29);
}

int tsdf_point_map_normals(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                           const float* point, const float* normal, float* out, int mem_kind) {
  TraceRange trace_("tsdf_point_map_normals");
  if (!e || !frame_args_ok(e, K, pose, W, H) || !point || !normal || !out || !mem_kind_ok(mem_kind)) {
    set_error("tsdf_point_map_normals: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_point_map_normals")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const float max_depth = 1.0f;  // not read by the kernel
  if (mem_kind == TSDF_MEM_DEVICE) return normals_launch(e, K, W, H, pose, max_depth, point, normal, out);
  // host maps: staged (sections 16-byte aligned), the result copied out
  const size_t n = (size_t)W * H;
  Sections L;
  const int h_pt = L.add(n * 12), h_nr = L.add(n * 12), h_out = L.add(n * 12);
  int rc = track_stage(e, L.total());
  if (rc) return rc;
  uint8_t* b = e->tk_stage;
  HIP_OK(hipMemcpyAsync(L.at<float>(b, h_pt), point, n * 12, hipMemcpyHostToDevice, e->stream));
  HIP_OK(hipMemcpyAsync(L.at<float>(b, h_nr), normal, n * 12, hipMemcpyHostToDevice, e->stream));
  rc = normals_launch(e, K, W, H, pose, max_depth, L.at<float>(b, h_pt), L.at<float>(b, h_nr), L.at<float>(b, h_out));
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(out, L.at<float>(b, h_out), n * 12, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

void tsdf_track_config_default(tsdf_track_config* c) {
  if (!c) return;
  *c = tsdf_track_config{};
  c->levels = 3;
  const int stride[3] = {4, 2, 1}, iterations[3] = {4, 5, 10};  // KinectFusion's schedule
  for (int l = 0; l < 3; ++l) c->stride[l] = stride[l], c->iterations[l] = iterations[l];
  c->max_dist = 0.1f;
  c->eps_rot = 0.0f;
  c->eps_trans = 0.0f;
  c->min_inliers = 6;
}

int tsdf_track(tsdf_engine* e, const float* depth, int W, int H, int mem_kind, const tsdf_intrinsics* K,
               const tsdf_pose* guess, float max_depth, const tsdf_track_config* cfg, tsdf_track_result* out) {
  TraceRange trace_("tsdf_track");
  tsdf_track_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_track_config_default(&c);
  bool ok = e && depth && frame_args_ok(e, K, guess, W, H) && out && mem_kind_ok(mem_kind) && c.levels >= 1 &&
            c.levels <= 3 && c.max_dist >= 0.0f;
  for (int l = 0; ok && l < c.levels; ++l) ok = c.stride[l] >= 1 && c.iterations[l] >= 0;
  if (!ok) {
    set_error("tsdf_track: invalid argument (levels 1..3, stride >= 1, iterations >= 0, max_dist >= 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_track")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const size_t n = (size_t)W * H;
  if (n * 3 > e->tk_pnormal.cap) {  // the model maps: resized when the frame size grows
    release_all(e->tk_point, e->tk_normal, e->tk_pnormal);
    int rc = e->tk_point.ensure(n * 3, "tsdf_track: hipMalloc tk_point");
    if (!rc) rc = e->tk_normal.ensure(n * 3, "tsdf_track: hipMalloc tk_normal");
    if (!rc) rc = e->tk_pnormal.ensure(n * 3, "tsdf_track: hipMalloc tk_pnormal");
    if (rc) return rc;
  }
  const float* d = depth;
  if (mem_kind == TSDF_MEM_HOST) {
    int rc = track_stage(e, n * 4);
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(e->tk_stage, depth, n * 4, hipMemcpyHostToDevice, e->stream));
    d = reinterpret_cast<const float*>(e->tk_stage.p);
  }
  int rc = surface_launch(e, K, W, H, guess, max_depth, SurfaceOut{e->tk_point, e->tk_normal, nullptr, nullptr, nullptr});
  if (rc) return rc;
  // the normals the loop uses come from the model's points (k_surface_normals: why)
  rc = normals_launch(e, K, W, H, guess, max_depth, e->tk_point, e->tk_normal, e->tk_pnormal);
  if (rc) return rc;
  tsdf_pose est = *guess;
  tsdf_track_result r{};
  r.status = TSDF_TRACK_OK;
  const bool early = c.eps_rot > 0.0f || c.eps_trans > 0.0f;
  for (int l = 0; l < c.levels && r.status == TSDF_TRACK_OK; ++l) {
    for (int it = 0; it < c.iterations[l]; ++it) {
      double s[kIcpSums];
      rc = icp_launch(e, d, W, H, K, &est, e->tk_point, e->tk_pnormal, W, H, K, guess, c.stride[l], c.max_dist,
                      max_depth, s);
      if (rc) return rc;
      r.inliers = (int32_t)s[28];
      r.rmse = s[28] > 0.0 ? (float)std::sqrt(s[27] / s[28]) : 0.0f;
      double xi[6], rhs[6];
      for (int i = 0; i < 6; ++i) rhs[i] = -s[21 + i];
      if (r.inliers < c.min_inliers || !track_host::solve_spd6(s, rhs, xi)) {
        r.status = TSDF_TRACK_DEGENERATE;  // the last good estimate stands
        break;
      }
      double R_wc[9], p_wc[3];
      const float q[4] = {est.qx, est.qy, est.qz, est.qw}, t[3] = {est.tx, est.ty, est.tz};
      float q2[4], t2[3];
      track_host::pose_to_world(q, t, R_wc, p_wc);
      track_host::apply_twist(xi, R_wc, p_wc);
      track_host::world_to_pose(R_wc, p_wc, q2, t2);
      bool finite = true;
      for (float v : q2) finite = finite && std::isfinite(v);
      for (float v : t2) finite = finite && std::isfinite(v);
      if (!finite) {
        r.status = TSDF_TRACK_DEGENERATE;
        break;
      }
      est = tsdf_pose{q2[0], q2[1], q2[2], q2[3], t2[0], t2[1], t2[2]};
      r.iterations += 1;
      if (early && std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) <= (double)c.eps_rot &&
          std::sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]) <= (double)c.eps_trans)
        break;
    }
  }
  r.cam_T_world = est;
  *out = r;
  return TSDF_OK;
}
