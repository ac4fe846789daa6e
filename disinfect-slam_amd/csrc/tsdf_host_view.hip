// tsdf_host_view.hip -- view gain (DESIGN.md "View gain"; kernels in tsdf_view.hip): tsdf_view_config_default
// and tsdf_view_gain.
#include <cmath>
#include <vector>

#include "tsdf_host.h"
#include "tsdf_view.h"

static_assert(TSDF_VIEW_BATCH == tsdf::kViewBatch && TSDF_VIEW_BATCH_PIXELS == tsdf::kViewBatchPixels,
              "the kernels' constants");

void tsdf_view_config_default(const tsdf_engine* e, tsdf_view_config* c) {
  if (!c) return;
  *c = tsdf_view_config{};
  c->far = 3.0f;
  c->miss_depth = c->far;
  if (e) {
    c->step = e->cfg.voxel_size;
    c->margin = e->cfg.truncation;
  }
}

namespace {

constexpr int kViewMaxViews = 4096, kViewMaxSamples = 65536;
constexpr int64_t kViewMaxPixels = (int64_t)1 << 26;  // V * W * H

}  // namespace

int tsdf_view_gain(tsdf_engine* e, const tsdf_view_config* cfg, const uint8_t* state, const uint32_t* seen,
                   const tsdf_pose* views, int32_t V, int64_t* gain, float* depth_out, int mem_kind) {
  TraceRange trace_("tsdf_view_gain");
  bool ok = e && cfg && state && mem_kind_ok(mem_kind) && V >= 0 && V <= kViewMaxViews && (V == 0 || (views && gain));
  int J = 0;
  if (ok) {
    ok = box_dims_ok(cfg->dims) && box_in_block_range(cfg->origin, cfg->dims, 0) && cfg->width >= 1 && cfg->width <= e->cfg.max_width && cfg->height >= 1 &&
         cfg->height <= e->cfg.max_height && (int64_t)V * cfg->width * cfg->height <= kViewMaxPixels &&
         std::isfinite(cfg->far) && cfg->far > 0.0f && std::isfinite(cfg->step) && cfg->step > 0.0f &&
         std::isfinite(cfg->margin) && cfg->margin >= 0.0f && std::isfinite(cfg->miss_depth) &&
         cfg->miss_depth >= 0.0f && cfg->miss_depth <= cfg->far;
    if (ok) {
      // f2i(far / step): truncation with saturation (the quotient is positive, or +inf)
      const float q = cfg->far / cfg->step;
      J = q >= 2147483648.0f ? 0x7FFFFFFF : (int)q;
      ok = J >= 1 && J <= kViewMaxSamples;
    }
  }
  if (!ok) {
    set_error("tsdf_view_gain: invalid argument (" BOX_LIMITS_TEXT ", the box inside the block range, "
              "width and height 1..the engine's, V 0..4096, V * width * height <= 2^26, far and step > 0 with "
              "1 <= far / step <= 65536, margin >= 0, miss_depth 0..far, all finite, cfg and state non-NULL, views "
              "and gain with V > 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (V == 0) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const int W = cfg->width, H = cfg->height;
  const size_t npix = (size_t)W * H;
  const size_t n = box_voxels(cfg->dims), words = (size_t)box_words(cfg->dims);
  const int batch = (int)std::min<int64_t>(kViewBatch, std::max<int64_t>(1, kViewBatchPixels / (int64_t)npix));
  const bool host = mem_kind == TSDF_MEM_HOST;
  // the views as the kernels take them: make_params' world_T_cam, and the brick culls' rule for a rigid motion
  std::vector<ViewCam> cams((size_t)V);
  FrameParams P0{};
  for (int i = 0; i < V; ++i) {
    const FrameParams P = make_params(e, &cfg->K, W, H, &views[i], cfg->far);
    if (i == 0) P0 = P;
    ViewCam& c = cams[(size_t)i];
    c.cq = P.cq, c.ct = P.ct, c.wq = P.wq, c.wt = P.wt;
    c.dmax_bits = 0;
    const float q[4] = {P.cq.x, P.cq.y, P.cq.z, P.cq.w};
    c.rigid = pose_is_rigid(q) ? 1 : 0;
  }
  // sections: views | gains | a batch's pixel records | host arrays' staging: state, seen, a batch's depth
  Sections L;
  const int h_cam = L.add((size_t)V * sizeof(ViewCam)), h_gain = L.add((size_t)V * 8),
            h_pix = L.add((size_t)batch * npix * sizeof(FreePix)), h_state = L.add(staged(host, state, n)),
            h_seen = L.add(staged(host, seen, 4 * words)), h_depth = L.add(staged(host, depth_out, (size_t)batch * npix * 4));
  int rc = e->vw_buf.ensure(L.total(), "tsdf_view_gain: hipMalloc vw_buf");
  if (rc) return rc;
  const Stage St{L, e->vw_buf.p, host, s};
  ViewCam* dcam = L.at<ViewCam>(St.base, h_cam);
  unsigned long long* dgain = L.at<unsigned long long>(St.base, h_gain);
  FreePix* dpix = L.at<FreePix>(St.base, h_pix);
  float* ddepth = St.ptr(h_depth, depth_out);  // (a host call's: a batch's staging)
  HIP_OK(hipMemcpyAsync(dcam, cams.data(), (size_t)V * sizeof(ViewCam), hipMemcpyHostToDevice, s));
  HIP_OK(hipMemsetAsync(dgain, 0, (size_t)V * 8, s));
  ViewDepthArgs D{};
  D.ox = cfg->origin[0], D.oy = cfg->origin[1], D.oz = cfg->origin[2];
  D.nx = cfg->dims[0], D.ny = cfg->dims[1], D.nz = cfg->dims[2];
  D.W = W, D.H = H;
  D.ifx = P0.ifx, D.ify = P0.ify, D.icx = P0.icx, D.icy = P0.icy;
  D.voxel = P0.voxel, D.inv_voxel = P0.inv_voxel;
  D.step = cfg->step, D.miss = cfg->miss_depth;
  D.J = J;
  D.skip = e->env.view_skip ? 1 : 0;
  HIP_OK(St.in(h_state, state, n, &D.state));
  D.pix = dpix;
  ViewGainArgs G{};
  G.ox = D.ox, G.oy = D.oy, G.oz = D.oz;
  G.nx = D.nx, G.ny = D.ny, G.nz = D.nz;
  G.wx = (G.nx + 31) >> 5;
  G.W = W, G.H = H;
  G.fx = P0.fx, G.fy = P0.fy, G.cx = P0.cx, G.cy = P0.cy;
  G.voxel = P0.voxel, G.margin = cfg->margin;
  G.cull = e->env.view_skip ? 1 : 0;
  G.state = D.state;
  HIP_OK(St.in(h_seen, seen, 4 * words, &G.seen));
  G.pix = dpix;
  const dim3 bricks = free_brick_grid(G.nx, G.ny, G.nz);
  for (int v0 = 0; v0 < V; v0 += batch) {
    const int nv = std::min(batch, V - v0);
    D.cam = dcam + v0;
    D.depth_out = depth_out ? (host ? ddepth : depth_out + (size_t)v0 * npix) : nullptr;
    hipLaunchKernelGGL(k_view_depth, dim3((unsigned)((npix + 255) / 256), (unsigned)nv), dim3(256), 0, s, D);
    LAUNCH_OK("k_view_depth");
    G.nv = nv;
    G.cam = dcam + v0;
    G.gain = dgain + v0;
    hipLaunchKernelGGL(k_view_gain, bricks, dim3(256), 0, s, G);
    LAUNCH_OK("k_view_gain");
    // (the next batch's march overwrites the staging: the stream orders this copy before it)
    if (host && depth_out)
      HIP_OK(hipMemcpyAsync(depth_out + (size_t)v0 * npix, ddepth, (size_t)nv * npix * 4, hipMemcpyDeviceToHost, s));
  }
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters are the gains");
  HIP_OK(hipMemcpyAsync(gain, dgain, (size_t)V * 8, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}
