// tsdf_host_render.hip -- reading the volume out: the raycast view grid, tsdf_rgbd_half /
// tsdf_feed_rgbd_frame, the raycast family, tsdf_query, tsdf_reset, and the block records (render /
// pack / import, bands, halo).
#include <cmath>
#include <vector>

#include "tsdf_host.h"

// The view grid of one raycast of camera P (tsdf_kernels.h ViewGrid). Its cube reaches every voxel
// a ray can read: positions up to max_step * step_size / voxel grid units from the camera centre
// (|direction| = 1 up to rounding), plus the binary search, the +-1 gradient neighbours and the
// rounding to the nearest voxel (2.5 voxels). n = 0 (hash lookups) when the cube would exceed
// kViewMaxN cells per axis, the brick bitmap `lds_words` of LDS, or the pool a cell's index bits.
// (ViewShape: the cube of `half` blocks on every side of its centre block)
void view_shape_half(const tsdf_engine* e, int half, int lds_words, ViewShape* out) {
  ViewShape& S = *out;
  S = ViewShape{};
  S.half = half;
  S.n = 2 * S.half + 1;
  S.nb = (S.n + 3) / 4;
  S.ns = (S.nb + 3) / 4;
  S.nbw = (S.nb * S.nb * S.nb + 31) / 32;
  S.nw = S.nbw + (S.ns * S.ns * S.ns + 31) / 32;
  S.cells = (int64_t)S.nb * S.nb * S.nb * 64;
  S.ok = S.n <= kViewMaxN && S.nw <= lds_words && e->D.nblocks <= (1 << kViewIdxBits);
}
static void view_shape(const tsdf_engine* e, const FrameParams& P, float step_size, int lds_words, ViewShape* out) {
  *out = ViewShape{};
  const double max_step = std::ceil((double)P.max_depth / (double)step_size);
  const double reach = max_step * (double)step_size / (double)P.voxel * (1.0 + 1e-5) + 2.5;
  if (!(reach < 1e6)) return;
  view_shape_half(e, (int)std::ceil(reach / kBlockLen) + 1, lds_words, out);
}
// whether view_grid_for(P) would clear or reallocate the grid's cells (a deferred raycast reading the
// previous grid must run first): the same shape and the same two conditions view_grid_for acts on
bool view_grid_resets(const tsdf_engine* e, const FrameParams& P, float step_size, int lds_words) {
  ViewShape S;
  view_shape(e, P, step_size, lds_words, &S);
  return S.ok && ((size_t)S.cells > e->vg_cell.cap || e->vg_gen == kViewGenMax);
}

// the engine's grid with shape S (S.ok), under a new generation
int view_grid_take(tsdf_engine* e, const ViewShape& S, ViewGrid* V) {
  *V = ViewGrid{};
  V->flags = e->vg_flags;
  V->bits = e->vg_bits;
  if (!S.ok) return TSDF_OK;
  const int n = S.n, nb = S.nb, ns = S.ns, nbw = S.nbw, nw = S.nw, half = S.half;
  if ((size_t)S.cells > e->vg_cell.cap) {
    int rc = e->vg_cell.ensure((size_t)S.cells, "view grid: hipMalloc vg_cell");
    if (rc) return rc;
    e->vg_gen = kViewGenMax;  // new cells: cleared like exhausted generations
  }
  if (e->vg_gen == kViewGenMax) {  // generations exhausted: stale cells must not match gen 1 again
    HIP_OK(hipMemsetAsync(e->vg_cell, 0, e->vg_cell.cap * 4, e->stream));
    e->vg_gen = 0;
  }
  e->vg_gen += 1;
  e->vg_calls += 1;
  V->cell = e->vg_cell;
  V->n = n;
  V->nb = nb;
  V->ns = ns;
  V->nbw = nbw;
  V->nw = nw;
  V->half = half;
  V->gen = e->vg_gen;
  return TSDF_OK;
}
int view_grid_for(tsdf_engine* e, const FrameParams& P, float step_size, int lds_words, ViewGrid* V) {
  ViewShape S;
  view_shape(e, P, step_size, lds_words, &S);
  return view_grid_take(e, S, V);
}

namespace {

// cv::resize x0.5 + convertTo + mask (k_rgbd_half) of a W x H frame into device rgb_out / depth_out
int rgbd_half(tsdf_engine* e, const uint8_t* rgb, const uint16_t* depth, const uint8_t* mask, int W,
              int H, float depth_factor, uint8_t* rgb_out, float* depth_out, int mem_kind) {
  hipStream_t s = e->stream;
  const size_t np = (size_t)W * H;
  if (mem_kind == TSDF_MEM_HOST) {
    if (np > e->fe_mask.cap) {
      release_all(e->fe_rgb, e->fe_depth, e->fe_mask);
      int rc = e->fe_rgb.ensure(np * 3, "rgbd_half: hipMalloc fe_rgb");
      if (!rc) rc = e->fe_depth.ensure(np, "rgbd_half: hipMalloc fe_depth");
      if (!rc) rc = e->fe_mask.ensure(np, "rgbd_half: hipMalloc fe_mask");
      if (rc) return rc;
    }
    HIP_OK(hipMemcpyAsync(e->fe_rgb, rgb, np * 3, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(e->fe_depth, depth, np * 2, hipMemcpyHostToDevice, s));
    if (mask) HIP_OK(hipMemcpyAsync(e->fe_mask, mask, np, hipMemcpyHostToDevice, s));
    rgb = e->fe_rgb;
    depth = e->fe_depth;
    mask = mask ? e->fe_mask.p : nullptr;
  }
  const float alpha = (float)(1. / (double)depth_factor);  // convertTo(CV_32FC1, 1. / factor)
  const int w = W / 2, h = H / 2;
  hipLaunchKernelGGL(k_rgbd_half, dim3((w + 63) / 64, (h + 3) / 4), dim3(256), 0, s, rgb, depth, mask,
                     W, H, alpha, rgb_out, depth_out);
  LAUNCH_OK("k_rgbd_half");
  return TSDF_OK;
}

bool rgbd_args_ok(const uint8_t* rgb, const uint16_t* depth, int W, int H, float depth_factor,
                  int mem_kind) {
  return rgb && depth && W >= 2 && H >= 2 && W % 2 == 0 && H % 2 == 0 && depth_factor > 0.0f &&
         (mem_kind == TSDF_MEM_HOST || mem_kind == TSDF_MEM_DEVICE);
}

int ensure_fe_out(tsdf_engine* e, int64_t npix) {
  if ((size_t)npix <= e->fe_out_depth.cap) return TSDF_OK;
  release_all(e->fe_out_rgb, e->fe_out_depth);
  int rc = e->fe_out_rgb.ensure((size_t)npix * 3, "rgbd_half: hipMalloc fe_out_rgb");
  if (!rc) rc = e->fe_out_depth.ensure((size_t)npix, "rgbd_half: hipMalloc fe_out_depth");
  return rc;
}

}  // namespace

int tsdf_rgbd_half(tsdf_engine* e, const uint8_t* rgb, const uint16_t* depth, const uint8_t* mask,
                   int width, int height, float depth_factor, uint8_t* rgb_out, float* depth_out,
                   int mem_kind) {
  if (!e || !rgbd_args_ok(rgb, depth, width, height, depth_factor, mem_kind) || !rgb_out || !depth_out) {
    set_error("tsdf_rgbd_half: invalid argument (even width / height, depth_factor > 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  JOIN_RENDER(e);
  const int64_t nout = (int64_t)(width / 2) * (height / 2);
  if (mem_kind == TSDF_MEM_DEVICE)
    return rgbd_half(e, rgb, depth, mask, width, height, depth_factor, rgb_out, depth_out, mem_kind);
  int rc = ensure_fe_out(e, nout);
  if (rc) return rc;
  rc = rgbd_half(e, rgb, depth, mask, width, height, depth_factor, e->fe_out_rgb, e->fe_out_depth, mem_kind);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(rgb_out, e->fe_out_rgb, (size_t)nout * 3, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipMemcpyAsync(depth_out, e->fe_out_depth, (size_t)nout * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_feed_rgbd_frame(tsdf_engine* e, const uint8_t* rgb, const uint16_t* depth,
                         const uint8_t* mask, int width, int height, float depth_factor,
                         const tsdf_intrinsics* K, const tsdf_pose* cam_T_world, float max_depth,
                         int mem_kind) {
  TraceRange trace_("tsdf_feed_rgbd_frame");
  if (!e || !rgbd_args_ok(rgb, depth, width, height, depth_factor, mem_kind)) {
    set_error("tsdf_feed_rgbd_frame: invalid argument (even width / height, depth_factor > 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  JOIN_RENDER(e);
  const int w = width / 2, h = height / 2;
  int rc = ensure_fe_out(e, (int64_t)w * h);
  if (rc) return rc;
  rc = rgbd_half(e, rgb, depth, mask, width, height, depth_factor, e->fe_out_rgb, e->fe_out_depth, mem_kind);
  if (rc) return rc;
  // TSDFSystem::Integrate without ht / lt (disinfect_slam.cc:66; ones, tsdf_module.cc:29-33)
  tsdf_frame f{};
  f.width = w;
  f.height = h;
  f.rgb = e->fe_out_rgb;
  f.depth = e->fe_out_depth;
  f.ht = nullptr;
  f.lt = nullptr;
  f.mem_kind = TSDF_MEM_DEVICE;
  return tsdf_integrate(e, &f, K, cam_T_world, max_depth);
}


namespace {
int raycast_impl(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                 float max_depth, int row0, int nrows, uint8_t* rgba, uint8_t* normal, int mem_kind,
                 bool deferred = false) {
  if (!e || !K || !pose || W <= 0 || H <= 0 || (int64_t)W * H > e->max_pixels || row0 < 0 || nrows < 1 ||
      row0 + nrows > H || (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE)) {
    set_error("tsdf_raycast: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  FrameParams P = make_params(e, K, W, H, pose, max_depth);
  P.row0 = row0;
  P.nrows = nrows;
  uchar4* o1 = mem_kind == TSDF_MEM_DEVICE ? reinterpret_cast<uchar4*>(rgba) : (rgba ? e->rc_rgba.p : nullptr);
  uchar4* o2 = mem_kind == TSDF_MEM_DEVICE ? reinterpret_cast<uchar4*>(normal) : (normal ? e->rc_norm.p : nullptr);
  const float step = e->cfg.truncation / 2;
  ViewGrid V;
  int rc;
  // The C5 loop (a deferred raycast while the frame's unpipelined update is still pending): that
  // update's launch builds the view grid too (k_integrate_vg), one launch and boundary fewer
  bool fused = false;
  if (deferred && mem_kind == TSDF_MEM_DEVICE && e->ps == tsdf_engine::kPipeU && !sharded(e) &&
      e->p_P.pack_pixels) {
    JOIN_RENDER(e);  // (a deferred raycast still pending reads the previous grid)
    rc = view_grid_for(e, P, step, kViewGraphBitmapWords, &V);
    if (rc) return rc;
    if (V.n) {
      rc = update_with_grid(e, P, V);
      if (rc) return rc;
      fused = true;
    }
  }
  if (!fused) {
    ENTER(e);
    rc = view_grid_for(e, P, step, kViewBitmapWords, &V);
    if (rc) return rc;
    if (V.n) {
      hipLaunchKernelGGL(k_view_grid, dim3(kOccWords / 256), dim3(256), 0, e->stream, e->D, P, V);
      LAUNCH_OK("k_view_grid");
    }
  }
  if (V.n) {
    hipLaunchKernelGGL(k_view_pack, dim3(kViewPackGrid), dim3(256), 0, e->stream, V);
    LAUNCH_OK("k_view_pack");
  }
  if (deferred && V.n && V.nw <= kViewGraphBitmapWords && mem_kind == TSDF_MEM_DEVICE) {
    // (tsdf_raycast_deferred: the launch waits for the next call, join_render / frame_ingest)
    e->rd.pending = true;
    e->rd.P = P;
    e->rd.V = V;
    e->rd.step = step;
    e->rd.rgba = o1;
    e->rd.normal = o2;
    return TSDF_OK;
  }
  const size_t lds = V.n ? (size_t)V.nw * 4 : 0;
  const dim3 rgrid((W + 15) / 16, (nrows + 15) / 16);
  hipLaunchKernelGGL(k_raycast, rgrid, dim3(256), lds, e->stream, e->D, P, step, V, o1, o2);
  LAUNCH_OK("k_raycast");
  if (mem_kind == TSDF_MEM_HOST) {
    ENTER(e);
    const size_t bytes = (size_t)W * nrows * 4;
    if (rgba) HIP_OK(hipMemcpyAsync(rgba, e->rc_rgba, bytes, hipMemcpyDeviceToHost, e->stream));
    if (normal) HIP_OK(hipMemcpyAsync(normal, e->rc_norm, bytes, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  }
  return TSDF_OK;
}
}  // namespace

int tsdf_raycast(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                 float max_depth, uint8_t* rgba, uint8_t* normal, int mem_kind) {
  TraceRange trace_("tsdf_raycast");
  return raycast_impl(e, K, W, H, pose, max_depth, 0, H, rgba, normal, mem_kind);
}

int tsdf_raycast_deferred(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                          float max_depth, uint8_t* rgba, uint8_t* normal) {
  TraceRange trace_("tsdf_raycast_deferred");
  return raycast_impl(e, K, W, H, pose, max_depth, 0, H, rgba, normal, TSDF_MEM_DEVICE, true);
}

int tsdf_raycast_rows(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                      float max_depth, int row0, int nrows, uint8_t* rgba, uint8_t* normal, int mem_kind) {
  TraceRange trace_("tsdf_raycast_rows");
  return raycast_impl(e, K, W, H, pose, max_depth, row0, nrows, rgba, normal, mem_kind);
}

int tsdf_query(tsdf_engine* e, const float* bounds, tsdf_voxel* out, int64_t capacity,
               int64_t* count) {
  TraceRange trace_("tsdf_query");
  if (!e || !count) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  short4 lo = make_short4(0, 0, 0, 0), hi = make_short4(0, 0, 0, 0);
  if (bounds) {  // BoundingCube::Scale<short>(1. / voxel_size_) (voxel_tsdf.cuh:21-26, :429)
    const float scale = (float)(1. / (double)e->cfg.voxel_size);
    lo = make_short4(h_f2s(bounds[0] * scale), h_f2s(bounds[2] * scale), h_f2s(bounds[4] * scale), 0);
    hi = make_short4(h_f2s(bounds[1] * scale), h_f2s(bounds[3] * scale), h_f2s(bounds[5] * scale), 0);
  }
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(k_query_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, bounds ? 1 : 0,
                     lo, hi);
  hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, e->D, e->q_sel,
                     e->q_count);
  LAUNCH_OK("query select");
  int32_t nsel = 0;
  HIP_OK(hipMemcpyAsync(&nsel, e->q_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const int64_t nvox = (int64_t)nsel * kBlockVolume;
  *count = nvox;
  if (!out) return TSDF_OK;
  if (capacity < nvox) {
    set_error("tsdf_query: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  if (nsel == 0) return TSDF_OK;
  if (int rc = e->q_out.ensure((size_t)nvox, "tsdf_query: hipMalloc q_out")) return rc;
  hipLaunchKernelGGL(k_query_download, dim3(nsel), dim3(kBlockVolume), 0, s, e->D, e->q_sel,
                     e->cfg.voxel_size, e->q_out);
  LAUNCH_OK("k_query_download");
  HIP_OK(hipMemcpyAsync(out, e->q_out, (size_t)nvox * sizeof(float4), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

namespace {
// the nsel blocks listed in q_sel as TSDF_BLOCK_RECORD_BYTES records into out (host or device)
int pack_selected(tsdf_engine* e, int32_t nsel, void* out, int mem_kind, const char* what) {
  hipStream_t s = e->stream;
  const size_t bytes = (size_t)nsel * kBlockRecBytes;
  uint8_t* dst = reinterpret_cast<uint8_t*>(out);
  DevBuf<uint8_t> tmp;  // (freed on return: after the synchronisation below)
  if (mem_kind == TSDF_MEM_HOST) {
    if (int rc = tmp.ensure(bytes, "block records: hipMalloc staging")) return rc;
    dst = tmp;
  }
  hipLaunchKernelGGL(k_render_pack, dim3(nsel), dim3(256), 0, s, e->D, e->q_sel, dst);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess && tmp) err = hipMemcpyAsync(out, tmp, bytes, hipMemcpyDeviceToHost, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) {
    set_error(what, err);
    return TSDF_ERR_HIP;
  }
  return TSDF_OK;
}
}  // namespace

static_assert(kBlockRecBytes == TSDF_BLOCK_RECORD_BYTES, "render record layout");

int tsdf_reset(tsdf_engine* e) {
  TraceRange trace_("tsdf_reset");
  if (!e) return TSDF_ERR_INVALID_ARG;
  if (e->shard_phase != 0) {
    set_error("tsdf_reset: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  // a shard's pending pipelined frames need the exchange protocol to complete: reset drops them
  // (init_state below re-initialises every per-frame buffer); one volume's are flushed first
  if (sharded(e)) e->ps = tsdf_engine::kPipeNone;
  ENTER(e);
  if (!init_state(e)) {
    set_error("tsdf_reset: initialisation failed");
    return TSDF_ERR_HIP;
  }
  return TSDF_OK;
}

namespace {
// the render cull of camera P (tsdf_render_blocks): the pixel-centre pyramid of rows [r0, r1) grown
// by one lookup's reach, cut at the marched length
RenderCull render_cull(const tsdf_engine* e, const FrameParams& P, int W, int r0, int r1) {
  // ray_cast_kernel's march (voxel_tsdf.cu:248-250): max_step samples truncation / 2 apart
  const double step = (double)(e->cfg.truncation / 2);
  const double max_step = std::ceil((double)P.max_depth / step);
  RenderCull C{};
  C.a0 = P.icx;
  C.a1 = (float)(W - 1) * P.ifx + P.icx;
  C.b0 = (float)r0 * P.ify + P.icy;  // the rays' own y / z slopes (pixel_ray's float operations)
  C.b1 = (float)(r1 - 1) * P.ify + P.icy;
  C.na0 = std::sqrt(1.0f + C.a0 * C.a0);
  C.na1 = std::sqrt(1.0f + C.a1 * C.a1);
  C.nb0 = std::sqrt(1.0f + C.b0 * C.b0);
  C.nb1 = std::sqrt(1.0f + C.b1 * C.b1);
  // bounding sphere of the voxel centres (3.5 sqrt 3 voxels) + nearest-voxel rounding (sqrt 3 / 2)
  // + the +-1 gradient neighbours = 7.93 voxels; 10 leaves room for float error
  C.reach = 10.0f * e->cfg.voxel_size;
  C.len = (float)(max_step * step) + C.reach;
  return C;
}

}  // namespace

int tsdf_render_blocks(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H,
                       const tsdf_pose* pose, float max_depth, void* out, int64_t capacity,
                       int64_t* count, int mem_kind) {
  TraceRange trace_("tsdf_render_blocks");
  if (!e || !K || !pose || !count || W <= 0 || H <= 0 || !(max_depth > 0) ||
      (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE)) {
    set_error("tsdf_render_blocks: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const FrameParams P = make_params(e, K, W, H, pose, max_depth);
  const RenderCull C = render_cull(e, P, W, 0, H);
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(k_render_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, P, C);
  hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, e->D, e->q_sel,
                     e->q_count);
  LAUNCH_OK("render select");
  int32_t nsel = 0;
  HIP_OK(hipMemcpyAsync(&nsel, e->q_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  *count = nsel;
  if (!out || nsel == 0) return TSDF_OK;
  if (capacity < nsel) {
    set_error("tsdf_render_blocks: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  return pack_selected(e, nsel, out, mem_kind, "tsdf_render_blocks");
}

namespace {
int ensure_groups(tsdf_engine* e, int n) {
  if ((size_t)n <= e->g_count.cap) return TSDF_OK;
  release_all(e->g_visbits, e->g_wgcnt, e->g_sel, e->g_count);
  int rc = e->g_visbits.ensure((size_t)n * kOccWords, "grouped selection: hipMalloc g_visbits");
  if (!rc) rc = e->g_wgcnt.ensure((size_t)n * (kOccWords / 256), "grouped selection: hipMalloc g_wgcnt");
  if (!rc) rc = e->g_sel.ensure((size_t)n * e->D.nblocks, "grouped selection: hipMalloc g_sel");
  if (!rc) rc = e->g_count.ensure((size_t)n, "grouped selection: hipMalloc g_count");
  return rc;
}

// the groups of S: selection, per-group lists (entry order) and their counts (one host round trip);
// then, when out != NULL, the records group by group (TSDF_BLOCK_RECORD_BYTES each) into out
int group_records(tsdf_engine* e, const FrameParams& P, const GroupSel& S, void* out, int64_t capacity,
                  int64_t* counts, int mem_kind, const char* what) {
  int rc = ensure_groups(e, S.ngroups);
  if (rc) return rc;
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(k_group_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, P, S, e->g_visbits,
                     e->g_wgcnt);
  for (int g = 0; g < S.ngroups; ++g) {
    EngineDev Dg = e->D;
    Dg.visbits = e->g_visbits + (size_t)g * kOccWords;
    Dg.wgcnt = e->g_wgcnt + (size_t)g * (kOccWords / 256);
    hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, Dg, e->g_sel + (size_t)g * e->D.nblocks,
                       e->g_count + g);
  }
  LAUNCH_OK(what);
  std::vector<int32_t> n(S.ngroups);
  HIP_OK(hipMemcpyAsync(n.data(), e->g_count, sizeof(int32_t) * S.ngroups, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  int64_t total = 0;
  for (int g = 0; g < S.ngroups; ++g) {
    counts[g] = n[g];
    total += n[g];
  }
  if (!out || total == 0) return TSDF_OK;
  if (capacity < total) {
    set_error("grouped block records: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  uint8_t* dst = reinterpret_cast<uint8_t*>(out);
  DevBuf<uint8_t> tmp;  // (freed on return: after the synchronisation below)
  if (mem_kind == TSDF_MEM_HOST) {
    if (int rc = tmp.ensure((size_t)total * kBlockRecBytes, "block records: hipMalloc staging")) return rc;
    dst = tmp;
  }
  int64_t off = 0;
  for (int g = 0; g < S.ngroups; ++g) {
    if (n[g])
      hipLaunchKernelGGL(k_render_pack, dim3(n[g]), dim3(256), 0, s, e->D, e->g_sel + (size_t)g * e->D.nblocks,
                         dst + (size_t)off * kBlockRecBytes);
    off += n[g];
  }
  hipError_t err = hipGetLastError();
  if (err == hipSuccess && tmp) err = hipMemcpyAsync(out, tmp, (size_t)total * kBlockRecBytes, hipMemcpyDeviceToHost, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) {
    set_error(what, err);
    return TSDF_ERR_HIP;
  }
  return TSDF_OK;
}
}  // namespace

int tsdf_render_bands(tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* pose,
                      float max_depth, int nbands, const int32_t* rows, void* out, int64_t capacity,
                      int64_t* counts, int mem_kind) {
  TraceRange trace_("tsdf_render_bands");
  bool ok = e && K && pose && counts && rows && W > 0 && H > 0 && max_depth > 0 && nbands >= 1 &&
            nbands <= kMaxGroups && (mem_kind == TSDF_MEM_HOST || mem_kind == TSDF_MEM_DEVICE);
  for (int b = 0; ok && b < nbands; ++b) ok = rows[b] >= 0 && rows[b] < rows[b + 1] && rows[b + 1] <= H;
  if (!ok) {
    set_error("tsdf_render_bands: invalid argument (1..64 bands of increasing rows within the image)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const FrameParams P = make_params(e, K, W, H, pose, max_depth);
  GroupSel S{};
  S.mode = kGroupBands;
  S.ngroups = nbands;
  S.cull = render_cull(e, P, W, 0, H);
  for (int b = 0; b < nbands; ++b) {
    const RenderCull C = render_cull(e, P, W, rows[b], rows[b + 1]);
    S.b0[b] = C.b0;
    S.b1[b] = C.b1;
    S.nb0[b] = C.nb0;
    S.nb1[b] = C.nb1;
  }
  return group_records(e, P, S, out, capacity, counts, mem_kind, "tsdf_render_bands");
}

int tsdf_pack_halo(tsdf_engine* e, void* out, int64_t capacity, int64_t* counts, int mem_kind) {
  TraceRange trace_("tsdf_pack_halo");
  if (!e || !counts || e->cfg.shard_count < 2 || (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE)) {
    set_error("tsdf_pack_halo: invalid argument (a shard engine)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (e->shard_phase != 0) {
    set_error("tsdf_pack_halo: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  FrameParams P{};
  P.shard_index = e->cfg.shard_index;
  P.shard_count = e->cfg.shard_count;
  GroupSel S{};
  S.mode = kGroupHalo;
  S.ngroups = e->cfg.shard_count;
  return group_records(e, P, S, out, capacity, counts, mem_kind, "tsdf_pack_halo");
}

int tsdf_pack_blocks(tsdf_engine* e, const float* bounds, void* out, int64_t capacity,
                     int64_t* count, int mem_kind) {
  TraceRange trace_("tsdf_pack_blocks");
  if (!e || !count || (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE)) {
    set_error("tsdf_pack_blocks: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  short4 lo = make_short4(0, 0, 0, 0), hi = make_short4(0, 0, 0, 0);
  if (bounds) {  // the Query block selection (voxel_tsdf.cuh:21-26, voxel_tsdf.cu:429)
    const float scale = (float)(1. / (double)e->cfg.voxel_size);
    lo = make_short4(h_f2s(bounds[0] * scale), h_f2s(bounds[2] * scale), h_f2s(bounds[4] * scale), 0);
    hi = make_short4(h_f2s(bounds[1] * scale), h_f2s(bounds[3] * scale), h_f2s(bounds[5] * scale), 0);
  }
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(k_query_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, bounds ? 1 : 0,
                     lo, hi);
  hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, e->D, e->q_sel,
                     e->q_count);
  LAUNCH_OK("pack select");
  int32_t nsel = 0;
  HIP_OK(hipMemcpyAsync(&nsel, e->q_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  *count = nsel;
  if (!out || nsel == 0) return TSDF_OK;
  if (capacity < nsel) {
    set_error("tsdf_pack_blocks: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  return pack_selected(e, nsel, out, mem_kind, "tsdf_pack_blocks");
}

int tsdf_import_blocks(tsdf_engine* e, const void* records, int64_t n, int mem_kind, int replace) {
  TraceRange trace_("tsdf_import_blocks");
  if (!e || n < 0 || (n > 0 && !records) ||
      (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE)) {
    set_error("tsdf_import_blocks: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  if (e->shard_phase != 0) {
    set_error("tsdf_import_blocks: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (replace && !init_state(e, false)) {
    set_error("tsdf_import_blocks: clearing the volume failed");
    return TSDF_ERR_HIP;
  }
  if (n == 0) return TSDF_OK;
  hipStream_t s = e->stream;
  const size_t bytes = (size_t)n * kBlockRecBytes;
  const uint8_t* recs = reinterpret_cast<const uint8_t*>(records);
  DevBuf<uint8_t> tmp;  // (freed on return)
  if (mem_kind == TSDF_MEM_HOST) {
    if (int rc = tmp.ensure(bytes, "tsdf_import_blocks: hipMalloc staging")) return rc;
    hipError_t err = hipMemcpyAsync(tmp, records, bytes, hipMemcpyHostToDevice, s);
    if (err != hipSuccess) {
      set_error("tsdf_import_blocks upload", err);
      return TSDF_ERR_HIP;
    }
    recs = tmp;
  }
  auto done = [&](int rc) {  // the stream may still be reading the staged records: it finishes first
    if (tmp) (void)hipStreamSynchronize(s);
    return rc;
  };
  // VoxelHashTable::Allocate keeps <= 1 structural change per bucket per launch (voxel_hash.cu:
  // 80-118): resolver launches over the still-missing keys until every record has its block
  for (int64_t base = 0; base < n; base += kNewKeyCap) {
    const int m = (int)std::min<int64_t>(kNewKeyCap, n - base);
    const uint8_t* chunk = recs + (size_t)base * kBlockRecBytes;
    int32_t missing = m;
    for (int round = 0; missing > 0; ++round) {
      if (round == 64) {
        set_error("tsdf_import_blocks: keys still missing after 64 allocation launches");
        return done(TSDF_ERR_HIP);
      }
      hipLaunchKernelGGL(k_import_keys, dim3((m + 255) / 256), dim3(256), 0, s, e->D, chunk, m);
      if (hipGetLastError() != hipSuccess) return done(TSDF_ERR_HIP);
      int rc = launch_resolve_alloc(e, FrameParams{}, (uint32_t)m, 0);
      if (rc) return done(rc);
      // every record whose block exists gets its payload; the rest are counted (one round trip
      // for that count and the status word)
      if (hipMemsetAsync(e->q_count, 0, sizeof(int32_t), s) != hipSuccess) return done(TSDF_ERR_HIP);
      hipLaunchKernelGGL(k_import_payload, dim3((unsigned)m), dim3(256), 0, s, e->D, chunk, e->q_count);
      if (hipGetLastError() != hipSuccess ||
          hipMemcpyAsync(e->h_ctr, e->D.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipMemcpyAsync(&missing, e->q_count, sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess)
        return done(TSDF_ERR_HIP);
      if (missing > 0 && (e->h_ctr->status & TSDF_STATUS_POOL_EXHAUSTED)) {
        set_error("tsdf_import_blocks: voxel block pool exhausted");
        return done(TSDF_ERR_OUT_OF_MEMORY);
      }
    }
  }
  return done(TSDF_OK);
}
