// tsdf_host_free.hip -- observed free space (DESIGN.md "Observed free space"; kernels in tsdf_free.hip):
// tsdf_free_words, tsdf_free_observe and tsdf_free_apply.
#include "tsdf_host.h"
#include "tsdf_free.h"

namespace {

// the limits and every voxel of the box in a block of the int16 block range
bool free_box_ok(const int32_t* origin, const int32_t* dims) {
  return box_dims_ok(dims) && box_in_block_range(origin, dims, 0);
}

}  // namespace

int64_t tsdf_free_words(const int32_t dims[3]) { return dims && box_dims_ok(dims) ? box_words(dims) : 0; }

int tsdf_free_observe(tsdf_engine* e, const tsdf_free_box* box, uint32_t* bits, const float* depth, int width,
                      int height, int mem_kind, const tsdf_intrinsics* K, const tsdf_pose* cam_T_world,
                      float max_depth) {
  TraceRange trace_("tsdf_free_observe");
  if (!e || !box || !bits || !depth || !K || !cam_T_world || !mem_kind_ok(mem_kind) ||
      !free_box_ok(box->origin, box->dims) || width < 1 || width > e->cfg.max_width || height < 1 ||
      height > e->cfg.max_height || !(max_depth > 0.0f)) {
    set_error("tsdf_free_observe: invalid argument (" BOX_LIMITS_TEXT ", the box inside the block "
              "range, width and height 1..the engine's, max_depth > 0, box, bits, depth, K and pose non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const FrameParams P = make_params(e, K, width, height, cam_T_world, max_depth);
  FreeArgs A{};
  A.ox = box->origin[0], A.oy = box->origin[1], A.oz = box->origin[2];
  A.nx = box->dims[0], A.ny = box->dims[1], A.nz = box->dims[2];
  A.wx = (A.nx + 31) >> 5;
  A.W = width, A.H = height;
  A.fx = P.fx, A.fy = P.fy, A.cx = P.cx, A.cy = P.cy;
  A.cq = P.cq, A.ct = P.ct;
  A.voxel = P.voxel, A.trunc = P.trunc, A.max_depth = max_depth;
  A.cull_words = e->env.free_cull ? 1 : 0;
  // The brick cull takes cam_T_world for a rigid motion (pose_is_rigid); any other q, and a truncation that is
  // not positive (free would not need hz < d), go without it.
  const float q[4] = {P.cq.x, P.cq.y, P.cq.z, P.cq.w};
  A.cull_bricks = (e->env.free_cull && pose_is_rigid(q) && P.trunc > 0.0f) ? 1 : 0;
  const size_t words = (size_t)box_words(box->dims), npix = (size_t)width * height;
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: pixel records | host arrays' staging: bits, depth
  Sections L;
  const int h_pix = L.add(npix * sizeof(FreePix)), h_bits = L.add(staged(host, bits, 4 * words)),
            h_depth = L.add(staged(host, depth, 4 * npix));
  int rc = e->fr_buf.ensure(L.total(), "tsdf_free_observe: hipMalloc fr_buf");
  if (rc) return rc;
  const Stage St{L, e->fr_buf.p, host, s};
  FreePix* pix = L.at<FreePix>(St.base, h_pix);
  uint32_t* dbits = nullptr;
  const float* ddepth = nullptr;
  HIP_OK(St.in(h_bits, bits, 4 * words, &dbits));
  HIP_OK(St.in(h_depth, depth, 4 * npix, &ddepth));
  A.bits = dbits;
  A.pix = pix;
  hipLaunchKernelGGL(k_free_pixels, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, ddepth, width, height, P.ifx,
                     P.ify, P.icx, P.icy, max_depth, pix);
  LAUNCH_OK("k_free_pixels");
  hipLaunchKernelGGL(k_free_observe, free_brick_grid(A.nx, A.ny, A.nz), dim3(256), 0, s, A);
  LAUNCH_OK("k_free_observe");
  HIP_OK(St.back(bits, dbits, 4 * words));
  if (host) HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_free_apply(tsdf_engine* e, const tsdf_free_box* box, const uint32_t* bits, const int32_t origin[3],
                    const int32_t dims[3], uint8_t* state, int mem_kind, int64_t* promoted) {
  TraceRange trace_("tsdf_free_apply");
  if (!e || !box || !bits || !origin || !dims || !state || !mem_kind_ok(mem_kind) ||
      !free_box_ok(box->origin, box->dims) || !free_box_ok(origin, dims)) {
    set_error("tsdf_free_apply: invalid argument (both boxes: " BOX_LIMITS_TEXT ", inside the block "
              "range; box, bits, origin, dims and state non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  FreeApplyArgs A{};
  A.nx = dims[0], A.ny = dims[1], A.nz = dims[2];
  A.dx = origin[0] - box->origin[0], A.dy = origin[1] - box->origin[1], A.dz = origin[2] - box->origin[2];
  A.lx = box->dims[0], A.ly = box->dims[1], A.lz = box->dims[2];
  A.wx = (A.lx + 31) >> 5;
  const size_t words = (size_t)box_words(box->dims), n = box_voxels(dims);
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: the counter | host arrays' staging: bits, state
  Sections L;
  const int h_ctr = L.add(16), h_bits = L.add(staged(host, bits, 4 * words)), h_state = L.add(staged(host, state, n));
  int rc = e->fr_buf.ensure(L.total(), "tsdf_free_apply: hipMalloc fr_buf");
  if (rc) return rc;
  const Stage St{L, e->fr_buf.p, host, s};
  unsigned long long* dctr = L.at<unsigned long long>(St.base, h_ctr);
  HIP_OK(St.in(h_bits, bits, 4 * words, &A.bits));
  HIP_OK(St.in(h_state, state, n, &A.state));
  A.promoted = promoted ? dctr : nullptr;
  if (promoted) HIP_OK(hipMemsetAsync(dctr, 0, L.size(h_ctr), s));
  const size_t per_wg = 256 * (size_t)kFreeApplyChunk;
  hipLaunchKernelGGL(k_free_apply, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(256), 0, s, A);
  LAUNCH_OK("k_free_apply");
  unsigned long long count = 0;
  if (promoted) HIP_OK(hipMemcpyAsync(&count, dctr, sizeof(count), hipMemcpyDeviceToHost, s));
  HIP_OK(St.back(state, A.state, n));
  if (host || promoted) HIP_OK(hipStreamSynchronize(s));
  if (promoted) *promoted = (int64_t)count;
  return TSDF_OK;
}
