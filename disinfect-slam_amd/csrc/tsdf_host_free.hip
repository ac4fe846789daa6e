// tsdf_host_free.hip -- observed free space (DESIGN.md "Observed free space"; kernels in tsdf_free.hip):
// tsdf_free_words, tsdf_free_observe and tsdf_free_apply.
#include <cmath>

#include "tsdf_host.h"
#include "tsdf_free.h"

namespace {

constexpr int kFreeMaxDim = 2048;
constexpr int64_t kFreeMaxVoxels = (int64_t)1 << 28;

bool free_dims_ok(const int32_t* dims) {
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > kFreeMaxDim) return false;
    n *= dims[a];
  }
  return n <= kFreeMaxVoxels;
}
// dims as above and every voxel of the box in a block of the int16 block range
bool free_box_ok(const int32_t* origin, const int32_t* dims) {
  if (!free_dims_ok(dims)) return false;
  for (int a = 0; a < 3; ++a) {
    const int64_t lo = (int64_t)origin[a] >> kBlockLenBits;
    const int64_t hi = ((int64_t)origin[a] + dims[a] - 1) >> kBlockLenBits;
    if (lo < -32768 || hi > 32767) return false;
  }
  return true;
}
int64_t free_words(const int32_t* dims) { return (int64_t)dims[2] * dims[1] * ((dims[0] + 31) >> 5); }

}  // namespace

int64_t tsdf_free_words(const int32_t dims[3]) { return dims && free_dims_ok(dims) ? free_words(dims) : 0; }

int tsdf_free_observe(tsdf_engine* e, const tsdf_free_box* box, uint32_t* bits, const float* depth, int width,
                      int height, int mem_kind, const tsdf_intrinsics* K, const tsdf_pose* cam_T_world,
                      float max_depth) {
  TraceRange trace_("tsdf_free_observe");
  if (!e || !box || !bits || !depth || !K || !cam_T_world || !mem_kind_ok(mem_kind) ||
      !free_box_ok(box->origin, box->dims) || width < 1 || width > e->cfg.max_width || height < 1 ||
      height > e->cfg.max_height || !(max_depth > 0.0f)) {
    set_error("tsdf_free_observe: invalid argument (dims 1..2048, at most 2^28 voxels, the box inside the block "
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
  // The brick cull takes cam_T_world for a rigid motion. For q = s u with u a unit quaternion the rotation
  // formula gives (1 - s^2) v + s^2 R v, so with |s^2 - 1| <= 2^-10 it stretches no length by more than
  // 1 + 2^-9, far inside the sphere's slack; any other q, and a truncation that is not positive (free would
  // not need hz < d), go without it.
  const double n2 = (double)P.cq.x * P.cq.x + (double)P.cq.y * P.cq.y + (double)P.cq.z * P.cq.z + (double)P.cq.w * P.cq.w;
  A.cull_bricks = (e->env.free_cull && std::fabs(n2 - 1.0) <= 0x1p-10 && P.trunc > 0.0f) ? 1 : 0;
  const size_t words = (size_t)free_words(box->dims), npix = (size_t)width * height;
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: pixel records | host arrays' staging: bits, depth
  const size_t b_pix = up16(npix * sizeof(FreePix)), b_bits = host ? up16(4 * words) : 0, b_depth = host ? up16(4 * npix) : 0;
  int rc = e->fr_buf.ensure(b_pix + b_bits + b_depth, "tsdf_free_observe: hipMalloc fr_buf");
  if (rc) return rc;
  uint8_t* b = e->fr_buf;
  FreePix* pix = reinterpret_cast<FreePix*>(b);
  uint32_t* dbits = host ? reinterpret_cast<uint32_t*>(b + b_pix) : bits;
  const float* ddepth = host ? reinterpret_cast<const float*>(b + b_pix + b_bits) : depth;
  if (host) {
    HIP_OK(hipMemcpyAsync(dbits, bits, 4 * words, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(b + b_pix + b_bits, depth, 4 * npix, hipMemcpyHostToDevice, s));
  }
  A.bits = dbits;
  A.pix = pix;
  hipLaunchKernelGGL(k_free_pixels, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, ddepth, width, height, P.ifx,
                     P.ify, P.icx, P.icy, max_depth, pix);
  LAUNCH_OK("k_free_pixels");
  const dim3 grid((unsigned)((A.nx + kFreeBrickX - 1) / kFreeBrickX), (unsigned)((A.ny + kFreeBrickY - 1) / kFreeBrickY),
                  (unsigned)((A.nz + kFreeBrickZ - 1) / kFreeBrickZ));
  hipLaunchKernelGGL(k_free_observe, grid, dim3(256), 0, s, A);
  LAUNCH_OK("k_free_observe");
  if (host) {
    HIP_OK(hipMemcpyAsync(bits, dbits, 4 * words, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  return TSDF_OK;
}

int tsdf_free_apply(tsdf_engine* e, const tsdf_free_box* box, const uint32_t* bits, const int32_t origin[3],
                    const int32_t dims[3], uint8_t* state, int mem_kind, int64_t* promoted) {
  TraceRange trace_("tsdf_free_apply");
  if (!e || !box || !bits || !origin || !dims || !state || !mem_kind_ok(mem_kind) ||
      !free_box_ok(box->origin, box->dims) || !free_box_ok(origin, dims)) {
    set_error("tsdf_free_apply: invalid argument (both boxes: dims 1..2048, at most 2^28 voxels, inside the block "
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
  const size_t words = (size_t)free_words(box->dims), n = (size_t)A.nx * A.ny * A.nz;
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: the counter | host arrays' staging: bits, state
  const size_t b_ctr = 16, b_bits = host ? up16(4 * words) : 0, b_state = host ? up16(n) : 0;
  int rc = e->fr_buf.ensure(b_ctr + b_bits + b_state, "tsdf_free_apply: hipMalloc fr_buf");
  if (rc) return rc;
  uint8_t* b = e->fr_buf;
  uint32_t* dbits = reinterpret_cast<uint32_t*>(b + b_ctr);
  uint8_t* dstate = b + b_ctr + b_bits;
  if (host) {
    HIP_OK(hipMemcpyAsync(dbits, bits, 4 * words, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(dstate, state, n, hipMemcpyHostToDevice, s));
  }
  A.bits = host ? dbits : bits;
  A.state = host ? dstate : state;
  A.promoted = promoted ? reinterpret_cast<unsigned long long*>(b) : nullptr;
  if (promoted) HIP_OK(hipMemsetAsync(b, 0, b_ctr, s));
  const size_t per_wg = 256 * (size_t)kFreeApplyChunk;
  hipLaunchKernelGGL(k_free_apply, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(256), 0, s, A);
  LAUNCH_OK("k_free_apply");
  unsigned long long count = 0;
  if (promoted) HIP_OK(hipMemcpyAsync(&count, b, sizeof(count), hipMemcpyDeviceToHost, s));
  if (host) HIP_OK(hipMemcpyAsync(state, dstate, n, hipMemcpyDeviceToHost, s));
  if (host || promoted) HIP_OK(hipStreamSynchronize(s));
  if (promoted) *promoted = (int64_t)count;
  return TSDF_OK;
}
