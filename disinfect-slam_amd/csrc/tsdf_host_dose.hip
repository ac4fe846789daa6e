// tsdf_host_dose.hip -- UV dose (DESIGN.md "UV dose"; kernels in tsdf_dose.hip): tsdf_surface_normals
// and tsdf_uv_dose.
#include <cmath>
#include <cstring>

#include "tsdf_host.h"

void tsdf_uv_config_default(const tsdf_engine* e, tsdf_uv_config* c) {
  if (!c) return;
  *c = tsdf_uv_config{};
  const float voxel = e ? e->cfg.voxel_size : 0.005f;
  c->bias = 2.0f * voxel;
  c->step = voxel;
  c->min_range = 0.05f;
  c->max_range = 5.0f;
  c->sample_offset = 0.0f;
  c->min_weight = 1;
  c->use_grid = 1;
}

namespace {

// one lane per point: the launch's workgroups
bool lanes_ok(int64_t n) { return n >= 0 && (n + 255) / 256 <= (int64_t)INT32_MAX; }

// room for m emitters (device and pinned), and the pinned copy free to be written
int dose_buffers(tsdf_engine* e, int32_t m) {
  if (!e->uv_ev) HIP_OK(hipEventCreateWithFlags(&e->uv_ev, hipEventDisableTiming));
  if (e->uv_busy) {
    HIP_OK(hipEventSynchronize(e->uv_ev));
    e->uv_busy = false;
  }
  if (m <= e->uv_cap) return TSDF_OK;
  e->uv_dev.release();
  if (e->uv_h) (void)hipHostFree(e->uv_h);
  e->uv_h = nullptr;
  e->uv_cap = 0;
  const size_t bytes = (size_t)m * 20 + 32;  // float4 + flag per emitter, the box
  if (int rc = e->uv_dev.ensure(bytes, "tsdf_uv_dose: hipMalloc uv_dev")) return rc;
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&e->uv_h), bytes));
  e->uv_cap = m;
  return TSDF_OK;
}

}  // namespace

// (tsdf_host.h; tsdf_uv_irradiance shares it) The block grid of a dose launch: a cube over the ray origins of the irradiated receivers
// and the emitters that irradiate one (k_dose_bounds), two voxels of room around them. Every sample lies
// between a ray's two ends, so inside the box; a lookup outside the grid would go to the hash table all
// the same.
int dose_view_grid(tsdf_engine* e, DoseParams& A, const tsdf_uv_emitter* em, int32_t* box, int32_t* hbox,
                   ViewGrid* Vp) {
  ViewGrid& V = *Vp;
  hipStream_t s = e->stream;
  const int32_t m = A.m;
  const dim3 grid((unsigned)((A.n + 255) / 256));
  int32_t* flag = box + 8;
  for (int a = 0; a < 3; ++a) hbox[a] = INT32_MAX, hbox[3 + a] = INT32_MIN;
  std::memset(hbox + 8, 0, (size_t)m * 4);
  HIP_OK(hipMemcpyAsync(box, hbox, 32 + (size_t)m * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_dose_bounds, grid, dim3(256), 0, s, A, box, flag);
  LAUNCH_OK("k_dose_bounds");
  HIP_OK(hipMemcpyAsync(hbox, box, 32 + (size_t)m * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const int32_t* hflag = hbox + 8;
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = hbox[a], hi[a] = hbox[3 + a];
  for (int32_t k = 0; k < m; ++k) {
    if (!hflag[k]) continue;
    const float ec[3] = {em[k].x, em[k].y, em[k].z};
    for (int a = 0; a < 3; ++a) {
      const double v = (double)(ec[a] / A.voxel - A.offset);
      lo[a] = std::min(lo[a], std::floor(v));
      hi[a] = std::max(hi[a], std::ceil(v));
    }
  }
  bool ok = lo[0] <= hi[0];  // (some receiver is irradiated)
  int cb[3] = {0, 0, 0}, half = 0;
  for (int a = 0; ok && a < 3; ++a) {
    ok = lo[a] > -1e6 && hi[a] < 1e6;
    if (!ok) break;
    const int b0 = ((int)lo[a] - 2) >> kBlockLenBits, b1 = ((int)hi[a] + 2) >> kBlockLenBits;
    cb[a] = (b0 + b1) >> 1;
    half = std::max(half, std::max(cb[a] - b0, b1 - cb[a]));
  }
  if (ok && 2 * half + 1 <= kViewMaxN) {  // (a wider box: hash lookups, V.n stays 0)
    ViewShape S;
    view_shape_half(e, half, kViewBitmapWords, &S);
    if (int rc = view_grid_take(e, S, &V)) return rc;
  }
  if (V.n) {
    // k_view_grid places the cube by a camera centre: the centre block's first voxel, in voxel units
    FrameParams P{};
    P.voxel = 1.0f;
    P.wt = {(float)(cb[0] * kBlockLen), (float)(cb[1] * kBlockLen), (float)(cb[2] * kBlockLen)};
    A.ox = cb[0] - half;
    A.oy = cb[1] - half;
    A.oz = cb[2] - half;
    hipLaunchKernelGGL(k_view_grid, dim3(kOccWords / 256), dim3(256), 0, s, e->D, P, V);
    hipLaunchKernelGGL(k_view_pack, dim3(kViewPackGrid), dim3(256), 0, s, V);
    LAUNCH_OK("k_view_grid");
  }
  return TSDF_OK;
}

namespace {

// tsdf_uv_dose on device arrays (after ENTER)
int dose_launch(tsdf_engine* e, const float* points, const float* normals, int64_t n, const tsdf_uv_emitter* em,
                int32_t m, const tsdf_uv_config& c, float* dose) {
  int rc = dose_buffers(e, m);
  if (rc) return rc;
  hipStream_t s = e->stream;
  const size_t o_box = (size_t)e->uv_cap * 16;  // (then the flags, 32 bytes on)
  std::memcpy(e->uv_h, em, (size_t)m * 16);
  HIP_OK(hipMemcpyAsync(e->uv_dev, e->uv_h, (size_t)m * 16, hipMemcpyHostToDevice, s));
  DoseParams A{};
  A.points = points;
  A.normals = normals;
  A.dose = dose;
  A.n = n;
  A.emit = reinterpret_cast<const float4*>(e->uv_dev.p);
  A.m = m;
  A.voxel = e->cfg.voxel_size;
  A.bias = c.bias;
  A.sv = c.step / e->cfg.voxel_size;
  A.min_range = c.min_range;
  A.max_range = c.max_range;
  A.offset = c.sample_offset;
  A.min_weight = c.min_weight;
  const dim3 grid((unsigned)((n + 255) / 256));
  ViewGrid V{};
  V.flags = e->vg_flags;
  V.bits = e->vg_bits;
  if (c.use_grid) {
    rc = dose_view_grid(e, A, em, reinterpret_cast<int32_t*>(e->uv_dev + o_box),
                        reinterpret_cast<int32_t*>(e->uv_h + o_box), &V);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_uv_dose, grid, dim3(256), V.n ? (size_t)V.nw * 4 : 0, s, e->D, A, V);
  LAUNCH_OK("k_uv_dose");
  HIP_OK(hipEventRecord(e->uv_ev, s));
  e->uv_busy = true;
  return TSDF_OK;
}

}  // namespace

int tsdf_surface_normals(tsdf_engine* e, const float* points, int64_t n, float sample_offset, float* normals,
                         int mem_kind) {
  TraceRange trace_("tsdf_surface_normals");
  if (!e || !lanes_ok(n) || (n > 0 && (!points || !normals)) || !std::isfinite(sample_offset) ||
      !mem_kind_ok(mem_kind)) {
    set_error("tsdf_surface_normals: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_surface_normals")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (n == 0) return TSDF_OK;
  hipStream_t s = e->stream;
  const float* p = points;
  float* out = normals;
  const size_t bytes = (size_t)n * 12;
  if (mem_kind == TSDF_MEM_HOST) {
    Sections L;
    const int h_p = L.add(bytes), h_out = L.add(bytes);
    int rc = track_stage(e, L.total());
    if (rc) return rc;
    HIP_OK(hipMemcpyAsync(L.at<float>(e->tk_stage.p, h_p), points, bytes, hipMemcpyHostToDevice, s));
    p = L.at<float>(e->tk_stage.p, h_p);
    out = L.at<float>(e->tk_stage.p, h_out);
  }
  hipLaunchKernelGGL(k_point_normals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, e->D, p, n,
                     e->cfg.voxel_size, sample_offset, out);
  LAUNCH_OK("k_point_normals");
  if (mem_kind == TSDF_MEM_HOST) {
    HIP_OK(hipMemcpyAsync(normals, out, bytes, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
  }
  return TSDF_OK;
}

int tsdf_uv_dose(tsdf_engine* e, const float* points, const float* normals, int64_t n, const tsdf_uv_emitter* emitters,
                 int32_t m, const tsdf_uv_config* cfg, float* dose, int mem_kind) {
  TraceRange trace_("tsdf_uv_dose");
  tsdf_uv_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_uv_config_default(e, &c);
  // (written so that a NaN fails; |bias| <= max_range and max_range / step <= 65536 bound a ray's samples)
  if (!e || !lanes_ok(n) || m < 0 || (n > 0 && (!points || !normals || !dose)) || (m > 0 && !emitters) ||
      !mem_kind_ok(mem_kind) || !(c.min_range > 0.0f) || !(c.max_range >= c.min_range) || !std::isfinite(c.max_range) ||
      !(c.step > 0.0f) || !(c.max_range / c.step <= 65536.0f) || !(std::fabs(c.bias) <= c.max_range) ||
      !std::isfinite(c.sample_offset)) {
    set_error("tsdf_uv_dose: invalid argument (0 < min_range <= max_range, step > 0, max_range / step <= 65536, "
              "|bias| <= max_range)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_uv_dose")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (n == 0 || m == 0) return TSDF_OK;
  if (mem_kind == TSDF_MEM_DEVICE) return dose_launch(e, points, normals, n, emitters, m, c, dose);
  hipStream_t s = e->stream;
  Sections L;
  const int h_p = L.add((size_t)n * 12), h_nr = L.add((size_t)n * 12), h_d = L.add((size_t)n * 4);
  int rc = track_stage(e, L.total());
  if (rc) return rc;
  uint8_t* b = e->tk_stage;
  float *p = L.at<float>(b, h_p), *nr = L.at<float>(b, h_nr), *d = L.at<float>(b, h_d);
  HIP_OK(hipMemcpyAsync(p, points, (size_t)n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(nr, normals, (size_t)n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(d, dose, (size_t)n * 4, hipMemcpyHostToDevice, s));
  rc = dose_launch(e, p, nr, n, emitters, m, c, d);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(dose, d, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}
