// tsdf_host_plan.hip -- lamp-stop planning (DESIGN.md "Lamp-stop planning"; kernels in tsdf_plan.hip):
// tsdf_uv_irradiance and tsdf_uv_plan.
#include <cmath>
#include <cstring>

#include "tsdf_host.h"

namespace {

// one lane per receiver: the launch's workgroups
bool lanes_ok(int64_t n) { return n >= 0 && (n + 255) / 256 <= (int64_t)INT32_MAX; }
// candidates per launch: the grid's second dimension
constexpr int kRowsPerLaunch = 65535;

// `bytes` of pl_dev and of its pinned copy, the pinned copy free to be written
int plan_buffers(tsdf_engine* e, size_t bytes) {
  if (!e->pl_ev) HIP_OK(hipEventCreateWithFlags(&e->pl_ev, hipEventDisableTiming));
  if (e->pl_busy) {
    HIP_OK(hipEventSynchronize(e->pl_ev));
    e->pl_busy = false;
  }
  if (bytes <= e->pl_cap) return TSDF_OK;
  e->pl_dev.release();
  if (e->pl_h) (void)hipHostFree(e->pl_h);
  e->pl_h = nullptr;
  e->pl_cap = 0;
  if (int rc = e->pl_dev.ensure(bytes, "tsdf_uv_plan: hipMalloc pl_dev")) return rc;
  HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&e->pl_h), bytes));
  e->pl_cap = bytes;
  return TSDF_OK;
}

// tsdf_uv_irradiance on device arrays (after ENTER): m = first[C] > 0 emitters
int irradiance_launch(tsdf_engine* e, const float* points, const float* normals, int64_t n, const tsdf_uv_emitter* em,
                      const int32_t* first, int32_t C, const tsdf_uv_config& c, float* out) {
  const int32_t m = first[C];
  // the emitters, the offsets, then the box words and flags of k_dose_bounds
  const size_t o_first = (size_t)m * 16, o_box = o_first + up16((size_t)(C + 1) * 4);
  int rc = plan_buffers(e, o_box + 32 + (size_t)m * 4);
  if (rc) return rc;
  hipStream_t s = e->stream;
  if (m) std::memcpy(e->pl_h, em, (size_t)m * 16);
  std::memcpy(e->pl_h + o_first, first, (size_t)(C + 1) * 4);
  HIP_OK(hipMemcpyAsync(e->pl_dev, e->pl_h, o_box, hipMemcpyHostToDevice, s));
  DoseParams A{};
  A.points = points;
  A.normals = normals;
  A.dose = nullptr;
  A.n = n;
  A.emit = reinterpret_cast<const float4*>(e->pl_dev.p);
  A.m = m;
  A.voxel = e->cfg.voxel_size;
  A.bias = c.bias;
  A.sv = c.step / e->cfg.voxel_size;
  A.min_range = c.min_range;
  A.max_range = c.max_range;
  A.offset = c.sample_offset;
  A.min_weight = c.min_weight;
  ViewGrid V{};
  V.flags = e->vg_flags;
  V.bits = e->vg_bits;
  // one bounds pass over every candidate's emitters, one read-back, one grid for the whole call
  if (c.use_grid && m > 0) {
    rc = dose_view_grid(e, A, em, reinterpret_cast<int32_t*>(e->pl_dev + o_box),
                        reinterpret_cast<int32_t*>(e->pl_h + o_box), &V);
    if (rc) return rc;
  }
  const int32_t* dfirst = reinterpret_cast<const int32_t*>(e->pl_dev + o_first);
  for (int32_t c0 = 0; c0 < C; c0 += kRowsPerLaunch) {
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)std::min<int32_t>(kRowsPerLaunch, C - c0));
    hipLaunchKernelGGL(k_uv_irradiance, grid, dim3(256), V.n ? (size_t)V.nw * 4 : 0, s, e->D, A, V, dfirst, c0, out);
    LAUNCH_OK("k_uv_irradiance");
  }
  HIP_OK(hipEventRecord(e->pl_ev, s));
  e->pl_busy = true;
  return TSDF_OK;
}

}  // namespace

int tsdf_uv_irradiance(tsdf_engine* e, const float* points, const float* normals, int64_t n,
                       const tsdf_uv_emitter* emitters, const int32_t* first, int32_t C, const tsdf_uv_config* cfg,
                       float* out, int mem_kind) {
  TraceRange trace_("tsdf_uv_irradiance");
  tsdf_uv_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_uv_config_default(e, &c);
  // (written so that a NaN fails; the conditions of tsdf_uv_dose)
  bool ok = e && lanes_ok(n) && C >= 0 && (C == 0 || first) && (n == 0 || C == 0 || (points && normals && out)) &&
            mem_kind_ok(mem_kind) && c.min_range > 0.0f && c.max_range >= c.min_range && std::isfinite(c.max_range) &&
            c.step > 0.0f && c.max_range / c.step <= 65536.0f && std::fabs(c.bias) <= c.max_range &&
            std::isfinite(c.sample_offset);
  if (ok && C > 0) {
    ok = first[0] == 0;
    for (int32_t k = 0; ok && k < C; ++k) ok = first[k + 1] >= first[k];
    ok = ok && (first[C] == 0 || emitters);
  }
  // (every row's last element has an int64 index)
  ok = ok && (n == 0 || (int64_t)C <= INT64_MAX / 4 / n);
  if (!ok) {
    set_error("tsdf_uv_irradiance: invalid argument (first[0] == 0, first non-decreasing, first[C] emitters; "
              "0 < min_range <= max_range, step > 0, max_range / step <= 65536, |bias| <= max_range)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_uv_irradiance")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (n == 0 || C == 0) return TSDF_OK;
  if (mem_kind == TSDF_MEM_DEVICE) return irradiance_launch(e, points, normals, n, emitters, first, C, c, out);
  hipStream_t s = e->stream;
  const size_t bo = (size_t)C * (size_t)n * 4;
  Sections L;
  const int h_p = L.add((size_t)n * 12), h_nr = L.add((size_t)n * 12), h_d = L.add(bo);
  int rc = track_stage(e, L.total());
  if (rc) return rc;
  uint8_t* b = e->tk_stage;
  float *p = L.at<float>(b, h_p), *nr = L.at<float>(b, h_nr), *d = L.at<float>(b, h_d);
  HIP_OK(hipMemcpyAsync(p, points, (size_t)n * 12, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(nr, normals, (size_t)n * 12, hipMemcpyHostToDevice, s));
  rc = irradiance_launch(e, p, nr, n, emitters, first, C, c, d);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(out, d, bo, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

void tsdf_uv_plan_config_default(tsdf_uv_plan_config* c) {
  if (!c) return;
  c->max_stops = 16;
  c->min_gain = 0.0f;
}

int tsdf_uv_plan(tsdf_engine* e, const float* irradiance, int32_t C, int64_t n, float* need, const float* weight,
                 const tsdf_uv_plan_config* cfg, int32_t* stops, double* gains, int32_t* num_stops, int mem_kind) {
  TraceRange trace_("tsdf_uv_plan");
  tsdf_uv_plan_config c;
  if (cfg)
    c = *cfg;
  else
    tsdf_uv_plan_config_default(&c);
  const bool work = C > 0 && n > 0 && c.max_stops > 0;
  if (!e || !lanes_ok(n) || C < 0 || (n > 0 && (int64_t)C > INT64_MAX / 4 / n) || !num_stops || c.max_stops < 0 ||
      c.max_stops > 65536 || !(c.min_gain == c.min_gain) || !mem_kind_ok(mem_kind) ||
      (work && (!irradiance || !need || !stops || !gains))) {
    set_error("tsdf_uv_plan: invalid argument (0 <= max_stops <= 65536, min_gain not NaN)");
    return TSDF_ERR_INVALID_ARG;
  }
  *num_stops = 0;
  if (!work) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const int G = (int)((n + kPlanChunk - 1) / kPlanChunk);
  // PlanState, the gains, the stops
  const size_t o_gain = 16, o_stop = o_gain + (size_t)c.max_stops * 8, bytes = o_stop + (size_t)c.max_stops * 4;
  int rc = plan_buffers(e, bytes);
  if (rc) return rc;
  rc = e->pl_part.ensure((size_t)G * (size_t)C, "tsdf_uv_plan: hipMalloc pl_part");
  if (rc) return rc;
  PlanArgs P{};
  P.E = irradiance;
  P.need = need;
  P.weight = weight;
  if (mem_kind == TSDF_MEM_HOST) {
    Sections L;  // (the weights have their section, given or not)
    const int h_E = L.add((size_t)C * (size_t)n * 4), h_need = L.add((size_t)n * 4), h_w = L.add((size_t)n * 4);
    rc = e->pl_stage.ensure(L.total(), "tsdf_uv_plan: hipMalloc pl_stage");
    if (rc) return rc;
    uint8_t* b = e->pl_stage;
    float *dE = L.at<float>(b, h_E), *dneed = L.at<float>(b, h_need), *dw = L.at<float>(b, h_w);
    HIP_OK(hipMemcpyAsync(dE, irradiance, (size_t)C * (size_t)n * 4, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(dneed, need, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (weight) HIP_OK(hipMemcpyAsync(dw, weight, (size_t)n * 4, hipMemcpyHostToDevice, s));
    P.E = dE;
    P.need = dneed;
    P.weight = weight ? dw : nullptr;
  }
  P.n = n;
  P.C = C;
  P.part = e->pl_part;
  P.state = reinterpret_cast<PlanState*>(e->pl_dev.p);
  P.gains = reinterpret_cast<double*>(e->pl_dev + o_gain);
  P.stops = reinterpret_cast<int32_t*>(e->pl_dev + o_stop);
  std::memset(e->pl_h, 0, bytes);
  HIP_OK(hipMemcpyAsync(e->pl_dev, e->pl_h, bytes, hipMemcpyHostToDevice, s));
  // Every round is enqueued; a round after the one that stopped finds PlanState::stopped and returns at
  // once, so the host reads nothing until the end.
  const dim3 rows((unsigned)((n + 255) / 256));
  for (int r = 0; r < c.max_stops; ++r) {
    for (int64_t c0 = 0; c0 < C; c0 += (int64_t)kRowsPerLaunch * kPlanRows) {
      const int64_t groups = std::min<int64_t>(kRowsPerLaunch, (C - c0 + kPlanRows - 1) / kPlanRows);
      hipLaunchKernelGGL(k_plan_gain, dim3((unsigned)G, (unsigned)groups), dim3(256), 0, s, P, (int)c0);
    }
    hipLaunchKernelGGL(k_plan_final, dim3(1), dim3(256), 0, s, P, G, r, c.min_gain);
    hipLaunchKernelGGL(k_plan_apply, rows, dim3(256), 0, s, P);
    LAUNCH_OK("k_plan_gain / k_plan_final / k_plan_apply");
  }
  HIP_OK(hipMemcpyAsync(e->pl_h, e->pl_dev, bytes, hipMemcpyDeviceToHost, s));
  if (mem_kind == TSDF_MEM_HOST) HIP_OK(hipMemcpyAsync(need, P.need, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  const PlanState* st = reinterpret_cast<const PlanState*>(e->pl_h);
  const int32_t k = std::min(std::max(st->nstops, 0), c.max_stops);
  std::memcpy(gains, e->pl_h + o_gain, (size_t)k * 8);
  std::memcpy(stops, e->pl_h + o_stop, (size_t)k * 4);
  *num_stops = k;
  return TSDF_OK;
}
