// tsdf_host_frontier.hip -- frontier mask and connected components (DESIGN.md "Frontiers and components";
// kernels in tsdf_frontier.hip): tsdf_frontier_mark, tsdf_components_config_default and tsdf_components.
#include <algorithm>
#include <cstddef>

#include "tsdf_host.h"
#include "tsdf_frontier.h"

static_assert(sizeof(tsdf_component) == sizeof(tsdf::CcRec) && offsetof(tsdf_component, lo) == offsetof(tsdf::CcRec, lo) &&
                  offsetof(tsdf_component, hi) == offsetof(tsdf::CcRec, hi) &&
                  offsetof(tsdf_component, sum) == offsetof(tsdf::CcRec, sum) &&
                  offsetof(tsdf_component, goal) == offsetof(tsdf::CcRec, goal) &&
                  offsetof(tsdf_component, goal_key) == offsetof(tsdf::CcRec, goal_key),
              "CcRec is tsdf_component");
static_assert(TSDF_COMPONENT_NONE == tsdf::kCcNone && TSDF_TRAVEL_UNREACHED == tsdf::kCcUnreached, "the kernels' constants");

void tsdf_components_config_default(tsdf_components_config* c) {
  if (!c) return;
  *c = tsdf_components_config{};
  c->min_size = 1;
}

namespace {

// components a call makes room for before it has counted them: one per 512 voxels (a tile's worth)
constexpr size_t kCcReserveShift = 9, kCcReserveMin = 4096;
// scratch per component: its accumulators and its record, a section each. Both are whole multiples of 16 bytes,
// so the two sections hold exactly `reserve` components and a buffer's room for them is a plain quotient.
constexpr size_t kCcAccBytes = kCcReplicas * sizeof(CcAcc), kCcPerComponent = kCcAccBytes + sizeof(CcRec);
static_assert(kCcAccBytes % 16 == 0 && sizeof(CcRec) % 16 == 0, "the per-component sections need no rounding");

size_t cc_tiles(const int32_t* dims) {
  size_t t = 1;
  for (int a = 0; a < 3; ++a) t *= (size_t)box_tiles(dims[a], kCcTileBits);
  return t;
}

}  // namespace

int tsdf_frontier_mark(tsdf_engine* e, const int32_t dims[3], const uint8_t* state, const uint32_t* cost, uint8_t* mask,
                       int mem_kind, int64_t* marked) {
  TraceRange trace_("tsdf_frontier_mark");
  if (!e || !dims || !state || !mask || !mem_kind_ok(mem_kind) || !box_dims_ok(dims)) {
    set_error("tsdf_frontier_mark: invalid argument (" BOX_LIMITS_TEXT ", dims, state and mask non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const size_t n = box_voxels(dims);
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: control words | host arrays' staging: state, cost, mask
  Sections L;
  const int h_ctl = L.add(sizeof(CcCtl)), h_state = L.add(staged(host, state, n)),
            h_cost = L.add(staged(host, cost, 4 * n)), h_mask = L.add(staged(host, mask, n));
  int rc = e->cc_buf.ensure(L.total(), "tsdf_frontier_mark: hipMalloc cc_buf");
  if (rc) return rc;
  const Stage St{L, e->cc_buf.p, host, s};
  CcCtl* dctl = L.at<CcCtl>(St.base, h_ctl);
  FrontierArgs A{};
  A.nx = dims[0], A.ny = dims[1], A.nz = dims[2];
  HIP_OK(St.in(h_state, state, n, &A.state));
  HIP_OK(St.in(h_cost, cost, 4 * n, &A.cost));
  A.mask = St.ptr(h_mask, mask);
  A.ctl = marked ? dctl : nullptr;
  if (marked) HIP_OK(hipMemsetAsync(dctl, 0, L.size(h_ctl), s));
  hipLaunchKernelGGL(k_frontier_mark, dim3((unsigned)cc_tiles(dims)), dim3(kCcTileVox), 0, s, A);
  LAUNCH_OK("k_frontier_mark");
  CcCtl ctl{};
  if (marked) HIP_OK(hipMemcpyAsync(&ctl, dctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
  HIP_OK(St.back(mask, A.mask, n));
  if (host || marked) HIP_OK(hipStreamSynchronize(s));
  if (marked) *marked = (int64_t)ctl.marked;
  return TSDF_OK;
}

int tsdf_components(tsdf_engine* e, const tsdf_components_config* cfg, const uint8_t* mask, const uint32_t* key,
                    uint32_t* label, int mem_kind, tsdf_component* clusters, int32_t capacity, int32_t* count,
                    int32_t* total) {
  TraceRange trace_("tsdf_components");
  if (!e || !cfg || !mask || !label || !count || !mem_kind_ok(mem_kind) || !box_dims_ok(cfg->dims) || cfg->min_size < 1 ||
      capacity < 0 || (capacity > 0 && !clusters)) {
    set_error("tsdf_components: invalid argument (" BOX_LIMITS_TEXT ", min_size >= 1, capacity >= 0, "
              "cfg, mask, label and count non-NULL, clusters with capacity > 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  CcArgs A{};
  A.nx = cfg->dims[0], A.ny = cfg->dims[1], A.nz = cfg->dims[2];
  A.tx = box_tiles(A.nx, kCcTileBits), A.ty = box_tiles(A.ny, kCcTileBits), A.tz = box_tiles(A.nz, kCcTileBits);
  const size_t n = box_voxels(cfg->dims), tiles = cc_tiles(cfg->dims);
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: control words | a slot per voxel | host arrays' staging: mask, key, label | accumulators | records.
  // The last two hold `reserve` components each, a number the call has to choose before it has counted them:
  // one per 512 voxels, or as many as the buffer it finds has room for. A mask with more is labelled once
  // more, into a buffer sized by the count -- the labelling is a function of the mask, so the count stands.
  Sections L;
  const int h_ctl = L.add(sizeof(CcCtl)), h_slot = L.add(4 * n), h_mask = L.add(staged(host, mask, n)),
            h_key = L.add(staged(host, key, 4 * n)), h_label = L.add(staged(host, label, 4 * n));
  const int fixed = L.n;
  const size_t b_fixed = L.total();
  size_t reserve = std::max(kCcReserveMin, n >> kCcReserveShift);
  if (e->cc_buf.cap > b_fixed) reserve = std::max(reserve, (e->cc_buf.cap - b_fixed) / kCcPerComponent);
  CcCtl ctl{};
  CcRec* drec = nullptr;
  Stage St{L, nullptr, host, s};
  for (int pass = 0;; ++pass) {
    L.keep(fixed);
    const int h_acc = L.add(reserve * kCcAccBytes), h_rec = L.add(reserve * sizeof(CcRec));
    int rc = e->cc_buf.ensure(L.total(), "tsdf_components: hipMalloc cc_buf");
    if (rc) return rc;
    St.base = e->cc_buf.p;
    A.ctl = L.at<CcCtl>(St.base, h_ctl);
    A.slot = L.at<uint32_t>(St.base, h_slot);
    A.label = St.ptr(h_label, label);
    A.acc = L.at<CcAcc>(St.base, h_acc);
    drec = L.at<CcRec>(St.base, h_rec);
    HIP_OK(St.in(h_mask, mask, n, &A.mask));
    HIP_OK(St.in(h_key, key, 4 * n, &A.key));
    HIP_OK(hipMemsetAsync(A.ctl, 0, L.size(h_ctl), s));
    hipLaunchKernelGGL(k_cc_local, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
    LAUNCH_OK("k_cc_local");
    if (tiles > 1) {
      hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
      LAUNCH_OK("k_cc_merge");
    }
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A);
    LAUNCH_OK("k_cc_flatten");
    HIP_OK(hipMemcpyAsync(&ctl, A.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (ctl.total <= reserve) break;
    if (pass > 0) {
      set_error("tsdf_components: two labellings of one mask counted different components");
      return TSDF_ERR_HIP;
    }
    reserve = ctl.total;
  }
  if (ctl.total > 0) {
    HIP_OK(hipMemsetAsync(A.acc, 0, (size_t)ctl.total * kCcReplicas * sizeof(CcAcc), s));
    hipLaunchKernelGGL(k_cc_stats, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
    LAUNCH_OK("k_cc_stats");
    hipLaunchKernelGGL(k_cc_emit, dim3((ctl.total + 255u) / 256u), dim3(256), 0, s, A, ctl.total, (uint32_t)cfg->min_size, drec);
    LAUNCH_OK("k_cc_emit");
    HIP_OK(hipMemcpyAsync(&ctl, A.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
  }
  HIP_OK(St.back(label, A.label, 4 * n));
  HIP_OK(hipStreamSynchronize(s));
  *count = (int32_t)ctl.count;
  if (total) *total = (int32_t)ctl.total;
  if (capacity == 0 || ctl.count == 0) return TSDF_OK;
  if ((int64_t)ctl.count > (int64_t)capacity) {
    set_error("tsdf_components: more clusters than capacity");
    return TSDF_ERR_CAPACITY;
  }
  // (unique labels: the order of the table does not depend on the order the device appended in)
  HIP_OK(hipMemcpyAsync(clusters, drec, (size_t)ctl.count * sizeof(tsdf_component), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  std::sort(clusters, clusters + ctl.count, [](const tsdf_component& a, const tsdf_component& b2) { return a.label < b2.label; });
  return TSDF_OK;
}
