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

constexpr int kCcMaxDim = 2048;
constexpr int64_t kCcMaxVoxels = (int64_t)1 << 28;
// components a call makes room for before it has counted them: one per 512 voxels (a tile's worth)
constexpr size_t kCcReserveShift = 9, kCcReserveMin = 4096;
// scratch per component: its accumulators and its record
constexpr size_t kCcPerComponent = kCcReplicas * sizeof(CcAcc) + sizeof(CcRec);

bool cc_dims_ok(const int32_t* dims) {
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > kCcMaxDim) return false;
    n *= dims[a];
  }
  return n <= kCcMaxVoxels;
}
size_t cc_tiles(const int32_t* dims) {
  size_t t = 1;
  for (int a = 0; a < 3; ++a) t *= (size_t)((dims[a] + kCcTile - 1) >> kCcTileBits);
  return t;
}

}  // namespace

int tsdf_frontier_mark(tsdf_engine* e, const int32_t dims[3], const uint8_t* state, const uint32_t* cost, uint8_t* mask,
                       int mem_kind, int64_t* marked) {
  TraceRange trace_("tsdf_frontier_mark");
  if (!e || !dims || !state || !mask || !mem_kind_ok(mem_kind) || !cc_dims_ok(dims)) {
    set_error("tsdf_frontier_mark: invalid argument (dims 1..2048, at most 2^28 voxels, dims, state and mask non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: control words | host arrays' staging: state, cost, mask
  const size_t b_ctl = up16(sizeof(CcCtl)), b_state = host ? up16(n) : 0, b_cost = host && cost ? up16(4 * n) : 0,
               b_mask = host ? up16(n) : 0;
  int rc = e->cc_buf.ensure(b_ctl + b_state + b_cost + b_mask, "tsdf_frontier_mark: hipMalloc cc_buf");
  if (rc) return rc;
  uint8_t* b = e->cc_buf;
  uint8_t* dstate = b + b_ctl;
  uint32_t* dcost = reinterpret_cast<uint32_t*>(b + b_ctl + b_state);
  uint8_t* dmask = b + b_ctl + b_state + b_cost;
  if (host) {
    HIP_OK(hipMemcpyAsync(dstate, state, n, hipMemcpyHostToDevice, s));
    if (cost) HIP_OK(hipMemcpyAsync(dcost, cost, 4 * n, hipMemcpyHostToDevice, s));
  }
  FrontierArgs A{};
  A.nx = dims[0], A.ny = dims[1], A.nz = dims[2];
  A.state = host ? dstate : state;
  A.cost = cost ? (host ? dcost : cost) : nullptr;
  A.mask = host ? dmask : mask;
  A.ctl = marked ? reinterpret_cast<CcCtl*>(b) : nullptr;
  if (marked) HIP_OK(hipMemsetAsync(b, 0, b_ctl, s));
  hipLaunchKernelGGL(k_frontier_mark, dim3((unsigned)cc_tiles(dims)), dim3(kCcTileVox), 0, s, A);
  LAUNCH_OK("k_frontier_mark");
  CcCtl ctl{};
  if (marked) HIP_OK(hipMemcpyAsync(&ctl, b, sizeof(ctl), hipMemcpyDeviceToHost, s));
  if (host) HIP_OK(hipMemcpyAsync(mask, dmask, n, hipMemcpyDeviceToHost, s));
  if (host || marked) HIP_OK(hipStreamSynchronize(s));
  if (marked) *marked = (int64_t)ctl.marked;
  return TSDF_OK;
}

int tsdf_components(tsdf_engine* e, const tsdf_components_config* cfg, const uint8_t* mask, const uint32_t* key,
                    uint32_t* label, int mem_kind, tsdf_component* clusters, int32_t capacity, int32_t* count,
                    int32_t* total) {
  TraceRange trace_("tsdf_components");
  if (!e || !cfg || !mask || !label || !count || !mem_kind_ok(mem_kind) || !cc_dims_ok(cfg->dims) || cfg->min_size < 1 ||
      capacity < 0 || (capacity > 0 && !clusters)) {
    set_error("tsdf_components: invalid argument (dims 1..2048, at most 2^28 voxels, min_size >= 1, capacity >= 0, "
              "cfg, mask, label and count non-NULL, clusters with capacity > 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  CcArgs A{};
  A.nx = cfg->dims[0], A.ny = cfg->dims[1], A.nz = cfg->dims[2];
  A.tx = (A.nx + kCcTile - 1) >> kCcTileBits, A.ty = (A.ny + kCcTile - 1) >> kCcTileBits, A.tz = (A.nz + kCcTile - 1) >> kCcTileBits;
  const size_t n = (size_t)A.nx * A.ny * A.nz, tiles = cc_tiles(cfg->dims);
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: control words | a slot per voxel | host arrays' staging: mask, key, label | accumulators | records.
  // The last two hold `reserve` components each, a number the call has to choose before it has counted them:
  // one per 512 voxels, or as many as the buffer it finds has room for. A mask with more is labelled once
  // more, into a buffer sized by the count -- the labelling is a function of the mask, so the count stands.
  const size_t b_ctl = up16(sizeof(CcCtl)), b_slot = up16(4 * n), b_mask = host ? up16(n) : 0,
               b_key = host && key ? up16(4 * n) : 0, b_label = host ? up16(4 * n) : 0;
  const size_t b_fixed = b_ctl + b_slot + b_mask + b_key + b_label;
  size_t reserve = std::max(kCcReserveMin, n >> kCcReserveShift);
  if (e->cc_buf.cap > b_fixed) reserve = std::max(reserve, (e->cc_buf.cap - b_fixed) / kCcPerComponent);
  CcCtl ctl{};
  uint8_t* b = nullptr;
  for (int pass = 0;; ++pass) {
    int rc = e->cc_buf.ensure(b_fixed + reserve * kCcPerComponent, "tsdf_components: hipMalloc cc_buf");
    if (rc) return rc;
    b = e->cc_buf;
    A.ctl = reinterpret_cast<CcCtl*>(b);
    A.slot = reinterpret_cast<uint32_t*>(b + b_ctl);
    A.mask = host ? b + b_ctl + b_slot : mask;
    A.key = key ? (host ? reinterpret_cast<const uint32_t*>(b + b_ctl + b_slot + b_mask) : key) : nullptr;
    A.label = host ? reinterpret_cast<uint32_t*>(b + b_ctl + b_slot + b_mask + b_key) : label;
    A.acc = reinterpret_cast<CcAcc*>(b + b_fixed);
    if (host) {
      HIP_OK(hipMemcpyAsync(b + b_ctl + b_slot, mask, n, hipMemcpyHostToDevice, s));
      if (key) HIP_OK(hipMemcpyAsync(b + b_ctl + b_slot + b_mask, key, 4 * n, hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipMemsetAsync(b, 0, b_ctl, s));
    hipLaunchKernelGGL(k_cc_local, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
    LAUNCH_OK("k_cc_local");
    if (tiles > 1) {
      hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
      LAUNCH_OK("k_cc_merge");
    }
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A);
    LAUNCH_OK("k_cc_flatten");
    HIP_OK(hipMemcpyAsync(&ctl, b, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (ctl.total <= reserve) break;
    if (pass > 0) {
      set_error("tsdf_components: two labellings of one mask counted different components");
      return TSDF_ERR_HIP;
    }
    reserve = ctl.total;
  }
  CcRec* drec = reinterpret_cast<CcRec*>(A.acc + reserve * kCcReplicas);
  if (ctl.total > 0) {
    HIP_OK(hipMemsetAsync(A.acc, 0, (size_t)ctl.total * kCcReplicas * sizeof(CcAcc), s));
    hipLaunchKernelGGL(k_cc_stats, dim3((unsigned)tiles), dim3(kCcTileVox), 0, s, A);
    LAUNCH_OK("k_cc_stats");
    hipLaunchKernelGGL(k_cc_emit, dim3((ctl.total + 255u) / 256u), dim3(256), 0, s, A, ctl.total, (uint32_t)cfg->min_size, drec);
    LAUNCH_OK("k_cc_emit");
    HIP_OK(hipMemcpyAsync(&ctl, b, sizeof(ctl), hipMemcpyDeviceToHost, s));
  }
  if (host) HIP_OK(hipMemcpyAsync(label, A.label, 4 * n, hipMemcpyDeviceToHost, s));
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
