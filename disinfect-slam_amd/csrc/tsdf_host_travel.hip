// tsdf_host_travel.hip -- travel field (DESIGN.md "Travel field"; kernels in tsdf_travel.hip):
// tsdf_travel_field and tsdf_travel_paths.
#include <cstdio>
#include <vector>

#include "tsdf_host.h"
#include "tsdf_travel.h"

void tsdf_travel_config_default(tsdf_travel_config* c) {
  if (!c) return;
  *c = tsdf_travel_config{};
}

namespace {

// rounds enqueued between two reads of the control words
constexpr int kTravelBatch = 32;

// TSDF_TRAVEL_LOG=1 (a measurement aid, off by default): one round per batch, and after each round a line
// "tsdf_travel_field: round r tiles n" on stderr -- the tiles listed for that round. The field is the same.
bool travel_log() {
  static const bool on = [] {
    const char* v = std::getenv("TSDF_TRAVEL_LOG");
    return v && v[0] == '1';
  }();
  return on;
}

}  // namespace

int tsdf_travel_field(tsdf_engine* e, const tsdf_travel_config* cfg, const uint16_t* d2, const uint8_t* state,
                      const int32_t* seeds, int32_t S, uint32_t* cost, int mem_kind, int32_t* seeded,
                      int32_t* rounds) {
  TraceRange trace_("tsdf_travel_field");
  if (!e || !cfg || !d2 || !state || !cost || !mem_kind_ok(mem_kind) || !box_dims_ok(cfg->dims) ||
      cfg->clearance2 < 0 || cfg->clearance2 > 255 * 255 || (cfg->unknown_free != 0 && cfg->unknown_free != 1) ||
      S < 0 || (S > 0 && !seeds)) {
    set_error("tsdf_travel_field: invalid argument (" BOX_LIMITS_TEXT ", clearance2 0..65025, "
              "unknown_free 0 or 1, d2, state and cost non-NULL, S >= 0 with seeds)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  TravelArgs A{};
  A.nx = cfg->dims[0], A.ny = cfg->dims[1], A.nz = cfg->dims[2];
  A.tx = box_tiles(A.nx, kTravelTileBits), A.ty = box_tiles(A.ny, kTravelTileBits), A.tz = box_tiles(A.nz, kTravelTileBits);
  A.clearance2 = cfg->clearance2;
  A.unknown_free = cfg->unknown_free;
  const size_t n = box_voxels(cfg->dims), tiles = (size_t)A.tx * A.ty * A.tz;
  const bool host = mem_kind == TSDF_MEM_HOST;
  // sections: control words | stamps | two lists | seeds | host arrays' staging: cost, d2, state
  Sections L;
  const int h_ctl = L.add(sizeof(TravelCtl)), h_stamp = L.add(4 * tiles), h_list0 = L.add(4 * tiles),
            h_list1 = L.add(4 * tiles), h_seeds = L.add((size_t)S * 12);
  const int h_cost = L.add(staged(host, cost, 4 * n)), h_d2 = L.add(staged(host, d2, 2 * n)),
            h_state = L.add(staged(host, state, n));
  int rc = e->tv_buf.ensure(L.total(), "tsdf_travel_field: hipMalloc tv_buf");
  if (rc) return rc;
  const Stage St{L, e->tv_buf.p, host, s};
  A.ctl = L.at<TravelCtl>(St.base, h_ctl);
  A.stamp = L.at<uint32_t>(St.base, h_stamp);
  A.list[0] = L.at<uint32_t>(St.base, h_list0);
  A.list[1] = L.at<uint32_t>(St.base, h_list1);
  int32_t* dseeds = L.at<int32_t>(St.base, h_seeds);
  A.cost = St.ptr(h_cost, cost);
  HIP_OK(St.in(h_d2, d2, 2 * n, &A.d2));
  HIP_OK(St.in(h_state, state, n, &A.state));
  // (the control words and the stamps are one range: sections are contiguous)
  HIP_OK(hipMemsetAsync(A.ctl, 0, L.size(h_ctl) + L.size(h_stamp), s));
  HIP_OK(hipMemsetAsync(A.cost, 0xFF, 4 * n, s));
  if (S > 0) {
    HIP_OK(hipMemcpyAsync(dseeds, seeds, (size_t)S * 12, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_travel_seed, dim3((unsigned)(((int64_t)S + 255) / 256)), dim3(256), 0, s, A, dseeds, (int)S);
    LAUNCH_OK("k_travel_seed");
  }
  // Round k makes every voxel final whose cheapest path crosses fewer than k tile faces, so voxels + 2
  // rounds are more than any field needs. A round that finds no tile listed returns at once, and so does
  // every round after it: the host reads the control words once per batch.
  const dim3 grid((unsigned)std::min<size_t>(tiles, (size_t)kTravelGrid));
  const uint64_t bound = (uint64_t)n + 2;
  TravelCtl ctl{};
  uint64_t r = 0;
  for (;;) {
    if (S > 0) {
      for (int k = 0, nb = travel_log() ? 1 : kTravelBatch; k < nb; ++k)
        hipLaunchKernelGGL(k_travel_round, grid, dim3(512), 0, s, A, (uint32_t)++r);
      LAUNCH_OK("k_travel_round");
    }
    HIP_OK(hipMemcpyAsync(&ctl, A.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (S > 0 && travel_log() && ctl.count[r % 3])
      std::fprintf(stderr, "tsdf_travel_field: round %u tiles %u\n", (unsigned)r, ctl.count[r % 3]);
    if (S == 0 || ctl.count[(r + 1) % 3] == 0) break;
    if (r > bound) {
      set_error("tsdf_travel_field: the rounds passed their bound (voxels + 2) without converging");
      return TSDF_ERR_HIP;
    }
  }
  HIP_OK(St.back(cost, A.cost, 4 * n));
  if (host) HIP_OK(hipStreamSynchronize(s));
  if (seeded) *seeded = (int32_t)ctl.seeded;
  if (rounds) *rounds = (int32_t)ctl.rounds;
  return TSDF_OK;
}

int tsdf_travel_paths(tsdf_engine* e, const int32_t dims[3], const uint32_t* cost, int mem_kind,
                      const int32_t* targets, int32_t T, int32_t max_len, int32_t* path, int32_t* len) {
  TraceRange trace_("tsdf_travel_paths");
  // (a walk visits a voxel once, so a box's voxels bound one target's path: the cap on T * max_len)
  if (!e || !dims || !cost || !mem_kind_ok(mem_kind) || !box_dims_ok(dims) || T < 0 || max_len < 0 ||
      (int64_t)T * max_len > kBoxMaxVoxels || (T > 0 && (!targets || !len || (max_len > 0 && !path)))) {
    set_error("tsdf_travel_paths: invalid argument (" BOX_LIMITS_TEXT ", T >= 0, max_len >= 0, "
              "T * max_len <= 2^28, cost, targets, path and len non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (T == 0) return TSDF_OK;
  if (mem_kind == TSDF_MEM_HOST) {
    for (int32_t t = 0; t < T; ++t)
      len[t] = travel_walk(cost, dims[0], dims[1], dims[2], targets[3 * (size_t)t], targets[3 * (size_t)t + 1],
                           targets[3 * (size_t)t + 2], max_len, path + (size_t)t * (size_t)max_len);
    return TSDF_OK;
  }
  HIP_OK(hipSetDevice(e->device));
  hipStream_t s = e->stream;
  // sections: targets | lengths | paths
  const size_t b_p = (size_t)T * (size_t)max_len * 4;
  Sections L;
  const int h_t = L.add((size_t)T * 12), h_l = L.add((size_t)T * 4), h_p = L.add(b_p);
  int rc = e->tv_buf.ensure(L.total(), "tsdf_travel_paths: hipMalloc tv_buf");
  if (rc) return rc;
  uint8_t* b = e->tv_buf;
  int32_t* dt = L.at<int32_t>(b, h_t);
  int32_t* dl = L.at<int32_t>(b, h_l);
  int32_t* dp = L.at<int32_t>(b, h_p);
  HIP_OK(hipMemcpyAsync(dt, targets, (size_t)T * 12, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_travel_paths, dim3((unsigned)((T + 63) / 64)), dim3(64), 0, s, cost, dims[0], dims[1], dims[2],
                     dt, (int)T, max_len, dp, dl);
  LAUNCH_OK("k_travel_paths");
  // (a walk writes min(|len|, max_len) entries of its row: the rest of the caller's row stays as it was)
  std::vector<int32_t> rows((size_t)T * (size_t)max_len);
  HIP_OK(hipMemcpyAsync(len, dl, (size_t)T * 4, hipMemcpyDeviceToHost, s));
  if (b_p) HIP_OK(hipMemcpyAsync(rows.data(), dp, b_p, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (int32_t t = 0; t < T; ++t) {
    const int64_t k = std::min<int64_t>(len[t] < 0 ? -(int64_t)len[t] : (int64_t)len[t], max_len);
    std::copy_n(rows.data() + (size_t)t * (size_t)max_len, (size_t)k, path + (size_t)t * (size_t)max_len);
  }
  return TSDF_OK;
}
