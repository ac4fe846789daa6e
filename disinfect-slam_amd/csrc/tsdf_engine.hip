// tsdf_engine.hip -- the core of the engine's host side: error state, environment knobs, create /
// destroy / synchronize, stream ordering, stats and profiling. The rest of the C ABI declared in
// include/disinfect_tsdf.h lives in the tsdf_host_*.hip files, one subsystem each; tsdf_host.h is
// what they share. No HIP type crosses the ABI, and none of these files defines a kernel.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "tsdf_host.h"

static thread_local std::string g_last_error;

void set_error(const char* what, hipError_t e) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  g_last_error = buf;
}
void set_error(const char* what) { g_last_error = what; }

// ---------------------------------------------------------------------------------------------
// Environment knobs: A/B experiments and tests only (the defaults are the measured best; nothing a
// drop-in caller needs to set). Read once by tsdf_create (read_env_knobs); every other file reads
// none. TSDF_ROCTX (roctx ranges) is read on first use by the tracing wrapper.
//   TSDF_PIPELINE=0               unpipelined frames: two launches per frame (k_ingest_dda, k_integrate)
//   TSDF_PIPE_MAX_PIXELS=n        largest frame (pixels) that is pipelined (default 2^20: C4, 1280x720, is within it)
//   TSDF_FRAME_ORDER=0..2         k_frame grid order of its parts (PipeArgs.order; default 2)
//   TSDF_FRAME_UPD_WGS=n          (A/B) k_frame update workgroups in total (default kFrameUpdWgsPer4Cu / 4 = 3 per CU: 768)
//   TSDF_CAND_CAP=n               (tests) smaller carve-candidate list, to exercise its overflow
//   TSDF_MESH_GRID=n              (tests) fewer k_mesh workgroups, to exercise its grid stride
//   TSDF_FREE_CULL=0              (A/B, tests) tsdf_free_observe without its two culls (full words, bricks outside the frustum)
//   TSDF_VIEW_SKIP=0              (A/B, tests) tsdf_view_gain with the plain march (no ray / box cut) and no per-view brick cull
// ---------------------------------------------------------------------------------------------
static EnvKnobs read_env_knobs() {
  EnvKnobs k;
  auto num = [](const char* n, long long dflt) {
    const char* v = std::getenv(n);
    return v ? std::atoll(v) : dflt;
  };
  if (const char* v = std::getenv("TSDF_PIPELINE")) k.pipeline = v[0] != '0';
  if (const char* v = std::getenv("TSDF_FREE_CULL")) k.free_cull = v[0] != '0';
  if (const char* v = std::getenv("TSDF_VIEW_SKIP")) k.view_skip = v[0] != '0';
  k.pipe_max_pixels = num("TSDF_PIPE_MAX_PIXELS", -1);
  k.frame_order = (int)std::max(-1ll, num("TSDF_FRAME_ORDER", -1));
  k.frame_upd_wgs = (int)num("TSDF_FRAME_UPD_WGS", 0);
  k.cand_cap = (int)num("TSDF_CAND_CAP", 0);
  k.mesh_grid = (int)num("TSDF_MESH_GRID", 0);
  return k;
}

tsdf_engine::~tsdf_engine() {
  void* ptrs[] = {D.pipe,  D.ctag,  D.rtag,     D.fo,       D.table,   D.lock_tag, D.heap,      D.pool,
                  D.occ,   D.ctr,   D.nk_key,   D.nk_order, D.nk_list, D.pairs,    D.fresh,     D.vis,
                  D.band,  D.cand,  D.arrive,   D.swdirty,  D.fresh_vis, D.pend,   D.pixA,      D.pixC,
                  D.visbits, D.wgcnt, D.dbg};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (h_ctr) (void)hipHostFree(h_ctr);
  if (uv_h) (void)hipHostFree(uv_h);
  if (uv_ev) (void)hipEventDestroy(uv_ev);
  if (pl_h) (void)hipHostFree(pl_h);
  if (pl_ev) (void)hipEventDestroy(pl_ev);
  for (auto& ev : events)
    for (hipEvent_t x : ev) (void)hipEventDestroy(x);
  if (order_ev) (void)hipEventDestroy(order_ev);
  for (int j = 0; j < kUpStreams; ++j) {
    if (ustream[j]) (void)hipStreamDestroy(ustream[j]);
    for (int k = 0; k < 2; ++k)
      if (up_done[k][j]) (void)hipEventDestroy(up_done[k][j]);
  }
  for (int k = 0; k < 2; ++k)
    if (up_free[k]) (void)hipEventDestroy(up_free[k]);
  if (own_stream && stream) (void)hipStreamDestroy(stream);
}

FrameParams make_params(const tsdf_engine* e, const tsdf_intrinsics* K, int W, int H,
                        const tsdf_pose* p, float max_depth) {
  FrameParams P{};
  P.fx = K->fx;
  P.fy = K->fy;
  P.cx = K->cx;
  P.cy = K->cy;
  P.ifx = 1.0f / K->fx;  // CameraIntrinsics::Inverse (camera.cuh:34-39)
  P.ify = 1.0f / K->fy;
  P.icx = -K->cx * P.ifx;
  P.icy = -K->cy * P.ify;
  P.cq = {p->qx, p->qy, p->qz, p->qw};
  P.ct = {p->tx, p->ty, p->tz};
  // SE3::Inverse on the host (lie_group.cuh:22-24); squaredNorm as a Packet4f reduction
  const float n2 = (p->qx * p->qx + p->qz * p->qz) + (p->qy * p->qy + p->qw * p->qw);
  if (n2 > 0.0f)
    P.wq = {-p->qx / n2, -p->qy / n2, -p->qz / n2, p->qw / n2};
  else
    P.wq = {0.f, 0.f, 0.f, 0.f};
  const f3 nt = {-p->tx, -p->ty, -p->tz};
  P.wt = h_qrot(P.wq, nt);
  P.voxel = e->cfg.voxel_size;
  P.trunc = e->cfg.truncation;
  P.inv_trunc = 1.0f / e->cfg.truncation;
  P.inv_voxel = 1.0f / e->cfg.voxel_size;
  P.inv_max_depth = 1.0f / max_depth;
  P.max_depth = max_depth;
  P.W = W;
  P.H = H;
  P.maxs = e->maxs;
  P.shard_index = e->cfg.shard_index;
  P.shard_count = e->cfg.shard_count;
  P.tile_lo = 0;
  P.tile_hi = 1 << 30;
  P.tail = kTailResolve;
  P.slot_cap = 0;
  P.slot = nullptr;
  P.pack_pixels = 1;
  P.row0 = 0;
  P.nrows = H;
  P.depth = nullptr;
  P.rgb = nullptr;
  P.ht = nullptr;
  P.lt = nullptr;
  P.pix_off = 0;  // pixel-record buffer 0 (a pipelined frame may take buffer 1)
  return P;
}

// launches what an earlier call left pending: a batched graph's frames, then the deferred raycasts
// (keep_deferred: a deferred raycast stays pending -- tsdf_stream_wait orders the engine stream after
// another stream's work, which the raycast may follow as well; keep_graph: the graph frame that
// renders rdg itself calls)
int join_render(tsdf_engine* e, bool keep_deferred, bool keep_graph) {
  if (e->gbatch) {  // the frames of a batched graph not launched yet, before anything else
    int rc = graph_flush_batch(e->gbatch);
    if (rc) return rc;
  }
  if (e->rdg.pending && !keep_deferred && !keep_graph) {  // (a graph frame's deferred raycast: its args slot)
    e->rdg.pending = false;
    const dim3 rgrid((e->rdg.W + 15) / 16, (e->rdg.H + 15) / 16);
    hipLaunchKernelGGL(k_raycast_g, rgrid, dim3(256), 0, e->stream, e->D, e->rdg.args);
    HIP_OK(hipGetLastError());
  }
  if (e->rd.pending && !keep_deferred) {  // a deferred raycast no ingest took up: launched alone, before anything else
    e->rd.pending = false;
    const tsdf_engine::DeferredRender& r = e->rd;
    const dim3 rgrid((r.P.W + 15) / 16, (r.P.nrows + 15) / 16);
    hipLaunchKernelGGL(k_raycast, rgrid, dim3(256), (size_t)r.V.nw * 4, e->stream, e->D, r.P, r.step, r.V, r.rgba,
                       r.normal);
    HIP_OK(hipGetLastError());
  }
  return TSDF_OK;
}

int read_counters(tsdf_engine* e) {
  ENTER(e);
  HIP_OK(hipMemcpyAsync(e->h_ctr, e->D.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

void tsdf_config_default(tsdf_config* c) {
  if (!c) return;
  c->voxel_size = 0.005f;
  c->truncation = 0.03f;
  c->max_width = 1920;
  c->max_height = 1080;
  c->num_block_bits = 18;
  c->shard_index = 0;
  c->shard_count = 1;
  c->stream = nullptr;
  c->use_stream = 0;
}

const char* tsdf_error_string(int code) {
  switch (code) {
    case TSDF_OK: return "ok";
    case TSDF_ERR_INVALID_ARG: return "invalid argument";
    case TSDF_ERR_OUT_OF_MEMORY: return "out of device memory";
    case TSDF_ERR_HIP: return "HIP runtime error";
    case TSDF_ERR_CAPACITY: return "output buffer too small";
    case TSDF_ERR_NO_DEVICE: return "no HIP device";
    case TSDF_ERR_PIPELINE: return "pipelined frame wait timed out";
    default: return "unknown error";
  }
}
const char* tsdf_last_error(void) { return g_last_error.c_str(); }
void tsdf_set_last_error(const char* what) { g_last_error = what ? what : ""; }

uint32_t tsdf_hash_block(int16_t x, int16_t y, int16_t z) { return hash_block(x, y, z); }
int32_t tsdf_block_owner(int16_t x, int16_t y, int16_t z, int32_t n) {
  return (int32_t)brick_owner(x, y, z, (uint32_t)(n < 1 ? 1 : n));
}
int32_t tsdf_num_entries(void) { return (int32_t)kNumEntry; }
int32_t tsdf_num_blocks(const tsdf_engine* e) { return e ? e->D.nblocks : 0; }

// empty volume: table, occupancy, free stack, voxel pool, counters and key sets (tsdf_create,
// tsdf_reset); with_pool false leaves the voxel pool as it is (tsdf_import_blocks replace: every
// block that becomes live is written by the import, free blocks are never read)
bool init_state(tsdf_engine* e, bool with_pool) {
  hipStream_t s = e->stream;
  const EngineDev& D = e->D;
  const int nb = D.nblocks;
  bool ok = true;
  ok &= hipMemsetAsync(D.lock_tag, 0, sizeof(uint32_t) * kNumBucket, s) == hipSuccess;
  if (with_pool) ok &= hipMemsetAsync(D.pool, 0, (size_t)nb * kBlockBytes, s) == hipSuccess;
  ok &= hipMemsetAsync(D.occ, 0, sizeof(unsigned long long) * kOccWords, s) == hipSuccess;
  ok &= hipMemsetAsync(D.nk_key, 0, sizeof(unsigned long long) * kNewKeyCap, s) == hipSuccess;
  ok &= hipMemsetAsync(D.nk_order, 0xFF, sizeof(uint32_t) * kNewKeyCap, s) == hipSuccess;
  ok &= hipMemsetAsync(D.band, 0, sizeof(int32_t) * 3 * kBands * kBandStride, s) == hipSuccess;
  ok &= hipMemsetAsync(D.pipe, 0, sizeof(unsigned long long) * kPipeWords, s) == hipSuccess;
  ok &= hipMemsetAsync(D.ctag, 0, sizeof(uint32_t) * 2 * (size_t)nb, s) == hipSuccess;
  ok &= hipMemsetAsync(D.rtag, 0, sizeof(uint32_t) * (size_t)nb, s) == hipSuccess;
  ok &= hipMemsetAsync(D.fo, 0xFF, sizeof(unsigned long long) * (size_t)kNumEntry, s) == hipSuccess;
  ok &= hipMemsetAsync(D.visbits, 0, sizeof(unsigned long long) * kOccWords, s) == hipSuccess;
  ok &= hipMemsetAsync(D.arrive, 0, sizeof(unsigned long long) * kArriveWords, s) == hipSuccess;
  ok &= hipMemsetAsync(D.swdirty, 0, sizeof(unsigned long long) * (kOccWords / 64), s) == hipSuccess;
  DevCounters c0{};
  c0.free_count = nb;
  ok &= hipMemcpyAsync(D.ctr, &c0, sizeof(c0), hipMemcpyHostToDevice, s) == hipSuccess;
  hipLaunchKernelGGL(k_init_table, dim3(kNumEntry / 256), dim3(256), 0, s, D.table);
  hipLaunchKernelGGL(k_init_heap, dim3((nb + 255) / 256), dim3(256), 0, s, D.heap, nb);
  if (with_pool)
    hipLaunchKernelGGL(k_init_prob, dim3((unsigned)(((size_t)nb * (kBlockVolume / 4) + 255) / 256)),
                       dim3(256), 0, s, D.pool, nb);
  ok &= hipGetLastError() == hipSuccess;
  ok &= hipStreamSynchronize(s) == hipSuccess;
  return ok;
}

int tsdf_create(const tsdf_config* cfg_in, int device, tsdf_engine** out) {
  if (!out) return TSDF_ERR_INVALID_ARG;
  *out = nullptr;
  tsdf_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    tsdf_config_default(&cfg);
  if (!(cfg.voxel_size > 0) || !(cfg.truncation > 0) || cfg.max_width <= 0 ||
      cfg.max_height <= 0 || cfg.num_block_bits < 1 || cfg.num_block_bits > 22 ||
      cfg.shard_count < 1 || cfg.shard_count > kMaxShards || cfg.shard_index < 0 ||
      cfg.shard_index >= cfg.shard_count) {
    set_error("tsdf_create: invalid config");
    return TSDF_ERR_INVALID_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    set_error("tsdf_create: no such HIP device");
    return TSDF_ERR_NO_DEVICE;
  }
  HIP_OK(hipSetDevice(device));
  tsdf_engine* e = new tsdf_engine();
  e->cfg = cfg;
  e->env = read_env_knobs();
  e->device = device;
  // DDA samples per pixel: step_grid = ceil(max|2 trunc dir / voxel| / 8) + 1 (voxel_tsdf.cu:136)
  e->maxs = (int)std::ceil(2.0 * cfg.truncation / cfg.voxel_size * 1.0001 / kBlockLen) + 1;
  e->max_pixels = (int64_t)cfg.max_width * cfg.max_height;
  e->order_range = e->max_pixels * e->maxs;
  if (e->maxs > kMaxDdaSamples || e->order_range > kMaxOrderRange) {
    delete e;
    set_error("tsdf_create: truncation / voxel ratio or image size beyond the supported "
              "candidate order space (maxs <= 6, width*height*maxs <= 8M)");
    return TSDF_ERR_INVALID_ARG;
  }
  const int nb = 1 << cfg.num_block_bits;
  EngineDev& D = e->D;
  D.nblocks = nb;
  auto fail = [&](int code) {  // (this device is current: hipSetDevice above)
    delete e;
    return code;
  };
#define ALLOC(ptr, n)                                 \
  do {                                                \
    hipError_t _e = dmalloc(&(ptr), (size_t)(n));     \
    if (_e != hipSuccess) {                           \
      set_error("tsdf_create: hipMalloc " #ptr, _e);  \
      return fail(TSDF_ERR_OUT_OF_MEMORY);            \
    }                                                 \
  } while (0)
#define SCRATCH(buf, n) \
  if ((buf).ensure((size_t)(n), "tsdf_create: hipMalloc " #buf)) return fail(TSDF_ERR_OUT_OF_MEMORY)
  ALLOC(D.table, kNumEntry);
  ALLOC(D.lock_tag, kNumBucket);
  ALLOC(D.heap, nb);
  ALLOC(D.pool, (size_t)nb * kBlockBytes);
  ALLOC(D.occ, kOccWords);
  ALLOC(D.ctr, 1);
  ALLOC(D.nk_key, kNewKeyCap);
  ALLOC(D.nk_order, kNewKeyCap);
  ALLOC(D.nk_list, kNewKeyCap);
  ALLOC(D.pairs, std::max<size_t>(kNewKeyCap, (size_t)nb));
  ALLOC(D.fresh, kNewKeyCap);
  // two frames' visible lists, three frames' band counts (pipelined frames: frame_view)
  ALLOC(D.vis, (size_t)2 * kBands * nb);
  ALLOC(D.band, 3 * kBands * kBandStride);
  ALLOC(D.pipe, kPipeWords);
  ALLOC(D.ctag, (size_t)2 * nb);
  ALLOC(D.rtag, nb);
  ALLOC(D.fo, kNumEntry);
  // carve candidates of one frame: a shard's list takes every shard's (their visible blocks and the
  // entries exhausted pools left without voxels), so it is sized like the resolver's D.pairs scratch;
  // more are clamped with TSDF_STATUS_SHARD_OVERFLOW. TSDF_CAND_CAP (tests) sets a smaller list.
  D.cand_cap = (int32_t)std::max<size_t>(kNewKeyCap, (size_t)nb);
  if (e->env.cand_cap > 0) D.cand_cap = std::min(D.cand_cap, std::max(1024, e->env.cand_cap));
  ALLOC(D.cand, (size_t)2 * D.cand_cap);  // two frames' lists (frame_view)
  ALLOC(D.arrive, kArriveWords);
  ALLOC(D.swdirty, kOccWords / 64);
  ALLOC(D.fresh_vis, kNewKeyCap);
  ALLOC(D.pend, kNewKeyCap);
  {  // one resident wave of k_integrate workgroups: no second-round stragglers
    int per_cu = 0, ncu = 0;
    // (a shard's raw-frame variant is sized by its own occupancy)
    const void* kfn = cfg.shard_count > 1 ? reinterpret_cast<const void*>(k_integrate_t<false, true>)
                                          : reinterpret_cast<const void*>(k_integrate_t<false, false>);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, kIntegrateThreads, 0) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
      return fail(TSDF_ERR_HIP);
    D.integrate_grid = std::max(8, std::min(kIntegrateGrid, (per_cu * ncu) & ~7));
    int per_cu_pre = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_pre, reinterpret_cast<const void*>(k_frame),
                                                     kIntegrateThreads, 0) != hipSuccess)
      return fail(TSDF_ERR_HIP);
    // 3 update workgroups per CU by default (of 7 that fit): the other slots take the sweep's and
    // the tile pairs' workgroups from the start. Round 11 (7 waves per SIMD, 1,792 slots; same box,
    // interleaved, 3 runs, driver command / 300 frames): 704 24.88-24.97k / 28.26-28.39k frames/s, 768
    // 26.56-26.88k / 28.97-29.12k, 832 24.55-24.64k / 28.52-29.08k, 896 25.90-26.09k / 27.71-29.25k
    // (profiles/ab/r11_upd_wgs_ab.txt). Round 7, at 6 waves and 2.75 per CU (tile pairs, 600 tile workgroups at 640x480;
    // same box, interleaved, driver command / 300 frames): 704 21.21-21.26k / 24.86-25.01k frames/s,
    // 640 20.69-20.91k / 24.42-24.68k, 608 20.39-20.55k / 24.40-24.48k (the parent, 1,200 tile workgroups
    // and 640: 20.93-21.13k / 23.29-23.52k; profiles/ab/r7_tile_pairs_ab.txt). Round 6, final build (exact semantic chain, 6 waves per
    // SIMD, no packed fp32): 640 update workgroups 20.94-20.99k frames/s on the driver command, 704
    // 20.8-21.0k, 768 20.6k, 896 20.2k (profiles/ab/r6_upd_wgs_nopk_ab.txt); with packed fp32 768 was
    // ahead (19.6k vs 18.7-19.4k at 640). Round 5 (log-odds state, 7 waves): 640 23.9k, 768
    // 23.3-23.5k, 512 23.4-23.7k; earlier rounds: 4 per CU 22.0-22.5k, 5 21.0-21.3k, 7 18.5-18.7k
    int upd = kFrameUpdWgsPer4Cu * ncu / 4;
    if (e->env.frame_upd_wgs > 0) upd = e->env.frame_upd_wgs;
    D.integrate_grid_pre = std::max(8, std::min({kIntegrateGrid, upd, per_cu_pre * ncu}) & ~7);
  }
  ALLOC(D.pixA, 2 * e->max_pixels);  // two buffers: a pipelined frame's and the next one's
  ALLOC(D.pixC, 2 * e->max_pixels);
  e->pipeline = e->env.pipeline;
  if (e->env.pipe_max_pixels >= 0) e->pipe_max_pixels = e->env.pipe_max_pixels;
  if (e->env.frame_order >= 0) e->frame_order = std::min(2, e->env.frame_order);
  ALLOC(D.visbits, kOccWords);
  ALLOC(D.wgcnt, kOccWords / 256);
  ALLOC(D.dbg, (size_t)kDiagKernels * kDiagMaxWg * kDiagStamps);
  if (hipMemset(D.dbg, 0, (size_t)kDiagKernels * kDiagMaxWg * kDiagStamps * 8) != hipSuccess)
    return fail(TSDF_ERR_HIP);
  SCRATCH(e->s_rgb, 2 * e->max_pixels * 3);  // two upload slots (host frames)
  SCRATCH(e->s_depth, 2 * e->max_pixels);
  SCRATCH(e->s_ht, 2 * e->max_pixels);
  SCRATCH(e->s_lt, 2 * e->max_pixels);
  SCRATCH(e->rc_rgba, e->max_pixels);
  SCRATCH(e->rc_norm, e->max_pixels);
  SCRATCH(e->vg_flags, (size_t)kViewBitmapWords * 32);
  SCRATCH(e->vg_bits, kViewBitmapWords);
  if (hipMemset(e->vg_flags, 0, (size_t)kViewBitmapWords * 32) != hipSuccess)
    return fail(TSDF_ERR_HIP);
  SCRATCH(e->q_sel, nb);
  SCRATCH(e->q_count, 1);
  SCRATCH(e->m_counts, nb);
  SCRATCH(e->m_offsets, nb);
  SCRATCH(e->m_total, 1);
  SCRATCH(e->m_nbr, (size_t)27 * nb);
  e->mesh_grid = std::min(kMeshGrid, nb);
  if (e->env.mesh_grid > 0) e->mesh_grid = std::min(e->mesh_grid, e->env.mesh_grid);
  SCRATCH(e->t_count, 1);
#undef ALLOC
#undef SCRATCH
  D = frame_view(D, 0u);  // the base view (sharded / graph / hash-level paths): frame parity 0
  if (hipHostMalloc(reinterpret_cast<void**>(&e->h_ctr), sizeof(DevCounters)) != hipSuccess)
    return fail(TSDF_ERR_OUT_OF_MEMORY);
  if (cfg.use_stream) {  // the caller's stream; NULL is the legacy default stream (torch's default)
    e->stream = reinterpret_cast<hipStream_t>(cfg.stream);
  } else {
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess)
      return fail(TSDF_ERR_HIP);
    e->own_stream = true;
  }
  for (int j = 0; j < tsdf_engine::kUpStreams; ++j) {
    if (hipStreamCreateWithFlags(&e->ustream[j], hipStreamNonBlocking) != hipSuccess)
      return fail(TSDF_ERR_HIP);
    for (int k = 0; k < 2; ++k)
      if (hipEventCreateWithFlags(&e->up_done[k][j], hipEventDisableTiming) != hipSuccess)
        return fail(TSDF_ERR_HIP);
  }
  for (int k = 0; k < 2; ++k)
    if (
        hipEventCreateWithFlags(&e->up_free[k], hipEventDisableTiming) != hipSuccess)
      return fail(TSDF_ERR_HIP);
  if (!init_state(e)) {
    set_error("tsdf_create: initialisation failed");
    return fail(TSDF_ERR_HIP);
  }
  *out = e;
  return TSDF_OK;
}

int tsdf_destroy(tsdf_engine* e) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  (void)hipSetDevice(e->device);
  (void)join_render(e);  // (a deferred raycast's outputs are still written)
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  delete e;
  return TSDF_OK;
}

int tsdf_synchronize(tsdf_engine* e) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  // a pipelined frame whose in-kernel wait timed out has wrong results: an error here, not only a
  // status bit. The status word is read on the engine stream into the pinned counter
  // mirror (no device-wide sync); the timeout bit is reported once and then cleared, so the next
  // synchronize reports only a new timeout (the flags are per-launch tags: later launches are not
  // affected). TSDF_STATUS_PIPELINE_TIMEOUT stays visible in tsdf_get_stats until then.
  HIP_OK(hipMemcpyAsync(&e->h_ctr->status, &e->D.ctr->status, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  if (e->h_ctr->status & TSDF_STATUS_PIPELINE_TIMEOUT) {
    const uint32_t st = e->h_ctr->status & ~(uint32_t)TSDF_STATUS_PIPELINE_TIMEOUT;
    HIP_OK(hipMemcpyAsync(&e->D.ctr->status, &st, sizeof(st), hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    set_error("tsdf_synchronize: a pipelined frame's in-kernel wait timed out (TSDF_STATUS_PIPELINE_TIMEOUT)");
    return TSDF_ERR_PIPELINE;
  }
  return TSDF_OK;
}

int tsdf_stream_wait(tsdf_engine* e, void* stream) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  hipStream_t other = reinterpret_cast<hipStream_t>(stream);
  if (other == e->stream) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  int rc = join_render(e, true);
  if (rc) return rc;
  if (!e->order_ev) HIP_OK(hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(e->order_ev, other));
  HIP_OK(hipStreamWaitEvent(e->stream, e->order_ev, 0));
  return TSDF_OK;
}

int tsdf_stream_signal(tsdf_engine* e, void* stream) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  hipStream_t other = reinterpret_cast<hipStream_t>(stream);
  if (other == e->stream) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  JOIN_RENDER(e);
  if (!e->order_ev) HIP_OK(hipEventCreateWithFlags(&e->order_ev, hipEventDisableTiming));
  HIP_OK(hipEventRecord(e->order_ev, e->stream));
  HIP_OK(hipStreamWaitEvent(other, e->order_ev, 0));
  return TSDF_OK;
}

int tsdf_get_stream(tsdf_engine* e, void** stream) {
  if (!e || !stream) return TSDF_ERR_INVALID_ARG;
  *stream = reinterpret_cast<void*>(e->stream);
  return TSDF_OK;
}

int tsdf_get_stats(tsdf_engine* e, tsdf_stats* o, int clear_status) {
  if (!e || !o) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  int rc = read_counters(e);
  if (rc) return rc;
  const DevCounters& c = *e->h_ctr;
  std::memset(o, 0, sizeof(*o));
  o->frames = (int64_t)c.frames;
  o->free_blocks = c.free_count;
  o->active_blocks = e->D.nblocks - c.free_count;
  o->last_num_visible = c.n_vis;
  o->last_num_alloc = c.last_alloc;
  o->last_num_deleted = c.last_deleted;
  o->last_num_new_keys = c.last_new_keys;
  o->last_num_updated = (int64_t)c.last_updated;
  o->total_visible = (int64_t)c.total_visible;
  o->total_updated = (int64_t)c.total_updated;
  o->total_alloc = (int64_t)c.total_alloc;
  o->total_deleted = (int64_t)c.total_deleted;
  o->status = c.status;
  if (clear_status && c.status) {
    HIP_OK(hipMemsetAsync(&e->D.ctr->status, 0, sizeof(uint32_t), e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
  }
  return TSDF_OK;
}

int tsdf_profile_begin(tsdf_engine* e, int mode, int every) {
  if (!e || (mode != TSDF_PROFILE_PHASES && mode != TSDF_PROFILE_INTEGRATE &&
             mode != TSDF_PROFILE_KERNEL) || every < 1)
    return TSDF_ERR_INVALID_ARG;
  e->prof_mode = mode;
  e->prof_every = every;
  e->prof_calls = 0;
  e->prof_pipelined = 0;
  int rc = read_counters(e);
  if (rc) return rc;
  e->prof_vis0 = e->h_ctr->total_visible;
  e->prof_upd0 = e->h_ctr->total_updated;
  e->prof_ticks0 = e->h_ctr->integrate_ticks;
  e->prof_ing0 = e->h_ctr->ingest_ticks;
  e->prof_ra0 = e->h_ctr->resolve_alloc_ticks;
  e->prof_rd0 = e->h_ctr->resolve_delete_ticks;
  e->ev_used = 0;
  e->profiling = true;
  return TSDF_OK;
}

int tsdf_profile_end(tsdf_engine* e, tsdf_profile* o) {
  if (!e || !o) return TSDF_ERR_INVALID_ARG;
  e->profiling = false;
  int rc = read_counters(e);
  if (rc) return rc;
  std::memset(o, 0, sizeof(*o));
  o->frames = (int64_t)e->ev_used;
  o->calls = e->prof_calls;
  o->pipelined = e->prof_pipelined;
  for (size_t i = 0; i < e->ev_used; ++i) {
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; ++k)
      if (e->prof_mode == TSDF_PROFILE_PHASES || k == 2)
        HIP_OK(hipEventElapsedTime(&ms[k], e->events[i][k], e->events[i][k + 1]));
    o->ms_allocate += ms[0];
    o->ms_visible += ms[1];
    o->ms_integrate += ms[2];
    o->ms_carve += ms[3];
  }
  o->sum_visible = (int64_t)(e->h_ctr->total_visible - e->prof_vis0);
  o->sum_updated = (int64_t)(e->h_ctr->total_updated - e->prof_upd0);
  o->ms_integrate_device = (double)(e->h_ctr->integrate_ticks - e->prof_ticks0) * 1e-5;
  o->ms_ingest_device = (double)(e->h_ctr->ingest_ticks - e->prof_ing0) * 1e-5;
  o->ms_resolve_alloc_device = (double)(e->h_ctr->resolve_alloc_ticks - e->prof_ra0) * 1e-5;
  o->ms_resolve_delete_device = (double)(e->h_ctr->resolve_delete_ticks - e->prof_rd0) * 1e-5;
  return TSDF_OK;
}

int tsdf_debug_stamps(tsdf_engine* e, uint64_t* out, int64_t capacity, int* enabled) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  // (no flush of pending pipelined frames: the stamps are those of the launches so far)
#ifdef TSDF_DIAG_STAMPS
  if (enabled) *enabled = 1;
#else
  if (enabled) *enabled = 0;
#endif
  const int64_t n = (int64_t)kDiagKernels * kDiagMaxWg * kDiagStamps;
  if (!out) return TSDF_OK;
  if (capacity < n) {
    set_error("tsdf_debug_stamps: capacity too small");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipStreamSynchronize(e->stream));
  HIP_OK(hipMemcpy(out, e->D.dbg, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemset(e->D.dbg, 0, n * sizeof(uint64_t)));
  return TSDF_OK;
}
