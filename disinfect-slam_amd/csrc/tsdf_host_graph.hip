// tsdf_host_graph.hip -- tsdf_graph and the tsdf_graph_* entry points.
#include <cstring>

#include "tsdf_host.h"

// ---------------------------------------------------------------------------------------------
// Graph-captured frame loop (BASELINE config C5): the whole per-frame sequence -- argument upload,
// k_ingest_dda, k_resolve_alloc, k_integrate, k_resolve_delete and (optionally) k_raycast -- is one
// hipGraph launch. The graph's first node copies a FrameArgs block (cameras, frame and output
// pointers) from a pinned host slot, so one instantiated graph serves every frame; kSlots graphs
// with their own slots let the host fill frame i+1 while frame i runs.
// ---------------------------------------------------------------------------------------------
#ifndef TSDF_GRAPH_DONE_FLAGS
#define TSDF_GRAPH_DONE_FLAGS hipEventDisableTiming
#endif
constexpr unsigned kGraphDoneFlags = TSDF_GRAPH_DONE_FLAGS;
struct tsdf_graph {
  static constexpr int kSlots = 4;
  static constexpr int kSegs = 3;  // a shard's frame: begin / update / end around the exchanges
  tsdf_engine* e = nullptr;
  int W = 0, H = 0, RW = 0, RH = 0;
  bool shard = false;     // a shard engine's graph (tsdf_graph_create_shard)
  bool pipe = false;      // pipelined frames: each launch is one k_frame_g (no render camera)
  bool defer = false;     // render-deferring graph (tsdf_graph_create_deferred): each launch renders the
                          // previous frame's camera beside its ingest (k_render_ingest_g)
  int slice_index = 0, slice_count = 1;
  int cur = -1;           // a shard's frame in flight: its slot
  hipStream_t cap = nullptr;  // capture stream (the engine stream may be a legacy default stream)
  FrameArgs* d_args = nullptr;
  FrameArgs* h_args = nullptr;  // pinned
  hipGraph_t graph[kSlots][kSegs] = {};
  hipGraphExec_t exec[kSlots][kSegs] = {};
  hipEvent_t done[kSlots] = {};
  bool used[kSlots] = {};
  int next = 0;
  // batched graphs (tsdf_graph_create_batch): slot k's graph runs `batch` frames, args entries
  // [k batch, (k + 1) batch); one[k][j] runs entry j alone (a batch launched before it is full)
  static constexpr int kMaxBatch = 32;
  int batch = 1;
  int fill = 0;           // frames of the current slot's batch written, not launched
  hipGraph_t one_g[kSlots][kMaxBatch] = {};
  hipGraphExec_t one[kSlots][kMaxBatch] = {};
};

namespace {

void graph_free(tsdf_graph* g) {
  if (g->e && g->e->gbatch == g) g->e->gbatch = nullptr;
  for (int i = 0; i < tsdf_graph::kSlots; ++i) {
    for (int j = 0; j < tsdf_graph::kSegs; ++j) {
      if (g->exec[i][j]) (void)hipGraphExecDestroy(g->exec[i][j]);
      if (g->graph[i][j]) (void)hipGraphDestroy(g->graph[i][j]);
    }
    for (int j = 0; j < tsdf_graph::kMaxBatch; ++j) {
      if (g->one[i][j]) (void)hipGraphExecDestroy(g->one[i][j]);
      if (g->one_g[i][j]) (void)hipGraphDestroy(g->one_g[i][j]);
    }
    if (g->done[i]) (void)hipEventDestroy(g->done[i]);
  }
  if (g->d_args) (void)hipFree(g->d_args);
  if (g->h_args) (void)hipHostFree(g->h_args);
  if (g->cap) (void)hipStreamDestroy(g->cap);
  delete g;
}

int graph_create(tsdf_engine* e, int width, int height, int render_width, int render_height, bool defer,
                 tsdf_graph** out, int batch = 1) {
  if (e && e->cfg.shard_count > 1) {
    set_error("tsdf_graph_create: a shard's graph frames are tsdf_graph_create_shard / tsdf_graph_shard_*");
    return TSDF_ERR_INVALID_ARG;
  }
  if (!e || !out || width <= 0 || height <= 0 || width > e->cfg.max_width || height > e->cfg.max_height ||
      render_width < 0 || render_height < 0 || (int64_t)render_width * render_height > e->max_pixels ||
      (render_width == 0) != (render_height == 0) || batch < 1 || batch > tsdf_graph::kMaxBatch) {
    set_error("tsdf_graph_create: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  auto* g = new tsdf_graph();
  g->batch = batch;
  g->e = e;
  g->W = width;
  g->H = height;
  g->RW = render_width;
  g->RH = render_height;
  // frames without a render camera pipeline like tsdf_integrate; a render camera needs each frame
  // complete before its raycast, so those graphs keep the two-launch frame
  g->pipe = render_width == 0 && e->pipeline && e->maxs <= 3 && pipe_frame_size(e, width, height);
  g->defer = defer && render_width && e->maxs <= 3;  // (k_render_ingest_g is the 1024-slot ingest)
  auto fail = [&](hipError_t err, const char* what) {
    set_error(what, err);
    graph_free(g);
    return TSDF_ERR_HIP;
  };
  hipError_t err;
  if ((err = hipStreamCreateWithFlags(&g->cap, hipStreamNonBlocking)) != hipSuccess) return fail(err, "graph stream");
  const int nargs = tsdf_graph::kSlots * batch;
  if ((err = hipMalloc(&g->d_args, sizeof(FrameArgs) * nargs)) != hipSuccess) return fail(err, "graph args");
  if ((err = hipHostMalloc(&g->h_args, sizeof(FrameArgs) * nargs)) != hipSuccess)
    return fail(err, "graph host args");
  std::memset(g->h_args, 0, sizeof(FrameArgs) * nargs);
  const int tiles_x = (width + 15) / 16;
  const int tile_wgs = tile_pair_wgs(tiles_x, tiles_x * ((height + 15) / 16));
  // the engine's queued work must be done before the capture stream records anything
  if ((err = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(err, "graph sync");
  // the nodes of one frame (args entry A)
  auto frame_nodes = [&](const FrameArgs* A) {
    if (g->pipe) {  // one k_frame per frame, its grid sized for the largest launch (steady state)
      const int nwg = kPipeHead + kPipeFreshWG + e->D.integrate_grid_pre + tile_wgs + kVisWorkgroups;
      hipLaunchKernelGGL(k_frame_g, dim3(nwg), dim3(kIntegrateThreads), 0, g->cap, e->D, A);
    } else {
      const int rgx = (render_width + 15) / 16, nray = rgx * ((render_height + 15) / 16);
      if (g->defer)  // the previous frame's raycast (args->prev; none: its workgroups exit) + this ingest
        hipLaunchKernelGGL(k_render_ingest_g, dim3(nray + kVisWorkgroups + tile_wgs), dim3(256), 0, g->cap, e->D,
                           A, rgx, nray);
      else if (e->maxs <= 3)
        hipLaunchKernelGGL(k_ingest_dda_g<1024>, dim3(kVisWorkgroups + tile_wgs), dim3(256), 0, g->cap, e->D, A);
      else
        hipLaunchKernelGGL(k_ingest_dda_g<2048>, dim3(kVisWorkgroups + tile_wgs), dim3(256), 0, g->cap, e->D, A);
      if (render_width)  // the render camera's view grid built in the update launch
        hipLaunchKernelGGL(k_integrate_vg_g, dim3(e->D.integrate_grid + kOccWords / 256), dim3(kIntegrateThreads), 0,
                           g->cap, e->D, A, e->D.integrate_grid);
      else
        hipLaunchKernelGGL((k_integrate_t<true, false>), dim3(e->D.integrate_grid), dim3(kIntegrateThreads), 0,
                           g->cap, e->D, FrameParams{}, A);
    }
    if (render_width) {
      if (g->pipe)
        hipLaunchKernelGGL(k_view_grid_g, dim3(kOccWords / 256), dim3(256), 0, g->cap, e->D, A);
      hipLaunchKernelGGL(k_view_pack_g, dim3(kViewPackGrid), dim3(256), 0, g->cap, A);
      const dim3 rgrid((render_width + 15) / 16, (render_height + 15) / 16);
      if (!g->defer) hipLaunchKernelGGL(k_raycast_g, rgrid, dim3(256), 0, g->cap, e->D, A);
    }
  };
  // the args upload of entries [a0, a0 + n): one wave reads the pinned slots over the fabric (a kernel
  // node, no DMA engine in the graph)
  auto upload_node = [&](int a0, int n) {
    hipLaunchKernelGGL(k_copy_words, dim3(1), dim3(n > 1 ? 256 : 64), 0, g->cap,
                       reinterpret_cast<uint32_t*>(g->d_args + a0), reinterpret_cast<const uint32_t*>(g->h_args + a0),
                       (int)(sizeof(FrameArgs) * n / 4));
  };
  auto capture = [&](hipGraph_t* gr, hipGraphExec_t* ex, int a0, int n) -> hipError_t {
    hipError_t er = hipStreamBeginCapture(g->cap, hipStreamCaptureModeThreadLocal);
    if (er != hipSuccess) return er;
    upload_node(a0, n);
    for (int j = 0; j < n; ++j) frame_nodes(g->d_args + a0 + j);
    if ((er = hipStreamEndCapture(g->cap, gr)) != hipSuccess) return er;
    return hipGraphInstantiate(ex, *gr, nullptr, nullptr, 0);
  };
  for (int k = 0; k < tsdf_graph::kSlots; ++k) {
    if ((err = hipEventCreateWithFlags(&g->done[k], kGraphDoneFlags)) != hipSuccess) return fail(err, "graph event");
    if ((err = capture(&g->graph[k][0], &g->exec[k][0], k * batch, batch)) != hipSuccess)
      return fail(err, "graph capture");
    for (int j = 0; batch > 1 && j < batch; ++j)  // (a batch launched before it is full)
      if ((err = capture(&g->one_g[k][j], &g->one[k][j], k * batch + j, 1)) != hipSuccess)
        return fail(err, "graph capture (single frame)");
  }
  *out = g;
  return TSDF_OK;
}
}  // namespace

// launch the frames of g's current batch that were written but not launched (each alone)
int graph_flush_batch(tsdf_graph* g) {
  tsdf_engine* e = g->e;
  if (e->gbatch == g) e->gbatch = nullptr;
  if (g->fill == 0) return TSDF_OK;
  const int k = g->next, n = g->fill;
  g->fill = 0;
  g->next = (k + 1) % tsdf_graph::kSlots;
  for (int j = 0; j < n; ++j) HIP_OK(hipGraphLaunch(g->one[k][j], e->stream));
  HIP_OK(hipEventRecord(g->done[k], e->stream));
  g->used[k] = true;
  return TSDF_OK;
}

int tsdf_graph_create(tsdf_engine* e, int width, int height, int render_width, int render_height,
                      tsdf_graph** out) {
  return graph_create(e, width, height, render_width, render_height, false, out);
}

int tsdf_graph_create_deferred(tsdf_engine* e, int width, int height, int render_width, int render_height,
                               tsdf_graph** out) {
  return graph_create(e, width, height, render_width, render_height, true, out);
}

int tsdf_graph_create_batch(tsdf_engine* e, int width, int height, int render_width, int render_height,
                            int deferred, int frames_per_launch, tsdf_graph** out) {
  return graph_create(e, width, height, render_width, render_height, deferred != 0, out, frames_per_launch);
}

// A shard's graph frame: three captured segments per args slot -- (0) the args upload + k_ingest_dda_g
// over the slice (its tail packs the slice's keys into keys_out; slice_count 1: it resolves them, no
// key exchange), (1) k_resolve_alloc_g merging the key inbox (split DDA only) + the raw-frame
// k_integrate (its tail packs the carve candidates into cands_out), (2) k_resolve_delete_g of the
// candidate inbox. The caller's exchanges (RCCL all-gathers on the engine stream) run between them:
// stream-ordered collectives of another library cannot be recorded into the engine's graphs.
int tsdf_graph_create_shard(tsdf_engine* e, int width, int height, int slice_index, int slice_count,
                            tsdf_graph** out) {
  if (!e || !out || e->cfg.shard_count < 2 || width <= 0 || height <= 0 || width > e->cfg.max_width ||
      height > e->cfg.max_height || slice_count < 1 || slice_index < 0 || slice_index >= slice_count) {
    set_error("tsdf_graph_create_shard: invalid argument (a shard engine; the slice of its DDA)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  auto* g = new tsdf_graph();
  g->e = e;
  g->W = width;
  g->H = height;
  g->shard = true;
  g->slice_index = slice_index;
  g->slice_count = slice_count;
  auto fail = [&](hipError_t err, const char* what) {
    set_error(what, err);
    graph_free(g);
    return TSDF_ERR_HIP;
  };
  hipError_t err;
  if ((err = hipStreamCreateWithFlags(&g->cap, hipStreamNonBlocking)) != hipSuccess) return fail(err, "graph stream");
  if ((err = hipMalloc(&g->d_args, sizeof(FrameArgs) * tsdf_graph::kSlots)) != hipSuccess) return fail(err, "graph args");
  if ((err = hipHostMalloc(&g->h_args, sizeof(FrameArgs) * tsdf_graph::kSlots)) != hipSuccess)
    return fail(err, "graph host args");
  std::memset(g->h_args, 0, sizeof(FrameArgs) * tsdf_graph::kSlots);
  const int tiles_x = (width + 15) / 16, tiles_y = (height + 15) / 16;
  const int rows = (tiles_y + slice_count - 1) / slice_count;
  const int tile_wgs = tile_pair_wgs(
      tiles_x, (std::min(tiles_y, (slice_index + 1) * rows) - std::min(tiles_y, slice_index * rows)) * tiles_x);
  if ((err = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(err, "graph sync");
  for (int k = 0; k < tsdf_graph::kSlots; ++k) {
    const FrameArgs* A = g->d_args + k;
    if ((err = hipEventCreateWithFlags(&g->done[k], kGraphDoneFlags)) != hipSuccess) return fail(err, "graph event");
    for (int seg = 0; seg < tsdf_graph::kSegs; ++seg) {
      if ((err = hipStreamBeginCapture(g->cap, hipStreamCaptureModeThreadLocal)) != hipSuccess)
        return fail(err, "hipStreamBeginCapture");
      if (seg == 0) {
        hipLaunchKernelGGL(k_copy_words, dim3(1), dim3(64), 0, g->cap, reinterpret_cast<uint32_t*>(g->d_args + k),
                           reinterpret_cast<const uint32_t*>(g->h_args + k), (int)(sizeof(FrameArgs) / 4));
        if (e->maxs <= 3)
          hipLaunchKernelGGL(k_ingest_dda_g<1024>, dim3(kVisWorkgroups + tile_wgs), dim3(256), 0, g->cap, e->D, A);
        else
          hipLaunchKernelGGL(k_ingest_dda_g<2048>, dim3(kVisWorkgroups + tile_wgs), dim3(256), 0, g->cap, e->D, A);
      } else if (seg == 1) {
        if (slice_count > 1)
          hipLaunchKernelGGL(k_resolve_alloc_g, dim3(1), dim3(kRT), 0, g->cap, e->D, A);
        hipLaunchKernelGGL((k_integrate_t<true, true>), dim3(e->D.integrate_grid), dim3(kIntegrateThreads), 0,
                           g->cap, e->D, FrameParams{}, A);
      } else {
        hipLaunchKernelGGL(k_resolve_delete_g, dim3(1), dim3(kRT), 0, g->cap, e->D, A);
      }
      if ((err = hipStreamEndCapture(g->cap, &g->graph[k][seg])) != hipSuccess) return fail(err, "hipStreamEndCapture");
      if ((err = hipGraphInstantiate(&g->exec[k][seg], g->graph[k][seg], nullptr, nullptr, 0)) != hipSuccess)
        return fail(err, "hipGraphInstantiate");
    }
  }
  *out = g;
  return TSDF_OK;
}

int tsdf_graph_shard_begin(tsdf_graph* g, const tsdf_frame* f, const tsdf_intrinsics* K, const tsdf_pose* pose,
                           float max_depth, void* keys_out, const void* keys_in, int32_t key_cap, void* cands_out,
                           const void* cands_in, int32_t cand_cap) {
  TraceRange trace_("tsdf_graph_shard_begin");
  const bool split = g && g->slice_count > 1;
  if (!g || !g->shard || !f || !K || !pose || f->mem_kind != TSDF_MEM_DEVICE || f->width != g->W ||
      f->height != g->H || !f->depth || !f->rgb || (f->ht == nullptr) != (f->lt == nullptr) || !cands_out ||
      !cands_in || cand_cap < 1 || (split && (!keys_out || !keys_in || key_cap < 1))) {
    set_error("tsdf_graph_shard_begin: invalid argument (a shard graph; device frame of its size; the key "
              "slot / inbox of a split DDA and the candidate slot / inbox)");
    return TSDF_ERR_INVALID_ARG;
  }
  tsdf_engine* e = g->e;
  if (e->shard_phase != 0) {
    set_error("tsdf_graph_shard_begin: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  const int k = g->next;
  g->next = (k + 1) % tsdf_graph::kSlots;
  if (g->used[k]) HIP_OK(hipEventSynchronize(g->done[k]));  // slot k's upload has run
  FrameArgs& a = g->h_args[k];
  a = FrameArgs{};
  a.P = make_params(e, K, f->width, f->height, pose, max_depth);
  FrameParams& P = a.P;
  P.depth = f->depth;
  P.rgb = f->rgb;
  P.ht = f->ht;
  P.lt = f->lt;
  P.pack_pixels = 0;  // a shard's k_integrate reads the raw frame
  const int tiles_x = (f->width + 15) / 16, tiles_y = (f->height + 15) / 16;
  const int rows = (tiles_y + g->slice_count - 1) / g->slice_count;
  P.tile_lo = std::min(tiles_y, g->slice_index * rows) * tiles_x;
  P.tile_hi = std::min(tiles_y, (g->slice_index + 1) * rows) * tiles_x;
  if (split) {
    P.tail = kTailPack;
    P.slot = reinterpret_cast<ShardRec*>(keys_out);
    P.slot_cap = key_cap;
  }
  a.depth = f->depth;
  a.rgb = f->rgb;
  a.ht = f->ht;
  a.lt = f->lt;
  a.range = (uint32_t)((size_t)f->width * f->height * e->maxs);
  a.tiles_x = tiles_x;
  a.tiles = P.tile_hi - P.tile_lo;
  a.keys_out = reinterpret_cast<ShardRec*>(keys_out);
  a.keys_in = reinterpret_cast<const ShardRec*>(keys_in);
  a.key_cap = key_cap;
  a.cands_out = reinterpret_cast<ShardRec*>(cands_out);
  a.cands_in = reinterpret_cast<const ShardRec*>(cands_in);
  a.cand_cap = cand_cap;
  a.nshard = e->cfg.shard_count;
  HIP_OK(hipGraphLaunch(g->exec[k][0], e->stream));
  // the host slot is read by segment 0's upload only (segments 1 and 2 read the device copy, which
  // only segment 0 of the slot's next use rewrites, after them on the stream)
  HIP_OK(hipEventRecord(g->done[k], e->stream));
  g->used[k] = true;
  g->cur = k;
  e->shard_phase = 1;
  return TSDF_OK;
}

int tsdf_graph_shard_update(tsdf_graph* g) {
  TraceRange trace_("tsdf_graph_shard_update");
  if (!g || !g->shard || g->cur < 0 || g->e->shard_phase != 1) {
    set_error("tsdf_graph_shard_update: no graph frame begun");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(g->e->device));
  HIP_OK(hipGraphLaunch(g->exec[g->cur][1], g->e->stream));
  g->e->shard_phase = 2;
  return TSDF_OK;
}

int tsdf_graph_shard_end(tsdf_graph* g) {
  TraceRange trace_("tsdf_graph_shard_end");
  if (!g || !g->shard || g->cur < 0 || g->e->shard_phase != 2) {
    set_error("tsdf_graph_shard_end: no graph frame updated");
    return TSDF_ERR_INVALID_ARG;
  }
  tsdf_engine* e = g->e;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  HIP_OK(hipGraphLaunch(g->exec[g->cur][2], e->stream));
  g->cur = -1;
  e->shard_phase = 0;
  return TSDF_OK;
}

int tsdf_graph_frame(tsdf_graph* g, const tsdf_frame* f, const tsdf_intrinsics* K, const tsdf_pose* pose,
                     float max_depth, const tsdf_intrinsics* render_K, const tsdf_pose* render_pose,
                     uint8_t* rgba, uint8_t* normal) {
  TraceRange trace_("tsdf_graph_frame");
  if (!g || g->shard || !f || !K || !pose || f->mem_kind != TSDF_MEM_DEVICE || f->width != g->W ||
      f->height != g->H || !f->depth || !f->rgb || (f->ht == nullptr) != (f->lt == nullptr) ||
      (g->RW && (!render_K || !render_pose))) {
    set_error("tsdf_graph_frame: invalid argument (device frame of the graph's size)");
    return TSDF_ERR_INVALID_ARG;
  }
  tsdf_engine* e = g->e;
  if (e->shard_phase != 0) {
    set_error("tsdf_graph_frame: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  // this graph's deferred raycast of the previous frame: rendered by this launch (k_render_ingest_g).
  // It stays pending (a later call launches it) until the graph launch below, so an error return on
  // the way leaves it to the engine's next call instead of dropping its images. (Batched
  // graphs: the previous frame may sit in this batch, not launched yet; nothing else ran since.)
  const FrameArgs* prev = (g->defer && e->rdg.pending && e->rdg.g == g) ? e->rdg.args : nullptr;
  if (g->fill == 0) {
    if (e->gbatch && e->gbatch != g) {
      int rc = graph_flush_batch(e->gbatch);
      if (rc) return rc;
    }
    int rc = join_render(e, false, prev != nullptr);  // (not the raycast this launch takes)
    if (!rc && !g->pipe) rc = flush_pending(e);  // (pipelined: the pending frames continue in this launch)
    if (rc) return rc;
  }
  const int k = g->next, j = g->fill;
  if (j == 0 && g->used[k]) HIP_OK(hipEventSynchronize(g->done[k]));  // slot k's last batch has run
  const int ai = k * g->batch + j;  // this frame's args entry
  FrameArgs& a = g->h_args[ai];
  a.P = make_params(e, K, f->width, f->height, pose, max_depth);
  if (g->RW) a.R = make_params(e, render_K, g->RW, g->RH, render_pose, max_depth);
  a.depth = f->depth;
  a.rgb = f->rgb;
  a.ht = f->ht;
  a.lt = f->lt;
  a.rgba = reinterpret_cast<uchar4*>(rgba);
  a.normal = reinterpret_cast<uchar4*>(normal);
  a.step_size = e->cfg.truncation / 2;
  if (g->RW) {
    if (g->fill > 0 && view_grid_resets(e, a.R, a.step_size, kViewGraphBitmapWords)) {
      // the batch's frames read the grid this call resets or reallocates: they run first, and this
      // frame opens the next batch (recomputed from the start)
      int rc = graph_flush_batch(g);
      if (rc) return rc;
      return tsdf_graph_frame(g, f, K, pose, max_depth, render_K, render_pose, rgba, normal);
    }
    if (prev && view_grid_resets(e, a.R, a.step_size, kViewGraphBitmapWords)) {  // (it reads the old grid)
      e->rdg.pending = false;
      hipLaunchKernelGGL(k_raycast_g, dim3((g->RW + 15) / 16, (g->RH + 15) / 16), dim3(256), 0, e->stream, e->D,
                         prev);
      LAUNCH_OK("k_raycast_g");
      prev = nullptr;
    }
    int rc = view_grid_for(e, a.R, a.step_size, kViewGraphBitmapWords, &a.V);
    if (rc) return rc;
    a.vtag = 0x80000000u | (uint32_t)(e->vg_calls & 0x7FFFFFFFu);  // (never a frame id)
  }
  a.prev = prev;
  a.range = (uint32_t)((size_t)f->width * f->height * e->maxs);
  a.tiles_x = (f->width + 15) / 16;
  a.tiles = a.tiles_x * ((f->height + 15) / 16);
  uint32_t fid = 0;
  if (g->pipe) {  // this frame's ingest + the pending frames' carving / allocation / update
    fid = next_fid(e);
    a.P.depth = f->depth;
    a.P.rgb = f->rgb;
    a.P.ht = f->ht;
    a.P.lt = f->lt;
    a.P.pix_off = (fid & 1u) ? (int)e->max_pixels : 0;
    a.Pu = e->p_P;
    a.pipe = pipe_step(e, true, fid, a.P);
    finish_args(e, a.pipe, a.Pu);
    if (e->profiling && a.pipe.has_update) ++e->prof_pipelined;
  }
  if (prev) e->rdg.pending = false;  // rendered by this launch
  g->fill = j + 1;
  e->gbatch = g;
  const bool hash_raycast = g->defer && !a.V.n;  // (no grid: it reads the table the next ingest writes)
  if (g->fill == g->batch) {  // the batch is full: one launch runs its frames
    e->gbatch = nullptr;
    g->fill = 0;
    g->next = (k + 1) % tsdf_graph::kSlots;
    HIP_OK(hipGraphLaunch(g->exec[k][0], e->stream));
    HIP_OK(hipEventRecord(g->done[k], e->stream));
    g->used[k] = true;
  } else if (hash_raycast) {  // it must run after this frame, before the next one's ingest
    int rc = graph_flush_batch(g);
    if (rc) return rc;
  }
  if (g->defer) {
    // a view grid's raycast waits for the next frame's launch; a hash-lookup raycast runs now, after
    // this frame's graph
    if (a.V.n) {
      e->rdg.pending = true;
      e->rdg.g = g;
      e->rdg.args = g->d_args + ai;
      e->rdg.W = g->RW;
      e->rdg.H = g->RH;
    } else {
      hipLaunchKernelGGL(k_raycast_g, dim3((g->RW + 15) / 16, (g->RH + 15) / 16), dim3(256), 0, e->stream, e->D,
                         g->d_args + ai);
      LAUNCH_OK("k_raycast_g");
    }
  }
  if (g->pipe) pipe_advance(e, fid, a.P);
  return TSDF_OK;
}

int tsdf_graph_destroy(tsdf_graph* g) {
  if (!g) return TSDF_ERR_INVALID_ARG;
  (void)hipSetDevice(g->e->device);
  (void)graph_flush_batch(g);
  (void)join_render(g->e);
  (void)hipStreamSynchronize(g->e->stream);
  graph_free(g);
  return TSDF_OK;
}
