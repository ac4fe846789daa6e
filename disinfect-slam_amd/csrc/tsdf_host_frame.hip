// tsdf_host_frame.hip -- one frame on the host side: upload slots, the ingest / update / k_frame
// launches and the pipelined-frame state, tsdf_integrate, tsdf_flush and the tsdf_integrate_shard_*
// family.
#include "tsdf_host.h"

// the allocation resolver as its own launch: hash-level test path and imports (frame_mode 0)
int launch_resolve_alloc(tsdf_engine* e, const FrameParams& P, uint32_t range, int frame_mode) {
  hipLaunchKernelGGL(k_resolve_alloc, dim3(1), dim3(kRT), 0, e->stream, e->D, P, range, frame_mode,
                     (const ShardRec*)nullptr, 0, 0);
  if (!frame_mode)
    hipLaunchKernelGGL(k_fresh_init, dim3(512), dim3(256), 0, e->stream, e->D);
  LAUNCH_OK("allocate");
  return TSDF_OK;
}

// the launch that reads the pending uploaded frame has been enqueued on the engine stream: its slot is
// free for an upload once the engine stream gets here
// and the call returns only once the upload is complete: the caller may reuse its host buffers (the
// reference's synchronous cudaMemcpy contract)
static int upload_release(tsdf_engine* e) {
  if (e->up_pending < 0) return TSDF_OK;
  const int k = e->up_pending;
  e->up_pending = -1;
  HIP_OK(hipEventRecord(e->up_free[k], e->stream));
  e->up_used[k] = true;
  for (int j = 0; j < e->up_nstreams; ++j) HIP_OK(hipEventSynchronize(e->up_done[k][j]));
  return TSDF_OK;
}

// the next profiling event set (a std::deque: push_back never moves the sets earlier frames hold)
static int take_events(tsdf_engine* e, std::array<hipEvent_t, 5>** out) {
  if (e->ev_used == e->events.size()) {
    std::array<hipEvent_t, 5> a{};
    // (no system-scope fence when an event completes: with it, the dispatch an event pair is bound to
    // ran ~6 us longer than the others -- 50.1 vs 44.3 us in the driver command's kernel trace)
    for (auto& x : a) HIP_OK(hipEventCreateWithFlags(&x, hipEventDisableSystemFence));
    e->events.push_back(a);
  }
  *out = &e->events[e->ev_used++];
  return TSDF_OK;
}

// Phase 1 of a frame: stage host inputs, then (launch) k_ingest_dda on view Dv (the frame's lists,
// counts and candidates: frame_view): pixel records for the whole frame, the DDA over tiles of slice
// `slice_index` of `slice_count` -- contiguous bands of tile rows --, the visibility of the existing
// blocks, and the allocation in its last workgroup. *P / *ev carry the frame to the later phases.
static int frame_ingest(tsdf_engine* e, const EngineDev& Dv, const tsdf_frame* f, const tsdf_intrinsics* K,
                 const tsdf_pose* pose, float max_depth, int slice_index, int slice_count, FrameParams* P,
                 std::array<hipEvent_t, 5>** ev_out, void* keys_out = nullptr, int key_cap = 0,
                 bool launch = true, int pix_buf = 0) {
  if (!e || !f || !K || !pose || !f->depth || !f->rgb || f->width <= 0 || f->height <= 0 ||
      (int64_t)f->width * f->height > e->max_pixels || f->width > e->cfg.max_width ||
      f->height > e->cfg.max_height || (f->ht == nullptr) != (f->lt == nullptr) ||
      slice_count < 1 || slice_index < 0 || slice_index >= slice_count) {
    set_error("tsdf_integrate: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  const int W = f->width, H = f->height;
  const size_t np = (size_t)W * H;
  hipStream_t s = e->stream;
  const float* depth = f->depth;
  const uint8_t* rgb = f->rgb;
  const float* ht = f->ht;
  const float* lt = f->lt;
  if (f->mem_kind == TSDF_MEM_HOST) {  // voxel_tsdf.cu:358-365 (H2D; pageable or pinned host memory)
    // The upload runs on the upload streams into the next of two staging slots, beside the frames the
    // engine stream is still running; the engine stream waits for it (up_done) and the slot's next
    // upload waits until the launch reading this frame is enqueued and done (up_free, recorded by
    // upload_release). The call returns once the copies are complete, so the caller may reuse its
    // buffers (the reference's synchronous cudaMemcpy contract).
    if (int rc = upload_release(e)) return rc;
    const int k = e->up_next;
    e->up_next ^= 1;
    // the copies round-robin over the upload streams: they run on several DMA engines at once; the
    // engine stream waits for each
    const void* src[4] = {rgb, depth, ht, lt};
    const size_t bytes[4] = {np * 3, np * 4, np * 4, np * 4};
    void* dst[4] = {e->s_rgb + (size_t)k * e->max_pixels * 3, e->s_depth + (size_t)k * e->max_pixels,
                    e->s_ht + (size_t)k * e->max_pixels, e->s_lt + (size_t)k * e->max_pixels};
    const int ncopy = ht ? 4 : 2;
    e->up_nstreams = std::min((int)tsdf_engine::kUpStreams, ncopy);
    for (int j = 0; j < e->up_nstreams; ++j)
      if (e->up_used[k]) HIP_OK(hipStreamWaitEvent(e->ustream[j], e->up_free[k], 0));
    for (int c = 0; c < ncopy; ++c)
      HIP_OK(hipMemcpyAsync(dst[c], src[c], bytes[c], hipMemcpyHostToDevice, e->ustream[c % e->up_nstreams]));
    for (int j = 0; j < e->up_nstreams; ++j) {
      HIP_OK(hipEventRecord(e->up_done[k][j], e->ustream[j]));
      HIP_OK(hipStreamWaitEvent(s, e->up_done[k][j], 0));
    }
    rgb = static_cast<const uint8_t*>(dst[0]);
    depth = static_cast<const float*>(dst[1]);
    if (ht) {
      ht = static_cast<const float*>(dst[2]);
      lt = static_cast<const float*>(dst[3]);
    }
    // (the host waits for the copies in upload_release, after the launch that reads them is enqueued:
    // the enqueue overlaps the transfer)
    e->up_pending = k;
  } else if (f->mem_kind != TSDF_MEM_DEVICE) {
    set_error("tsdf_integrate: bad mem_kind");
    return TSDF_ERR_INVALID_ARG;
  }
  *P = make_params(e, K, W, H, pose, max_depth);
  P->depth = depth;
  P->rgb = rgb;
  P->ht = ht;
  P->lt = lt;
  P->pix_off = pix_buf ? (int)e->max_pixels : 0;  // which of the two pixel-record buffers
  // a shard's k_integrate reads the raw frame: no whole-frame pixel pass in its ingest
  P->pack_pixels = e->cfg.shard_count > 1 ? 0 : 1;
  const int tiles_x = (W + 15) / 16, tiles_y = (H + 15) / 16;
  P->tile_lo = 0;
  P->tile_hi = tiles_x * tiles_y;
  if (slice_count > 1) {  // contiguous bands of tile rows
    const int rows = (tiles_y + slice_count - 1) / slice_count;
    P->tile_lo = std::min(tiles_y, slice_index * rows) * tiles_x;
    P->tile_hi = std::min(tiles_y, (slice_index + 1) * rows) * tiles_x;
  }
  const int tiles = P->tile_hi - P->tile_lo;  // the launch covers the DDA's tiles only
  if (keys_out) {  // the last workgroup packs the keys for the exchange instead of resolving them
    P->tail = kTailPack;
    P->slot = reinterpret_cast<ShardRec*>(keys_out);
    P->slot_cap = key_cap;
  }
  std::array<hipEvent_t, 5>* ev = nullptr;
  if (e->profiling && (e->prof_calls++ % e->prof_every) == 0) {
    int rc = take_events(e, &ev);
    if (rc) return rc;
  }
  *ev_out = ev;
  if (!launch) return TSDF_OK;
  if (ev && e->prof_mode == TSDF_PROFILE_PHASES) HIP_OK(hipEventRecord((*ev)[0], s));
  // ---- allocate (voxel_tsdf.cu:377-386) + visibility (:388-397) ----
  // k_ingest_dda sweeps the blocks that already exist for visibility beside the DDA; its last
  // workgroup resolves the new keys and appends the blocks it creates to the visible lists
  if (e->rd.pending && e->maxs <= 3 && slice_count == 1 && !keys_out && e->cfg.shard_count <= 1) {
    // the deferred raycast of the previous frame in the same launch (k_render_ingest)
    e->rd.pending = false;
    const tsdf_engine::DeferredRender& r = e->rd;
    const int rgx = (r.P.W + 15) / 16, nray = rgx * ((r.P.nrows + 15) / 16);
    hipLaunchKernelGGL(k_render_ingest, dim3(nray + kVisWorkgroups + tile_pair_wgs(tiles_x, tiles)), dim3(256), 0, s, Dv, r.P, r.step, r.V,
                       r.rgba, r.normal, rgx, nray, *P, depth, rgb, ht, lt, tiles_x, tiles);
    LAUNCH_OK("k_render_ingest");
    return TSDF_OK;
  }
  JOIN_RENDER(e);  // a deferred raycast this ingest cannot take up runs first
  if (e->maxs <= 3)
    hipLaunchKernelGGL(k_ingest_dda<1024>, dim3(kVisWorkgroups + tile_pair_wgs(tiles_x, tiles)), dim3(256), 0, s, Dv, *P, depth,
                       rgb, ht, lt, tiles_x, tiles);
  else
    hipLaunchKernelGGL(k_ingest_dda<2048>, dim3(kVisWorkgroups + tile_pair_wgs(tiles_x, tiles)), dim3(256), 0, s, Dv, *P, depth,
                       rgb, ht, lt, tiles_x, tiles);
  LAUNCH_OK("k_ingest_dda");
  return TSDF_OK;
}

// Phase 2: fused update (+ carve minimum) on view Dv; the last workgroup carves (kTailResolve) or
// packs a shard's carve candidates into cands_out. (Measured and not kept in round 1: running the
// update of the existing blocks beside the allocation resolver, on a second stream or as a dispatch
// without the AQL barrier bit: the resolver's chain of dependent HBM round trips slows ~2.5x under
// the update's memory load.)
static int frame_update(tsdf_engine* e, const EngineDev& Dv, FrameParams P, std::array<hipEvent_t, 5>* ev,
                 void* cands_out = nullptr, int cand_cap = 0) {
  hipStream_t s = e->stream;
  JOIN_RENDER(e);  // the update writes the pool a deferred raycast still pending reads
  const bool all_ev = ev && e->prof_mode == TSDF_PROFILE_PHASES;
  if (all_ev) HIP_OK(hipEventRecord((*ev)[1], s));
  P.tail = cands_out ? kTailPack : kTailResolve;
  P.slot = reinterpret_cast<ShardRec*>(cands_out);
  P.slot_cap = cand_cap;
  // ---- update (voxel_tsdf.cu:474-481) + space carving (:483-488) ----
  auto kfn = P.pack_pixels ? k_integrate_t<false, false> : k_integrate_t<false, true>;
  if (ev && e->prof_mode == TSDF_PROFILE_KERNEL) {
    // the two events are bound to the kernel's own dispatch packet (its begin / end timestamps,
    // the interval rocprofv3's kernel trace reports): no marker packets enter the stream
    hipExtLaunchKernelGGL(kfn, dim3(e->D.integrate_grid), dim3(kIntegrateThreads), 0, s,
                          (*ev)[2], (*ev)[3], 0, Dv, P, (const FrameArgs*)nullptr);
  } else {
    if (ev) HIP_OK(hipEventRecord((*ev)[2], s));
    hipLaunchKernelGGL(kfn, dim3(e->D.integrate_grid), dim3(kIntegrateThreads), 0, s,
                       Dv, P, (const FrameArgs*)nullptr);
    if (ev) HIP_OK(hipEventRecord((*ev)[3], s));
  }
  LAUNCH_OK("k_integrate");
  if (all_ev && !cands_out) HIP_OK(hipEventRecord((*ev)[4], s));
  return TSDF_OK;
}

// the launch-wide fields of a k_frame's arguments
void finish_args(tsdf_engine* e, PipeArgs& A, const FrameParams& Pu) {
  A.tag = ++e->pipe_tag ? e->pipe_tag : ++e->pipe_tag;  // (0: the flags' initial value)
  A.nint = e->D.integrate_grid_pre;
  A.order = e->frame_order;
  A.range = A.has_alloc ? (uint32_t)((size_t)Pu.W * Pu.H * e->maxs) : 0u;
  if (!A.has_frame) A.tiles = A.tiles_x = 0;
  A.tile_wgs = tile_pair_wgs(A.tiles_x, A.tiles);
}

// One k_frame launch (tsdf_fuse.hip): frame A.fid_carve's carving, frame A.fid_alloc's allocation and
// update (camera / pixel records Pu), frame A.fid_new's ingest (Pn) -- the parts A enables.
static int launch_frame(tsdf_engine* e, PipeArgs A, const FrameParams& Pu, const FrameParams& Pn,
                 std::array<hipEvent_t, 5>* ev) {
  hipStream_t s = e->stream;
  JOIN_RENDER(e);
  finish_args(e, A, Pu);
  const int nwg = kPipeHead + (A.has_update ? A.nint : 0) + pipe_fresh_wgs(A) +
                  (A.has_frame ? A.tile_wgs + kVisWorkgroups : 0);
  if (e->profiling && A.has_frame) ++e->prof_pipelined;  // (frame launches; not the flush's)
  if (ev && e->prof_mode == TSDF_PROFILE_KERNEL) {
    hipExtLaunchKernelGGL(k_frame, dim3(nwg), dim3(kIntegrateThreads), 0, s, (*ev)[2], (*ev)[3], 0, e->D, Pu, Pn, A);
  } else {
    // (phase events: the launch is the whole frame -- "integrate" spans it, the other phases are empty)
    const bool all_ev = ev && e->prof_mode == TSDF_PROFILE_PHASES;
    if (all_ev) HIP_OK(hipEventRecord((*ev)[0], s));
    if (all_ev) HIP_OK(hipEventRecord((*ev)[1], s));
    if (ev) HIP_OK(hipEventRecord((*ev)[2], s));
    hipLaunchKernelGGL(k_frame, dim3(nwg), dim3(kIntegrateThreads), 0, s, e->D, Pu, Pn, A);
    if (ev) HIP_OK(hipEventRecord((*ev)[3], s));
    if (all_ev) HIP_OK(hipEventRecord((*ev)[4], s));
  }
  LAUNCH_OK("k_frame");
  return TSDF_OK;
}

// Frames up to pipe_max_pixels (2^20; TSDF_PIPE_MAX_PIXELS) are pipelined (k_frame). Larger frames take the two
// launches. With one workgroup per 16x16 tile the gate stood at 2^19: a 1280x720 frame's 3,600 tile workgroups
// did not fit beside the update (C4, driver-size runs: 13.0-13.3k frames/s pipelined against 14.6-14.8k in two
// launches). With tile pairs (1,800 workgroups) the pipelined form is ahead at both lengths (same box,
// interleaved: 17.6-17.8k against 14.4k at the driver's length, 19.4-19.5k against 15.9k over 300 frames;
// profiles/ab/r7_c4_gate_ab.txt); nothing larger has been measured.
bool pipe_frame_size(const tsdf_engine* e, int w, int h) { return (int64_t)w * h <= e->pipe_max_pixels; }

// The k_frame launch that continues the pending frames, with (has_frame) the ingest of a new frame
// fid whose parameters are Pn; the state moves to kPipeCAU (or kPipeAU from kPipeNone).
PipeArgs pipe_step(tsdf_engine* e, bool has_frame, uint32_t fid, const FrameParams& Pn) {
  PipeArgs A{};
  const int ps = e->ps;
  if (ps != tsdf_engine::kPipeNone) {
    A.has_update = 1;
    A.fid_alloc = e->p_fid;
    A.fresh_ready = ps == tsdf_engine::kPipeU;  // p_fid's new blocks were listed by its k_ingest_dda
    A.has_alloc = ps != tsdf_engine::kPipeU;
    A.has_carve = ps == tsdf_engine::kPipeCAU;
    A.fid_carve = e->p_carve;
  }
  if (has_frame) {
    A.has_frame = 1;
    A.fid_new = fid;
    A.tiles_x = (Pn.W + 15) / 16;
    A.tiles = A.tiles_x * ((Pn.H + 15) / 16);
  }
  return A;
}
void pipe_advance(tsdf_engine* e, uint32_t fid, const FrameParams& Pn) {
  if (e->ps == tsdf_engine::kPipeNone) {
    e->ps = tsdf_engine::kPipeAU;
  } else {
    e->p_carve = e->p_fid;
    e->ps = tsdf_engine::kPipeCAU;
  }
  e->p_fid = fid;
  e->p_P = Pn;
}
uint32_t next_fid(tsdf_engine* e) {
  uint32_t fid = e->fid_next++;
  // never 0; after 2^32 - 1 (= 3 mod 6) comes 4: consecutive frames keep distinct parity (frame_view's
  // two-frame lists) and residue mod 3 (its three band views)
  if (fid == 0u) {
    fid = 4u;
    e->fid_next = 5u;
  }
  return fid;
}

// complete the pending frames (pipelined): kPipeU -- the frame's update with its carving in its last
// workgroup (k_integrate); kPipeCAU -- one k_frame for the pending carving, allocation and update,
// then one for that frame's own carving
int flush_pending(tsdf_engine* e) {
  if (e->ps == tsdf_engine::kPipeNone) return TSDF_OK;
  if (sharded(e)) {  // its carvings need every shard's candidates: only the exchange protocol can
    set_error("a pipelined sharded frame is pending: complete it with tsdf_integrate_shard_pipe(frame = "
              "NULL) until *pending == 0");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  const int ps = e->ps;
  e->ps = tsdf_engine::kPipeNone;
  if (ps == tsdf_engine::kPipeU) {
    // a sampled frame's update is timed here (the C5 loop: a raycast after every frame flushes it);
    // (PHASES mode: its allocation ran in the ingest launch before, so event 0 opens at the update)
    std::array<hipEvent_t, 5>* ev = nullptr;
    if (e->p_sampled && e->profiling) {
      int rc = take_events(e, &ev);
      if (rc) return rc;
      if (e->prof_mode == TSDF_PROFILE_PHASES) HIP_OK(hipEventRecord((*ev)[0], e->stream));
    }
    e->p_sampled = false;
    return frame_update(e, frame_view(e->D, e->p_fid), e->p_P, ev);
  }
  PipeArgs A{};
  A.has_carve = ps == tsdf_engine::kPipeCAU;
  A.fid_carve = e->p_carve;
  A.has_alloc = 1;
  A.has_update = 1;
  A.fid_alloc = e->p_fid;
  const FrameParams none{};
  int rc = launch_frame(e, A, e->p_P, none, nullptr);
  if (rc) return rc;
  PipeArgs C{};
  C.has_carve = 1;
  C.fid_carve = e->p_fid;
  return launch_frame(e, C, none, none, nullptr);
}

// The pending unpipelined update (ps == kPipeU) with the view grid of render camera R built in the same
// launch (k_integrate_vg; raycast_impl's deferred C5 path). Events as flush_pending + frame_update.
int update_with_grid(tsdf_engine* e, const FrameParams& R, const ViewGrid& V) {
  hipStream_t s = e->stream;
  std::array<hipEvent_t, 5>* ev = nullptr;
  if (e->p_sampled && e->profiling) {
    int rc = take_events(e, &ev);
    if (rc) return rc;
    if (e->prof_mode == TSDF_PROFILE_PHASES) HIP_OK(hipEventRecord((*ev)[0], s));
  }
  e->p_sampled = false;
  e->ps = tsdf_engine::kPipeNone;
  const EngineDev Dv = frame_view(e->D, e->p_fid);
  FrameParams P = e->p_P;
  P.tail = kTailResolve;
  P.slot = nullptr;
  P.slot_cap = 0;
  const uint32_t vtag = 0x80000000u | (uint32_t)(e->vg_calls & 0x7FFFFFFFu);  // (never a frame id)
  const int nint = e->D.integrate_grid;
  const dim3 grid(nint + kOccWords / 256);
  const bool all_ev = ev && e->prof_mode == TSDF_PROFILE_PHASES;
  if (all_ev) HIP_OK(hipEventRecord((*ev)[1], s));
  if (ev && e->prof_mode == TSDF_PROFILE_KERNEL) {
    hipExtLaunchKernelGGL(k_integrate_vg, grid, dim3(kIntegrateThreads), 0, s, (*ev)[2], (*ev)[3], 0, Dv, P, R, V,
                          vtag, nint);
  } else {
    if (ev) HIP_OK(hipEventRecord((*ev)[2], s));
    hipLaunchKernelGGL(k_integrate_vg, grid, dim3(kIntegrateThreads), 0, s, Dv, P, R, V, vtag, nint);
    if (ev) HIP_OK(hipEventRecord((*ev)[3], s));
  }
  LAUNCH_OK("k_integrate_vg");
  if (all_ev) HIP_OK(hipEventRecord((*ev)[4], s));
  return TSDF_OK;
}

// One frame (TSDFGrid::Integrate). Pipelined (one volume, <= 3 DDA samples per pixel):
// tsdf_integrate of frame c launches ONE k_frame that carves frame c - 2, allocates and updates frame
// c - 1 and runs frame c's ingest; what remains (c - 1's carving, c's allocation and update) runs in
// the next call's launch, or in flush_pending, which every other entry point (and tsdf_flush /
// tsdf_synchronize) calls first. Stream order and the in-launch flags keep every result identical to
// the unpipelined two launches per frame.
int tsdf_integrate(tsdf_engine* e, const tsdf_frame* f, const tsdf_intrinsics* K,
                   const tsdf_pose* pose, float max_depth) {
  TraceRange trace_("tsdf_integrate");
  if (e && sharded(e)) {
    set_error("tsdf_integrate: a shard of a sharded volume integrates through tsdf_integrate_shard_*");
    return TSDF_ERR_INVALID_ARG;
  }
  if (!e || !f || !K || !pose) {  // (before anything reads the frame: pipe_frame_size below does)
    set_error("tsdf_integrate: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  const bool pipe = e->pipeline && e->maxs <= 3 && pipe_frame_size(e, f->width, f->height);
  if (!pipe) {
    int rc = flush_pending(e);
    if (rc) return rc;
  }
  const uint32_t fid = next_fid(e);
  const EngineDev Dv = frame_view(e->D, fid);
  FrameParams P;
  std::array<hipEvent_t, 5>* ev = nullptr;
  // the first frame after a flush runs k_ingest_dda (its ingest and allocation in one launch)
  const bool ingest_alone = !pipe || e->ps == tsdf_engine::kPipeNone;
  int rc = frame_ingest(e, Dv, f, K, pose, max_depth, 0, 1, &P, &ev, nullptr, 0, ingest_alone, (int)(fid & 1u));
  if (rc) {
    (void)upload_release(e);  // (a failed launch after the upload: the host buffers are still read)
    return rc;
  }
  if (!pipe) {
    rc = frame_update(e, Dv, P, ev);
    const int ru = upload_release(e);
    return rc ? rc : ru;
  }
  if (ingest_alone) {
    // (no k_frame / k_integrate launch to time in this call: the slot is released, and the update,
    // if a flush launches it as k_integrate, takes one then)
    if (ev) --e->ev_used;
    e->p_sampled = ev != nullptr;
    e->ps = tsdf_engine::kPipeU;
    e->p_fid = fid;
    e->p_P = P;
    return upload_release(e);  // (k_ingest_dda read the frame)
  }
  rc = launch_frame(e, pipe_step(e, true, fid, P), e->p_P, P, ev);
  if (rc) {
    (void)upload_release(e);
    return rc;
  }
  pipe_advance(e, fid, P);
  return upload_release(e);  // (the launch's tiles read the frame)
}

int tsdf_flush(tsdf_engine* e) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  return TSDF_OK;
}

// ---------------------------------------------------------------------------------------------
// Sharded frames. Every shard keeps the whole hash index and holds the voxels of its
// own blocks; one frame is three calls around two all-gathers (include/disinfect_tsdf.h).
// ---------------------------------------------------------------------------------------------
int64_t tsdf_shard_slot_bytes(int32_t cap) {
  if (cap < 1) return 0;
  return (int64_t)(cap + 1) * (int64_t)sizeof(ShardRec);
}

int tsdf_integrate_shard_begin(tsdf_engine* e, const tsdf_frame* f, const tsdf_intrinsics* K,
                               const tsdf_pose* pose, float max_depth, int32_t slice_index,
                               int32_t slice_count, void* keys_out, int32_t key_cap) {
  TraceRange trace_("tsdf_integrate_shard_begin");
  if (!e || !sharded(e) || e->shard_phase != 0 || (keys_out && key_cap < 1) ||
      (!keys_out && slice_count != 1)) {
    set_error("tsdf_integrate_shard_begin: invalid argument (a shard engine between frames; a key "
              "slot unless slice_count == 1)");
    return TSDF_ERR_INVALID_ARG;
  }
  ENTER(e);
  FrameParams P;
  std::array<hipEvent_t, 5>* ev = nullptr;
  // split DDA: the last workgroup packs this slice's keys into keys_out; whole-frame DDA (no key
  // exchange): it resolves the allocation right away, like one volume
  int rc = frame_ingest(e, e->D, f, K, pose, max_depth, slice_index, slice_count, &P, &ev, keys_out, key_cap);
  // (a host frame: its upload is complete on return -- the slot itself is released after _update)
  if (e->up_pending >= 0)
    for (int j = 0; j < e->up_nstreams; ++j) HIP_OK(hipEventSynchronize(e->up_done[e->up_pending][j]));
  if (rc) return rc;
  P.tail = kTailResolve;
  P.slot = nullptr;
  P.slot_cap = 0;
  e->shard_P = P;
  e->shard_ev = ev;
  e->shard_keys_packed = keys_out != nullptr;
  e->shard_phase = 1;
  return TSDF_OK;
}

int tsdf_integrate_shard_update(tsdf_engine* e, const void* keys_in, int32_t key_cap, void* cands_out,
                                int32_t cand_cap) {
  TraceRange trace_("tsdf_integrate_shard_update");
  if (!e || e->shard_phase != 1 || (keys_in != nullptr) != e->shard_keys_packed ||
      (keys_in && key_cap < 1) || !cands_out || cand_cap < 1) {
    set_error("tsdf_integrate_shard_update: invalid argument (after tsdf_integrate_shard_begin; the "
              "key inbox iff _begin packed keys; a candidate slot)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  if (keys_in) {  // merge every shard's keys, then the ordered allocation (one workgroup)
    const FrameParams& P = e->shard_P;
    hipLaunchKernelGGL(k_resolve_alloc, dim3(1), dim3(kRT), 0, e->stream, e->D, P,
                       (uint32_t)((size_t)P.W * P.H * e->maxs), 1, reinterpret_cast<const ShardRec*>(keys_in),
                       key_cap, e->cfg.shard_count);
    LAUNCH_OK("k_resolve_alloc");
  }
  int rc = frame_update(e, e->D, e->shard_P, e->shard_ev, cands_out, cand_cap);
  if (rc) return rc;
  e->shard_phase = 2;
  return upload_release(e);  // (a shard's k_integrate reads the raw frame)
}

int tsdf_integrate_shard_end(tsdf_engine* e, const void* cands_in, int32_t cand_cap) {
  TraceRange trace_("tsdf_integrate_shard_end");
  if (!e || e->shard_phase != 2 || !cands_in || cand_cap < 1) {
    set_error("tsdf_integrate_shard_end: invalid argument (after tsdf_integrate_shard_update; the "
              "candidate inbox)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  hipLaunchKernelGGL(k_resolve_delete, dim3(1), dim3(kRT), 0, e->stream, e->D, (const VisRec*)e->D.cand,
                     (const int32_t*)e->D.ncand, 0, reinterpret_cast<const ShardRec*>(cands_in),
                     cand_cap, e->cfg.shard_count);
  LAUNCH_OK("k_resolve_delete");
  e->shard_phase = 0;
  std::array<hipEvent_t, 5>* ev = e->shard_ev;
  if (ev && e->prof_mode == TSDF_PROFILE_PHASES) HIP_OK(hipEventRecord((*ev)[4], e->stream));
  return TSDF_OK;
}

// ---------------------------------------------------------------------------------------------
// Pipelined sharded frames (one exchange per frame): every shard runs the whole frame's
// DDA against its copy of the index (no key exchange: --mode sharded), so only the carve candidates
// cross the shards. Call n launches one k_frame: frame n - 2's carving of every shard's candidates
// (cands_in: the all-gathered slots of call n - 1), frame n - 1's allocation and update (its
// candidates into cands_out, for the exchange after this call), frame n's ingest.
// ---------------------------------------------------------------------------------------------
// tsdf_integrate_shard_pipe, and a group's form (dsts: the update's last workgroup writes the
// candidate slot into the ndst device slots listed at dsts -- a device array; dsts_host: the same
// pointers, for the zeroed headers of the first call -- instead of cands_out)
static int shard_pipe_impl(tsdf_engine* e, const tsdf_frame* f, const tsdf_intrinsics* K, const tsdf_pose* pose,
                           float max_depth, const void* cands_in, void* cands_out, ShardRec* const* dsts,
                           ShardRec* const* dsts_host, int ndst, int32_t cand_cap, int32_t* pending) {
  HIP_OK(hipSetDevice(e->device));
  JOIN_RENDER(e);
  *pending = 0;
  const ShardRec* in = reinterpret_cast<const ShardRec*>(cands_in);
  ShardRec* out = reinterpret_cast<ShardRec*>(cands_out);
  auto shard_args = [&](PipeArgs& A) {
    A.cands_in = A.has_carve ? in : nullptr;
    A.cands_out = A.has_update ? out : nullptr;
    A.cands_dst = A.has_update ? dsts : nullptr;
    A.ndst = ndst;
    A.cand_cap = cand_cap;
    A.nshard = e->cfg.shard_count;
  };
  const FrameParams none{};
  if (!f) {  // one step of completing the pending frames
    const int ps = e->ps;
    if (ps == tsdf_engine::kPipeNone) return TSDF_OK;
    PipeArgs A{};
    if (ps == tsdf_engine::kPipeC) {
      A.has_carve = 1;
      A.fid_carve = e->p_fid;
      shard_args(A);
      int rc = launch_frame(e, A, none, none, nullptr);
      if (rc) return rc;
      e->ps = tsdf_engine::kPipeNone;
      return TSDF_OK;
    }
    A = pipe_step(e, false, 0u, none);
    shard_args(A);
    int rc = launch_frame(e, A, e->p_P, none, nullptr);
    if (rc) return rc;
    e->ps = tsdf_engine::kPipeC;  // (p_fid's carving, after the exchange of its candidates)
    *pending = 1;
    return TSDF_OK;
  }
  if (e->ps == tsdf_engine::kPipeC) {
    set_error("tsdf_integrate_shard_pipe: a flush is in progress (call with frame = NULL until *pending == 0)");
    return TSDF_ERR_INVALID_ARG;
  }
  const uint32_t fid = next_fid(e);
  FrameParams P;
  std::array<hipEvent_t, 5>* ev = nullptr;
  int rc = frame_ingest(e, frame_view(e->D, fid), f, K, pose, max_depth, 0, 1, &P, &ev, nullptr, 0, false,
                        (int)(fid & 1u));
  if (rc) return rc;
  P.pack_pixels = 1;  // every shard packs the whole frame's pixel records (its blocks project anywhere)
  if (e->ps == tsdf_engine::kPipeNone) {  // the first frame: ingest + allocation in one launch
    const EngineDev Dv = frame_view(e->D, fid);
    const int tiles = P.tile_hi - P.tile_lo, tiles_x = (P.W + 15) / 16;
    HIP_OK(hipMemsetAsync(&e->D.ctr->n_pend, 0, sizeof(int32_t), e->stream));  // (its allocation's list)
    hipLaunchKernelGGL(k_ingest_dda<1024>, dim3(kVisWorkgroups + tile_pair_wgs(tiles_x, tiles)), dim3(256), 0, e->stream, Dv, P, P.depth,
                       P.rgb, P.ht, P.lt, tiles_x, tiles);
    LAUNCH_OK("k_ingest_dda");
    if (dsts_host) {  // (no candidates from this call)
      for (int d = 0; d < ndst; ++d) HIP_OK(hipMemsetAsync(dsts_host[d], 0, sizeof(ShardRec), e->stream));
    } else {
      HIP_OK(hipMemsetAsync(out, 0, sizeof(ShardRec), e->stream));
    }
    if (ev) --e->ev_used;
    e->ps = tsdf_engine::kPipeU;
    e->p_fid = fid;
    e->p_P = P;
    return upload_release(e);
  }
  PipeArgs A = pipe_step(e, true, fid, P);
  shard_args(A);
  rc = launch_frame(e, A, e->p_P, P, ev);
  if (rc) return rc;
  pipe_advance(e, fid, P);
  return upload_release(e);
}

// the group's entry (csrc/tsdf_group.hip, declared in csrc/tsdf_internal.h): tsdf_integrate_shard_pipe
// with the candidate slot written into the ndst slots at dsts_dev (device array) instead of an
// outgoing slot
int tsdf_integrate_shard_pipe_fanout(tsdf_engine* e, const tsdf_frame* f, const tsdf_intrinsics* K,
                                     const tsdf_pose* pose, float max_depth, const void* cands_in,
                                     void* const* dsts_dev, void* const* dsts_host, int ndst, int32_t cand_cap,
                                     int32_t* pending) {
  TraceRange trace_("tsdf_integrate_shard_pipe_fanout");
  if (!e || !sharded(e) || e->shard_phase != 0 || !cands_in || !dsts_dev || !dsts_host || ndst < 1 ||
      cand_cap < 1 || !pending || (f && (!K || !pose)) || e->maxs > 3) {
    set_error("tsdf_integrate_shard_pipe_fanout: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  ShardRec* self = reinterpret_cast<ShardRec*>(dsts_host[e->cfg.shard_index % ndst]);
  return shard_pipe_impl(e, f, K, pose, max_depth, cands_in, self, reinterpret_cast<ShardRec* const*>(dsts_dev),
                         reinterpret_cast<ShardRec* const*>(dsts_host), ndst, cand_cap, pending);
}

int tsdf_integrate_shard_pipe(tsdf_engine* e, const tsdf_frame* f, const tsdf_intrinsics* K,
                              const tsdf_pose* pose, float max_depth, const void* cands_in, void* cands_out,
                              int32_t cand_cap, int32_t* pending) {
  TraceRange trace_("tsdf_integrate_shard_pipe");
  if (!e || !sharded(e) || e->shard_phase != 0 || !cands_in || !cands_out || cand_cap < 1 || !pending ||
      (f && (!K || !pose)) || e->maxs > 3) {
    set_error("tsdf_integrate_shard_pipe: invalid argument (a shard engine between frames, both slots, "
              "<= 3 DDA samples per pixel)");
    return TSDF_ERR_INVALID_ARG;
  }
  return shard_pipe_impl(e, f, K, pose, max_depth, cands_in, cands_out, nullptr, nullptr, 0, cand_cap, pending);
}

int tsdf_integrate_shard_abort(tsdf_engine* e) {
  TraceRange trace_("tsdf_integrate_shard_abort");
  if (!e || !sharded(e)) {
    set_error("tsdf_integrate_shard_abort: not a shard engine");
    return TSDF_ERR_INVALID_ARG;
  }
  if (e->shard_phase == 0 && e->ps == tsdf_engine::kPipeNone) return TSDF_OK;  // nothing pending
  HIP_OK(hipSetDevice(e->device));
  // (not ENTER: a pending pipelined sharded frame cannot be flushed without the exchange protocol --
  // it is dropped here with the rest of the frame's state)
  JOIN_RENDER(e);
  e->shard_phase = 0;
  e->shard_ev = nullptr;
  e->ps = tsdf_engine::kPipeNone;
  hipLaunchKernelGGL(k_shard_abort, dim3(1), dim3(256), 0, e->stream, e->D);
  LAUNCH_OK("k_shard_abort");
  if (int rc = upload_release(e)) return rc;
  return TSDF_OK;
}
