/*
 * disinfect_tsdf.h -- C ABI of the MI355X (gfx950) TSDF semantic-fusion engine.
 *
 * Drop-in boundary for the TSDF hot path of yuzhou42/disinfect-slam. The reference exposes this
 * path as C++ classes (no FFI): TSDFGrid (utils/tsdf/voxel_tsdf.cuh:32-124), VoxelHashTable
 * (utils/tsdf/voxel_hash.cuh:47-183), VoxelMemPool (utils/tsdf/voxel_mem.cuh:95-174) and the
 * threaded TSDFSystem facade (modules/tsdf_module.h:35-107). Each entry point below names the
 * reference interface it replaces. Plain pointers and sizes only: no HIP, torch or OpenCV types.
 * The C++17 facade in disinfect-slam_amd/host/ rebuilds TSDFGrid / TSDFSystem on top of it.
 *
 * All calls return TSDF_OK (0) or a TSDF_ERR_* code; nothing throws across this boundary
 * (the reference returns void and only printf's CUDA errors in Debug, utils/cuda/errors.cuh:9-29).
 * An engine handle is not thread safe (TSDFGrid is not re-entrant either); TSDFSystem serialises.
 */
#ifndef DISINFECT_TSDF_H
#define DISINFECT_TSDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSDF_OK 0
#define TSDF_ERR_INVALID_ARG 1
#define TSDF_ERR_OUT_OF_MEMORY 2
#define TSDF_ERR_HIP 3
#define TSDF_ERR_CAPACITY 4 /* caller buffer too small (two-call pattern) */
#define TSDF_ERR_NO_DEVICE 5
#define TSDF_ERR_PIPELINE 6 /* tsdf_synchronize: a pipelined frame's wait timed out since the last report
                               (results wrong); the status bit is cleared once reported */

#define TSDF_MEM_HOST 0   /* pointer is host memory: engine copies it (pageable is fine) */
#define TSDF_MEM_DEVICE 1 /* pointer is device memory on the engine's GPU */

/* status bits (tsdf_stats.status): sticky, cleared by tsdf_get_stats(..., clear=1) */
#define TSDF_STATUS_POOL_EXHAUSTED 1u  /* an allocation found no free block (voxel_mem.cu:39) */
#define TSDF_STATUS_NEWKEY_OVERFLOW 2u /* more new blocks in one frame than the key set holds */
#define TSDF_STATUS_DDA_OVERFLOW 4u    /* a DDA ray took more samples than sized for */
#define TSDF_STATUS_RESOLVE_ABORT 8u   /* allocation resolver made no progress (internal error) */
#define TSDF_STATUS_SHARD_OVERFLOW 16u /* a sharded frame had more keys / candidates than a slot holds */
#define TSDF_STATUS_SHARD_ABORTED 32u  /* a pending sharded frame was aborted (the shards may differ) */
#define TSDF_STATUS_PIPELINE_TIMEOUT 64u /* a pipelined frame's in-kernel wait timed out (internal error) */

typedef struct tsdf_engine tsdf_engine;
typedef struct tsdf_graph tsdf_graph;

typedef struct tsdf_config {
  float voxel_size;   /* [m] TSDFGrid(voxel_size, truncation), voxel_tsdf.cuh:40 */
  float truncation;   /* [m] */
  int max_width;      /* largest integrate / raycast image; reference MAX_IMG_* = 1920x1080 */
  int max_height;     /*   (voxel_tsdf.cu:10-12) */
  int num_block_bits; /* voxel-block pool = 2^bits blocks; reference NUM_BLOCK_BITS 18 */
  int shard_index;    /* spatial sharding: this engine holds the voxels of blocks b with */
  int shard_count;    /*   owner(b) = hash(b >> 2) mod count == index; 1 = unsharded (<= 64) */
  void* stream;       /* hipStream_t to run on when use_stream != 0 (NULL then means the legacy */
  int use_stream;     /*   default stream); use_stream == 0: an engine-owned stream */
} tsdf_config;

/* Fill reference defaults: 5 mm / 3 cm, 1920x1080, 2^18 blocks, unsharded. */
void tsdf_config_default(tsdf_config* cfg);

typedef struct tsdf_intrinsics { /* CameraIntrinsics<float> (utils/cuda/camera.cuh:12-51) */
  float fx, fy, cx, cy;
} tsdf_intrinsics;

typedef struct tsdf_pose { /* SE3<float> cam_T_world (utils/cuda/lie_group.cuh:6-45) */
  float qx, qy, qz, qw;    /* Eigen::Quaternionf coefficients (x, y, z, w) */
  float tx, ty, tz;
} tsdf_pose;

typedef struct tsdf_frame { /* the four cv::Mat inputs of TSDFGrid::Integrate (voxel_tsdf.cuh:58) */
  int width, height;
  const uint8_t* rgb;  /* height x width x 3, RGB order (CV_8UC3) */
  const float* depth;  /* height x width metres (CV_32FC1); 0 = invalid */
  const float* ht;     /* height x width high-touch probability; NULL -> all ones */
  const float* lt;     /* height x width low-touch probability;  NULL -> all ones */
  int mem_kind;        /* TSDF_MEM_HOST or TSDF_MEM_DEVICE (all four pointers alike) */
} tsdf_frame;

typedef struct tsdf_voxel { /* VoxelSpatialTSDF (utils/tsdf/voxel_types.cuh:48-57), 16 B */
  float x, y, z, tsdf;
} tsdf_voxel;

typedef struct tsdf_stats {
  int64_t frames;            /* integrate calls so far */
  int32_t active_blocks;     /* VoxelHashTable::NumActiveBlock (voxel_hash.cu:207) */
  int32_t free_blocks;       /* VoxelMemPool::NumFreeBlocks (voxel_mem.cu:63-67) */
  int32_t last_num_visible;  /* N_vis of the last integrate */
  int32_t last_num_alloc;    /* blocks allocated by the last integrate */
  int32_t last_num_deleted;  /* blocks removed by space carving in the last integrate */
  int32_t last_num_new_keys; /* unique missing visible keys the last DDA produced */
  int64_t last_num_updated;  /* voxels updated by the last integrate */
  int64_t total_visible;     /* sum of N_vis over all integrate calls */
  int64_t total_updated;     /* sum of updated voxels over all integrate calls */
  int64_t total_alloc;
  int64_t total_deleted;
  uint32_t status;           /* TSDF_STATUS_* bits */
  uint32_t reserved;
} tsdf_stats;

typedef struct tsdf_profile { /* device time of the integrate phases between begin/end */
  int64_t frames;      /* integrate calls that were event-timed (every `every`-th call) */
  double ms_allocate;  /* DDA + visibility sweep of the existing blocks (one kernel) + ordered
                          allocation resolve, which lists the new blocks as visible */
  double ms_visible;   /* ~0: visibility runs inside the allocate phase (kept for the layout) */
  double ms_integrate; /* the fused TSDF/RGB/weight/semantic update kernel (+ carve minimum) */
  double ms_carve;     /* space-carving compaction + delete resolve */
  int64_t sum_visible; /* sum of N_vis over the profiled frames */
  int64_t sum_updated; /* sum of updated voxels over the profiled frames */
  double ms_integrate_device; /* k_integrate first-workgroup start -> last-workgroup end, summed
                                 over the profiled frames (in-kernel 100 MHz clock; excludes the
                                 dispatch overhead the HIP events of ms_integrate include) */
  int64_t calls;       /* all integrate calls between begin and end (sum_* and the device
                          clock cover all of them; the ms_* event times only `frames`) */
  /* in-kernel 100 MHz clock, summed over the calls (the two resolvers run inside the ingest and
     update kernels' last-arriving workgroups, so no kernel trace can time them apart): */
  double ms_ingest_device;          /* k_ingest_dda start -> its last workgroup's arrival */
  double ms_resolve_alloc_device;   /* ordered allocation resolve (VoxelHashTable::Allocate) */
  double ms_resolve_delete_device;  /* ordered carving resolve (VoxelHashTable::Delete) */
  int64_t pipelined;   /* pipelined frame launches (k_frame: the previous frame's carving, this
                          frame's allocation and update, the next frame's ingest; their events /
                          device clock include that work) */
} tsdf_profile;

/* ---- engine lifetime: TSDFGrid::TSDFGrid / ~TSDFGrid (voxel_tsdf.cu:309-345) ---- */
int tsdf_create(const tsdf_config* cfg, int device, tsdf_engine** out);
int tsdf_destroy(tsdf_engine* e);

/* TSDFGrid::Integrate (voxel_tsdf.cu:347-375): allocate -> visibility -> update -> carve.
 * Asynchronous on the engine stream when the frame is TSDF_MEM_DEVICE (inputs must stay valid
 * until the next engine call or tsdf_synchronize); host frames are copied before returning.
 * Pipelined frames (one volume, truncation / voxel <= 6 -- at most 3 DDA samples per pixel): the
 * frame's allocation is enqueued at once and its update / carving is deferred; the next
 * tsdf_integrate enqueues it in one launch with the next frame's pixel work, and every other entry
 * point that reads or writes the volume (raycast, query, stats, snapshots, mesh, ..., tsdf_flush,
 * tsdf_synchronize) enqueues it first, so every observable result is that of the frames in order.
 * tsdf_stream_wait / tsdf_stream_signal do not enqueue it (they order the frame's inputs, which the
 * deferred part no longer reads). TSDF_PIPELINE=0 in the environment disables the deferral (on by default). */
int tsdf_integrate(tsdf_engine* e, const tsdf_frame* frame, const tsdf_intrinsics* K,
                   const tsdf_pose* cam_T_world, float max_depth);
/* Enqueue a deferred update (pipelined frames) on the engine stream without waiting for it: after
 * tsdf_flush, a synchronisation of the engine stream covers every frame integrated so far. */
int tsdf_flush(tsdf_engine* e);

/* Sharded volume (no reference counterpart: TSDFGrid is single-GPU). An engine
 * created with shard_count > 1 is shard `shard_index` of one volume: it keeps the whole hash index
 * (VoxelHashTable, voxel_hash.cuh:47-183) and holds the voxels of the blocks whose 4^3-block brick
 * hashes to it (tsdf_block_owner). Every shard applies every Allocate / Delete to its index --
 * another shard's block is an occupied entry without voxels here -- so the bucket-lock outcomes
 * (one structural change per bucket per launch, voxel_hash.cu:80-118,137-170) are those of ONE
 * volume, and the union of the shards equals the unsharded volume block for block and voxel for
 * voxel. TSDFGrid::Integrate (voxel_tsdf.cu:347-375) of a shard is three calls around two
 * exchanges, all asynchronous on the engine stream:
 *   1. tsdf_integrate_shard_begin: the visibility of this shard's blocks and the
 *      block_allocate_kernel DDA (voxel_tsdf.cu:104-147) over slice `slice_index` of `slice_count`
 *      (bands of 16-pixel tile rows). No pixel records are packed: the update in _update gathers
 *      the raw frame again, so a DEVICE frame (depth, rgb, ht, lt) must stay allocated and
 *      unmodified until _update has been enqueued and has run in stream order (a host frame is
 *      staged by _begin and may be reused at once). The keys it finds missing from the index go to
 *      keys_out: one slot of
 *      tsdf_shard_slot_bytes(key_cap) bytes (record 0 = count header, then 16-B records).
 *      slice_count == 1 with keys_out == NULL: every shard runs the whole DDA and finds the same
 *      keys itself, so no key exchange is needed (keys_in NULL below).
 *   2. the caller all-gathers the key slots (e.g. RCCL all-gather over xGMI): keys_in = shard_count
 *      slots, slot s from shard s. tsdf_integrate_shard_update merges them (smallest candidate
 *      order per key = the whole frame's DDA), runs the ordered allocation (pool blocks only for
 *      owned keys), the fused update of this shard's visible blocks, and writes its space-carving
 *      candidates (space_carving_kernel, voxel_tsdf.cu:207-230) to cands_out (one slot).
 *   3. the caller all-gathers the candidate slots; tsdf_integrate_shard_end deletes the union in
 *      hash-entry order (every shard's index) and releases this shard's pool blocks.
 * Exchanges must be ordered between the calls on the engine stream (same stream, or
 * tsdf_stream_wait / tsdf_stream_signal). No other engine call may come between _begin and _end;
 * tsdf_integrate / feed / graph frames refuse a shard. More records than a slot holds set
 * TSDF_STATUS_SHARD_OVERFLOW (the shards then diverge: size the caps for the first frame). */
int64_t tsdf_shard_slot_bytes(int32_t cap);
/* Pipelined sharded frames: ONE exchange per frame (no reference counterpart; the sharded form of
 * TSDFGrid::Integrate, voxel_tsdf.cu:347-375, pipelined like tsdf_integrate). Every shard runs the
 * whole frame's DDA against its copy of the index, so the new keys need no exchange and only the
 * carve candidates cross the shards. Per frame, on every shard: tsdf_integrate_shard_pipe(frame,
 * cands_in, cands_out), then the caller all-gathers cands_out (one slot of
 * tsdf_shard_slot_bytes(cand_cap)) into cands_in (shard_count slots, slot s from shard s) for the next
 * call. The call carves the frame before the previous one (every shard's candidates, from cands_in),
 * allocates and updates the previous frame (this shard's candidates into cands_out) and ingests this
 * one. To complete the frames: call with frame == NULL (and the exchange after each call) until
 * *pending is 0. Until then every other volume entry point returns TSDF_ERR_INVALID_ARG. The frame's
 * buffers are read by this call only. */
int tsdf_integrate_shard_pipe(tsdf_engine* e, const tsdf_frame* frame, const tsdf_intrinsics* K,
                              const tsdf_pose* cam_T_world, float max_depth, const void* cands_in,
                              void* cands_out, int32_t cand_cap, int32_t* pending);
int tsdf_integrate_shard_begin(tsdf_engine* e, const tsdf_frame* frame, const tsdf_intrinsics* K,
                               const tsdf_pose* cam_T_world, float max_depth, int32_t slice_index,
                               int32_t slice_count, void* keys_out, int32_t key_cap);
int tsdf_integrate_shard_update(tsdf_engine* e, const void* keys_in, int32_t key_cap, void* cands_out,
                                int32_t cand_cap);
int tsdf_integrate_shard_end(tsdf_engine* e, const void* cands_in, int32_t cand_cap);
/* Abort a pending sharded frame (e.g. a failed exchange between the phases) or the pending frames of
 * tsdf_integrate_shard_pipe: the engine returns to "between frames" so later calls (a new frame,
 * reset, snapshot_load, ...) work again. Structural changes a phase already made stay, so the shards
 * may no longer agree: TSDF_STATUS_SHARD_ABORTED is set, and the caller should restore every shard
 * from a snapshot (or reset, which also drops pending pipelined shard frames). No pending frame: OK. */
int tsdf_integrate_shard_abort(tsdf_engine* e);

/* ---- A sharded volume owned by the library (SURVEY.md 8b tsdf_create_sharded; no reference
 * counterpart: TSDFGrid, voxel_tsdf.cu:309-375, is single-GPU). ONE volume spatially sharded over n
 * engines of this process -- shard i on devices[i]; a device may repeat (several shards of one GPU) --
 * running the pipelined sharded frames of tsdf_integrate_shard_pipe with the exchange inside the
 * library: each shard's update kernel writes its carve candidates straight into every shard's inbox
 * (device stores, peer stores over xGMI between GPUs; no copy, no host round trip, no collective
 * library), inboxes double-buffered by call parity. Shards of one device share one stream; across
 * devices each call waits for the previous call of every other device (events). The union of the
 * shards equals the unsharded volume block for block and voxel for voxel; truncation / voxel <= 6.
 * cfg: as tsdf_create (shard_index / shard_count / stream are the group's). Frames: host memory, or
 * device memory on devices[0] (copied to the other devices). tsdf_group_integrate is pipelined like
 * tsdf_integrate; every other group call (flush, stats, query, raycast, shard, synchronize) first
 * completes the pending frames. tsdf_group_query returns the unsharded volume's voxels shard by shard
 * (each shard in entry order); tsdf_group_raycast renders exactly what the unsharded volume renders
 * (render replicas into an engine on devices[0]); tsdf_group_shard gives shard i's engine (e.g. for
 * tsdf_debug_dump); tsdf_group_get_stats sums the shards' counts (each holds, acquires, releases,
 * sees and updates its own blocks: the sums are the unsharded volume's), frames and new keys once.
 * n = 1 is one unsharded engine behind the same calls (tsdf_integrate's pipelined frames). */
typedef struct tsdf_group tsdf_group;
int tsdf_group_create(const tsdf_config* cfg, const int* devices, int n, tsdf_group** out);
int tsdf_group_destroy(tsdf_group* g);
int tsdf_group_size(const tsdf_group* g);
int tsdf_group_integrate(tsdf_group* g, const tsdf_frame* frame, const tsdf_intrinsics* K,
                         const tsdf_pose* cam_T_world, float max_depth);
int tsdf_group_flush(tsdf_group* g);
int tsdf_group_synchronize(tsdf_group* g);
int tsdf_group_shard(tsdf_group* g, int index, tsdf_engine** out);
int tsdf_group_get_stats(tsdf_group* g, tsdf_stats* out, int clear_status);
int tsdf_group_query(tsdf_group* g, const float* bounds, tsdf_voxel* out, int64_t capacity, int64_t* count);
int tsdf_group_raycast(tsdf_group* g, const tsdf_intrinsics* K, int width, int height,
                       const tsdf_pose* cam_T_world, float max_depth, uint8_t* rgba, uint8_t* normal,
                       int mem_kind);
/* Orders `stream` (a hipStream_t of devices[0]) after every shard's queued work: a device frame passed to
 * tsdf_group_integrate is read by the group's own streams after the call returns (its launch, and the
 * peer copies to the other devices), so a caller that reuses or frees the frame's memory on its stream
 * calls this first (the Python Group does, after every device-frame integrate) -- the group's analogue of
 * tsdf_stream_signal. Does not complete pending frames and does not wait on the host. */
int tsdf_group_stream_signal(tsdf_group* g, void* stream);

/* Stream ordering with a caller's HIP stream (e.g. torch's current stream) for device buffers
 * passed to an engine that runs on its own stream: tsdf_stream_wait makes the engine stream wait
 * for the work queued on `stream` so far (before the engine reads a buffer the caller wrote);
 * tsdf_stream_signal makes `stream` wait for the engine's queued work (before the caller reads a
 * buffer the engine wrote, or frees one it reads). tsdf_get_stream returns the engine stream. */
int tsdf_stream_wait(tsdf_engine* e, void* stream);
int tsdf_stream_signal(tsdf_engine* e, void* stream);
int tsdf_get_stream(tsdf_engine* e, void** stream);

/* DISINFSystem::feed_rgbd_frame (disinfect_slam/disinfect_slam.cc:31-67) after the pose lookup:
 * cv::resize(x0.5) of rgb (height x width x 3 u8), depth (height x width u16 raw sensor units) and
 * the optional mask (height x width u8, NULL = none), depth.convertTo(CV_32FC1, 1 / depth_factor),
 * depth = 0 where the resized mask is 0, then TSDFGrid::Integrate of the (width/2 x height/2)
 * frame with ht = lt = ones, all on the GPU. width and height must be even (OpenCV's fast 2x2 area
 * path; see csrc/tsdf_frontend.hip). K is the intrinsics of the half-size image. */
int tsdf_feed_rgbd_frame(tsdf_engine* e, const uint8_t* rgb, const uint16_t* depth,
                         const uint8_t* mask, int width, int height, float depth_factor,
                         const tsdf_intrinsics* K, const tsdf_pose* cam_T_world, float max_depth,
                         int mem_kind);
/* The preprocessing step alone: rgb_out (height/2 x width/2 x 3 u8), depth_out (f32), in host or
 * device memory like the inputs (mem_kind). */
int tsdf_rgbd_half(tsdf_engine* e, const uint8_t* rgb, const uint16_t* depth, const uint8_t* mask,
                   int width, int height, float depth_factor, uint8_t* rgb_out, float* depth_out,
                   int mem_kind);

/* Graph-captured frame loop (BASELINE config C5): TSDFGrid::Integrate (+ optionally RayCast of a
 * render camera into device buffers) as ONE hipGraph launch per frame, with the same results as
 * tsdf_integrate + tsdf_raycast(TSDF_MEM_DEVICE). A graph is bound to one engine, one frame size and
 * one render size (0 x 0 = no raycast). tsdf_graph_frame takes device frames (TSDF_MEM_DEVICE) that
 * must stay valid until the frame has run (tsdf_synchronize); rgba / normal are device buffers of
 * render_height x render_width x 4 u8 (either may be NULL). Asynchronous; profiling events are
 * not recorded for graph frames. */
int tsdf_graph_create(tsdf_engine* e, int width, int height, int render_width, int render_height,
                      tsdf_graph** out);
/* A render-deferring graph (the C5 loop's form of tsdf_raycast_deferred): each frame's raycast is
 * rendered by the graph's NEXT launch, in one kernel with that frame's ingest (k_render_ingest_g), or
 * by the engine's next other call (tsdf_flush, tsdf_synchronize, a query, ...), which launches it
 * alone first. So frame i's rgba / normal are complete once tsdf_graph_frame(i + 1) -- or any other
 * call -- has run, in engine-stream order, and must stay valid until then. Images, volume and
 * statistics are identical to tsdf_graph_create's. Views too deep for a view grid render right after
 * their frame's graph launch. */
int tsdf_graph_create_deferred(tsdf_engine* e, int width, int height, int render_width, int render_height,
                               tsdf_graph** out);
/* A batched graph: each hipGraphLaunch runs frames_per_launch (<= 32) consecutive frames -- their
 * arguments uploaded by one node, their nodes back to back -- so the launch's fixed cost (on this ROCm
 * ~13.5 us of idle GPU between launches) is paid once per batch. tsdf_graph_frame writes a
 * frame into the current batch and launches the batch when it is full; the engine's next other call
 * (tsdf_flush, tsdf_synchronize, a query, another graph's frame, ...) launches a partly filled batch
 * first (its frames one by one). So a frame's outputs (its volume update, rgba / normal) are written
 * once its batch has launched, in engine-stream order; everything else as tsdf_graph_create (deferred
 * != 0: tsdf_graph_create_deferred), results identical. */
int tsdf_graph_create_batch(tsdf_engine* e, int width, int height, int render_width, int render_height,
                            int deferred, int frames_per_launch, tsdf_graph** out);
int tsdf_graph_frame(tsdf_graph* g, const tsdf_frame* frame, const tsdf_intrinsics* K,
                     const tsdf_pose* cam_T_world, float max_depth, const tsdf_intrinsics* render_K,
                     const tsdf_pose* render_cam_T_world, uint8_t* rgba, uint8_t* normal);
int tsdf_graph_destroy(tsdf_graph* g);
/* A shard's graph frames (BASELINE config C5 on a sharded volume): the sharded frame of
 * tsdf_integrate_shard_* as three captured segments around the caller's two exchanges --
 *   tsdf_graph_shard_begin: the DDA of slice slice_index of slice_count (keys into keys_out; with
 *     slice_count 1 every shard runs the whole DDA and keys_out / keys_in are unused);
 *   (the caller all-gathers the key slots into keys_in) tsdf_graph_shard_update: merge, allocate,
 *     update this shard's blocks (raw frame), carve candidates into cands_out;
 *   (the caller all-gathers the candidate slots into cands_in) tsdf_graph_shard_end: the deletes.
 * Every buffer is named at _begin (device memory, valid until _end has run). The exchanges are not
 * recorded into the engine's graphs: stream-ordered collectives of another library (RCCL through
 * torch.distributed) cannot be captured into a graph this library owns. Same results as
 * tsdf_integrate_shard_*. */
int tsdf_graph_create_shard(tsdf_engine* e, int width, int height, int slice_index, int slice_count,
                            tsdf_graph** out);
int tsdf_graph_shard_begin(tsdf_graph* g, const tsdf_frame* frame, const tsdf_intrinsics* K,
                           const tsdf_pose* cam_T_world, float max_depth, void* keys_out,
                           const void* keys_in, int32_t key_cap, void* cands_out, const void* cands_in,
                           int32_t cand_cap);
int tsdf_graph_shard_update(tsdf_graph* g);
int tsdf_graph_shard_end(tsdf_graph* g);

/* TSDFGrid::RayCast (voxel_tsdf.cu:490-506; ray_cast_kernel :232-307). rgba / normal are
 * height x width x 4 u8 (either may be NULL), host or device memory per mem_kind. */
int tsdf_raycast(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                 const tsdf_pose* cam_T_world, float max_depth, uint8_t* rgba, uint8_t* normal,
                 int mem_kind);
/* tsdf_raycast into device buffers with its k_raycast launch deferred to the engine's next call: when
 * that call is tsdf_integrate, the raycast runs in ONE launch with the new frame's ingest (pixel
 * records, DDA, visibility sweep, allocation -- which write nothing the raycast reads), filling the
 * slots the latency-bound raycast leaves; any other call (tsdf_flush, tsdf_synchronize, a query, ...)
 * launches it alone first. The images are those of the volume at this call (bit-identical to
 * tsdf_raycast); they are written in engine-stream order by that next call, so a consumer orders
 * after it (or calls tsdf_flush). rgba / normal must stay valid until then. Views too deep for a view
 * grid take tsdf_raycast's immediate path. (The C5 loop: examples/tsdf/online.cc:60 +
 * modules/renderer_module.cc:105 integrate then render every frame.) */
int tsdf_raycast_deferred(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                          const tsdf_pose* cam_T_world, float max_depth, uint8_t* rgba, uint8_t* normal);

/* TSDFGrid::GatherVoxels (bounds = {xmin, xmax, ymin, ymax, zmin, zmax}, voxel_tsdf.cu:427-454)
 * or GatherValid (bounds == NULL, :399-425). Two-call pattern: *count receives the number of
 * voxels (blocks x 512, entry order then OffsetToIndex); out (host) is filled when non-NULL and
 * capacity >= *count, else TSDF_ERR_CAPACITY. */
int tsdf_query(tsdf_engine* e, const float* bounds, tsdf_voxel* out, int64_t capacity,
               int64_t* count);

/* Render replicas of a spatially sharded volume (the raycast composite SURVEY.md 8e
 * names). The blocks a raycast of (K, W, H, pose, max_depth) can read -- a conservative superset --
 * are packed as TSDF_BLOCK_RECORD_BYTES records {int16 x, y, z, 0; 8 zero bytes; the 6 KiB block:
 * tsdf f32[512], prob f32[512], rgbw u8x4[512]} in entry order. Two-call: out == NULL returns
 * *count only; then out must hold capacity >= *count records (host or device memory per mem_kind).
 * tsdf_import_blocks allocates every record's block in the engine (resolver launches until none is
 * missing) and writes its payload; replace != 0 first empties the volume (table, occupancy, free
 * stack, counters; free pool blocks keep stale contents, which nothing reads), so the engine then
 * holds exactly the records' blocks. A scratch engine that imported every shard's records renders
 * with tsdf_raycast exactly what the unsharded volume renders (ray_cast_kernel,
 * voxel_tsdf.cu:232-307). tsdf_reset empties an engine to its state as created (pool included).
 * No reference counterpart: TSDFGrid is single-GPU. */
#define TSDF_BLOCK_RECORD_BYTES 6160
int tsdf_render_blocks(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                       const tsdf_pose* cam_T_world, float max_depth, void* out, int64_t capacity,
                       int64_t* count, int mem_kind);
int tsdf_import_blocks(tsdf_engine* e, const void* records, int64_t n, int mem_kind,
                       int replace);
int tsdf_reset(tsdf_engine* e);
/* The same records for the Query block selection (bounds as tsdf_query, NULL = every live block):
 * a replica that imports every shard's records with bounds NULL is the whole unsharded volume, so
 * its tsdf_extract_mesh equals the unsharded mesh (as a set of triangles). */
int tsdf_pack_blocks(tsdf_engine* e, const float* bounds, void* out, int64_t capacity,
                     int64_t* count, int mem_kind);

/* Sharded extraction that divides the work (no reference counterpart):
 * - tsdf_raycast_rows: rows [row0, row0 + nrows) of the W x H raycast of tsdf_raycast, bit for bit the
 *   same pixels, into rgba / normal of nrows x width x 4 u8 (ray_cast_kernel, voxel_tsdf.cu:232-307).
 * - tsdf_render_bands: the shard's own blocks a raycast of rows [rows[b], rows[b + 1]) can read, for
 *   each band b < nbands (<= 64): the records of tsdf_render_blocks, grouped band by band, counts[b]
 *   per band (a block may be in several bands). Two-call: out == NULL returns the counts. Each rank of
 *   a sharded render sends band b's records to the rank that renders band b (an all-to-all), imports
 *   what it receives into a replica and renders its band with tsdf_raycast_rows.
 * - tsdf_pack_halo: a shard's own blocks that another shard's marching cubes read -- the blocks with a
 *   neighbour (of 26) owned by shard d go to group d (counts[shard_count]); the caller routes group d
 *   to shard d. A replica holding a shard's own blocks (tsdf_pack_blocks) plus the halo it received
 *   meshes that shard's part of the volume with tsdf_extract_mesh_owned.
 * - tsdf_extract_mesh_owned: tsdf_extract_mesh of the blocks whose brick owner
 *   (tsdf_block_owner(., shard_count)) is shard_index; the other selected blocks are read as
 *   neighbours only. The shards' parts together are the volume's mesh (as a set of triangles). */
int tsdf_raycast_rows(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                      const tsdf_pose* cam_T_world, float max_depth, int row0, int nrows, uint8_t* rgba,
                      uint8_t* normal, int mem_kind);
int tsdf_render_bands(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                      const tsdf_pose* cam_T_world, float max_depth, int nbands, const int32_t* rows,
                      void* out, int64_t capacity, int64_t* counts, int mem_kind);
int tsdf_pack_halo(tsdf_engine* e, void* out, int64_t capacity, int64_t* counts, int mem_kind);
int tsdf_extract_mesh_owned(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                            int shard_index, int shard_count, float* triangles, int64_t capacity,
                            int64_t* num_triangles, int mem_kind);

/* Marching-cubes mesh of the volume (GPU; replaces Query + KrisLibrary
 * SparseTSDFReconstruction::ExtractMesh in examples/ros_camera_driver/ros_offline.cc:258-318).
 * bounds as tsdf_query (NULL = every allocated block). Samples sit at voxel centres + half a
 * voxel (ros_offline.cc:281-283); a voxel of a selected block contributes its tsdf when its
 * weight >= min_weight (0 = every voxel, like the reference), every other grid point reads
 * missing_tsdf (KrisLibrary defaultValue = truncation distance; 0.99 ~ the reference's auto
 * value). Output: triangles[9 * i .. 9 * i + 8] = three xyz vertices, normals (right-hand
 * rule) toward increasing tsdf; deterministic order (blocks in hash-entry order). Two-call:
 * triangles == NULL returns the count only. mem_kind: where `triangles` lives. A device
 * `triangles` buffer may be passed in ONE call: *num_triangles is always set, and when it
 * exceeds capacity nothing is written and TSDF_ERR_CAPACITY is returned. */
int tsdf_extract_mesh(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                      float* triangles, int64_t capacity, int64_t* num_triangles, int mem_kind);

/* The same mesh with shared vertices and the volume's semantics attached: what the reference
 * publishes as shape_msgs::Mesh from Meshing::TriMesh verts + tris in tsdfCb
 * (examples/ros_camera_driver/ros_offline.cc:286-313), plus colour and high-touch probability.
 * Block selection, sampling rule, meshed cells, triangle order and winding are those of
 * tsdf_extract_mesh: triangle i is triangle i of the soup, positions[indices[...]] equals it bit for
 * bit.
 * Vertices: one per crossed grid edge (one sample < 0, the other not). Endpoint a is the lower one
 * along the edge's axis, b = a + 1 on it. keys = global voxel coordinate of a (8 * block + local),
 * then the axis 0 / 1 / 2: the vertex's identity across extractions. Two crossed edges with one
 * position (tt == 0 at a shared corner) stay two vertices.
 *   position: tt = va / (va - vb); axis coordinate pa + tt * (pb - pa) (the soup's expression);
 *   an endpoint is valid when its tsdf, not missing_tsdf, was its sample. Both valid:
 *   prob = qa + tt * (qb - qa), each rgbw byte (uint8_t)(int)(fa + tt * (fb - fa) + 0.5f), all
 *   fp32 op by op; one valid: that endpoint's prob and rgbw unchanged.
 * Vertex order: selected blocks in entry order; an edge belongs to the block of its lower endpoint
 * when that block is selected, else to the block of its upper endpoint (the lower endpoint then has
 * local coordinate -1 on the axis); inside a block by the lower endpoint's local (z, y, x), then
 * the axis. The order does not depend on launch sizes or scheduling.
 * out == NULL: the two counts only. TSDF_MEM_HOST: the two-call pattern. TSDF_MEM_DEVICE: one call
 * may do everything; both counts are always set, and when either capacity is too small (or there
 * are more than INT32_MAX vertices) nothing is written and TSDF_ERR_CAPACITY is returned.
 * positions and indices are required with out. Completes a pending pipelined frame first. Not
 * available on a shard engine (shard_count > 1): TSDF_ERR_INVALID_ARG. */
typedef struct tsdf_mesh_out {
  float* positions;  /* 3 per vertex */
  uint8_t* rgba;     /* 4 per vertex: r, g, b, weight (4-byte aligned); NULL = skip */
  float* prob;       /* 1 per vertex: high-touch probability; NULL = skip */
  int32_t* keys;     /* 4 per vertex: gx, gy, gz, axis; NULL = skip */
  int32_t* indices;  /* 3 per triangle */
  int64_t vertex_capacity, triangle_capacity;
  int mem_kind;      /* TSDF_MEM_HOST or TSDF_MEM_DEVICE (all pointers alike) */
} tsdf_mesh_out;
int tsdf_extract_mesh_indexed(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                              const tsdf_mesh_out* out, int64_t* num_vertices, int64_t* num_triangles);

/* ---- Pose tracking against the volume (frame-to-model point-to-plane ICP, KinectFusion style) ----
 * All four calls complete a pending pipelined frame first and are not available on a shard engine
 * (shard_count > 1): TSDF_ERR_INVALID_ARG.
 *
 * tsdf_raycast_surface: what tsdf_raycast sees, as float maps. The march is tsdf_raycast's (view grid,
 * step = truncation / 2, sequential position sums, hit test prev > 0 && cur <= 0 && prev - cur <= 1.5):
 * a pixel has a surface only where tsdf_raycast writes alpha 255, at the same step. With hp the
 * position at the hit step and sg the step's increment (voxel units), prev / cur the march's own two
 * samples (prev = +1 after a missing block or an empty region):
 *   p1 = hp - sg; s = prev / (prev - cur); pv = p1 + s * sg; point = pv * voxel_size;
 *   depth = (cam_T_world * point).z
 * normal, prob and rgbw come from the voxel the shaded images use (the end of their binary search):
 * nr = the six-neighbour central difference (a missing neighbour reads +1), normal = nr / sqrt(nr . nr),
 * prob and rgbw that voxel's stored values (0 when its block is missing). nr . nr zero or not finite:
 * no surface. A pixel without a surface holds zeros in every map. fp32, one operation at a time. */
typedef struct tsdf_surface_out {
  float* point;    /* H x W x 3: world position of the surface [m] */
  float* normal;   /* H x W x 3: unit normal, world frame, toward increasing tsdf */
  float* depth;    /* H x W: camera z of point [m]; 0 = no surface       NULL = skip */
  float* prob;     /* H x W: high-touch probability of the hit voxel      NULL = skip */
  uint8_t* rgbw;   /* H x W x 4: the hit voxel's stored r, g, b, weight (4-byte aligned)  NULL = skip */
  int mem_kind;    /* TSDF_MEM_HOST or TSDF_MEM_DEVICE, all pointers alike */
} tsdf_surface_out;
int tsdf_raycast_surface(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                         const tsdf_pose* cam_T_world, float max_depth, const tsdf_surface_out* out);

/* tsdf_icp_linearize: one Gauss-Newton linearisation of the point-to-plane error of a depth frame at
 * the estimate cam_T_world against the maps of a tsdf_raycast_surface call. For every pixel (u, v)
 * with u % stride == 0 && v % stride == 0, in fp32 op by op:
 *   d = depth[v * W + u], kept if d > 0 && d <= max_depth; pc = (ray.x * d, ray.y * d, d) with
 *   ray = K^-1 (u, v, 1); pw = world_T_cam * pc; pm = model.cam_T_world * pw, kept if pm.z > 0;
 *   um = rint(fx_m * (pm.x / pm.z) + cx_m), vm likewise (half to even), kept inside the model map;
 *   q = point[vm, um], n = normal[vm, um], kept if n != 0; e = pw - q, kept if e . e <= max_dist^2;
 *   r = n . e; J = (pw x n, n)
 * and the sums below over the kept pixels in double (every product exact). The same arguments give
 * the same 29 doubles bit for bit: no atomics, a fixed addition tree. */
typedef struct tsdf_icp_model {          /* the maps of a tsdf_raycast_surface call */
  const float* point; const float* normal;
  int width, height; tsdf_intrinsics K; tsdf_pose cam_T_world;
} tsdf_icp_model;
/* out[0..20]  = upper triangle of A = sum J J^T, row-major (i <= j)
   out[21..26] = b = sum J r
   out[27]     = sum r^2
   out[28]     = count */
int tsdf_icp_linearize(tsdf_engine* e, const float* depth, int width, int height,
                       const tsdf_intrinsics* K, const tsdf_pose* cam_T_world /* estimate */,
                       const tsdf_icp_model* model, int stride, float max_dist, float max_depth,
                       double* out29 /* host */, int mem_kind /* depth and the model maps */);

/* tsdf_track: the pose of a depth frame. One tsdf_raycast_surface of the model from the guess with
 * (K, width, height, max_depth). The loop's model normals are taken from that call's points, not its
 * normal map (nearest-voxel central differences are too coarse where a depth pixel spans several
 * voxels): at a pixel whose four neighbours and itself have a surface,
 * c = (p[v+1][u] - p[v-1][u]) x (p[v][u+1] - p[v][u-1]), turned to face the camera, over its length;
 * no normal (the pixel is not a correspondence) on the border, beside a hole, or where c is more than
 * acos(0.3) off the viewing ray. Then per level up to iterations[l] times: tsdf_icp_linearize at
 * stride[l]; on the host in double the Cholesky solve of A xi = -b, xi = (omega, t); world_T_cam <-
 * (exp([omega]x), t) * world_T_cam; the estimate rounded to a float unit quaternion and translation.
 * TSDF_TRACK_DEGENERATE (count < min_inliers, or a Cholesky pivot <= 0 or not finite; an all-zero
 * depth frame is the first) stops with the last good estimate; the call still returns TSDF_OK.
 * rmse = sqrt(sum r^2 / count) and inliers = count of the last linearisation. */
typedef struct tsdf_track_config {
  int levels;             /* 1..3 */
  int stride[3];          /* coarse to fine */
  int iterations[3];
  float max_dist;         /* [m] correspondence gate */
  float eps_rot;          /* stop a level early when |omega| <= eps_rot and */
  float eps_trans;        /*   |t| <= eps_trans; 0 = never */
  int min_inliers;        /* fewer -> TSDF_TRACK_DEGENERATE */
} tsdf_track_config;
/* Defaults: levels = 3, stride {4, 2, 1}, iterations {4, 5, 10} (KinectFusion's schedule), max_dist =
 * 0.1 (its 10 cm gate), eps_rot = eps_trans = 0, min_inliers = 6 (the algebraic minimum) */
void tsdf_track_config_default(tsdf_track_config* cfg);
#define TSDF_TRACK_OK 0
#define TSDF_TRACK_DEGENERATE 1
typedef struct tsdf_track_result {
  tsdf_pose cam_T_world; int32_t status, iterations, inliers; float rmse;
} tsdf_track_result;
int tsdf_track(tsdf_engine* e, const float* depth, int width, int height, int mem_kind,
               const tsdf_intrinsics* K, const tsdf_pose* guess_cam_T_world, float max_depth,
               const tsdf_track_config* cfg /* NULL = defaults */, tsdf_track_result* out);

/* tsdf_point_map_normals: tsdf_track's model normals as a call, for a loop composed of
 * tsdf_raycast_surface and tsdf_icp_linearize. point and normal are the H x W x 3 maps of a
 * tsdf_raycast_surface call from (K, width, height, cam_T_world); normal says only where a surface is
 * (any component != 0). out (H x W x 3) receives the normals by tsdf_track's rule above, fp32 one
 * operation at a time: with to = p - camera centre and c turned so that c . to <= 0, a pixel keeps
 * c / sqrt(c . c) if c . c > 0 and finite and (c . to)^2 >= 0.3^2 * ((c . c) * (to . to)); zeros elsewhere.
 * Of the camera only its centre and the size are used. The three maps are host or device memory, all
 * alike (mem_kind). out must not overlap point or normal: a pixel reads its neighbours' points while
 * others are written. It is the launch tsdf_track makes. */
int tsdf_point_map_normals(tsdf_engine* e, const tsdf_intrinsics* K, int width, int height,
                           const tsdf_pose* cam_T_world, const float* point, const float* normal,
                           float* out, int mem_kind);

/* ---- UV dose on surface points (no reference counterpart: its planner receives the mesh over ROS and
 * irradiates off-board) ----
 * How much UV energy per area each surface point has received from a list of point emitters: the
 * inverse-square and cosine law, with a shadow ray marched through the volume. Receivers are any surface
 * points with unit normals: the vertices of tsdf_extract_mesh_indexed (sample_offset 0.5: the mesh's
 * half-voxel shift) or the maps of tsdf_raycast_surface (sample_offset 0). Both calls complete a pending
 * pipelined frame first, run asynchronously on the engine stream for device memory and copy for host
 * memory, are not available on a shard engine (shard_count > 1: TSDF_ERR_INVALID_ARG), only read the
 * volume and set no status bits. n == 0 (or m == 0) is TSDF_OK with nothing written.
 * Everything below is fp32, one operation at a time; dot3(a, b) = a.x b.x + (a.y b.y + a.z b.z),
 * round() is half away from zero, saturated to int16.
 *
 * tsdf_surface_normals: per component v = round(p / voxel_size - sample_offset); nr = the six-neighbour
 * central difference of the tsdf at v (a voxel of a missing block reads +1, as tsdf_raycast_surface's);
 * nn = dot3(nr, nr); the normal is nr / sqrtf(nn), or zeros unless nn > 0 && nn < inf.
 *
 * tsdf_uv_dose, receiver i with position p and normal n: an all-zero normal leaves dose[i] unchanged.
 * Otherwise acc = 0 and for the emitters k = 0 .. m - 1 in order: d = e_k - p, r2 = dot3(d, d),
 * r = sqrtf(r2), c = dot3(n, d) / r; the emitter counts when r >= min_range && r <= max_range && c > 0
 * and it is visible, and then acc = acc + (energy_k * 0.07957747f) * (c / r2)   [1 / (4 pi)].
 * Finally dose[i] = dose[i] + acc. The order of the sum is part of the contract (no atomics).
 * Visibility: o = p + bias * n; ov = o / voxel_size - sample_offset; ev = e_k / voxel_size -
 * sample_offset; dv = ev - ov; L = sqrtf(dot3(dv, dv)); sv = step / voxel_size. With !(L > 0) the only
 * sample is s_0 = ov; otherwise sg = (dv / L) * sv per component, J = (int)(L / sv), and the samples are
 * s_j = ov + (float)j * sg for j = 0 .. J (one product and one sum per component, no running sums).
 * Sample j occludes when the voxel round(s_j) lies in an allocated block, its fusion weight is
 * >= min_weight and its tsdf is <= 0. The emitter is visible when no sample occludes.
 * Also required: step > 0, max_range >= min_range, |bias| <= max_range (they bound a ray's samples). */
typedef struct tsdf_uv_emitter {
  float x, y, z; /* world position [m] */
  float energy;  /* radiant energy emitted there [J] = power [W] * dwell [s] */
} tsdf_uv_emitter;
typedef struct tsdf_uv_config {
  float bias;          /* [m] shadow ray starts at p + bias * n */
  float step;          /* [m] shadow-ray sample spacing */
  float min_range;     /* [m] > 0; an emitter nearer than this contributes nothing */
  float max_range;     /* [m] one farther contributes nothing; max_range / step <= 65536 */
  float sample_offset; /* [voxels] voxel coordinate of world x is x / voxel_size - sample_offset:
                          0 for tsdf_raycast_surface points, 0.5 for mesh vertices */
  int min_weight;      /* a voxel occludes only with fusion weight >= this */
  int use_grid;        /* 1: the call may build a dense block grid over the rays to skip empty space;
                          0: hash lookups only. Same bytes either way */
} tsdf_uv_config;
/* bias = 2 voxels, step = 1 voxel, min_range 0.05, max_range 5, sample_offset 0, min_weight 1, use_grid 1 */
void tsdf_uv_config_default(const tsdf_engine* e, tsdf_uv_config* cfg);
int tsdf_surface_normals(tsdf_engine* e, const float* points, int64_t n, float sample_offset,
                         float* normals, int mem_kind);
int tsdf_uv_dose(tsdf_engine* e, const float* points, const float* normals, int64_t n,
                 const tsdf_uv_emitter* emitters /* host */, int32_t m, const tsdf_uv_config* cfg /* NULL = defaults */,
                 float* dose /* n, in/out [J/m^2] */, int mem_kind /* points, normals, dose alike */);

/* ---- Lamp-stop planning: batched irradiance and a greedy choice of stops (no reference counterpart) ----
 * tsdf_uv_irradiance: the dose each of C candidate lamp placements alone would add to each of n receivers,
 * as a C x n matrix from one call. Candidate c's emitters are emitters[first[c] .. first[c + 1] - 1];
 * first holds C + 1 offsets and first[C] is the number of emitters the caller's array holds.
 * out[c * n + i] is exactly the acc of tsdf_uv_dose above for receiver i over candidate c's emitters in that
 * order: the bytes tsdf_uv_dose writes into a zero dose given only those emitters. A zero normal gives 0; a
 * candidate that is empty, out of range or fully shadowed gives a row of zeros. The answer does not depend
 * on use_grid, on the other candidates of the batch or on mem_kind. Required: first[0] == 0, first
 * non-decreasing, and tsdf_uv_dose's conditions on the configuration; anything else is
 * TSDF_ERR_INVALID_ARG. n == 0 or C == 0 is TSDF_OK with nothing written. Like the dose calls it completes a
 * pending pipelined frame first, runs asynchronously on the engine stream for device memory and copies for
 * host memory, refuses a shard engine, only reads the volume and sets no status bits. C * n may pass 2^31.
 *
 * tsdf_uv_plan: greedy selection on such a matrix E. need[i] is the dose receiver i still lacks, weight[i]
 * what a joule per square metre is worth there (e.g. vertex area * touch probability; finite and >= 0).
 * Rounds r = 0, 1, ... run while r < max_stops. In fp32, one operation at a time:
 *   g(c, i) = E[c][i] > 0 && need[i] > 0 ? weight[i] * fminf(E[c][i], need[i]) : 0
 * -- for every input that is not a NaN this is t = fminf(E[c][i], need[i]), g = t > 0 ? weight[i] * t : 0;
 * written with both tests a NaN in E or need contributes nothing, where fminf alone would hand its partner
 * through. G[c] is the sum of g(c, i) over i in double, by a fixed addition tree that depends on n only (no
 * atomics; the same in every round and for every candidate; DESIGN.md "Lamp-stop planning" gives it). b is
 * the lowest c with the largest G[c]. The loop stops when !(G[b] > 0) || !(G[b] >= min_gain). Otherwise
 * stops[r] = b, gains[r] = G[b], and in fp32 need[i] = fmaxf(need[i] - E[b][i], 0) for the entries with
 * E[b][i] > 0; every other entry stays as it is. A candidate may be picked again (a longer dwell). The same
 * inputs give the same stops, gains and need, bit for bit.
 * *num_stops is the number of rounds that chose a stop; entries of stops / gains past it are not written.
 * C == 0, n == 0 or max_stops == 0 is TSDF_OK with *num_stops = 0. Required: 0 <= max_stops <= 65536,
 * min_gain not a NaN. irradiance, need and weight are mem_kind memory alike; stops, gains and num_stops are
 * host memory, and the call returns after one synchronisation of the engine stream (no read per round).
 * It does not touch the volume: the engine lends its stream and scratch (grown on demand, freed by
 * tsdf_destroy), pending frames stay pending, and a shard engine (shard_count > 1) serves as well as any
 * other. */
int tsdf_uv_irradiance(tsdf_engine* e, const float* points, const float* normals, int64_t n,
                       const tsdf_uv_emitter* emitters /* host, all candidates concatenated */,
                       const int32_t* first /* host, C + 1 offsets into emitters */, int32_t C,
                       const tsdf_uv_config* cfg /* NULL = defaults */,
                       float* out /* C x n, row-major: row c = candidate c */, int mem_kind);
typedef struct tsdf_uv_plan_config {
  int32_t max_stops; /* rounds at most */
  float min_gain;    /* a round whose best gain is below this ends the plan */
} tsdf_uv_plan_config;
/* max_stops 16, min_gain 0 */
void tsdf_uv_plan_config_default(tsdf_uv_plan_config* cfg);
int tsdf_uv_plan(tsdf_engine* e, const float* irradiance /* C x n */, int32_t C, int64_t n,
                 float* need /* n, in/out [J/m^2] */, const float* weight /* n, NULL = all 1 */,
                 const tsdf_uv_plan_config* cfg /* NULL = defaults */, int32_t* stops /* host, max_stops */,
                 double* gains /* host, max_stops */, int32_t* num_stops /* host */, int mem_kind);

/* ---- Box calls: the limits of every box of voxels the calls below take ----
 * A box is dims = (nx, ny, nz) voxels, with an origin in global voxel coordinates where a call reads the volume
 * or a layer. Every box call requires each dims[i] in 1 .. TSDF_BOX_MAX_DIM and nx * ny * nz <=
 * TSDF_BOX_MAX_VOXELS: "the box limits" below. */
#define TSDF_BOX_MAX_DIM 2048
#define TSDF_BOX_MAX_VOXELS ((int64_t)1 << 28)

/* ---- Euclidean distance field over a box of the volume (no reference counterpart) ----
 * The exact squared Euclidean distance, in voxels, from every voxel of a box to the nearest surface
 * voxel of the volume -- the layer a planner asks for clearance, which the TSDF only knows inside its
 * truncation band. All integers apart from the two float comparisons below, so the result is exact.
 * For a voxel v (global voxel coordinates 8 * block + local):
 *   observed(v): the block of v is allocated and the voxel's fusion weight is >= min_weight;
 *   inside(v):   observed(v) && tsdf(v) <= 0 (the raycast's hit test, the dose's occlusion test);
 *   free(v):     observed(v) && !inside(v);
 *   surface(v):  inside(v) and at least one of the six face neighbours of v is free. The neighbours are
 *                read from the volume, also when they lie outside the box: the site set of a box is the
 *                volume's site set cut to the box and does not depend on where the box's faces fall;
 *   site(v):     surface(v); with TSDF_EDT_UNKNOWN surface(v) || !observed(v).
 * d2(v) = min(R * R, min over the sites s inside the box of |v - s|^2), R = max_dist; a box without
 * sites gives R * R everywhere. Only sites inside the box count, so a voxel at least R voxels from every
 * face of the box holds the volume's true saturated distance: a caller pads its region by R. d2 at a
 * free voxel is the clearance, at an inside voxel the penetration depth; state gives the sign.
 * Required: the box limits (TSDF_BOX_MAX_DIM, TSDF_BOX_MAX_VOXELS), every voxel of the box grown by one voxel
 * inside the int16 block range, max_dist in 1 .. 255, min_weight >= 0, sites one of the two values, d2
 * non-NULL; anything else is TSDF_ERR_INVALID_ARG with nothing written. The call completes a pending
 * pipelined frame first, runs asynchronously on the engine stream for device memory and copies and
 * synchronises for host memory, is not available on a shard engine (shard_count > 1:
 * TSDF_ERR_INVALID_ARG), only reads the volume and sets no status bits. Its scratch (about 3 bytes per
 * voxel, 6 for host outputs) belongs to the engine, grows on demand and is freed by tsdf_destroy. */
#define TSDF_EDT_SURFACE 1 /* sites: surface voxels */
#define TSDF_EDT_UNKNOWN 2 /* sites: also every unobserved voxel of the box */
typedef struct tsdf_edt_config {
  int32_t origin[3];  /* first voxel of the box, global voxel coordinates, x y z */
  int32_t dims[3];    /* nx, ny, nz voxels */
  int32_t max_dist;   /* R [voxels], 1 .. 255: distances saturate at R */
  int32_t min_weight; /* >= 0: a voxel is observed when its block exists and its fusion weight >= this */
  int32_t sites;      /* TSDF_EDT_SURFACE, or TSDF_EDT_SURFACE | TSDF_EDT_UNKNOWN */
} tsdf_edt_config;
typedef struct tsdf_edt_out {
  uint16_t* d2;   /* nz * ny * nx, x fastest: min(R * R, squared distance [voxels^2] to the nearest site) */
  uint8_t* state; /* same shape: 0 unobserved, 1 observed free (tsdf > 0), 2 observed inside (tsdf <= 0);
                     NULL: skipped */
  int mem_kind;   /* TSDF_MEM_HOST or TSDF_MEM_DEVICE, both pointers alike */
} tsdf_edt_out;
/* max_dist 255, min_weight 1, sites TSDF_EDT_SURFACE; origin and dims zero */
void tsdf_edt_config_default(tsdf_edt_config* cfg);
int tsdf_distance_field(tsdf_engine* e, const tsdf_edt_config* cfg, const tsdf_edt_out* out);

/* ---- Travel field over the box of a distance field: reachability and paths (no reference counterpart) ----
 * The least travel cost from a set of seed voxels to every voxel of a box through passable voxels, and the
 * paths back. The inputs are the d2 and state arrays tsdf_distance_field wrote (or any arrays of that
 * shape), not the volume. All integers, so the result is exact. For a voxel v of the box:
 *   passable(v): d2[v] >= clearance2 && (state[v] == 1 || (unknown_free && state[v] == 0));
 *                state 2 (inside a surface) is never passable.
 * A step goes from a passable voxel to a passable voxel among its 26 neighbours inside the box and costs
 * 2 + |dx| + |dy| + |dz|: 3 across a face, 4 across an edge, 5 across a corner (the <3, 4, 5> chamfer), so
 * cost / 3 is a length in voxels. There is no rule beyond the two end points of a step: a diagonal step may
 * pass between two surface voxels that touch at a corner; clearance2 >= 4 rules that out, since every
 * passable voxel is then two voxels or more from every surface voxel.
 * cost[v] is the least total over all such paths from any seed that lies inside the box and is passable: 0
 * at those seeds, TSDF_TRAVEL_UNREACHED wherever no path exists, impassable voxels included. Seeds outside
 * the box or impassable are ignored; *seeded is the number of seeds used, duplicates counted once per
 * entry. S == 0 or no usable seed gives a field of TSDF_TRAVEL_UNREACHED, TSDF_OK and *seeded = 0. The
 * field is the unique least fixed point of the relaxation, so it does not depend on scheduling. *rounds is
 * the number of relaxation rounds the call ran: implementation defined, reported for tests and
 * measurements. The largest possible cost is 5 * 2^28, below 2^32.
 * unknown_free = 1 is the optimistic planner: space no frame has observed is passable, observed surfaces
 * and their clearance margin are not. The volume only holds blocks near surfaces, so the open interior of a
 * room is state 0 and a field with unknown_free = 0 is confined to the thin observed-free shell around the
 * surfaces. With unknown_free = 1 an unobserved gap in a wall leaks: the field passes through it.
 * Required: e, cfg, d2, state and cost non-NULL, the box limits (TSDF_BOX_MAX_DIM, TSDF_BOX_MAX_VOXELS),
 * clearance2 in 0 .. 65025, unknown_free 0 or 1, mem_kind one of the two, S >= 0 and seeds non-NULL when
 * S > 0; anything else is TSDF_ERR_INVALID_ARG with nothing written. d2, state and cost are mem_kind memory
 * alike (host: the call copies up and down; device: it runs on the engine stream); seeds, seeded and rounds
 * are host memory. Either way the call has synchronised the engine stream when it returns: it reads a
 * convergence counter once per batch of rounds. Should the rounds pass their proven bound (voxels + 2) the
 * call returns TSDF_ERR_HIP instead of going on. The call does not touch the volume: the engine lends its
 * stream and scratch (grown on demand, freed by tsdf_destroy), it sets no status bits, pending frames stay
 * pending, and a shard engine (shard_count > 1) serves as well as any other.
 *
 * tsdf_travel_paths walks back from each target over such a field. v = target; while cost[v] != 0 take the
 * first direction k, in the order dz slowest, then dy, then dx, each running -1, 0, 1 with (0, 0, 0)
 * skipped, for which n = v + dir[k] lies in the box, cost[n] != TSDF_TRAVEL_UNREACHED and cost[n] + w[k] ==
 * cost[v] (no wrap-around: the sum is taken in 64 bits), and go on from n. A field written by
 * tsdf_travel_field always has such a neighbour; if none is found the walk ends there, len[t] is the
 * negated number of voxels so far, and the call still returns TSDF_OK. path[t * max_len + j] is the j-th
 * voxel of the walk as the linear index (z * ny + y) * nx + x, the target first and the seed last. len[t]
 * is the full number of voxels, both ends included; only the first max_len are written, so len[t] > max_len
 * (or len[t] < -max_len) tells the caller to ask again. len[t] = 0 for a target outside the box or
 * unreached. The costs along a walk strictly decrease, so it ends on any input. Host and device cost give
 * the same paths. Required: e, dims and cost non-NULL, dims as above, T >= 0, max_len >= 0,
 * T * max_len <= 2^28 (the longest walk there can be, for one target), and targets, len (and path when
 * max_len > 0) non-NULL when T > 0; anything else is TSDF_ERR_INVALID_ARG with nothing written. A device
 * field's call stages T * max_len indices in engine scratch, which stays until tsdf_destroy. targets, path and len are host memory; the call synchronises
 * the engine stream for a device field and does not use the GPU for a host field. */
#define TSDF_TRAVEL_UNREACHED 0xFFFFFFFFu
typedef struct tsdf_travel_config {
  int32_t dims[3];      /* nx, ny, nz of the box: the distance field's */
  int32_t clearance2;   /* 0 .. 65025 [voxels^2]: passable needs d2 >= clearance2 */
  int32_t unknown_free; /* 0: unobserved voxels (state 0) are obstacles; 1: passable like free ones */
} tsdf_travel_config;
/* clearance2 0, unknown_free 0; dims zero */
void tsdf_travel_config_default(tsdf_travel_config* cfg);
int tsdf_travel_field(tsdf_engine* e, const tsdf_travel_config* cfg, const uint16_t* d2,
                      const uint8_t* state /* nz * ny * nx, x fastest; mem_kind */,
                      const int32_t* seeds /* host, S x 3 box-local x y z */, int32_t S,
                      uint32_t* cost /* nz * ny * nx; mem_kind */, int mem_kind,
                      int32_t* seeded /* host, may be NULL */, int32_t* rounds /* host, may be NULL */);
int tsdf_travel_paths(tsdf_engine* e, const int32_t dims[3], const uint32_t* cost, int mem_kind /* cost */,
                      const int32_t* targets /* host, T x 3 box-local */, int32_t T, int32_t max_len,
                      int32_t* path /* host, T x max_len linear voxel indices */, int32_t* len /* host, T */);

/* ---- Observed free space: a bit per voxel of a box, set by depth frames (no reference counterpart) ----
 * The volume holds blocks near surfaces only, so the open interior of a room is state 0 (unobserved) in every
 * distance field. Every depth frame carries the evidence that the space its rays crossed is empty; these calls
 * keep it, whether or not a voxel's block exists, and promote a distance field's state with it, so that
 * tsdf_travel_field(..., unknown_free = 0) floods exactly the space that was observed empty and a gap in a
 * wall nobody looked through does not leak.
 *
 * The test is the voxel update's own geometry with one more condition. For the voxel g = (gx, gy, gz) in
 * global voxel coordinates and a frame (depth W x H, K, cam_T_world, max_depth), with the engine's
 * voxel_size and truncation:
 *   pw = (float)g * voxel;  pc = cam_T_world * pw        (Eigen's order: SE3::Apply over _transformVector)
 *   hx = fx pc.x + cx pc.z;  hy = fy pc.y + cy pc.z;  hz = pc.z
 *   u = f2i(roundf(hx / hz));  v = f2i(roundf(hy / hz))  (half away from zero; the conversion truncates,
 *                                                         saturates and turns NaN into 0)
 *   in image: 0 <= u < W and 0 <= v < H;  d = depth[v W + u];  valid: d != 0 and d <= max_depth
 *   range = |Kinv (u, v, 1)|: x = (1 / fx) u + (-cx (1 / fx)) 1, y likewise, sqrt(x x + (y y + 1 1))
 *   sdf = range (d - hz)
 *   free(g, frame) = in image && valid && sdf >= truncation && hz > 0
 * all in float32, one IEEE operation at a time with no contraction: the same operations in the same order
 * as the update. sdf >= truncation is the update's fminf(1, sdf / truncation) == 1: had the voxel's block
 * existed and been empty, this frame would have written tsdf exactly 1 into it. hz > 0 is new and
 * deliberate: the update also touches voxels behind the camera plane whose quotient happens to land in the
 * image, and a safety layer must not call those observed. A NaN sdf fails >=, so it is not free. The camera
 * centre has hz = 0 and is never marked: a caller seeds a travel field at a voxel in front of the camera.
 *
 * A layer is the caller's: a box (origin and dims in global voxels) and uint32_t bits[nz * ny * wx] with
 * wx = ceil(nx / 32). Voxel (x, y, z) of the box is bit x & 31 of word (z * ny + y) * wx + (x >> 5). The
 * library never sets the padding bits of a row's last word. A cleared layer is all zeros.
 * tsdf_free_words: the number of words, nz * ny * ceil(nx / 32); 0 for invalid dims.
 * tsdf_free_observe: bits |= free(., frame) over the box. Idempotent and monotone: bits are only ever set,
 * and a frame observed twice changes nothing. It does not depend on TSDF_FREE_CULL (an A/B and test knob
 * read at tsdf_create: 0 disables the two exact culls of the kernel).
 * tsdf_free_apply: state[v] = 1 wherever state[v] == 0, v lies inside the layer's box and its bit is set,
 * for every voxel v of the state array's box (origin, dims; nz * ny * nx bytes, x fastest: a distance
 * field's). States 1 and 2, and voxels outside the layer's box, stay as they are: an inside voxel is never
 * promoted. The two boxes may overlap partly, nest or be disjoint. *promoted is the number of voxels changed.
 * Required, of the layer's box and of apply's state box alike: the box limits (TSDF_BOX_MAX_DIM,
 * TSDF_BOX_MAX_VOXELS), every voxel in a block of the int16 block range (origin >> 3 >= -32768,
 * (origin + dims - 1) >> 3 <= 32767); width / height in 1 .. the engine's max_width / max_height;
 * max_depth > 0; mem_kind one of the
 * two; every pointer non-NULL except promoted. Anything else is TSDF_ERR_INVALID_ARG with nothing written.
 * Neither call touches the volume: the engine lends its stream and scratch (grown on demand, freed by
 * tsdf_destroy), no status bits are set, pending pipelined frames stay pending -- the natural use is one
 * observe per integrated frame -- and a shard engine (shard_count > 1) serves as well as any other.
 * Device memory (bits and depth, or bits and state, alike): observe is asynchronous on the engine stream,
 * and its inputs must stay valid until the next engine call or tsdf_synchronize; apply is asynchronous when
 * promoted is NULL, else it synchronises the engine stream once. Host memory: the call copies up, runs,
 * copies down and synchronises. K, cam_T_world, box, origin, dims and promoted are host memory. */
typedef struct tsdf_free_box {
  int32_t origin[3]; /* global voxel coordinates of the box's first voxel */
  int32_t dims[3];   /* nx, ny, nz */
} tsdf_free_box;
int64_t tsdf_free_words(const int32_t dims[3]);
int tsdf_free_observe(tsdf_engine* e, const tsdf_free_box* box, uint32_t* bits, const float* depth, int width,
                      int height, int mem_kind /* bits and depth alike */, const tsdf_intrinsics* K,
                      const tsdf_pose* cam_T_world, float max_depth);
int tsdf_free_apply(tsdf_engine* e, const tsdf_free_box* box, const uint32_t* bits, const int32_t origin[3],
                    const int32_t dims[3], uint8_t* state, int mem_kind /* bits and state alike */,
                    int64_t* promoted /* host, may be NULL */);

/* ---- Frontiers and connected components over a box (no reference counterpart) ----
 * Where the map ends, as a short list of places to look from. A frontier is an observed-free, reachable voxel
 * that touches unobserved space; tsdf_components clusters any voxel mask into its 26-connected components and
 * reports each one's size, place and cheapest member. All integers, so the results are exact. Boxes as
 * everywhere: dims = (nx, ny, nz) within the box limits (TSDF_BOX_MAX_DIM, TSDF_BOX_MAX_VOXELS), arrays
 * nz * ny * nx with x fastest,
 * linear index (z * ny + y) * nx + x.
 *
 * tsdf_frontier_mark: mask[v] = 1 when all three hold, else 0:
 *   state[v] == 1;  cost == NULL or cost[v] != TSDF_TRAVEL_UNREACHED;
 *   at least one of the six face neighbours of v inside the box has state 0.
 * Neighbours outside the box never count, as the travel field's steps do not: a box that is all state 1 has no
 * frontier. *marked is the number of ones. state is a distance field's state and cost a travel field's cost
 * over the same box. The distance field should use surface sites only (TSDF_EDT_SURFACE): with
 * TSDF_EDT_UNKNOWN sites every passable voxel keeps its clearance from unobserved space, so no voxel next to
 * unobserved space is reached and no frontier is marked. state should have been promoted by tsdf_free_apply:
 * otherwise the whole outer skin of the thin observed shell around the surfaces is "frontier".
 * state, cost and mask are mem_kind memory alike. Device memory: asynchronous on the engine stream when marked
 * is NULL, one synchronisation otherwise (tsdf_free_apply's rule). Host memory: the call copies up, runs,
 * copies down and synchronises. Required: e, dims, state and mask non-NULL, dims as above, mem_kind one of the
 * two; anything else is TSDF_ERR_INVALID_ARG with nothing written.
 *
 * tsdf_components: members are the voxels with mask[v] != 0. Two members are adjacent when they are among
 * each other's 26 neighbours inside the box (the travel field's steps); components are the classes of the
 * transitive closure. label[v] is the least linear index among the members of v's component, and
 * TSDF_COMPONENT_NONE for a voxel off the mask. The labelling is therefore unique: it does not depend on
 * scheduling or on the order of any atomic. *total is the number of components, *count the number with
 * size >= min_size, and clusters[0 .. *count) are those, in ascending label. goal is the member with the least
 * key[v], ties to the least linear index, and goal_key its key -- with key a travel field's cost, the
 * component's cheapest voxel to travel to, goal_key / 3 voxels away; key == NULL gives goal = label and
 * goal_key = 0. lo, hi and sum are in box-local voxel coordinates; sum / size is the centroid.
 * capacity == 0 (clusters may then be NULL) is the query form: labels and counts are written and the call
 * returns TSDF_OK. *count > capacity > 0 writes labels and counts, nothing to clusters, and returns
 * TSDF_ERR_CAPACITY. label is written in full on every accepted call. Required: e, cfg, mask, label and count
 * non-NULL, dims as above, min_size >= 1, capacity >= 0, clusters non-NULL when capacity > 0, mem_kind one of
 * the two; anything else is TSDF_ERR_INVALID_ARG with nothing written. mask, key and label are mem_kind
 * memory alike; cfg, clusters, count and total are host memory. The call has synchronised the engine stream
 * when it returns.
 * Both calls leave the volume alone: the engine lends its stream and scratch (grown on demand, freed by
 * tsdf_destroy: 4 bytes per voxel plus 576 per component for tsdf_components, 9 more per voxel for host
 * arrays), no status bits are set, pending pipelined frames stay pending, and a shard engine
 * (shard_count > 1) serves as well as any other. */
#define TSDF_COMPONENT_NONE 0xFFFFFFFFu
typedef struct tsdf_components_config {
  int32_t dims[3];  /* nx, ny, nz of the box */
  int32_t min_size; /* >= 1: clusters lists the components with at least this many voxels */
} tsdf_components_config;
typedef struct tsdf_component {
  uint32_t label;    /* least linear index of the component */
  uint32_t size;     /* voxels */
  int32_t lo[3];     /* box-local bounding box, x y z, inclusive */
  int32_t hi[3];
  int64_t sum[3];    /* sums of the members' box-local x, y, z: centroid = sum / size */
  uint32_t goal;     /* linear index of the member with the least key[v], ties to the least index; label when
                        key is NULL */
  uint32_t goal_key; /* key[goal]; 0 when key is NULL */
} tsdf_component;
/* min_size 1; dims zero */
void tsdf_components_config_default(tsdf_components_config* cfg);
int tsdf_frontier_mark(tsdf_engine* e, const int32_t dims[3], const uint8_t* state,
                       const uint32_t* cost /* may be NULL */, uint8_t* mask, int mem_kind /* all three alike */,
                       int64_t* marked /* host, may be NULL */);
int tsdf_components(tsdf_engine* e, const tsdf_components_config* cfg, const uint8_t* mask,
                    const uint32_t* key /* may be NULL */, uint32_t* label, int mem_kind /* all three alike */,
                    tsdf_component* clusters /* host */, int32_t capacity, int32_t* count /* host */,
                    int32_t* total /* host, may be NULL */);

/* ---- View gain: the unobserved voxels a candidate camera pose would observe (no reference counterpart) ----
 * Frontier clusters say where to look from; this says what a pose there would show. For V candidate poses over
 * the box of a distance field's state array, tsdf_view_gain predicts each pose's depth image from the state
 * and counts the unobserved voxels (state 0) that image would mark free by tsdf_free_observe's own test. All
 * integers and single float32 operations, one IEEE operation at a time with no contraction: the results are
 * exact, and do not depend on scheduling, batching or TSDF_VIEW_SKIP (an A/B and test knob read at
 * tsdf_create: 0 selects the plain march and disables the per-view brick cull).
 *
 * Predicted depth of view i (cam_T_world = views[i]) at pixel (u, v):
 *   dc = (ifx u + icx 1, ify v + icy 1, 1) with ifx = 1 / fx, icx = -cx ifx (y likewise): the free test's ray
 *   range = sqrt(dc.x dc.x + (dc.y dc.y + 1 1))
 *   world_T_cam = SE3::Inverse of cam_T_world in host float order (n2 = (qx qx + qz qz) + (qy qy + qw qw),
 *                 q' = (-qx, -qy, -qz, qw) / n2 or zero when n2 is not positive, t' = q' * (-t))
 *   J = f2i(far / step), required in 1 .. 65536
 *   for j = 1 .. J:  z_j = (float)j * step;  pc_j = (dc.x z_j, dc.y z_j, z_j);  pw_j = world_T_cam * pc_j;
 *                    g_j = round(pw_j / voxel_size) per component, half away from zero, saturating, NaN -> 0
 *   pred[i][v W + u] = z_j of the first j with g_j inside the box and state[g_j] == 2, else miss_depth.
 * Every sample is a product and a transform of j, never a running sum. A sample outside the box is
 * transparent (the camera may stand outside the box), and so are states 0 and 1 and every byte other than 2.
 * depth_out, when non-NULL, receives pred (V x H x W).
 *
 * Gain: vis(g, i) is tsdf_free_observe's free(g, frame) with depth = pred[i], valid reduced to d != 0 (no
 * max_depth test: (float)J * step may round above far) and truncation replaced by margin; the projection, the
 * rounding, sdf = range (d - hz) >= margin and hz > 0 stay.
 *   gain[i] = #{ g in the box : state[g] == 0 && !seen(g) && vis(g, i) }
 * seen is a free layer over the same box (tsdf_free_words layout; NULL: none; padding bits are ignored): the
 * voxels that views already chosen will observe. To commit view i a caller ORs it in with
 * tsdf_free_observe(seen, depth_out + i W H, ...): with margin == truncation and max_depth >= 2 far the new
 * bits on state-0 voxels then number exactly gain[i].
 * Required: the box limits (TSDF_BOX_MAX_DIM, TSDF_BOX_MAX_VOXELS), the box inside the int16 block range;
 * width / height in
 * 1 .. the engine's max_width / max_height; V in 0 .. 4096 and V W H <= 2^26; far > 0, step > 0, margin >= 0,
 * miss_depth 0 or in (0, far], all finite; mem_kind one of the two; e, cfg and state non-NULL, views and gain
 * non-NULL when V > 0. Anything else is TSDF_ERR_INVALID_ARG with nothing written. V == 0 returns TSDF_OK.
 * state, seen and depth_out are mem_kind memory alike; cfg, views and gain are host memory. With host arrays
 * the call copies up and down; either way it has synchronised the engine stream once when it returns.
 * Views are taken TSDF_VIEW_BATCH at a time, fewer while a batch's W H pixels exceed TSDF_VIEW_BATCH_PIXELS
 * (at least one): the scratch holds 8 bytes per pixel of a batch, 72 bytes per view and, for host arrays,
 * their staging. A cam_T_world that is no rotation (|n2 - 1| > 2^-10) goes without the brick cull and gives
 * the same result. The call never touches the volume: the engine lends its stream and scratch (grown on
 * demand, freed by tsdf_destroy), no status bits are set, pending pipelined frames stay pending, and a shard
 * engine (shard_count > 1) serves as well as any other. */
#define TSDF_VIEW_BATCH 64
#define TSDF_VIEW_BATCH_PIXELS (1 << 22)
typedef struct tsdf_view_config {
  int32_t origin[3];   /* the box of `state` (and of `seen`), global voxels */
  int32_t dims[3];     /* nx, ny, nz */
  int32_t width, height;
  tsdf_intrinsics K;   /* of every candidate view */
  float far;           /* > 0 [m]: how deep a ray is marched */
  float step;          /* > 0 [m]: sample spacing along the optical axis */
  float margin;        /* >= 0 [m]: a voxel counts when range * (d - hz) >= margin; the engine's
                          truncation gives tsdf_free_observe's own test */
  float miss_depth;    /* depth of a ray that meets no surface: 0 (no return, nothing seen along it) or
                          in (0, far] (the optimistic sensor: free out to there) */
} tsdf_view_config;
/* far 3, step = voxel_size, margin = truncation, miss_depth = far; origin, dims, width, height and K zero */
void tsdf_view_config_default(const tsdf_engine* e, tsdf_view_config* cfg);
int tsdf_view_gain(tsdf_engine* e, const tsdf_view_config* cfg, const uint8_t* state,
                   const uint32_t* seen /* may be NULL */, const tsdf_pose* views /* host, V cam_T_world */,
                   int32_t V, int64_t* gain /* host, V */, float* depth_out /* V*H*W, may be NULL */,
                   int mem_kind /* state, seen and depth_out alike */);

int tsdf_get_stats(tsdf_engine* e, tsdf_stats* out, int clear_status);
int tsdf_synchronize(tsdf_engine* e);
/* mode TSDF_PROFILE_PHASES: HIP events between all four phases of an integrate call;
 * TSDF_PROFILE_INTEGRATE: only the two events bracketing the fused update kernel (the other
 * phase times read 0). Events are recorded on every `every`-th integrate call (1 = all): each
 * event is a queue marker that costs the stream ~3 us, so a timed loop samples. */
#define TSDF_PROFILE_PHASES 0
#define TSDF_PROFILE_INTEGRATE 1
/* TSDF_PROFILE_KERNEL: ms_integrate from two events bound to the k_integrate dispatch itself
 * (hipExtLaunchKernel start/stop events = the kernel's begin/end timestamps, as a kernel trace
 * reports them); adds nothing to the stream, so `every` = 1 times every launch. */
#define TSDF_PROFILE_KERNEL 2
int tsdf_profile_begin(tsdf_engine* e, int mode, int every);
int tsdf_profile_end(tsdf_engine* e, tsdf_profile* out);

/* Snapshot / restore of the whole volume between frames (checkpoint / resume): hash table,
 * occupancy, free-block stack, voxel pool and counters, so a restored engine continues a frame
 * stream bit for bit. Two-call: tsdf_snapshot_bytes, then tsdf_snapshot_save into a host buffer of
 * that size. tsdf_snapshot_load accepts only a snapshot of an engine with the same voxel size,
 * truncation, pool size and shard layout whose counters, free stack and entries are consistent
 * (every pool index in range, each block exactly once on the stack or in the table);
 * TSDF_ERR_INVALID_ARG otherwise, the engine unchanged. */
int tsdf_snapshot_bytes(tsdf_engine* e, int64_t* bytes);
int tsdf_snapshot_save(tsdf_engine* e, void* out, int64_t capacity);
int tsdf_snapshot_load(tsdf_engine* e, const void* in, int64_t size);

/* Test-only full state dump (Query exposes only tsdf): the 2^22-entry hash table as
 * (x, y, z, offset) int16 quadruples + pool idx int32, the free-block heap, the free counter and
 * the SoA voxel pools (tsdf f32, prob f32, rgbw u8x4 per voxel, pool-index major). Host buffers;
 * any NULL pointer is skipped. */
int tsdf_debug_dump(tsdf_engine* e, int16_t* entry_pos_off, int32_t* entry_idx, int32_t* heap,
                    int32_t* free_count, float* tsdf, float* prob, uint8_t* rgbw);
/* Diagnostic builds only (make DIAG=1): per-workgroup 100 MHz phase stamps of the last launch of
 * each frame kernel, [8 kernels][4096 workgroups][8 stamps] u64, cleared after the copy. *enabled
 * reports whether the library was built with stamps. out == NULL only queries enabled. */
int tsdf_debug_stamps(tsdf_engine* e, uint64_t* out, int64_t capacity, int* enabled);
int32_t tsdf_num_entries(void);
int32_t tsdf_num_blocks(const tsdf_engine* e);

/* ---- VoxelHashTable / VoxelMemPool level (voxel_hash.cu, voxel_mem.cu), host arrays ---- */
/* One launch of VoxelHashTable::Allocate over keys (xyz int16 triples) + ResetLocks. Keys are
 * linearised in list order. */
int tsdf_hash_allocate(tsdf_engine* e, const int16_t* keys, int n);
/* One launch of VoxelHashTable::Delete over keys in list order + ResetLocks. */
int tsdf_hash_delete(tsdf_engine* e, const int16_t* keys, int n);
/* VoxelHashTable::Retrieve (voxel_hash.cuh:104-161) of voxel points: rgbw, tsdf, prob (defaults
 * 0 / 1 / 0 when missing) and the block meta (x, y, z, offset; idx -1 if missing). */
int tsdf_hash_retrieve(tsdf_engine* e, const int16_t* points, int n, uint8_t* rgbw, float* tsdf,
                       float* prob, int16_t* block_pos_off, int32_t* block_idx);
/* RetrieveMutable + store of rgbw (voxel_hash_test.cu:47-54); *missing = points not found. */
int tsdf_hash_assign(tsdf_engine* e, const int16_t* points, int n, const uint8_t* rgbw,
                     int* missing);
int tsdf_num_active_blocks(tsdf_engine* e, int32_t* out);
/* VoxelMemPool::AquireBlock / ReleaseBlock, n sequential calls (voxel_mem.cu:37-61). */
int tsdf_pool_acquire(tsdf_engine* e, int n, int32_t* idx_out);
int tsdf_pool_release(tsdf_engine* e, const int32_t* idx, int n);
int tsdf_pool_set_weight(tsdf_engine* e, int32_t block, uint8_t weight);
int tsdf_pool_get_weights(tsdf_engine* e, int32_t block, uint8_t* out512);

/* Hash of a block coordinate (voxel_hash.cu:31-35) and the shard owner of a block. */
uint32_t tsdf_hash_block(int16_t x, int16_t y, int16_t z);
int32_t tsdf_block_owner(int16_t x, int16_t y, int16_t z, int32_t shard_count);

const char* tsdf_error_string(int code);
const char* tsdf_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DISINFECT_TSDF_H */
