// tsdf_host.h -- what the engine's host files (tsdf_engine.hip, tsdf_host_*.hip) share: the engine
// struct, the error plumbing, the owner of device scratch and the helpers that cross files. Private to
// those files: the kernel files and tsdf_group.hip do not include it (tsdf_internal.h is the group's
// interface), and nothing declared here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <deque>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "disinfect_tsdf.h"
#include "tsdf_box.h"
#include "tsdf_internal.h"
#include "tsdf_kernels.h"
#include "tsdf_resolve.h"

using namespace tsdf;

#pragma GCC visibility push(hidden)

// ---- error plumbing: the message tsdf_last_error returns (thread-local, tsdf_engine.hip) ----
void set_error(const char* what, hipError_t e);
void set_error(const char* what);

#define HIP_OK(expr)                  \
  do {                                \
    hipError_t _e = (expr);           \
    if (_e != hipSuccess) {           \
      set_error(#expr, _e);           \
      return TSDF_ERR_HIP;            \
    }                                 \
  } while (0)

#define LAUNCH_OK(what)                        \
  do {                                         \
    hipError_t _e = hipGetLastError();         \
    if (_e != hipSuccess) {                    \
      set_error(what, _e);                     \
      return TSDF_ERR_HIP;                     \
    }                                          \
  } while (0)

// ---- host float math: same expressions (and -ffp-contract=off) as tsdf_device.h / the oracle ----
inline f3 h_cross(f3 a, f3 b) {
  f3 r;
  r.x = a.y * b.z - a.z * b.y;
  r.y = a.z * b.x - a.x * b.z;
  r.z = a.x * b.y - a.y * b.x;
  return r;
}
inline f3 h_qrot(quatf q, f3 v) {
  const f3 qv = {q.x, q.y, q.z};
  f3 uv = h_cross(qv, v);
  uv.x += uv.x;
  uv.y += uv.y;
  uv.z += uv.z;
  const f3 c = h_cross(qv, uv);
  f3 r;
  r.x = (v.x + q.w * uv.x) + c.x;
  r.y = (v.y + q.w * uv.y) + c.y;
  r.z = (v.z + q.w * uv.z) + c.z;
  return r;
}
inline int16_t h_f2s(float f) {
  if (f != f) return 0;
  if (f >= 32767.0f) return 32767;
  if (f <= -32768.0f) return -32768;
  return (int16_t)f;
}
// tsdf_box.h stands alone: its constants are the public header's and the kernels'
static_assert(kBoxMaxDim == TSDF_BOX_MAX_DIM && kBoxMaxVoxels == TSDF_BOX_MAX_VOXELS, "the public box limits");
static_assert(kBoxBlockBits == kBlockLenBits, "box_in_block_range's block");
// the limits as every box call's error text states them
#define TSDF_STR_(x) #x
#define TSDF_STR(x) TSDF_STR_(x)
#define BOX_LIMITS_TEXT "dims 1.." TSDF_STR(TSDF_BOX_MAX_DIM) ", at most 2^28 voxels"
static_assert(TSDF_BOX_MAX_VOXELS == (int64_t)1 << 28, "BOX_LIMITS_TEXT");

template <typename T>
hipError_t dmalloc(T** p, size_t count) {
  return hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(count, 1) * sizeof(T));
}

// The owner of one device buffer: engine scratch (freed with the engine) or a call's temporary (freed
// when it leaves scope -- after the synchronisation the call ends with). Grow-only; `cap` counts
// elements. Converts to its pointer, so launches and copies take it as they took the raw pointer.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // room for n elements. Nothing happens when it is there; otherwise the old buffer goes first, and
  // a failed allocation leaves the buffer empty (TSDF_ERR_HIP, `what` in the message).
  int ensure(size_t n, const char* what) {
    if (n <= cap) return TSDF_OK;
    release();
    const hipError_t err = dmalloc(&p, n);
    if (err != hipSuccess) {
      p = nullptr;
      set_error(what, err);
      return TSDF_ERR_HIP;
    }
    cap = n;
    return TSDF_OK;
  }
};
// Buffers that grow together: the caller checks the capacity of the one it allocates last (set only
// once every earlier allocation succeeded), frees them all with this, then calls ensure on each.
template <typename... B>
void release_all(B&... b) {
  (b.release(), ...);
}

// Host-or-device staging of a box call's arrays over its Sections (DESIGN.md "Box calls"). A device call hands
// the kernels the caller's pointers; a host call stages each array in a section of the scratch buffer, uploads
// inputs before and downloads outputs after. A null optional array takes no room and yields null either way.
// The helpers enqueue only the copy they name, where they are called: the order of a call's copies, memsets
// and launches, and its one synchronisation, stay the call's own.
inline size_t staged(bool host, const void* p, size_t bytes) { return host && p ? bytes : 0; }
struct Stage {
  const Sections& L;
  void* base;
  bool host;
  hipStream_t s;
  // the device pointer of an output array (or of an input whose upload is not due yet)
  template <typename T>
  T* ptr(int h, T* p) const {
    return !p ? nullptr : host ? L.at<T>(base, h) : p;
  }
  // the device pointer of an input array in *dev, its upload enqueued for a host call
  template <typename T, typename U>
  hipError_t in(int h, T* p, size_t bytes, U** dev) const {
    *dev = ptr(h, p);
    return host && p ? hipMemcpyAsync(L.at<void>(base, h), p, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
  }
  // the download of an output array from the pointer ptr / in gave, for a host call
  hipError_t back(void* p, const void* dev, size_t bytes) const {
    return host && p ? hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
  }
};

// roctx ranges around the C-ABI calls (SURVEY.md 5 tracing): host-side enqueue intervals that
// `rocprofv3 --marker-trace` lines up with the kernels they launch. Off unless TSDF_ROCTX=1.
inline bool roctx_on() {
  static const bool on = [] {
    const char* v = std::getenv("TSDF_ROCTX");
    return v && v[0] == '1';
  }();
  return on;
}
struct TraceRange {
  const bool on;
  explicit TraceRange(const char* name) : on(roctx_on()) {
    if (on) roctxRangePushA(name);
  }
  ~TraceRange() {
    if (on) roctxRangePop();
  }
};

// the environment's A/B and test knobs (the table of variables: read_env_knobs, tsdf_engine.hip)
struct EnvKnobs {
  bool pipeline = true;
  bool free_cull = true;  // (beside `pipeline`, in its padding: the struct keeps its size)
  bool view_skip = true;  // (likewise)
  int64_t pipe_max_pixels = -1;
  int frame_order = -1, frame_upd_wgs = 0, cand_cap = 0, mesh_grid = 0;
};

struct tsdf_graph;  // tsdf_host_graph.hip

struct tsdf_engine {
  tsdf_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // a deferred raycast (tsdf_raycast_deferred): its view grid is built; the k_raycast launch waits
  // for the engine's next call -- fused with the next frame's ingest (k_render_ingest) when that call
  // is tsdf_integrate, alone otherwise (join_render)
  struct DeferredRender {
    bool pending = false;
    FrameParams P{};
    ViewGrid V{};
    float step = 0.f;
    uchar4* rgba = nullptr;
    uchar4* normal = nullptr;
  } rd;
  // the deferred raycast of a render-deferring graph frame (tsdf_graph_create_deferred): its args slot
  // (camera, view grid, outputs) on the device; taken up by the graph's next frame (k_render_ingest_g),
  // launched alone (k_raycast_g) by any other call
  struct DeferredGraphRender {
    bool pending = false;
    const tsdf_graph* g = nullptr;
    const FrameArgs* args = nullptr;
    int W = 0, H = 0;
  } rdg;
  // a batched graph (tsdf_graph_create_batch) whose current batch holds frames not launched yet:
  // every other call launches them first (join_render -> graph_flush_batch)
  struct tsdf_graph* gbatch = nullptr;
  EngineDev D{};
  int maxs = 3;
  int64_t order_range = 0;  // candidate order space: max_pixels * maxs
  int64_t max_pixels = 0;
  // host-frame staging
  // host frames (TSDF_MEM_HOST, voxel_tsdf.cu:358-365): two staging slots filled on the upload stream
  // (a copy engine) while the engine stream runs the previous frames; slot k at offset k * max_pixels
  DevBuf<uint8_t> s_rgb;
  DevBuf<float> s_depth, s_ht, s_lt;
  // upload streams: a frame's copies spread over them (several DMA engines share the host link)
  static constexpr int kUpStreams = 2;
  hipStream_t ustream[kUpStreams] = {};
  hipEvent_t up_done[2][kUpStreams] = {};  // slot k's copies on stream j complete (the engine stream waits)
  int up_nstreams = 0;                     // streams the pending upload used
  hipEvent_t up_free[2] = {nullptr, nullptr};  // slot k's last reader launched before this (the upload waits)
  bool up_used[2] = {false, false};       // up_free[k] has been recorded
  int up_next = 0;                        // the slot of the next host frame
  int up_pending = -1;                    // the slot of a frame whose reading launch is not enqueued yet
  // raycast / query / test scratch
  DevBuf<uchar4> rc_rgba, rc_norm;
  // raycast view grid (tsdf_kernels.h ViewGrid): cells, the two brick bitmaps, generation
  DevBuf<uint32_t> vg_cell;
  DevBuf<uint8_t> vg_flags;
  DevBuf<uint32_t> vg_bits;
  uint32_t vg_gen = 0;
  uint64_t vg_calls = 0;
  DevBuf<VisRec> q_sel;
  DevBuf<int32_t> q_count;
  DevBuf<float4> q_out;  // voxels
  // grouped selections (render bands / halo destinations): per group a bitmap, its per-workgroup
  // counts, the emitted list and its count (g_count.cap groups)
  DevBuf<unsigned long long> g_visbits;
  DevBuf<int32_t> g_wgcnt;
  DevBuf<VisRec> g_sel;
  DevBuf<int32_t> g_count;
  // mesh extraction scratch
  DevBuf<int32_t> m_counts, m_offsets;
  DevBuf<int64_t> m_total;
  DevBuf<int32_t> m_nbr;        // k_mesh: 27 neighbour pool indices per selected block
  int mesh_grid = 0;            // k_mesh workgroups: min(kMeshGrid, pool blocks)
  DevBuf<float> m_out;          // 9 floats per triangle
  // indexed mesh scratch (tsdf_extract_mesh_indexed): allocated by its first call, grow-only
  DevBuf<unsigned long long> mi_emask;  // the edge records: mi_cap() selected blocks x kEdgeWords
  DevBuf<uint16_t> mi_epre;             // x kEdgePre
  int32_t mi_cap() const { return (int32_t)(mi_epre.cap / kEdgePre); }
  DevBuf<int32_t> mi_vcounts, mi_voffsets;  // pool blocks (k_scan_counts runs over every selected block)
  DevBuf<int64_t> mi_vtotal;
  DevBuf<int32_t> mi_selmap;            // pool blocks
  DevBuf<uint8_t> mi_out;               // staging of a host output
  // pose tracking (tsdf_raycast_surface / tsdf_icp_linearize / tsdf_track): allocated on first use, grow-only
  DevBuf<float> tk_point, tk_normal;  // tsdf_track's model maps, 3 floats per pixel
  DevBuf<float> tk_pnormal;           // the normals its linearisations use (k_surface_normals)
  DevBuf<uint8_t> tk_stage;           // host maps / frames staged on the device
  DevBuf<double> tk_part;  // k_icp_partial's per-workgroup sums, then the 29 totals (its last kIcpSums)
  // UV dose (tsdf_uv_dose): the emitters on the device, then 6 box words and one flag per emitter
  // (k_dose_bounds); uv_h the pinned copy they are uploaded from / read back to, free again once uv_ev
  // has passed. Grow-only.
  DevBuf<uint8_t> uv_dev;
  uint8_t* uv_h = nullptr;
  int32_t uv_cap = 0;  // emitters
  hipEvent_t uv_ev = nullptr;
  bool uv_busy = false;
  // lamp-stop planning (tsdf_uv_irradiance / tsdf_uv_plan; tsdf_host_plan.hip), grow-only. pl_dev: an
  // irradiance call's emitters, candidate offsets, 8 box words and one flag per emitter, or a plan's
  // PlanState, gains and stops; pl_h (pl_cap bytes) the pinned copy they are uploaded from / read back to,
  // free again once pl_ev has passed. pl_part: k_plan_gain's sums. pl_stage: a plan's host arrays staged
  // on the device.
  DevBuf<uint8_t> pl_dev;
  uint8_t* pl_h = nullptr;
  size_t pl_cap = 0;
  hipEvent_t pl_ev = nullptr;
  bool pl_busy = false;
  DevBuf<double> pl_part;
  DevBuf<uint8_t> pl_stage;
  // hash-level test scratch (tsdf_hash_* / tsdf_pool_*): t_s4.cap points
  DevBuf<int16_t> t_keys;
  DevBuf<VisRec> t_recs;
  DevBuf<int32_t> t_count, t_i32;
  DevBuf<uint32_t> t_u32;
  DevBuf<float> t_f0, t_f1;
  DevBuf<short4> t_s4;
  DevCounters* h_ctr = nullptr;  // pinned readback
  // profiling
  bool profiling = false;
  int prof_mode = TSDF_PROFILE_PHASES;
  int prof_every = 1;        // event-time every n-th integrate call
  int64_t prof_calls = 0;    // integrate calls since profile_begin
  int64_t prof_pipelined = 0;  // update launches with the next frame's pixel tiles since profile_begin
  // a deque: a deferred frame (pipelined, sharded) keeps a pointer to its events across later calls
  std::deque<std::array<hipEvent_t, 5>> events;
  size_t ev_used = 0;
  unsigned long long prof_vis0 = 0, prof_upd0 = 0, prof_ticks0 = 0, prof_ing0 = 0, prof_ra0 = 0, prof_rd0 = 0;
  // sharded frame (tsdf_integrate_shard_*): 0 idle, 1 after _begin, 2 after _update
  hipEvent_t order_ev = nullptr;  // tsdf_stream_wait / _signal
  int shard_phase = 0;
  bool shard_keys_packed = false;  // _begin wrote a key slot (split DDA): _update merges an inbox
  FrameParams shard_P{};
  std::array<hipEvent_t, 5>* shard_ev = nullptr;
  // pipelined frames (tsdf_integrate on one volume, k_frame): what the next launch
  // continues. kPipeNone: nothing pending. kPipeU: frame p_fid's ingest and allocation ran
  // (k_ingest_dda), its update is pending. kPipeCAU: frame p_carve's carving and frame p_fid's
  // allocation and update are pending (p_fid's tiles probed and inserted its keys, its sweep listed
  // its blocks). Every other entry point first completes them (flush_pending).
  bool pipeline = true;
  int64_t pipe_max_pixels = (int64_t)1 << 20;  // larger frames take two launches (pipe_frame_size)
  static constexpr int kPipeNone = 0, kPipeU = 1, kPipeCAU = 2, kPipeAU = 3, kPipeC = 4;  // kPipeAU:
  // p_fid's allocation and update are pending with no carving (after a graph frame that started a
  // stream); kPipeC: only p_fid's carving is pending (a shard's pipelined frames, between flush steps)
  int ps = kPipeNone;
  uint32_t fid_next = 1;  // engine-wide frame ids (views, tags; never 0)
  uint32_t p_carve = 0, p_fid = 0;
  FrameParams p_P{};      // frame p_fid's camera / frame / pixel-record buffer
  bool p_sampled = false;  // kPipeU: the frame was sampled for profiling (its update, when flushed
                           //   as k_integrate, takes an event pair then)
  uint32_t pipe_tag = 0;  // one per k_frame launch: its flags' value
  int frame_order = 2;    // PipeArgs.order (TSDF_FRAME_ORDER, 0..2): sweep, update, tiles (measured best)
  EnvKnobs env;           // the environment's A/B and test knobs, read once at tsdf_create
  // feed_rgbd_frame staging: raw full-size inputs (host frames) and the half-size outputs
  // (fe_mask.cap / fe_out_depth.cap pixels)
  DevBuf<uint8_t> fe_rgb;
  DevBuf<uint16_t> fe_depth;
  DevBuf<uint8_t> fe_mask;
  DevBuf<uint8_t> fe_out_rgb;
  DevBuf<float> fe_out_depth;
  // distance field (tsdf_distance_field): the site bitmap, the x pass's bytes, the y pass's u16 and, for
  // host outputs, their staging, one section each (tsdf_host_edt.hip). Grow-only.
  DevBuf<uint8_t> edt_buf;
  // travel field (tsdf_travel_field / tsdf_travel_paths; tsdf_host_travel.hip): the round control words, the
  // tiles' wake-up stamps, the two tile lists, the seeds and, for host arrays, their staging, one section
  // each; or a paths call's targets, lengths and paths. Grow-only. (Last: the frame path's fields keep
  // their offsets.)
  DevBuf<uint8_t> tv_buf;
  // observed free space (tsdf_free_observe / tsdf_free_apply; tsdf_host_free.hip): a frame's pixel records
  // or an apply's counter, then, for host arrays, their staging, one section each. Grow-only. (Last, as
  // tv_buf was: the frame path's fields keep their offsets.)
  DevBuf<uint8_t> fr_buf;
  // frontiers and components (tsdf_frontier_mark / tsdf_components; tsdf_host_frontier.hip): the control
  // words, a slot per voxel, the host arrays' staging, then accumulators and records per component, one
  // section each. Grow-only. (Last, as fr_buf was.)
  DevBuf<uint8_t> cc_buf;
  // view gain (tsdf_view_gain; tsdf_host_view.hip): the views, their gains, a batch's pixel records and, for
  // host arrays, their staging, one section each. Grow-only. (Last, as cc_buf was.)
  DevBuf<uint8_t> vw_buf;

  tsdf_engine() = default;
  // D's buffers, the pinned mirrors, events and streams; the scratch above frees itself. The caller has
  // made the engine's device current (tsdf_destroy; tsdf_create before it allocates).
  ~tsdf_engine();
};

// ---- helpers that cross the host files (the file that defines each) ----
// tsdf_engine.hip
FrameParams make_params(const tsdf_engine* e, const tsdf_intrinsics* K, int W, int H, const tsdf_pose* p,
                        float max_depth);
int join_render(tsdf_engine* e, bool keep_deferred = false, bool keep_graph = false);
int read_counters(tsdf_engine* e);
bool init_state(tsdf_engine* e, bool with_pool = true);
inline bool sharded(const tsdf_engine* e) { return e->cfg.shard_count > 1; }
inline bool mem_kind_ok(int k) { return k == TSDF_MEM_HOST || k == TSDF_MEM_DEVICE; }
inline bool frame_args_ok(const tsdf_engine* e, const tsdf_intrinsics* K, const tsdf_pose* pose, int W, int H) {
  return K && pose && W > 0 && H > 0 && (int64_t)W * H <= e->max_pixels;
}
// tsdf_host_frame.hip
int launch_resolve_alloc(tsdf_engine* e, const FrameParams& P, uint32_t range, int frame_mode);
int flush_pending(tsdf_engine* e);
int update_with_grid(tsdf_engine* e, const FrameParams& R, const ViewGrid& V);
bool pipe_frame_size(const tsdf_engine* e, int w, int h);
PipeArgs pipe_step(tsdf_engine* e, bool has_frame, uint32_t fid, const FrameParams& Pn);
void pipe_advance(tsdf_engine* e, uint32_t fid, const FrameParams& Pn);
void finish_args(tsdf_engine* e, PipeArgs& A, const FrameParams& Pu);
uint32_t next_fid(tsdf_engine* e);
// tsdf_host_graph.hip
int graph_flush_batch(tsdf_graph* g);
// tsdf_host_render.hip: the raycast view grid
// The cube's shape for a camera: ok = false when a view grid does not apply (hash lookups)
struct ViewShape {
  bool ok = false;
  int n = 0, nb = 0, ns = 0, nbw = 0, nw = 0, half = 0;
  int64_t cells = 0;  // brick-major (view_cell)
};
void view_shape_half(const tsdf_engine* e, int half, int lds_words, ViewShape* out);
bool view_grid_resets(const tsdf_engine* e, const FrameParams& P, float step_size, int lds_words);
int view_grid_take(tsdf_engine* e, const ViewShape& S, ViewGrid* V);
int view_grid_for(tsdf_engine* e, const FrameParams& P, float step_size, int lds_words, ViewGrid* V);
// tsdf_host_dose.hip: the block grid of a dose launch with A's receivers and emitters (em: their host
// copy). box: 8 + A.m device words (6 box words, two spare, one flag per emitter), hbox the same in pinned
// memory. Synchronises the stream once. *V keeps n == 0 (hash lookups) when the rays' cube is wider than a grid.
int dose_view_grid(tsdf_engine* e, DoseParams& A, const tsdf_uv_emitter* em, int32_t* box, int32_t* hbox,
                   ViewGrid* V);
// tsdf_host_track.hip: tracking, surface maps and dose are refused on a shard engine
bool track_refused(const tsdf_engine* e, const char* what);
// room for `bytes` of host maps / frames staged on the device
inline int track_stage(tsdf_engine* e, size_t bytes) { return e->tk_stage.ensure(bytes, "hipMalloc tk_stage"); }

#define JOIN_RENDER(e)              \
  do {                              \
    int _rc = join_render(e);       \
    if (_rc) return _rc;            \
  } while (0)

// every entry point that reads or writes the volume (or orders against it) first enqueues a deferred
// update (pipelined frames) and launches a deferred raycast or batch (join_render)
#define ENTER(e)                       \
  do {                                 \
    int _rc = join_render(e);          \
    if (_rc) return _rc;               \
    _rc = flush_pending(e);            \
    if (_rc) return _rc;               \
  } while (0)

#pragma GCC visibility pop
