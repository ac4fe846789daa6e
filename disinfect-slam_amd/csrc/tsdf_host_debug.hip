// tsdf_host_debug.hip -- snapshot / restore, tsdf_debug_dump and the hash- and pool-level test hooks
// (tsdf_hash_*, tsdf_pool_*).
#include <cstring>
#include <vector>

#include "tsdf_host.h"

// the test scratch for n points (at least 1024)
static int ensure_test_cap(tsdf_engine* e, int n) {
  if ((size_t)n <= e->t_s4.cap) return TSDF_OK;
  release_all(e->t_keys, e->t_recs, e->t_i32, e->t_u32, e->t_f0, e->t_f1, e->t_s4);
  const size_t cap = (size_t)std::max(n, 1024);
  int rc = e->t_keys.ensure(cap * 3, "test scratch: hipMalloc t_keys");
  if (!rc) rc = e->t_recs.ensure(cap, "test scratch: hipMalloc t_recs");
  if (!rc) rc = e->t_i32.ensure(cap, "test scratch: hipMalloc t_i32");
  if (!rc) rc = e->t_u32.ensure(cap, "test scratch: hipMalloc t_u32");
  if (!rc) rc = e->t_f0.ensure(cap, "test scratch: hipMalloc t_f0");
  if (!rc) rc = e->t_f1.ensure(cap, "test scratch: hipMalloc t_f1");
  if (!rc) rc = e->t_s4.ensure(cap, "test scratch: hipMalloc t_s4");
  return rc;
}

// ---------------------------------------------------------------------------------------------
// Snapshot / restore (SURVEY.md 5 checkpoint / resume; the reference only dumps GatherValid to a
// file, examples/tsdf/offline.cc:181-187). The whole engine state between frames -- hash table,
// occupancy bitmap, free-block stack, voxel pool (free blocks included: a re-acquired block keeps
// its old colour, voxel_mem.cu:43-51) and counters -- so a restored engine continues a stream bit
// for bit. Layout: header | counters | table | occ | heap | pool.
// ---------------------------------------------------------------------------------------------
namespace {
struct SnapshotHeader {
  char magic[8];  // "TSDFSNAP"
  uint32_t version;
  int32_t nblocks;
  float voxel, truncation;
  int64_t bytes;
  int32_t shard_index, shard_count;
};
constexpr uint32_t kSnapshotVersion = 2;

// A snapshot is accepted only if the state it describes is one the engine could have reached: the
// free stack and the table's pool indices partition the pool, foreign entries only on a shard,
// the occupancy bits are exactly the entries with voxels here, and every bucket's list ends. A
// corrupt or hand-edited one would otherwise send the next frame's kernels out of bounds.
bool snapshot_consistent(const tsdf_engine* e, const uint8_t* p) {
  const int nb = e->D.nblocks;
  DevCounters c;
  std::memcpy(&c, p, sizeof(c));
  p += sizeof(DevCounters);
  const int4* table = reinterpret_cast<const int4*>(p);
  p += (size_t)kNumEntry * 16;
  const uint64_t* occ = reinterpret_cast<const uint64_t*>(p);
  p += (size_t)kOccWords * 8;
  const int32_t* heap = reinterpret_cast<const int32_t*>(p);
  if (c.free_count < 0 || c.free_count > nb) return false;
  std::vector<uint8_t> seen((size_t)nb, 0);
  for (int i = 0; i < c.free_count; ++i) {
    const int32_t b = heap[i];
    if (b < 0 || b >= nb || seen[b]) return false;
    seen[b] = 1;
  }
  int64_t occupied = 0, held = 0;
  for (uint32_t en = 0; en < kNumEntry; ++en) {
    const int32_t idx = table[en].z;
    const bool bit = (occ[en >> 6] >> (en & 63)) & 1ull;
    if (idx == -1) {
      if (bit) return false;
      continue;
    }
    ++occupied;
    if (idx == kForeignIdx) {
      if (e->cfg.shard_count <= 1 || bit) return false;
      continue;
    }
    if (idx < 0 || idx >= nb || seen[idx] || !bit) return false;
    seen[idx] = 1;
    ++held;
  }
  if (held + c.free_count != nb) return false;
  // bucket lists (slot 1's offset chain) end within the occupied entries
  for (uint32_t b = 0; b < kNumBucket; ++b) {
    uint32_t last = 2 * b + 1;
    int16_t off = (int16_t)((uint32_t)table[last].y >> 16);
    for (int64_t steps = 0; off; ++steps) {
      if (steps > occupied) return false;
      last = (uint32_t)(last + (int32_t)off) & kEntryMask;
      off = (int16_t)((uint32_t)table[last].y >> 16);
    }
  }
  return true;
}

int64_t snapshot_bytes(const tsdf_engine* e) {
  return (int64_t)sizeof(SnapshotHeader) + (int64_t)sizeof(DevCounters) + (int64_t)kNumEntry * 16 +
         (int64_t)kOccWords * 8 + (int64_t)e->D.nblocks * 4 + (int64_t)e->D.nblocks * kBlockBytes;
}
}  // namespace

int tsdf_snapshot_bytes(tsdf_engine* e, int64_t* bytes) {
  if (!e || !bytes) return TSDF_ERR_INVALID_ARG;
  *bytes = snapshot_bytes(e);
  return TSDF_OK;
}

int tsdf_snapshot_save(tsdf_engine* e, void* out, int64_t capacity) {
  TraceRange trace_("tsdf_snapshot_save");
  if (!e || !out) return TSDF_ERR_INVALID_ARG;
  if (e->shard_phase != 0) {
    set_error("tsdf_snapshot_save: a sharded frame is pending");
    return TSDF_ERR_INVALID_ARG;
  }
  const int64_t need = snapshot_bytes(e);
  if (capacity < need) {
    set_error("tsdf_snapshot_save: buffer smaller than tsdf_snapshot_bytes");
    return TSDF_ERR_CAPACITY;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  hipStream_t s = e->stream;
  uint8_t* p = static_cast<uint8_t*>(out);
  SnapshotHeader h{};
  std::memcpy(h.magic, "TSDFSNAP", 8);
  h.version = kSnapshotVersion;
  h.nblocks = e->D.nblocks;
  h.voxel = e->cfg.voxel_size;
  h.truncation = e->cfg.truncation;
  h.bytes = need;
  h.shard_index = e->cfg.shard_index;
  h.shard_count = e->cfg.shard_count;
  std::memcpy(p, &h, sizeof(h));
  p += sizeof(h);
  HIP_OK(hipMemcpyAsync(p, e->D.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost, s));
  p += sizeof(DevCounters);
  HIP_OK(hipMemcpyAsync(p, e->D.table, (size_t)kNumEntry * 16, hipMemcpyDeviceToHost, s));
  p += (size_t)kNumEntry * 16;
  HIP_OK(hipMemcpyAsync(p, e->D.occ, (size_t)kOccWords * 8, hipMemcpyDeviceToHost, s));
  p += (size_t)kOccWords * 8;
  HIP_OK(hipMemcpyAsync(p, e->D.heap, (size_t)e->D.nblocks * 4, hipMemcpyDeviceToHost, s));
  p += (size_t)e->D.nblocks * 4;
  HIP_OK(hipMemcpyAsync(p, e->D.pool, (size_t)e->D.nblocks * kBlockBytes, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_snapshot_load(tsdf_engine* e, const void* in, int64_t size) {
  TraceRange trace_("tsdf_snapshot_load");
  if (!e || !in || size < (int64_t)sizeof(SnapshotHeader)) return TSDF_ERR_INVALID_ARG;
  SnapshotHeader h;
  std::memcpy(&h, in, sizeof(h));
  if (std::memcmp(h.magic, "TSDFSNAP", 8) != 0 || h.version != kSnapshotVersion || h.nblocks != e->D.nblocks ||
      h.voxel != e->cfg.voxel_size || h.truncation != e->cfg.truncation || h.bytes != snapshot_bytes(e) ||
      size < h.bytes || h.shard_index != e->cfg.shard_index || h.shard_count != e->cfg.shard_count ||
      e->shard_phase != 0) {
    set_error("tsdf_snapshot_load: not a snapshot of an engine with this configuration");
    return TSDF_ERR_INVALID_ARG;
  }
  if (!snapshot_consistent(e, static_cast<const uint8_t*>(in) + sizeof(h))) {
    set_error("tsdf_snapshot_load: inconsistent snapshot (pool indices, free stack, occupancy or "
              "bucket lists)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  hipStream_t s = e->stream;
  const uint8_t* p = static_cast<const uint8_t*>(in) + sizeof(h);
  HIP_OK(hipMemcpyAsync(e->D.ctr, p, sizeof(DevCounters), hipMemcpyHostToDevice, s));
  p += sizeof(DevCounters);
  HIP_OK(hipMemcpyAsync(e->D.table, p, (size_t)kNumEntry * 16, hipMemcpyHostToDevice, s));
  p += (size_t)kNumEntry * 16;
  HIP_OK(hipMemcpyAsync(e->D.occ, p, (size_t)kOccWords * 8, hipMemcpyHostToDevice, s));
  p += (size_t)kOccWords * 8;
  HIP_OK(hipMemcpyAsync(e->D.heap, p, (size_t)e->D.nblocks * 4, hipMemcpyHostToDevice, s));
  p += (size_t)e->D.nblocks * 4;
  HIP_OK(hipMemcpyAsync(e->D.pool, p, (size_t)e->D.nblocks * kBlockBytes, hipMemcpyHostToDevice, s));
  // lock words hold older epochs than the restored counter's (launches lock with epoch + 1)
  HIP_OK(hipMemsetAsync(e->D.lock_tag, 0, sizeof(uint32_t) * kNumBucket, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_debug_dump(tsdf_engine* e, int16_t* pos_off, int32_t* idx, int32_t* heap,
                    int32_t* free_count, float* tsdf_out, float* prob, uint8_t* rgbw) {
  if (!e) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  hipStream_t s = e->stream;
  if (pos_off || idx) {
    DevBuf<short4> dpos;  // (freed when the block ends: after its synchronisation)
    DevBuf<int32_t> didx;
    if (int rc = dpos.ensure(kNumEntry, "tsdf_debug_dump: hipMalloc table")) return rc;
    if (int rc = didx.ensure(kNumEntry, "tsdf_debug_dump: hipMalloc table")) return rc;
    hipLaunchKernelGGL(k_dump_table, dim3(kNumEntry / 256), dim3(256), 0, s, e->D, dpos, didx);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && pos_off)
      err = hipMemcpyAsync(pos_off, dpos, sizeof(short4) * kNumEntry, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && idx)
      err = hipMemcpyAsync(idx, didx, sizeof(int32_t) * kNumEntry, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {
      set_error("tsdf_debug_dump table", err);
      return TSDF_ERR_HIP;
    }
  }
  if (heap)
    HIP_OK(hipMemcpyAsync(heap, e->D.heap, sizeof(int32_t) * e->D.nblocks, hipMemcpyDeviceToHost, s));
  if (free_count) {
    int rc = read_counters(e);
    if (rc) return rc;
    *free_count = e->h_ctr->free_count;
  }
  if (tsdf_out || prob || rgbw) {
    const size_t nv = (size_t)e->D.nblocks * kBlockVolume;
    DevBuf<float> dt, dp;  // (freed when the block ends: after its synchronisation)
    DevBuf<uint32_t> dc;
    if (int rc = dt.ensure(nv, "tsdf_debug_dump: hipMalloc pool")) return rc;
    if (int rc = dp.ensure(nv, "tsdf_debug_dump: hipMalloc pool")) return rc;
    if (int rc = dc.ensure(nv, "tsdf_debug_dump: hipMalloc pool")) return rc;
    hipLaunchKernelGGL(k_dump_pool, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, e->D, dt,
                       dp, dc);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && tsdf_out) err = hipMemcpyAsync(tsdf_out, dt, nv * 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && prob) err = hipMemcpyAsync(prob, dp, nv * 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess && rgbw) err = hipMemcpyAsync(rgbw, dc, nv * 4, hipMemcpyDeviceToHost, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);
    if (err != hipSuccess) {
      set_error("tsdf_debug_dump pool", err);
      return TSDF_ERR_HIP;
    }
  }
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_hash_allocate(tsdf_engine* e, const int16_t* keys, int n) {
  if (!e || n < 0 || (n > 0 && !keys) || n > (int)kNewKeyCap) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(e->t_keys, keys, sizeof(int16_t) * 3 * n, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_keys_to_newset, dim3((n + 255) / 256), dim3(256), 0, e->stream, e->D,
                     e->t_keys, n);
  LAUNCH_OK("k_keys_to_newset");
  rc = launch_resolve_alloc(e, FrameParams{}, (uint32_t)n, 0);
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_hash_delete(tsdf_engine* e, const int16_t* keys, int n) {
  if (!e || n < 0 || (n > 0 && !keys)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  std::vector<VisRec> recs(n);
  for (int i = 0; i < n; ++i) {
    recs[i].x = keys[3 * i];
    recs[i].y = keys[3 * i + 1];
    recs[i].z = keys[3 * i + 2];
    recs[i].pad = 0;
    recs[i].idx = -1;
    recs[i].entry = -1;
  }
  HIP_OK(hipMemcpyAsync(e->t_recs, recs.data(), sizeof(VisRec) * n, hipMemcpyHostToDevice, e->stream));
  HIP_OK(hipMemcpyAsync(e->t_count, &n, sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_resolve_delete, dim3(1), dim3(kRT), 0, e->stream, e->D, (const VisRec*)e->t_recs,
                     (const int32_t*)e->t_count, 1, (const ShardRec*)nullptr, 0, 0);
  LAUNCH_OK("k_resolve_delete");
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_hash_retrieve(tsdf_engine* e, const int16_t* pts, int n, uint8_t* rgbw, float* tsdf_out,
                       float* prob, int16_t* bpo, int32_t* bidx) {
  if (!e || n < 0 || (n > 0 && !pts)) return TSDF_ERR_INVALID_ARG;
  if (n == 0) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  hipStream_t s = e->stream;
  HIP_OK(hipMemcpyAsync(e->t_keys, pts, sizeof(int16_t) * 3 * n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_hash_retrieve, dim3((n + 255) / 256), dim3(256), 0, s, e->D, e->t_keys, n,
                     e->t_u32, e->t_f0, e->t_f1, e->t_s4, e->t_i32);
  LAUNCH_OK("k_hash_retrieve");
  if (rgbw) HIP_OK(hipMemcpyAsync(rgbw, e->t_u32, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (tsdf_out) HIP_OK(hipMemcpyAsync(tsdf_out, e->t_f0, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (prob) HIP_OK(hipMemcpyAsync(prob, e->t_f1, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (bpo) HIP_OK(hipMemcpyAsync(bpo, e->t_s4, 8 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (bidx) HIP_OK(hipMemcpyAsync(bidx, e->t_i32, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}

int tsdf_hash_assign(tsdf_engine* e, const int16_t* pts, int n, const uint8_t* rgbw, int* missing) {
  if (!e || n < 0 || (n > 0 && (!pts || !rgbw))) return TSDF_ERR_INVALID_ARG;
  if (missing) *missing = 0;
  if (n == 0) return TSDF_OK;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  hipStream_t s = e->stream;
  HIP_OK(hipMemcpyAsync(e->t_keys, pts, sizeof(int16_t) * 3 * n, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(e->t_u32, rgbw, 4 * (size_t)n, hipMemcpyHostToDevice, s));
  HIP_OK(hipMemsetAsync(e->t_count, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_hash_assign, dim3((n + 255) / 256), dim3(256), 0, s, e->D, e->t_keys, n,
                     e->t_u32, e->t_count);
  LAUNCH_OK("k_hash_assign");
  int m = 0;
  HIP_OK(hipMemcpyAsync(&m, e->t_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (missing) *missing = m;
  return TSDF_OK;
}

int tsdf_num_active_blocks(tsdf_engine* e, int32_t* out) {
  if (!e || !out) return TSDF_ERR_INVALID_ARG;
  int rc = read_counters(e);
  if (rc) return rc;
  *out = e->D.nblocks - e->h_ctr->free_count;
  return TSDF_OK;
}

int tsdf_pool_acquire(tsdf_engine* e, int n, int32_t* idx_out) {
  if (!e || n < 0 || (n > 0 && !idx_out)) return TSDF_ERR_INVALID_ARG;
  ENTER(e);
  if (n == 0) return TSDF_OK;
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pool_acquire, dim3(1), dim3(64), 0, e->stream, e->D, n, e->t_i32);
  LAUNCH_OK("k_pool_acquire");
  HIP_OK(hipMemcpyAsync(idx_out, e->t_i32, 4 * (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_pool_release(tsdf_engine* e, const int32_t* idx, int n) {
  if (!e || n < 0 || (n > 0 && !idx)) return TSDF_ERR_INVALID_ARG;
  ENTER(e);
  if (n == 0) return TSDF_OK;
  int rc = ensure_test_cap(e, n);
  if (rc) return rc;
  HIP_OK(hipMemcpyAsync(e->t_i32, idx, 4 * (size_t)n, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_pool_release, dim3(1), dim3(64), 0, e->stream, e->D, e->t_i32, n);
  LAUNCH_OK("k_pool_release");
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_pool_set_weight(tsdf_engine* e, int32_t block, uint8_t w) {
  if (!e || block < 0 || block >= e->D.nblocks) return TSDF_ERR_INVALID_ARG;
  ENTER(e);
  hipLaunchKernelGGL(k_pool_weight, dim3(1), dim3(kBlockVolume), 0, e->stream, e->D, block, 1, w,
                     (uint8_t*)nullptr);
  LAUNCH_OK("k_pool_weight");
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

int tsdf_pool_get_weights(tsdf_engine* e, int32_t block, uint8_t* out) {
  if (!e || !out || block < 0 || block >= e->D.nblocks) return TSDF_ERR_INVALID_ARG;
  ENTER(e);
  int rc = ensure_test_cap(e, kBlockVolume);
  if (rc) return rc;
  uint8_t* d = reinterpret_cast<uint8_t*>(e->t_u32.p);
  hipLaunchKernelGGL(k_pool_weight, dim3(1), dim3(kBlockVolume), 0, e->stream, e->D, block, 0,
                     (uint8_t)0, d);
  LAUNCH_OK("k_pool_weight");
  HIP_OK(hipMemcpyAsync(out, d, kBlockVolume, hipMemcpyDeviceToHost, e->stream));
  HIP_OK(hipStreamSynchronize(e->stream));
  return TSDF_OK;
}

