// tsdf_host_mesh.hip -- marching-cubes mesh extraction: tsdf_extract_mesh, _owned and _indexed
// (kernels in tsdf_mesh.hip).
#include <limits>

#include "tsdf_host.h"

namespace {
int extract_mesh_impl(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight, int own_index,
                      int own_count, float* triangles, int64_t capacity, int64_t* num_triangles, int mem_kind) {
  if (!e || !num_triangles || (mem_kind != TSDF_MEM_HOST && mem_kind != TSDF_MEM_DEVICE) || own_count < 1 ||
      own_count > kMaxShards || own_index < 0 || own_index >= own_count) {
    set_error("tsdf_extract_mesh: invalid argument");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  short4 lo = make_short4(0, 0, 0, 0), hi = make_short4(0, 0, 0, 0);
  if (bounds) {  // the Query block selection (voxel_tsdf.cuh:21-26, voxel_tsdf.cu:429)
    const float scale = (float)(1. / (double)e->cfg.voxel_size);
    lo = make_short4(h_f2s(bounds[0] * scale), h_f2s(bounds[2] * scale), h_f2s(bounds[4] * scale), 0);
    hi = make_short4(h_f2s(bounds[1] * scale), h_f2s(bounds[3] * scale), h_f2s(bounds[5] * scale), 0);
  }
  hipStream_t s = e->stream;
  hipLaunchKernelGGL(k_query_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, bounds ? 1 : 0,
                     lo, hi);
  hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, e->D, e->q_sel,
                     e->q_count);
  LAUNCH_OK("mesh select");
  // selection, count, scan and (device output) emission enqueued back to back: the kernels read
  // the selected-block count and the triangle total from device memory, and the host reads the
  // total once at the end (a host output needs it first, to size the staging buffer)
  const MeshParams M{e->cfg.voxel_size, missing_tsdf, min_weight, own_index, own_count};
  hipLaunchKernelGGL(k_mesh<false>, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M,
                     e->m_counts, (const int32_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, e->m_nbr, (float*)nullptr);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, e->m_counts, e->q_count, e->m_offsets,
                     e->m_total);
  LAUNCH_OK("mesh count");
  const bool dev_out = triangles && mem_kind == TSDF_MEM_DEVICE;
  if (dev_out) {
    hipLaunchKernelGGL(k_mesh<true>, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M,
                       e->m_counts, (const int32_t*)e->m_offsets, (const int64_t*)e->m_total, capacity, e->m_nbr,
                       reinterpret_cast<float*>(triangles));
    LAUNCH_OK("mesh emit");
  }
  int64_t ntri = 0;
  HIP_OK(hipMemcpyAsync(&ntri, e->m_total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  *num_triangles = ntri;
  if (!triangles || ntri == 0) return TSDF_OK;
  if (capacity < ntri) {  // (device output: the emit pass wrote nothing)
    set_error("tsdf_extract_mesh: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  if (dev_out) return TSDF_OK;
  if (int rc = e->m_out.ensure((size_t)ntri * 9, "tsdf_extract_mesh: hipMalloc m_out")) return rc;
  hipLaunchKernelGGL(k_mesh<true>, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M,
                     e->m_counts, (const int32_t*)e->m_offsets, (const int64_t*)e->m_total, ntri, e->m_nbr, e->m_out);
  LAUNCH_OK("mesh emit");
  HIP_OK(hipMemcpyAsync(triangles, e->m_out, (size_t)ntri * 9 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}
}  // namespace

int tsdf_extract_mesh(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                      float* triangles, int64_t capacity, int64_t* num_triangles, int mem_kind) {
  TraceRange trace_("tsdf_extract_mesh");
  return extract_mesh_impl(e, bounds, missing_tsdf, min_weight, 0, 1, triangles, capacity, num_triangles,
                           mem_kind);
}

int tsdf_extract_mesh_owned(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                            int shard_index, int shard_count, float* triangles, int64_t capacity,
                            int64_t* num_triangles, int mem_kind) {
  TraceRange trace_("tsdf_extract_mesh_owned");
  return extract_mesh_impl(e, bounds, missing_tsdf, min_weight, shard_index, shard_count, triangles, capacity,
                           num_triangles, mem_kind);
}

int tsdf_extract_mesh_indexed(tsdf_engine* e, const float* bounds, float missing_tsdf, int min_weight,
                              const tsdf_mesh_out* out, int64_t* num_vertices, int64_t* num_triangles) {
  TraceRange trace_("tsdf_extract_mesh_indexed");
  if (!e || !num_vertices || !num_triangles ||
      (out && (!out->positions || !out->indices || out->vertex_capacity < 0 || out->triangle_capacity < 0 ||
               (reinterpret_cast<uintptr_t>(out->rgba) & 3) != 0 ||
               (out->mem_kind != TSDF_MEM_HOST && out->mem_kind != TSDF_MEM_DEVICE)))) {
    set_error("tsdf_extract_mesh_indexed: invalid argument (positions and indices are required with out; rgba 4-byte aligned)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (e->cfg.shard_count > 1) {
    set_error("tsdf_extract_mesh_indexed: not available on a shard engine (shard_count > 1)");
    return TSDF_ERR_INVALID_ARG;
  }
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  short4 lo = make_short4(0, 0, 0, 0), hi = make_short4(0, 0, 0, 0);
  if (bounds) {  // the Query block selection (voxel_tsdf.cuh:21-26, voxel_tsdf.cu:429)
    const float scale = (float)(1. / (double)e->cfg.voxel_size);
    lo = make_short4(h_f2s(bounds[0] * scale), h_f2s(bounds[2] * scale), h_f2s(bounds[4] * scale), 0);
    hi = make_short4(h_f2s(bounds[1] * scale), h_f2s(bounds[3] * scale), h_f2s(bounds[5] * scale), 0);
  }
  hipStream_t s = e->stream;
  const int nb = e->D.nblocks;
  // per pool block, allocated by the first call. The vertex counts and their scan are among them:
  // k_scan_counts scans as many counts as blocks are selected, also in the pass that finds the
  // selection larger than the edge records hold (it checks no capacity).
  if (int rc = e->mi_selmap.ensure((size_t)nb, "tsdf_extract_mesh_indexed: hipMalloc mi_selmap")) return rc;
  if (int rc = e->mi_vtotal.ensure(1, "tsdf_extract_mesh_indexed: hipMalloc mi_vtotal")) return rc;
  if (int rc = e->mi_vcounts.ensure((size_t)nb, "tsdf_extract_mesh_indexed: hipMalloc mi_vcounts")) return rc;
  if (int rc = e->mi_voffsets.ensure((size_t)nb, "tsdf_extract_mesh_indexed: hipMalloc mi_voffsets")) return rc;
  const MeshParams M{e->cfg.voxel_size, missing_tsdf, min_weight, 0, 1};
  const bool dev_out = out && out->mem_kind == TSDF_MEM_DEVICE;
  const int64_t vmax = std::numeric_limits<int32_t>::max();
  MeshIndexedOut O{};
  if (out) {
    O = MeshIndexedOut{out->positions, out->rgba, out->prob, out->keys, out->indices,
                       std::min(out->vertex_capacity, vmax), out->triangle_capacity};
  }
  auto scratch = [&] {
    return MeshIndexed{e->m_nbr,      e->m_counts,   e->m_offsets,  e->m_total,   e->mi_emask, e->mi_epre,
                       e->mi_vcounts, e->mi_voffsets, e->mi_vtotal, e->mi_selmap, e->mi_cap()};
  };
  auto emit = [&](const MeshIndexedOut& o) {
    hipLaunchKernelGGL(k_mesh_verts, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M, scratch(), o);
    hipLaunchKernelGGL(k_mesh_index, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M, scratch(), o);
  };
  // selection, the two count passes, their scans and (device output) the vertex and index passes
  // enqueued back to back; the host reads the selection size and the two totals once at the end. A
  // selection larger than the scratch holds makes every pass return at once: the scratch grows and
  // the passes run again (the first call, and after the volume has grown).
  int32_t nsel = 0;
  int64_t nv = 0, nt = 0;
  for (;;) {
    hipLaunchKernelGGL(k_query_count, dim3(kOccWords / 256), dim3(256), 0, s, e->D, bounds ? 1 : 0, lo, hi);
    hipLaunchKernelGGL(k_vis_emit, dim3(kOccWords / 256), dim3(256), 0, s, e->D, e->q_sel, e->q_count);
    LAUNCH_OK("indexed mesh select");
    if (e->mi_cap() > 0) {
      hipLaunchKernelGGL(k_mesh<false>, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M,
                         e->m_counts, (const int32_t*)nullptr, (const int64_t*)nullptr, (int64_t)0, e->m_nbr,
                         (float*)nullptr);
      hipLaunchKernelGGL(k_mesh_edges, dim3(e->mesh_grid), dim3(256), 0, s, e->D, e->q_sel, e->q_count, M, scratch());
      hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, e->m_counts, e->q_count, e->m_offsets, e->m_total);
      hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, e->mi_vcounts, e->q_count, e->mi_voffsets,
                         e->mi_vtotal);
      LAUNCH_OK("indexed mesh count");
      if (dev_out) {
        emit(O);
        LAUNCH_OK("indexed mesh emit");
      }
      HIP_OK(hipMemcpyAsync(&nv, e->mi_vtotal, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(&nt, e->m_total, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    }
    HIP_OK(hipMemcpyAsync(&nsel, e->q_count, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (nsel <= e->mi_cap()) break;
    release_all(e->mi_emask, e->mi_epre);
    const size_t cap = (size_t)std::min<int64_t>(nb, std::max<int64_t>((int64_t)nsel + nsel / 4, 1024));
    int rc = e->mi_emask.ensure(cap * kEdgeWords, "tsdf_extract_mesh_indexed: hipMalloc mi_emask");
    if (!rc) rc = e->mi_epre.ensure(cap * kEdgePre, "tsdf_extract_mesh_indexed: hipMalloc mi_epre");
    if (rc) return rc;
  }
  if (nsel == 0) nv = nt = 0;
  *num_vertices = nv;
  *num_triangles = nt;
  if (!out || (nv == 0 && nt == 0)) return TSDF_OK;
  if (nv > vmax || out->vertex_capacity < nv || out->triangle_capacity < nt) {  // (nothing was written)
    set_error("tsdf_extract_mesh_indexed: capacity too small");
    return TSDF_ERR_CAPACITY;
  }
  if (dev_out) return TSDF_OK;
  // host output: the passes write a staging buffer (sections 16-byte aligned), copied out per array
  Sections L;  // (every array has its section, asked for or not)
  const int h_pos = L.add((size_t)nv * 12), h_idx = L.add((size_t)nt * 12), h_rgba = L.add((size_t)nv * 4),
            h_prob = L.add((size_t)nv * 4), h_keys = L.add((size_t)nv * 16);
  if (int rc = e->mi_out.ensure(L.total(), "tsdf_extract_mesh_indexed: hipMalloc mi_out")) return rc;
  uint8_t* b = e->mi_out;
  const MeshIndexedOut S{L.at<float>(b, h_pos),
                         out->rgba ? L.at<uint8_t>(b, h_rgba) : nullptr,
                         out->prob ? L.at<float>(b, h_prob) : nullptr,
                         out->keys ? L.at<int32_t>(b, h_keys) : nullptr,
                         L.at<int32_t>(b, h_idx),
                         nv,
                         nt};
  emit(S);
  LAUNCH_OK("indexed mesh emit");
  HIP_OK(hipMemcpyAsync(out->positions, S.positions, (size_t)nv * 12, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(out->indices, S.indices, (size_t)nt * 12, hipMemcpyDeviceToHost, s));
  if (out->rgba) HIP_OK(hipMemcpyAsync(out->rgba, S.rgba, (size_t)nv * 4, hipMemcpyDeviceToHost, s));
  if (out->prob) HIP_OK(hipMemcpyAsync(out->prob, S.prob, (size_t)nv * 4, hipMemcpyDeviceToHost, s));
  if (out->keys) HIP_OK(hipMemcpyAsync(out->keys, S.keys, (size_t)nv * 16, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}
