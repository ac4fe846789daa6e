// tsdf_host_edt.hip -- Euclidean distance field (DESIGN.md "Distance field"; kernels in tsdf_edt.hip):
// tsdf_distance_field.
#include "tsdf_host.h"

void tsdf_edt_config_default(tsdf_edt_config* c) {
  if (!c) return;
  *c = tsdf_edt_config{};
  c->max_dist = 255;
  c->min_weight = 1;
  c->sites = TSDF_EDT_SURFACE;
}

namespace {

bool edt_args_ok(const tsdf_edt_config& c) {
  // (the box grown by one voxel: a surface voxel's face neighbours are read)
  return box_dims_ok(c.dims) && box_in_block_range(c.origin, c.dims, 1) && c.max_dist >= 1 && c.max_dist <= 255 &&
         c.min_weight >= 0 && (c.sites == TSDF_EDT_SURFACE || c.sites == (TSDF_EDT_SURFACE | TSDF_EDT_UNKNOWN));
}

// one y or z pass: lines of L elements `stride` apart, ncol side by side in each of `slabs` slabs
template <typename In>
int line_pass(hipStream_t s, int64_t ncol, int64_t stride, int64_t slab, int slabs, int L, int R, const In* in,
              uint16_t* out) {
  EdtLine P{};
  P.ncol = ncol;
  P.stride = stride;
  P.slab = slab;
  P.L = L;
  P.A = std::min(R - 1, L - 1);
  P.cap = (uint32_t)(R * R);
  const bool small = 128 + 2 * P.A <= kEdtRowsSmall;
  P.T = small ? 128 : 256;
  static_assert(256 + 2 * 254 <= kEdtRowsLarge, "the large form's tile and apron");
  const dim3 grid((unsigned)((ncol + 63) / 64), (unsigned)((L + P.T - 1) / P.T), (unsigned)slabs);
  if (small)
    hipLaunchKernelGGL((k_edt_line<In, kEdtRowsSmall, 256>), grid, dim3(256), 0, s, P, in, out);
  else
    hipLaunchKernelGGL((k_edt_line<In, kEdtRowsLarge, 1024>), grid, dim3(1024), 0, s, P, in, out);
  LAUNCH_OK("k_edt_line");
  return TSDF_OK;
}

}  // namespace

int tsdf_distance_field(tsdf_engine* e, const tsdf_edt_config* cfg, const tsdf_edt_out* out) {
  TraceRange trace_("tsdf_distance_field");
  if (!e || !cfg || !out || !out->d2 || !mem_kind_ok(out->mem_kind) || !edt_args_ok(*cfg)) {
    set_error("tsdf_distance_field: invalid argument (" BOX_LIMITS_TEXT ", the box inside the block "
              "range, max_dist 1..255, min_weight >= 0, sites SURFACE or SURFACE | UNKNOWN, d2 non-NULL)");
    return TSDF_ERR_INVALID_ARG;
  }
  if (track_refused(e, "tsdf_distance_field")) return TSDF_ERR_INVALID_ARG;
  HIP_OK(hipSetDevice(e->device));
  ENTER(e);
  hipStream_t s = e->stream;
  const tsdf_edt_config& c = *cfg;
  EdtBox B{};
  B.ox = c.origin[0], B.oy = c.origin[1], B.oz = c.origin[2];
  B.nx = c.dims[0], B.ny = c.dims[1], B.nz = c.dims[2];
  B.cx0 = B.ox >> kBlockLenBits, B.cy0 = B.oy >> kBlockLenBits, B.cz0 = B.oz >> kBlockLenBits;
  B.cbx = ((B.ox + B.nx - 1) >> kBlockLenBits) - B.cx0 + 1;
  B.cby = ((B.oy + B.ny - 1) >> kBlockLenBits) - B.cy0 + 1;
  B.cbz = ((B.oz + B.nz - 1) >> kBlockLenBits) - B.cz0 + 1;
  B.rowbytes = (B.cbx + 3) & ~3;
  B.R = c.max_dist;
  B.min_weight = c.min_weight;
  B.unknown = (c.sites & TSDF_EDT_UNKNOWN) ? 1 : 0;
  const size_t n = box_voxels(c.dims), b_bits = (size_t)B.ny * B.nz * B.rowbytes;
  const bool host = out->mem_kind == TSDF_MEM_HOST;
  // sections: bitmap | x pass (u8) | y pass (u16) | host outputs' staging: d2, state
  Sections L;
  const int h_bits = L.add(b_bits), h_g = L.add(n), h_t = L.add(2 * n);
  const int h_d2 = L.add(staged(host, out->d2, 2 * n)), h_state = L.add(staged(host, out->state, n));
  int rc = e->edt_buf.ensure(L.total(), "tsdf_distance_field: hipMalloc edt_buf");
  if (rc) return rc;
  const Stage St{L, e->edt_buf.p, host, s};
  uint8_t* bits = L.at<uint8_t>(St.base, h_bits);
  uint8_t* g = L.at<uint8_t>(St.base, h_g);
  uint16_t* t = L.at<uint16_t>(St.base, h_t);
  uint16_t* d2 = St.ptr(h_d2, out->d2);
  uint8_t* state = St.ptr(h_state, out->state);
  HIP_OK(hipMemsetAsync(bits, 0, L.size(h_bits), s));
  if (state) HIP_OK(hipMemsetAsync(state, 0, n, s));
  hipLaunchKernelGGL(k_edt_classify, dim3((unsigned)(B.cbx * B.cby * B.cbz)), dim3(256), 0, s, e->D, B, bits, state);
  LAUNCH_OK("k_edt_classify");
  hipLaunchKernelGGL(k_edt_x, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, B,
                     reinterpret_cast<const uint32_t*>(bits), g);
  LAUNCH_OK("k_edt_x");
  const int64_t nx = B.nx, nxy = (int64_t)B.nx * B.ny;
  rc = line_pass<uint8_t>(s, nx, nx, nxy, B.nz, B.ny, B.R, g, t);  // along y: a slab per z
  if (rc) return rc;
  rc = line_pass<uint16_t>(s, nxy, nxy, 0, 1, B.nz, B.R, t, d2);   // along z: every (y, x) a line
  if (rc) return rc;
  HIP_OK(St.back(out->d2, d2, 2 * n));
  HIP_OK(St.back(out->state, state, n));
  if (host) HIP_OK(hipStreamSynchronize(s));
  return TSDF_OK;
}
