// tsdf_dose.hip -- UV dose on surface points (DESIGN.md "UV dose"): the nearest voxel's unit normal
// of each point (k_point_normals), and for every receiver the inverse-square and cosine law over a list
// of point emitters with a shadow ray marched through the volume (k_uv_dose). k_dose_bounds measures
// what the block grid of a k_uv_dose call has to cover. All three only read the volume.
#include "tsdf_dose_march.h"

namespace tsdf {

__global__ __launch_bounds__(256) void k_point_normals(EngineDev D, const float* __restrict__ points, int64_t n,
                                                       float voxel, float offset, float* __restrict__ normals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const RayView R = hash_view();
  RayCache c;
  c.bx = c.by = c.bz = 0x7FFFFFFF;
  c.idx = -1;
  c.empty = 0;
  const f3 v = to_voxel(load3(points, i), voxel, offset);
  const int16_t fx = round_s16(v.x), fy = round_s16(v.y), fz = round_s16(v.z);
  const float gxp = ray_tsdf(D, R, c, (int16_t)(fx + 1), fy, fz);
  const float gxn = ray_tsdf(D, R, c, (int16_t)(fx - 1), fy, fz);
  const float gyp = ray_tsdf(D, R, c, fx, (int16_t)(fy + 1), fz);
  const float gyn = ray_tsdf(D, R, c, fx, (int16_t)(fy - 1), fz);
  const float gzp = ray_tsdf(D, R, c, fx, fy, (int16_t)(fz + 1));
  const float gzn = ray_tsdf(D, R, c, fx, fy, (int16_t)(fz - 1));
  const f3 nr = {gxp - gxn, gyp - gyn, gzp - gzn};
  const float nn = dot3(nr, nr);
  f3 out = {0.0f, 0.0f, 0.0f};
  if (nn > 0.0f && nn < __builtin_inff()) {  // (NaN fails both)
    const float len = sqrtf(nn);
    out = {nr.x / len, nr.y / len, nr.z / len};
  }
  normals[3 * i] = out.x;
  normals[3 * i + 1] = out.y;
  normals[3 * i + 2] = out.z;
}

__global__ __launch_bounds__(256) void k_dose_bounds(DoseParams A, int32_t* __restrict__ box,
                                                     int32_t* __restrict__ eflag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < A.n;
  const f3 p = load3(A.points, valid ? i : 0), nrm = load3(A.normals, valid ? i : 0);
  const bool recv = valid && (nrm.x != 0.0f || nrm.y != 0.0f || nrm.z != 0.0f);
  bool any = false;
  for (int k = 0; k < A.m; ++k) {
    float c, r2;
    const bool lit = recv && irradiates(A, p, nrm, A.emit[k], c, r2);
    any = any || lit;
    const unsigned long long b = __builtin_amdgcn_ballot_w64(lit);
    if (b != 0ull && lane_id() == __ffsll((long long)b) - 1) eflag[k] = 1;  // (every writer writes 1)
  }
  const f3 o = {p.x + A.bias * nrm.x, p.y + A.bias * nrm.y, p.z + A.bias * nrm.z};
  const f3 ov = to_voxel(o, A.voxel, A.offset);
  // a lit receiver is within max_range of an emitter: finite coordinates (f2i saturates the rest)
  int lo[3] = {f2i(floorf(ov.x)), f2i(floorf(ov.y)), f2i(floorf(ov.z))};
  int hi[3] = {f2i(ceilf(ov.x)), f2i(ceilf(ov.y)), f2i(ceilf(ov.z))};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!any) lo[a] = 0x7FFFFFFF, hi[a] = (int)0x80000000;
    for (int s = 32; s > 0; s >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], s, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], s, 64));
    }
  }
  if (lane_id() == 0 && lo[0] <= hi[0]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&box[a], lo[a]);
      atomicMax(&box[3 + a], hi[a]);
    }
  }
}

// (dose_body, tsdf_dose_march.h)
__global__ __launch_bounds__(256) void k_uv_dose(EngineDev D, DoseParams A, ViewGrid V) {
  extern __shared__ uint32_t sbits[];
  const int nw = V.n ? V.nw : 0;
  for (int i = threadIdx.x; i < nw; i += 256) sbits[i] = V.bits[i];
  __syncthreads();
  dose_body<false>(D, A, V, sbits, nullptr, 0, nullptr);
}

}  // namespace tsdf
