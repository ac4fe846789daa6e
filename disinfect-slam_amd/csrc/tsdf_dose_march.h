// tsdf_dose_march.h -- what the dose kernels share (tsdf_dose.hip: k_uv_dose; tsdf_plan.hip:
// k_uv_irradiance): the receiver / emitter law and the shadow-ray march of DESIGN.md "UV dose". Device
// code, included by those two files only.
#pragma once
#include "tsdf_raycast.h"

namespace tsdf {

namespace {
// a RayView without a grid: every lookup goes to the hash table (ray_block's last branch)
__device__ __forceinline__ RayView hash_view() {
  RayView R;
  R.cell = nullptr;
  R.bits = nullptr;
  R.n = R.nb = R.ns = R.nbw = 0;
  R.ox = R.oy = R.oz = 0;
  R.gen = 0;
  return R;
}
__device__ __forceinline__ f3 load3(const float* __restrict__ a, int64_t i) {
  return f3{a[3 * i], a[3 * i + 1], a[3 * i + 2]};
}
// voxel coordinate of world position w: w / voxel - offset per component
__device__ __forceinline__ f3 to_voxel(f3 w, float voxel, float offset) {
  return f3{w.x / voxel - offset, w.y / voxel - offset, w.z / voxel - offset};
}
// What a receiver and an emitter exchange without the volume in the way: r2, the cosine c, and whether
// the emitter counts at all (in range, on the normal's side). A NaN anywhere fails the test.
__device__ __forceinline__ bool irradiates(const DoseParams& A, f3 p, f3 nrm, float4 E, float& c, float& r2) {
  const f3 d = {E.x - p.x, E.y - p.y, E.z - p.z};
  r2 = dot3(d, d);
  const float r = sqrtf(r2);
  c = dot3(nrm, d) / r;
  return r >= A.min_range && r <= A.max_range && c > 0.0f;
}

// The body of both dose kernels after they staged V's brick bitmap in LDS (sbits, V.nw words). One lane per receiver (256 per workgroup along x); the emitters in list
// order in the outer, wave-uniform loop, so the 64 lanes of
// a wave -- neighbouring mesh vertices or surface pixels -- march a tight bundle of rays toward one
// point. Sample j of a ray is ov + (float)j * sg, a product and a sum, not a running sum: the samples
// do not depend on how the march visits them. The lanes step over a scalar sample counter (as the
// raycast's march: lanes stepping together overlap their loads), each holding the region of its last
// lookup -- the present block's pool index, or the missing block, empty brick or empty superbrick --
// as the open box of positions whose nearest voxel lies in it: round_s16(s) is in [lo, hi] for every s
// with lo - 0.5 < s < hi + 0.5 (ties go to a lookup, which is always right), and the box is cut to the
// int16 voxel range round_s16 saturates to. A lane whose ray is done (occluded, or past its last
// sample) idles until no lane of the wave is live.
// kRows false: k_uv_dose -- all A.m emitters, dose[i] = dose[i] + acc for a receiver with a normal.
// kRows true: k_uv_irradiance -- workgroup row blockIdx.y is candidate c = c0 + blockIdx.y, its emitters
// first[c] .. first[c + 1] - 1, and out[c * n + i] = acc for every receiver (0 without a normal).
template <bool kRows>
__device__ __forceinline__ void dose_body(const EngineDev& D, const DoseParams& A, const ViewGrid& V,
                                          const uint32_t* sbits, const int32_t* __restrict__ first, int c0,
                                          float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < A.n;
  const f3 p = load3(A.points, valid ? i : 0), nrm = load3(A.normals, valid ? i : 0);
  const bool recv = valid && (nrm.x != 0.0f || nrm.y != 0.0f || nrm.z != 0.0f);
  RayView R;
  R.cell = V.cell;
  R.bits = sbits;
  R.n = V.n;
  R.nb = V.nb;
  R.ns = V.ns;
  R.nbw = V.nbw;
  R.gen = V.gen;
  R.ox = A.ox;
  R.oy = A.oy;
  R.oz = A.oz;
  const f3 o = {p.x + A.bias * nrm.x, p.y + A.bias * nrm.y, p.z + A.bias * nrm.z};
  const f3 ov = to_voxel(o, A.voxel, A.offset);
  const float inf = __builtin_inff();
  float acc = 0.0f;
  int kbeg = 0, kend = A.m;
  if constexpr (kRows) {
    kbeg = first[c0 + (int)blockIdx.y];
    kend = first[c0 + (int)blockIdx.y + 1];
  }
  for (int k = kbeg; k < kend; ++k) {
    const float4 E = A.emit[k];  // (uniform)
    float c, r2;
    bool lit = recv && irradiates(A, p, nrm, E, c, r2);
    if (__builtin_amdgcn_ballot_w64(lit) == 0ull) continue;
    const f3 ev = to_voxel(f3{E.x, E.y, E.z}, A.voxel, A.offset);
    const f3 dv = {ev.x - ov.x, ev.y - ov.y, ev.z - ov.z};
    const float L = sqrtf(dot3(dv, dv));
    f3 sg = {0.0f, 0.0f, 0.0f};
    int J = 0;
    if (L > 0.0f) {
      sg = {dv.x / L * A.sv, dv.y / L * A.sv, dv.z / L * A.sv};
      // (the cap never binds: the host admits max_range / step <= 65536 and |bias| <= max_range)
      J = min(f2i(L / A.sv), 1 << 18);
    }
    // the region of the last lookup: none yet
    f3 flo = {inf, inf, inf}, fhi = {-inf, -inf, -inf};
    int32_t ridx = -1;
    int live = lit ? 1 : 0;
    for (int j = 0;; ++j) {
      if (__builtin_amdgcn_ballot_w64(live != 0) == 0ull) break;
      const float fj = (float)j;
      const f3 s = {ov.x + fj * sg.x, ov.y + fj * sg.y, ov.z + fj * sg.z};
      const bool inside = s.x > flo.x && s.x < fhi.x && s.y > flo.y && s.y < fhi.y && s.z > flo.z && s.z < fhi.z;
      // (inside an empty region: nothing occludes, nothing to read)
      if (live != 0 && (!inside || ridx >= 0)) {
        const int16_t px = round_s16(s.x), py = round_s16(s.y), pz = round_s16(s.z);
        if (!inside) {
          const int bx = px >> kBlockLenBits, by = py >> kBlockLenBits, bz = pz >> kBlockLenBits;
          int empty;
          ridx = march_lookup(D, R, bx, by, bz, empty);
          // 2^sh blocks per axis: a block, an empty brick, an empty superbrick (the raycast's regions)
          const int sh = 2 * empty;
          const int rx = (R.ox + (((bx - R.ox) >> sh) << sh)) * kBlockLen;
          const int ry = (R.oy + (((by - R.oy) >> sh) << sh)) * kBlockLen;
          const int rz = (R.oz + (((bz - R.oz) >> sh) << sh)) * kBlockLen;
          const float len = (float)(kBlockLen << sh);
          flo = {fmaxf((float)rx - 0.5f, -32768.5f), fmaxf((float)ry - 0.5f, -32768.5f),
                 fmaxf((float)rz - 0.5f, -32768.5f)};
          fhi = {fminf((float)rx - 0.5f + len, 32767.5f), fminf((float)ry - 0.5f + len, 32767.5f),
                 fminf((float)rz - 0.5f + len, 32767.5f)};
          if (empty) {  // a brick's bit speaks for the grid's blocks only: no farther than the grid
            const float gl = (float)(R.n * kBlockLen);
            const f3 g0 = {(float)(R.ox * kBlockLen) - 0.5f, (float)(R.oy * kBlockLen) - 0.5f,
                           (float)(R.oz * kBlockLen) - 0.5f};
            flo = {fmaxf(flo.x, g0.x), fmaxf(flo.y, g0.y), fmaxf(flo.z, g0.z)};
            fhi = {fminf(fhi.x, g0.x + gl), fminf(fhi.y, g0.y + gl), fminf(fhi.z, g0.z + gl)};
          }
        }
        if (ridx >= 0) {
          const uint8_t* blk = D.pool + (size_t)ridx * kBlockBytes;
          const int off = voxel_off(px, py, pz);
          if (reinterpret_cast<const float*>(blk)[off] <= 0.0f &&
              (int)(reinterpret_cast<const uint32_t*>(blk + kRgbwOffset)[off] >> 24) >= A.min_weight) {
            lit = false;  // occluded
            live = 0;
          }
        }
      }
      if (j >= J) live = 0;
    }
    if (lit) acc = acc + (E.w * 0.07957747f) * (c / r2);
  }
  if constexpr (kRows) {
    if (valid) out[(int64_t)(c0 + (int)blockIdx.y) * A.n + i] = recv ? acc : 0.0f;
  } else {
    if (recv) A.dose[i] = A.dose[i] + acc;
  }
}
}  // namespace

}  // namespace tsdf
