// tsdf_view.hip -- view gain (DESIGN.md "View gain"): the unobserved voxels of a box that a candidate camera
// pose would observe. k_view_depth predicts each view's depth image by marching the state array of a distance
// field, one lane per pixel, to the first sample in a state-2 voxel; k_view_gain is tsdf_free_observe's gather
// turned round: a workgroup per 64 x 8 x 8 brick keeps the brick's candidate voxels (state 0, not in `seen`)
// and counts, view by view, those the free test passes against the predicted image. Integers and single IEEE
// float32 operations throughout: the counts do not depend on the order of any atomic. The kernels do not
// touch the volume.
#include "tsdf_view.h"

namespace tsdf {

namespace {
// f2i(roundf(f)) for |f| < 2^22 (round_s16's form without the int16 clamp); beyond that the result is
// within one of it and far outside every box (|voxel| <= 2^18 + 2047), NaN -> 0 either way
__device__ __forceinline__ int round_vox(float f) {
  const int r = f2i(f + __builtin_copysignf(0.5f, f));
  return fabsf(f) < 0.5f ? 0 : r;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return __builtin_amdgcn_readfirstlane(v);
}

// The samples of a ray that can lie in the box: [jlo, jhi], empty when jlo > jhi, never narrower than the
// truth. Sample j sits near (wt + z_j D) / voxel in voxels, D = world_T_cam's rotation of dc: the same linear
// map as the march's, so only roundings differ, and those stay under a fraction of a voxel while every
// coordinate is below kViewSkipExtent. The box, grown by kViewSlack voxels, is cut per axis (slab test) in
// z; the interval then grows by two samples and 2^-18 relative. Anything out of range, infinite or NaN
// keeps the whole march.
__device__ __forceinline__ void march_interval(const ViewDepthArgs& A, const ViewCam& Cm, f3 dc, int& jlo,
                                               int& jhi) {
  const f3 D = qrot(Cm.wq, dc);
  const float av = fabsf(A.voxel);
  const float zfar = (float)A.J * A.step;
  const float lim = kViewSkipExtent * av;
  const float w[3] = {Cm.wt.x, Cm.wt.y, Cm.wt.z}, dd[3] = {D.x, D.y, D.z};
  const int o[3] = {A.ox, A.oy, A.oz}, n[3] = {A.nx, A.ny, A.nz};
  float t0 = 0.0f, t1 = zfar;
  bool ok = A.voxel > 0.0f && zfar < 0x1p60f, empty = false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ok = ok && fabsf(w[a]) <= lim && fabsf(dd[a]) * zfar <= lim;
    const float lo = ((float)o[a] - (0.5f + kViewSlack)) * A.voxel;
    const float hi = ((float)(o[a] + n[a]) - (0.5f - kViewSlack)) * A.voxel;
    if (dd[a] == 0.0f) {
      empty = empty || w[a] < lo || w[a] > hi;
    } else {
      const float ta = (lo - w[a]) / dd[a], tb = (hi - w[a]) / dd[a];
      ok = ok && ta == ta && tb == tb;
      t0 = fmaxf(t0, fminf(ta, tb));
      t1 = fminf(t1, fmaxf(ta, tb));
    }
  }
  if (!ok) return;
  if (empty || t0 > t1) {
    jlo = 1, jhi = 0;
    return;
  }
  const float jl = t0 * (1.0f - 0x1p-18f) / A.step - 2.0f, jh = t1 * (1.0f + 0x1p-18f) / A.step + 2.0f;
  if (!(jl == jl && jh == jh)) return;
  jlo = max(jlo, f2i(jl));  // (truncation toward zero of a value already two samples below)
  jhi = min(jhi, f2i(jh) + 1);
}

// brick_culled of the free layer (tsdf_free.hip) for a candidate view: max_depth replaced by the largest
// depth of the view's predicted image. vis needs 0 < hz, hz <= d (range (d - hz) >= margin >= 0) and a rounded
// pixel inside the image; the sphere's slack keeps every comparison strict. A NaN makes each false: no cull.
__device__ __forceinline__ bool view_brick_culled(const ViewGainArgs& A, const ViewCam& Cm, float dmax, int x0,
                                                  int y0, int z0) {
  const f3 cw = {((float)(A.ox + x0) + 31.5f) * A.voxel, ((float)(A.oy + y0) + 3.5f) * A.voxel,
                 ((float)(A.oz + z0) + 3.5f) * A.voxel};
  const f3 c = se3_apply(Cm.cq, Cm.ct, cw);
  const float r = kFreeBrickRadius * fabsf(A.voxel);
  if (c.z + r <= 0.0f) return true;
  if (c.z - r >= dmax) return true;
  const float l = A.cx + 1.5f, rt = A.cx - ((float)A.W + 0.5f);
  const float t = A.cy + 1.5f, b = A.cy - ((float)A.H + 0.5f);
  if (A.fx * c.x + l * c.z < -r * sqrtf(A.fx * A.fx + l * l)) return true;
  if (A.fx * c.x + rt * c.z > r * sqrtf(A.fx * A.fx + rt * rt)) return true;
  if (A.fy * c.y + t * c.z < -r * sqrtf(A.fy * A.fy + t * t)) return true;
  if (A.fy * c.y + b * c.z > r * sqrtf(A.fy * A.fy + b * b)) return true;
  return false;
}
}  // namespace

__global__ __launch_bounds__(256) void k_view_depth(ViewDepthArgs A) {
  const int npix = A.W * A.H;  // (at most 2^26)
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  const int view = (int)blockIdx.y;
  const bool valid = i < npix;
  const int ii = valid ? i : 0;
  const int v = ii / A.W, u = ii - v * A.W;
  const ViewCam Cm = A.cam[view];  // (uniform)
  const f3 dc = pixel_ray(A.ifx, A.ify, A.icx, A.icy, u, v);
  const float range = sqrtf(dot3(dc, dc));
  int jlo = 1, jhi = A.J;
  if (A.skip) march_interval(A, Cm, dc, jlo, jhi);
  if (!valid) jlo = 1, jhi = 0;
  bool live = jlo <= jhi;
  // the 64 neighbouring rays of a wave step over one scalar sample counter (as the dose march does): their
  // one-byte loads overlap and share cache lines
  const int wlo = wave_min_i(live ? jlo : 0x7FFFFFFF), whi = wave_max_i(live ? jhi : 0);
  float d = A.miss;
  for (int j = wlo; j <= whi; ++j) {
    if (__builtin_amdgcn_ballot_w64(live) == 0ull) break;
    if (live && j >= jlo) {
      // a product and a transform of j, never a running sum
      const float z = (float)j * A.step;
      const f3 pc = {dc.x * z, dc.y * z, z};
      const f3 pw = se3_apply(Cm.wq, Cm.wt, pc);
      const int gx = round_vox(quot_const(pw.x, A.voxel, A.inv_voxel)) - A.ox;
      const int gy = round_vox(quot_const(pw.y, A.voxel, A.inv_voxel)) - A.oy;
      const int gz = round_vox(quot_const(pw.z, A.voxel, A.inv_voxel)) - A.oz;
      // (a saturated coordinate minus the origin may wrap: the unsigned compare still rejects it, as the
      // origin's magnitude is below 2^19 and the dims below 2^12)
      if ((unsigned)gx < (unsigned)A.nx && (unsigned)gy < (unsigned)A.ny && (unsigned)gz < (unsigned)A.nz &&
          A.state[((size_t)gz * A.ny + gy) * A.nx + gx] == 2) {
        d = z;
        live = false;
      }
    }
    if (j >= jhi) live = false;
  }
  if (valid) {
    FreePix p;
    p.d = d;
    p.range = range;
    A.pix[(size_t)view * npix + i] = p;
    if (A.depth_out) A.depth_out[(size_t)view * npix + i] = d;
  }
  // the view's largest depth: d is never negative and never NaN, so the bits order as the floats do
  uint32_t m = valid ? __float_as_uint(d) : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
  if (((int)threadIdx.x & 63) == 0 && m) atomicMax(&A.cam[view].dmax_bits, m);
}

__global__ __launch_bounds__(256) void k_view_gain(ViewGainArgs A) {
  constexpr int kRows = kFreeBrickY * kFreeBrickZ;
  __shared__ unsigned long long s_cand[kRows];  // a row's candidates: state 0 and not seen
  __shared__ uint32_t s_cnt[kViewBatch];
  __shared__ int s_list[kViewBatch];  // the views that may see the brick
  __shared__ int s_nlive, s_any;
  const int x0 = (int)blockIdx.x * kFreeBrickX, y0 = (int)blockIdx.y * kFreeBrickY, z0 = (int)blockIdx.z * kFreeBrickZ;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_nlive = 0, s_any = 0;
  if (tid < kViewBatch) s_cnt[tid] = 0;
  __syncthreads();
  const int x = x0 + lane;
  for (int row = wave; row < kRows; row += 4) {
    const int y = y0 + (row & (kFreeBrickY - 1)), z = z0 + (row >> 3);
    bool c = false;
    if (x < A.nx && y < A.ny && z < A.nz) {
      const size_t r = (size_t)z * A.ny + y;
      c = A.state[r * A.nx + x] == 0;
      if (c && A.seen) c = !((A.seen[r * A.wx + (x >> 5)] >> (x & 31)) & 1u);
    }
    const unsigned long long m = __ballot(c);
    if (lane == 0) {
      s_cand[row] = m;
      if (m) s_any = 1;
    }
  }
  __syncthreads();
  if (!s_any) return;  // (the whole workgroup)
  if (tid < A.nv) {
    const ViewCam Cm = A.cam[tid];
    const float dmax = __uint_as_float(Cm.dmax_bits);
    // (an image of zeros sees nothing: d != 0 fails everywhere)
    const bool dead = A.cull && (dmax == 0.0f || (Cm.rigid && view_brick_culled(A, Cm, dmax, x0, y0, z0)));
    if (!dead) s_list[atomicAdd(&s_nlive, 1)] = tid;
  }
  __syncthreads();
  const int nlive = s_nlive;
  const int npix = A.W * A.H;
  const float gx = (float)(A.ox + x) * A.voxel;
  for (int k = 0; k < nlive; ++k) {
    const int vi = __builtin_amdgcn_readfirstlane(s_list[k]);
    const ViewCam Cm = A.cam[vi];
    const FreePix* __restrict__ pix = A.pix + (size_t)vi * npix;
    uint32_t count = 0;  // wave-uniform
    for (int row = wave; row < kRows; row += 4) {
      const unsigned long long m = s_cand[row];
      if (!m) continue;  // (wave-uniform)
      bool vis = false;
      if ((m >> lane) & 1ull) {
        const int y = y0 + (row & (kFreeBrickY - 1)), z = z0 + (row >> 3);
        const f3 pw = {gx, (float)(A.oy + y) * A.voxel, (float)(A.oz + z) * A.voxel};
        const f3 pc = se3_apply(Cm.cq, Cm.ct, pw);
        const float hx = A.fx * pc.x + A.cx * pc.z;
        const float hy = A.fy * pc.y + A.cy * pc.z;
        const float hz = pc.z;
        const float rz = __builtin_amdgcn_rcpf(hz);
        const int u = round_quot_i(hx, hz, rz);  // f2i(roundf(hx / hz)), exactly
        const int v = round_quot_i(hy, hz, rz);
        if (u >= 0 && u < A.W && v >= 0 && v < A.H) {
          const FreePix p = pix[v * A.W + u];
          const float sdf = p.range * (p.d - hz);
          vis = p.d != 0.0f && sdf >= A.margin && hz > 0.0f;
        }
      }
      count += (uint32_t)__popcll(__ballot(vis));
    }
    if (count && lane == 0) atomicAdd(&s_cnt[vi], count);
  }
  __syncthreads();
  // (a brick holds 2^15 voxels: a view's count fits the word)
  if (tid < A.nv && s_cnt[tid]) atomicAdd(&A.gain[tid], (unsigned long long)s_cnt[tid]);
}

}  // namespace tsdf
