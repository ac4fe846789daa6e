// tsdf_track.hip -- frame-to-model pose tracking (DESIGN.md "Pose tracking"): the raycast's hits as
// float surface maps (k_raycast_surface) and one point-to-plane ICP linearisation of a depth frame
// against such maps (k_icp_partial + k_icp_final). The Gauss-Newton loop around them runs on the host
// (tsdf_track, tsdf_engine.hip; the solve and the pose update in tsdf_track_host.h).
#include "tsdf_raycast.h"

namespace tsdf {

__global__ __launch_bounds__(256) TSDF_RAY_PK void k_raycast_surface(EngineDev D, FrameParams P, float step_size,
                                                                     ViewGrid V, SurfaceOut S) {
  extern __shared__ uint32_t sbits[];
  raycast<true>(D, P, step_size, V, sbits, nullptr, nullptr, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x,
                gridDim.x * gridDim.y, S);
}

// tsdf_track's model normals, from the surface points: the six-neighbour central difference of
// nearest-voxel samples that the surface maps carry is a usable normal only where a depth pixel is no
// wider than a voxel (DESIGN.md "Pose tracking": a median 31 degrees off at four voxels per pixel, and
// point-to-plane ICP then converges to a wrong pose), while the points themselves are good. At a pixel
// whose four neighbours and itself have a surface: c = (p[v+1][u] - p[v-1][u]) x (p[v][u+1] - p[v][u-1]),
// turned to face the camera, over its length. No normal (zeros: the linearisation drops the pixel) on
// the border, beside a hole, and where c is more than acos(kTrackMinCos) off the viewing ray: a
// grazing surface, or a difference across a depth edge. One thread per pixel, 16x16 tiles.
__global__ __launch_bounds__(256) void k_surface_normals(FrameParams P, const float* __restrict__ point,
                                                         const float* __restrict__ normal, float* __restrict__ out) {
  const int u = blockIdx.x * 16 + (threadIdx.x & 15), v = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (u >= P.W || v >= P.H) return;
  const size_t i = (size_t)v * P.W + u;
  auto has = [&](size_t k) { return normal[3 * k] != 0.0f || normal[3 * k + 1] != 0.0f || normal[3 * k + 2] != 0.0f; };
  auto at = [&](size_t k) { return f3{point[3 * k], point[3 * k + 1], point[3 * k + 2]}; };
  f3 n = {0.0f, 0.0f, 0.0f};
  if (u > 0 && v > 0 && u < P.W - 1 && v < P.H - 1 && has(i) && has(i - 1) && has(i + 1) && has(i - P.W) &&
      has(i + P.W)) {
    const f3 a = at(i + 1), b = at(i - 1), c1 = at(i + P.W), d = at(i - P.W), p = at(i);
    const f3 dx = {a.x - b.x, a.y - b.y, a.z - b.z}, dy = {c1.x - d.x, c1.y - d.y, c1.z - d.z};
    f3 c = cross3(dy, dx);
    const f3 to = {p.x - P.wt.x, p.y - P.wt.y, p.z - P.wt.z};
    const float dv = dot3(c, to);
    if (dv > 0.0f) c = {-c.x, -c.y, -c.z};
    const float nn = dot3(c, c);
    if (nn > 0.0f && nn < __builtin_inff() && dv * dv >= (kTrackMinCos * kTrackMinCos) * (nn * dot3(to, to))) {
      const float len = sqrtf(nn);
      n = {c.x / len, c.y / len, c.z / len};
    }
  }
  out[3 * i] = n.x;
  out[3 * i + 1] = n.y;
  out[3 * i + 2] = n.z;
}

// The 29 sums of one linearisation, deterministic: which sample a lane takes and the shape of the
// addition tree depend on (W, H, stride) alone.
//   lane       one sample: its 29 terms in double (each product of two floats is exact), zeros when
//              a gate drops the sample
//   wave       xor butterfly over lanes 32, 16, 8, 4, 2, 1: every lane ends with the same sum (both
//              partners of a step add the same two values)
//   workgroup  the four waves' sums through LDS, ((w0 + w1) + w2) + w3
//   grid       k_icp_final, one workgroup: the nwg partials in kIcpChunks runs of ceil(nwg / kIcpChunks)
//              consecutive workgroups, each run added in index order from 0, then the runs' sums in
//              index order from 0
// No atomics and no waits: two launches.
__global__ __launch_bounds__(256) void k_icp_partial(IcpParams I, double* __restrict__ part) {
  __shared__ double sw[4][kIcpSums];
  const int s = blockIdx.x * 256 + threadIdx.x;
  float J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float r = 0.0f;
  bool keep = false;
  if (s < I.nsamples) {
    const int u = (s % I.nsx) * I.stride, v = (s / I.nsx) * I.stride;
    const float d = I.depth[(size_t)v * I.F.W + u];
    if (d > 0.0f && d <= I.F.max_depth) {  // (a NaN fails)
      const f3 ray = pixel_ray(I.F, u, v);
      const f3 pc = {ray.x * d, ray.y * d, d};
      const f3 pw = se3_apply(I.F.wq, I.F.wt, pc);
      const f3 pm = se3_apply(I.M.cq, I.M.ct, pw);
      if (pm.z > 0.0f) {
        // the nearest model pixel, half to even (v_rndne_f32); compared as floats: no conversion of
        // a value outside int's range, and a NaN fails
        const float fu = rintf(I.M.fx * (pm.x / pm.z) + I.M.cx);
        const float fv = rintf(I.M.fy * (pm.y / pm.z) + I.M.cy);
        if (fu >= 0.0f && fu < (float)I.M.W && fv >= 0.0f && fv < (float)I.M.H) {
          const size_t m = ((size_t)(int)fv * I.M.W + (int)fu) * 3;
          const f3 q = {I.point[m], I.point[m + 1], I.point[m + 2]};
          const f3 n = {I.normal[m], I.normal[m + 1], I.normal[m + 2]};
          if (n.x != 0.0f || n.y != 0.0f || n.z != 0.0f) {
            const f3 e = {pw.x - q.x, pw.y - q.y, pw.z - q.z};
            if (dot3(e, e) <= I.max_dist2) {
              r = dot3(n, e);
              const f3 c = cross3(pw, n);
              J[0] = c.x, J[1] = c.y, J[2] = c.z, J[3] = n.x, J[4] = n.y, J[5] = n.z;
              keep = true;
            }
          }
        }
      }
    }
  }
  double a[kIcpSums];
  const double rd = (double)r;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) a[k++] = (double)J[i] * (double)J[j];
#pragma unroll
  for (int i = 0; i < 6; ++i) a[21 + i] = (double)J[i] * rd;
  a[27] = rd * rd;
  a[28] = keep ? 1.0 : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int i = 0; i < kIcpSums; ++i) a[i] += __shfl_xor(a[i], o, 64);
  const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (ln == 0)
#pragma unroll
    for (int i = 0; i < kIcpSums; ++i) sw[wv][i] = a[i];
  __syncthreads();
  if (threadIdx.x < kIcpSums) {
    const int i = threadIdx.x;
    part[(size_t)blockIdx.x * kIcpSums + i] = ((sw[0][i] + sw[1][i]) + sw[2][i]) + sw[3][i];
  }
}

// (a single thread per sum walking every partial measured 279 us for the 1200 workgroups of a 640x480
// frame at stride 1: one exposed load latency per partial)
__global__ __launch_bounds__(1024) void k_icp_final(const double* __restrict__ part, int nwg,
                                                    double* __restrict__ out) {
  __shared__ double sc[kIcpChunks][kIcpSums];
  const int i = threadIdx.x % kIcpSums, c = threadIdx.x / kIcpSums;
  if (c < kIcpChunks) {
    const int len = (nwg + kIcpChunks - 1) / kIcpChunks;
    const int g1 = min(nwg, (c + 1) * len);
    int g = c * len;
    double acc = 0.0;
    for (; g + 8 <= g1; g += 8) {  // eight loads in flight, added in index order
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = part[(size_t)(g + k) * kIcpSums + i];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; g < g1; ++g) acc += part[(size_t)g * kIcpSums + i];
    sc[c][i] = acc;
  }
  __syncthreads();
  if (threadIdx.x < kIcpSums) {
    double acc = 0.0;
    for (int k = 0; k < kIcpChunks; ++k) acc += sc[k][threadIdx.x];
    out[threadIdx.x] = acc;
  }
}

}  // namespace tsdf
