// tsdf_edt.hip -- exact Euclidean distance field over a box of the volume (DESIGN.md "Distance field"):
// the voxels' classes and the site bitmap (k_edt_classify), then a separable transform: the distance
// along x from the bitmap (k_edt_x), and the min-plus with (i - j)^2 along y and along z (k_edt_line).
// All integers but the comparisons tsdf <= 0 and weight >= min_weight. The kernels only read the volume.
#include "tsdf_kernels.h"

namespace tsdf {

namespace {
// classes of a voxel (the `state` output)
constexpr uint8_t kUnobserved = 0, kFree = 1, kInside = 2;
__device__ __forceinline__ uint8_t voxel_class(const uint8_t* __restrict__ blk, int off, int min_weight) {
  const float t = reinterpret_cast<const float*>(blk)[off];
  const int w = (int)(reinterpret_cast<const uint32_t*>(blk + kRgbwOffset)[off] >> 24);
  return w >= min_weight ? (t <= 0.0f ? kInside : kFree) : kUnobserved;
}
// cell (a, b, c) in [-1, 8]^3 of the staged classes
__device__ __forceinline__ int cls_at(int a, int b, int c) { return (a + 1) + 10 * (b + 1) + 100 * (c + 1); }
}  // namespace

// The block and its six face neighbours are looked up once (lanes 0-6); a present block's classes are
// staged in LDS with the one-voxel face halo (edges and corners of the 10^3 cube are never read), as
// k_mesh_edges stages its samples. A wave holds one z-slice of the block per round, x fastest, so the
// ballot of the site predicate is the slice's eight row bytes.
__global__ __launch_bounds__(256) void k_edt_classify(EngineDev D, EdtBox B, uint8_t* __restrict__ bits,
                                                      uint8_t* __restrict__ state) {
  __shared__ int32_t s_idx[7];
  __shared__ uint8_t s_cls[1000];
  const int t = threadIdx.x;
  const int cell = blockIdx.x;
  const int ci = cell % B.cbx, cj = (cell / B.cbx) % B.cby, ck = cell / (B.cbx * B.cby);
  if (t < 7) {
    int b[3] = {B.cx0 + ci, B.cy0 + cj, B.cz0 + ck};
    if (t) b[(t - 1) >> 1] += (t & 1) ? -1 : 1;  // 1 -x, 2 +x, 3 -y, 4 +y, 5 -z, 6 +z
    int32_t idx = -1;
    if (b[0] >= -32768 && b[0] <= 32767 && b[1] >= -32768 && b[1] <= 32767 && b[2] >= -32768 && b[2] <= 32767) {
      const int32_t e = find_local(D.table, (int16_t)b[0], (int16_t)b[1], (int16_t)b[2]);
      if (e >= 0) idx = D.table[e].z;
    }
    s_idx[t] = idx;
  }
  __syncthreads();
  const int32_t ib = s_idx[0];
  if (ib < 0 && !B.unknown) return;  // (the whole workgroup: no site, state stays 0, no pool read)
  if (ib >= 0) {
    const uint8_t* blk = D.pool + (size_t)ib * kBlockBytes;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int v = t + 256 * h;
      s_cls[cls_at(v & 7, (v >> 3) & 7, v >> 6)] = voxel_class(blk, v, B.min_weight);
    }
    for (int h = t; h < 384; h += 256) {
      const int f = h >> 6, a = h & 7, b = (h >> 3) & 7;
      const int far = (f & 1) ? 0 : 7, at = (f & 1) ? 8 : -1;  // the neighbour's layer, and where it goes
      const int axis = f >> 1;
      const int x = axis == 0 ? far : a, y = axis == 1 ? far : (axis == 0 ? a : b), z = axis == 2 ? far : b;
      const int hx = axis == 0 ? at : x, hy = axis == 1 ? at : y, hz = axis == 2 ? at : z;
      const int32_t in = s_idx[1 + f];
      uint8_t c = kUnobserved;
      if (in >= 0) c = voxel_class(D.pool + (size_t)in * kBlockBytes, x + 8 * y + 64 * z, B.min_weight);
      s_cls[cls_at(hx, hy, hz)] = c;
    }
    __syncthreads();
  }
  const int x = t & 7, y = (t >> 3) & 7;
  const int lx = (B.cx0 + ci) * kBlockLen + x - B.ox, ly = (B.cy0 + cj) * kBlockLen + y - B.oy;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int z = (t >> 6) + 4 * h;
    const int lz = (B.cz0 + ck) * kBlockLen + z - B.oz;
    const bool in_row = (unsigned)ly < (unsigned)B.ny && (unsigned)lz < (unsigned)B.nz;
    const bool in_box = in_row && (unsigned)lx < (unsigned)B.nx;
    uint8_t c = kUnobserved;
    bool site = B.unknown != 0;
    if (ib >= 0) {
      c = s_cls[cls_at(x, y, z)];
      const bool nfree = s_cls[cls_at(x - 1, y, z)] == kFree || s_cls[cls_at(x + 1, y, z)] == kFree ||
                         s_cls[cls_at(x, y - 1, z)] == kFree || s_cls[cls_at(x, y + 1, z)] == kFree ||
                         s_cls[cls_at(x, y, z - 1)] == kFree || s_cls[cls_at(x, y, z + 1)] == kFree;
      site = (c == kInside && nfree) || (B.unknown && c == kUnobserved);
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(site && in_box);
    const size_t row = (size_t)lz * B.ny + ly;
    if (in_row && x == 0) bits[row * B.rowbytes + ci] = (uint8_t)(m >> (threadIdx.x & 56));
    if (in_box && state && ib >= 0) state[row * B.nx + lx] = c;
  }
}

// Nearest site bit of the row at or before the voxel, and at or after it: the voxel's word masked, then
// whole words outward while they can still beat the best so far (at most R / 32 + 1 each way).
__global__ __launch_bounds__(256) void k_edt_x(EdtBox B, const uint32_t* __restrict__ bits, uint8_t* __restrict__ g) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (a box holds at most 2^28 voxels)
  if (i >= (uint32_t)(B.nx * B.ny * B.nz)) return;
  const uint32_t row = i / (uint32_t)B.nx;
  const int nw = B.rowbytes >> 2;
  const uint32_t* __restrict__ w = bits + (size_t)row * nw;
  const int X = (int)(i - row * B.nx) + (B.ox - B.cx0 * kBlockLen);  // the voxel's bit in the row
  int best = B.R;
  int wi = X >> 5;
  uint32_t m = w[wi] & (0xFFFFFFFFu >> (31 - (X & 31)));
  for (;;) {
    if (m) {
      best = min(best, X - (wi * 32 + 31 - __clz((int)m)));
      break;
    }
    if (--wi < 0 || X - (wi * 32 + 31) >= best) break;
    m = w[wi];
  }
  wi = X >> 5;
  m = w[wi] & (0xFFFFFFFFu << (X & 31));
  for (;;) {
    if (m) {
      best = min(best, wi * 32 + (__ffs((int)m) - 1) - X);
      break;
    }
    if (++wi >= nw || wi * 32 - X >= best) break;
    m = w[wi];
  }
  g[i] = (uint8_t)best;
}

// The windowed min-plus. Lane = line, so every global and LDS access of a wave is 64 consecutive
// elements. A wave takes the tile's outputs NT / 64 apart and walks k = 1, 2, ... outward from each. What
// is still to come at step k is at least m + k^2, m the least staged element of the lane's line, so the
// wave leaves as soon as m + k^2 reaches the best of each of its 64 lines: at once in empty space (m = cap),
// after a few steps near a surface, and never later than A, since in[j] + (i - j)^2 >= cap for
// |i - j| >= R. Elements outside the line are staged as cap, lanes beyond the last line as 0 (they never
// hold the wave back).
template <typename In, int ROWS, int NT>
__global__ __launch_bounds__(NT) void k_edt_line(EdtLine P, const In* __restrict__ in, uint16_t* __restrict__ out) {
  constexpr int NW = NT / 64;
  __shared__ uint16_t s[ROWS * 64];
  __shared__ uint16_t s_min[NW * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const bool live = c < P.ncol;
  const int i0 = blockIdx.y * P.T;
  const int nout = min(P.T, P.L - i0);
  const int rows = nout + 2 * P.A;
  const int64_t base = (int64_t)blockIdx.z * P.slab + c;
  uint32_t m = live ? P.cap : 0u;
  for (int r = wv; r < rows; r += NW) {
    const int j = i0 - P.A + r;
    uint32_t v = live ? P.cap : 0u;
    if (live && j >= 0 && j < P.L) {
      v = in[base + (int64_t)j * P.stride];
      if (sizeof(In) == 1) v = v * v;
    }
    s[r * 64 + lane] = (uint16_t)v;
    m = min(m, v);
  }
  s_min[wv * 64 + lane] = (uint16_t)m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) m = min(m, (uint32_t)s_min[w * 64 + lane]);
  for (int o = wv; o < nout; o += NW) {
    const uint16_t* q = s + (o + P.A) * 64 + lane;
    uint32_t best = q[0];
    for (int k = 1; k <= P.A; ++k) {
      const uint32_t kk = (uint32_t)(k * k);
      if (__builtin_amdgcn_ballot_w64(m + kk < best) == 0ull) break;
      best = min(best, min((uint32_t)q[-k * 64], (uint32_t)q[k * 64]) + kk);
    }
    if (live) out[base + (int64_t)(i0 + o) * P.stride] = (uint16_t)best;
  }
}

template __global__ void k_edt_line<uint8_t, kEdtRowsSmall, 256>(EdtLine, const uint8_t*, uint16_t*);
template __global__ void k_edt_line<uint16_t, kEdtRowsSmall, 256>(EdtLine, const uint16_t*, uint16_t*);
template __global__ void k_edt_line<uint8_t, kEdtRowsLarge, 1024>(EdtLine, const uint8_t*, uint16_t*);
template __global__ void k_edt_line<uint16_t, kEdtRowsLarge, 1024>(EdtLine, const uint16_t*, uint16_t*);

}  // namespace tsdf
