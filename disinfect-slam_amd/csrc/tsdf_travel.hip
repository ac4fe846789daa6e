// tsdf_travel.hip -- travel field over the box of a distance field (DESIGN.md "Travel field"): tile-wise
// label correcting over 8^3 tiles. k_travel_seed writes the seeds and lists their tiles and the tiles they
// face; each k_travel_round relaxes the listed tiles in LDS until nothing in them changes and lists the
// neighbour tiles whose facing voxels changed for the next round; k_travel_paths walks back from targets.
// All integers. Every value ever stored in cost is the cost of a real path from a seed and values only
// decrease, so the field the rounds end with -- the least fixed point -- does not depend on the order of
// workgroups or atomics. The kernels do not touch the volume.
#include "tsdf_travel.h"

namespace tsdf {

namespace {
// a tile's stamp raised to round r: true for the one caller that lists it for that round
__device__ __forceinline__ void travel_list(const TravelArgs& A, uint32_t tile, uint32_t r) {
  if (atomicMax(&A.stamp[tile], r) < r) A.list[r & 1][atomicAdd(&A.ctl->count[r % 3], 1u)] = tile;
}
// cell (a, b, c) in [-1, 8]^3 of the staged costs
__device__ __forceinline__ int cell_at(int a, int b, int c) { return (a + 1) + 10 * (b + 1) + 100 * (c + 1); }
}  // namespace

__global__ __launch_bounds__(256) void k_travel_seed(TravelArgs A, const int32_t* __restrict__ seeds, int S) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= S) return;
  const int x = seeds[3 * (size_t)i], y = seeds[3 * (size_t)i + 1], z = seeds[3 * (size_t)i + 2];
  if ((unsigned)x >= (unsigned)A.nx || (unsigned)y >= (unsigned)A.ny || (unsigned)z >= (unsigned)A.nz) return;
  const size_t v = ((size_t)z * A.ny + y) * A.nx + x;
  if (!travel_passable(A.d2[v], A.state[v], A.clearance2, A.unknown_free)) return;
  A.cost[v] = 0;  // (duplicates store the same value)
  atomicAdd(&A.ctl->seeded, 1u);
  // Its tile and the up to seven tiles it faces (the rounds' rule: {0, sx} x {0, sy} x {0, sz}): a round
  // wakes neighbours only for voxels it lowered, and no round lowers a seed, so a seed on a tile's border
  // has to list the tiles that stage it in their halo itself.
  const int ti = x >> kTravelTileBits, tj = y >> kTravelTileBits, tk = z >> kTravelTileBits;
  const int lx = x & (kTravelTile - 1), ly = y & (kTravelTile - 1), lz = z & (kTravelTile - 1);
  const int sx = lx == 0 ? -1 : (lx == kTravelTile - 1 ? 1 : 0), sy = ly == 0 ? -1 : (ly == kTravelTile - 1 ? 1 : 0),
            sz = lz == 0 ? -1 : (lz == kTravelTile - 1 ? 1 : 0);
  for (int q = 0; q < 8; ++q) {
    const int ax = (q & 1) ? sx : 0, ay = (q & 2) ? sy : 0, az = (q & 4) ? sz : 0;
    if (q && !(ax | ay | az)) continue;  // (q > 0 that names the seed's own tile again)
    const int a = ti + ax, b = tj + ay, d = tk + az;
    if ((unsigned)a < (unsigned)A.tx && (unsigned)b < (unsigned)A.ty && (unsigned)d < (unsigned)A.tz)
      travel_list(A, (uint32_t)((d * A.ty + b) * A.tx + a), 1u);
  }
}

// One voxel per lane. The tile's costs and a one-voxel halo (10^3 words) are staged in LDS; a halo cell
// outside the box, like an impassable voxel anywhere, holds UNREACHED and offers no step. Inside the tile
// the sweeps are Jacobi: every lane reads its 26 neighbours, a barrier, the lanes that improved store, a
// barrier. Another tile of the same round may be writing the halo's voxels while they are staged: either
// value is the cost of a real path, and a tile that changed a facing voxel lists this one for the next
// round, which then stages the final values.
__global__ __launch_bounds__(512) void k_travel_round(TravelArgs A, uint32_t r) {
  __shared__ uint32_t s_c[1000];
  __shared__ uint32_t s_wake[27];
  const int t = threadIdx.x;
  const uint32_t count = A.ctl->count[r % 3];
  if (blockIdx.x == 0 && t == 0) {
    A.ctl->count[(r + 2) % 3] = 0;
    if (count) A.ctl->rounds = r;
  }
  if (count == 0) return;  // (uniform: converged, or no seed)
  const uint32_t* __restrict__ list = A.list[r & 1];
  const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
  const int me = cell_at(lx, ly, lz);
  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t tile = list[i];
    const int ti = (int)(tile % (uint32_t)A.tx), tj = (int)(tile / (uint32_t)A.tx % (uint32_t)A.ty),
              tk = (int)(tile / (uint32_t)(A.tx * A.ty));
    const int x0 = ti << kTravelTileBits, y0 = tj << kTravelTileBits, z0 = tk << kTravelTileBits;
    if (t < 27) s_wake[t] = 0;
    for (int h = t; h < 1000; h += 512) {
      const int x = x0 + h % 10 - 1, y = y0 + h / 10 % 10 - 1, z = z0 + h / 100 - 1;
      const bool in = (unsigned)x < (unsigned)A.nx && (unsigned)y < (unsigned)A.ny && (unsigned)z < (unsigned)A.nz;
      s_c[h] = in ? A.cost[((size_t)z * A.ny + y) * A.nx + x] : kTravelUnreached;
    }
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    const bool in = x < A.nx && y < A.ny && z < A.nz;
    const size_t v = ((size_t)z * A.ny + y) * A.nx + x;
    const bool pass = in && travel_passable(A.d2[v], A.state[v], A.clearance2, A.unknown_free);
    __syncthreads();
    const uint32_t c0 = s_c[me];
    uint32_t c = c0;
    for (;;) {
      uint32_t m = c;
      if (pass) {
        // the least neighbour of each step length; UNREACHED + w would wrap, so the test comes first
        uint32_t m3 = kTravelUnreached, m4 = kTravelUnreached, m5 = kTravelUnreached;
#pragma unroll
        for (int k = 0; k < 27; ++k) {
          const int dx = k % 3 - 1, dy = k / 3 % 3 - 1, dz = k / 9 - 1;
          const int w = (dx != 0) + (dy != 0) + (dz != 0);
          if (w == 0) continue;
          const uint32_t n = s_c[me + dx + 10 * dy + 100 * dz];
          if (w == 1) m3 = min(m3, n);
          if (w == 2) m4 = min(m4, n);
          if (w == 3) m5 = min(m5, n);
        }
        if (m3 != kTravelUnreached) m = min(m, m3 + 3u);
        if (m4 != kTravelUnreached) m = min(m, m4 + 4u);
        if (m5 != kTravelUnreached) m = min(m, m5 + 5u);
      }
      const bool better = m < c;
      if (!__syncthreads_or(better)) break;  // (every lane has read its neighbours)
      if (better) s_c[me] = c = m;
      __syncthreads();
    }
    if (c < c0) {
      A.cost[v] = c;
      const int sx = lx == 0 ? -1 : (lx == 7 ? 1 : 0), sy = ly == 0 ? -1 : (ly == 7 ? 1 : 0),
                sz = lz == 0 ? -1 : (lz == 7 ? 1 : 0);
      // the tiles this voxel faces: every non-zero choice of {0, sx} x {0, sy} x {0, sz}
      for (int q = 1; q < 8; ++q) {
        const int ax = (q & 1) ? sx : 0, ay = (q & 2) ? sy : 0, az = (q & 4) ? sz : 0;
        if (ax | ay | az) s_wake[(ax + 1) + 3 * (ay + 1) + 9 * (az + 1)] = 1;
      }
    }
    __syncthreads();
    if (t < 27 && s_wake[t]) {
      const int a = ti + t % 3 - 1, b = tj + t / 3 % 3 - 1, d = tk + t / 9 - 1;
      if ((unsigned)a < (unsigned)A.tx && (unsigned)b < (unsigned)A.ty && (unsigned)d < (unsigned)A.tz)
        travel_list(A, (uint32_t)((d * A.ty + b) * A.tx + a), r + 1u);
    }
    __syncthreads();  // (s_c and s_wake are the next tile's)
  }
}

__global__ __launch_bounds__(64) void k_travel_paths(const uint32_t* __restrict__ cost, int nx, int ny, int nz,
                                                     const int32_t* __restrict__ targets, int T, int32_t max_len,
                                                     int32_t* __restrict__ path, int32_t* __restrict__ len) {
  const int t = (int)(blockIdx.x * 64u + threadIdx.x);
  if (t >= T) return;
  len[t] = travel_walk(cost, nx, ny, nz, targets[3 * (size_t)t], targets[3 * (size_t)t + 1], targets[3 * (size_t)t + 2],
                       max_len, path + (size_t)t * (size_t)max_len);
}

}  // namespace tsdf
