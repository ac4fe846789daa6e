// tsdf_travel.h -- the travel field's kernels and what they share with their host side (tsdf_travel.hip,
// tsdf_host_travel.hip; DESIGN.md "Travel field"). Not part of tsdf_kernels.h: no other file needs it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsdf {

constexpr uint32_t kTravelUnreached = 0xFFFFFFFFu;
// the box's cover by 8^3 tiles (k_edt_classify's, from the box's first voxel)
constexpr int kTravelTileBits = 3, kTravelTile = 1 << kTravelTileBits;
// workgroups of a round: a fixed grid that strides over the device-side tile count
constexpr int kTravelGrid = 1024;

// What the rounds leave for each other and for the host. Round r (from 1) reads count[r % 3] tiles of
// list[r & 1], appends to list[(r + 1) & 1] under count[(r + 1) % 3] and clears count[(r + 2) % 3], the
// count of round r - 1 that round r + 1 appends under. A round that finds its count 0 has nothing to do,
// and neither has any after it.
struct TravelCtl {
  uint32_t count[3];
  uint32_t rounds;  // the last round that had tiles
  uint32_t seeded;  // seeds used
  uint32_t pad[3];
};

struct TravelArgs {
  int nx, ny, nz;  // the box
  int tx, ty, tz;  // its tiles
  int clearance2, unknown_free;
  const uint16_t* d2;
  const uint8_t* state;
  uint32_t* cost;
  uint32_t* stamp;  // per tile: the last round it was listed for
  uint32_t* list[2];
  TravelCtl* ctl;
};

__host__ __device__ inline bool travel_passable(uint16_t d2, uint8_t state, int clearance2, int unknown_free) {
  return (int)d2 >= clearance2 && (state == 1 || (unknown_free && state == 0));
}

// one lane per seed, over a cost field of TSDF_TRAVEL_UNREACHED: cost 0 at a seed inside the box and passable,
// its tile and the tiles it faces listed for round 1
__global__ void k_travel_seed(TravelArgs A, const int32_t* seeds, int S);
// round r: every listed tile relaxed in LDS until nothing in it changes, written back if it changed, the
// neighbour tiles whose facing voxels changed listed for round r + 1
__global__ void k_travel_round(TravelArgs A, uint32_t r);

// One walk of tsdf_travel_paths (the contract's rule), on the host for a host field and one lane per target
// on the device: the same code, so the same paths. Returns len; writes at most max_len indices.
__host__ __device__ inline int32_t travel_walk(const uint32_t* cost, int nx, int ny, int nz, int x, int y, int z,
                                               int32_t max_len, int32_t* path) {
  if ((unsigned)x >= (unsigned)nx || (unsigned)y >= (unsigned)ny || (unsigned)z >= (unsigned)nz) return 0;
  uint32_t c = cost[((size_t)z * ny + y) * nx + x];
  if (c == kTravelUnreached) return 0;
  int32_t n = 0;
  for (;;) {
    if (n < max_len) path[n] = (int32_t)(((size_t)z * ny + y) * nx + x);
    ++n;
    if (c == 0) return n;
    bool found = false;
    for (int k = 0; k < 27 && !found; ++k) {
      const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
      if (k == 13) continue;
      const int a = x + dx, b = y + dy, d = z + dz;
      if ((unsigned)a >= (unsigned)nx || (unsigned)b >= (unsigned)ny || (unsigned)d >= (unsigned)nz) continue;
      const uint32_t cn = cost[((size_t)d * ny + b) * nx + a];
      const uint32_t w = 2u + (uint32_t)(dx != 0) + (uint32_t)(dy != 0) + (uint32_t)(dz != 0);
      // (in 64 bits: cn < c, so the costs of a walk strictly decrease and it ends on any input)
      if (cn != kTravelUnreached && (uint64_t)cn + w == (uint64_t)c) {
        x = a, y = b, z = d, c = cn;
        found = true;
      }
    }
    if (!found) return -n;
  }
}

// one lane per target: len[t] and the first max_len voxels of its walk
__global__ void k_travel_paths(const uint32_t* cost, int nx, int ny, int nz, const int32_t* targets, int T,
                               int32_t max_len, int32_t* path, int32_t* len);

}  // namespace tsdf
