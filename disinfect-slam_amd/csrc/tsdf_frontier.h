// tsdf_frontier.h -- the frontier mask's and the connected components' kernels and what they share with their
// host side (tsdf_frontier.hip, tsdf_host_frontier.hip; DESIGN.md "Frontiers and components"). Not part of
// tsdf_kernels.h: no other file needs it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsdf {

constexpr uint32_t kCcNone = 0xFFFFFFFFu;       // TSDF_COMPONENT_NONE
constexpr uint32_t kCcUnreached = 0xFFFFFFFFu;  // TSDF_TRAVEL_UNREACHED
// the box's cover by 8^3 tiles from its first voxel (the travel field's cover, restated); a workgroup is
// 512 lanes, lane t the tile's voxel (t & 7, (t >> 3) & 7, t >> 6): a wave is one z slice
constexpr int kCcTileBits = 3, kCcTile = 1 << kCcTileBits, kCcTileVox = kCcTile * kCcTile * kCcTile;
// Members of one 2 x 2 x 2 cell are pairwise adjacent, so a tile meets at most 4^3 components. The statistics'
// LDS table holds twice as many keys, which keeps its probe sequences short.
constexpr int kCcTileRoots = 64, kCcHash = 2 * kCcTileRoots;
// Accumulators per component: a tile folds into the one its index chooses, so the thousands of tiles of one
// large component spread their atomics over this many cache lines (and L2 channels) instead of one.
constexpr int kCcReplicas = 8;

// the control words of a tsdf_frontier_mark or tsdf_components call
struct CcCtl {
  unsigned long long marked;  // k_frontier_mark: ones written
  uint32_t total;             // k_cc_flatten: components (each root took one slot)
  uint32_t count;             // k_cc_emit: records with size >= min_size
  uint32_t pad[4];
};

// A component's accumulator. Every field starts as 0 (one memset) and is folded with an atomic whose identity
// is 0: the least coordinates and the goal are kept complemented, under atomicMax. A component owns
// kCcReplicas of them in a row; k_cc_emit folds the row into a tsdf_component of the same 64 bytes.
struct CcAcc {
  uint32_t label;
  uint32_t size;
  uint32_t hi[3];
  uint32_t nlo[3];          // max of ~coordinate
  unsigned long long sum[3];
  unsigned long long ngoal; // max of ~((key << 32) | index)
};
static_assert(sizeof(CcAcc) == 64, "CcAcc is a tsdf_component's size");
// tsdf_component, field for field (the host side asserts it)
struct CcRec {
  uint32_t label, size;
  int32_t lo[3], hi[3];
  long long sum[3];
  uint32_t goal, goal_key;
};

struct CcArgs {
  int nx, ny, nz;  // the box
  int tx, ty, tz;  // its tiles
  const uint8_t* mask;
  const uint32_t* key;  // or null
  uint32_t* label;
  uint32_t* slot;  // per voxel, read at roots only: the root's row of accumulators
  CcAcc* acc;      // kCcReplicas per slot
  CcCtl* ctl;
};

struct FrontierArgs {
  int nx, ny, nz;
  const uint8_t* state;
  const uint32_t* cost;  // or null
  uint8_t* mask;
  CcCtl* ctl;  // or null: no count
};

// a workgroup per tile: mask[v] for its voxels; ctl->marked += the ones, once per workgroup that has any
__global__ void k_frontier_mark(FrontierArgs A);
// a workgroup per tile: label[v] = the least member of v's component within the tile, kCcNone off the mask
__global__ void k_cc_local(CcArgs A);
// a lane per voxel: members on a tile face joined with their members in other tiles (union-find, atomicMin)
__global__ void k_cc_merge(CcArgs A);
// a lane per voxel: label[v] = its root; every root takes the next accumulator: slot[root] = ctl->total++
__global__ void k_cc_flatten(CcArgs A);
// a workgroup per tile: its members folded per distinct root in LDS, one update per root into acc
__global__ void k_cc_stats(CcArgs A);
// a lane per component: its accumulators folded; those with size >= min_size appended to out, ctl->count of them
__global__ void k_cc_emit(CcArgs A, uint32_t total, uint32_t min_size, CcRec* out);

}  // namespace tsdf
