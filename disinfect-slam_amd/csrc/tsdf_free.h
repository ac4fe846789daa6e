// tsdf_free.h -- the observed-free-space layer's kernels and what they share with their host side
// (tsdf_free.hip, tsdf_host_free.hip; DESIGN.md "Observed free space"). Not part of tsdf_kernels.h: no other
// file needs it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsdf_device.h"

namespace tsdf {

// a workgroup's brick of the layer's box: 64 x 8 x 8 voxels, a wave per x row of 64 (two words of the layer)
constexpr int kFreeBrickX = 64, kFreeBrickY = 8, kFreeBrickZ = 8;
// The radius of a brick's bounding sphere in voxels: half its diagonal, sqrt(31.5^2 + 3.5^2 + 3.5^2) = 31.89,
// grown by one voxel and rounded up.
constexpr float kFreeBrickRadius = 33.0f;
// the launch grid of a workgroup per brick over a box (host side)
inline dim3 free_brick_grid(int nx, int ny, int nz) {
  return dim3((unsigned)((nx + kFreeBrickX - 1) / kFreeBrickX), (unsigned)((ny + kFreeBrickY - 1) / kFreeBrickY),
              (unsigned)((nz + kFreeBrickZ - 1) / kFreeBrickZ));
}
// state bytes a lane of k_free_apply takes, 256 apart
constexpr int kFreeApplyChunk = 16;

// one pixel of the frame as the per-voxel pass gathers it: the depth, 0 where the update would skip the
// pixel (d == 0 || d > max_depth), and img_depth_to_range_ of the pixel
struct alignas(8) FreePix {
  float d, range;
};

struct FreeArgs {
  int ox, oy, oz;  // the layer's box (global voxels)
  int nx, ny, nz;
  int wx;          // words per x row
  int W, H;
  float fx, fy, cx, cy;
  quatf cq;  // cam_T_world
  f3 ct;
  float voxel, trunc, max_depth;
  int cull_words;   // skip words whose in-range bits are all set
  int cull_bricks;  // skip bricks outside the frustum (the host clears it for a cam_T_world that is no rotation)
  uint32_t* bits;
  const FreePix* pix;
};

struct FreeApplyArgs {
  int nx, ny, nz;     // the state array's box
  int dx, dy, dz;     // its origin minus the layer's
  int lx, ly, lz, wx; // the layer's dims and words per row
  const uint32_t* bits;
  uint8_t* state;
  unsigned long long* promoted;
};

// one lane per pixel: its FreePix record
__global__ void k_free_pixels(const float* depth, int W, int H, float ifx, float ify, float icx, float icy,
                              float max_depth, FreePix* pix);
// bits |= free(., frame) over the box: a 256-thread workgroup per brick
__global__ void k_free_observe(FreeArgs A);
// one lane per state byte, kFreeApplyChunk bytes in turn: 0 -> 1 where the layer's bit is set; *promoted += the
// number changed, once per workgroup
__global__ void k_free_apply(FreeApplyArgs A);

}  // namespace tsdf
