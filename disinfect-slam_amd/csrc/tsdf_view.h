// tsdf_view.h -- the view-gain kernels and what they share with their host side (tsdf_view.hip,
// tsdf_host_view.hip; DESIGN.md "View gain"). Not part of tsdf_kernels.h: no other file needs it. The brick
// shape, its radius and the pixel record are the free layer's (tsdf_free.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tsdf_device.h"
#include "tsdf_free.h"

namespace tsdf {

// views a launch pair takes at most: k_view_gain's counters in LDS, one thread per view for the brick cull
constexpr int kViewBatch = 64;
// and pixel records a batch holds at most (8 bytes each): batch = min(kViewBatch, max(1, this / (W * H)))
constexpr int64_t kViewBatchPixels = (int64_t)1 << 22;
// The march skips samples only while every coordinate it bounds stays below this many voxels: the float error
// of a sample's position is then a small fraction of a voxel (about 10 roundings of 2^-24 relative each:
// under 0.2 voxels at 2^18), well inside kViewSlack. 2^18 voxels is the extent of the int16 block range.
constexpr float kViewSkipExtent = 262144.0f;
// voxels the box grows by before the ray is cut against it: half a voxel of rounding, the error above, spare
constexpr float kViewSlack = 3.0f;

// one candidate view on the device (64 bytes): cam_T_world, world_T_cam as make_params derives it, the
// largest predicted depth as the bits of a non-negative float (k_view_depth raises it with atomicMax: the
// order of non-negative floats is that of their bits) and whether the pose is a rigid motion (brick cull)
struct alignas(16) ViewCam {
  quatf cq;
  f3 ct;
  uint32_t dmax_bits;
  quatf wq;
  f3 wt;
  int rigid;
};

struct ViewDepthArgs {
  int ox, oy, oz;  // the box of `state` (global voxels)
  int nx, ny, nz;
  int W, H;
  float ifx, ify, icx, icy;
  float voxel, inv_voxel;  // inv_voxel = RN(1 / voxel) on the host (quot_const)
  float step, miss;
  int J;     // samples 1 .. J
  int skip;  // cut every ray against the box first (0: the plain march)
  const uint8_t* state;
  ViewCam* cam;      // the batch's views; grid y is the view
  FreePix* pix;      // W * H records per view
  float* depth_out;  // W * H floats per view, or NULL
};

struct ViewGainArgs {
  int ox, oy, oz;
  int nx, ny, nz;
  int wx;  // words per x row of `seen`
  int W, H;
  float fx, fy, cx, cy;
  float voxel, margin;
  int nv;    // views of the batch, at most kViewBatch
  int cull;  // skip (brick, view) pairs outside the view's frustum or beyond its largest depth
  const uint8_t* state;
  const uint32_t* seen;  // or NULL
  const ViewCam* cam;
  const FreePix* pix;
  unsigned long long* gain;  // one per view of the batch
};

// one lane per pixel, grid y the view: the first sample of the ray in a state-2 voxel of the box
__global__ void k_view_depth(ViewDepthArgs A);
// gain[i] += #{unobserved, unseen voxels of the brick that view i sees}: a 256-thread workgroup per brick
__global__ void k_view_gain(ViewGainArgs A);

}  // namespace tsdf
