// tsdf_free.hip -- observed free space (DESIGN.md "Observed free space"): a bit per voxel of a box, set when a
// depth frame saw the voxel as free by the voxel update's own test, whether or not the voxel's block exists.
// k_free_pixels turns the frame into {depth or 0, range} records; k_free_observe is a gather, one lane per
// voxel, a wave per x row of 64 voxels whose ballot is two words of the layer; k_free_apply promotes a
// distance field's state from 0 to 1 where the bit is set. Every word of the layer is written by one wave
// only and launches are ordered by the stream: plain loads and stores, no atomics on the layer. The kernels
// do not touch the volume.
#include "tsdf_free.h"

namespace tsdf {

__global__ __launch_bounds__(256) void k_free_pixels(const float* __restrict__ depth, int W, int H, float ifx,
                                                     float ify, float icx, float icy, float max_depth,
                                                     FreePix* __restrict__ pix) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  const float d = depth[i];
  const f3 pc = pixel_ray(ifx, ify, icx, icy, x, y);
  FreePix p;
  p.d = (d == 0 || d > max_depth) ? 0.0f : d;  // (a NaN depth stays: its sdf is NaN, which is not free)
  p.range = sqrtf(dot3(pc, pc));               // img_depth_to_range_ (block_allocate_kernel)
  pix[i] = p;
}

namespace {
// A brick no voxel of which can be free in this frame. c: the centre of the brick in camera space; every
// voxel lies within r of it (kFreeBrickRadius: one voxel of slack). Free needs 0 < hz < d <= max_depth and
// a rounded pixel inside the image, i.e. the quotients hx / hz in [-1/2, W - 1/2) and hy / hz in
// [-1/2, H - 1/2); the planes below are those of the image grown by one pixel. A NaN anywhere makes every
// comparison false: no cull.
__device__ __forceinline__ bool brick_culled(const FreeArgs& A, int x0, int y0, int z0) {
  const f3 cw = {((float)(A.ox + x0) + 31.5f) * A.voxel, ((float)(A.oy + y0) + 3.5f) * A.voxel,
                 ((float)(A.oz + z0) + 3.5f) * A.voxel};
  const f3 c = se3_apply(A.cq, A.ct, cw);
  const float r = kFreeBrickRadius * fabsf(A.voxel);
  if (c.z + r <= 0.0f) return true;          // behind the camera plane
  if (c.z - r >= A.max_depth) return true;   // beyond every valid depth
  // hx / hz >= -3/2 for hz > 0: fx x + (cx + 3/2) z >= 0; the sphere lies on the other side
  const float l = A.cx + 1.5f, rt = A.cx - ((float)A.W + 0.5f);
  const float t = A.cy + 1.5f, b = A.cy - ((float)A.H + 0.5f);
  if (A.fx * c.x + l * c.z < -r * sqrtf(A.fx * A.fx + l * l)) return true;
  if (A.fx * c.x + rt * c.z > r * sqrtf(A.fx * A.fx + rt * rt)) return true;
  if (A.fy * c.y + t * c.z < -r * sqrtf(A.fy * A.fy + t * t)) return true;
  if (A.fy * c.y + b * c.z > r * sqrtf(A.fy * A.fy + b * b)) return true;
  return false;
}
}  // namespace

__global__ __launch_bounds__(256) void k_free_observe(FreeArgs A) {
  const int x0 = (int)blockIdx.x * kFreeBrickX, y0 = (int)blockIdx.y * kFreeBrickY, z0 = (int)blockIdx.z * kFreeBrickZ;
  if (A.cull_bricks && brick_culled(A, x0, y0, z0)) return;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int x = x0 + lane;
  const int wi = x >> 5;  // the lane's word of its row
  const bool has_word = wi < A.wx;
  // the bits of that word inside the box: the padding of a row's last word is never set
  const int left = A.nx - (wi << 5);
  const uint32_t in_range = !has_word ? 0u : (left >= 32 ? 0xFFFFFFFFu : ((1u << left) - 1u));
  const float gx = (float)(A.ox + x) * A.voxel;
  for (int row = wave; row < kFreeBrickY * kFreeBrickZ; row += 4) {
    const int y = y0 + (row & (kFreeBrickY - 1)), z = z0 + (row >> 3);
    if (y >= A.ny || z >= A.nz) continue;  // (wave-uniform)
    uint32_t* word = A.bits + ((size_t)z * A.ny + y) * A.wx + wi;
    const uint32_t cur = has_word ? *word : 0u;
    bool is_free = false;
    const bool todo = x < A.nx && !(A.cull_words && (cur & in_range) == in_range);
    if (todo) {
      const f3 pw = {gx, (float)(A.oy + y) * A.voxel, (float)(A.oz + z) * A.voxel};
      const f3 pc = se3_apply(A.cq, A.ct, pw);
      const float hx = A.fx * pc.x + A.cx * pc.z;
      const float hy = A.fy * pc.y + A.cy * pc.z;
      const float hz = pc.z;
      const float rz = __builtin_amdgcn_rcpf(hz);
      const int u = round_quot_i(hx, hz, rz);  // f2i(roundf(hx / hz)), exactly
      const int v = round_quot_i(hy, hz, rz);
      if (u >= 0 && u < A.W && v >= 0 && v < A.H) {
        const FreePix p = A.pix[v * A.W + u];
        const float sdf = p.range * (p.d - hz);
        is_free = p.d != 0.0f && sdf >= A.trunc && hz > 0.0f;
      }
    }
    const unsigned long long m = __ballot(is_free);
    const uint32_t mine = (uint32_t)(lane < 32 ? m : m >> 32);
    const uint32_t now = cur | mine;
    if ((lane & 31) == 0 && has_word && now != cur) *word = now;
  }
}

__global__ __launch_bounds__(256) void k_free_apply(FreeApplyArgs A) {
  // a workgroup takes kFreeApplyChunk runs of 256 consecutive bytes and counts them into the device word
  // once: one atomic per wave of 64 bytes took 2.6 ms for a 400^3 box, against 0.14 ms uncounted
  __shared__ uint32_t wg_count;
  if (threadIdx.x == 0) wg_count = 0;
  const int n = A.nx * A.ny * A.nz;  // (at most 2^28)
  const int base = (int)blockIdx.x * (256 * kFreeApplyChunk) + (int)threadIdx.x;
  uint32_t count = 0;  // wave-uniform
  for (int k = 0; k < kFreeApplyChunk; ++k) {
    const int i = base + k * 256;
    bool hit = false;
    if (i < n) {
      const int row = i / A.nx;
      const int x = i - row * A.nx, z = row / A.ny, y = row - z * A.ny;
      const int a = x + A.dx, b = y + A.dy, c = z + A.dz;  // the voxel in the layer's box
      if ((unsigned)a < (unsigned)A.lx && (unsigned)b < (unsigned)A.ly && (unsigned)c < (unsigned)A.lz) {
        const uint32_t w = A.bits[((size_t)c * A.ly + b) * A.wx + (a >> 5)];
        if (((w >> (a & 31)) & 1u) && A.state[i] == 0) {
          A.state[i] = 1;
          hit = true;
        }
      }
    }
    count += (uint32_t)__popcll(__ballot(hit));
  }
  if (!A.promoted) return;
  __syncthreads();
  if (count && ((int)threadIdx.x & 63) == 0) atomicAdd(&wg_count, count);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count) atomicAdd(A.promoted, (unsigned long long)wg_count);
}

}  // namespace tsdf
