// tsdf_box.h -- what the box calls share (DESIGN.md "Box calls"): the limits of a box of voxels outside the
// hash, its counters, the rigid-pose rule and the carve-up of a scratch buffer into sections. Plain C++ with
// no HIP in it, so host/tests/box_host_main.cc compiles it alone (tests/test_box_cpu.py); tsdf_host.h includes
// it for the host files and pins its constants to the public header's and the kernels'.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tsdf {

// TSDF_BOX_MAX_DIM and TSDF_BOX_MAX_VOXELS (include/disinfect_tsdf.h; tsdf_host.h asserts they are these)
constexpr int kBoxMaxDim = 2048;
constexpr int64_t kBoxMaxVoxels = (int64_t)1 << 28;
// voxels per block edge as a shift: kBlockLenBits (tsdf_host.h asserts it)
constexpr int kBoxBlockBits = 3;

// every axis 1..kBoxMaxDim and at most kBoxMaxVoxels voxels in all
inline bool box_dims_ok(const int32_t* dims) {
  int64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1 || dims[a] > kBoxMaxDim) return false;
    n *= dims[a];
  }
  return n <= kBoxMaxVoxels;
}
// every voxel of the box, grown by `grow` voxels on each side, in a block of the int16 block range
inline bool box_in_block_range(const int32_t* origin, const int32_t* dims, int grow) {
  for (int a = 0; a < 3; ++a) {
    const int64_t lo = ((int64_t)origin[a] - grow) >> kBoxBlockBits;
    const int64_t hi = ((int64_t)origin[a] + dims[a] - 1 + grow) >> kBoxBlockBits;
    if (lo < -32768 || hi > 32767) return false;
  }
  return true;
}
inline size_t box_voxels(const int32_t* dims) { return (size_t)dims[0] * (size_t)dims[1] * (size_t)dims[2]; }
// the words of a bit layer over the box: nz * ny * ceil(nx / 32)
inline int64_t box_words(const int32_t* dims) { return (int64_t)dims[2] * dims[1] * ((dims[0] + 31) >> 5); }
// tiles of 2^bits voxels that cover n voxels along an axis
inline int box_tiles(int n, int bits) { return (n + (1 << bits) - 1) >> bits; }

// Whether a pose's quaternion (x, y, z, w) makes it a rigid motion for the brick culls. For q = s u with u a
// unit quaternion the rotation formula gives (1 - s^2) v + s^2 R v, so with |s^2 - 1| <= 2^-10 it stretches no
// length by more than 1 + 2^-9, far inside a brick sphere's slack.
inline bool pose_is_rigid(const float* q) {
  const double n2 = (double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3];
  const double d = n2 - 1.0;
  return (d < 0 ? -d : d) <= 0x1p-10;
}

// sections of a scratch buffer are 16-byte aligned
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// The carve-up of one scratch buffer. A call declares its sections once, in order, each with its byte size
// (add returns the section's handle), asks for total(), makes room for that once and resolves each handle
// against the buffer's base (at). Two rules hold, and calls rely on them:
//  - sections are contiguous in declaration order: a section ends where the next one starts, so two neighbours
//    can be cleared or copied as one range (tsdf_travel_field clears its control words and stamps so);
//  - every section starts on a 16-byte boundary of the buffer: a size is rounded up to 16, and a size of 0
//    takes no room (the section then starts where the next one does).
// keep(k) forgets every section after the first k: a call whose trailing sizes change declares them again
// (tsdf_components), and the leading offsets stay as they were. A call may declare kMax sections (the largest,
// tsdf_travel_field, has eight); one more is refused: add writes nothing and returns -1, which at resolves to
// null, so a call that outgrows kMax faults on its first run instead of overlapping its neighbours.
struct Sections {
  static constexpr int kMax = 12;
  size_t off[kMax + 1] = {0};
  int n = 0;
  int add(size_t bytes) {
    if (n == kMax) return -1;
    off[n + 1] = off[n] + up16(bytes);
    return n++;
  }
  void keep(int k) { n = k; }
  size_t total() const { return off[n]; }
  size_t offset(int h) const { return off[h]; }
  size_t size(int h) const { return off[h + 1] - off[h]; }  // rounded
  template <typename T>
  T* at(void* base, int h) const {
    return h < 0 ? nullptr : reinterpret_cast<T*>(static_cast<unsigned char*>(base) + off[h]);
  }
};

}  // namespace tsdf
