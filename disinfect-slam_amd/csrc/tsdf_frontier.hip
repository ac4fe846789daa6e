// tsdf_frontier.hip -- frontier mask and connected components of a voxel mask (DESIGN.md "Frontiers and
// components"). k_frontier_mark: observed-free, reachable voxels that touch unobserved space. Components, 26-
// connected, labelled by their least linear index: k_cc_local labels each 8^3 tile in LDS, k_cc_merge joins
// the tiles with a union-find over the label array (atomicMin: every store keeps label[x] <= x inside x's
// component, so a component's final root is its least member whatever the order of the atomics), k_cc_flatten
// points every member at its root and numbers the roots, k_cc_stats folds size, sums, bounding box and goal
// per distinct root inside a workgroup before one update per root leaves it for one of the component's
// accumulators, k_cc_emit folds those and filters by size.
// Integers only; plain vector stores and HIP atomics. The kernels do not touch the volume.
#include "tsdf_frontier.h"

namespace tsdf {

namespace {

__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The root of member x. label[y] <= y for every member y, so the walk strictly descends and ends; the guard
// p >= x also ends it on an array that broke that rule.
__device__ __forceinline__ uint32_t cc_find(const uint32_t* label, uint32_t x) {
  for (;;) {
    const uint32_t p = cc_load(label + x);
    if (p >= x) return x;
    x = p;
  }
}
// Joins the components of members a and b: the greater root goes under the lesser. When another lane moved
// the greater root first, the atomic's return value is where it went: that value and the lesser root are
// joined instead. a + b strictly decreases from try to try.
__device__ __forceinline__ void cc_union(uint32_t* label, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(label, a);
    b = cc_find(label, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b, b = t;
    }
    const uint32_t old = atomicMin(label + a, b);
    if (old == a) return;
    a = old;
  }
}

struct CcTile {
  int x, y, z;  // the lane's voxel
  bool in;      // inside the box
  size_t v;     // its linear index (when in)
};
__device__ __forceinline__ CcTile cc_tile(int nx, int ny, int nz, int tx, int ty) {
  const int t = (int)threadIdx.x;
  const int b = (int)blockIdx.x, bi = b % tx, bj = (b / tx) % ty, bk = b / (tx * ty);
  CcTile T;
  T.x = (bi << kCcTileBits) + (t & 7), T.y = (bj << kCcTileBits) + ((t >> 3) & 7), T.z = (bk << kCcTileBits) + (t >> 6);
  T.in = T.x < nx && T.y < ny && T.z < nz;
  T.v = ((size_t)T.z * ny + T.y) * nx + T.x;
  return T;
}

// one component's worth of a lane's, a wave's or a tile's members (0 is the identity of every field) into an
// accumulator
__device__ __forceinline__ void cc_fold_global(CcAcc* a, uint32_t root, uint32_t size, unsigned long long sx,
                                               unsigned long long sy, unsigned long long sz, uint32_t hx, uint32_t hy,
                                               uint32_t hz, uint32_t nlx, uint32_t nly, uint32_t nlz,
                                               unsigned long long ngoal) {
  a->label = root;  // (every writer of this word writes the same value)
  atomicAdd(&a->size, size);
  atomicAdd(&a->sum[0], sx), atomicAdd(&a->sum[1], sy), atomicAdd(&a->sum[2], sz);
  atomicMax(&a->hi[0], hx), atomicMax(&a->hi[1], hy), atomicMax(&a->hi[2], hz);
  atomicMax(&a->nlo[0], nlx), atomicMax(&a->nlo[1], nly), atomicMax(&a->nlo[2], nlz);
  atomicMax(&a->ngoal, ngoal);
}

// the accumulator of `root` that this workgroup folds into
__device__ __forceinline__ CcAcc* cc_acc(const CcArgs& A, uint32_t root) {
  return A.acc + ((size_t)A.slot[root] * kCcReplicas + (blockIdx.x & (kCcReplicas - 1)));
}

}  // namespace

__global__ __launch_bounds__(512) void k_frontier_mark(FrontierArgs A) {
  constexpr int H = kCcTile + 2;
  __shared__ uint8_t s[H * H * H];
  __shared__ uint32_t ones;
  const int tx = (A.nx + kCcTile - 1) >> kCcTileBits, ty = (A.ny + kCcTile - 1) >> kCcTileBits;
  const CcTile T = cc_tile(A.nx, A.ny, A.nz, tx, ty);
  const int t = (int)threadIdx.x;
  const int x0 = T.x - (t & 7) - 1, y0 = T.y - ((t >> 3) & 7) - 1, z0 = T.z - (t >> 6) - 1;  // the halo's corner
  if (t == 0) ones = 0;
  for (int i = t; i < H * H * H; i += kCcTileVox) {
    const int x = x0 + i % H, y = y0 + (i / H) % H, z = z0 + i / (H * H);
    // outside the box reads as "not 0"
    const bool in = (unsigned)x < (unsigned)A.nx && (unsigned)y < (unsigned)A.ny && (unsigned)z < (unsigned)A.nz;
    s[i] = in ? A.state[((size_t)z * A.ny + y) * A.nx + x] : (uint8_t)1;
  }
  __syncthreads();
  bool m = false;
  if (T.in) {
    const int c = ((t >> 6) + 1) * H * H + (((t >> 3) & 7) + 1) * H + (t & 7) + 1;
    m = s[c] == 1 && (s[c - 1] == 0 || s[c + 1] == 0 || s[c - H] == 0 || s[c + H] == 0 || s[c - H * H] == 0 ||
                      s[c + H * H] == 0);
    if (m && A.cost) m = A.cost[T.v] != kCcUnreached;
    A.mask[T.v] = m ? 1 : 0;
  }
  if (!A.ctl) return;
  const unsigned long long b = __ballot(m);
  if ((t & 63) == 0 && b) atomicAdd(&ones, (uint32_t)__popcll(b));
  __syncthreads();
  if (t == 0 && ones) atomicAdd(&A.ctl->marked, (unsigned long long)ones);
}

__global__ __launch_bounds__(512) void k_cc_local(CcArgs A) {
  __shared__ uint32_t lab[kCcTileVox];
  const CcTile T = cc_tile(A.nx, A.ny, A.nz, A.tx, A.ty);
  const int t = (int)threadIdx.x;
  const bool member = T.in && A.mask[T.v] != 0;
  lab[t] = member ? (uint32_t)t : kCcNone;
  if (!__syncthreads_or(member)) {  // an empty tile
    if (T.in) A.label[T.v] = kCcNone;
    return;
  }
  // the lane's neighbours inside the tile, as a bit per direction
  const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
  uint32_t dirs = 0;
  for (int k = 0; k < 27; ++k) {
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
    if (k != 13 && (unsigned)(lx + dx) < 8u && (unsigned)(ly + dy) < 8u && (unsigned)(lz + dz) < 8u) dirs |= 1u << k;
  }
  // Every member takes the least label among itself and its member neighbours, then follows that label's own
  // chain down, until a sweep changes nothing. Labels only decrease, stay members of the lane's component and
  // are read and written as whole words, so sweeps need no order among their lanes; in a sweep that changed
  // nothing every member's label is at most its neighbours', hence constant over a component, and the least
  // member of a component has kept its own index.
  volatile uint32_t* vl = lab;
  int changed;
  do {
    changed = 0;
    if (member) {
      const uint32_t cur = vl[t];
      uint32_t m = cur;
#pragma unroll
      for (int k = 0; k < 27; ++k) {
        if (dirs >> k & 1u) {
          const uint32_t q = vl[t + (k % 3 - 1) + ((k / 3) % 3 - 1) * 8 + (k / 9 - 1) * 64];
          m = q < m ? q : m;
        }
      }
      for (;;) {
        const uint32_t q = vl[m];
        if (q >= m) break;
        m = q;
      }
      if (m < cur) {
        vl[t] = m;
        changed = 1;
      }
    }
  } while (__syncthreads_or(changed));
  if (T.in) {
    uint32_t g = kCcNone;
    if (member) {
      // inside a tile the global index order is the local (z, y, x) order: the local root is the least member
      const int r = (int)lab[t];
      g = (uint32_t)(((size_t)(T.z - lz + (r >> 6)) * A.ny + (T.y - ly + ((r >> 3) & 7))) * A.nx + (T.x - lx + (r & 7)));
    }
    A.label[T.v] = g;
  }
}

__global__ __launch_bounds__(512) void k_cc_merge(CcArgs A) {
  const CcTile T = cc_tile(A.nx, A.ny, A.nz, A.tx, A.ty);
  const int t = (int)threadIdx.x;
  const int lx = t & 7, ly = (t >> 3) & 7, lz = t >> 6;
  if (!T.in || !(lx == 0 || lx == 7 || ly == 0 || ly == 7 || lz == 0 || lz == 7)) return;
  if (cc_load(A.label + T.v) == kCcNone) return;
  for (int k = 0; k < 13; ++k) {  // the 13 directions towards lower indices: each pair is joined from its greater end
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
    if ((unsigned)(lx + dx) < 8u && (unsigned)(ly + dy) < 8u && (unsigned)(lz + dz) < 8u) continue;  // same tile
    const int x = T.x + dx, y = T.y + dy, z = T.z + dz;
    if ((unsigned)x >= (unsigned)A.nx || (unsigned)y >= (unsigned)A.ny || (unsigned)z >= (unsigned)A.nz) continue;
    const size_t n = ((size_t)z * A.ny + y) * A.nx + x;
    if (cc_load(A.label + n) == kCcNone) continue;
    cc_union(A.label, (uint32_t)T.v, (uint32_t)n);
  }
}

__global__ __launch_bounds__(256) void k_cc_flatten(CcArgs A) {
  const size_t n = (size_t)A.nx * A.ny * A.nz, v = (size_t)blockIdx.x * 256u + threadIdx.x;
  bool root = false;
  if (v < n) {
    const uint32_t l = cc_load(A.label + v);
    if (l != kCcNone) {
      root = l == (uint32_t)v;
      if (!root) {
        const uint32_t r = cc_find(A.label, l);
        if (r != l) A.label[v] = r;
      }
    }
  }
  // the roots of a wave take consecutive accumulators: one atomic per wave
  const unsigned long long b = __ballot(root);
  if (b) {
    const int lane = (int)(threadIdx.x & 63u), first = __ffsll((long long)b) - 1;
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(&A.ctl->total, (uint32_t)__popcll(b));
    base = (uint32_t)__shfl((int)base, first);
    if (root) A.slot[v] = base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
  }
}

__global__ __launch_bounds__(512) void k_cc_stats(CcArgs A) {
  __shared__ uint32_t h_key[kCcHash], h_size[kCcHash], h_sum[3][kCcHash], h_hi[3][kCcHash], h_nlo[3][kCcHash];
  __shared__ unsigned long long h_goal[kCcHash];
  const CcTile T = cc_tile(A.nx, A.ny, A.nz, A.tx, A.ty);
  const int t = (int)threadIdx.x;
  if (t < kCcHash) {
    h_key[t] = kCcNone, h_size[t] = 0, h_goal[t] = 0;
    for (int a = 0; a < 3; ++a) h_sum[a][t] = 0, h_hi[a][t] = 0, h_nlo[a][t] = 0;
  }
  const uint32_t r = T.in ? A.label[T.v] : kCcNone;
  const bool member = r != kCcNone;
  if (!__syncthreads_or(member)) return;
  // the lane's own part; a lane off the mask holds the identity
  uint32_t size = member, sx = member ? T.x : 0, sy = member ? T.y : 0, sz = member ? T.z : 0;
  uint32_t hx = sx, hy = sy, hz = sz;
  uint32_t nlx = member ? ~(uint32_t)T.x : 0, nly = member ? ~(uint32_t)T.y : 0, nlz = member ? ~(uint32_t)T.z : 0;
  unsigned long long ngoal = 0;
  if (member) ngoal = ~(((unsigned long long)(A.key ? A.key[T.v] : 0u) << 32) | (unsigned long long)T.v);
  // A wave whose members share one root (the common case: a z slice inside one component) folds itself
  // through its lanes first and sends one part to LDS.
  const unsigned long long mb = __ballot(member);
  bool send = member;
  if (mb) {
    const int first = __ffsll((long long)mb) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)r, first);
    if (__ballot(member && r != r0) == 0) {
      for (int o = 32; o > 0; o >>= 1) {
        size += (uint32_t)__shfl_xor((int)size, o);
        sx += (uint32_t)__shfl_xor((int)sx, o), sy += (uint32_t)__shfl_xor((int)sy, o), sz += (uint32_t)__shfl_xor((int)sz, o);
        uint32_t q;
        q = (uint32_t)__shfl_xor((int)hx, o), hx = q > hx ? q : hx;
        q = (uint32_t)__shfl_xor((int)hy, o), hy = q > hy ? q : hy;
        q = (uint32_t)__shfl_xor((int)hz, o), hz = q > hz ? q : hz;
        q = (uint32_t)__shfl_xor((int)nlx, o), nlx = q > nlx ? q : nlx;
        q = (uint32_t)__shfl_xor((int)nly, o), nly = q > nly ? q : nly;
        q = (uint32_t)__shfl_xor((int)nlz, o), nlz = q > nlz ? q : nlz;
        const unsigned long long g = __shfl_xor(ngoal, o);
        ngoal = g > ngoal ? g : ngoal;
      }
      send = (t & 63) == first;
    }
  }
  if (send) {
    // the root's entry of the table: at most kCcTileRoots distinct roots meet kCcHash entries, so a free or
    // matching entry comes up within kCcHash probes
    uint32_t h = (r * 2654435761u) >> (32 - 7);
    static_assert(kCcHash == 128, "the hash takes 7 bits");
    int e = -1;
    for (int p = 0; p < kCcHash; ++p) {
      const uint32_t old = atomicCAS(&h_key[h], kCcNone, r);
      if (old == kCcNone || old == r) {
        e = (int)h;
        break;
      }
      h = (h + 1) & (kCcHash - 1);
    }
    if (e >= 0) {
      atomicAdd(&h_size[e], size);
      atomicAdd(&h_sum[0][e], sx), atomicAdd(&h_sum[1][e], sy), atomicAdd(&h_sum[2][e], sz);
      atomicMax(&h_hi[0][e], hx), atomicMax(&h_hi[1][e], hy), atomicMax(&h_hi[2][e], hz);
      atomicMax(&h_nlo[0][e], nlx), atomicMax(&h_nlo[1][e], nly), atomicMax(&h_nlo[2][e], nlz);
      atomicMax(&h_goal[e], ngoal);
    } else {  // (a table that filled up: labels that are no labelling; the part goes out on its own)
      cc_fold_global(cc_acc(A, r), r, size, sx, sy, sz, hx, hy, hz, nlx, nly, nlz, ngoal);
    }
  }
  __syncthreads();
  if (t < kCcHash && h_key[t] != kCcNone) {
    const uint32_t root = h_key[t];
    cc_fold_global(cc_acc(A, root), root, h_size[t], h_sum[0][t], h_sum[1][t], h_sum[2][t], h_hi[0][t], h_hi[1][t],
                   h_hi[2][t], h_nlo[0][t], h_nlo[1][t], h_nlo[2][t], h_goal[t]);
  }
}

__global__ __launch_bounds__(256) void k_cc_emit(CcArgs A, uint32_t total, uint32_t min_size, CcRec* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  CcAcc a{};
  if (i < total) {
    for (int k = 0; k < kCcReplicas; ++k) {
      const CcAcc p = A.acc[(size_t)i * kCcReplicas + k];
      if (p.size == 0) continue;  // (a replica no tile chose: all zeros)
      a.label = p.label, a.size += p.size;
      for (int c = 0; c < 3; ++c) {
        a.hi[c] = p.hi[c] > a.hi[c] ? p.hi[c] : a.hi[c], a.nlo[c] = p.nlo[c] > a.nlo[c] ? p.nlo[c] : a.nlo[c];
        a.sum[c] += p.sum[c];
      }
      a.ngoal = p.ngoal > a.ngoal ? p.ngoal : a.ngoal;
    }
  }
  const bool keep = i < total && a.size >= min_size;
  const unsigned long long b = __ballot(keep);
  if (!b) return;
  const int lane = (int)(threadIdx.x & 63u), first = __ffsll((long long)b) - 1;
  uint32_t base = 0;
  if (lane == first) base = atomicAdd(&A.ctl->count, (uint32_t)__popcll(b));
  base = (uint32_t)__shfl((int)base, first);
  if (!keep) return;
  const unsigned long long goal = ~a.ngoal;
  CcRec rec;
  rec.label = a.label, rec.size = a.size;
  for (int k = 0; k < 3; ++k) {
    rec.lo[k] = (int32_t)~a.nlo[k], rec.hi[k] = (int32_t)a.hi[k];
    rec.sum[k] = (long long)a.sum[k];
  }
  rec.goal = (uint32_t)goal, rec.goal_key = (uint32_t)(goal >> 32);
  out[base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = rec;
}

}  // namespace tsdf
