// tsdf_plan.hip -- lamp-stop planning (DESIGN.md "Lamp-stop planning"): the dose each of C candidate lamp
// placements alone would add to each receiver (k_uv_irradiance: k_uv_dose's march, the candidate as the
// grid's second dimension), and the greedy selection on that C x n matrix (k_plan_gain, k_plan_final,
// k_plan_apply: one round each, no atomics, a fixed addition tree). k_uv_irradiance only reads the volume;
// the plan kernels do not touch it.
#include "tsdf_dose_march.h"

namespace tsdf {

__global__ __launch_bounds__(256) void k_uv_irradiance(EngineDev D, DoseParams A, ViewGrid V,
                                                       const int32_t* __restrict__ first, int c0,
                                                       float* __restrict__ out) {
  extern __shared__ uint32_t sbits[];
  const int nw = V.n ? V.nw : 0;
  for (int i = threadIdx.x; i < nw; i += 256) sbits[i] = V.bits[i];
  __syncthreads();
  dose_body<true>(D, A, V, sbits, first, c0, out);
}

// The gain sums' tree (it depends on n only): receiver i belongs to chunk g = i / kPlanChunk, item
// j = (i % kPlanChunk) / 256 and thread t = i % 256 of that chunk's workgroup.
//   thread t:    its kPlanItems terms, as doubles, added in item order from 0
//   wave:        butterfly over lane distance 32, 16, 8, 4, 2, 1 (every lane ends with the same sum)
//   workgroup:   ((wave 0 + wave 1) + wave 2) + wave 3  ->  part[g * C + c]
// (a workgroup does this for kPlanRows candidates in turn, with the chunk's need and weight in registers)
//   k_plan_final: the chunks of a candidate in index order from 0
// A receiver past n contributes +0.0, which changes no sum (no term is negative zero: a term is a positive
// product or +0.0).
__global__ __launch_bounds__(256) void k_plan_gain(PlanArgs P, int c0) {
  __shared__ double sw[kPlanRows][4];
  if (P.state->stopped) return;  // (uniform)
  const int cb = c0 + (int)blockIdx.y * kPlanRows;
  const int64_t i0 = (int64_t)blockIdx.x * kPlanChunk + threadIdx.x;
  // the chunk's need and weight once for the workgroup's kPlanRows candidates
  float nd[kPlanItems], w[kPlanItems];
#pragma unroll
  for (int j = 0; j < kPlanItems; ++j) {
    const int64_t i = i0 + (int64_t)j * 256;
    const bool in = i < P.n;
    nd[j] = in ? P.need[i] : 0.0f;
    w[j] = in && P.weight ? P.weight[i] : 1.0f;
  }
  for (int r = 0; r < kPlanRows && cb + r < P.C; ++r) {  // (uniform)
    const float* __restrict__ row = P.E + (int64_t)(cb + r) * P.n;
    float e[kPlanItems];
#pragma unroll
    for (int j = 0; j < kPlanItems; ++j) {
      const int64_t i = i0 + (int64_t)j * 256;
      e[j] = i < P.n ? row[i] : 0.0f;
    }
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < kPlanItems; ++j) {
      // (both tests: fminf alone would hand a NaN's partner through)
      const float g = e[j] > 0.0f && nd[j] > 0.0f ? w[j] * fminf(e[j], nd[j]) : 0.0f;
      a += (double)g;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) sw[r][threadIdx.x >> 6] = a;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kPlanRows && cb + t < P.C)
    P.part[(int64_t)blockIdx.x * P.C + cb + t] = ((sw[t][0] + sw[t][1]) + sw[t][2]) + sw[t][3];
}

namespace {
// the better of two (gain, candidate) pairs: the larger gain, the lower candidate between equal gains
__device__ __forceinline__ bool plan_better(double a, int ai, double b, int bi) {
  return a > b || (a == b && ai < bi);
}
}  // namespace

// One workgroup. Thread t adds the G partials of the candidates t, t + 256, ... in index order (eight
// loads in flight; part is chunk-major, so the 256 threads read consecutive doubles) and keeps the best of
// its own; the workgroup's best by plan_better, a total order on (gain, candidate), so the way the pairs
// meet does not matter. Then round r's decision.
__global__ __launch_bounds__(256) void k_plan_final(PlanArgs P, int G, int r, float min_gain) {
  __shared__ double sv[4];
  __shared__ int si[4];
  if (P.state->stopped) return;  // (uniform)
  double bv = -1.0;              // (no gain is negative with weights >= 0: any candidate beats it)
  int bi = 0x7FFFFFFF;
  for (int c = threadIdx.x; c < P.C; c += 256) {
    double acc = 0.0;
    int g = 0;
    for (; g + 8 <= G; g += 8) {
      double v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = P.part[(int64_t)(g + k) * P.C + c];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += v[k];
    }
    for (; g < G; ++g) acc += P.part[(int64_t)g * P.C + c];
    if (plan_better(acc, c, bv, bi)) bv = acc, bi = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (plan_better(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  if ((threadIdx.x & 63) == 0) sv[threadIdx.x >> 6] = bv, si[threadIdx.x >> 6] = bi;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k)
      if (plan_better(sv[k], si[k], bv, bi)) bv = sv[k], bi = si[k];
    if (!(bv > 0.0) || !(bv >= (double)min_gain) || bi < 0 || bi >= P.C) {
      P.state->stopped = 1;
    } else {
      P.state->best = bi;
      P.state->nstops = r + 1;
      P.gains[r] = bv;
      P.stops[r] = bi;
    }
  }
}

__global__ __launch_bounds__(256) void k_plan_apply(PlanArgs P) {
  if (P.state->stopped) return;  // (uniform)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  const float e = P.E[(int64_t)P.state->best * P.n + i];
  if (e > 0.0f) P.need[i] = fmaxf(P.need[i] - e, 0.0f);
}

}  // namespace tsdf
