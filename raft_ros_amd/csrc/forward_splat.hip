// Warm start for video: forward-splat of the previous pair's low-resolution flow with
// nearest-neighbour fill, the device form of forward_interpolate (utils/utils.py, reference
// core/utils/utils.py:26-54), made exact and deterministic:
//   source pixel s = y * W + x with flow (dx, dy) is the point (x1, y1) = ((double)x + dx,
//   (double)y + dy), valid iff 0 < x1 < W and 0 < y1 < H (NaN / Inf fail the comparisons);
//   out[:, yt, xt] = the flow of the valid point that minimises d2 = (x1 - xt)^2 + (y1 - yt)^2
//   (fp64, no FMA contraction), exact ties to the lowest s; all zeros when no point is valid.
//
// Two kernels after one memset of the list heads (-1):
//   bin:    one thread per source pixel; a valid point is pushed (one atomicExch) onto the
//           linked list of its integer cell (floor(x1), floor(y1)), always inside the image.
//   gather: one thread per target pixel scans the square of cells [xt - R, xt + R - 1] x
//           [yt - R, yt + R - 1] for R = 1, 2, ..., visiting only the new ring.  Every point
//           outside the square is at Chebyshev distance >= R, so the search stops once
//           best d2 < R^2 (strictly: a point at distance exactly R may carry a lower index).
//           Selection is by the pair (d2, s): the order of a list never shows.
// Only the source index is stored; (x1, y1) is recomputed from s and flow[s].  A few tens of
// thousands of points: plain global memory, no LDS, no host read-back (graph capturable).
#include "common.h"

// hipcc contracts a * b + c into an FMA by default; the distances must round like the
// separate fp64 multiply and add of the oracle
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

__device__ __forceinline__ bool splat_point(const float* __restrict__ f, long HW, int W, int H, int s, double& x1,
                                            double& y1) {
  x1 = (double)(s % W) + (double)f[s];
  y1 = (double)(s / W) + (double)f[HW + s];
  return x1 > 0.0 && x1 < (double)W && y1 > 0.0 && y1 < (double)H;
}

__global__ __launch_bounds__(256) void splat_bin_kernel(SplatArgs a) {
  const long HW = (long)a.H * a.W;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * HW) return;
  const int b = (int)(idx / HW), s = (int)(idx - b * HW);
  double x1, y1;
  if (!splat_point(a.flow + (long)b * 2 * HW, HW, a.W, a.H, s, x1, y1)) return;
  // 0 < x1 < W, 0 < y1 < H: the cell lies in [0, W) x [0, H)
  const int cell = (int)y1 * a.W + (int)x1;
  a.next[idx] = atomicExch(a.heads + b * HW + cell, s);
  a.any[b] = 0;  // every writer stores the same value
}

struct Best {
  double d2;
  int s;
};

__device__ __forceinline__ void scan_cell(const SplatArgs& a, const float* __restrict__ f, const int* __restrict__ heads,
                                          const int* __restrict__ next, long HW, int cx, int cy, int xt, int yt,
                                          Best& best) {
  for (int s = heads[cy * a.W + cx]; s >= 0; s = next[s]) {
    double x1, y1;
    splat_point(f, HW, a.W, a.H, s, x1, y1);
    const double ex = x1 - (double)xt, ey = y1 - (double)yt;
    const double d2 = ex * ex + ey * ey;
    if (d2 < best.d2 || (d2 == best.d2 && s < best.s)) {
      best.d2 = d2;
      best.s = s;
    }
  }
}

__global__ __launch_bounds__(256) void splat_gather_kernel(SplatArgs a) {
  const long HW = (long)a.H * a.W;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.B * HW) return;
  const int b = (int)(idx / HW), t = (int)(idx - b * HW);
  const int xt = t % a.W, yt = t / a.W;
  const float* f = a.flow + (long)b * 2 * HW;
  float* o = a.out + (long)b * 2 * HW;
  Best best{__builtin_inf(), -1};
  if (a.any[b] == 0) {
    const int* heads = a.heads + b * HW;
    const int* next = a.next + b * HW;
    const int rmax = max(a.H, a.W);  // the square of R = max(H, W) holds every cell
    for (int R = 1; R <= rmax; ++R) {
      const int x0 = xt - R, x1 = xt + R - 1, y0 = yt - R, y1 = yt + R - 1;
      const int cx0 = max(x0, 0), cx1 = min(x1, a.W - 1);
      if (y0 >= 0)
        for (int cx = cx0; cx <= cx1; ++cx) scan_cell(a, f, heads, next, HW, cx, y0, xt, yt, best);
      if (y1 < a.H)
        for (int cx = cx0; cx <= cx1; ++cx) scan_cell(a, f, heads, next, HW, cx, y1, xt, yt, best);
      const int cy0 = max(y0 + 1, 0), cy1 = min(y1 - 1, a.H - 1);
      if (x0 >= 0)
        for (int cy = cy0; cy <= cy1; ++cy) scan_cell(a, f, heads, next, HW, x0, cy, xt, yt, best);
      if (x1 < a.W)
        for (int cy = cy0; cy <= cy1; ++cy) scan_cell(a, f, heads, next, HW, x1, cy, xt, yt, best);
      if (best.d2 < (double)R * (double)R) break;
      if (x0 <= 0 && y0 <= 0 && x1 >= a.W - 1 && y1 >= a.H - 1) break;  // the whole image is scanned
    }
  }
  o[t] = best.s >= 0 ? f[best.s] : 0.f;
  o[HW + t] = best.s >= 0 ? f[HW + best.s] : 0.f;
}

}  // namespace

hipError_t launch_forward_splat(const SplatArgs& a, hipStream_t s) {
  const long tot = (long)a.B * a.H * a.W;
  if (tot == 0) return hipSuccess;
  // heads and the per-image "no valid point" words are one allocation: all -1
  RAFT_HIP_CHECK(hipMemsetAsync(a.heads, 0xff, (size_t)(tot + a.B) * sizeof(int), s));
  const dim3 grid((unsigned)((tot + 255) / 256));
  hipLaunchKernelGGL(splat_bin_kernel, grid, dim3(256), 0, s, a);
  RAFT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(splat_gather_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
