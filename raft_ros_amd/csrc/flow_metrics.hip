// Validation metrics of a flow prediction on the device: end-point error and threshold counts.
//
// Per pixel (x, y) of image b, all in fp32, every operation rounded on its own (the sequence of
// eval/validate.py's host loops; ops/metrics.py holds it in torch ops, flow_metrics_ref):
//   pr = flow_pr[b, :, top + y, left + x]      the padded prediction, cropped in place
//   du = pr_u - gt_u;  dv = pr_v - gt_v;  epe = sqrtf(du*du + dv*dv)
//   mag = sqrtf(gt_u*gt_u + gt_v*gt_v)
//   counted = no valid given, or valid >= 0.5     (a select: a NaN at an uncounted pixel is dropped)
//   outlier = epe > 3 && epe / mag > 0.05         (mag == 0 gives inf or NaN; a NaN compares false)
// epe_sum[b] = float64 sum of epe over the counted pixels; counts[b] = counted, epe < 1, epe < 3,
// epe < 5, outliers.
//
// Two launches, no memset, no atomics, no host read-back.  First: a thread takes 4 consecutive
// pixels of one row (a row's last group may be short), a block 256 groups of one image.  The
// thread sums in float64 in pixel order, the wave by an xor butterfly, the block over its waves in
// index order; the counts travel as five 12-bit fields of one 64-bit integer (a block counts at
// most 1024 pixels).  Every block writes its partial.  Second: one block per image sums that
// image's partials, thread t the partials t, t + 256, ... in order, then wave and block as before.
// The order of every sum is fixed by (H, W) alone: the result does not depend on the order in
// which blocks finish, on B or on the image's place in the batch.  The kernel boundary on the
// stream hands the partials over.
//
// Loads: gt and valid as float4 when W % 4 == 0, pr as float4 when also left % 4 == 0 and
// Wp % 4 == 0 (bases 16-byte aligned); scalar otherwise, coalesced either way.
#include "common.h"

// every step must round like the torch op sequence
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

constexpr int kField = 12;  // bits per packed count: 4 * 256 = 1024 < 4096

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// VG: gt and valid by float4;  VP: pr by float4 (implies VG)
template <bool VG, bool VP>
__global__ __launch_bounds__(256) void flow_metrics_kernel(FlowMetricsArgs a) {
  __shared__ double wsum[4];
  __shared__ unsigned long long wcnt[4];
  const unsigned nblk = (unsigned)a.nblk;
  const unsigned b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;  // the grid is B * nblk exactly
  const unsigned gpr = (unsigned)flow_metrics_row_groups(a.W);
  const unsigned g = blk * 256u + threadIdx.x;  // group of the image; < H * gpr + 256 < 2^32
  const unsigned y = g / gpr;
  double s = 0.0;
  unsigned long long c = 0;
  if (y < (unsigned)a.H) {
    const unsigned x0 = (g - y * gpr) * 4u;  // < W
    const size_t HW = (size_t)a.H * a.W, HWp = (size_t)a.Hp * a.Wp;
    const float* gt = a.gt + (size_t)b * 2 * HW + (size_t)y * a.W + x0;
    const float* pr = a.pr + (size_t)b * 2 * HWp + (size_t)(a.top + y) * a.Wp + a.left + x0;
    const float* va = a.valid ? a.valid + (size_t)b * HW + (size_t)y * a.W + x0 : nullptr;
    const int n = VG ? 4 : min(4, a.W - (int)x0);
    float gu[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
    float pu[4] = {0.f, 0.f, 0.f, 0.f}, pv[4] = {0.f, 0.f, 0.f, 0.f};
    float vl[4] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (VG) {
      const float4 U = *reinterpret_cast<const float4*>(gt);
      const float4 V = *reinterpret_cast<const float4*>(gt + HW);
      gu[0] = U.x, gu[1] = U.y, gu[2] = U.z, gu[3] = U.w;
      gv[0] = V.x, gv[1] = V.y, gv[2] = V.z, gv[3] = V.w;
      if (va) {
        const float4 M = *reinterpret_cast<const float4*>(va);
        vl[0] = M.x, vl[1] = M.y, vl[2] = M.z, vl[3] = M.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) {
          gu[j] = gt[j];
          gv[j] = gt[HW + j];
          if (va) vl[j] = va[j];
        }
    }
    if constexpr (VP) {
      const float4 U = *reinterpret_cast<const float4*>(pr);
      const float4 V = *reinterpret_cast<const float4*>(pr + HWp);
      pu[0] = U.x, pu[1] = U.y, pu[2] = U.z, pu[3] = U.w;
      pv[0] = V.x, pv[1] = V.y, pv[2] = V.z, pv[3] = V.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) {
          pu[j] = pr[j];
          pv[j] = pr[HWp + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float du = pu[j] - gu[j], dv = pv[j] - gv[j];
      const float epe = sqrtf(du * du + dv * dv);
      const float mag = sqrtf(gu[j] * gu[j] + gv[j] * gv[j]);
      const bool out = epe > 3.0f && epe / mag > 0.05f;
      if (j < n && vl[j] >= 0.5f) {  // a NaN valid is not counted
        s += (double)epe;
        c += 1ull | (epe < 1.0f ? 1ull << kField : 0ull) | (epe < 3.0f ? 1ull << 2 * kField : 0ull) |
             (epe < 5.0f ? 1ull << 3 * kField : 0ull) | (out ? 1ull << 4 * kField : 0ull);
      }
    }
  }
  s = wave_sum_f64(s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = s;
    wcnt[threadIdx.x >> 6] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    c = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    a.part_sum[blockIdx.x] = s;
    int* pc = a.part_cnt + (size_t)blockIdx.x * kMetricCounts;
#pragma unroll
    for (int k = 0; k < kMetricCounts; ++k) pc[k] = (int)(c >> k * kField & ((1ull << kField) - 1));
  }
}

// one block per image: its nblk partials in a fixed order
__global__ __launch_bounds__(256) void flow_metrics_finish_kernel(FlowMetricsArgs a) {
  __shared__ double wsum[4];
  __shared__ int wcnt[4][kMetricCounts];
  const unsigned b = blockIdx.x;
  const double* ps = a.part_sum + (size_t)b * a.nblk;
  const int* pc = a.part_cnt + (size_t)b * a.nblk * kMetricCounts;
  double s = 0.0;
  int c[kMetricCounts] = {0, 0, 0, 0, 0};  // an image has fewer than 2^31 pixels
  for (int i = threadIdx.x; i < a.nblk; i += 256) {
    s += ps[i];
#pragma unroll
    for (int k = 0; k < kMetricCounts; ++k) c[k] += pc[(size_t)i * kMetricCounts + k];
  }
  s = wave_sum_f64(s);
#pragma unroll
  for (int k = 0; k < kMetricCounts; ++k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_xor(c[k], off, kWave);
  }
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = s;
#pragma unroll
    for (int k = 0; k < kMetricCounts; ++k) wcnt[threadIdx.x >> 6][k] = c[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.epe_sum[b] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
#pragma unroll
    for (int k = 0; k < kMetricCounts; ++k)
      a.counts[b * kMetricCounts + k] = wcnt[0][k] + wcnt[1][k] + wcnt[2][k] + wcnt[3][k];
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_flow_metrics(const FlowMetricsArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.H <= 0 || a.W <= 0) return hipSuccess;  // the caller zeroes the results
  if (a.top < 0 || a.left < 0 || (long)a.top + a.H > a.Hp || (long)a.left + a.W > a.Wp) return hipErrorInvalidValue;
  if ((long)a.B * a.H * a.W >= (1L << 31) || a.nblk != flow_metrics_blocks(a.H, a.W)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((long)a.B * a.nblk));  // <= B * H * W
  const bool vg = a.W % 4 == 0 && aligned16(a.gt) && (!a.valid || aligned16(a.valid));
  const bool vp = vg && a.left % 4 == 0 && a.Wp % 4 == 0 && aligned16(a.pr);
  if (vp)
    hipLaunchKernelGGL((flow_metrics_kernel<true, true>), grid, dim3(256), 0, s, a);
  else if (vg)
    hipLaunchKernelGGL((flow_metrics_kernel<true, false>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((flow_metrics_kernel<false, false>), grid, dim3(256), 0, s, a);
  RAFT_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(flow_metrics_finish_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
