// Working-resolution inference: the model runs on frames reduced by an integer factor D and
// its flow comes back at the camera's resolution, in the camera's pixel units.
//
// ingest_frames_scaled: uint8 (N, H, W, 3) -> fp32 (N, 3, hp, wp), the box (area) downscale by
// D and the replicate padding of ingest_frames in one launch.  Low-resolution cell (i, j) covers
// rows [iD, min((i+1)D, H)) x columns [jD, min((j+1)D, W)); its value is float(sum) / float(count)
// with the integer sum of the cell's bytes (at most 64 * 255: exact) and the number of its pixels
// inside the image (the last row / column of cells may be partial): one IEEE fp32 division.  One
// thread produces 4 consecutive pixels of an output row for the three channels; away from the
// padding its input per source row is 12 D contiguous bytes, next to its neighbours'.  A padding
// pixel recomputes the cell of its clamped index.  D = 2, 3, 4 are template constants (unrolled
// sums), other factors loop.  D = 1 is bitwise ingest_frames (x / 1.0f).
//
// upscale_flow: fp32 (B, 2, hp, wp) -> fp32 (B, 2, H, W): the unpadded low-resolution image inside
// the padded frame sampled bilinearly with pixel centres aligned (align_corners=False), clamped
// at the border, times D.  Per axis and output index x, with n low-resolution samples:
//   q = x / D, r = x % D, t = 2r + 1 - D;  t >= 0: i0 = q, num = t;  else i0 = q - 1, num = t + 2D
//   fx = float(num) / float(2D);  fx = 0 when i0 < 0 or i0 >= n - 1
//   i0 = clamp(i0, 0, n - 1), i1 = min(i0 + 1, n - 1)
// so the weight is one rounding of an exact rational at any width.  The lerp rounds step by step
// in the order of fb_consistency.hip (ops/frame_scale.py upscale_flow_ref is the same sequence in
// torch ops).  One thread produces 4 consecutive pixels of an output row for both components:
// the row weight and the two source rows once, the column cell and remainder once and stepped
// from there.  The low-resolution taps (each shared by up to (D + 1)^2 outputs) go through the
// cache.
//
// Both: no atomics, no memset, one launch on the given stream; float4 stores when the output
// width is a multiple of 4 and the base is 16-byte aligned, scalar stores with a tail otherwise.
#include "common.h"

// every step rounds on its own, like the torch sequences
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

// sum of the three channels of cell columns [x0, x0 + D) x rows [r0, r0 + D) inside the image
template <int DT>
__device__ __forceinline__ void cell_sums(const unsigned char* __restrict__ img, int H, int W, int D, int r0, int x0,
                                          int s[3]) {
  s[0] = s[1] = s[2] = 0;
  if constexpr (DT > 0) {
#pragma unroll
    for (int dy = 0; dy < DT; ++dy) {
      if (r0 + dy < H) {
        const unsigned char* p = img + ((long)(r0 + dy) * W + x0) * 3;
#pragma unroll
        for (int dx = 0; dx < DT; ++dx) {
          if (x0 + dx < W) {
            s[0] += p[3 * dx];
            s[1] += p[3 * dx + 1];
            s[2] += p[3 * dx + 2];
          }
        }
      }
    }
  } else {
    const int r1 = min(r0 + D, H), x1 = min(x0 + D, W);
    for (int y = r0; y < r1; ++y) {
      const unsigned char* p = img + ((long)y * W + x0) * 3;
      for (int dx = 0; dx < x1 - x0; ++dx) {
        s[0] += p[3 * dx];
        s[1] += p[3 * dx + 1];
        s[2] += p[3 * dx + 2];
      }
    }
  }
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void ingest_scaled_kernel(IngestScaledArgs a) {
  const int D = DT > 0 ? DT : a.D;
  const int Wq = (a.wp + 3) / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.N * a.hp * Wq) return;
  const int xq = (int)(idx % Wq);
  const long t = idx / Wq;
  const int y = (int)(t % a.hp), n = (int)(t / a.hp);
  const int ci = min(max(y - a.pt, 0), a.h - 1);
  const int r0 = ci * D;
  const int rows = min(r0 + D, a.H) - r0;
  const unsigned char* img = a.in + (long)n * a.H * a.W * 3;
  float c[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a column past wp (last group of a row) clamps to a valid cell and is not stored
    const int cj = min(max(xq * 4 + j - a.pl, 0), a.w - 1);
    const int x0 = cj * D;
    const int cols = min(x0 + D, a.W) - x0;
    int s[3];
    cell_sums<DT>(img, a.H, a.W, D, r0, x0, s);
    const float cnt = (float)(rows * cols);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][j] = (float)s[ch] / cnt;
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* o = a.out + (((long)n * 3 + ch) * a.hp + y) * a.wp + xq * 4;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xq * 4 + j < a.wp) o[j] = c[ch][j];
    }
  }
}

// one axis of the upscale: output index x over n low-resolution samples -> (i0, i1, weight of i1)
__device__ __forceinline__ void axis_taps(int q, int r, int D, int n, int& i0, int& i1, float& f) {
  const int t = 2 * r + 1 - D;
  int num;
  if (t >= 0) {
    i0 = q;
    num = t;
  } else {
    i0 = q - 1;
    num = t + 2 * D;
  }
  f = (float)num / (float)(2 * D);
  if (i0 < 0 || i0 >= n - 1) f = 0.f;
  i0 = min(max(i0, 0), n - 1);
  i1 = min(i0 + 1, n - 1);
}

template <bool VEC>
__global__ __launch_bounds__(256) void upscale_flow_kernel(UpscaleFlowArgs a) {
  const int Wq = (a.W + 3) / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.B * a.H * Wq) return;
  const int xq = (int)(idx % Wq);
  const long tt = idx / Wq;
  const int y = (int)(tt % a.H), b = (int)(tt / a.H);
  const int D = a.D;
  int y0, y1;
  float fy;
  axis_taps(y / D, y % D, D, a.h, y0, y1, fy);
  const long plane = (long)a.hp * a.wp;
  const float* u = a.flow + (long)b * 2 * plane + a.left;
  const float* row0 = u + (long)(a.top + y0) * a.wp;
  const float* row1 = u + (long)(a.top + y1) * a.wp;
  const float scale = (float)D;
  float o[2][4];
  int q = (xq * 4) / D, r = (xq * 4) % D;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a column past W (last group of a row) clamps to a valid cell and is not stored
    int x0, x1;
    float fx;
    axis_taps(min(q, a.w - 1), r, D, a.w, x0, x1, fx);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float a00 = row0[c * plane + x0], a01 = row0[c * plane + x1];
      const float a10 = row1[c * plane + x0], a11 = row1[c * plane + x1];
      float top = a01 - a00;
      top = fx * top;
      top = a00 + top;
      float bot = a11 - a10;
      bot = fx * bot;
      bot = a10 + bot;
      float s = bot - top;
      s = fy * s;
      s = top + s;
      o[c][j] = s * scale;
    }
    if (++r == D) {
      r = 0;
      ++q;
    }
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float* p = a.out + (((long)b * 2 + c) * a.H + y) * a.W + xq * 4;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(p) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xq * 4 + j < a.W) p[j] = o[c][j];
    }
  }
}

template <int DT>
hipError_t launch_ingest_scaled(const IngestScaledArgs& a, const dim3& grid, hipStream_t s) {
  if (a.wp % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0)
    hipLaunchKernelGGL((ingest_scaled_kernel<DT, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((ingest_scaled_kernel<DT, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ingest_frames_scaled(const IngestScaledArgs& a, hipStream_t s) {
  const long groups = (long)a.N * a.hp * ((a.wp + 3) / 4);
  if (groups == 0) return hipSuccess;
  if (a.D < 1 || a.h != (a.H + a.D - 1) / a.D || a.w != (a.W + a.D - 1) / a.D) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((groups + 255) / 256));
  switch (a.D) {
    case 2: return launch_ingest_scaled<2>(a, grid, s);
    case 3: return launch_ingest_scaled<3>(a, grid, s);
    case 4: return launch_ingest_scaled<4>(a, grid, s);
    default: return launch_ingest_scaled<0>(a, grid, s);
  }
}

hipError_t launch_upscale_flow(const UpscaleFlowArgs& a, hipStream_t s) {
  const long groups = (long)a.B * a.H * ((a.W + 3) / 4);
  if (groups == 0) return hipSuccess;
  if (a.D < 1 || a.h != (a.H + a.D - 1) / a.D || a.w != (a.W + a.D - 1) / a.D || a.left < 0 || a.top < 0 ||
      a.left + a.w > a.wp || a.top + a.h > a.hp)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (a.W % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0)
    hipLaunchKernelGGL(upscale_flow_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(upscale_flow_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
