// Forward-backward consistency of a flow pair: where can the forward flow be trusted?
//
// Per pixel (x, y) of image b, all in fp32, every multiply and add rounded on its own:
//   u, v = fw[b, :, y, x];  px = x + u, py = y + v                       the pixel's target
//   target outside [0, W-1] x [0, H-1] (NaN counts as outside): occ = 2, err2 = +inf
//   otherwise s = bw[b] read bilinearly at the target (the right / lower neighbour clamped to
//   the last column / row, where its weight is 0):
//     top = a00 + fx (a01 - a00), bot = a10 + fx (a11 - a10), s_c = top + fy (bot - top)
//   err2 = (u + s_0)^2 + (v + s_1)^2
//   occ  = err2 <= alpha1 ((u^2 + v^2) + (s_0^2 + s_1^2)) + alpha2 ? 0 : 1      (NaN -> 1)
// and counts[b] = the number of pixels of class 1 and of class 2.  ops/consistency.py holds the
// same sequence in torch ops (fb_consistency_ref); the two agree bitwise.
//
// One memset of the counts and one launch, no host read-back.  Each thread handles 4 consecutive
// pixels of the flat (B * H * W) index: fw as two float4 when H * W is a multiple of 4 (the
// group then lies in one image, 16-byte aligned), the 4 mask bytes as one dword and the 4 errors
// as one float4 (a group starts at a multiple of 4 whatever H * W is); the last group may be
// short (scalar stores).  Otherwise a group may straddle images: each pixel uses its own image's
// base and counter.  The bw gathers are scalar.  Counts: a block's 1024 pixels touch the images
// [b_lo, b_hi]; per image one packed wave + block sum and one integer atomicAdd per non-zero
// class, so the result does not depend on the order of arrival.
#include "common.h"

// every step must round like the torch op sequence
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

// one pixel p = y * W + x of an image with backward flow bw (2, H, W) -> class, err2
__device__ __forceinline__ int fb_pixel(const FbConsistencyArgs& a, const float* __restrict__ bw, unsigned p, float u,
                                        float v, float& err2) {
  const int y = (int)(p / (unsigned)a.W), x = (int)(p - (unsigned)y * (unsigned)a.W);
  const float px = (float)x + u, py = (float)y + v;
  const bool inside = px >= 0.f && px <= (float)(a.W - 1) && py >= 0.f && py <= (float)(a.H - 1);
  if (!inside) {
    err2 = __builtin_inff();
    return 2;
  }
  const float x0f = floorf(px), y0f = floorf(py);
  const float fx = px - x0f, fy = py - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;  // in [0, W-1] x [0, H-1]: inside
  const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
  const float* r0 = bw + (long)y0 * a.W;
  const float* r1 = bw + (long)y1 * a.W;
  float s[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float a00 = r0[c * a.HW + x0], a01 = r0[c * a.HW + x1];
    const float a10 = r1[c * a.HW + x0], a11 = r1[c * a.HW + x1];
    const float top = a00 + fx * (a01 - a00);
    const float bot = a10 + fx * (a11 - a10);
    s[c] = top + fy * (bot - top);
  }
  const float du = u + s[0], dv = v + s[1];
  err2 = du * du + dv * dv;
  const float thr = a.alpha1 * ((u * u + v * v) + (s[0] * s[0] + s[1] * s[1])) + a.alpha2;
  return err2 <= thr ? 0 : 1;
}

template <bool VEC>
__global__ __launch_bounds__(256) void fb_consistency_kernel(FbConsistencyArgs a) {
  __shared__ int part[2][4];
  // B * H * W < 2^31 (checked by the launcher): pixel indices are 32-bit, element offsets 64-bit
  const unsigned HW = (unsigned)a.HW, tot = (unsigned)a.B * HW;
  const unsigned blk0 = blockIdx.x * 1024u;  // < tot: the grid covers tot exactly
  const unsigned q0 = blk0 + threadIdx.x * 4u;  // group of 4 pixels of the flat index; < tot + 1024
  const int n = q0 >= tot ? 0 : (tot - q0 < 4u ? (int)(tot - q0) : 4);
  int cls[4] = {0, 0, 0, 0};
  int img[4] = {-1, -1, -1, -1};  // image of each pixel; -1: past the end, counted nowhere
  float e[4] = {0.f, 0.f, 0.f, 0.f};
  if (n > 0) {
    if constexpr (VEC) {  // H * W % 4 == 0: n == 4 and the group lies in one image
      const unsigned b = q0 / HW, p = q0 - b * HW;
      const float* f = a.fw + (size_t)b * 2 * HW + p;
      const float4 U = *reinterpret_cast<const float4*>(f);
      const float4 V = *reinterpret_cast<const float4*>(f + a.HW);
      const float u[4] = {U.x, U.y, U.z, U.w}, v[4] = {V.x, V.y, V.z, V.w};
      const float* bw = a.bw + (size_t)b * 2 * HW;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cls[j] = fb_pixel(a, bw, p + j, u[j], v[j], e[j]);
        img[j] = (int)b;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          const unsigned q = q0 + j;
          const unsigned b = q / HW, p = q - b * HW;
          const float* f = a.fw + (size_t)b * 2 * HW + p;
          cls[j] = fb_pixel(a, a.bw + (size_t)b * 2 * HW, p, f[0], f[HW], e[j]);
          img[j] = (int)b;
        }
      }
    }
    if (n == 4) {  // q0 is a multiple of 4: dword / 16-byte aligned from aligned bases
      *reinterpret_cast<unsigned*>(a.occ + q0) =
          (unsigned)cls[0] | (unsigned)cls[1] << 8 | (unsigned)cls[2] << 16 | (unsigned)cls[3] << 24;
      *reinterpret_cast<float4*>(a.err2 + q0) = make_float4(e[0], e[1], e[2], e[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < n) {
          a.occ[q0 + j] = (unsigned char)cls[j];
          a.err2[q0 + j] = e[j];
        }
    }
  }
  // counts: the images this block touches (block-uniform bounds, so every thread takes part)
  const unsigned blk_last = (tot - blk0 > 1024u ? blk0 + 1024u : tot) - 1u;
  const int b_lo = (int)(blk0 / HW), b_hi = (int)(blk_last / HW);
  for (int b = b_lo, it = 0; b <= b_hi; ++b, ++it) {
    int c = 0;  // class 1 in the low half, class 2 in the high half: at most 1024 each
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (img[j] == b) c += cls[j] == 1 ? 1 : (cls[j] == 2 ? 1 << 16 : 0);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, kWave);
    int* pt = part[it & 1];  // alternating buffers: one barrier per image
    if ((threadIdx.x & 63) == 0) pt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
      c = (pt[0] + pt[1]) + (pt[2] + pt[3]);
      if (c & 0xffff) atomicAdd(a.counts + 2 * b, c & 0xffff);
      if (c >> 16) atomicAdd(a.counts + 2 * b + 1, c >> 16);
    }
  }
}

}  // namespace

hipError_t launch_fb_consistency(const FbConsistencyArgs& a, hipStream_t s) {
  const long tot = (long)a.B * a.HW;
  if (tot == 0) return hipSuccess;
  if (tot >= (1L << 31) || a.HW != (long)a.H * a.W) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a.occ) & 3) || (reinterpret_cast<uintptr_t>(a.err2) & 15))
    return hipErrorInvalidValue;
  RAFT_HIP_CHECK(hipMemsetAsync(a.counts, 0, (size_t)a.B * 2 * sizeof(int), s));
  const dim3 grid((unsigned)((tot + 1023) / 1024));
  if (a.HW % 4 == 0 && (reinterpret_cast<uintptr_t>(a.fw) & 15) == 0)
    hipLaunchKernelGGL(fb_consistency_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(fb_consistency_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
