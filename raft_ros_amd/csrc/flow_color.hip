// Device-side frame path: what the ROS node and demo.py do around the model.
//
// flow_to_image: the Middlebury colour coding of utils/flow_viz.py (reference
// core/utils/flow_viz.py) of a (B, 2, H, W) fp32 flow, each image normalised by its own
// largest radius.  One memset of the B maxima and two launches, no host read-back:
//   radmax: rad = sqrt(u^2 + v^2) per pixel, wave + block maximum, one atomicMax per block on
//           the bit pattern (non-negative floats order like their bits; a maximum does not
//           depend on the order of its operands, so the result is deterministic).
//   color:  u, v / (rad_max + 1e-5), the radius again from the normalised components, the
//           angle -> position on the 55-entry wheel, blend of the two neighbouring hues,
//           desaturation (rad <= 1) or dimming by 0.75, floor(255 * col), packed RGB / BGR.
// The arithmetic follows numpy's, type by type: everything up to the wheel position ``fk`` is
// fp32 there (true divisions, separate multiply and add, signed zeros kept); ``fk - k0`` mixes
// fp32 with int32 and is float64 from there on, and so is the blend here.  The wheel is stored
// already divided by 255.0 (a double division at compile time, the one numpy does per pixel).
// What is left to differ is the last bit of atan2f.
//
// Each thread colours 4 consecutive pixels of the flat (B * H * W) pixel index and writes
// their 12 bytes as 3 dwords: such a group is 12-byte aligned whatever H * W is, it may
// straddle two images (each pixel looks up its own image's maximum), and the last group may
// be short (byte stores).  Loads are float4 when H * W is a multiple of 4.
//
// ingest_frames: uint8 (N, H, W, 3) -> fp32 (N, 3, Hp, Wp) with replicate padding in one
// launch; 4 output pixels of a row per thread, float4 stores when Wp is a multiple of 4.
#include <algorithm>

#include "common.h"

// the radius must round like numpy's separate multiply and add
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

constexpr int kNCols = 55;
constexpr float kPiF = 3.14159274101257324f;  // float32(np.pi): ``arctan2(...) / np.pi`` on an fp32 array

struct Wheel {
  double v[kNCols * 3];
};

// make_colorwheel() / 255.0: segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; in each, one
// channel ramps (floor(255 * i / n)) up or down between a saturated and an empty one
constexpr Wheel make_wheel() {
  Wheel w{};
  const int seg[6] = {15, 6, 4, 11, 13, 6};
  int k = 0;
  for (int s = 0; s < 6; ++s) {
    for (int i = 0; i < seg[s]; ++i, ++k) {
      const double up = (double)((255 * i) / seg[s]), down = 255.0 - up;
      double r = 0.0, g = 0.0, b = 0.0;
      switch (s) {
        case 0: r = 255.0; g = up; break;
        case 1: r = down; g = 255.0; break;
        case 2: g = 255.0; b = up; break;
        case 3: g = down; b = 255.0; break;
        case 4: r = up; b = 255.0; break;
        default: r = 255.0; b = down; break;
      }
      w.v[3 * k + 0] = r / 255.0;
      w.v[3 * k + 1] = g / 255.0;
      w.v[3 * k + 2] = b / 255.0;
    }
  }
  return w;
}

__constant__ Wheel kWheel = make_wheel();

// np.clip(x, 0, c): -0.0 and NaN pass through
__device__ __forceinline__ float clip0(float x, float c) { return x < 0.f ? 0.f : (x > c ? c : x); }

__device__ __forceinline__ float radius(const FlowColorArgs& a, float u, float v) {
  if (a.has_clip) {
    u = clip0(u, a.clip);
    v = clip0(v, a.clip);
  }
  return sqrtf(u * u + v * v);
}

template <bool VEC>
__global__ __launch_bounds__(256) void flow_radmax_kernel(FlowColorArgs a) {
  __shared__ float part[4];
  const int b = blockIdx.y;
  const float* u = a.flow + (long)b * 2 * a.HW;
  const float* v = u + a.HW;
  float m = 0.f;  // radii are >= +0; fmaxf drops a NaN
  if constexpr (VEC) {
    for (long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4; i < a.HW; i += (long)gridDim.x * 1024) {
      const float4 U = *reinterpret_cast<const float4*>(u + i);
      const float4 V = *reinterpret_cast<const float4*>(v + i);
      m = fmaxf(fmaxf(m, radius(a, U.x, V.x)), radius(a, U.y, V.y));
      m = fmaxf(fmaxf(m, radius(a, U.z, V.z)), radius(a, U.w, V.w));
    }
  } else {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < a.HW; i += (long)gridDim.x * 256)
      m = fmaxf(m, radius(a, u[i], v[i]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
    atomicMax(a.rad_max + b, __float_as_uint(m));
  }
}

// one pixel: (u, v) and the normaliser rad_max + eps -> 3 bytes in output channel order
__device__ __forceinline__ void color_pixel(const FlowColorArgs& a, const double* __restrict__ wheel, float u, float v,
                                            float nrm, unsigned char* px) {
  if (a.has_clip) {
    u = clip0(u, a.clip);
    v = clip0(v, a.clip);
  }
  u = u / nrm;
  v = v / nrm;
  const float rad = sqrtf(u * u + v * v);
  const float ang = atan2f(-v, -u) / kPiF;
  const float fk = (ang + 1.f) / 2.f * (float)(kNCols - 1);
  // finite flow gives 0 <= fk <= 54; anything else (NaN compares false) is clamped into the wheel
  const int k0 = fk >= 0.f ? (fk < (float)(kNCols - 1) ? (int)floorf(fk) : kNCols - 1) : 0;
  const int k1 = k0 + 1 == kNCols ? 0 : k0 + 1;
  const double frac = (double)fk - (double)k0;
  const bool inside = rad <= 1.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double c0 = wheel[3 * k0 + ch], c1 = wheel[3 * k1 + ch];
    double col = (1.0 - frac) * c0 + frac * c1;
    col = inside ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
    const double t = floor(255.0 * col);
    const int level = t >= 0.0 ? (t <= 255.0 ? (int)t : 255) : 0;  // NaN -> 0
    px[a.bgr ? 2 - ch : ch] = (unsigned char)level;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void flow_color_kernel(FlowColorArgs a) {
  __shared__ double wheel[kNCols * 3];
  for (int i = threadIdx.x; i < kNCols * 3; i += 256) wheel[i] = kWheel.v[i];
  __syncthreads();
  const long tot = (long)a.B * a.HW;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;  // group of 4 pixels of the flat index
  const long q0 = g * 4;
  if (q0 >= tot) return;
  const int n = tot - q0 < 4 ? (int)(tot - q0) : 4;
  float u[4], v[4], nrm[4];
  if constexpr (VEC) {  // H * W % 4 == 0: the group lies in one image, 16-byte aligned
    const long b = q0 / a.HW, p = q0 - b * a.HW;
    const float* f = a.flow + b * 2 * a.HW + p;
    const float4 U = *reinterpret_cast<const float4*>(f);
    const float4 V = *reinterpret_cast<const float4*>(f + a.HW);
    u[0] = U.x, u[1] = U.y, u[2] = U.z, u[3] = U.w;
    v[0] = V.x, v[1] = V.y, v[2] = V.z, v[3] = V.w;
    nrm[0] = nrm[1] = nrm[2] = nrm[3] = __uint_as_float(a.rad_max[b]) + 1e-5f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long q = q0 + j < tot ? q0 + j : tot - 1;  // past the end: repeat the last pixel, never stored
      const long b = q / a.HW, p = q - b * a.HW;
      const float* f = a.flow + b * 2 * a.HW + p;
      u[j] = f[0];
      v[j] = f[a.HW];
      nrm[j] = __uint_as_float(a.rad_max[b]) + 1e-5f;
    }
  }
  unsigned char px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) color_pixel(a, wheel, u[j], v[j], nrm[j], px + 3 * j);
  if (n == 4) {
    unsigned* o = reinterpret_cast<unsigned*>(a.img) + 3 * g;  // byte 12 * g of a 4-byte aligned base
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o[k] = (unsigned)px[4 * k] | (unsigned)px[4 * k + 1] << 8 | (unsigned)px[4 * k + 2] << 16 |
             (unsigned)px[4 * k + 3] << 24;
  } else {
    unsigned char* o = a.img + 3 * q0;
#pragma unroll
    for (int k = 0; k < 9; ++k)
      if (k < 3 * n) o[k] = px[k];
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void ingest_frames_kernel(IngestArgs a) {
  const int Wq = (a.Wp + 3) / 4;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)a.N * a.Hp * Wq) return;
  const int xq = (int)(idx % Wq);
  const long t = idx / Wq;
  const int y = (int)(t % a.Hp), n = (int)(t / a.Hp);
  const int sy = min(max(y - a.pt, 0), a.H - 1);
  const unsigned char* row = a.in + ((long)n * a.H + sy) * a.W * 3;
  float c[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // a column past Wp (last group of a row) clamps to a valid source and is not stored
    const int sx = min(max(xq * 4 + j - a.pl, 0), a.W - 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch][j] = (float)row[sx * 3 + ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* o = a.out + (((long)n * 3 + ch) * a.Hp + y) * a.Wp + xq * 4;
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(o) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xq * 4 + j < a.Wp) o[j] = c[ch][j];
    }
  }
}

}  // namespace

hipError_t launch_flow_to_image(const FlowColorArgs& a, hipStream_t s) {
  const long tot = (long)a.B * a.HW;
  if (tot == 0) return hipSuccess;
  if (reinterpret_cast<uintptr_t>(a.img) & 3) return hipErrorInvalidValue;
  RAFT_HIP_CHECK(hipMemsetAsync(a.rad_max, 0, (size_t)a.B * sizeof(unsigned), s));
  const bool vec = a.HW % 4 == 0 && (reinterpret_cast<uintptr_t>(a.flow) & 15) == 0;
  // up to 1024 pixels per block and pass of the grid-stride loop; at most 256 blocks an image
  const dim3 rgrid((unsigned)std::min(256L, (a.HW + 1023) / 1024), (unsigned)a.B);
  if (vec)
    hipLaunchKernelGGL(flow_radmax_kernel<true>, rgrid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(flow_radmax_kernel<false>, rgrid, dim3(256), 0, s, a);
  RAFT_HIP_CHECK(hipGetLastError());
  const dim3 cgrid((unsigned)((tot + 1023) / 1024));
  if (vec)
    hipLaunchKernelGGL(flow_color_kernel<true>, cgrid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(flow_color_kernel<false>, cgrid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_ingest_frames(const IngestArgs& a, hipStream_t s) {
  const long groups = (long)a.N * a.Hp * ((a.Wp + 3) / 4);
  if (groups == 0) return hipSuccess;
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (a.Wp % 4 == 0 && (reinterpret_cast<uintptr_t>(a.out) & 15) == 0)
    hipLaunchKernelGGL(ingest_frames_kernel<true>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(ingest_frames_kernel<false>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
