// Training augmentation of a padded uint8 batch as one op: colour jitter, occlusion eraser and the
// resize / flip / crop warp of data/augment.py (BatchAugmentor.apply is the same arithmetic in
// torch ops, the CPU path and the tests' oracle).
//
// One memset of a per-sample statistics buffer and three launches, no host read-back:
//   pass 1  for every pixel inside the sample's (h, w) region apply the jitter rounds that precede
//           the contrast round of that sample's order and sum the luma.  Symmetric samples sum both
//           images into slot 0 (PIL sees the pair stacked), asymmetric ones image 2 into slot 1.
//   pass 2  all four rounds with m = floor(mean + 0.5) from pass 1; the jittered pair is stored as
//           one packed dword per pixel (r | g << 8 | b << 16: values are integers after every
//           round's rounding) and image 2's three channel sums are accumulated for the eraser.
//   pass 3  every crop pixel is mapped back through flip, resize and crop to a source coordinate,
//           clamped to the region; four bilinear taps from the packed images and from the flow; an
//           image-2 tap inside an active eraser box reads floor(channel mean) instead.
// Pixels outside the region are never read or written.
//
// Sparse ground truth (KITTI, HD1K; augment_batch_sparse, BatchAugmentor._sparse_flow is the oracle):
// a sparse sample's flow is not interpolated.  Every region pixel with valid >= 1 is scattered to
// its rounded position in the resized map (kept strictly inside when resized, as the reference's
// resize_sparse_flow_map keeps 0 < x < w1), flipped horizontally and cropped; where several land
// on one crop pixel the largest row-major source index wins, the reference's last writer.  Pass 2
// visits every region pixel anyway and does the scatter for sparse samples: one integer atomicMax
// of source index + 1 into the winner buffer win, which lies behind the statistics and is zeroed
// by the same memset.  An integer maximum does not depend on the order of arrival.  (As a launch
// of its own the scatter was 3 % slower on the Sintel-stage mixture and 3 % faster on the KITTI
// stage, profiles/augment_bench.log: the launch count stays three.)  Pass 3 then
// skips a sparse sample's flow taps, reads its four winners and gathers their flow; the images of
// a sparse sample are computed like any other.  The dense op instantiates neither.
//
// Sums are integers: the luma of integer-valued channels is 0 or at least 0.114 and below 256, so
// luma * 2^27 is an exact integer below 2^35, and up to 2^27 of them fit a 64-bit sum.  Integer
// atomics are associative: the statistics, and with them the outputs, do not depend on the order
// of arrival.  The means are then taken in fp64.
//
// The jitter is fp32 in the order of the torch expressions, every multiply and add rounded on its
// own; x / 255 and h / 6 are IEEE divisions, % 1 is fmodf plus 1 when negative, and the uint8
// rounding is rintf (half to even) and a clamp.  The bilinear blend uses the weights of
// grid_sample, (1 - fy)(1 - fx) ..., on the unnormalised source coordinate itself: a sample's
// result does not depend on the padded size of the batch it is in.
#include "common.h"

// every step must round like the torch op sequence
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

constexpr double kLumaScale = 134217728.0;  // 2^27
constexpr int kStatLuma = 0;                // stats[b][0..1]: luma sums * 2^27 (pair or image 1, image 2)
constexpr int kStatChan = 2;                // stats[b][2..4]: channel sums of the jittered image 2

struct Rgb {
  float r, g, b;
};

__host__ __device__ __forceinline__ float q8(float x) { return fminf(fmaxf(rintf(x), 0.f), 255.f); }

__host__ __device__ __forceinline__ float luma(const Rgb& p) { return (p.r * 0.299f + p.g * 0.587f) + p.b * 0.114f; }

__host__ __device__ __forceinline__ float mod1(float x) {  // torch's x % 1.0
  const float m = fmodf(x, 1.f);
  return m < 0.f ? m + 1.f : m;
}

__host__ __device__ __forceinline__ Rgb hue_round(const Rgb& p, float f) {
  const float r = p.r / 255.f, g = p.g / 255.f, b = p.b / 255.f;
  const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
  const float d = mx - mn;
  const float s = mx > 0.f ? d / fmaxf(mx, 1e-8f) : 0.f;
  const float dd = fmaxf(d, 1e-8f);
  float h = mx == r ? (g - b) / dd : (mx == g ? 2.f + (b - r) / dd : 4.f + (r - g) / dd);
  h = d > 0.f ? mod1(h / 6.f) : 0.f;
  h = mod1(h + f);
  const float h6 = h * 6.f;
  const float fi = floorf(h6);
  const float fr = h6 - fi;
  const float v = mx;
  const float pp = v * (1.f - s), qq = v * (1.f - s * fr), tt = v * (1.f - s * (1.f - fr));
  const int i = (int)fi % 6;  // h in [0, 1]: fi in 0..6
  Rgb o;
  o.r = i == 0 || i == 5 ? v : (i == 1 ? qq : (i == 4 ? tt : pp));
  o.g = i == 0 ? tt : (i == 1 || i == 2 ? v : (i == 3 ? qq : pp));
  o.b = i == 0 || i == 1 ? pp : (i == 2 ? tt : (i == 5 ? qq : v));
  o.r = q8(o.r * 255.f);
  o.g = q8(o.g * 255.f);
  o.b = q8(o.b * 255.f);
  return o;
}

// one round of ColorJitter: op 0 brightness, 1 contrast (m = the rounded luma mean), 2 saturation, 3 hue
__host__ __device__ __forceinline__ Rgb jitter_round(const Rgb& p, int op, float f, float m) {
  Rgb o;
  switch (op) {
    case 0:
      o.r = q8(p.r * f);
      o.g = q8(p.g * f);
      o.b = q8(p.b * f);
      return o;
    case 1:
      o.r = q8(m + f * (p.r - m));
      o.g = q8(m + f * (p.g - m));
      o.b = q8(m + f * (p.b - m));
      return o;
    case 2: {
      const float g = q8(luma(p));
      o.r = q8(g + f * (p.r - g));
      o.g = q8(g + f * (p.g - g));
      o.b = q8(g + f * (p.b - g));
      return o;
    }
    default:
      return hue_round(p, f);
  }
}

// The jitter of one pixel.  FULL: all four rounds with the contrast mean m.  Otherwise the rounds
// in front of the contrast round only: what the contrast round's luma mean is taken over.
template <bool FULL>
__host__ __device__ __forceinline__ Rgb jitter_pixel(Rgb p, const float* f, const int* o, float m) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = o[k] & 3;
    if (!FULL && op == 1) break;
    p = jitter_round(p, op, f[op], m);
  }
  return p;
}

__host__ __device__ __forceinline__ int clampi(long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// the contrast round's m of a sample: floor(mean luma + 0.5), the mean in fp64 from the exact sum
__host__ __device__ __forceinline__ float contrast_mean(long long sum, long count) {
  const double mean = (double)sum / kLumaScale / (double)(count < 1 ? 1 : count);
  return (float)floor(mean + 0.5);
}

__device__ __forceinline__ Rgb load_rgb(const unsigned char* p) {
  Rgb c;
  c.r = (float)p[0];
  c.g = (float)p[1];
  c.b = (float)p[2];
  return c;
}

// block sum of N 64-bit integers per thread, then one atomic per non-zero sum from thread 0
template <int N>
__device__ __forceinline__ void block_atomic_sum(long long (&v)[N], long long* dst) {
  __shared__ long long part[4][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off, kWave);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const long long s = (part[0][i] + part[1][i]) + (part[2][i] + part[3][i]);
      if (s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(dst + i), static_cast<unsigned long long>(s));
    }
  }
}

// what the scatter of a sparse sample needs of its drawn parameters
struct SparseMap {
  float sx, sy;
  int resize, hflip, rh, rw, x0, y0;
};

__device__ __forceinline__ SparseMap sparse_map(const AugmentArgs& a, int b) {
  const float* pf = a.pf + (long)b * kAugPF;
  const int* pi = a.pi + (long)b * kAugPI;
  SparseMap m;
  m.sx = pf[kAugSx];
  m.sy = pf[kAugSy];
  m.resize = (a.flags[b] & kAugResize) != 0;
  m.hflip = pi[kAugHflip] != 0;
  m.rh = pi[kAugRh];
  m.rw = pi[kAugRw];
  m.x0 = pi[kAugX0];
  m.y0 = pi[kAugY0];
  return m;
}

// Region pixel (x, y) at padded offset off of sparse sample b -> its crop pixel, if it has one:
// win = max(win, source index + 1).
__device__ __forceinline__ void scatter_pixel(const AugmentArgs& a, int b, const SparseMap& m, int x, int y, long off) {
  if (!(a.valid[off] >= 1.f)) return;  // a NaN is not valid
  long xn = x, yn = y;
  if (m.resize) {
    const float xf = rintf((float)x * m.sx), yf = rintf((float)y * m.sy);  // half to even, like torch.round
    if (!(xf > 0.f && yf > 0.f && xf < 2147483648.f && yf < 2147483648.f)) return;  // or a NaN
    xn = (long)xf;
    yn = (long)yf;
    if (xn >= m.rw || yn >= m.rh) return;
  }
  if (m.hflip) xn = (long)m.rw - 1 - xn;
  const long cx = xn - m.x0, cy = yn - m.y0;
  if (cx < 0 || cx >= a.cw || cy < 0 || cy >= a.ch) return;
  // inside (B, ch, cw); y * Wm + x + 1 <= Hm * Wm <= 2^26
  atomicMax(a.win + ((long)b * a.ch + cy) * a.cw + cx, y * a.Wm + x + 1);
}

// passes 1 and 2: grid (blocks, B), a block strides over the in-region pixels of its sample.
// SCATTER (pass 2 of augment_batch_sparse): the sparse samples' valid pixels are scattered too.
template <bool FULL, bool SCATTER = false>
__global__ __launch_bounds__(256) void augment_jitter_kernel(AugmentArgs a) {
  const int b = blockIdx.y;
  const int h = clampi(a.size[2 * b], 0, a.Hm), w = clampi(a.size[2 * b + 1], 0, a.Wm);
  const int n = h * w;  // <= Hm * Wm <= 2^26 (checked by the launcher)
  const float* pf = a.pf + (long)b * kAugPF;
  const int* pi = a.pi + (long)b * kAugPI;
  float f1[4], f2[4];
  int o1[4], o2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f1[k] = pf[kAugF1 + k];
    f2[k] = pf[kAugF2 + k];
    o1[k] = pi[kAugO1 + k];
    o2[k] = pi[kAugO2 + k];
  }
  const int slot2 = pi[kAugAsym] != 0 ? 1 : 0;
  long long* st = a.stats + (long)b * kAugStats;
  float m1 = 0.f, m2 = 0.f;
  if (FULL) {
    const long cnt = slot2 ? (long)n : 2L * n;
    m1 = contrast_mean(st[kStatLuma], cnt);
    m2 = contrast_mean(st[kStatLuma + slot2], cnt);
  }
  long long acc[3] = {0, 0, 0};
  const long base = (long)b * a.Hm * a.Wm;
  bool sp = false;
  SparseMap sm{};
  if constexpr (SCATTER) {
    sp = (a.flags[b] & kAugSparse) != 0;
    if (sp) sm = sparse_map(a, b);
  }
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n; p += gridDim.x * 256) {
    const int y = p / w, x = p - y * w;
    const long off = base + (long)y * a.Wm + x;  // in-region pixel: off < B * Hm * Wm
    if constexpr (SCATTER) {
      if (sp) scatter_pixel(a, b, sm, x, y, off);
    }
    const Rgb c1 = jitter_pixel<FULL>(load_rgb(a.img1 + 3 * off), f1, o1, m1);
    const Rgb c2 = jitter_pixel<FULL>(load_rgb(a.img2 + 3 * off), f2, o2, m2);
    if (FULL) {
      const unsigned r2 = (unsigned)c2.r, g2 = (unsigned)c2.g, b2 = (unsigned)c2.b;
      a.jit1[off] = (unsigned)c1.r | (unsigned)c1.g << 8 | (unsigned)c1.b << 16;
      a.jit2[off] = r2 | g2 << 8 | b2 << 16;
      acc[0] += r2;
      acc[1] += g2;
      acc[2] += b2;
    } else {
      const long long l1 = (long long)((double)luma(c1) * kLumaScale);
      const long long l2 = (long long)((double)luma(c2) * kLumaScale);
      acc[0] += slot2 ? l1 : l1 + l2;
      acc[1] += slot2 ? l2 : 0;
    }
  }
  if (FULL) {
    block_atomic_sum<3>(acc, st + kStatChan);
  } else {
    long long two[2] = {acc[0], acc[1]};
    block_atomic_sum<2>(two, st + kStatLuma);
  }
}

struct Tap {
  int i0, i1;    // the two taps, inside the region
  float w0, w1;  // their weights
};

// crop pixel c -> resized (flipped) pixel -> source coordinate, clamped to [0, n - 1]
__device__ __forceinline__ Tap source_tap(int c, int origin, int flip, int rn, float scale, int n) {
  float r = (float)origin + (float)c;
  if (flip) r = ((float)rn - 1.f) - r;
  const float s = fminf(fmaxf((r + 0.5f) / scale - 0.5f, 0.f), (float)n - 1.f);  // a NaN becomes 0
  const float fl = floorf(s);
  Tap t;
  t.w1 = s - fl;
  t.w0 = 1.f - t.w1;
  t.i0 = (int)fl;
  t.i1 = t.i0 + 1 < n ? t.i0 + 1 : n - 1;
  return t;
}

__device__ __forceinline__ float blend(float nw, float ne, float sw, float se, float wnw, float wne, float wsw,
                                       float wse) {
  return ((nw * wnw + ne * wne) + sw * wsw) + se * wse;
}

// pass 3: grid (blocks, B), a thread writes 4 consecutive pixels of one crop row.  SPARSE
// (augment_batch_sparse): a sparse sample's flow and valid come from its winners, not from taps.
template <bool VEC, bool SPARSE = false>
__global__ __launch_bounds__(256) void augment_warp_kernel(AugmentArgs a) {
  const int b = blockIdx.y;
  const int G = (a.cw + 3) >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.ch * G) return;
  const int y = t / G, xg = (t - y * G) * 4;
  const int n = a.cw - xg < 4 ? a.cw - xg : 4;
  const int h = clampi(a.size[2 * b], 0, a.Hm), w = clampi(a.size[2 * b + 1], 0, a.Wm);
  const float* pf = a.pf + (long)b * kAugPF;
  const int* pi = a.pi + (long)b * kAugPI;
  const float sx = pf[kAugSx], sy = pf[kAugSy];
  const int hflip = pi[kAugHflip] != 0, vflip = pi[kAugVflip] != 0;
  float o[9][4];  // img1 rgb, img2 rgb, flow uv, valid
#pragma unroll
  for (int c = 0; c < 9; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) o[c][j] = 0.f;
  if (h > 0 && w > 0) {  // an empty region has nothing to sample: zeros
    const int nbox = clampi(pi[kAugNbox], 0, 2);
    int bx[2], by[2], ex[2], ey[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      bx[k] = pi[kAugBox + 4 * k];
      by[k] = pi[kAugBox + 4 * k + 1];
      ex[k] = bx[k] + pi[kAugBox + 4 * k + 2];
      ey[k] = by[k] + pi[kAugBox + 4 * k + 3];
    }
    const long long* st = a.stats + (long)b * kAugStats + kStatChan;
    const long cnt = (long)h * w;
    // floor(mean) of integer sums: the integer quotient
    const unsigned fill = (unsigned)(st[0] / cnt) | (unsigned)(st[1] / cnt) << 8 | (unsigned)(st[2] / cnt) << 16;
    const Tap ty = source_tap(y, pi[kAugY0], vflip, pi[kAugRh], sy, h);
    const long base = (long)b * a.Hm * a.Wm;
    const long row0 = base + (long)ty.i0 * a.Wm, row1 = base + (long)ty.i1 * a.Wm;
    const float fu = hflip ? -1.f : 1.f, fv = vflip ? -1.f : 1.f;
    bool sp = false;
    if constexpr (SPARSE) sp = (a.flags[b] & kAugSparse) != 0;
    if constexpr (SPARSE) {
      if (sp) {
        const int* wp = a.win + (long)b * a.ch * a.cw + (long)y * a.cw + xg;
        int wv[4] = {0, 0, 0, 0};
        if constexpr (VEC) {  // cw % 4 == 0: the group is 16-byte aligned
          const int4 v4 = *reinterpret_cast<const int4*>(wp);
          wv[0] = v4.x;
          wv[1] = v4.y;
          wv[2] = v4.z;
          wv[3] = v4.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (j < n) wv[j] = wp[j];
        }
        const bool rs = (a.flags[b] & kAugResize) != 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (wv[j] > 0) {  // the winner's source index + 1: a region pixel of this sample
            const float2 f = *reinterpret_cast<const float2*>(a.flow + 2 * (base + (wv[j] - 1)));
            o[6][j] = (rs ? f.x * sx : f.x) * fu;
            o[7][j] = rs ? f.y * sy : f.y;  // no vertical flip for sparse samples
            o[8][j] = 1.f;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < n) {
        const Tap tx = source_tap(xg + j, pi[kAugX0], hflip, pi[kAugRw], sx, w);
        const float wnw = ty.w0 * tx.w0, wne = ty.w0 * tx.w1, wsw = ty.w1 * tx.w0, wse = ty.w1 * tx.w1;
        const long q[4] = {row0 + tx.i0, row0 + tx.i1, row1 + tx.i0, row1 + tx.i1};  // in-region pixels
        const int qx[4] = {tx.i0, tx.i1, tx.i0, tx.i1}, qy[4] = {ty.i0, ty.i0, ty.i1, ty.i1};
        unsigned c1[4], c2[4];
        float2 fl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          c1[k] = a.jit1[q[k]];
          c2[k] = a.jit2[q[k]];
          fl[k] = sp ? make_float2(0.f, 0.f) : *reinterpret_cast<const float2*>(a.flow + 2 * q[k]);
          bool er = false;
#pragma unroll
          for (int e = 0; e < 2; ++e)
            er |= e < nbox && qx[k] >= bx[e] && qx[k] < ex[e] && qy[k] >= by[e] && qy[k] < ey[e];
          if (er) c2[k] = fill;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int sh = 8 * c;
          o[c][j] = q8(blend((float)(c1[0] >> sh & 255u), (float)(c1[1] >> sh & 255u), (float)(c1[2] >> sh & 255u),
                             (float)(c1[3] >> sh & 255u), wnw, wne, wsw, wse));
          o[3 + c][j] = q8(blend((float)(c2[0] >> sh & 255u), (float)(c2[1] >> sh & 255u), (float)(c2[2] >> sh & 255u),
                                 (float)(c2[3] >> sh & 255u), wnw, wne, wsw, wse));
        }
        if (!sp) {
          const float u = blend(fl[0].x, fl[1].x, fl[2].x, fl[3].x, wnw, wne, wsw, wse) * sx * fu;
          const float v = blend(fl[0].y, fl[1].y, fl[2].y, fl[3].y, wnw, wne, wsw, wse) * sy * fv;
          o[6][j] = u;
          o[7][j] = v;
          o[8][j] = fabsf(u) < 1000.f && fabsf(v) < 1000.f ? 1.f : 0.f;
        }
      }
    }
  }
  const long plane = (long)a.ch * a.cw;
  const long at = (long)y * a.cw + xg;
  float* dst[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    dst[c] = a.out1 + ((long)b * 3 + c) * plane + at;
    dst[3 + c] = a.out2 + ((long)b * 3 + c) * plane + at;
  }
  dst[6] = a.oflow + (long)b * 2 * plane + at;
  dst[7] = dst[6] + plane;
  dst[8] = a.ovalid + (long)b * plane + at;
#pragma unroll
  for (int c = 0; c < 9; ++c) {
    if constexpr (VEC) {  // cw % 4 == 0: n == 4 and every row group is 16-byte aligned
      *reinterpret_cast<float4*>(dst[c]) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < n) dst[c][j] = o[c][j];
    }
  }
}
}  // namespace

hipError_t launch_augment_batch(const AugmentArgs& a, hipStream_t s) {
  if (a.B == 0 || a.ch == 0 || a.cw == 0) return hipSuccess;
  const long HW = (long)a.Hm * a.Wm;
  // 32-bit in-sample pixel index and exact 64-bit luma sums; grid.y is the batch
  if (a.B < 0 || a.B > 65535 || a.Hm < 0 || a.Wm < 0 || HW > (1L << 26) || a.ch < 0 || a.cw < 0 ||
      (long)a.ch * a.cw >= (1L << 31))
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a.flow) & 7) || (reinterpret_cast<uintptr_t>(a.out1) & 15) ||
      (reinterpret_cast<uintptr_t>(a.out2) & 15) || (reinterpret_cast<uintptr_t>(a.oflow) & 15) ||
      (reinterpret_cast<uintptr_t>(a.ovalid) & 15))
    return hipErrorInvalidValue;
  // sparse ground truth: all three pointers or none; win directly behind stats, so that the one
  // memset zeroes both
  const bool sparse = a.valid != nullptr || a.flags != nullptr || a.win != nullptr;
  size_t zero = (size_t)a.B * kAugStats * sizeof(long long);
  if (sparse) {
    if (a.valid == nullptr || a.flags == nullptr || a.win != reinterpret_cast<int*>(a.stats + (long)a.B * kAugStats) ||
        (reinterpret_cast<uintptr_t>(a.win) & 15))
      return hipErrorInvalidValue;
    zero += (size_t)a.B * a.ch * a.cw * sizeof(int);
  }
  RAFT_HIP_CHECK(hipMemsetAsync(a.stats, 0, zero, s));
  if (HW > 0) {
    const dim3 grid((unsigned)(HW + 255) / 256 < 1024u ? (unsigned)(HW + 255) / 256 : 1024u, (unsigned)a.B);
    hipLaunchKernelGGL(augment_jitter_kernel<false>, grid, dim3(256), 0, s, a);
    if (sparse)
      hipLaunchKernelGGL((augment_jitter_kernel<true, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(augment_jitter_kernel<true>, grid, dim3(256), 0, s, a);
  }
  const long groups = (long)a.ch * ((a.cw + 3) >> 2);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)a.B);
  if (sparse) {
    if (a.cw % 4 == 0)
      hipLaunchKernelGGL((augment_warp_kernel<true, true>), grid, dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL((augment_warp_kernel<false, true>), grid, dim3(256), 0, s, a);
  } else if (a.cw % 4 == 0) {
    hipLaunchKernelGGL(augment_warp_kernel<true>, grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL(augment_warp_kernel<false>, grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace raft_amd
