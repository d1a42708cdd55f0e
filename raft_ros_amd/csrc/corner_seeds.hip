// Corner seeds: the Shi-Tomasi corner of every cell of the point tracker's grid, in integers.
//
// Per image of frames (B, H, W, 3) uint8, the roi being the pixels [0, w) x [0, h):
//   g  = (c0 + 2 c1 + c2 + 2) >> 2
//   Ix = (g[y-1,x+1] + 2 g[y,x+1] + g[y+1,x+1]) - (the same at x-1), Iy the same across rows, every
//        coordinate clamped into the image
//   a, b, c = the sums of Ix^2, Ix Iy, Iy^2 over the 3 x 3 window, the gradients taken at clamped
//        coordinates (the gradient *of the clamped pixel*, not a gradient formed from clamped grays)
//   score = (a + c) - isqrt((a - c)^2 + 4 b^2), the exact integer floor of the root: the double
//        root, floored, then corrected by two integer compares, so that no rounding of a library
//        root reaches the result.  0 <= score <= 18 727 200.
//   a candidate of cell (y / S, x / S) is a roi pixel whose offsets in the cell lie in
//        [margin, S - 1 - margin]; a cell's winner has the largest score, then the lowest y * w + x.
// ops/corners.py holds the same sequence in integer torch ops (corner_seeds_ref); the two agree
// bitwise.
//
// Three launches, no host read-back: the fill of the per-cell keys (a kernel, not a memset node,
// for the reason at the top of track_points.hip), the score pass and the decode.
//
// Score pass: a workgroup of 256 threads takes a tile of 64 x 16 roi pixels.
//   1. the bytes of the 20 halo rows (68 pixels, 204 bytes at most) go to LDS as they lie in
//      memory: LDS dword k of a row is the aligned global dword k of that row's span, loaded as a
//      dword when it lies inside the span and byte by byte at the two ends.  Nothing outside the
//      span [3 xa, 3 xb + 3) of a row is read.
//   2. gray of the 68 x 20 halo (clamped coordinates) from the LDS bytes, one int each.
//   3. (Ix, Iy) of the 66 x 18 gradient halo, once per pixel, packed as two int16 (|I| <= 1020).
//      The gradient of a halo pixel outside the image is that of the clamped pixel, whose own
//      3 x 3 grays lie inside the gray halo.
//   4. a wave takes 4 rows of 64 pixels: lane = column, so every LDS read has stride 1 over the
//      lanes (no bank conflict); the 6 gradient rows are summed along x once and serve 4 windows.
//   5. argmax: the rows of a wave that share a cell row are combined in registers, the lanes
//      that share a cell by a segmented shuffle reduction, and the first lane of every cell
//      issues one 64-bit atomicMax of score << 32 | (0xffffffff - (y * w + x)): the largest score
//      wins, then the lowest index, whatever the order of arrival.
#include "common.h"

namespace raft_amd {
namespace {

constexpr int kTX = 64, kTY = 16;               // output tile
constexpr int kGW = kTX + 4, kGH = kTY + 4;     // gray halo
constexpr int kDW = kTX + 2, kDH = kTY + 2;     // gradient halo
constexpr int kRawDw = (3 + 3 * kGW + 3) / 4;   // dwords of a halo row's bytes, any misalignment: 52
constexpr int kRows = kTY / 4;                  // rows per wave

__global__ __launch_bounds__(256) void corner_clear_kernel(unsigned long long* __restrict__ keys, unsigned n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) keys[i] = 0ull;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// exact floor(sqrt(d)) for 0 <= d < 2^53
__device__ __forceinline__ long long isqrt53(long long d) {
  long long r = (long long)__builtin_floor(__builtin_sqrt((double)d));
  if (r * r > d) r -= 1;
  if ((r + 1) * (r + 1) <= d) r += 1;
  return r;
}

// The lanes of a wave hold keys of the cells gx of one cell row; gx does not decrease with the
// lane.  The first lane of every run of equal gx gets the run's largest key and, when that is
// not 0, puts it into row[gx].  Every lane of the wave takes part.
__device__ __forceinline__ void flush_keys(unsigned long long key, int gx, unsigned long long* __restrict__ row) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_down(key, off, 64);
    const int og = __shfl_down(gx, off, 64);
    if (lane + off < 64 && og == gx && o > key) key = o;
  }
  const int pg = __shfl_up(gx, 1, 64);
  if ((lane == 0 || pg != gx) && key != 0ull) atomicMax(row + gx, key);  // key != 0: gx < Gx
}

__global__ __launch_bounds__(256) void corner_score_kernel(CornerSeedsArgs a) {
  __shared__ uint32_t raw[kGH * kRawDw];
  __shared__ int gray[kGH * kGW];
  __shared__ uint32_t grad[kDH * kDW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, b = blockIdx.z;  // x0 < w <= W, y0 < h <= H
  const int H = a.H, W = a.W;
  const size_t pitch = (size_t)3 * W;
  const unsigned char* img = a.frames + (size_t)b * H * pitch;
  // the pixels of a halo row that lie in the image: [xa, xb], nb bytes from byte 3 xa of the row
  const int xa = max(x0 - 2, 0), xb = min(x0 + kTX + 1, W - 1);
  const int nb = 3 * (xb - xa + 1);

  // 1. the rows' bytes
  unsigned char* raw8 = reinterpret_cast<unsigned char*>(raw);
  for (int i = tid; i < kGH * kRawDw; i += 256) {
    const int ly = i / kRawDw, k = i - ly * kRawDw;
    const int cy = clampi(y0 - 2 + ly, 0, H - 1);
    const unsigned char* p0 = img + (size_t)cy * pitch + 3 * xa;
    const int mis = (int)(reinterpret_cast<uintptr_t>(p0) & 3u);
    const int lo = 4 * k - mis;  // the dword's first byte, relative to p0
    if (lo >= 0 && lo + 4 <= nb) {
      raw[i] = *reinterpret_cast<const uint32_t*>(p0 + lo);  // aligned: p0 - mis is
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = lo + j;
        if (o >= 0 && o < nb) raw8[4 * i + j] = p0[o];
      }
    }
  }
  __syncthreads();

  // 2. gray at clamped coordinates
  for (int i = tid; i < kGH * kGW; i += 256) {
    const int ly = i / kGW, lx = i - ly * kGW;
    const int cy = clampi(y0 - 2 + ly, 0, H - 1), cx = clampi(x0 - 2 + lx, 0, W - 1);  // cx in [xa, xb]
    const int mis = (int)(reinterpret_cast<uintptr_t>(img + (size_t)cy * pitch + 3 * xa) & 3u);
    const unsigned char* px = raw8 + 4 * ly * kRawDw + mis + 3 * (cx - xa);
    gray[i] = ((int)px[0] + 2 * (int)px[1] + (int)px[2] + 2) >> 2;
  }
  __syncthreads();

  // 3. the gradient of every pixel of the gradient halo, taken at the clamped pixel
  for (int i = tid; i < kDH * kDW; i += 256) {
    const int ly = i / kDW, lx = i - ly * kDW;
    // the clamped pixel in gray-halo coordinates: in [1, kGH - 2] x [1, kGW - 2]
    const int gy = clampi(y0 - 1 + ly, 0, H - 1) - (y0 - 2), gx = clampi(x0 - 1 + lx, 0, W - 1) - (x0 - 2);
    const int* g = gray + gy * kGW + gx;
    const int nw = g[-kGW - 1], n = g[-kGW], ne = g[-kGW + 1];
    const int we = g[-1], ea = g[1];
    const int sw = g[kGW - 1], s = g[kGW], se = g[kGW + 1];
    const int ix = (ne + 2 * ea + se) - (nw + 2 * we + sw);
    const int iy = (sw + 2 * s + se) - (nw + 2 * n + ne);
    grad[i] = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
  }
  __syncthreads();

  // 4. and 5.
  const int lane = tid & 63, wv = tid >> 6;
  const int x = x0 + lane;
  const int S = a.S;
  const int gx = x / S;
  const int ox = x - gx * S;
  const bool xcand = x < a.w && ox >= a.margin && ox <= S - 1 - a.margin;
  // the sums along x of the 6 gradient rows this wave's 4 windows read
  int ra[kRows + 2], rb[kRows + 2], rc[kRows + 2];
#pragma unroll
  for (int r = 0; r < kRows + 2; ++r) {
    const uint32_t* gr = grad + (wv * kRows + r) * kDW + lane;
    int sa = 0, sb = 0, sc = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const uint32_t v = gr[d];
      const int ix = (int)(short)(v & 0xffffu), iy = (int)(short)(v >> 16);
      sa += ix * ix;
      sb += ix * iy;
      sc += iy * iy;
    }
    ra[r] = sa;
    rb[r] = sb;
    rc[r] = sc;
  }
  unsigned long long* keys = a.keys + (size_t)b * a.N;
  unsigned long long best = 0ull;
  int cur_gy = -1;  // uniform over the wave, like y
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int y = y0 + wv * kRows + r;
    if (y >= a.h) break;
    const int gy = y / S;
    const int oy = y - gy * S;
    if (gy != cur_gy) {
      if (cur_gy >= 0) flush_keys(best, gx, keys + (size_t)cur_gy * a.Gx);
      best = 0ull;
      cur_gy = gy;
    }
    if (xcand && oy >= a.margin && oy <= S - 1 - a.margin) {
      const long long sa = ra[r] + ra[r + 1] + ra[r + 2];  // <= 9 * 1020^2
      const long long sb = rb[r] + rb[r + 1] + rb[r + 2];
      const long long sc = rc[r] + rc[r + 1] + rc[r + 2];
      const long long d = (sa - sc) * (sa - sc) + 4 * sb * sb;  // < 2^53
      const long long score = (sa + sc) - isqrt53(d);           // in [0, 2^25)
      const unsigned long long key =
          (unsigned long long)score << 32 | (unsigned long long)(0xffffffffu - (unsigned)(y * a.w + x));
      if (key > best) best = key;
    }
  }
  if (cur_gy >= 0) flush_keys(best, gx, keys + (size_t)cur_gy * a.Gx);
}

__global__ __launch_bounds__(256) void corner_decode_kernel(CornerSeedsArgs a) {
  const unsigned tot = (unsigned)a.B * (unsigned)a.N;  // < 2^31 (checked by the launcher)
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= tot) return;
  const int cell = (int)(i % (unsigned)a.N);
  const unsigned long long key = a.keys[i];
  const long long score = (long long)(key >> 32);
  int sx, sy;
  if (key != 0ull && score > a.min_score) {
    const unsigned idx = 0xffffffffu - (unsigned)(key & 0xffffffffull);
    sy = (int)(idx / (unsigned)a.w);
    sx = (int)(idx - (unsigned)sy * (unsigned)a.w);
  } else {
    // the clamped centre of the cell, track_points' seed (64-bit: S may be huge)
    const int gy = cell / a.Gx, gx = cell - gy * a.Gx;
    const long cx = (long)gx * a.S + a.S / 2, cy = (long)gy * a.S + a.S / 2;
    sx = (int)(cx < a.w - 1 ? cx : a.w - 1);
    sy = (int)(cy < a.h - 1 ? cy : a.h - 1);
  }
  a.seeds[2 * (size_t)i] = (float)(a.left + sx);
  a.seeds[2 * (size_t)i + 1] = (float)(a.top + sy);
  a.score[i] = key != 0ull ? (int)score : -1;
}

}  // namespace

hipError_t launch_corner_seeds(const CornerSeedsArgs& a, hipStream_t s) {
  const long tot = (long)a.B * a.N;
  if (tot == 0) return hipSuccess;
  if (tot >= (1L << 31) || a.H < 1 || a.W < 1 || (long)a.H * a.W >= (1L << 31)) return hipErrorInvalidValue;
  if (a.S < 1 || a.w < 1 || a.h < 1 || a.w > a.W || a.h > a.H || a.margin < 0 || 2L * a.margin > (long)a.S - 1)
    return hipErrorInvalidValue;
  if (a.Gx != (a.w - 1) / a.S + 1 || a.Gy != (a.h - 1) / a.S + 1 || (long)a.Gx * a.Gy != a.N)
    return hipErrorInvalidValue;
  const unsigned tiles_y = (unsigned)((a.h + kTY - 1) / kTY);
  if (a.B > 65535 || tiles_y > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(corner_clear_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a.keys, (unsigned)tot);
  hipLaunchKernelGGL(corner_score_kernel, dim3((unsigned)((a.w + kTX - 1) / kTX), tiles_y, (unsigned)a.B), dim3(256),
                     0, s, a);
  hipLaunchKernelGGL(corner_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
