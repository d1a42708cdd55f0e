// Point tracks: a grid of points, one per cell of the roi, advanced by one pair's flow.
//
// The roi (left, top, w, h) of the (H, W) frame is tiled by Gy x Gx cells of size S; an image
// holds N = Gy * Gx slots, one point each, and after every call every cell holds exactly one
// point.  All arithmetic is fp32, every multiply and add rounded on its own; ops/track.py holds
// the same sequence in torch ops (track_points_ref) and the two agree bitwise.
//
// Phase 1 (one thread per slot):
//   p = pos; outside the roi (NaN counts as outside): status 2, err2 = +inf
//   f = fw read bilinearly at p (the formula of fb_consistency.hip's fb_pixel), q = p + f
//   q outside the roi: status 2, err2 = +inf
//   with bw: s = bw read bilinearly at q, err2 = (f0 + s0)^2 + (f1 + s1)^2, status 1 unless
//            err2 <= alpha1 ((f0^2 + f1^2) + (s0^2 + s1^2)) + alpha2 (NaN -> 1); without: err2 = 0
//   a survivor claims the cell of q: one 64-bit atomicMin of (0xffffffff - age) << 32 | slot into
//   the key of that cell (all ones = unclaimed): the oldest point wins, among equal ages the
//   lowest slot, whatever the order of arrival.
// Phase 2 (one workgroup per image, looping over N in chunks of the block size):
//   a survivor that owns its cell: status 0, pos_out = q, prev = p, id kept, age + 1; any other
//   survivor: status 3.  The slots whose status is not 0 are as many as the unowned cells: the
//   k-th such slot in slot order takes the k-th unowned cell in cell order (two exclusive scans),
//   pos_out = the seed of that cell (seeds[b, cell] when the caller gives seeds, else the cell's
//   clamped centre), prev = NaN, id = epoch * N + slot, age = 0.
//   counts[b] = the slots per status, from integer sums in LDS.
// epoch_out = epoch + 1 is written by one thread of phase 1, which reads epoch nowhere else.
//
// Three launches, no host read-back: the fill of the keys and the two phases.  The fill is a
// kernel, not a memset: captured into a graph with the op's other work, a memset node of this size
// (8 bytes a slot) filled the array with other values from the second replay on, while the same
// three nodes replayed alone were right every time; a fill kernel replays like any other launch.
//
// Every flow read is clamped into the frame: p and q are tested inside the roi, which lies inside
// the frame, before their floor is taken, so NaN never reaches a float-to-int conversion and every
// cell index is in [0, N).
#include "common.h"

// every step must round like the torch op sequence
#pragma clang fp contract(off)

namespace raft_amd {
namespace {

constexpr int kTrackBlock2 = 1024;  // phase 2: one workgroup per image
constexpr unsigned long long kNoClaim = ~0ull;

__device__ __forceinline__ bool in_roi(const TrackPointsArgs& a, float x, float y) {
  return x >= (float)a.left && x <= (float)(a.left + a.w - 1) && y >= (float)a.top && y <= (float)(a.top + a.h - 1);
}

// both components of the flow f (2, H, W) read bilinearly at (x, y) inside the frame
__device__ __forceinline__ void flow_at(const TrackPointsArgs& a, const float* __restrict__ f, float x, float y,
                                        float out[2]) {
  const float x0f = floorf(x), y0f = floorf(y);
  const float fx = x - x0f, fy = y - y0f;
  const int x0 = (int)x0f, y0 = (int)y0f;  // in [0, W-1] x [0, H-1]: inside
  const int x1 = min(x0 + 1, a.W - 1), y1 = min(y0 + 1, a.H - 1);
  const float* r0 = f + (long)y0 * a.W;
  const float* r1 = f + (long)y1 * a.W;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float a00 = r0[c * a.HW + x0], a01 = r0[c * a.HW + x1];
    const float a10 = r1[c * a.HW + x0], a11 = r1[c * a.HW + x1];
    const float top = a00 + fx * (a01 - a00);
    const float bot = a10 + fx * (a11 - a10);
    out[c] = top + fy * (bot - top);
  }
}

// the cell of a point inside the roi
__device__ __forceinline__ int cell_of(const TrackPointsArgs& a, float x, float y) {
  return (((int)floorf(y) - a.top) / a.S) * a.Gx + ((int)floorf(x) - a.left) / a.S;
}

__global__ __launch_bounds__(256) void track_clear_kernel(unsigned long long* __restrict__ keys, unsigned n) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) keys[i] = kNoClaim;
}

__global__ __launch_bounds__(256) void track_phase1_kernel(TrackPointsArgs a) {
  // B * N < 2^31 (checked by the launcher)
  const unsigned N = (unsigned)a.N, tot = (unsigned)a.B * N;
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i == 0) *a.epoch_out = *a.epoch + 1;
  if (i >= tot) return;
  const unsigned b = i / N, slot = i - b * N;
  const float px = a.pos[2 * (size_t)i], py = a.pos[2 * (size_t)i + 1];
  int st = 2;
  float e = __builtin_inff(), qx = px, qy = py;
  if (in_roi(a, px, py)) {
    float f[2];
    flow_at(a, a.fw + (size_t)b * 2 * a.HW, px, py, f);
    qx = px + f[0];
    qy = py + f[1];
    if (in_roi(a, qx, qy)) {
      if (a.bw != nullptr) {
        float s[2];
        flow_at(a, a.bw + (size_t)b * 2 * a.HW, qx, qy, s);
        const float du = f[0] + s[0], dv = f[1] + s[1];
        e = du * du + dv * dv;
        const float thr = a.alpha1 * ((f[0] * f[0] + f[1] * f[1]) + (s[0] * s[0] + s[1] * s[1])) + a.alpha2;
        st = e <= thr ? 0 : 1;
      } else {
        e = 0.f;
        st = 0;
      }
      if (st == 0) {
        const int cell = cell_of(a, qx, qy);  // in [0, N): q is inside the roi
        const unsigned long long key = (unsigned long long)(0xffffffffu - (unsigned)a.age[i]) << 32 | slot;
        atomicMin(a.keys + (size_t)b * N + cell, key);
      }
    }
  }
  a.status[i] = (unsigned char)st;
  a.err2[i] = e;
  a.pos_out[2 * (size_t)i] = qx;
  a.pos_out[2 * (size_t)i + 1] = qy;
}

// exclusive scan of a flag over the workgroup; total = the sum.  Every thread takes part.
__device__ __forceinline__ int block_scan_flag(bool flag, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int excl = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[wv] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kTrackBlock2 / 64; ++k) {
    const int t = wsum[k];
    base += k < wv ? t : 0;
    tot += t;
  }
  __syncthreads();  // wsum is free again
  total = tot;
  return base + excl;
}

__global__ __launch_bounds__(kTrackBlock2) void track_phase2_kernel(TrackPointsArgs a) {
  __shared__ int wsum[kTrackBlock2 / 64];
  __shared__ int cnt[4];
  const int N = a.N, b = blockIdx.x;
  const size_t off = (size_t)b * N;
  const unsigned long long* keys = a.keys + off;
  int* free_cells = a.free_cells + off;
  if (threadIdx.x < 4) cnt[threadIdx.x] = 0;
  // the unowned cells in cell order
  int nfree = 0;
  for (int c0 = 0; c0 < N; c0 += kTrackBlock2) {
    const int c = c0 + (int)threadIdx.x;
    const bool unowned = c < N && keys[c] == kNoClaim;
    int tot;
    const int k = nfree + block_scan_flag(unowned, wsum, tot);
    if (unowned) free_cells[k] = c;  // k < N: at most N cells
    nfree += tot;
  }
  __threadfence_block();
  __syncthreads();  // the list is complete and visible to the workgroup (cnt is zero, too)
  const long long epoch = *a.epoch;
  int nlost = 0;
  for (int s0 = 0; s0 < N; s0 += kTrackBlock2) {
    const int slot = s0 + (int)threadIdx.x;
    const bool valid = slot < N;
    const size_t i = off + (valid ? slot : 0);
    int st = -1;
    float qx = 0.f, qy = 0.f;
    if (valid) {
      st = a.status[i];
      if (st == 0) {
        qx = a.pos_out[2 * i];
        qy = a.pos_out[2 * i + 1];
        const int cell = cell_of(a, qx, qy);  // phase 1 found q inside the roi
        if ((unsigned)(keys[cell] & 0xffffffffull) != (unsigned)slot) st = 3;
      }
    }
    const bool lost = valid && st != 0;
    int tot;
    const int k = nlost + block_scan_flag(lost, wsum, tot);
    nlost += tot;
    if (valid && st == 0) {
      a.prev[2 * i] = a.pos[2 * i];
      a.prev[2 * i + 1] = a.pos[2 * i + 1];
      a.ids_out[i] = a.ids[i];
      a.age_out[i] = a.age[i] + 1;
    } else if (lost && k < nfree) {  // always: the lost slots are as many as the unowned cells
      const int cell = free_cells[k];
      if (a.seeds != nullptr) {  // the caller's seed of the cell
        a.pos_out[2 * i] = a.seeds[2 * (off + cell)];
        a.pos_out[2 * i + 1] = a.seeds[2 * (off + cell) + 1];
      } else {
        const int gy = cell / a.Gx, gx = cell - gy * a.Gx;
        // the seed of the cell: its centre, clamped into a partial cell (64-bit: S may be huge)
        const long cx = (long)gx * a.S + a.S / 2, cy = (long)gy * a.S + a.S / 2;
        a.pos_out[2 * i] = (float)(a.left + (int)(cx < a.w - 1 ? cx : a.w - 1));
        a.pos_out[2 * i + 1] = (float)(a.top + (int)(cy < a.h - 1 ? cy : a.h - 1));
      }
      a.prev[2 * i] = __builtin_nanf("");
      a.prev[2 * i + 1] = __builtin_nanf("");
      a.ids_out[i] = epoch * (long long)N + slot;
      a.age_out[i] = 0;
      if (st == 3) a.status[i] = 3;
    }
    // the slots per status: one LDS integer add per wave and status
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = __popcll(__ballot(st == s));
      if ((threadIdx.x & 63) == 0 && n) atomicAdd(&cnt[s], n);
    }
  }
  __syncthreads();
  if (threadIdx.x < 4) a.counts[4 * b + threadIdx.x] = cnt[threadIdx.x];
}

}  // namespace

hipError_t launch_track_points(const TrackPointsArgs& a, hipStream_t s) {
  const long tot = (long)a.B * a.N;
  if (tot == 0) return hipSuccess;
  if (tot >= (1L << 31) || a.HW != (long)a.H * a.W) return hipErrorInvalidValue;
  if (a.S < 1 || a.w < 1 || a.h < 1 || a.left < 0 || a.top < 0 || (long)a.left + a.w > a.W ||
      (long)a.top + a.h > a.H)
    return hipErrorInvalidValue;
  if (a.Gx != (a.w - 1) / a.S + 1 || a.Gy != (a.h - 1) / a.S + 1 || (long)a.Gx * a.Gy != a.N)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(track_clear_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a.keys, (unsigned)tot);
  hipLaunchKernelGGL(track_phase1_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(track_phase2_kernel, dim3((unsigned)a.B), dim3(kTrackBlock2), 0, s, a);
  return hipGetLastError();
}

}  // namespace raft_amd
