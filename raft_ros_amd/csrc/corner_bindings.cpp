// Torch op of the corner seeds (csrc/corner_seeds.hip); Python side raft_ros_amd/ops/corners.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include <tuple>

#include "kernel_abi.h"

namespace raft_amd {

// frames (B, H, W, 3) uint8, the cell size S, the roi size (w, h) inside the frame, the origin
// (left, top) added to the seeds, the margin and min_score -> seeds (B, N, 2) fp32, score (B, N)
// int32.  Three launches on the current stream, no host read-back.
std::tuple<at::Tensor, at::Tensor> corner_seeds(const at::Tensor& frames, int64_t S, int64_t w, int64_t h,
                                                int64_t left, int64_t top, int64_t margin, int64_t min_score) {
  const char* op = "raft_amd::corner_seeds: ";
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous(),
              op, "frames must be a contiguous uint8 (B, H, W, 3) CUDA tensor, got ", frames.sizes());
  const long B = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(H >= 1 && W >= 1 && H * W < (1L << 31), op, "frames of ", H, " x ", W, " pixels: empty or too large");
  TORCH_CHECK(S >= 1 && S < (1L << 31), op, "the cell size must be at least 1, got ", S);
  TORCH_CHECK(w >= 1 && h >= 1 && w <= W && h <= H, op, "the roi size (", w, ", ", h, ") must lie inside the ", H,
              " x ", W, " frame");
  TORCH_CHECK(margin >= 0 && 2 * margin <= S - 1, op, "the margin needs 0 <= 2 * margin <= S - 1, got margin ",
              margin, " with S ", S);
  // fp32 holds every seed coordinate exactly
  TORCH_CHECK(left >= -(1L << 23) && left + w <= (1L << 23) && top >= -(1L << 23) && top + h <= (1L << 23), op,
              "the origin (", left, ", ", top, ") is out of range");
  const long Gx = (w - 1) / S + 1, Gy = (h - 1) / S + 1, N = Gx * Gy;
  TORCH_CHECK(B * N < (1L << 31) && B <= 65535, op, "B * N too large");
  c10::DeviceGuard guard(frames.device());
  at::Tensor seeds = at::empty({B, N, 2}, frames.options().dtype(at::kFloat));
  at::Tensor score = at::empty({B, N}, frames.options().dtype(at::kInt));
  if (B == 0) return {seeds, score};
  at::Tensor keys = at::empty({B, N}, frames.options().dtype(at::kLong));
  CornerSeedsArgs a{};
  a.frames = frames.data_ptr<unsigned char>();
  a.keys = reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>());
  a.seeds = seeds.data_ptr<float>();
  a.score = score.data_ptr<int>();
  a.min_score = (long long)min_score;
  a.B = (int)B;
  a.N = (int)N;
  a.H = (int)H;
  a.W = (int)W;
  a.w = (int)w;
  a.h = (int)h;
  a.left = (int)left;
  a.top = (int)top;
  a.S = (int)S;
  a.Gx = (int)Gx;
  a.Gy = (int)Gy;
  a.margin = (int)margin;
  const hipError_t e = launch_corner_seeds(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, op, hipGetErrorString(e));
  return {seeds, score};
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def(
      "corner_seeds(Tensor frames, int S, int w, int h, int left, int top, int margin, int min_score) -> "
      "(Tensor seeds, Tensor score)");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("corner_seeds", &raft_amd::corner_seeds);
}
