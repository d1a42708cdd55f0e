// Torch ops of working-resolution inference (csrc/frame_scale.hip); Python side
// raft_ros_amd/ops/frame_scale.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include "kernel_abi.h"

namespace raft_amd {

// frames (N, H, W, 3) uint8 -> (N, 3, ceil(H / D) + pad_t + pad_b, ceil(W / D) + pad_l + pad_r) fp32:
// the box downscale by D = scale (integer sum of a cell over its pixel count, one fp32 division),
// replicate padded, in one launch.
at::Tensor ingest_frames_scaled(const at::Tensor& frames, int64_t scale, int64_t pad_l, int64_t pad_r, int64_t pad_t,
                                int64_t pad_b) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous(),
              "raft_amd::ingest_frames_scaled: frames must be a contiguous uint8 (N, H, W, 3) CUDA tensor");
  TORCH_CHECK(scale >= 1 && scale <= 8, "raft_amd::ingest_frames_scaled: scale must lie in 1..8, got ", scale);
  const long N = frames.size(0), H = frames.size(1), W = frames.size(2), D = scale;
  TORCH_CHECK(pad_l >= 0 && pad_r >= 0 && pad_t >= 0 && pad_b >= 0,
              "raft_amd::ingest_frames_scaled: negative padding");
  TORCH_CHECK(N == 0 || (H > 0 && W > 0),
              "raft_amd::ingest_frames_scaled: empty frames cannot be replicate padded");
  TORCH_CHECK(pad_l < (1L << 31) && pad_r < (1L << 31) && pad_t < (1L << 31) && pad_b < (1L << 31),
              "raft_amd::ingest_frames_scaled: padding too large");
  const long h = (H + D - 1) / D, w = (W + D - 1) / D;
  const long hp = h + pad_t + pad_b, wp = w + pad_l + pad_r;
  // input and output offsets, the output's in groups of 4 pixels a row
  TORCH_CHECK(3 * N * H * W < (1L << 31) && 3 * N * hp * (wp + 3) < (1L << 31),
              "raft_amd::ingest_frames_scaled: N * H * W too large");
  c10::DeviceGuard guard(frames.device());
  at::Tensor out = at::empty({N, 3, hp, wp}, frames.options().dtype(at::kFloat));
  IngestScaledArgs a{};
  a.in = frames.data_ptr<unsigned char>();
  a.out = out.data_ptr<float>();
  a.N = (int)N;
  a.H = (int)H;
  a.W = (int)W;
  a.D = (int)D;
  a.h = (int)h;
  a.w = (int)w;
  a.pl = (int)pad_l;
  a.pt = (int)pad_t;
  a.hp = (int)hp;
  a.wp = (int)wp;
  const hipError_t e = launch_ingest_frames_scaled(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::ingest_frames_scaled: ", hipGetErrorString(e));
  return out;
}

// flow (B, 2, hp, wp) fp32, the model's output on the padded low-resolution frame whose unpadded
// image is [top, top + h) x [left, left + w) -> (B, 2, H, W) fp32 on the camera frame: bilinear
// with pixel centres aligned, clamped at the border, times D = scale.  One launch; the input
// is only read and the result is a fresh tensor.
at::Tensor upscale_flow(const at::Tensor& flow, int64_t scale, int64_t left, int64_t top, int64_t w, int64_t h,
                        int64_t H, int64_t W) {
  TORCH_CHECK(flow.is_cuda() && flow.scalar_type() == at::kFloat && flow.dim() == 4 && flow.size(1) == 2 &&
                  flow.is_contiguous(),
              "raft_amd::upscale_flow: flow must be a contiguous fp32 (B, 2, hp, wp) CUDA tensor");
  TORCH_CHECK(scale >= 1 && scale <= 8, "raft_amd::upscale_flow: scale must lie in 1..8, got ", scale);
  const long B = flow.size(0), hp = flow.size(2), wp = flow.size(3), D = scale;
  TORCH_CHECK(w > 0 && h > 0 && left >= 0 && top >= 0 && left + w <= wp && top + h <= hp,
              "raft_amd::upscale_flow: the image (left ", left, ", top ", top, ", ", w, " x ", h,
              ") does not lie inside the ", wp, " x ", hp, " flow");
  TORCH_CHECK(H > 0 && W > 0 && (H + D - 1) / D == h && (W + D - 1) / D == w, "raft_amd::upscale_flow: a ", W, " x ", H,
              " frame reduced by ", D, " is not ", w, " x ", h);
  // input and output offsets, the output's in groups of 4 pixels a row
  TORCH_CHECK(2 * B * hp * wp < (1L << 31) && 2 * B * H * (W + 3) < (1L << 31),
              "raft_amd::upscale_flow: B * H * W too large");
  c10::DeviceGuard guard(flow.device());
  at::Tensor out = at::empty({B, 2, H, W}, flow.options());
  UpscaleFlowArgs a{};
  a.flow = flow.data_ptr<float>();
  a.out = out.data_ptr<float>();
  a.B = (int)B;
  a.D = (int)D;
  a.hp = (int)hp;
  a.wp = (int)wp;
  a.left = (int)left;
  a.top = (int)top;
  a.w = (int)w;
  a.h = (int)h;
  a.H = (int)H;
  a.W = (int)W;
  const hipError_t e = launch_upscale_flow(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::upscale_flow: ", hipGetErrorString(e));
  return out;
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def("ingest_frames_scaled(Tensor frames, int scale, int pad_l, int pad_r, int pad_t, int pad_b) -> Tensor");
  m.def("upscale_flow(Tensor flow, int scale, int left, int top, int w, int h, int H, int W) -> Tensor");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("ingest_frames_scaled", &raft_amd::ingest_frames_scaled);
  m.impl("upscale_flow", &raft_amd::upscale_flow);
}
