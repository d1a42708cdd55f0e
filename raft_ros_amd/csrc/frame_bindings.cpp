// Torch ops of the device-side frame path (csrc/flow_color.hip); Python side
// raft_ros_amd/ops/frame_io.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include "kernel_abi.h"

namespace raft_amd {

// flow (B, 2, H, W) fp32 -> (B, H, W, 3) uint8 colour coding, each image normalised by its own
// largest radius.  One memset and two launches on the current stream, no host read-back.
at::Tensor flow_to_image(const at::Tensor& flow, c10::optional<double> clip_flow, bool bgr) {
  TORCH_CHECK(flow.is_cuda() && flow.scalar_type() == at::kFloat && flow.dim() == 4 && flow.size(1) == 2 &&
                  flow.is_contiguous(),
              "raft_amd::flow_to_image: flow must be a contiguous fp32 (B, 2, H, W) CUDA tensor");
  const long B = flow.size(0), H = flow.size(2), W = flow.size(3);
  // 3 * B * H * W output bytes, 4 pixels a thread, B as a grid dimension
  TORCH_CHECK(3 * B * H * W < (1L << 31) && B < (1L << 16), "raft_amd::flow_to_image: B * H * W too large");
  c10::DeviceGuard guard(flow.device());
  at::Tensor img = at::empty({B, H, W, 3}, flow.options().dtype(at::kByte));
  at::Tensor ws = at::empty({B}, flow.options().dtype(at::kInt));
  FlowColorArgs a{};
  a.flow = flow.data_ptr<float>();
  a.img = img.data_ptr<unsigned char>();
  a.rad_max = reinterpret_cast<unsigned*>(ws.data_ptr<int>());
  a.has_clip = clip_flow.has_value();
  a.clip = a.has_clip ? (float)*clip_flow : 0.f;
  a.bgr = bgr;
  a.B = (int)B;
  a.HW = H * W;
  const hipError_t e = launch_flow_to_image(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::flow_to_image: ", hipGetErrorString(e));
  return img;
}

// frames (N, H, W, 3) uint8 -> (N, 3, H + pad_t + pad_b, W + pad_l + pad_r) fp32, replicate
// padded: F.pad(frames.permute(0, 3, 1, 2).float(), [l, r, t, b], mode="replicate") in one launch.
at::Tensor ingest_frames(const at::Tensor& frames, int64_t pad_l, int64_t pad_r, int64_t pad_t, int64_t pad_b) {
  TORCH_CHECK(frames.is_cuda() && frames.scalar_type() == at::kByte && frames.dim() == 4 && frames.size(3) == 3 &&
                  frames.is_contiguous(),
              "raft_amd::ingest_frames: frames must be a contiguous uint8 (N, H, W, 3) CUDA tensor");
  const long N = frames.size(0), H = frames.size(1), W = frames.size(2);
  TORCH_CHECK(pad_l >= 0 && pad_r >= 0 && pad_t >= 0 && pad_b >= 0, "raft_amd::ingest_frames: negative padding");
  TORCH_CHECK(N == 0 || (H > 0 && W > 0), "raft_amd::ingest_frames: empty frames cannot be replicate padded");
  TORCH_CHECK(pad_l < (1L << 31) && pad_r < (1L << 31) && pad_t < (1L << 31) && pad_b < (1L << 31),
              "raft_amd::ingest_frames: padding too large");
  const long Hp = H + pad_t + pad_b, Wp = W + pad_l + pad_r;
  TORCH_CHECK(3 * N * Hp * (Wp + 3) < (1L << 31), "raft_amd::ingest_frames: N * H * W too large");
  c10::DeviceGuard guard(frames.device());
  at::Tensor out = at::empty({N, 3, Hp, Wp}, frames.options().dtype(at::kFloat));
  IngestArgs a{};
  a.in = frames.data_ptr<unsigned char>();
  a.out = out.data_ptr<float>();
  a.N = (int)N;
  a.H = (int)H;
  a.W = (int)W;
  a.pl = (int)pad_l;
  a.pt = (int)pad_t;
  a.Hp = (int)Hp;
  a.Wp = (int)Wp;
  const hipError_t e = launch_ingest_frames(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::ingest_frames: ", hipGetErrorString(e));
  return out;
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def("flow_to_image(Tensor flow, float? clip_flow, bool bgr) -> Tensor");
  m.def("ingest_frames(Tensor frames, int pad_l, int pad_r, int pad_t, int pad_b) -> Tensor");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("flow_to_image", &raft_amd::flow_to_image);
  m.impl("ingest_frames", &raft_amd::ingest_frames);
}
