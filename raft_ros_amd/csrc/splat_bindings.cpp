// Torch op of the warm-start forward splat (csrc/forward_splat.hip); Python side
// raft_ros_amd/ops/warm_start.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include "kernel_abi.h"

namespace raft_amd {

// flow (B, 2, H, W) fp32 -> the flow forward-projected onto the next frame's grid, holes
// filled by the nearest projected point.  Runs on the current stream, no host read-back.
at::Tensor forward_splat_nearest(const at::Tensor& flow) {
  TORCH_CHECK(flow.is_cuda() && flow.scalar_type() == at::kFloat && flow.dim() == 4 && flow.size(1) == 2 &&
                  flow.is_contiguous(),
              "raft_amd::forward_splat_nearest: flow must be a contiguous fp32 (B, 2, H, W) CUDA tensor");
  const long B = flow.size(0), H = flow.size(2), W = flow.size(3);
  TORCH_CHECK(2 * B * H * W + B < (1L << 31), "raft_amd::forward_splat_nearest: B * H * W too large");
  c10::DeviceGuard guard(flow.device());
  at::Tensor out = at::empty_like(flow);
  at::Tensor ws = at::empty({2 * B * H * W + B}, flow.options().dtype(at::kInt));
  SplatArgs a{};
  a.flow = flow.data_ptr<float>();
  a.out = out.data_ptr<float>();
  a.heads = ws.data_ptr<int>();
  a.any = a.heads + B * H * W;
  a.next = a.any + B;
  a.B = (int)B;
  a.H = (int)H;
  a.W = (int)W;
  const hipError_t e = launch_forward_splat(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::forward_splat_nearest: ", hipGetErrorString(e));
  return out;
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) { m.def("forward_splat_nearest(Tensor flow) -> Tensor"); }

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) { m.impl("forward_splat_nearest", &raft_amd::forward_splat_nearest); }
