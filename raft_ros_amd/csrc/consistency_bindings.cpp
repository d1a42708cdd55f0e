// Torch op of the forward-backward consistency check (csrc/fb_consistency.hip); Python side
// raft_ros_amd/ops/consistency.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include <tuple>

#include "kernel_abi.h"

namespace raft_amd {

// flow_fw, flow_bw (B, 2, H, W) fp32 -> occ (B, H, W) uint8 (0 consistent, 1 inconsistent, 2 the
// forward flow leaves the frame), err2 (B, H, W) fp32, counts (B, 2) int32 (pixels of class 1 / 2).
// One memset and one launch on the current stream, no host read-back.
std::tuple<at::Tensor, at::Tensor, at::Tensor> fb_consistency(const at::Tensor& flow_fw, const at::Tensor& flow_bw,
                                                              double alpha1, double alpha2) {
  TORCH_CHECK(flow_fw.is_cuda() && flow_fw.scalar_type() == at::kFloat && flow_fw.dim() == 4 &&
                  flow_fw.size(1) == 2 && flow_fw.is_contiguous(),
              "raft_amd::fb_consistency: flow_fw must be a contiguous fp32 (B, 2, H, W) CUDA tensor");
  TORCH_CHECK(flow_bw.is_cuda() && flow_bw.scalar_type() == at::kFloat && flow_bw.is_contiguous(),
              "raft_amd::fb_consistency: flow_bw must be a contiguous fp32 CUDA tensor");
  TORCH_CHECK(flow_bw.sizes() == flow_fw.sizes(), "raft_amd::fb_consistency: flow_fw and flow_bw differ in shape: ",
              flow_fw.sizes(), " and ", flow_bw.sizes());
  TORCH_CHECK(flow_bw.device() == flow_fw.device(), "raft_amd::fb_consistency: flow_fw and flow_bw are on different devices");
  const long B = flow_fw.size(0), H = flow_fw.size(2), W = flow_fw.size(3);
  // a flat 32-bit pixel index, 4 pixels a thread
  TORCH_CHECK(H < (1L << 31) && W < (1L << 31) && (H == 0 || W == 0 || B * H < (1L << 31) / W),
              "raft_amd::fb_consistency: B * H * W too large");
  c10::DeviceGuard guard(flow_fw.device());
  at::Tensor occ = at::empty({B, H, W}, flow_fw.options().dtype(at::kByte));
  at::Tensor err2 = at::empty({B, H, W}, flow_fw.options());
  at::Tensor counts = at::empty({B, 2}, flow_fw.options().dtype(at::kInt));
  if (B == 0 || H * W == 0) {
    if (B > 0) counts.zero_();
    return {occ, err2, counts};
  }
  FbConsistencyArgs a{};
  a.fw = flow_fw.data_ptr<float>();
  a.bw = flow_bw.data_ptr<float>();
  a.occ = occ.data_ptr<unsigned char>();
  a.err2 = err2.data_ptr<float>();
  a.counts = counts.data_ptr<int>();
  a.alpha1 = (float)alpha1;
  a.alpha2 = (float)alpha2;
  a.B = (int)B;
  a.H = (int)H;
  a.W = (int)W;
  a.HW = H * W;
  const hipError_t e = launch_fb_consistency(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::fb_consistency: ", hipGetErrorString(e));
  return {occ, err2, counts};
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def("fb_consistency(Tensor flow_fw, Tensor flow_bw, float alpha1, float alpha2) -> (Tensor occ, Tensor err2, Tensor counts)");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("fb_consistency", &raft_amd::fb_consistency);
}
