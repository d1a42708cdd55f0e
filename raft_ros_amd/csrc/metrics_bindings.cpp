// Torch op of the validation metrics (csrc/flow_metrics.hip); Python side
// raft_ros_amd/ops/metrics.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include <tuple>

#include "kernel_abi.h"

namespace raft_amd {

// flow_pr (B, 2, Hp, Wp) fp32 read at the crop [top, top + H) x [left, left + W), flow_gt
// (B, 2, H, W) fp32, valid (B, H, W) fp32 or none -> epe_sum (B,) float64, counts (B, 5) int32
// (counted pixels, epe < 1, epe < 3, epe < 5, KITTI outliers).  Two launches on the current
// stream, no host read-back.
std::tuple<at::Tensor, at::Tensor> flow_metrics(const at::Tensor& flow_pr, const at::Tensor& flow_gt,
                                                const c10::optional<at::Tensor>& valid, int64_t top, int64_t left) {
  TORCH_CHECK(flow_pr.is_cuda() && flow_pr.scalar_type() == at::kFloat && flow_pr.dim() == 4 &&
                  flow_pr.size(1) == 2 && flow_pr.is_contiguous(),
              "raft_amd::flow_metrics: flow_pr must be a contiguous fp32 (B, 2, Hp, Wp) CUDA tensor");
  TORCH_CHECK(flow_gt.is_cuda() && flow_gt.scalar_type() == at::kFloat && flow_gt.dim() == 4 &&
                  flow_gt.size(1) == 2 && flow_gt.is_contiguous(),
              "raft_amd::flow_metrics: flow_gt must be a contiguous fp32 (B, 2, H, W) CUDA tensor");
  TORCH_CHECK(flow_gt.device() == flow_pr.device(), "raft_amd::flow_metrics: flow_pr and flow_gt are on different devices");
  TORCH_CHECK(flow_gt.size(0) == flow_pr.size(0), "raft_amd::flow_metrics: flow_pr and flow_gt differ in batch: ",
              flow_pr.sizes(), " and ", flow_gt.sizes());
  const long B = flow_gt.size(0), H = flow_gt.size(2), W = flow_gt.size(3);
  const long Hp = flow_pr.size(2), Wp = flow_pr.size(3);
  TORCH_CHECK(top >= 0 && left >= 0 && top <= Hp - H && left <= Wp - W, "raft_amd::flow_metrics: the crop of ", H, " x ", W,
              " at (", top, ", ", left, ") leaves the prediction ", flow_pr.sizes());
  if (valid.has_value()) {
    const at::Tensor& v = *valid;
    TORCH_CHECK(v.is_cuda() && v.scalar_type() == at::kFloat && v.is_contiguous(),
                "raft_amd::flow_metrics: valid must be a contiguous fp32 CUDA tensor");
    TORCH_CHECK(v.dim() == 3 && v.size(0) == B && v.size(1) == H && v.size(2) == W,
                "raft_amd::flow_metrics: valid must be (B, H, W) = (", B, ", ", H, ", ", W, "), got ", v.sizes());
    TORCH_CHECK(v.device() == flow_pr.device(), "raft_amd::flow_metrics: flow_pr and valid are on different devices");
  }
  // 32-bit pixel and block indices
  TORCH_CHECK(H < (1L << 31) && W < (1L << 31) && Hp < (1L << 31) && Wp < (1L << 31) &&
                  (H == 0 || W == 0 || B * H < (1L << 31) / W),
              "raft_amd::flow_metrics: B * H * W too large");
  c10::DeviceGuard guard(flow_pr.device());
  at::Tensor epe_sum = at::empty({B}, flow_pr.options().dtype(at::kDouble));
  at::Tensor counts = at::empty({B, (long)kMetricCounts}, flow_pr.options().dtype(at::kInt));
  if (B == 0 || H * W == 0) {
    if (B > 0) {
      epe_sum.zero_();
      counts.zero_();
    }
    return {epe_sum, counts};
  }
  const long nblk = flow_metrics_blocks(H, W);
  at::Tensor part_sum = at::empty({B, nblk}, epe_sum.options());
  at::Tensor part_cnt = at::empty({B, nblk, (long)kMetricCounts}, counts.options());
  FlowMetricsArgs a{};
  a.pr = flow_pr.data_ptr<float>();
  a.gt = flow_gt.data_ptr<float>();
  a.valid = valid.has_value() ? valid->data_ptr<float>() : nullptr;
  a.part_sum = part_sum.data_ptr<double>();
  a.part_cnt = part_cnt.data_ptr<int>();
  a.epe_sum = epe_sum.data_ptr<double>();
  a.counts = counts.data_ptr<int>();
  a.B = (int)B;
  a.H = (int)H;
  a.W = (int)W;
  a.Hp = (int)Hp;
  a.Wp = (int)Wp;
  a.top = (int)top;
  a.left = (int)left;
  a.nblk = (int)nblk;
  const hipError_t e = launch_flow_metrics(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, "raft_amd::flow_metrics: ", hipGetErrorString(e));
  return {epe_sum, counts};
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def("flow_metrics(Tensor flow_pr, Tensor flow_gt, Tensor? valid, int top, int left) -> (Tensor epe_sum, Tensor counts)");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("flow_metrics", &raft_amd::flow_metrics);
}
