// Torch op of the point tracks (csrc/track_points.hip); Python side raft_ros_amd/ops/track.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include <optional>
#include <tuple>

#include "kernel_abi.h"

namespace raft_amd {

using TrackOut =
    std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor>;

// pos (B, N, 2) fp32, ids (B, N) int64, age (B, N) int32, epoch (1) int64, flow_fw and optionally
// flow_bw (B, 2, H, W) fp32, the roi (left, top, w, h) and the cell size S -> pos_out, prev,
// ids_out, age_out, epoch_out, status (B, N) uint8, err2 (B, N) fp32, counts (B, 4) int32.
// Three launches on the current stream, no host read-back.  ``seeds`` (B, N, 2) fp32, where the
// fresh point of every cell starts, or null: the cell's clamped centre.  The one body of both ops.
static TrackOut track_points_impl(const char* op, const at::Tensor& pos, const at::Tensor& ids, const at::Tensor& age,
                                  const at::Tensor& epoch, const at::Tensor& flow_fw,
                                  const std::optional<at::Tensor>& flow_bw, const at::Tensor* seeds, int64_t left,
                                  int64_t top, int64_t w, int64_t h, int64_t S, double alpha1, double alpha2) {
  TORCH_CHECK(flow_fw.is_cuda() && flow_fw.scalar_type() == at::kFloat && flow_fw.dim() == 4 &&
                  flow_fw.size(1) == 2 && flow_fw.is_contiguous(),
              op, "flow_fw must be a contiguous fp32 (B, 2, H, W) CUDA tensor");
  const bool has_bw = flow_bw.has_value() && flow_bw->defined();
  if (has_bw) {
    TORCH_CHECK(flow_bw->is_cuda() && flow_bw->scalar_type() == at::kFloat && flow_bw->is_contiguous(), op,
                "flow_bw must be a contiguous fp32 CUDA tensor");
    TORCH_CHECK(flow_bw->sizes() == flow_fw.sizes(), op, "flow_fw and flow_bw differ in shape: ", flow_fw.sizes(),
                " and ", flow_bw->sizes());
    TORCH_CHECK(flow_bw->device() == flow_fw.device(), op, "flow_fw and flow_bw are on different devices");
  }
  const long B = flow_fw.size(0), H = flow_fw.size(2), W = flow_fw.size(3);
  TORCH_CHECK(H < (1L << 31) && W < (1L << 31), op, "frame too large");
  TORCH_CHECK(S >= 1 && S < (1L << 31), op, "the cell size must be at least 1, got ", S);
  TORCH_CHECK(w >= 1 && h >= 1 && left >= 0 && top >= 0 && left + w <= W && top + h <= H, op, "the roi (", left, ", ",
              top, ", ", w, ", ", h, ") must lie inside the ", H, " x ", W, " frame with w, h >= 1");
  const long Gx = (w - 1) / S + 1, Gy = (h - 1) / S + 1, N = Gx * Gy;
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kFloat && pos.is_contiguous() && pos.dim() == 3 &&
                  pos.size(0) == B && pos.size(1) == N && pos.size(2) == 2,
              op, "pos must be a contiguous fp32 (", B, ", ", N, ", 2) CUDA tensor (the grid has ", Gy, " x ", Gx,
              " cells), got ", pos.sizes());
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.is_contiguous() && ids.dim() == 2 &&
                  ids.size(0) == B && ids.size(1) == N,
              op, "ids must be a contiguous int64 (", B, ", ", N, ") CUDA tensor, got ", ids.sizes());
  TORCH_CHECK(age.is_cuda() && age.scalar_type() == at::kInt && age.is_contiguous() && age.dim() == 2 &&
                  age.size(0) == B && age.size(1) == N,
              op, "age must be a contiguous int32 (", B, ", ", N, ") CUDA tensor, got ", age.sizes());
  TORCH_CHECK(epoch.is_cuda() && epoch.scalar_type() == at::kLong && epoch.numel() == 1, op,
              "epoch must be an int64 CUDA tensor of one element");
  TORCH_CHECK(pos.device() == flow_fw.device() && ids.device() == flow_fw.device() &&
                  age.device() == flow_fw.device() && epoch.device() == flow_fw.device(),
              op, "all tensors must be on one device");
  TORCH_CHECK(B * N < (1L << 31), op, "B * N too large");
  if (seeds != nullptr) {
    TORCH_CHECK(seeds->is_cuda() && seeds->scalar_type() == at::kFloat && seeds->is_contiguous() &&
                    seeds->dim() == 3 && seeds->size(0) == B && seeds->size(1) == N && seeds->size(2) == 2,
                op, "seeds must be a contiguous fp32 (", B, ", ", N, ", 2) CUDA tensor, got ", seeds->sizes());
    TORCH_CHECK(seeds->device() == flow_fw.device(), op, "all tensors must be on one device");
  }
  c10::DeviceGuard guard(flow_fw.device());
  at::Tensor pos_out = at::empty({B, N, 2}, pos.options());
  at::Tensor prev = at::empty({B, N, 2}, pos.options());
  at::Tensor ids_out = at::empty({B, N}, ids.options());
  at::Tensor age_out = at::empty({B, N}, age.options());
  at::Tensor epoch_out = at::empty({1}, epoch.options());
  at::Tensor status = at::empty({B, N}, pos.options().dtype(at::kByte));
  at::Tensor err2 = at::empty({B, N}, pos.options());
  at::Tensor counts = at::empty({B, 4}, pos.options().dtype(at::kInt));
  if (B == 0) {  // nothing to launch; the epoch still advances
    epoch_out.copy_(epoch.reshape({1}) + 1);
    return {pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts};
  }
  at::Tensor keys = at::empty({B, N}, ids.options());
  at::Tensor free_cells = at::empty({B, N}, age.options());
  TrackPointsArgs a{};
  a.pos = pos.data_ptr<float>();
  a.ids = reinterpret_cast<const long long*>(ids.data_ptr<int64_t>());
  a.age = age.data_ptr<int>();
  a.epoch = reinterpret_cast<const long long*>(epoch.data_ptr<int64_t>());
  a.fw = flow_fw.data_ptr<float>();
  a.bw = has_bw ? flow_bw->data_ptr<float>() : nullptr;
  a.seeds = seeds != nullptr ? seeds->data_ptr<float>() : nullptr;
  a.pos_out = pos_out.data_ptr<float>();
  a.prev = prev.data_ptr<float>();
  a.ids_out = reinterpret_cast<long long*>(ids_out.data_ptr<int64_t>());
  a.age_out = age_out.data_ptr<int>();
  a.epoch_out = reinterpret_cast<long long*>(epoch_out.data_ptr<int64_t>());
  a.status = status.data_ptr<unsigned char>();
  a.err2 = err2.data_ptr<float>();
  a.counts = counts.data_ptr<int>();
  a.keys = reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>());
  a.free_cells = free_cells.data_ptr<int>();
  a.alpha1 = (float)alpha1;
  a.alpha2 = (float)alpha2;
  a.B = (int)B;
  a.N = (int)N;
  a.H = (int)H;
  a.W = (int)W;
  a.left = (int)left;
  a.top = (int)top;
  a.w = (int)w;
  a.h = (int)h;
  a.S = (int)S;
  a.Gx = (int)Gx;
  a.Gy = (int)Gy;
  a.HW = H * W;
  const hipError_t e = launch_track_points(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, op, hipGetErrorString(e));
  return {pos_out, prev, ids_out, age_out, epoch_out, status, err2, counts};
}

TrackOut track_points(const at::Tensor& pos, const at::Tensor& ids, const at::Tensor& age, const at::Tensor& epoch,
                      const at::Tensor& flow_fw, const std::optional<at::Tensor>& flow_bw, int64_t left, int64_t top,
                      int64_t w, int64_t h, int64_t S, double alpha1, double alpha2) {
  return track_points_impl("raft_amd::track_points: ", pos, ids, age, epoch, flow_fw, flow_bw, nullptr, left, top, w,
                           h, S, alpha1, alpha2);
}

TrackOut track_points_seeded(const at::Tensor& pos, const at::Tensor& ids, const at::Tensor& age,
                             const at::Tensor& epoch, const at::Tensor& flow_fw,
                             const std::optional<at::Tensor>& flow_bw, const at::Tensor& seeds, int64_t left,
                             int64_t top, int64_t w, int64_t h, int64_t S, double alpha1, double alpha2) {
  return track_points_impl("raft_amd::track_points_seeded: ", pos, ids, age, epoch, flow_fw, flow_bw, &seeds, left,
                           top, w, h, S, alpha1, alpha2);
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def(
      "track_points(Tensor pos, Tensor ids, Tensor age, Tensor epoch, Tensor flow_fw, Tensor? flow_bw, int left, "
      "int top, int w, int h, int S, float alpha1, float alpha2) -> (Tensor pos_out, Tensor prev, Tensor ids_out, "
      "Tensor age_out, Tensor epoch_out, Tensor status, Tensor err2, Tensor counts)");
  m.def(
      "track_points_seeded(Tensor pos, Tensor ids, Tensor age, Tensor epoch, Tensor flow_fw, Tensor? flow_bw, "
      "Tensor seeds, int left, int top, int w, int h, int S, float alpha1, float alpha2) -> (Tensor pos_out, "
      "Tensor prev, Tensor ids_out, Tensor age_out, Tensor epoch_out, Tensor status, Tensor err2, Tensor counts)");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("track_points", &raft_amd::track_points);
  m.impl("track_points_seeded", &raft_amd::track_points_seeded);
}
