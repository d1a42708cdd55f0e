// Torch ops of the training augmentation (csrc/augment.hip); Python side raft_ros_amd/ops/augment.py.
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>

#include <hip/hip_runtime.h>

#include <string>
#include <tuple>

#include "kernel_abi.h"

namespace raft_amd {
namespace {

using Augmented = std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor>;

// Both ops: the argument checks, the workspaces and the launch.  valid and flags are null for the
// dense op.
Augmented augment_run(const std::string& op, const at::Tensor& img1, const at::Tensor& img2, const at::Tensor& flow,
                      const at::Tensor* valid, const at::Tensor& size, const at::Tensor& pf, const at::Tensor& pi,
                      const at::Tensor* flags, int64_t ch, int64_t cw) {
  TORCH_CHECK(img1.is_cuda() && img1.scalar_type() == at::kByte && img1.dim() == 4 && img1.size(3) == 3 &&
                  img1.is_contiguous(),
              op, ": img1 must be a contiguous uint8 (B, Hm, Wm, 3) CUDA tensor");
  const long B = img1.size(0), Hm = img1.size(1), Wm = img1.size(2);
  const auto dev = img1.device();
  TORCH_CHECK(img2.device() == dev && img2.scalar_type() == at::kByte && img2.is_contiguous() &&
                  img2.sizes() == img1.sizes(),
              op, ": img2 must be a contiguous uint8 tensor of img1's shape and device");
  TORCH_CHECK(flow.device() == dev && flow.scalar_type() == at::kFloat && flow.is_contiguous() && flow.dim() == 4 &&
                  flow.size(0) == B && flow.size(1) == Hm && flow.size(2) == Wm && flow.size(3) == 2,
              op, ": flow must be a contiguous fp32 (B, Hm, Wm, 2) tensor on img1's device");
  TORCH_CHECK(size.device() == dev && size.scalar_type() == at::kLong && size.is_contiguous() && size.dim() == 2 &&
                  size.size(0) == B && size.size(1) == 2,
              op, ": size must be a contiguous int64 (B, 2) tensor on img1's device");
  TORCH_CHECK(pf.device() == dev && pf.scalar_type() == at::kFloat && pf.is_contiguous() && pf.dim() == 2 &&
                  pf.size(0) == B && pf.size(1) == kAugPF,
              op, ": pf must be a contiguous fp32 (B, ", kAugPF, ") tensor on img1's device");
  TORCH_CHECK(pi.device() == dev && pi.scalar_type() == at::kInt && pi.is_contiguous() && pi.dim() == 2 &&
                  pi.size(0) == B && pi.size(1) == kAugPI,
              op, ": pi must be a contiguous int32 (B, ", kAugPI, ") tensor on img1's device");
  if (valid != nullptr) {
    TORCH_CHECK(valid->device() == dev && valid->scalar_type() == at::kFloat && valid->is_contiguous() &&
                    valid->dim() == 3 && valid->size(0) == B && valid->size(1) == Hm && valid->size(2) == Wm,
                op, ": valid must be a contiguous fp32 (B, Hm, Wm) tensor on img1's device");
    TORCH_CHECK(flags->device() == dev && flags->scalar_type() == at::kInt && flags->is_contiguous() &&
                    flags->dim() == 1 && flags->size(0) == B,
                op, ": flags must be a contiguous int32 (B) tensor on img1's device");
  }
  TORCH_CHECK(ch >= 0 && cw >= 0 && ch < (1L << 31) && cw < (1L << 31) && (cw == 0 || ch < (1L << 31) / cw),
              op, ": bad crop size ", ch, " x ", cw);
  // exact 64-bit luma sums and a 32-bit pixel index per sample; the batch is the grid's y
  TORCH_CHECK(B <= 65535 && (Wm == 0 || Hm <= (1L << 26) / Wm), op, ": batch of ", B, " x ", Hm, " x ", Wm,
              " too large");
  c10::DeviceGuard guard(dev);
  const auto f32 = img1.options().dtype(at::kFloat);
  at::Tensor out1 = at::empty({B, 3, ch, cw}, f32), out2 = at::empty({B, 3, ch, cw}, f32);
  at::Tensor oflow = at::empty({B, 2, ch, cw}, f32), ovalid = at::empty({B, ch, cw}, f32);
  if (B == 0 || ch == 0 || cw == 0) return {out1, out2, oflow, ovalid};
  // the jittered pair, written and read inside each sample's region only
  at::Tensor jit = at::empty({2, B, Hm, Wm}, img1.options().dtype(at::kInt));
  // the statistics and, behind them in the same allocation, the sparse samples' winner buffer
  // (B, ch, cw) int32: one memset zeroes both
  const long win_words = valid != nullptr ? (B * ch * cw + 1) / 2 : 0;
  at::Tensor stats = at::empty({B * kAugStats + win_words}, img1.options().dtype(at::kLong));
  AugmentArgs a{};
  a.img1 = img1.data_ptr<unsigned char>();
  a.img2 = img2.data_ptr<unsigned char>();
  a.flow = flow.data_ptr<float>();
  a.size = reinterpret_cast<const long*>(size.data_ptr<int64_t>());
  a.pf = pf.data_ptr<float>();
  a.pi = pi.data_ptr<int>();
  a.jit1 = reinterpret_cast<unsigned*>(jit.data_ptr<int>());
  a.jit2 = a.jit1 + B * Hm * Wm;
  a.stats = reinterpret_cast<long long*>(stats.data_ptr<int64_t>());
  a.out1 = out1.data_ptr<float>();
  a.out2 = out2.data_ptr<float>();
  a.oflow = oflow.data_ptr<float>();
  a.ovalid = ovalid.data_ptr<float>();
  a.B = (int)B;
  a.Hm = (int)Hm;
  a.Wm = (int)Wm;
  a.ch = (int)ch;
  a.cw = (int)cw;
  if (valid != nullptr) {
    a.valid = valid->data_ptr<float>();
    a.flags = flags->data_ptr<int>();
    a.win = reinterpret_cast<int*>(a.stats + B * kAugStats);
  }
  const hipError_t e = launch_augment_batch(a, c10::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(e == hipSuccess, op, ": ", hipGetErrorString(e));
  return {out1, out2, oflow, ovalid};
}

}  // namespace

// img1, img2 (B, Hm, Wm, 3) uint8, flow (B, Hm, Wm, 2) fp32, size (B, 2) int64, the drawn parameters
// pf (B, kAugPF) fp32 and pi (B, kAugPI) int32 -> img1, img2 (B, 3, ch, cw), flow (B, 2, ch, cw),
// valid (B, ch, cw), all fp32.  One memset and three launches on the current stream, no host
// read-back.
Augmented augment_batch(const at::Tensor& img1, const at::Tensor& img2, const at::Tensor& flow, const at::Tensor& size,
                        const at::Tensor& pf, const at::Tensor& pi, int64_t ch, int64_t cw) {
  return augment_run("raft_amd::augment_batch", img1, img2, flow, nullptr, size, pf, pi, nullptr, ch, cw);
}

// The same with sparse ground truth: valid (B, Hm, Wm) fp32 and flags (B) int32 (kAugSparse |
// kAugResize per sample).  A sparse sample's flow and valid are the scatter of its valid pixels
// (BatchAugmentor._sparse_flow), a dense sample's as above.  Still one memset and three launches.
Augmented augment_batch_sparse(const at::Tensor& img1, const at::Tensor& img2, const at::Tensor& flow,
                               const at::Tensor& valid, const at::Tensor& size, const at::Tensor& pf,
                               const at::Tensor& pi, const at::Tensor& flags, int64_t ch, int64_t cw) {
  return augment_run("raft_amd::augment_batch_sparse", img1, img2, flow, &valid, size, pf, pi, &flags, ch, cw);
}

}  // namespace raft_amd

TORCH_LIBRARY_FRAGMENT(raft_amd, m) {
  m.def("augment_batch(Tensor img1, Tensor img2, Tensor flow, Tensor size, Tensor pf, Tensor pi, int ch, int cw) -> "
        "(Tensor out1, Tensor out2, Tensor out_flow, Tensor out_valid)");
  m.def("augment_batch_sparse(Tensor img1, Tensor img2, Tensor flow, Tensor valid, Tensor size, Tensor pf, Tensor pi, "
        "Tensor flags, int ch, int cw) -> (Tensor out1, Tensor out2, Tensor out_flow, Tensor out_valid)");
}

TORCH_LIBRARY_IMPL(raft_amd, CUDA, m) {
  m.impl("augment_batch", &raft_amd::augment_batch);
  m.impl("augment_batch_sparse", &raft_amd::augment_batch_sparse);
}
