"""Forward-backward consistency on the GPU: the HIP op bitwise against the torch reference on the
host copy of the same flows (``occ``, ``err2`` with its infinities, ``counts``), and
``FlowInference``'s bidirectional mode.

The specification fixes every rounding step, so no tolerance applies (consistency_cases.same: as
``torch.equal``, with a NaN equal to a NaN at the same place).
"""
import numpy as np
import pytest
import torch

import consistency_cases as cc
from raft_ros_amd.ops.consistency import fb_consistency, fb_consistency_ref
from raft_ros_amd.ros.node import FlowInference

pytestmark = pytest.mark.gpu


def _run(fw, bw, dev, *alphas, what=""):
    """Host flows (B, 2, H, W) -> the op's results, checked against the reference on the host."""
    got = fb_consistency(fw.to(dev), bw.to(dev), *alphas)
    assert all(g.device.type == "cuda" for g in got)
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.float32 and got[2].dtype == torch.int32
    cc.check(got, fb_consistency_ref(fw, bw, *alphas), what)
    return [g.cpu() for g in got]


def test_parity_field(cuda):
    fw, bw = cc.parity_pair()
    occ, err2, counts = _run(fw[None], bw[None], cuda, what="37x41")
    assert min(cc.class_shares(occ)) >= cc.MIN_SHARE
    one = fb_consistency(fw.to(cuda), bw.to(cuda))  # (2, H, W) in: B dropped
    assert one[0].shape == (37, 41) and one[2].shape == (2,)
    assert torch.equal(one[0].cpu(), occ[0]) and torch.equal(one[1].cpu(), err2[0]) and torch.equal(one[2].cpu(), counts[0])


def test_batch_with_unaligned_bases(cuda):
    fw, bw = cc.scaled_batch()
    assert (37 * 41) % 4 != 0
    occ, err2, counts = _run(fw, bw, cuda, what="B=3 scales 1/0.5/2")
    for b in range(3):  # an image of a batch is that image alone
        one = fb_consistency(fw[b].to(cuda), bw[b].to(cuda))
        assert torch.equal(one[0].cpu(), occ[b]) and torch.equal(one[1].cpu(), err2[b])
        assert torch.equal(one[2].cpu(), counts[b])


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (5, 3), (8, 16)])
def test_tails_one_row_and_vector_paths(cuda, shape):
    fw, bw = cc.random_pair(*shape, seed=2)
    _run(fw[None], bw[None], cuda, what=f"{shape}")
    pairs = [cc.random_pair(*shape, seed=s) for s in (5, 6, 7)]
    _run(torch.stack([p[0] for p in pairs]), torch.stack([p[1] * k for p, k in zip(pairs, (1.0, 0.25, 3.0))]), cuda,
         what=f"B=3 {shape}")


def test_edge_field(cuda):
    fw, bw = cc.edge_pair()
    other = cc.random_pair(cc.EDGE_H, cc.EDGE_W, seed=21)
    occ, err2, _ = _run(torch.stack([fw, other[0]]), torch.stack([bw, other[1]]), cuda, what="edge 16x24")
    for (y, x), (_, want) in cc.EDGE_POINTS.items():
        if want is not None:
            assert occ[0, y, x] == want and err2[0, y, x] == float("inf"), (y, x)
        else:
            assert occ[0, y, x] != 2 and torch.isfinite(err2[0, y, x]), (y, x)
    alone = fb_consistency(other[0].to(cuda), other[1].to(cuda))
    assert torch.equal(alone[0].cpu(), occ[1]) and torch.equal(alone[1].cpu(), err2[1])


def test_nonfinite_field(cuda):
    fw, bw = cc.nonfinite_pair()
    other = cc.random_pair(9, 13, seed=22)
    occ, err2, counts = _run(torch.stack([fw, other[0]]), torch.stack([bw, other[1]]), cuda, what="non-finite 9x13")
    for (_, y, x) in cc.NONFINITE_FW:
        assert occ[0, y, x] == 2 and err2[0, y, x] == float("inf")
    y, x = cc.NONFINITE_SAMPLER
    assert occ[0, y, x] == 1 and torch.isnan(err2[0, y, x])
    # the other image of the batch does not see them
    alone = fb_consistency(other[0].to(cuda), other[1].to(cuda))
    assert torch.equal(alone[0].cpu(), occ[1]) and torch.equal(alone[1].cpu(), err2[1])
    assert torch.equal(alone[2].cpu(), counts[1])


@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 16, 16)])
def test_zero_flows(cuda, shape):
    B, H, W = shape
    z = torch.zeros(B, 2, H, W, device=cuda)
    occ, err2, counts = fb_consistency(z, z)
    assert (occ == 0).all() and (err2 == 0).all() and (counts == 0).all()


def test_constant_flow_leaves_on_the_right(cuda):
    fw = torch.zeros(1, 2, 12, 20)
    fw[:, 0] = 3.0
    occ, err2, counts = _run(fw, -fw, cuda, what="+3 / -3")
    assert (occ[0, :, :17] == 0).all() and (err2[0, :, :17] == 0).all()
    assert (occ[0, :, 17:] == 2).all() and torch.isinf(err2[0, :, 17:]).all()
    assert counts.tolist() == [[0, 3 * 12]]


def test_components_and_axes_are_not_swapped(cuda):
    """u large, v small on the non-square field: x + v or reading component 1 for u would show."""
    fw, bw = cc.parity_pair()
    scale = torch.tensor([3.0, 0.2])[:, None, None]
    fw, bw = (fw * scale).contiguous(), (bw * scale).contiguous()
    occ, _, _ = _run(fw[None], bw[None], cuda, what="u >> v")
    swapped = fb_consistency_ref(fw.flip(0)[None].contiguous(), bw.flip(0)[None].contiguous())[0]
    assert not torch.equal(occ, swapped)  # the case can tell


def test_non_default_alphas(cuda):
    fw, bw = cc.parity_pair()
    base = _run(fw[None], bw[None], cuda, what="defaults")
    tight = _run(fw[None], bw[None], cuda, 0.0, 1e-3, what="alpha 0 / 1e-3")
    loose = _run(fw[None], bw[None], cuda, 0.5, 4.0, what="alpha 0.5 / 4")
    assert tight[2][0, 0] > base[2][0, 0] > loose[2][0, 0]
    assert tight[2][0, 1] == base[2][0, 1] == loose[2][0, 1]  # leaving the frame does not depend on them


def test_workload_shape_determinism_and_graph(cuda):
    """440 x 1024 once: parity, two calls bitwise equal, and a captured graph replayed on refilled
    inputs equal to the eager result."""
    (fw, bw), want = cc.workload()
    d_fw, d_bw = fw.to(cuda)[None], bw.to(cuda)[None]
    out = fb_consistency(d_fw, d_bw)
    cc.check(out, want, "440x1024")
    again = fb_consistency(d_fw, d_bw)
    assert all(torch.equal(a, o) for a, o in zip(again, out))

    s_fw, s_bw = torch.zeros_like(d_fw), torch.zeros_like(d_bw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fb_consistency(s_fw, s_bw)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fb_consistency(s_fw, s_bw)
    s_fw.copy_(d_fw)
    s_bw.copy_(d_bw)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(c, o) for c, o in zip(captured, out))
    graph.replay()  # the counts are zeroed inside the graph: a second replay does not add up
    torch.cuda.synchronize()
    assert torch.equal(captured[2], out[2])


def test_determinism_small_unaligned(cuda):
    fw, bw = [t.to(cuda) for t in cc.scaled_batch()]
    a, b = fb_consistency(fw, bw), fb_consistency(fw, bw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_op_argument_checks(cuda):
    op = torch.ops.raft_amd.fb_consistency
    f = torch.zeros(1, 2, 4, 8, device=cuda)
    with pytest.raises(RuntimeError):
        op(f.half(), f.half(), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f, f.half(), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(torch.zeros(1, 2, 4, 16, device=cuda)[..., ::2], f, 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f, torch.zeros(1, 2, 4, 16, device=cuda)[..., ::2], 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f, torch.zeros(1, 2, 8, 4, device=cuda), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f, torch.zeros(2, 2, 4, 8, device=cuda), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(torch.zeros(1, 3, 4, 8, device=cuda), torch.zeros(1, 3, 4, 8, device=cuda), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f, f.cpu(), 0.01, 0.5)
    with pytest.raises(RuntimeError):
        op(f.cpu(), f.cpu(), 0.01, 0.5)
    # empty inputs: empty outputs
    occ, err2, counts = op(torch.zeros(0, 2, 4, 8, device=cuda), torch.zeros(0, 2, 4, 8, device=cuda), 0.01, 0.5)
    assert occ.shape == (0, 4, 8) and err2.shape == (0, 4, 8) and counts.shape == (0, 2)
    occ, err2, counts = op(torch.zeros(2, 2, 0, 8, device=cuda), torch.zeros(2, 2, 0, 8, device=cuda), 0.01, 0.5)
    assert occ.shape == (2, 0, 8) and counts.cpu().tolist() == [[0, 0], [0, 0]]
    # non-contiguous or half-precision flows go through the Python layer's conversion
    fw, bw = cc.random_pair(6, 10, seed=3)
    cc.check(fb_consistency(fw.to(cuda).half()[None], bw.to(cuda).half()[None]),
             fb_consistency_ref(fw.half().float()[None], bw.half().float()[None]), "fp16 flows")
    wide_f, wide_b = torch.zeros(1, 2, 6, 20, device=cuda), torch.zeros(1, 2, 6, 20, device=cuda)
    wide_f[..., ::2], wide_b[..., ::2] = fw.to(cuda), bw.to(cuda)
    cc.check(fb_consistency(wide_f[..., ::2], wide_b[..., ::2]), fb_consistency_ref(fw[None], bw[None]), "strided flows")


# ---------------------------------------------------------------------------- FlowInference
def test_flow_inference_consistency(cuda):
    """Random-weight RAFT-small, 124 x 150 frames (padded to 128 x 152), one instance with
    ``device_io`` switched: the same weights and the same captured graphs."""
    torch.manual_seed(0)
    inf = FlowInference(None, small=True, device="cuda", iters=2, consistency=True)
    rng = np.random.RandomState(0)
    a, b, c = [(rng.rand(124, 150, 3) * 255).astype(np.uint8) for _ in range(3)]
    levels = np.array([0, 128, 255], np.uint8)
    for k, (p, q) in enumerate(((a, b), (b, c))):
        for device_io in (False, True):
            inf.device_io = device_io
            flow_fw, occ, err2, counts = [t.clone() for t in inf.flow_checked(p, q)]
            assert flow_fw.shape == (1, 2, 128, 152) and occ.shape == (1, 128, 152) and counts.shape == (1, 2)
            # the model's own output on the stacked batch, through the same runner
            with torch.inference_mode():  # as flow_checked runs it: the graph's buffers are inference tensors
                i1, i2 = inf._padded_pair(p, q)
                _, up = inf.runner(torch.cat([i1, i2]), torch.cat([i2, i1]))
                want = fb_consistency(up[0:1], up[1:2])
            assert torch.equal(flow_fw, up[0:1])
            assert torch.equal(occ, want[0]) and cc.same(err2, want[1]) and torch.equal(counts, want[2])
            cc.check((occ, err2, counts), fb_consistency_ref(up[0:1].cpu(), up[1:2].cpu()), f"pair {k} vs host")
            single = inf.flow(p, q)
            print(f"pair {k} device_io {device_io}: max |flow_fw - flow()| = {(flow_fw - single).abs().max().item():.3e}, "
                  f"counts {counts[0].tolist()}")
            img, mask = inf.visualize_checked(p, q)
            assert img.shape == (128, 152, 3) and img.dtype == np.uint8 and img.flags.owndata and img.flags.c_contiguous
            assert mask.shape == (128, 152) and mask.dtype == np.uint8 and mask.flags.owndata and mask.flags.c_contiguous
            assert set(np.unique(mask).tolist()) <= {0, 128, 255}
            assert np.array_equal(mask, levels[occ[0].cpu().numpy()])
            assert inf.last_counts.shape == (2,) and inf.last_counts.tolist() == counts[0].tolist()
            assert inf.last_counts.tolist() == [int((mask == 128).sum()), int((mask == 255).sum())]
    first_img, first_mask = inf.visualize_checked(a, b)
    inf.visualize_checked(b, c)  # the returned arrays own their memory: the next call does not change them
    again_img, again_mask = inf.visualize_checked(a, b)
    assert first_img.tobytes() == again_img.tobytes() and first_mask.tobytes() == again_mask.tobytes()
