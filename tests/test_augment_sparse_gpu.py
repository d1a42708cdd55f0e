"""Sparse ground truth (KITTI, HD1K) inside the HIP augmentation op raft_amd::augment_batch_sparse
(csrc/augment.hip) against the CPU torch path, ``BatchAugmentor.apply`` with ``_sparse_flow``, on
the cases of augment_sparse_cases.py.  A sparse sample's flow and valid are integer work and one
fp32 multiply: they must equal the oracle bitwise."""
import functools

import pytest
import torch

import augment_cases as ac
import augment_sparse_cases as sc
from raft_ros_amd.data import augment as A

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _native(name):
    """The native path on the case, through BatchAugmentor: (img1, img2, flow, valid) on the CPU."""
    case = sc.get_case(name)
    out = A.BatchAugmentor(case.specs, device=_cuda(), native=True).apply(case.batch, case.params)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in out)
    return tuple(t.cpu() for t in out)


def _check_images(name, kind, got, want):
    for k in range(2):
        d = (got[k] - want[k]).abs()
        diff, worst = (d > 0).float().mean().item(), d.max().item()
        print(f"{name} img{k + 1}: {diff:.2e} of the pixel-channels differ, largest difference {worst:g}")
        if kind == "exact":
            assert torch.equal(got[k], want[k]), f"{name} img{k + 1}"
        else:
            assert worst <= ac.IMG_MAX_LEVELS and diff <= ac.IMG_MAX_FRACTION, f"{name} img{k + 1}"


def _check_premise(name, case, want):
    """The branch the case is there for, measured on the oracle and the case itself."""
    pr = {i: sc.premise(case, i) for i in case.sparse_ids}
    p = case.params
    if name == "down_half":
        assert p["sx"][0] == 0.5 and p["sy"][0] == 0.5
        assert pr[0]["ties"] > 0  # x * 0.5 on .5: half to even
        assert (pr[0]["count"] >= 2).sum() > 1000 and pr[0]["count"].max() == 9  # 3 x 3 sources on one target
    elif name == "down_flip_tail":
        assert case.crop[1] % 4 != 0 and len(set(case.sizes)) == 3 and not p["sparse"][1]
        assert p["hflip"][0] and not p["hflip"][2]
        for i in (0, 2):
            assert (pr[i]["count"] >= 2).sum() > 100
        # the crop starts at the origin: the 0 < xn, 0 < yn rule empties its row 0 and column 0,
        # though the source has valid pixels there
        assert p["x0"][2] == 0 and p["y0"][2] == 0 and pr[2]["row0"] > 0 and pr[2]["col0"] > 0
        assert want[3][2][0].sum() == 0 and want[3][2][:, 0].sum() == 0 and want[3][2][1:, 1:].sum() > 0
    elif name == "up_aniso":
        assert p["sx"][0] > 1 and p["sy"][0] > 1 and p["sx"][0] != p["sy"][0]
        assert pr[0]["count"].max() == 1 and 0 < want[3][0].mean() < 0.5  # holes, no collisions
    elif name == "noresize":
        assert not p["resize"].any()
        # without resize the inside rule does not apply: the source's row 0 and column 0 arrive
        assert p["x0"][0] == 0 and p["y0"][0] == 0 and want[3][0][0].sum() > 0 and want[3][0][:, 0].sum() > 0
        assert p["hflip"][1] and want[3][1][:, -1].sum() > 0  # flipped, far origin: column 0 is the last column
        for i in (0, 1):
            assert pr[i]["count"].max() == 1 and 0 < want[3][i].mean() < 1
    elif name == "edge_valid":
        assert (case.samples[0]["valid"] == 0).all()
        assert want[2][0].abs().max() == 0 and want[3][0].max() == 0
        assert set(case.samples[1]["valid"].unique().tolist()) == {0.0, 0.5, 1.0}
        half = sc.premise(case, 1, thresh=0.5)["count"]
        assert ((half > 0) & (pr[1]["count"] == 0)).sum() > 100  # where only a 0.5 lands: not valid
        assert 0 < want[3][1].mean() < 1
    else:
        raise AssertionError(name)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_sparse_flow_and_valid_equal_the_cpu_oracle_bitwise(name):
    case = sc.get_case(name)
    got, want = _native(name), sc.oracle(name)
    assert [t.shape for t in got] == [t.shape for t in want]
    _check_premise(name, case, want)
    _check_images(name, case.kind, got, want)
    for i in range(len(case.samples)):
        if i in case.sparse_ids:
            wrong_f = (got[2][i] != want[2][i]).sum().item()
            wrong_v = (got[3][i] != want[3][i]).sum().item()
            print(f"{name} sample {i}: {wrong_f} flow values and {wrong_v} valid values differ")
            assert torch.equal(got[2][i], want[2][i]) and torch.equal(got[3][i], want[3][i]), (name, i)
        else:
            assert (got[2][i] - want[2][i]).abs().max() <= ac.FLOW_ATOL and torch.equal(got[3][i], want[3][i]), (name, i)


@pytest.mark.parametrize("name", ["down_half", "down_flip_tail", "noresize"])
def test_sparse_sample_of_a_batch_equals_the_sample_alone(name):
    """Bitwise: the winner is the largest source index in the batch's padded width or the sample's
    own, which order the sources alike."""
    dev = _cuda()
    case = sc.get_case(name)
    got = _native(name)
    aug = A.BatchAugmentor(case.specs, device=dev, native=True)
    for i, s in enumerate(case.samples):
        alone = aug.apply(A.collate_padded([s]), {k: v[i:i + 1] for k, v in case.params.items()})
        for k in range(4):
            assert torch.equal(alone[k][0].cpu(), got[k][i]), (name, i, k)


def test_same_call_twice_is_bitwise_equal():
    for name in ("down_half", "down_flip_tail"):
        case = sc.get_case(name)
        again = A.BatchAugmentor(case.specs, device=_cuda(), native=True).apply(case.batch, case.params)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(again, _native(name)))


def test_apply_is_capturable_in_a_graph():
    """``apply`` with sparse samples reads nothing back, so it can be captured.  The replay must zero
    the winner buffer itself: after other flow and valid are written into the captured inputs, a
    second replay equals the eager call on them."""
    dev = _cuda()
    case = sc.get_case("down_flip_tail")
    aug = A.BatchAugmentor(case.specs, device=dev, native=True)
    batch = {k: v.to(dev) for k, v in case.batch.items()}
    params = {k: v.to(dev) for k, v in case.params.items()}
    eager = [t.clone() for t in aug.apply(batch, params)]  # the warm-up call
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = aug.apply(batch, params)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o, e) for o, e in zip(out, eager))
    assert torch.equal(out[2].cpu(), _native("down_flip_tail")[2])
    # other ground truth of the same sizes, written in place
    others = [ac.make_sample(h, w, 650 + i, sparse=i in case.sparse_ids) for i, (h, w) in enumerate(case.sizes)]
    for s, spec in zip(others, case.batch["spec"].tolist()):
        s["spec"] = spec
    other = A.collate_padded(others)
    batch["flow"].copy_(other["flow"])
    batch["valid"].copy_(other["valid"])
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in out]
    eager = aug.apply(batch, params)
    assert all(torch.equal(r, e) for r, e in zip(replayed, eager))
    assert not torch.equal(replayed[3].cpu(), _native("down_flip_tail")[3])  # it is other data


def test_op_rejects_bad_arguments():
    from raft_ros_amd.ops._ext import ops
    from raft_ros_amd.ops.augment import augment_batch, pack_flags, pack_params

    dev = _cuda()
    case = sc.get_case("up_aniso")
    b = {k: v.to(dev) for k, v in case.batch.items()}
    p = {k: v.to(dev) for k, v in case.params.items()}
    augment_batch(b["img1"], b["img2"], b["flow"], b["size"], p, case.crop, valid=b["valid"])  # as it should be
    with pytest.raises(RuntimeError):  # valid of another shape
        augment_batch(b["img1"], b["img2"], b["flow"], b["size"], p, case.crop, valid=b["valid"][:, :-1])
    pf, pi = pack_params(p)
    flags = pack_flags(p)
    args = (b["img1"], b["img2"], b["flow"], b["valid"], b["size"], pf, pi, flags, *case.crop)
    ops().augment_batch_sparse(*args)
    with pytest.raises(RuntimeError):  # valid of another dtype
        ops().augment_batch_sparse(*args[:3], b["valid"].double(), *args[4:])
    with pytest.raises(RuntimeError):  # flags of another length
        ops().augment_batch_sparse(*args[:7], flags.repeat(2), *args[8:])
    with pytest.raises(RuntimeError):  # flags of another dtype
        ops().augment_batch_sparse(*args[:7], flags.long(), *args[8:])
