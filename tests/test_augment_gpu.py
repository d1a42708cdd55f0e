"""The HIP augmentation op raft_amd::augment_batch (csrc/augment.hip) against the CPU torch path
``BatchAugmentor.apply`` with the same explicit parameters (augment_cases.py)."""
import functools

import pytest
import torch

import augment_cases as ac
from raft_ros_amd.data import augment as A

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _native(name):
    """The native path on the case, through BatchAugmentor: (img1, img2, flow, valid) on the CPU."""
    case = ac.get_case(name)
    aug = A.BatchAugmentor(case.specs, device=_cuda(), native=True)
    out = aug.apply(case.batch, case.params)
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


def _check_flow(name, got, want, keep=None):
    d = (got[2] - want[2]).abs()
    if keep is not None:
        d = d[keep.expand_as(d)]
    print(f"{name} flow: largest difference {d.max().item():.2e}")
    assert d.max() <= ac.FLOW_ATOL, name


@pytest.mark.parametrize("name", [n for n in ac.CASE_NAMES if n not in ("invalid", "sparse_mix")])
def test_against_cpu_torch_path(name):
    """Exact cases (jitter, eraser, flips and crops at pixel centres; the tail shapes): images
    bitwise.  General cases (resize, stretch): within the caps.  Flow within 1e-3, valid equal."""
    case = ac.get_case(name)
    got, want = _native(name), ac.oracle(name)
    assert [t.shape for t in got] == [t.shape for t in want]
    _check_images(name, case.kind, got, want)
    _check_flow(name, got, want)
    assert torch.equal(got[3], want[3])


def test_invalid_flow_block():
    case = ac.get_case("invalid")
    got, want = _native("invalid"), ac.oracle("invalid")
    _check_images("invalid", case.kind, got, want)
    i = case.invalid_block[0]
    ring, inside = ac.invalid_masks(case)
    assert ring.float().mean() < 0.25 and inside.any()
    keep = torch.ones_like(got[3], dtype=torch.bool)
    keep[i] = ~ring
    assert torch.equal(got[3][keep], want[3][keep])
    assert (got[3][i][inside] == 0).all()  # inside the block every pixel is invalid
    assert (got[3][i][~ring & ~inside] == 1).all() and (got[3][1 - i] == 1).all()
    _check_flow("invalid", got, want, keep=(keep & (want[3] > 0))[:, None])


def test_sparse_mixture():
    """Images like every other case; the sparse sample's flow and valid are those of the torch
    path on the same device, bitwise: it is the same code."""
    dev = _cuda()
    case = ac.get_case("sparse_mix")
    got, want = _native("sparse_mix"), ac.oracle("sparse_mix")
    _check_images("sparse_mix", case.kind, got, want)
    torch_gpu = A.BatchAugmentor(case.specs, device=dev, native=False).apply(case.batch, case.params)
    for i in range(len(case.samples)):
        if i in case.sparse_ids:
            assert torch.equal(got[2][i], torch_gpu[2][i].cpu()) and torch.equal(got[3][i], torch_gpu[3][i].cpu())
            assert 0 < got[3][i].mean() < 1
        else:
            assert (got[2][i] - want[2][i]).abs().max() <= ac.FLOW_ATOL and torch.equal(got[3][i], want[3][i])


@pytest.mark.parametrize("name", ["exact2", "general1", "tail_w97"])
def test_sample_of_a_batch_equals_the_sample_alone(name):
    """Bitwise: a sample's result depends neither on its neighbours nor on the padded size."""
    dev = _cuda()
    case = ac.get_case(name)
    got = _native(name)
    aug = A.BatchAugmentor(case.specs, device=dev, native=True)
    for i, s in enumerate(case.samples):
        alone = aug.apply(A.collate_padded([s]), {k: v[i:i + 1] for k, v in case.params.items()})
        for k in range(4):
            assert torch.equal(alone[k][0].cpu(), got[k][i]), (name, i, k)


def test_same_call_twice_is_bitwise_equal():
    for name in ("exact0", "general0"):
        case = ac.get_case(name)
        again = A.BatchAugmentor(case.specs, device=_cuda(), native=True).apply(case.batch, case.params)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(again, _native(name)))


def test_wiring_same_seed_same_parameters():
    """native=True and native=False on the GPU: the same draws, outputs within the general caps."""
    dev = _cuda()
    case = ac.get_case("general0")
    nat = A.BatchAugmentor(case.specs, seed=7, device=dev, native=True)
    ref = A.BatchAugmentor(case.specs, seed=7, device=dev, native=False)
    for _ in range(2):
        pn, pr = nat.draw(case.batch), ref.draw(case.batch)
        assert pn.keys() == pr.keys() and all(torch.equal(pn[k], pr[k]) for k in pn)
    nat.gen.manual_seed(7)
    ref.gen.manual_seed(7)
    got = [t.cpu() for t in nat(case.batch)]
    want = [t.cpu() for t in ref(case.batch)]
    _check_images("wiring", "general", got, want)
    _check_flow("wiring", got, want)
    assert torch.equal(got[3], want[3])


def test_op_rejects_bad_arguments():
    from raft_ros_amd.ops.augment import augment_batch

    dev = _cuda()
    case = ac.get_case("tail_full")
    b = {k: v.to(dev) for k, v in case.batch.items()}
    p = {k: v.to(dev) for k, v in case.params.items()}
    with pytest.raises(ValueError):
        augment_batch(case.batch["img1"], case.batch["img2"], case.batch["flow"], case.batch["size"], case.params, case.crop)
    with pytest.raises(RuntimeError):  # size of another batch
        augment_batch(b["img1"], b["img2"], b["flow"], b["size"].repeat(2, 1), p, case.crop)
    with pytest.raises(RuntimeError):  # flow of another shape
        augment_batch(b["img1"], b["img2"], b["flow"][:, :-1], b["size"], p, case.crop)
