"""Sparse ground truth in the HIP augmentation op, the parts that need no GPU: the flags layout, the
wrapper's ``valid`` keyword on CPU tensors, the fake kernel of raft_amd::augment_batch_sparse, and
the hygiene of the cases that test_augment_sparse_gpu.py holds the op to."""
import pytest
import torch

import augment_cases as ac
import augment_sparse_cases as sc
from raft_ros_amd.data import augment as A
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops import augment as ops_augment
from raft_ros_amd.ops.augment import PF, PI


def test_pack_flags_layout():
    p = {"sparse": torch.tensor([False, True, False, True]), "resize": torch.tensor([False, False, True, True])}
    flags = ops_augment.pack_flags(p)
    assert flags.dtype == torch.int32 and flags.shape == (4,) and flags.is_contiguous()
    assert flags.tolist() == [0, 1, 2, 3]  # bit 0 sparse, bit 1 resize
    assert (ops_augment.SPARSE, ops_augment.RESIZE) == (1, 2)
    case = sc.get_case("down_flip_tail")
    flags = ops_augment.pack_flags(case.params)
    assert torch.equal((flags & 1).bool(), case.params["sparse"]) and torch.equal((flags & 2).bool(), case.params["resize"])
    assert flags.tolist() == [3, 2, 3]


def test_wrapper_with_valid_needs_gpu_tensors():
    case = sc.get_case("up_aniso")
    b = case.batch
    with pytest.raises(ValueError):
        ops_augment.augment_batch(b["img1"], b["img2"], b["flow"], b["size"], case.params, case.crop, valid=b["valid"])


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_meta_shape_of_augment_batch_sparse():
    m = torch.device("meta")
    img = torch.empty(3, 120, 160, 3, device=m, dtype=torch.uint8)
    flow = torch.empty(3, 120, 160, 2, device=m)
    valid = torch.empty(3, 120, 160, device=m)
    size = torch.empty(3, 2, device=m, dtype=torch.long)
    pf = torch.empty(3, PF, device=m)
    pi = torch.empty(3, PI, device=m, dtype=torch.int32)
    flags = torch.empty(3, device=m, dtype=torch.int32)
    i1, i2, f, v = _ext.ops().augment_batch_sparse(img, img, flow, valid, size, pf, pi, flags, 64, 97)
    assert i1.shape == i2.shape == (3, 3, 64, 97) and f.shape == (3, 2, 64, 97) and v.shape == (3, 64, 97)
    assert i1.dtype == f.dtype == v.dtype == torch.float32 and i1.device.type == "meta"


def test_native_switch_changes_nothing_on_the_cpu():
    """The sparse cases through ``native=True`` on a CPU device: the torch path, ``_sparse_flow``."""
    for name in ("down_half", "noresize"):
        case = sc.get_case(name)
        got = A.BatchAugmentor(case.specs, device="cpu", native=True).apply(case.batch, case.params)
        assert all(torch.equal(g, w) for g, w in zip(got, sc.oracle(name)))


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_case_hygiene(name):
    """As for the cases of augment_cases.py: no contrast or eraser mean on a rounding boundary
    (fp32 and fp64 means give the same images), and on the general cases the oracle against itself
    with fp64 sampling stays within a quarter of the share the GPU test allows, so the caps measure
    the op and not the case."""
    case = sc.get_case(name)
    o32, o64 = sc.oracle(name), sc.oracle(name, torch.float64)
    assert torch.equal(o32[0], o64[0]) and torch.equal(o32[1], o64[1])
    assert max(h * w for h, w in case.sizes) * 255 < 2 ** 24
    assert case.batch["img1"].shape[0] <= 4
    if case.kind == "general":
        s64 = A.BatchAugmentor(case.specs).apply(case.batch, case.params, sample_fp64=True)
        for k in range(2):
            d = (o32[k] - s64[k]).abs()
            assert d.max() <= ac.IMG_MAX_LEVELS and (d > 0).float().mean() <= ac.IMG_MAX_FRACTION / 4
        assert torch.equal(o32[3], s64[3])
    else:
        assert not case.params["resize"].any()


def test_premise_counts_agree_with_the_oracle():
    """``premise`` counts the landing sources with plain loops: where it counts none the oracle's
    valid is 0, elsewhere 1, on every sparse sample of every case."""
    for name in sc.CASE_NAMES:
        case = sc.get_case(name)
        assert list(case.params["sparse"].nonzero().flatten()) == list(case.sparse_ids)
        for i in case.sparse_ids:
            assert torch.equal(sc.oracle(name)[3][i], (sc.premise(case, i)["count"] > 0).float()), (name, i)
