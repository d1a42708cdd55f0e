"""The draw / apply split of ``BatchAugmentor``, the ``native`` switch on the CPU, the hygiene of
the cases that test_augment_gpu.py holds the HIP op to, and the op's fake kernel."""
from argparse import Namespace

import pytest
import torch

import augment_cases as ac
from raft_ros_amd.data import augment as A
from raft_ros_amd.data import datasets as D
from raft_ros_amd.ops import _ext
from raft_ros_amd.ops.augment import PF, PI, pack_params

PARAM_KEYS = {"f1", "o1", "f2", "o2", "asym", "erase", "nbox", "boxes", "sx", "sy", "resize", "rh", "rw", "hflip",
              "vflip", "x0", "y0", "sparse"}


def _mixture(spec_ids, seed=0):
    specs = [A.AugSpec((64, 96), -0.1, 1.0, True, False), A.AugSpec((64, 96), -0.2, 0.4, True, True)]
    samples = [ac.make_sample(100, 150, seed, noise=True, sparse=spec_ids[0] == 1),
               ac.make_sample(80, 120, seed + 1, noise=True, sparse=spec_ids[1] == 1),
               ac.make_sample(120, 110, seed + 2, sparse=spec_ids[2] == 1)]
    for s, sid in zip(samples, spec_ids):
        s["spec"] = sid
    return specs, A.collate_padded(samples)


@pytest.mark.parametrize("spec_ids", [(0, 0, 0), (1, 1, 1), (0, 1, 0)], ids=["dense", "sparse", "mixed"])
def test_apply_of_draw_is_call(spec_ids):
    for seed in (0, 5):
        specs, batch = _mixture(spec_ids, seed)
        a, b = A.BatchAugmentor(specs, seed=seed), A.BatchAugmentor(specs, seed=seed)
        for _ in range(2):  # the second batch: the generator moved on alike
            want = a(batch)
            params = b.draw(batch)
            assert set(params) == PARAM_KEYS
            assert all(v.shape[0] == 3 for v in params.values())
            got = b.apply(batch, params)
            assert all(torch.equal(g, w) for g, w in zip(got, want))
    # the asymmetric selection is folded into image 2's factors and order
    sym = ~params["asym"]
    assert torch.equal(params["f2"][sym], params["f1"][sym]) and torch.equal(params["o2"][sym], params["o1"][sym])


@pytest.mark.parametrize("spec_ids", [(0, 0, 0), (0, 1, 0)], ids=["dense", "mixed"])
def test_native_switch_changes_nothing_on_the_cpu(spec_ids):
    specs, batch = _mixture(spec_ids, 3)
    want = A.BatchAugmentor(specs, seed=4, native=False)(batch)
    got = A.BatchAugmentor(specs, seed=4, device="cpu", native=True)(batch)
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_fetch_dataloader_passes_native_augment(tmp_path, monkeypatch):
    from test_data_cpu import _fake_kitti, _fake_sintel

    monkeypatch.setenv("RAFT_DATASET_ROOT", str(tmp_path))
    _fake_sintel(str(tmp_path), h=96, w=128)
    _fake_kitti(str(tmp_path), h=96, w=140)
    args = Namespace(stage="sintel", image_size=[64, 96], batch_size=2, num_workers=0, device="cpu")
    assert D.fetch_dataloader(args).augmentor.native is False
    args.native_augment = True
    loader = D.fetch_dataloader(args)
    assert loader.augmentor.native is True
    i1, _, flow, valid = next(iter(loader))  # a CPU device: the torch path
    assert i1.shape == (2, 3, 64, 96) and flow.shape == (2, 2, 64, 96) and valid.shape == (2, 64, 96)


@pytest.mark.parametrize("name", ac.CASE_NAMES)
def test_case_hygiene_no_mean_on_a_rounding_boundary(name):
    """With fp32 and with fp64 means the torch path gives the same images: no contrast or eraser
    mean of the case sits where a correct kernel and the fp32 sum may disagree.  A case that
    fails is given another seed in augment_cases.py."""
    case = ac.get_case(name)
    o32, o64 = ac.oracle(name), ac.oracle(name, torch.float64)
    assert torch.equal(o32[0], o64[0]) and torch.equal(o32[1], o64[1])
    # image 2's channel sums stay exact in fp32
    assert max(h * w for h, w in case.sizes) * 255 < 2 ** 24


def test_cases_cover_what_they_claim():
    cases = ac.all_cases()
    assert [c.name for c in cases] == ac.CASE_NAMES
    exact = [c for c in cases if c.name.startswith("exact")]
    orders = {tuple(o) for c in exact for o in c.params["o1"].tolist()}
    assert orders == set(ac.PERMS)  # all 24 round orders
    for c in exact:
        p = c.params
        assert not p["resize"].any() and p["asym"].any() and not p["asym"].all()
        assert len({s for s in c.sizes}) > 1  # mixed sizes: size < (Hm, Wm) for some sample
    flips = {(bool(h), bool(v)) for c in exact for h, v in zip(c.params["hflip"], c.params["vflip"])}
    assert len(flips) == 4
    nbox = {int(n) if e else 0 for c in exact for n, e in zip(c.params["nbox"], c.params["erase"])}
    assert nbox == {0, 1, 2}
    assert any(c.crop[1] % 4 for c in cases) and any(c.crop[0] == 1 for c in cases)
    for c in cases:
        assert c.batch["img1"].shape[0] <= 4
    inv = ac.get_case("invalid")
    ring, inside = ac.invalid_masks(inv)
    assert 0 < ring.float().mean() < 0.25 and inside.any()


@pytest.mark.parametrize("name", [n for n in ac.CASE_NAMES if ac.get_case(n).kind == "general"])
def test_fp64_sampling_switch_stays_well_inside_the_general_caps(name):
    """The torch path against itself with fp64 bilinear sampling, on every general case: the
    oracle's own error is at most a quarter of the share the GPU tests allow, so the cap measures
    the op and not the case."""
    case = ac.get_case(name)
    o64 = A.BatchAugmentor(case.specs).apply(case.batch, case.params, sample_fp64=True)
    o32 = ac.oracle(name)
    assert all(t.dtype == torch.float32 for t in o64)
    for k in range(2):
        d = (o32[k] - o64[k]).abs()
        assert d.max() <= ac.IMG_MAX_LEVELS and (d > 0).float().mean() <= ac.IMG_MAX_FRACTION / 4
    ok = (o32[3] > 0)[:, None].expand_as(o32[2])  # not the block of invalid flow
    assert (o32[2] - o64[2]).abs()[ok].max() <= ac.FLOW_ATOL
    if case.invalid_block is None:
        assert torch.equal(o32[3], o64[3])


def test_pack_params_layout():
    case = ac.get_case("exact1")
    p = case.params
    pf, pi = pack_params(p)
    B = p["sx"].shape[0]
    assert pf.shape == (B, PF) and pf.dtype == torch.float32 and pi.shape == (B, PI) and pi.dtype == torch.int32
    assert torch.equal(pf[:, 0:4], p["f1"]) and torch.equal(pf[:, 4:8], p["f2"])
    assert torch.equal(pf[:, 8], p["sx"]) and torch.equal(pf[:, 9], p["sy"])
    assert torch.equal(pi[:, 0:4].long(), p["o1"]) and torch.equal(pi[:, 4:8].long(), p["o2"])
    assert torch.equal(pi[:, 8].bool(), p["asym"])
    assert torch.equal(pi[:, 9].long(), torch.where(p["erase"], p["nbox"], torch.zeros_like(p["nbox"])))
    assert torch.equal(pi[:, 10:18].long().view(B, 2, 4), p["boxes"])
    assert torch.equal(pi[:, 18:24].long(), torch.stack([p["rh"], p["rw"], p["hflip"].long(), p["vflip"].long(),
                                                         p["x0"], p["y0"]], 1))


@pytest.mark.skipif(not _ext.is_loaded(), reason=f"native library not built: {_ext.load_error()}")
def test_meta_shape_of_augment_batch():
    m = torch.device("meta")
    img = torch.empty(3, 120, 160, 3, device=m, dtype=torch.uint8)
    flow = torch.empty(3, 120, 160, 2, device=m)
    size = torch.empty(3, 2, device=m, dtype=torch.long)
    pf = torch.empty(3, PF, device=m)
    pi = torch.empty(3, PI, device=m, dtype=torch.int32)
    i1, i2, f, v = _ext.ops().augment_batch(img, img, flow, size, pf, pi, 64, 96)
    assert i1.shape == i2.shape == (3, 3, 64, 96) and f.shape == (3, 2, 64, 96) and v.shape == (3, 64, 96)
    assert i1.dtype == f.dtype == v.dtype == torch.float32
