"""GPU: the augmentation kernels (csrc/omni_augment.hip through omnifusion_amd/data.py) against the plain preprocess kernels followed by
torch.flip / torch.roll / channel indexing — the index map is exact, so every comparison but gamma's is bit for bit."""
import functools

import numpy as np
import pytest
import torch

from _augment_cases import BIG, GAMMA_GATE, GAMMAS, SHAPES, compose_numpy, compose_torch, frames, invert_torch, tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(dst, src) for dst, srcs in SHAPES + (BIG,) for src in srcs]


@functools.lru_cache(maxsize=None)
def _inputs(src):
    fr, dz = frames(1500 + src[0], 3, src)
    return fr, dz, torch.from_numpy(fr).to(DEV), torch.from_numpy(dz.view(np.int16)).to(DEV)


@functools.lru_cache(maxsize=None)
def _plain(dst, src):
    """the parent's own kernels on the same frames: rgb [3,3,H,W], depth, mask — computed once, never written to"""
    from omnifusion_amd.data import preprocess_depth, preprocess_rgb
    _, _, fr, dz = _inputs(src)
    return (preprocess_rgb(fr, dst),) + preprocess_depth(dz, dst)


def _aug(items, gamma=None):
    from omnifusion_amd.data import Augmentation
    return Augmentation([f for f, _, _ in items], [dx for _, dx, _ in items], [list(p) for _, _, p in items], gamma)


def _no_gamma(a):
    from omnifusion_amd.data import DeviceAugmentation
    d = a.to(DEV)
    return DeviceAugmentation(d.table, None)


@pytest.mark.parametrize("dst,src", CASES, ids=lambda v: "x".join(map(str, v)))
def test_index_map_is_exact(dst, src):
    from omnifusion_amd.data import Augmentation, augment_depth, augment_rgb
    from oracle import io_ref
    fr_np, _, fr, dz = _inputs(src)
    rgb, depth, mask = _plain(dst, src)
    for items in tables(dst[1]):
        want = compose_torch(rgb, items)
        for a in (_aug(items).to(DEV), _no_gamma(_aug(items))):                # an exponent of 1, and no gamma table at all
            assert torch.equal(augment_rgb(fr, dst, a), want), items
        d, m = augment_depth(dz, dst, _aug(items))
        assert torch.equal(d, compose_torch(depth, items, color=False)) and torch.equal(m, compose_torch(mask, items, color=False)), items
        if src[0] % dst[0] == 0 and src[1] % dst[1] == 0:                       # the restatement allows 0 there
            ref = compose_numpy(io_ref.preprocess_rgb(fr_np, *dst), items)
            assert np.array_equal(augment_rgb(fr, dst, _aug(items)).cpu().numpy(), ref), items
    ident = Augmentation.identity(3)
    assert torch.equal(augment_rgb(fr, dst, ident), rgb)
    d, m = augment_depth(dz, dst, ident)
    assert torch.equal(d, depth) and torch.equal(m, mask)


@pytest.mark.parametrize("dst,src", CASES, ids=lambda v: "x".join(map(str, v)))
def test_gamma(dst, src):
    """against float64(v32) ** float64(g32) rounded to float32, |d| <= 2e-6 (derived: _augment_cases.GAMMA_GATE); 0 and 1 exact; an
    exponent of 1 bit-identical to no gamma; the table and the direct powf give the same bits; the planes kernel gives them too"""
    from omnifusion_amd import _lib
    from omnifusion_amd.data import augment, augment_rgb
    _, _, fr, _ = _inputs(src)
    worst = 0.0
    for items in tables(dst[1])[:3]:
        a = _aug(items, GAMMAS)
        v32 = augment_rgb(fr, dst, _no_gamma(a))
        got = augment_rgb(fr, dst, a)
        g64 = a.gamma.to(DEV).double().view(3, 1, 1, 1)
        want = (v32.double() ** g64).float()
        err = float((got.double() - want.double()).abs().max())
        worst = max(worst, err)
        print(f"gamma {dst} <- {src} {items}: max |d| = {err:.3e}")
        assert err <= GAMMA_GATE
        assert torch.equal(got[0], v32[0])                                      # GAMMAS[0] == 1
        assert bool((got[v32 == 0] == 0).all()) and bool((got[v32 == 1] == 1).all())
        assert bool((v32 == 0).any()) and bool((v32 == 1).any()) or src != dst
        _lib.set_option("augment_lut", 0)
        try:
            direct = augment_rgb(fr, dst, a)
        finally:
            _lib.set_option("augment_lut", 1)
        assert torch.equal(direct, got)
        # float32 planes with colour: the same map and powf on the already preprocessed batch
        assert torch.equal(augment(_plain(dst, src)[0], a, color=True), got)
        assert torch.equal(augment(_plain(dst, src)[0], _no_gamma(a), color=True), v32)
    print(f"gamma {dst} <- {src}: worst max |d| = {worst:.3e} (gate {GAMMA_GATE:.1e})")


def test_planes_and_their_inverse():
    from omnifusion_amd.data import augment
    g = torch.Generator().manual_seed(3)
    xs = [torch.rand((3, 3, 5, 10), generator=g).to(DEV),
          torch.randint(-2 ** 40, 2 ** 40, (3, 1, 6, 12), generator=g).to(DEV),
          torch.randint(0, 256, (3, 1, 5, 10), generator=g).to(torch.uint8).to(DEV),
          torch.randint(-2 ** 15, 2 ** 15, (3, 6, 12), generator=g).to(torch.int16).to(DEV),
          torch.rand((3, 2, 64, 128), generator=g).to(DEV)]
    for x in xs:
        for items in tables(x.shape[-1]):
            a = _aug(items).to(DEV)
            x4 = x if x.dim() == 4 else x[:, None]
            y = augment(x, a)
            assert y.shape == x.shape and y.dtype == x.dtype and torch.equal(y.reshape(x4.shape), compose_torch(x4, items, color=False)), items
            assert torch.equal(augment(y, a, inverse=True), x), items
            assert torch.equal(augment(x, a, inverse=True).reshape(x4.shape), invert_torch(x4, items)), items
            if x.shape[1] == 3 and x.dim() == 4:
                assert torch.equal(augment(x, a, color=True), compose_torch(x, items))
                assert torch.equal(augment(x, a, color=True, inverse=True), augment(x, a, inverse=True))    # no colour on the way back


def test_argument_errors():
    from omnifusion_amd.data import Augmentation, DeviceAugmentation, augment, augment_depth, augment_rgb
    a3 = Augmentation.identity(3)
    x = torch.zeros((3, 3, 5, 10), device=DEV)
    with pytest.raises(ValueError, match="three channels"):
        augment(torch.zeros((3, 2, 5, 10), device=DEV), a3, color=True)
    with pytest.raises(ValueError, match="gamma needs a float32"):
        augment(torch.zeros((3, 3, 5, 10), dtype=torch.int64, device=DEV), Augmentation([0] * 3, [0] * 3, [[0, 1, 2]] * 3, [0.5, 1, 1]), color=True)
    assert augment(torch.ones((3, 3, 5, 10), dtype=torch.int64, device=DEV), a3, color=True).sum().item() == 450    # all exponents 1: fine
    with pytest.raises(ValueError, match="src and dst must differ"):
        augment(x, a3, out=x)
    with pytest.raises(ValueError, match="hold 3 items"):
        augment(x, Augmentation.identity(2))
    fr = torch.zeros((3, 5, 10, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="hold 3 items"):
        augment_rgb(fr, (5, 10), Augmentation.identity(4))
    with pytest.raises(ValueError, match="uint8"):
        augment_rgb(fr.float(), (5, 10), a3)
    with pytest.raises(NotImplementedError, match="down-scale"):
        augment_rgb(fr, (6, 10), a3)
    with pytest.raises(ValueError, match="16-bit"):
        augment_depth(fr[..., 0], (5, 10), a3)
    with pytest.raises(ValueError, match="int32"):
        DeviceAugmentation(torch.zeros((3, 5), dtype=torch.int64, device=DEV))


def test_capture_and_replay_follow_the_table():
    """captured once; the table tensors are rewritten in place between replays: the outputs follow, bit-equal to eager calls"""
    from omnifusion_amd.data import augment_depth, augment_rgb
    dst, src = (6, 12), (13, 27)
    _, _, fr, dz = _inputs(src)
    tabs = tables(dst[1])
    a = _aug(tabs[0], GAMMAS).to(DEV)
    rgb = torch.empty((3, 3) + dst, device=DEV)
    depth, mask = torch.empty((3, 1) + dst, device=DEV), torch.empty((3, 1) + dst, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up outside the capture
        augment_rgb(fr, dst, a, out=rgb)
        augment_depth(dz, dst, a, out=(depth, mask))
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment_rgb(fr, dst, a, out=rgb)
        augment_depth(dz, dst, a, out=(depth, mask))
    for items, gam in ((tabs[1], GAMMAS[::-1]), (tabs[3], (1.0, 1.0, 0.7)), (tabs[0], GAMMAS)):
        new = _aug(items, gam)
        table, gamma = new.pack()
        a.table.copy_(table.to(DEV))
        a.gamma.copy_(gamma.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        d, m = augment_depth(dz, dst, new)
        assert torch.equal(rgb, augment_rgb(fr, dst, new)) and torch.equal(depth, d) and torch.equal(mask, m), items


def test_train_feeder_delivers_every_batch_in_order():
    from omnifusion_amd.data import TrainBatch, TrainFeeder, augment_depth, augment_rgb, draw_augmentation
    rng = np.random.default_rng(21)
    lens = [2] * 6 + [1]
    batches = [(rng.integers(0, 256, (n, 64, 128, 3), dtype=np.uint8), rng.integers(0, 6000, (n, 64, 128), dtype=np.uint16)) for n in lens]
    flags = dict(flip=True, rotate=True, gamma=True, permute_color=True)
    feeder = TrainFeeder(batches, (32, 64), depth=3, generator=torch.Generator().manual_seed(31), np_random=np.random.RandomState(31), **flags)
    got = []
    for b in feeder:
        assert isinstance(b, TrainBatch) and b.rgb.is_cuda and b.rgb.shape[1:] == (3, 32, 64) and b.depth.shape == b.mask.shape
        used = (b.rgb * 2.0).sum()                                              # consume on the current stream (the buffers are reused: clone to keep)
        got.append((b.rgb.clone(), b.depth.clone(), b.mask.clone(), b.aug.table.clone(), b.aug.gamma.clone(), b.aug.host, used))
    assert [g[0].shape[0] for g in got] == lens
    gen, rs = torch.Generator().manual_seed(31), np.random.RandomState(31)
    for (rgb, depth, mask, table, gamma, host, _), (fr, dz) in zip(got, batches):
        want = draw_augmentation(fr.shape[0], 64, generator=gen, np_random=rs, **flags)
        wt, wg = want.pack()
        assert torch.equal(table.cpu(), wt) and torch.equal(gamma.cpu(), wg)
        assert torch.equal(host.pack()[0], wt) and torch.equal(host.pack()[1], wg)
        fr_d, dz_d = torch.from_numpy(fr).to(DEV), torch.from_numpy(dz.view(np.int16)).to(DEV)
        assert torch.equal(rgb, augment_rgb(fr_d, (32, 64), host))
        d, m = augment_depth(dz_d, (32, 64), host)
        assert torch.equal(depth, d) and torch.equal(mask, m)
    assert any(bool((g[3][:, 0] != 0).any()) for g in got) and any(bool((g[3][:, 1] != 0).any()) for g in got)    # something was drawn
