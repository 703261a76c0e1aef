"""CPU: the host half of the training input path (omnifusion_amd/data.py): `draw_augmentation` makes the reference loaders' own draws,
`Augmentation` validates what it is given, and nothing here runs without a GPU."""
import numpy as np
import pytest
import torch

from _augment_cases import loader_sequence

FLAGS = ("flip", "rotate", "gamma", "permute_color")
CONFIGS = [{k: k == on for k in FLAGS} for on in FLAGS] + [{k: True for k in FLAGS}]


def _seed(s):
    torch.manual_seed(s)
    np.random.seed(s)


def _np_state():
    st = np.random.get_state()
    return st[0], st[1].tolist(), st[2], st[3], st[4]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "+".join(k for k in FLAGS if c[k]))
def test_draws_are_the_loaders_draws(cfg):
    """B = 5, W = 64, the same seeds: equal flip, dx, perm, bit-equal gamma — and the SAME generator states afterwards (a disabled stage
    draws nothing, an enabled one draws exactly what the loader draws)."""
    from omnifusion_amd.data import draw_augmentation
    _seed(1234)
    fl, dx, perm, g = loader_sequence(5, 64, **cfg)
    t_state, n_state = torch.get_rng_state(), _np_state()
    _seed(1234)
    a = draw_augmentation(5, 64, **cfg)
    assert a.flip.tolist() == fl and a.dx.tolist() == dx and a.perm.tolist() == perm
    assert a.gamma.dtype == torch.float32 and a.gamma.numpy().tobytes() == g.tobytes()
    assert torch.equal(torch.get_rng_state(), t_state) and _np_state() == n_state
    # an explicit generator / RandomState gives the same parameters and leaves the global ones alone
    _seed(99)
    t0, n0 = torch.get_rng_state(), _np_state()
    b = draw_augmentation(5, 64, generator=torch.Generator().manual_seed(1234), np_random=np.random.RandomState(1234), **cfg)
    assert b.flip.tolist() == fl and b.dx.tolist() == dx and b.perm.tolist() == perm and b.gamma.numpy().tobytes() == g.tobytes()
    assert torch.equal(torch.get_rng_state(), t0) and _np_state() == n0


def test_ranges_over_200_draws():
    from omnifusion_amd.data import draw_augmentation
    a = draw_augmentation(200, 64, flip=True, rotate=True, gamma=True, permute_color=True, generator=torch.Generator().manual_seed(7),
                          np_random=np.random.RandomState(7))
    assert len(a) == 200 and set(a.dx.tolist()) == {0, 16, 32, 48} and set(a.flip.tolist()) == {0, 1}
    g = a.gamma.numpy()
    assert ((g == 1) | ((g > 0.5) & (g <= 1))).all() and (g == 1).any() and (g < 1).any()      # the quirk: coin 1 leaves the image alone
    assert all(sorted(r) == [0, 1, 2] for r in a.perm.tolist()) and any(r != [0, 1, 2] for r in a.perm.tolist())
    # nothing enabled: the identity, and no draw at all
    _seed(5)
    t0, n0 = torch.get_rng_state(), _np_state()
    e = draw_augmentation(4, 64)
    assert torch.equal(torch.get_rng_state(), t0) and _np_state() == n0
    assert e.flip.tolist() == [0] * 4 and e.dx.tolist() == [0] * 4 and e.perm.tolist() == [[0, 1, 2]] * 4 and e.gamma.tolist() == [1.0] * 4
    with pytest.raises(ValueError, match="width >= 4"):
        draw_augmentation(1, 3, rotate=True)
    assert draw_augmentation(1, 3, flip=True, generator=torch.Generator().manual_seed(0)).dx.tolist() == [0]


def test_augmentation_validates_and_packs():
    from omnifusion_amd.data import Augmentation
    a = Augmentation([1, 0], [5, -2], [[2, 0, 1], [0, 1, 2]], [0.5, 1.0])
    table, gamma = a.pack()
    assert table.dtype == torch.int32 and table.tolist() == [[1, 5, 2, 0, 1], [0, -2, 0, 1, 2]]
    assert gamma.dtype == torch.float32 and gamma.tolist() == [0.5, 1.0]
    i = Augmentation.identity(3)
    assert len(i) == 3 and i.pack()[0].tolist() == [[0, 0, 0, 1, 2]] * 3 and i.pack()[1].tolist() == [1.0] * 3
    with pytest.raises(ValueError, match="permutation"):
        Augmentation([0], [0], [[0, 0, 1]])
    with pytest.raises(ValueError, match="permutation"):
        Augmentation([0], [0], [[0, 1, 3]])
    with pytest.raises(ValueError, match="gamma"):
        Augmentation([0], [0], [[0, 1, 2]], [0.0])
    with pytest.raises(ValueError, match="gamma"):
        Augmentation([0], [0], [[0, 1, 2]], [-1.0])
    with pytest.raises(ValueError, match="integers"):
        Augmentation([0], [1.5], [[0, 1, 2]])
    with pytest.raises(ValueError, match="one length"):
        Augmentation([0, 1], [0], [[0, 1, 2]])
    with pytest.raises(ValueError, match="one length"):
        Augmentation([0], [0], [[0, 1, 2]], [1.0, 1.0])
    with pytest.raises(ValueError, match="host tensor"):                      # parameters are drawn and checked on the host
        Augmentation(torch.zeros(1, dtype=torch.int64, device="meta"), [0], [[0, 1, 2]])


def test_no_cpu_path():
    """The package still fails loudly without a GPU: a host tensor is refused, never augmented by something else."""
    from omnifusion_amd.data import Augmentation, augment, augment_depth, augment_rgb
    a = Augmentation.identity(1)
    with pytest.raises(ValueError, match="no CPU path"):
        augment_rgb(torch.zeros(1, 4, 8, 3, dtype=torch.uint8), (4, 8), a)
    with pytest.raises(ValueError, match="no CPU path"):
        augment_depth(torch.zeros(1, 4, 8, dtype=torch.int16), (4, 8), a)
    with pytest.raises(ValueError, match="no CPU path"):
        augment(torch.zeros(1, 3, 4, 8), a)
