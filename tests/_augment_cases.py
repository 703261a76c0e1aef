"""Cases of the augmentation tests (tests/test_augment_cpu.py, tests/test_augment_gpu.py): the parameter tables, the loaders' draw
sequence written out by hand, and the composition in torch / numpy that the device kernels are compared with.

The contract (dataset_loader_stanford.py:57-73, dataset_loader_360d.py:54-71), per item, after resize and /255:
    flip     coin = torch.randint(2, (1,)); coin == 0: np.flip(axis=1)
    rotate   dx = torch.randint(W, (1,)); dx = dx // (W // 4) * (W // 4); np.roll(dx, axis=1)
    gamma    p = torch.rand((1,)) + 1 (float32); coin = torch.randint(2, (1,)); coin == 0: p = 1 / p, rgb = rgb ** p
    permute  coin = torch.randint(4, (1,)); coin == 0: idx = np.random.permutation(3), rgb = rgb[:, :, idx]
"""
import numpy as np
import torch

PERMS = ((0, 1, 2), (2, 0, 1), (1, 0, 2))
GAMMAS = (1.0, 0.5, 1.0 / 1.7)
GAMMA_GATE = 2e-6          # 2 x (16 ulp of pow on values <= 1 = 9.5e-7, OpenCL's bound, + 3e-8 of the reference's own rounding)

# (destination, sources): the same size, 2x (OpenCV's half-up 2x2 path), a fractional odd one
SHAPES = (((6, 12), ((6, 12), (12, 24), (13, 27))),        # W % 4 == 0: the quad path at the same size
          ((5, 10), ((5, 10), (10, 20), (11, 23))))        # W % 4 != 0: the per-pixel path
BIG = ((64, 128), ((64, 128), (128, 256)))                 # several blocks per item


def shifts(W):
    return (0, 1, 3, W // 4, W - 1, W + 5, -2)


def tables(W):
    """Lists of three (flip, dx, perm) items that together hold every dx of shifts(W) with flip 0 and 1, and every permutation."""
    combos = [(f, dx) for dx in shifts(W) for f in (0, 1)]
    out = []
    for k in range(0, len(combos), 3):
        items = [combos[(k + i) % len(combos)] for i in range(3)]
        out.append([(f, dx, PERMS[(i + k // 3) % 3]) for i, (f, dx) in enumerate(items)])
    return out


def frames(seed, B, hw):
    """(uint8 [B,Hs,Ws,3], uint16 [B,Hs,Ws]); the first pixels hold 0 and 255 so that gamma sees both ends"""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (B,) + tuple(hw) + (3,), dtype=np.uint8)
    fr[:, 0, 0, :] = 0
    fr[:, 0, 1, :] = 255
    dz = rng.integers(0, 6000, (B,) + tuple(hw), dtype=np.uint16)
    return fr, dz


def compose_torch(x, items, color=True):
    """x [B,C,H,W] (any dtype, any device) -> per item: flip, then roll, then channel indexing"""
    out = []
    for b, (f, dx, perm) in enumerate(items):
        t = x[b]
        if f:
            t = torch.flip(t, dims=[-1])
        t = torch.roll(t, int(dx), dims=-1)
        if color:
            t = t[list(perm)]
        out.append(t)
    return torch.stack(out)


def compose_numpy(x, items):
    """x [B,3,H,W] float32 numpy: np.flip / np.roll / channel indexing, as the loader does it on HWC"""
    out = []
    for b, (f, dx, perm) in enumerate(items):
        t = x[b].transpose(1, 2, 0)
        if f:
            t = np.flip(t, axis=1)
        t = np.roll(t, int(dx), axis=1)
        t = t[:, :, list(perm)]
        out.append(t.transpose(2, 0, 1))
    return np.stack(out)


def invert_torch(y, items):
    """the inverse of compose_torch(color=False): roll back, then flip back"""
    out = []
    for b, (f, dx, _) in enumerate(items):
        t = torch.roll(y[b], -int(dx), dims=-1)
        if f:
            t = torch.flip(t, dims=[-1])
        out.append(t)
    return torch.stack(out)


def loader_sequence(B, W, flip, rotate, gamma, permute_color):
    """The loaders' call sequence on torch's global generator and numpy's global state, written out by hand from the list above.
    -> flip [B], dx [B], perm [B][3], gamma [B] (numpy float32)"""
    fl, dxs, perms, gs = [], [], [], []
    for _ in range(B):
        f, d, idx, g = 0, 0, [0, 1, 2], np.float32(1)
        if flip:
            if torch.randint(2, size=(1,))[0].item() == 0:
                f = 1
        if rotate:
            d = torch.randint(W, size=(1,))[0].item()
            d = d // (W // 4) * (W // 4)
        if gamma:
            p = ((2 - 1) * torch.rand((1,)) + 1).numpy()[0]
            if torch.randint(2, size=(1,))[0].item() == 0:
                p = 1 / p
                g = p
        if permute_color:
            if torch.randint(4, size=(1,))[0].item() == 0:
                idx = [int(v) for v in np.random.permutation(3)]
        fl.append(f); dxs.append(d); perms.append(idx); gs.append(g)
    return fl, dxs, perms, np.asarray(gs, dtype=np.float32)
