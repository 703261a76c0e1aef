"""Seeded inputs of the DIBR fixtures G14a-e (tools/gen_golden_dibr.py writes the reference's outputs for them; tests/test_dibr_*.py
regenerate the same inputs and compare).  Only outputs and float64 input checksums are stored in tests/golden/."""
import numpy as np

from _util import rng_uniform, smooth_erp

BASELINE = 0.26


def image_grid(H, W):
    u = np.broadcast_to(np.arange(W, dtype=np.float32)[None, :], (H, W))
    v = np.broadcast_to(np.arange(H, dtype=np.float32)[:, None], (H, W))
    return np.stack([u, v])[None].astype(np.float32)                        # [1,2,H,W], as spherical.create_image_grid


def zero_block(depth):
    """Exact zeros (a ReLU'd prediction, a hole of the ground truth) in a block that crosses row H/2 and column 3W/4 (quirk d2)."""
    H, W = depth.shape[-2:]
    depth[..., H // 2 - 6:H // 2 + 7, 3 * W // 4 - 5:3 * W // 4 + 6] = 0.0
    return depth


def smooth_depth(seed, B, H, W):
    return (0.3 + 7.7 * smooth_erp(seed, B, 1, H, W)).astype(np.float32)


def case(name):
    """-> dict(kind = 'render' | 'vertical' | 'horizontal', img, depth, coords (render) , baseline, max_depth)."""
    if name == "G14a":
        B, C, H, W = 2, 3, 64, 128
        img = smooth_erp(1401, B, C, H, W)
        depth = smooth_depth(1402, B, H, W)
        disp = (smooth_erp(1403, B, 2, H, W) - 0.5) * np.array([56.0, 28.0], np.float32)[None, :, None, None]
        coords = (image_grid(H, W) + disp).astype(np.float32)              # goes negative and beyond W / H at the borders
        return dict(kind="render", img=img, depth=depth, coords=coords, max_depth=20.0)
    if name == "G14b":
        B, C, H, W = 2, 3, 128, 256
        return dict(kind="vertical", img=smooth_erp(1411, B, C, H, W), depth=zero_block(smooth_depth(1412, B, H, W)), baseline=BASELINE)
    if name == "G14c":
        B, C, H, W = 1, 1, 256, 512
        return dict(kind="horizontal", img=smooth_erp(1421, B, C, H, W), depth=zero_block(smooth_depth(1422, B, H, W)), baseline=BASELINE)
    if name == "G14d":
        B, C, H, W = 2, 3, 128, 256
        return dict(kind="horizontal", img=smooth_erp(1431, B, C, H, W), depth=zero_block(smooth_depth(1432, B, H, W)), baseline=BASELINE)
    if name == "G14e":
        B, C, H, W = 2, 3, 128, 256
        depth = (0.3 + 7.7 * rng_uniform(1442, (B, 1, H, W))).astype(np.float32)
        return dict(kind="vertical", img=rng_uniform(1441, (B, C, H, W)), depth=zero_block(depth), baseline=BASELINE)
    raise KeyError(name)


NAMES = ("G14a", "G14b", "G14c", "G14d", "G14e")


def checksums(c):
    return {k: np.float64(np.asarray(v, np.float64).sum()) for k, v in c.items() if isinstance(v, np.ndarray)}


def run_reference(c):
    """The reference's own render / dibr_* on the CPU (needs /root/reference; test infrastructure only).  -> (recon, mask or None)."""
    import os
    import sys
    import torch
    from oracle import ref_loader
    root = ref_loader.REFERENCE_ROOT
    if root not in sys.path:
        sys.path.insert(0, root)
    import spherical as S360                                                 # the reference's packages (pure torch)
    import supervision as L
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    with torch.no_grad():
        if c["kind"] == "render":
            recon, mask = L.splatting.render(t(c["img"]), t(c["depth"]), t(c["coords"]), max_depth=c["max_depth"])
            return recon.numpy(), mask.numpy()
        # util.py imports the whole model zoo (and sklearn / matplotlib) at module level: its two DIBR functions are exec'd alone
        src = open(os.path.join(root, "util.py")).read()
        start, end = src.index("def dibr_vertical"), src.index("def get_sobel_kernel")
        ns = {"torch": torch, "S360": S360, "L": L}
        exec(compile(src[start:end], "util_dibr", "exec"), ns)               # executed here only, never stored
        B, C, H, W = c["img"].shape
        uvgrid = S360.create_image_grid(W, H)
        sgrid = S360.create_spherical_grid(W)
        fn = ns["dibr_vertical" if c["kind"] == "vertical" else "dibr_horizontal"]
        return fn(t(c["depth"]), t(c["img"]), uvgrid, sgrid, c["baseline"]).numpy(), None
