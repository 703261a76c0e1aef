"""Seeded inputs of the Chamfer fixtures G21a-e, a torch restatement of the one-directional Chamfer term written from its formula (DESIGN.md
§16; parametrised by dtype: float64 is the yardstick of the GPU tests) and — where the reference checkout is present — the reference's own
chamfer_distance_with_batch (tools/gen_golden_chamfer.py writes its results; tests/test_chamfer_*.py regenerate the same inputs and compare).
Only results and float64 input checksums are stored in tests/golden/.

    dist[b,i] = min over the valid j of |p1[b,i] - p2[b,j]|_2,  idx[b,i] = the argmin,  loss = sum over b and the valid i of dist[b,i]
"""
import numpy as np
import torch

from _geometry_cases import directional_residual, rel_error  # noqa: F401  (the same error measures)
from _util import rng_uniform

NAMES = ("G21a", "G21b", "G21c", "G21d", "G21e")
SHAPES = {"G21a": (2, 300, 517, 3), "G21b": (1, 1, 1, 3), "G21c": (3, 1000, 70, 3), "G21d": (2, 65, 4099, 3), "G21e": (2, 700, 900, 2)}
SEEDS = {"G21a": 2101, "G21b": 2111, "G21c": 2121, "G21d": 2131, "G21e": 2141}
MIN_GAP = 1e-5                                        # between a query's nearest and second-nearest valid target, float64
DIRECTION_H = 3e-3                                    # the step of the directional-derivative check (as tests/_geometry_cases.py)
DUPLICATES_PER_ITEM = 8                               # G21e: 16 points of p1 are exact copies of valid points of p2


def case(name):
    """-> dict(p1 [B,N,D], p2 [B,M,D]: float32, uniform in [-3, 3]; mask1 [B,N], mask2 [B,M]: bool or None; dup: [(b, i, j)]).  G21e: both masks
    at about 80 %, and per item 8 valid points of p1 are overwritten with 8 distinct valid points of p2 (distance 0, gradient 0)."""
    B, N, M, D = SHAPES[name]
    s = SEEDS[name]
    p1 = (6.0 * rng_uniform(s, (B, N, D)).astype(np.float64) - 3.0).astype(np.float32)
    p2 = (6.0 * rng_uniform(s + 1, (B, M, D)).astype(np.float64) - 3.0).astype(np.float32)
    mask1 = mask2 = None
    dup = []
    if name == "G21e":
        mask1, mask2 = rng_uniform(s + 2, (B, N)) < 0.8, rng_uniform(s + 3, (B, M)) < 0.8
        g = np.random.default_rng(s + 4)
        for b in range(B):
            ii = g.choice(np.flatnonzero(mask1[b]), DUPLICATES_PER_ITEM, replace=False)
            jj = g.choice(np.flatnonzero(mask2[b]), DUPLICATES_PER_ITEM, replace=False)
            for i, j in zip(ii, jj):
                p1[b, i] = p2[b, j]
                dup.append((b, int(i), int(j)))
    return dict(p1=p1, p2=p2, mask1=mask1, mask2=mask2, dup=dup)


def direction(name):
    """-> (v1 like p1, v2 like p2): float64 — the direction of the directional-derivative check: the float64 gradient itself, every point's
    vector scaled by a seeded factor in [0.5, 1.5].  (Along a random direction the terms of <grad, v> cancel to a few per cent of their
    size, and the queries whose nearest neighbour changes within the step — a kink of the loss — then dominate the residual.)"""
    B, N, M, D = SHAPES[name]
    s = SEEDS[name]
    r = run_restatement(case(name), torch.float64)
    return r["grad_p1"] * (0.5 + rng_uniform(s + 7, (B, N, 1)).astype(np.float64)), r["grad_p2"] * (0.5 + rng_uniform(s + 8, (B, M, 1)).astype(np.float64))


def checksums(c):
    return {k: np.float64(np.asarray(v, np.float64).sum()) for k, v in c.items() if isinstance(v, np.ndarray)}


def _valid(mask, b, n):
    return np.arange(n) if mask is None else np.flatnonzero(mask[b])


# ------------------------------------------------------------------ the restatement
def pair_distances(a, t):
    """[n,D], [m,D] -> [n,m]: the 2-norm of the direct differences (the reference's torch.norm(p1 - p2, 2, dim=3))."""
    return torch.linalg.vector_norm(a.unsqueeze(1) - t.unsqueeze(0), ord=2, dim=2)


def run_restatement(c, dtype, device="cpu", p1=None, p2=None):
    """-> dict(loss float; dist [B,N], idx [B,N] (-1 at masked queries), grad_p1, grad_p2 arrays).  Item by item over the valid points; the
    gradient is torch autograd's: 0 where the distance is 0."""
    P1 = torch.from_numpy(np.ascontiguousarray(c["p1"] if p1 is None else p1)).to(device=device, dtype=dtype).requires_grad_(True)
    P2 = torch.from_numpy(np.ascontiguousarray(c["p2"] if p2 is None else p2)).to(device=device, dtype=dtype).requires_grad_(True)
    B, N, _ = P1.shape
    M = P2.shape[1]
    dist, idx = np.zeros((B, N), np.float64), np.full((B, N), -1, np.int32)
    loss = 0.0
    for b in range(B):
        vi, vj = _valid(c["mask1"], b, N), _valid(c["mask2"], b, M)
        d, arg = pair_distances(P1[b, torch.from_numpy(vi).to(device)], P2[b, torch.from_numpy(vj).to(device)]).min(dim=1)
        loss = loss + d.sum()
        dist[b, vi] = d.detach().double().cpu().numpy()
        idx[b, vi] = vj[arg.cpu().numpy()]
    g1, g2 = torch.autograd.grad(loss, (P1, P2))
    return dict(loss=float(loss.detach()), dist=dist, idx=idx, grad_p1=g1.cpu().numpy(), grad_p2=g2.cpu().numpy())


def restatement_loss(c, dtype, p1, p2):
    return run_restatement(c, dtype, p1=p1, p2=p2)["loss"]


def gaps(c):
    """-> (the least gap between the nearest and the second-nearest valid target over the valid queries, float64; inf where an item has one
    valid target)."""
    B, N, _ = c["p1"].shape
    M = c["p2"].shape[1]
    least = float("inf")
    for b in range(B):
        vi, vj = _valid(c["mask1"], b, N), _valid(c["mask2"], b, M)
        if len(vj) < 2 or len(vi) == 0:
            continue
        d = pair_distances(torch.from_numpy(c["p1"][b, vi]).double(), torch.from_numpy(c["p2"][b, vj]).double())
        two = torch.topk(d, 2, dim=1, largest=False).values
        least = min(least, float((two[:, 1] - two[:, 0]).min()))
    return least


# ------------------------------------------------------------------ the reference's own function
def reference_function():
    """chamfer_distance_with_batch of the reference's util.py.  The module imports the whole model zoo at module level, so the function is
    exec'd alone — here only, never stored (needs the reference checkout; used by the generator and by the CPU test only)."""
    import os
    from oracle import ref_loader
    src = open(os.path.join(ref_loader.REFERENCE_ROOT, "util.py")).read()
    ns = {"torch": torch}
    exec(compile(src[src.index("def chamfer_distance_with_batch"):src.index("def map_coordinates")], "util_chamfer", "exec"), ns)
    return ns["chamfer_distance_with_batch"]


def run_reference(c, dtype, p1=None, p2=None):
    """-> dict(loss, grad_p1, grad_p2) from the reference's function and its autograd on the CPU: one call for the whole batch, or — with
    masks — one call per item on its valid points."""
    fn = reference_function()
    P1 = torch.from_numpy(np.ascontiguousarray(c["p1"] if p1 is None else p1)).to(dtype).requires_grad_(True)
    P2 = torch.from_numpy(np.ascontiguousarray(c["p2"] if p2 is None else p2)).to(dtype).requires_grad_(True)
    B, N, _ = P1.shape
    M = P2.shape[1]
    if c["mask1"] is None and c["mask2"] is None:
        loss = fn(P1, P2)
    else:
        loss = 0.0
        for b in range(B):
            vi, vj = torch.from_numpy(_valid(c["mask1"], b, N)), torch.from_numpy(_valid(c["mask2"], b, M))
            loss = loss + fn(P1[b, vi].unsqueeze(0), P2[b, vj].unsqueeze(0))
    g1, g2 = torch.autograd.grad(loss, (P1, P2))
    return dict(loss=float(loss.detach()), grad_p1=g1.numpy(), grad_p2=g2.numpy())
