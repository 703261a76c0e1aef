"""The synchronised batch normalisation (csrc/omni_batchnorm.hip omni_syncbn_*, ops.sync_batch_norm) restated in float64, and
the cases its tests share (test_syncbn_cpu.py, test_syncbn_gpu.py, _syncbn_rank_probe.py).  No GPU is needed to import this.

The operator on W ranks is one batch normalisation over the CONCATENATED batch, so the reference is the one of test_batchnorm_gpu.py on the
concatenation: float64 torch on the CPU, F.relu(F.batch_norm(x_all, ..., training=True) + res_all) with autograd against the concatenated
grad_out.  The gate is that file's, derived from the reference side alone: e32 = the normalised error of torch's own float32 run of the same
expression, and the device must satisfy err <= 8 . max(e32, 5e-7) per tensor kind.  ReLU cases take their seed, from the float64
reference alone, so that no pre-activation lies within ZMARGIN = 1e-5 of 0; `reference` asserts it.

`phases` is the four library calls in float64: per-shard records (sum x, sum x^2, rows), rank-ordered totals, mean / var / invstd and the
running buffers, the apply; per-shard records (sum dZ, sum dZ.xhat, rows), totals, dx.  test_syncbn_cpu.py holds it against the reference."""
import functools

import torch

from test_batchnorm_gpu import CONV_GATE, FACTOR, FLOOR, OUTS, REF101, REF101_PLAIN, TRAIN, ZMARGIN, nerr, torch_cpu    # noqa: F401  (the gate)

#        M   H    W    C   act    res     the split of M over the ranks
CASES = {
    "plain":       (4, 8, 8, 32, "none", False, (2, 2)),
    "odd105":      (3, 5, 7, 32, "relu", True, (1, 2)),                         # a ragged split
    "c4":          (4, 3, 3, 4, "relu", False, (1, 1, 2)),                      # the narrowest channel count
    "c96":         (4, 4, 4, 96, "none", True, (2, 2)),                         # idle quads in a column group
    "rows18":      (18, 1, 1, 512, "none", False, (9, 9)),                      # two column groups
    "single_rows": (3, 1, 1, 32, "none", False, (1, 1, 1)),                     # every rank holds ONE row: illegal on one device, legal here
    "rows10240":   (40, 16, 16, 32, "relu", True, (5,) * 8),                    # world 8, many slabs
    "offset":      (4, 8, 8, 32, "none", False, (2, 2)),                        # means 0 .. 300, spreads 1 and 0.1: a record in fp32 returns variance 0
    "shifted":     (4, 8, 8, 32, "relu", False, (2, 2)),                        # shard r's x moved by 3 r: local statistics fail grossly
}
SEEDS = {"rows10240": 5}                                                        # case -> seed where 0 leaves a pre-activation within ZMARGIN of 0
DEFAULT_SEED = 0


def bounds(name):
    """[(lo, hi)] of the shards' items"""
    out, lo = [], 0
    for m in CASES[name][6]:
        out.append((lo, lo + m))
        lo += m
    assert lo == CASES[name][0], name
    return out


def inputs(name, cfg=TRAIN):
    """the GLOBAL batch: the generator order of test_batchnorm_gpu.inputs"""
    M, H, W, C, act, has_res, _ = CASES[name]
    gen = torch.Generator().manual_seed(SEEDS.get(name, DEFAULT_SEED))
    rn = lambda *shape: torch.randn(*shape, generator=gen)
    x = rn(M, C, H, W)
    if name == "offset":
        c = torch.arange(C)
        x = x * torch.where(c % 2 == 0, 1.0, 0.1).view(1, C, 1, 1) + (100.0 * (c % 4)).view(1, C, 1, 1)
    if name == "shifted":
        for r, (lo, hi) in enumerate(bounds(name)):
            x[lo:hi] += 3.0 * r
    return {"x": x, "w": 1 + 0.1 * rn(C), "b": 0.1 * rn(C), "res": rn(M, C, H, W) if has_res else None, "g": rn(M, C, H, W),
            "rm": 0.5 * rn(C), "rv": 0.5 + torch.rand(C, generator=gen)}


@functools.lru_cache(maxsize=None)
def reference(name, cfg=TRAIN):
    """(inputs, float64 results on the concatenated batch, {kind: the gate's right side}); computed once, never modified"""
    d = inputs(name, cfg)
    act = CASES[name][4]
    r64, r32 = torch_cpu(d, act, cfg, torch.float64), torch_cpu(d, act, cfg, torch.float32)
    if act == "relu":
        assert r64["z"].abs().min().item() >= ZMARGIN, f"{name} {cfg}: a float64 pre-activation within {ZMARGIN} of 0 (pick another seed)"
    gate = {k: FACTOR * max(nerr(r32[k], r64[k]), FLOOR) for k in OUTS if r64[k] is not None}
    return d, r64, gate


def rows_of(t):
    """[m,C,H,W] -> [m.H.W, C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def like(rows, t):
    m, C, H, W = t.shape
    return rows.reshape(m, H, W, C).permute(0, 3, 1, 2)


def record(a, b):
    """a rank's exchange record: (sum a[c], sum b[c], rows), 2 C + 1 doubles"""
    return torch.cat([a.sum(0), b.sum(0), torch.tensor([float(a.shape[0])], dtype=torch.float64)])


def totals(table):
    """[world, L] -> [L]: the records added in ascending rank order"""
    t = table[0].clone()
    for r in range(1, table.shape[0]):
        t = t + table[r]
    return t


def phases(xs, ress, gs, w, b, rm, rv, momentum, eps, act):
    """The four phases in float64 on the shards xs / ress / gs (lists; ress[r] may be None; w, b may be None) ->
    {y, x (dx), res (dres): lists per shard; w, b: lists of the ranks' LOCAL sums; rm, rv: the updated buffers; saved: (mean, invstd)}"""
    f64 = lambda t: None if t is None else t.double()
    xs, ress, gs = [rows_of(f64(x)) for x in xs], [None if r is None else rows_of(f64(r)) for r in ress], [rows_of(f64(g)) for g in gs]
    C = xs[0].shape[1]
    gamma = torch.ones(C, dtype=torch.float64) if w is None else f64(w)
    beta = torch.zeros(C, dtype=torch.float64) if b is None else f64(b)
    # forward: stats -> gather -> finish -> apply
    tot = totals(torch.stack([record(x, x * x) for x in xs]))
    n = tot[2 * C]
    mean = tot[:C] / n
    var = (tot[C:2 * C] / n - mean * mean).clamp(min=0.0)
    invstd = 1.0 / (var + eps).sqrt()
    rm_new = (1.0 - momentum) * f64(rm) + momentum * mean
    rv_new = (1.0 - momentum) * f64(rv) + momentum * (var * (n / (n - 1.0)))
    zs = [(x - mean) * (invstd * gamma) + beta + (0.0 if r is None else r) for x, r in zip(xs, ress)]
    ys = [z.clamp(min=0.0) if act == "relu" else z for z in zs]
    # backward: reduce -> gather -> apply
    dzs = [torch.where(y > 0, g, torch.zeros_like(g)) if act == "relu" else g for y, g in zip(ys, gs)]
    xhs = [(x - mean) * invstd for x in xs]
    recs = [record(dz, dz * xh) for dz, xh in zip(dzs, xhs)]
    tot = totals(torch.stack(recs))
    k1, k2 = tot[:C] / tot[2 * C], tot[C:2 * C] / tot[2 * C]
    dxs = [gamma * invstd * ((dz - k1) - xh * k2) for dz, xh in zip(dzs, xhs)]
    return {"y": ys, "x": dxs, "res": dzs, "b": [r[:C] for r in recs], "w": [r[C:2 * C] for r in recs], "rm": rm_new, "rv": rv_new,
            "saved": (mean, invstd)}


def restatement_bound(x):
    """The float64 rounding of `phases` against torch's two-pass float64: 2^-53 per operation, a few dozen operations and sums whose
    relative error stays far below sqrt(rows) . 2^-53 — covered by 1024 . 2^-53 — times the cancellation of var = E x^2 - mean^2, which loses
    mean^2 / var of the relative precision (the `offset` data: up to 300^2 / 0.1^2 = 9e6)."""
    xr = rows_of(x.double())
    cancel = (xr.mean(0).pow(2) / xr.var(0, unbiased=False)).max().item()
    return 1024.0 * 2.0 ** -53 * (1.0 + cancel)
