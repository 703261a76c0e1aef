"""GPU, one process: the four library calls of the synchronised batch normalisation (csrc/omni_batchnorm.hip omni_syncbn_*)
on the shards of one batch — W ranks simulated in one process, the records stacked by the test where dist.all_gather_records would gather
them — against float64 torch autograd on the CONCATENATED batch (tests/_syncbn_ref.py: the reference, the cases and the gate of
test_batchnorm_gpu.py, err <= 8 . max(e32, 5e-7) per tensor kind, derived from the reference side alone).  Every buffer a call writes is
filled with NaN first.  Every measured error is printed; the largest per kind: DESIGN.md §28."""
import pytest
import torch

import _syncbn_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ACT = {"none": 0, "relu": 1}


def nhwc(t):
    return None if t is None else t.to(DEV).permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous().cpu()


def nans(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def call(fn, what, *args):
    from omnifusion_amd import _lib
    _lib.check(fn(*args), what)


def workspace(rows, C):
    from omnifusion_amd import _lib
    n = _lib.load().omni_batchnorm_workspace_bytes(rows, C)
    assert n > 0
    return nans(n // 4), n


def run_split(name, cfg=sr.TRAIN, d=None, g=None, split=None):
    """The four calls on every shard -> the concatenated y, dx, dres, the SUM of the shards' dgamma / dbeta (in double), and per shard the
    saved pair and the running buffers, on the CPU"""
    from omnifusion_amd import _lib
    L, P = _lib.load(), _lib.ptr
    _, momentum, eps, affine = cfg
    M, H, W, C, act, has_res, case_split = sr.CASES[name]
    d = d or sr.reference(name, cfg)[0]
    g = d["g"] if g is None else g
    cuts, lo = [], 0
    for m in (case_split if split is None else split):
        cuts.append((lo, lo + m))
        lo += m
    assert lo == M
    world, relu = len(cuts), act == "relu"
    w, b = (d["w"].to(DEV), d["b"].to(DEV)) if affine else (None, None)
    stream = _lib.stream_of(torch.empty(1, device=DEV))
    sh = []
    for a, e in cuts:
        x = nhwc(d["x"][a:e])
        sh.append({"x": x, "res": nhwc(d["res"][a:e]) if has_res else None, "g": nhwc(g[a:e]), "rows": x.shape[0] * H * W, "m": e - a})
    # forward: stats -> (gather) -> apply
    for s in sh:
        s["rec"] = nans(2 * C + 1, dtype=torch.float64)
        ws, nb = workspace(s["rows"], C)
        call(L.omni_syncbn_stats_f32, "stats", P(s["x"]), P(s["rec"]), s["rows"], C, P(ws), nb, stream)
    table = torch.stack([s["rec"] for s in sh]).contiguous()
    for s in sh:
        s["y"], s["saved"], s["rm"], s["rv"] = nans(s["m"], H, W, C), nans(2, C), d["rm"].to(DEV), d["rv"].to(DEV)
        call(L.omni_syncbn_fwd_apply_f32, "fwd_apply", P(s["x"]), P(s["res"]), P(w), P(b), P(table), world, P(s["rm"]), P(s["rv"]), P(s["y"]),
             P(s["saved"]), s["rows"], C, momentum, eps, ACT[act], stream)
    # backward: reduce -> (gather) -> apply.  dZ is written by the reduce pass where the residual wants it
    for s in sh:
        s["rec2"] = nans(2 * C + 1, dtype=torch.float64)
        s["dres"] = nans(s["m"], H, W, C) if relu and has_res else None
        s["dgamma"], s["dbeta"] = (nans(C), nans(C)) if affine else (None, None)
        ws, nb = workspace(s["rows"], C)
        call(L.omni_syncbn_bwd_reduce_f32, "bwd_reduce", P(s["g"]), P(s["x"]), P(s["y"]), P(s["saved"]), P(s["dres"]), P(s["rec2"]), P(s["dgamma"]),
             P(s["dbeta"]), s["rows"], C, ACT[act], P(ws), nb, stream)
    table2 = torch.stack([s["rec2"] for s in sh]).contiguous()
    for s in sh:
        s["dx"] = nans(s["m"], H, W, C)
        first, y = (s["dres"], None) if s["dres"] is not None else (s["g"], s["y"])
        call(L.omni_syncbn_bwd_apply_f32, "bwd_apply", P(first), P(y), P(s["x"]), P(w), P(s["saved"]), P(table2), world, P(s["dx"]), None,
             s["rows"], C, ACT[act], stream)
    torch.cuda.synchronize()
    cat = lambda k: nchw(torch.cat([s[k] for s in sh]))
    out = {"y": cat("y"), "x": cat("dx"), "res": (cat("dres") if relu else g.clone()) if has_res else None,
           "w": sum(s["dgamma"].double() for s in sh).cpu() if affine else None, "b": sum(s["dbeta"].double() for s in sh).cpu() if affine else None,
           "rm": sh[0]["rm"].cpu(), "rv": sh[0]["rv"].cpu()}
    out["per_shard"] = [{k: s[k].cpu() for k in ("saved", "rm", "rv")} for s in sh]
    out["tables"] = (table.cpu(), table2.cpu())
    return out


def check_gate(name, cfg, got, what=""):
    _, want, gate = sr.reference(name, cfg)
    for k in sr.OUTS:
        assert (got[k] is None) == (want[k] is None), (name, k)
        if want[k] is None:
            continue
        assert got[k].shape == want[k].shape and not torch.isnan(got[k]).any(), f"{name}{what}: NaN (an unwritten element) in {k}"
        e = sr.nerr(got[k], want[k])
        print(f"syncbn {name}{what} {'' if k in ('y', 'rm', 'rv') else 'd'}{k}: normalised error {e:.3e}  gate {gate[k]:.3e} (e32 {gate[k] / sr.FACTOR:.3e})")
        assert e <= gate[k], f"{name}{what}: {k}: {e:.3e} > {gate[k]:.3e}"


def shards_agree(got):
    first = got["per_shard"][0]
    return all(torch.equal(s[k], first[k]) for s in got["per_shard"] for k in ("saved", "rm", "rv"))


@pytest.mark.parametrize("name", list(sr.CASES))
def test_split_batch_vs_float64_on_the_concatenation(name):
    d, want, _ = sr.reference(name)
    got = run_split(name)
    check_gate(name, sr.TRAIN, got)
    assert shards_agree(got), f"{name}: saved or the running buffers differ between shards fed the same table"
    C = sr.CASES[name][3]
    assert got["tables"][0][:, 2 * C].tolist() == [float(m * sr.CASES[name][1] * sr.CASES[name][2]) for m in sr.CASES[name][6]]
    if sr.CASES[name][4] == "relu" and d["res"] is not None:
        assert torch.equal(got["res"], torch.where(want["z"] > 0, d["g"], torch.zeros_like(d["g"])))      # exact: a select
    again = run_split(name)
    assert all(got[k] is None or torch.equal(got[k], again[k]) for k in sr.OUTS), f"{name}: two runs differ"


@pytest.mark.parametrize("name", list(sr.CASES))
def test_world_one_has_the_bits_of_the_fused_calls(name):
    """the case's whole batch as ONE shard, fed its own record: bit for bit omni_batchnorm_fwd_f32 / _bwd_f32 on the same tensors"""
    from omnifusion_amd import _lib
    L, P = _lib.load(), _lib.ptr
    M, H, W, C, act, has_res, _ = sr.CASES[name]
    d = sr.reference(name)[0]
    got = run_split(name, split=(M,))
    relu = act == "relu"
    x, res, g, w, b = nhwc(d["x"]), nhwc(d["res"]), nhwc(d["g"]), d["w"].to(DEV), d["b"].to(DEV)
    rm, rv, rows = d["rm"].to(DEV), d["rv"].to(DEV), M * H * W
    y, saved, dx, dgamma, dbeta = nans(M, H, W, C), nans(2, C), nans(M, H, W, C), nans(C), nans(C)
    dres = nans(M, H, W, C) if relu and has_res else None
    stream = _lib.stream_of(x)
    ws, nb = workspace(rows, C)
    call(L.omni_batchnorm_fwd_f32, "fwd", P(x), P(res), P(w), P(b), P(rm), P(rv), P(y), P(saved), rows, C, 1, 0.1, 1e-5, ACT[act], P(ws), nb, stream)
    ws, nb = workspace(rows, C)
    call(L.omni_batchnorm_bwd_f32, "bwd", P(g), P(x), P(y), P(w), P(saved), P(dx), P(dres), P(dgamma), P(dbeta), rows, C, 1, ACT[act], P(ws), nb, stream)
    torch.cuda.synchronize()
    assert not torch.isnan(got["y"]).any() and not torch.isnan(got["x"]).any()
    assert torch.equal(got["y"], nchw(y)) and torch.equal(got["x"], nchw(dx))
    assert torch.equal(got["per_shard"][0]["saved"], saved.cpu())
    assert torch.equal(got["rm"], rm.cpu()) and torch.equal(got["rv"], rv.cpu())
    assert torch.equal(got["w"].float(), dgamma.cpu()) and torch.equal(got["b"].float(), dbeta.cpu())
    if dres is not None:
        assert torch.equal(got["res"], nchw(dres))


def test_a_nan_reaches_its_channel_on_every_shard_and_no_other():
    d, _, _ = sr.reference("plain")
    x = d["x"].clone()
    x[3, 3, 2, 2] = NAN                                                         # in the second shard
    got = run_split("plain", d=dict(d, x=x))
    ch3 = torch.zeros(32, dtype=torch.bool)
    ch3[3] = True
    for lo, hi in sr.bounds("plain"):
        for k in ("y", "x"):
            t = torch.isnan(got[k][lo:hi])
            assert torch.equal(t.flatten(2).all(2).all(0), ch3) and torch.equal(t.flatten(2).any(2).any(0), ch3), (k, lo)
    for s in got["per_shard"]:
        assert torch.equal(torch.isnan(s["saved"]).all(0), ch3) and torch.equal(torch.isnan(s["saved"]).any(0), ch3)
        assert torch.equal(torch.isnan(s["rm"]), ch3) and torch.equal(torch.isnan(s["rv"]), ch3)


def test_a_nan_behind_an_inactive_relu_changes_no_bit():
    d, want, _ = sr.reference("odd105")
    idx = (want["z"] < -0.1).nonzero()[0].tolist()
    g = d["g"].clone()
    g[tuple(idx)] = NAN
    a, b = run_split("odd105", g=g), run_split("odd105")
    assert all(torch.equal(a[k], b[k]) for k in sr.OUTS)
    assert torch.equal(a["tables"][1], b["tables"][1])


def test_world_outside_1_to_64_is_rejected():
    from omnifusion_amd import _lib
    L, P = _lib.load(), _lib.ptr
    x, y, saved, dx = nhwc(torch.randn(2, 32, 4, 4)), nans(2, 4, 4, 32), nans(2, 32), nans(2, 4, 4, 32)
    table = torch.zeros(1, 65, dtype=torch.float64, device=DEV)
    stream = _lib.stream_of(x)
    for world in (0, 65):
        with pytest.raises(ValueError, match="world must lie in"):
            call(L.omni_syncbn_fwd_apply_f32, "fwd_apply", P(x), None, None, None, P(table), world, None, None, P(y), P(saved), 32, 32, 0.1, 1e-5, 0,
                 stream)
        with pytest.raises(ValueError, match="world must lie in"):
            call(L.omni_syncbn_bwd_apply_f32, "bwd_apply", P(x), None, P(x), None, P(saved), P(table), world, P(dx), None, 32, 32, 0, stream)
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(saved).all() and torch.isnan(dx).all()      # nothing was launched


@pytest.mark.parametrize("cfg", [sr.REF101, sr.REF101_PLAIN], ids=["affine", "no_affine"])
def test_reference_transformer_settings(cfg):
    """momentum = 0.99, eps = 1e-6 (the reference's transformer BatchNorm2d), with and without weight and bias"""
    got = run_split("plain", cfg)
    check_gate("plain", cfg, got, f" [momentum 0.99, eps 1e-6, affine {cfg[3]}]")
    assert shards_agree(got)
    if not cfg[3]:
        assert got["w"] is None and got["b"] is None
