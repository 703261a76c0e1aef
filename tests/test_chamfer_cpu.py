"""CPU: the boundary of the Chamfer term (supervision.chamfer, util.chamfer_distance_with_batch) — declared, exported and bound symbols, the
workspace query, argument checks that return before a device is touched, the Python errors — and the float64 restatement of
tests/_chamfer_cases.py against the committed fixtures G21a-e and against the reference itself where the checkout is present."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _chamfer_cases as cc
from _util import golden
from oracle import ref_loader

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="reference checkout not present")
NEW_SYMBOLS = ("omni_chamfer_workspace_bytes", "omni_chamfer_nn_f32", "omni_chamfer_grad_f32")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "omnifusion.h")


def test_names_and_reexports():
    import omnifusion_amd.supervision as S
    from omnifusion_amd import util
    from omnifusion_amd.supervision import chamfer
    assert S.chamfer is chamfer
    for name in ("nearest_neighbours", "chamfer_distance", "depth_chamfer"):
        assert getattr(S, name) is getattr(chamfer, name)
    assert callable(util.chamfer_distance_with_batch)


def test_symbols_declared_exported_and_bound():
    from omnifusion_amd import _lib
    header = open(HEADER).read()
    L = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.omni_chamfer_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.omni_chamfer_nn_f32.argtypes) == 13 and len(L.omni_chamfer_grad_f32.argtypes) == 14
    assert _lib.get_option("chamfer_split") == 1


def test_workspace_query():
    from omnifusion_amd import _lib
    L = _lib.load()
    for bad in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 1), (1, 8, 8, 4), (-1, 8, 8, 3), (65536, 8, 8, 3)):
        assert L.omni_chamfer_workspace_bytes(*bad) == 0, bad
    for B, N, M, D in cc.SHAPES.values():
        n = L.omni_chamfer_workspace_bytes(B, N, M, D)
        assert n >= 8 * B * M * D + 8 * B * ((N + 511) // 512) + 4 * B            # the fixed-point sums, the loss partials, the scale words
    # few queries, many targets: the candidates of every chunk (8 bytes per query and chunk) are part of it
    assert L.omni_chamfer_workspace_bytes(2, 65, 4099, 3) >= 8 * 2 * 4099 * 3 + 8 * 2 * 65 * 2
    # N x M has no limit: the size grows with N + M, not with the product
    assert L.omni_chamfer_workspace_bytes(8, 1 << 20, 1 << 20, 3) < (1 << 30)


def test_c_boundary_rejects_before_touching_a_device():
    """Null pointers, sizes < 1, D outside {2, 3}, no upstream gradient, no requested gradient: OMNI_ERR_INVALID.  The non-null pointers
    below are never dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV = _lib.OMNI_ERR_INVALID
    assert L.omni_chamfer_nn_f32(z, p, z, z, 1, 8, 8, 3, p, p, p, p, z) == INV and L.omni_chamfer_nn_f32(p, z, z, z, 1, 8, 8, 3, p, p, p, p, z) == INV
    for k in range(4):                                                          # dist, idx, loss, workspace
        out = [p, p, p, p]
        out[k] = z
        assert L.omni_chamfer_nn_f32(p, p, z, z, 1, 8, 8, 3, *out, z) == INV
    for shape in ((0, 8, 8, 3), (1, 0, 8, 3), (1, 8, 0, 3), (1, 8, 8, 4), (1, 8, 8, 1)):
        assert L.omni_chamfer_nn_f32(p, p, z, z, *shape, p, p, p, p, z) == INV, shape
        assert L.omni_chamfer_grad_f32(p, p, z, p, p, z, *shape, p, p, p, z) == INV, shape
    assert L.omni_chamfer_nn_f32(p, p, z, z, 1, 8, 8, 5, p, p, p, p, z) == INV and b"D must be 2 or 3" in L.omni_last_error()
    assert L.omni_chamfer_nn_f32(p, p, z, z, 1, 8, 8, 3, p, p, p, ctypes.c_void_p(4100), z) == INV and b"aligned" in L.omni_last_error()
    assert L.omni_chamfer_nn_f32(p, p, z, z, 65536, 8, 8, 3, p, p, p, p, z) == _lib.OMNI_ERR_UNSUPPORTED
    assert L.omni_chamfer_grad_f32(z, p, z, p, p, z, 1, 8, 8, 3, p, p, p, z) == INV and L.omni_chamfer_grad_f32(p, p, z, z, p, z, 1, 8, 8, 3, p, p, p, z) == INV
    assert L.omni_chamfer_grad_f32(p, p, z, p, z, z, 1, 8, 8, 3, p, p, p, z) == INV and b"upstream" in L.omni_last_error()
    assert L.omni_chamfer_grad_f32(p, p, z, p, p, z, 1, 8, 8, 3, z, z, p, z) == INV and b"requested" in L.omni_last_error()
    assert L.omni_chamfer_grad_f32(p, p, z, p, p, z, 1, 8, 8, 3, p, p, z, z) == INV and b"workspace" in L.omni_last_error()


def test_python_errors():
    from omnifusion_amd.supervision import chamfer_distance, depth_chamfer, nearest_neighbours
    from omnifusion_amd.util import chamfer_distance_with_batch
    a, b = torch.rand(2, 5, 3), torch.rand(2, 7, 3)
    for fn in (chamfer_distance, nearest_neighbours, chamfer_distance_with_batch):
        with pytest.raises(ValueError, match="no CPU path"):
            fn(a, b)
        with pytest.raises(ValueError, match="must be a tensor"):
            fn(a.numpy(), b)
    with pytest.raises(ValueError, match="reduction"):
        chamfer_distance(a, b, reduction="max")
    d = torch.rand(1, 1, 8, 16)
    with pytest.raises(ValueError, match="no CPU path"):
        depth_chamfer(d, d, d > 0.5)
    with pytest.raises(ValueError, match="must be a tensor"):
        depth_chamfer(d, None, d)


def test_python_shape_and_dtype_errors():
    """The checks of rank, dtype, D, batch and mask shapes (supervision.chamfer._cloud / _mask / _run) on tensors that claim to be on the
    device: they are raised before anything is launched."""
    from omnifusion_amd.supervision import chamfer

    class OnDevice(torch.Tensor):                                              # a CPU tensor that answers is_cuda = True: the checks read nothing else
        @property
        def is_cuda(self):
            return True

    dev = lambda t: t.as_subclass(OnDevice)
    with pytest.raises(ValueError, match=r"non-empty \[B,N,D\]"):
        chamfer._cloud(dev(torch.rand(5, 3)), "p1")
    with pytest.raises(ValueError, match=r"non-empty \[B,N,D\]"):
        chamfer._cloud(dev(torch.rand(2, 0, 3)), "p1")
    with pytest.raises(ValueError, match="float32"):
        chamfer._cloud(dev(torch.rand(2, 5, 3).double()), "p1")
    with pytest.raises(ValueError, match="2-D or 3-D"):
        chamfer._cloud(dev(torch.rand(2, 5, 4)), "p1")
    for bad in (torch.rand(3, 7, 3), torch.rand(2, 7, 2)):
        with pytest.raises(ValueError, match="agree in B and D"):
            chamfer._run(dev(torch.rand(2, 5, 3)), dev(bad), None, None)
    with pytest.raises(ValueError, match=r"mask1 must be \[B,N\]"):
        chamfer._mask(torch.ones(2, 6), "mask1", torch.rand(2, 5, 3), "p1")
    with pytest.raises(ValueError, match="must not require grad"):
        chamfer._mask(torch.ones(2, 5, requires_grad=True), "mask1", torch.rand(2, 5, 3), "p1")
    m = chamfer._mask(torch.tensor([[0.0, 2.0, -1.0]]), "mask1", torch.rand(1, 3, 3), "p1")
    assert m.dtype == torch.uint8 and m.tolist() == [[0, 1, 1]]                 # valid means non-zero
    with pytest.raises(ValueError, match="same shape"):
        chamfer.depth_chamfer(dev(torch.rand(1, 1, 8, 16)), dev(torch.rand(1, 1, 8, 16)), dev(torch.ones(1, 1, 8, 8)))
    with pytest.raises(ValueError, match="stride"):
        chamfer.depth_chamfer(dev(torch.rand(1, 1, 8, 16)), dev(torch.rand(1, 1, 8, 16)), dev(torch.ones(1, 1, 8, 16)), stride=0)


@pytest.mark.parametrize("name", cc.NAMES)
def test_restatement_reproduces_golden(name):
    """The regenerated inputs are the fixture's, the float64 restatement gives its results, and the 1e-5 gap between a query's two nearest
    targets — what makes the exact index comparison of the GPU test legitimate — holds."""
    c, g = cc.case(name), golden(name + "_chamfer")
    assert tuple(c["p1"].shape[:2]) + tuple(c["p2"].shape[1:]) == cc.SHAPES[name]
    assert np.abs(c["p1"]).max() <= 3.0 and np.abs(c["p2"]).max() <= 3.0
    for k, v in cc.checksums(c).items():
        assert float(g["sum_" + k]) == float(v), f"{name}: the seeded input {k} is not the one the fixture was made from"
    r = cc.run_restatement(c, torch.float64)
    assert abs(r["loss"] - float(g["loss"])) <= 1e-12 * max(1.0, abs(float(g["loss"])))
    assert np.array_equal(r["idx"], g["idx"]) and g["idx"].dtype == np.int32
    for k in ("dist", "grad_p1", "grad_p2"):
        assert r[k].shape == g[k].shape and np.abs(r[k] - g[k]).max() <= 1e-12, k
    assert cc.gaps(c) >= cc.MIN_GAP and float(g["min_gap"]) >= cc.MIN_GAP
    assert np.array_equal(cc.run_restatement(c, torch.float32)["idx"], g["idx"])          # no index flips in float32 either
    if name == "G21e":
        assert len(c["dup"]) == 16 and 0.7 < c["mask1"].mean() < 0.9 and 0.7 < c["mask2"].mean() < 0.9
        for b, i, j in c["dup"]:
            assert c["mask1"][b, i] and c["mask2"][b, j] and np.array_equal(c["p1"][b, i], c["p2"][b, j])
            assert g["idx"][b, i] == j and g["dist"][b, i] == 0.0 and not g["grad_p1"][b, i].any()
        assert len({(b, j) for b, _, j in c["dup"]}) == 16                      # distinct originals
        assert (g["idx"][~c["mask1"]] == -1).all() and not g["dist"][~c["mask1"]].any()
        assert not g["grad_p1"][~c["mask1"]].any() and not g["grad_p2"][~c["mask2"]].any()


@needs_reference
@pytest.mark.parametrize("name", cc.NAMES)
def test_restatement_equals_reference(name):
    c = cc.case(name)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-5)):
        ref, r = cc.run_reference(c, dtype), cc.run_restatement(c, dtype)
        assert abs(r["loss"] - ref["loss"]) <= tol * max(1.0, abs(ref["loss"]))
        for k in ("grad_p1", "grad_p2"):
            assert cc.rel_error(r[k], ref[k]).max() <= tol, k


def test_fixture_sizes():
    sizes = {f: os.path.getsize(os.path.join(os.path.dirname(HEADER), "..", "tests", "golden", f)) for f in os.listdir(os.path.join(os.path.dirname(HEADER), "..", "tests", "golden"))}
    ours = [v for f, v in sizes.items() if f.startswith("G21")]
    assert len(ours) == 5 and max(ours) <= max(v for f, v in sizes.items() if not f.startswith("G21"))
