"""CPU: the f16x1 precision of training — the keyword on ops.conv2d, the modules, ops.convert and both trainable models;
the four C entry points beside their f16x3 siblings; their rejections before a device is touched; and the generated code: every f16x1
instantiation of the forward, data-gradient and weight-gradient kernels has exactly a third of its sibling's matrix instructions and fewer
LDS reads (counted as tests/test_precision_f16x1.py counts them: `v_mfma` and `ds_read` in the disassembly)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = {"omni_conv2d_split_weights_f16x1": "omni_conv2d_split_weights_f16x3", "omni_conv2d_nhwc_f16x1_ws": "omni_conv2d_nhwc_f16x3_ws",
         "omni_conv2d_bwd_data_f16x1": "omni_conv2d_bwd_data_f16x3", "omni_conv2d_bwd_weight_f16x1": "omni_conv2d_bwd_weight_f16x3"}
FAMILIES = ("conv_igemm_f32_kernel", "conv3x3_halo_f16x3_kernel", "conv_dgrad_kernel", "conv_wgrad_kernel")
BAD = ("f16x2", "fp16", "", "F16X1", None, 1)


class OnDevice(torch.Tensor):                                                  # a CPU tensor that answers is_cuda = True: the checks read nothing else
    @property
    def is_cuda(self):
        return True


def dev(t):
    return t.as_subclass(OnDevice)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    monkeypatch.setenv("OMNI_NET_PRECISION", "fp32")                           # the trainable modules do not read it


def test_functions_take_the_keyword_and_validate_it_before_a_launch():
    from omnifusion_amd import ops
    assert ops.PRECISIONS == ("f16x3", "f16x1")
    sig = inspect.signature(ops.conv2d).parameters["precision"]
    assert sig.kind is inspect.Parameter.KEYWORD_ONLY and sig.default == "f16x3"
    assert inspect.signature(ops.linear).parameters["precision"].default == "f16x3"
    X, Wt = dev(torch.rand(2, 32, 8, 8)), dev(torch.rand(32, 32, 3, 3))
    for bad in BAD:
        with pytest.raises(ValueError, match="precision must be 'f16x3' or 'f16x1'"):
            ops.conv2d(X, Wt, padding=1, precision=bad)
        with pytest.raises(ValueError, match="precision must be"):
            ops.linear(dev(torch.rand(4, 32)), dev(torch.rand(32, 32)), precision=bad)
    with pytest.raises(ValueError, match="training has no fp32 product path"):
        ops.conv2d(X, Wt, padding=1, precision="fp32")
    with pytest.raises(ValueError, match="training has no fp32 product path"):
        ops.linear(dev(torch.rand(4, 32)), dev(torch.rand(32, 32)), precision="fp32")
    with pytest.raises(TypeError):
        ops.conv2d(X, Wt, None, "f16x1")                                       # keyword-only
    with pytest.raises(ValueError, match="precision"):                        # the precision is checked first: nothing else is looked at
        ops.conv2d(torch.rand(2, 48, 8, 8), Wt, precision="half")
    with pytest.raises(ValueError, match="no CPU path"):                      # a valid mode goes on to the usual checks
        ops.conv2d(torch.rand(2, 32, 8, 8), torch.rand(32, 32, 3, 3), padding=1, precision="f16x1")


def test_modules_take_expose_and_show_the_precision():
    from omnifusion_amd import ops
    made = {"Conv2d": lambda **kw: ops.Conv2d(32, 64, 3, padding=1, act="relu", **kw), "Linear": lambda **kw: ops.Linear(64, 32, **kw),
            "TransformerBlock": lambda **kw: ops.TransformerBlock(**kw),
            "TransformerCascade": lambda **kw: ops.TransformerCascade(num_patch=10, depth=2, **kw)}
    for name, make in made.items():
        assert make().precision == "f16x3", name
        m = make(precision="f16x1")
        assert m.precision == "f16x1" and "precision=f16x1" in m.extra_repr() and "precision=f16x3" in make().extra_repr(), name
        for bad in BAD:
            with pytest.raises(ValueError, match="precision must be"):
                make(precision=bad)
        with pytest.raises(ValueError, match="training has no fp32 product path"):
            make(precision="fp32")
        a, b = make().state_dict(), m.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a), name
    assert set(made["Conv2d"](precision="f16x1").state_dict()) == set(torch.nn.Conv2d(32, 64, 3, padding=1).state_dict())
    assert set(made["Linear"](precision="f16x1").state_dict()) == set(torch.nn.Linear(64, 32).state_dict())
    cascade = made["TransformerCascade"](precision="f16x1")
    linears = [m for m in cascade.modules() if isinstance(m, ops.Linear)]
    assert len(linears) == 2 * 5 and all(m.precision == "f16x1" for m in linears)
    assert all(b.precision == "f16x1" for b in cascade.layer)
    assert all(m.precision == "f16x3" for m in made["TransformerCascade"]().modules() if isinstance(m, ops.Linear))


def test_convert_sets_the_precision_of_the_layers_it_creates():
    from omnifusion_amd import ops
    make = lambda: torch.nn.Sequential(torch.nn.Conv2d(3, 64, 7, stride=2, padding=3), torch.nn.BatchNorm2d(64), torch.nn.Conv2d(64, 64, 3, padding=1),
                                       torch.nn.Sequential(torch.nn.Conv2d(64, 32, 1)))
    assert inspect.signature(ops.convert).parameters["precision"].default is None
    for kw, want in (({}, "f16x3"), ({"precision": None}, "f16x3"), ({"precision": "f16x3"}, "f16x3"), ({"precision": "f16x1"}, "f16x1")):
        ref = make()
        model, names = ops.convert(make(), **kw)
        assert names == ["1", "2", "3.0"]
        convs = [m for m in model.modules() if isinstance(m, ops.Conv2d)]
        assert len(convs) == 2 and all(m.precision == want and f"precision={want}" in repr(m) for m in convs)
        assert type(model[0]) is torch.nn.Conv2d and list(model.state_dict()) == list(ref.state_dict())
    for bad in ("fp16", "", 3):
        with pytest.raises(ValueError, match="precision must be"):
            ops.convert(make(), precision=bad)
    with pytest.raises(ValueError, match="training has no fp32 product path"):
        ops.convert(make(), precision="fp32")
    root, names = ops.convert(torch.nn.Conv2d(32, 32, 3, padding=1), precision="f16x1")
    assert names == [""] and root.precision == "f16x1"


def _trainable():
    from omnifusion_amd.model.trainable import spherical_fusion as single
    from omnifusion_amd.model.trainable_iterative import spherical_fusion as iterative
    return (single, {}), (iterative, {"patch_size": (128, 128)})


def test_trainable_constructors_take_and_report_the_precision():
    from omnifusion_amd import ops
    from omnifusion_amd.model.trainable import _Conv, _Head, _Stem
    for cls, kw in _trainable():
        sig = inspect.signature(cls.__init__).parameters["precision"]
        assert sig.kind is inspect.Parameter.KEYWORD_ONLY and sig.default == "f16x3"
        assert cls(**kw).precision == "f16x3"                                  # OMNI_NET_PRECISION = fp32 is set and not read
        net = cls(**kw, precision="f16x1")
        assert net.precision == "f16x1" and net.transformer.precision == "f16x1"
        convs = [m for m in net.modules() if isinstance(m, _Conv) and not isinstance(m, (_Stem, _Head))]
        assert len(convs) == 35 + 1 + 9 and all(m.precision == "f16x1" for m in convs)        # ResNet-34 body, down / down1, the decoder
        assert all(m.precision == "f16x1" for m in net.modules() if isinstance(m, ops.Linear))
        dflt = cls(**kw)
        assert all(m.precision == "f16x3" for m in dflt.modules() if isinstance(m, (_Conv, ops.Linear)))
        for bad in ("f16x2", "fp16", "", "F16X1"):
            with pytest.raises(ValueError, match="precision must be"):
                cls(**kw, precision=bad)
        with pytest.raises(ValueError, match="training has no fp32 product path"):
            cls(**kw, precision="fp32")
        with pytest.raises(TypeError):
            cls(4, 18, (128, 128), (80, 80), "f16x1")                          # keyword-only
        a, b = dflt.state_dict(), net.state_dict()
        assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)


def test_entry_points_declared_exported_and_bound_like_their_siblings():
    from omnifusion_amd import _lib
    header = open(os.path.join(ROOT, "include", "omnifusion.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = _lib.load()
    for new, old in PAIRS.items():
        assert re.search(r"\bint\s+" + new + r"\s*\(", code), new
        assert new in _lib.EXPORTS and hasattr(L, new), new
        assert _lib.SIGNATURES[new] == _lib.SIGNATURES[old], new
        assert tuple(getattr(L, new).argtypes) == tuple(getattr(L, old).argtypes) and getattr(L, new).restype is getattr(L, old).restype
        args = lambda n: re.sub(r"\s+", " ", re.search(r"\bint\s+" + n + r"\s*\((.*?)\)\s*;", code, flags=re.S).group(1))
        assert args(new) == args(old), new                                     # the declared parameter lists, word for word
    assert L.omni_version() == 200
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(name in integration for name in PAIRS)


def test_c_boundary_rejects_before_touching_a_device():
    """The rejections of tests/test_conv_bwd_cpu.py for the f16x1 entry points, each with its sibling's code.  The non-null pointers are never
    dereferenced."""
    from omnifusion_amd import _lib
    L = _lib.load()
    p, z = ctypes.c_void_p(4096), None
    INV, UNS = _lib.OMNI_ERR_INVALID, _lib.OMNI_ERR_UNSUPPORTED
    big = 1 << 30
    good = (2, 8, 8, 32, 0, 32, 3, 3, 1, 1)
    for sfx in ("f16x1", "f16x3"):
        data, weight = getattr(L, "omni_conv2d_bwd_data_" + sfx), getattr(L, "omni_conv2d_bwd_weight_" + sfx)
        split, conv = getattr(L, "omni_conv2d_split_weights_" + sfx), getattr(L, "omni_conv2d_nhwc_" + sfx + "_ws")
        for fn in (data, weight):
            assert fn(z, p, p, p, p, *good, p, big, z) == INV
            assert fn(p, p, p, p, p, *good, p, 16, z) == INV and b"workspace" in L.omni_last_error()
            assert fn(p, p, p, p, p, 2, 8, 8, 48, 0, 32, 3, 3, 1, 1, p, big, z) == INV and b"multiples of 32" in L.omni_last_error()
            assert fn(p, p, p, p, p, 2, 8, 8, 32, 0, 32, 2, 2, 1, 0, p, big, z) == UNS and b"1x1 or 3x3" in L.omni_last_error()
            assert fn(p, p, p, p, p, 2, 8, 8, 32, 0, 32, 3, 3, 4, 1, p, big, z) == UNS and b"stride" in L.omni_last_error()
        assert data(p, p, p, z, z, *good, p, big, z) == INV and b"requested" in L.omni_last_error()
        assert data(p, p, p, z, p, *good, p, big, z) == INV                     # dx2 without a second source
        assert weight(p, p, z, p, p, 2, 8, 8, 32, 32, 32, 3, 3, 1, 1, p, big, z) == INV   # C2 > 0 without src2
        assert split(p, p, 32, 40, z) == INV and split(z, p, 32, 32, z) == INV
        #          src1 src2 wt bias res dst  M  H  W  C1  C2  Cout KH KW s  p  act splitk ws ws_bytes stream
        assert conv(z, z, p, z, z, p, 2, 8, 8, 32, 0, 32, 3, 3, 1, 1, 0, 1, z, 0, z) == INV and b"null" in L.omni_last_error()
        assert conv(p, z, p, z, z, p, 2, 8, 8, 48, 0, 32, 3, 3, 1, 1, 0, 1, z, 0, z) == INV and b"multiples of 32" in L.omni_last_error()
        assert conv(p, z, p, z, z, p, 2, 8, 8, 32, 32, 32, 3, 3, 1, 1, 0, 1, z, 0, z) == INV             # C2 > 0 without src2
        assert conv(p, z, p, z, z, p, 2, 8, 8, 32, 0, 32, 4, 4, 1, 1, 0, 1, z, 0, z) == INV and b"3x3" in L.omni_last_error()
        assert conv(p, z, p, z, z, p, 2, 8, 8, 64, 0, 32, 3, 3, 1, 1, 0, 4, z, 0, z) == INV and b"workspace" in L.omni_last_error()


def _kernels():
    """{family<template arguments>: (v_mfma, ds_read)} of the convolution kernels behind ops.conv2d, from the disassembly"""
    from omnifusion_amd import build, isa
    build.build()
    out = {}
    for obj in isa.objects():
        if os.path.basename(obj) not in ("omni_conv.o", "omni_conv_bwd.o"):
            continue
        cur = None
        for line in isa.disassemble(obj).splitlines():
            if line.endswith(">:"):
                m = re.match(r"_ZN12_GLOBAL__N_1\d+(" + "|".join(FAMILIES) + r")I(.*?)EEEv", line.split("<", 1)[1][:-2])
                cur = None
                if m:
                    args = re.findall(r"L[ib](\d+)E", m.group(2) + "E")
                    key = m.group(1) + "<" + ",".join(args) + ">"
                    assert key not in out, key
                    cur = out[key] = [0, 0]
            elif cur is not None and line.startswith("\t"):
                ins = line.split("//")[0].strip()
                cur[0] += ins.startswith("v_mfma")
                cur[1] += ins.startswith("ds_read")
    return out


def test_isa_f16x1_kernels_have_a_third_of_the_matrix_instructions():
    k = _kernels()
    # the last template argument is X1; the forward's fp32 form <..., F16X3 = 0, X1 = 0> has no f16x1 sibling
    x1 = sorted(n for n in k if n.endswith(",1>") or n.endswith("<1>"))
    x3 = sorted(n for n in k if n not in x1 and not (n.startswith("conv_igemm_f32_kernel") and n.endswith(",0,0>")))
    sibling = {n: re.sub(r"(,|<)1>$", r"\g<1>0>", n) for n in x1}
    assert sorted(sibling.values()) == x3, (x1, x3)
    assert len(x1) == 3 + 2 + 2 + 1                                            # forward tiles, halo tiles, dgrad tiles, wgrad
    for n, s in sibling.items():
        (m1, r1), (m3, r3) = k[n], k[s]
        print(f"{n}: v_mfma {m1} (sibling {m3}), ds_read {r1} (sibling {r3})")
        assert m1 > 0 and 3 * m1 == m3, (n, m1, m3)
        assert r1 < r3, (n, r1, r3)


def test_isa_check_passes():
    from omnifusion_amd import build, isa
    build.build()
    assert isa.check() == []
