"""Host side of the one-launch tap-product form of the 64 -> 64 decoder stages (Engine.taps_fused, omni_conv3x3_up2_taps_sh_f16x3): the
entry point is declared, exported and bound, and its argument checks answer before any launch — no device is needed."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _buf(nbytes):
    """a 16-byte aligned host buffer: the checks look at pointers and shapes only"""
    raw = ctypes.create_string_buffer(nbytes + 16)
    addr = (ctypes.addressof(raw) + 15) & ~15
    return raw, ctypes.c_void_p(addr)


def test_entry_point_is_declared_exported_and_bound():
    from omnifusion_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "omnifusion.h")).read()
    assert re.search(r"^int omni_conv3x3_up2_taps_sh_f16x3\(const void\* src, const void\* wt16t, const float\* bias, void\* dst, int fmt,\s*"
                     r"int M, int Hl, int Wl, int C, int Cout, int act, omni_stream_t stream\);", hdr, re.M)
    assert "omni_conv3x3_up2_taps_sh_f16x3" in _lib.EXPORTS
    assert _lib.SIGNATURES["omni_conv3x3_up2_taps_sh_f16x3"] == _lib.SIGNATURES["omni_conv3x3_up2_sh_f16x3"]     # shaped like the kernel it replaces
    L = _lib.load()
    assert hasattr(L, "omni_conv3x3_up2_taps_sh_f16x3")


def test_argument_checks_answer_without_a_device():
    from omnifusion_amd import _lib
    L = _lib.load()
    fn = L.omni_conv3x3_up2_taps_sh_f16x3
    keep, p = zip(*[_buf(64) for _ in range(4)])
    x, w, b, o = p
    assert fn(None, w, b, o, 1, 1, 16, 16, 64, 64, 1, None) == _lib.OMNI_ERR_INVALID                  # null tensors
    assert b"omni_conv3x3_up2_taps_sh" in L.omni_last_error()
    assert fn(x, None, b, o, 1, 1, 16, 16, 64, 64, 1, None) == _lib.OMNI_ERR_INVALID
    assert fn(x, w, b, None, 1, 1, 16, 16, 64, 64, 1, None) == _lib.OMNI_ERR_INVALID
    assert fn(x, w, b, o, 1, 0, 16, 16, 64, 64, 1, None) == _lib.OMNI_ERR_INVALID                     # empty shape
    assert fn(x, w, b, o, 1, 1, 16, 16, 48, 64, 1, None) == _lib.OMNI_ERR_INVALID                     # channels: multiples of 32
    assert fn(ctypes.c_void_p(x.value + 8), w, b, o, 1, 1, 16, 16, 64, 64, 1, None) == _lib.OMNI_ERR_INVALID     # 16-byte alignment
    for fmt, M, Hl, Wl, C, Cout, act in [(0, 1, 16, 16, 64, 64, 1),          # fp32 result
                                         (9, 1, 16, 16, 64, 64, 1),          # f16x1
                                         (1, 1, 16, 16, 32, 64, 1),          # C
                                         (1, 1, 16, 16, 64, 32, 1),          # Cout
                                         (1, 1, 16, 16, 128, 128, 1),
                                         (1, 1, 8, 8, 64, 64, 1),            # a map it has no form for
                                         (1, 1, 12, 32, 64, 64, 1),          # bands are 8 rows
                                         (1, 1, 32, 16, 64, 64, 1),
                                         (1, 1, 16, 16, 64, 64, 2)]:         # GELU
        assert fn(x, w, b, o, fmt, M, Hl, Wl, C, Cout, act, None) == _lib.OMNI_ERR_UNSUPPORTED, (fmt, M, Hl, Wl, C, Cout, act)
    del keep


def test_engine_routes_by_key_set_mode_and_shape_only():
    """the path is chosen by the layer key, the arithmetic mode and the shape — the source of the up-sampling router, down to the launch of the
    tap-product forms, names neither the batch nor the latency plan nor anything the per-forward context derives from them"""
    import inspect
    from omnifusion_amd.model._engine import Engine, _Forward
    assert Engine.taps_fused <= frozenset(("de_conv2_0", "de_conv3_0"))
    src = inspect.getsource(_Forward.up_conv)
    head = src[:src.index("omni_conv3x3_up2_taps_sh_f16x3")]
    assert "taps_first" in head and "taps_fused" in head and "terms == 3" in head
    assert not re.search(r"\b_?(bs|lone|lat|rows_form|plan_batch|latency_plan|SINGLE_BATCH|NOMINAL_BATCH)\b|self\.M\b", head)
