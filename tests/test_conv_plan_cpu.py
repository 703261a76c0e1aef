"""CPU: which kernel omni_conv2d_sh_f16x3_ws launches, on what grid — omni_conv2d_sh_plan (conv_sh_plan in csrc/omni_conv_sh.hip), no device needed.

Every kernel family gives the same bits by design, so no output comparison can see a wrong rule; the decision itself is checked here against
  * tests/golden/conv_plan_parent.json: the answers of the revision BEFORE the choice became a function, recorded from a throwaway build of it whose launch
    sites wrote down what they were about to launch (tools/conv_plan_golden.py says how; it also holds the case set), and
  * rows copied by hand from committed kernel traces of that revision (profiles/r21a_layers_*_b8.txt), which neither that build nor this code produced.
"""
import ctypes
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_plan_parent.json")
TILE, PM, HALO, HALO2 = 0, 1, 2, 3


def _lib():
    from omnifusion_amd import _lib as L
    return L, L.load()


def _plan(lib, fmt, dims, post=0):
    """the 14 integers of the header's comment, or -status"""
    out = (ctypes.c_int * 14)()
    rc = lib.omni_conv2d_sh_plan(fmt, *dims, post, out, 14)
    return list(out) if rc == 0 else -rc


class _Options:
    """options for the duration of a block; the values found are put back"""

    def __init__(self, L, names):
        self.L, self.saved = L, {n: L.get_option(n) for n in names}

    def set(self, base, **opts):
        for n in self.saved:
            self.L.set_option(n, opts.get(n, base[n]))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            self.L.set_option(n, v)


def test_the_plan_is_the_parents_for_every_recorded_case():
    """Every (shape, option set, post, arithmetic mode) of the golden file: the parent's family, template arguments, grid, block size and split-K factor,
    or the parent's error status."""
    L, lib = _lib()
    with open(GOLDEN) as f:
        g = json.load(f)
    assert len(g["shapes"]) >= 100 and len(g["option_sets"]) >= 35 and g["fields"][0] == "family" and len(g["fields"]) == 14
    assert {p[0] for p in g["plans"]} == {TILE, PM, HALO, HALO2}                       # (the file exercises every family)
    ncases, bad = 0, []
    with _Options(L, g["defaults"]) as o:                                              # (every option the choice reads is set: the file's defaults + the set's)
        for k, opts in enumerate(g["option_sets"]):
            o.set(g["defaults"], **opts)
            for shape, answers in zip(g["shapes"], g["answers"]):
                for post in (0, 1):
                    want = answers[post][k]
                    want = g["plans"][want] if want >= 0 else want
                    for x1 in (0, 8):
                        got = _plan(lib, shape[1] | x1, shape[2:], post)
                        ncases += 1
                        if got != want and len(bad) < 10:
                            bad.append((shape, opts, post, x1, got, want))
    print(f"{ncases} plans compared")
    assert not bad, bad


# (fmt, (M, H, W, C1, C2, Cout, KH, KW, stride, pad, splitk)), options, kernel and its template arguments, total threads of the trace's grid column, source
TRACE_ROWS = [
    ((1, (144, 32, 32, 64, 0, 64, 3, 3, 1, 1, 1)), dict(conv_halo2=0), (HALO, dict(bn=64, th=4, iw=0)), 294912,
     "profiles/r21a_layers_parent_b8.txt:6  layer1.0.c1 conv3x3_halo_sh_kernel<64, 4, false, 0, false>"),
    ((1, (144, 32, 32, 64, 0, 64, 3, 3, 1, 1, 1)), dict(conv_halo2=2), (HALO2, dict(iw=0)), 147456,
     "profiles/r21a_layers_halo2_b8.txt:6  layer1.0.c1 halo2_sh_kernel<0, false>"),
    ((1, (144, 16, 16, 128, 0, 128, 3, 3, 1, 1, 1)), dict(conv_halo2=2), (HALO2, dict(iw=16)), 73728,
     "profiles/r21a_layers_halo2_b8.txt:14  layer2.0.c2 halo2_sh_kernel<16, false>"),
    ((1, (144, 8, 8, 256, 0, 256, 3, 3, 1, 1, 1)), dict(), (PM, dict(bn=128)), 110592,
     "profiles/r21a_layers_parent_b8.txt:23  layer3.0.c2 conv_pm_sh_kernel<128, false>"),
    ((1, (144, 32, 32, 64, 0, 128, 1, 1, 2, 0, 1)), dict(), (TILE, dict(bm=256, bn=128, wm=4, wn=2, nst=3, nl=0, pp=0)), 73728,
     "profiles/r21a_layers_parent_b8.txt:12  layer2.0.ds conv_sh_kernel<256, 128, 4, 2, 3, 0, false, false, false>"),
]


@pytest.mark.parametrize("call,opts,kernel,threads,source", TRACE_ROWS, ids=[r[4].split()[1] + "-" + str(i) for i, r in enumerate(TRACE_ROWS)])
def test_the_plan_is_the_kernel_of_the_committed_traces(call, opts, kernel, threads, source):
    L, lib = _lib()
    with open(GOLDEN) as f:
        defaults = json.load(f)["defaults"]
    fields = ["family", "bm", "bn", "wm", "wn", "nst", "nl", "pp", "th", "iw", "grid_x", "grid_y", "threads", "splitk"]
    with _Options(L, defaults) as o:
        o.set(defaults, **opts)
        got = _plan(lib, call[0], call[1])
    assert got != -1 and isinstance(got, list), (source, got)
    got = dict(zip(fields, got))
    family, targs = kernel
    assert got["family"] == family, (source, got)
    assert {k: got[k] for k in targs} == targs, (source, got)
    assert got["grid_x"] * got["grid_y"] * got["threads"] == threads, (source, got)


def test_the_plan_rejects_what_the_convolution_rejects():
    L, lib = _lib()
    ok = (18, 8, 8, 64, 0, 64, 3, 3, 1, 1, 1)
    assert isinstance(_plan(lib, 1, ok), list)
    for bad, status in (((18, 8, 8, 48, 0, 64, 3, 3, 1, 1, 1), L.OMNI_ERR_INVALID),          # channels
                        ((18, 8, 8, 64, 0, 64, 5, 5, 1, 2, 1), L.OMNI_ERR_INVALID),          # kernels up to 3 x 3
                        ((0, 8, 8, 64, 0, 64, 3, 3, 1, 1, 1), L.OMNI_ERR_INVALID),
                        ((1 << 20, 64, 64, 64, 0, 64, 3, 3, 1, 1, 1), L.OMNI_ERR_UNSUPPORTED)):   # 32-bit row indices
        assert _plan(lib, 1, bad) == -status, bad
    assert _plan(lib, 1, (18, 8, 8, 64, 0, 64, 3, 3, 1, 1, 2), post=1) == -L.OMNI_ERR_UNSUPPORTED      # no post-activation addend with split-K
    out = (ctypes.c_int * 14)()
    assert lib.omni_conv2d_sh_plan(1, *ok, 0, out, 13) == L.OMNI_ERR_INVALID                          # room for 14 integers
    assert _plan(lib, 1, (18, 1, 1, 64, 0, 64, 1, 1, 1, 0, 40))[13] == 2                              # split-K: at most the K-steps
