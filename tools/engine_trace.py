"""The launch sequence of Engine.network / Engine.transformer as DATA, recorded without a GPU: the library is replaced by a stub that notes
every call and answers 0, the tensors are (untouched) CPU tensors, and only the pure host functions of the real library are let through.

    python tools/engine_trace.py --record tests/golden/engine_trace_parent.json     on the revision whose launches are to be pinned
    python tools/engine_trace.py --dump "single f16x3 bs1"                          one configuration in full, to diff against a parent checkout
    python tools/engine_trace.py --list                                             the configuration keys
    python tools/engine_trace.py --time 200                                         host time of Engine.network at bs 1 under the stub (median, ms)

The file runs unmodified against any revision of model/_engine.py that keeps `_p` as its only pointer maker: it replaces `_lib.load`,
`_lib.stream_of`, `torch.cuda.current_stream`, `torch.cuda.is_current_stream_capturing` and `_engine._p`, and reads the `_lib.check` labels
through `_lib.CALL_LOG`.  One line per library call: label | function | arguments, a pointer as `w:<key of Engine.w>` or
`b<k>:<storage bytes>[+<byte offset>]` (k: order of first appearance in the trace), the stream as `stream`, a null pointer as `0`.
tests/test_engine_trace_cpu.py replays the matrix against tests/golden/engine_trace_parent.json.
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from omnifusion_amd import _lib, weights                      # noqa: E402
from omnifusion_amd.model import _engine                      # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_trace_parent.json")
NROWS, N, P, FOV = 4, 18, 128, 80
PASS_THROUGH = ("omni_conv2d_splitk_plan", "omni_up2_heads_scratch_bytes", "omni_heads_pack_f16x3", "omni_patch_centers")   # pure host functions
ANCHORS = ("single f16x3 bs1", "single f16x3 bs8", "single f16x1 bs8", "single fp32 bs8", "iterative f16x3 bs1", "iterative f16x3 bs8")
SWITCHES = [dict(latency_plan=False), dict(fuse_ln=False), dict(fc2_slices=1), dict(fc2_slices=2), dict(fuse_fc2_ln=False), dict(fuse_up=False),
            dict(tail_chunk=1), dict(front_chunk=1), dict(fold_point_feat=False), dict(rows_gemm=False), dict(taps_first=frozenset()),
            dict(taps_first=frozenset(("de_conv0_0", "de_conv1_0"))), dict(taps_fused=frozenset()),
            dict(SINGLE_BATCH=1)]                             # (the last: layer1's final convolution plans S > 1 — the late `post` pass of the convolution shim)


def configurations():
    """{key: (what, iterative, precision, bs, confidence, {Engine switch: value})}, what = "network" | "transformer" """
    out = {}

    def add(model, prec, bs, confidence=True, what="network", **sw):
        tag = "".join(f" {k}={sorted(v) if isinstance(v, frozenset) else v}" for k, v in sw.items())
        head = "transformer" if what == "transformer" else model
        out[f"{head} {prec} bs{bs}" + ("" if confidence else " confidence=False") + tag] = (what, model == "iterative", prec, bs, confidence, sw)
    for model in ("single", "iterative"):
        for prec in _engine.PRECISIONS:
            for bs in (1, 2, 8):
                add(model, prec, bs)
    add("single", "f16x3", 2, confidence=False)
    for prec in ("f16x3", "fp32"):
        for confidence in (True, False):
            add("single", prec, 2, confidence=confidence, fuse_heads=False)
    for sw in SWITCHES:
        for bs in (1, 8):
            add("single", "f16x3", bs, **sw)
    for prec in _engine.PRECISIONS:
        for bs in (1, 3):
            add("single", prec, bs, what="transformer")
    return out


class _Ptr:
    def __init__(self, t):
        self.t = t


class _Stream:
    cuda_stream = 0

    def synchronize(self):
        pass


class Recorder:
    """the stand-in for the loaded library, and the maker of the symbolic names"""

    def __init__(self):
        self.real = _lib.load()
        self.calls, self.keep, self.bufs, self.w = [], [], {}, None
        self.quiet = False                                    # --time: answer 0 and note nothing, so that the engine's own host time shows

    def begin(self, w):
        self.calls, self.keep, self.bufs, self.w = [], [], {}, w

    def __getattr__(self, name):
        if name in PASS_THROUGH:
            return getattr(self.real, name)
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            if self.quiet:
                return 0
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.calls.append((name, [self.render(a, t) for a, t in zip(args, argtypes)]))
            return 0
        return call

    def ptr(self, t):
        if t is None:
            return None
        self.keep.append(t)                                   # alive until the trace ends: no address comes twice
        return _Ptr(t)

    def render(self, a, ctype):
        if ctype is not ctypes.c_void_p:
            assert isinstance(a, (int, float)), (a, ctype)
            return repr(a)
        if a is None:
            return "0"
        if isinstance(a, _Stream):
            return "stream"
        st = a.t.untyped_storage()
        base, off = st.data_ptr(), a.t.data_ptr() - st.data_ptr()
        name = next((f"w:{k}" for k, v in self.w.items() if v.untyped_storage().data_ptr() == base), None)
        if name is None:
            name = self.bufs.setdefault(base, f"b{len(self.bufs)}:{st.nbytes()}")
        return name + (f"+{off}" if off else "")


def state_dict(iterative, seed=1):
    rng = np.random.default_rng(seed)
    sd = {}
    for name, (shape, dtype) in weights.schema(N, iterative).items():
        if dtype == "int64":
            v = np.zeros(shape, np.int64)
        else:
            v = (0.05 * rng.standard_normal(shape)).astype(np.float32)
            if name.endswith("running_var"):
                v = 1.0 + np.abs(v)
        sd[name] = torch.from_numpy(v)
    return sd


class Tracer:
    """`patch(obj, name, value)` sets an attribute for the life of the tracer's user: pytest's monkeypatch.setattr, or `patched()` below"""

    def __init__(self, patch):
        self.patch, self.rec, self.packed = patch, Recorder(), {}
        stream = _Stream()
        patch(_lib, "load", lambda: self.rec)
        patch(_lib, "stream_of", lambda t: stream)
        patch(torch.cuda, "current_stream", lambda device=None: stream)
        patch(torch.cuda, "is_current_stream_capturing", lambda: False)
        patch(_engine, "_p", self.rec.ptr)

    def engine(self, iterative, precision):
        """a fresh lane over the weights packed once per model: its own copy of the `w` dict (the rows GEMMs cache into it), an empty workspace"""
        if iterative not in self.packed:
            e = _engine.Engine(NROWS, N, P, FOV, iterative, precision="f16x3")
            e.pack(state_dict(iterative), "cpu")
            self.packed[iterative] = e
        e = self.packed[iterative].lane()
        e.w, e.precision = dict(e.w), precision
        return e

    def run(self, cfg):
        """the call lines of one configuration"""
        what, iterative, precision, bs, confidence, switches = cfg
        for k, v in switches.items():
            self.patch(_engine.Engine, k, v)
        try:
            e = self.engine(iterative, precision)
            self.rec.begin(e.w)
            log = []
            self.patch(_lib, "CALL_LOG", log)
            new = lambda *s: torch.empty(s, dtype=torch.float32)
            if what == "transformer":
                e.transformer(new(bs * N, P // 32, P // 32, 32), bs)
            else:
                pf = e.w["point_feat"] if not iterative else \
                    e.mlp_points("mlp_points2", new(N, 3, P // 4, P // 4), new(bs, N, 1, P // 4, P // 4), bs * N)
                e.network(new(bs, N, 3, P, P), pf, bs, confidence)
            assert len(log) == len(self.rec.calls), (len(log), len(self.rec.calls))     # one _lib.check label per library call
            return [f"{label} | {name} | " + " ".join(args) for label, (name, args) in zip(log, self.rec.calls)]
        finally:
            self.patch(_lib, "CALL_LOG", None)
            self.rec.begin(None)
            for k in switches:                                # the class defaults (the values a patch-undo would restore as well)
                self.patch(_engine.Engine, k, DEFAULTS[k])


DEFAULTS = {k: getattr(_engine.Engine, k) for sw in SWITCHES + [dict(fuse_heads=False)] for k in sw}


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


@contextlib.contextmanager
def patched():
    """monkeypatch.setattr for the command line"""
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        yield patch
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)


def record(path):
    head = subprocess.run(["git", "-C", ROOT, "log", "-1", "--format=%H %s"], capture_output=True, text=True, check=True).stdout.strip()
    same = subprocess.run(["git", "-C", ROOT, "diff", "--quiet", "HEAD", "--", "omnifusion_amd/model/_engine.py"]).returncode == 0
    with patched() as patch:
        tr = Tracer(patch)
        traces = {k: tr.run(cfg) for k, cfg in configurations().items()}
    index = {}
    anchors = {k: [index.setdefault(line, len(index)) for line in traces[k]] for k in ANCHORS}
    rows = lambda items: "\n  " + ",\n  ".join(items) + "\n "                       # one entry per line
    pairs = lambda d: "{" + rows(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in d.items()) + "}"
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join([' "recorded_from": ' + json.dumps(head + ("" if same else " + an edited model/_engine.py")),
                                    ' "recorder": "tools/engine_trace.py --record"',
                                    ' "digests": ' + pairs({k: digest(v) for k, v in traces.items()}),
                                    ' "anchors": ' + pairs(anchors),
                                    ' "calls": [' + rows(map(json.dumps, index)) + "]"]) + "\n}\n")
    print(f"{len(traces)} configurations, {sum(map(len, traces.values()))} calls, {len(set(l for v in traces.values() for l in v))} distinct; "
          f"{len(index)} distinct in the {len(ANCHORS)} anchors -> {path}, {os.path.getsize(path)} bytes")


def host_time(n):
    with patched() as patch:
        tr = Tracer(patch)
        e = tr.engine(False, "f16x3")
        tr.rec.quiet = True
        x = torch.empty((1, N, 3, P, P), dtype=torch.float32, device="meta")      # every buffer of the forward follows its device: no memory is mapped
        ts = []
        for _ in range(n + 20):
            tr.rec.begin(e.w)                                 # (drops the tensors kept alive by the last call)
            t0 = time.perf_counter()
            e.network(x, e.w["point_feat"], 1, True)
            ts.append((time.perf_counter() - t0) * 1e3)
    ts = sorted(ts[20:])
    print(f"Engine.network, bs 1, stub library: median of {n} calls {ts[n // 2]:.3f} ms (min {ts[0]:.3f}, 90th percentile {ts[n * 9 // 10]:.3f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--record", metavar="PATH")
    ap.add_argument("--dump", metavar="KEY")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--time", type=int, metavar="CALLS")
    opt = ap.parse_args()
    if opt.list:
        print("\n".join(configurations()))
    if opt.dump:
        with patched() as patch:
            print("\n".join(Tracer(patch).run(configurations()[opt.dump])))
    if opt.record:
        record(opt.record)
    if opt.time:
        host_time(opt.time)
