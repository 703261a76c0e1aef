"""spherical_fusion (single pass) — host-side mirror of /root/reference/model/spherical_model.py:190-314.

Same class name, constructor arguments and forward signature as the reference, and an `nn.Module` like it:

    net = spherical_fusion(nrows=4, npatches=18, patch_size=(128, 128), fov=(80, 80))
    net = nn.DataParallel(convert_model(net))   # test.py:105-107 (single-GPU process; see below)
    net.load_state_dict(ckpt)                   # reference schema (5-D conv weights), 'module.' prefix optional
    net.cuda(); net.eval()
    depth = net(rgb, confidence=True)           # rgb [B,3,H,W] float32 on the GPU -> [B,1,H,W]

`state_dict()` / `parameters()` / `buffers()` expose exactly the reference's 363 (iterative: 375) tensors under the
reference's names (model/spherical_model.py:197-235): a checkpoint round-trips.  They are the MASTER copy; the forward
runs from packed device buffers (BN folded, implicit-GEMM weight layouts, split-half operands) rebuilt lazily whenever
the master copy changed (`load_state_dict` — also through a wrapping `nn.DataParallel` —, `.cuda()`, `.to()`).

The forward is a launch sequence over libomnifusion_hip.so (see _engine.py); there is no autograd through the network
(inference only, as test.py:197 runs the reference under torch.no_grad()): parameters have requires_grad=False and the
module is constructed in eval mode; `train(True)` is accepted, but a forward in training mode raises (batch-statistics
BatchNorm is not implemented).  Multi-GPU: one process per GPU shards the batch (omnifusion_amd/dist.py, bench.py) — the
fast way.  `nn.DataParallel` (test.py:105-111) works as well: over one device it is a pass-through; over several, every
replica thread runs on a per-DEVICE execution context (packed weights, lanes) owned by the wrapped module and guarded by a
lock (`_replicate_for_data_parallel`, `_device_context`) — replicas never share an Engine, and the packed weights are built
once per device from the master copy, not from the parameter broadcast DataParallel repeats on every forward.
"""
import contextlib
import os
import threading

import torch
from torch import nn

from ._engine import Engine, PRECISIONS, strip_module_prefix
from ..equi_pers.equi2pers_v3 import equi2pers_patches
from .. import _lib
from ..weights import schema

_BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


def _build_tree(root, sch):
    """register the reference's parameter / buffer names on a tree of plain container modules"""
    for name, (shape, dtype) in sch.items():
        *path, leaf = name.split(".")
        m = root
        for p in path:
            if p not in m._modules:
                m.add_module(p, nn.Module())
            m = m._modules[p]
        t = torch.zeros(shape, dtype=torch.int64 if dtype == "int64" else torch.float32)
        if leaf in _BUFFERS:
            m.register_buffer(leaf, t)
        else:
            m.register_parameter(leaf, nn.Parameter(t, requires_grad=False))


class _Pending:
    """result of a pipelined forward: tensors that a side stream is still writing"""
    def __init__(self, out, event, stream, input_read=None):
        self._out, self._event, self._stream, self._input_read = out, event, stream, input_read

    @property
    def event(self):
        """recorded on the side stream after the forward"""
        return self._event

    @property
    def input_read(self):
        """recorded right after equi2pers, the only reader of the input batch: the batch may be overwritten once it has completed"""
        return self._input_read if self._input_read is not None else self._event

    def get(self):
        cur = torch.cuda.current_stream(self._stream.device)
        cur.wait_event(self._event)
        for t in (self._out if isinstance(self._out, (list, tuple)) else [self._out]):
            t.record_stream(cur)                                           # allocated on the side stream, used on this one
        return self._out


def _concurrent_streams(n, device, candidates=12, spin=400_000, first=None):
    """n streams that really run side by side.  HIP multiplexes its streams onto a few hardware queues (4 by default) and two
    streams on one queue serialise — which pairs collide depends on every stream created before, so it is MEASURED: two spin
    kernels on a pair of candidate streams take T when the queues differ and 2T when they are the same.
    `first`: a stream the caller already works on (the others are chosen to run beside IT)."""
    import time
    dev = torch.device(device)
    cand = ([first] if first is not None else []) + [torch.cuda.Stream(device=dev) for _ in range(candidates)]

    def spin_pair(a, b):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with torch.cuda.stream(a):
            torch.cuda._sleep(spin)
        with torch.cuda.stream(b):
            torch.cuda._sleep(spin)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0

    spin_pair(cand[0], cand[0])                                            # warm-up
    serial = min(spin_pair(cand[0], cand[0]) for _ in range(3))
    chosen = [cand[0]]
    for c in cand[1:]:
        if len(chosen) == n:
            break
        if all(min(spin_pair(c, k) for _ in range(2)) < 0.75 * serial for k in chosen):
            chosen.append(c)
    while len(chosen) < n:                                                 # fewer independent queues than asked for: share
        chosen.append(cand[len(chosen) % len(cand)])
    return chosen


class _Pipelined:
    def __init__(self, net, depth, graphs=False):
        if depth < 1:
            raise ValueError("depth >= 1")
        self.net, self.depth, self.graphs = net, int(depth), bool(graphs)
        self.k, self.slots, self.version, self.captured = 0, None, None, {}

    def _enter(self, eng):
        net = self.net
        state = (net._eng, "LANES" in net.__dict__, net.__dict__.get("LANES"))
        net._eng, net.LANES = eng, 1                                       # whole batch per kernel; the overlap comes from the next batch
        return state

    def _leave(self, state):
        net = self.net
        net._eng = state[0]
        if state[1]:
            net.LANES = state[2]
        else:
            del net.LANES

    def _capture(self, slot, eng, stream, rgb, args, kwargs):
        """one hipGraph per (slot, input shape, arguments): the ~135 launches of a forward replay from ONE graph launch — below
        ~4 panoramas per forward the host cannot enqueue them as fast as several streams execute them"""
        net = self.net
        static_in = rgb.clone()
        state = self._enter(eng)
        try:
            stream.wait_stream(torch.cuda.current_stream(rgb.device))
            with torch.cuda.stream(stream):
                net.forward(static_in, *args, **kwargs)                    # warm-up on this slot: workspace, allocator pools
            torch.cuda.synchronize(rgb.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                static_out = net.forward(static_in, *args, **kwargs)
        finally:
            self._leave(state)
        return g, static_in, static_out

    def __call__(self, rgb, *args, **kwargs):
        net = self.net
        net._check(rgb)                                                    # (re)packs the weights if the master copy changed
        if self.slots is None or self.version != net._pack_version or self.slots[0][1].device != rgb.device:
            self.slots = [(net._eng.lane(), st) for st in _concurrent_streams(self.depth, rgb.device)]
            self.version, self.captured = net._pack_version, {}
        slot = self.k % self.depth
        eng, stream = self.slots[slot]
        self.k += 1
        cur = torch.cuda.current_stream(rgb.device)
        if self.graphs:
            key = (slot, tuple(rgb.shape), args, tuple(sorted(kwargs.items())))
            if key not in self.captured:
                self.captured[key] = self._capture(slot, eng, stream, rgb, args, kwargs)
            g, static_in, static_out = self.captured[key]
            stream.wait_stream(cur)
            rgb.record_stream(stream)
            with torch.cuda.stream(stream):
                static_in.copy_(rgb, non_blocking=True)
                input_read = stream.record_event()                         # the caller's batch has been copied
                g.replay()
                # the graph's output buffers are rewritten by this slot's next replay: hand out copies
                out = [t.clone() for t in static_out] if isinstance(static_out, (list, tuple)) else static_out.clone()
                event = stream.record_event()
            return _Pending(out, event, stream, input_read)
        stream.wait_stream(cur)                                            # the input was produced on the caller's stream
        rgb.record_stream(stream)
        state = self._enter(eng)
        net._want_input_event, net._input_read = True, None
        try:
            with torch.cuda.stream(stream):
                out = net.forward(rgb, *args, **kwargs)
                event = stream.record_event()
            input_read = net._input_read
        finally:
            net._want_input_event, net._input_read = False, None
            self._leave(state)
        return _Pending(out, event, stream, input_read)


class _DeviceContext:
    """execution context of one device: packed weights (Engine), half-batch lanes, and the lock that serialises the
    replica threads of an nn.DataParallel that share the device"""
    def __init__(self, eng):
        self.eng, self.lanes, self.version, self.lock = eng, None, -1, threading.RLock()


class spherical_fusion(nn.Module):
    _ITERATIVE = False
    _want_input_event = False     # pipelined(): record an event when the forward has finished reading its input batch
    _input_read = None
    # Two halves of the batch on two streams.  Every layer of the network is ONE kernel whose last blocks leave most of the
    # chip idle (the deep layers are 2.25 blocks per CU at 8 panoramas); with two independent half-batch chains in flight
    # the scheduler fills one chain's tail with the other chain's blocks.  Results are bit-identical to the single-stream
    # path (split-K is planned for a nominal batch, every output element is one k-ordered chain).  OMNI_LANES=1 disables.
    LANES = int(os.environ.get("OMNI_LANES", "2"))

    def __init__(self, nrows=4, npatches=18, patch_size=(128, 128), fov=(80, 80), *, precision=None):
        """precision: "f16x3" (fp32-class), "f16x1" (one fp16 product per convolution block: faster, ~1e-3 relative per convolution,
        see DESIGN.md 5) or "fp32"; None = OMNI_NET_PRECISION, else "f16x3".  Weights, state_dict and outputs keep their formats in every mode."""
        super().__init__()
        if precision is not None and precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS} (or None), got {precision!r}")
        self.nrows, self.npatches, self.patch_size, self.fov = nrows, npatches, patch_size, fov
        _build_tree(self, schema(npatches, self._ITERATIVE))
        self._eng = Engine(nrows, npatches, patch_size, fov, self._ITERATIVE, precision=precision)
        self._loaded = False          # a checkpoint has been loaded (the zero-initialised master copy is not a model)
        self._dirty = True            # packed buffers are out of date w.r.t. the master copy
        self._lanes = None
        self._master_version = 0      # bumped whenever the master copy changes (load_state_dict, .cuda() / .to())
        self.__dict__["_origin"] = None                  # a DataParallel replica: the wrapped module (plain attribute, not a submodule)
        self._contexts, self._contexts_lock = {}, threading.Lock()       # per-device contexts of the replicas (shared with them)
        self.training = False         # inference module: constructed in eval mode
        self.register_load_state_dict_post_hook(spherical_fusion._after_load)

    # ---- master copy <-> packed buffers
    @staticmethod
    def _after_load(module, incompatible_keys):
        # fires for a direct load_state_dict() AND when a wrapper (nn.DataParallel, test.py:107-110) loads through us
        if not incompatible_keys.missing_keys:
            module._loaded = True
        module._dirty = True
        module._master_version += 1

    def load_state_dict(self, state_dict, strict=True, assign=False):
        sd = strip_module_prefix(state_dict)                               # train_erp_depth.py:307 saves through DataParallel
        sd = {k: v for k, v in sd.items() if not k.endswith("total_ops") and not k.endswith("total_params")}   # thop residue
        return super().load_state_dict(sd, strict=strict, assign=assign)

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._dirty = True                                                 # .cuda() / .to(): repack on the new device
        self._master_version = self.__dict__.get("_master_version", 0) + 1
        return out

    # ---- nn.DataParallel over several devices (test.py:105-111).  torch replicates the module tree per forward: a replica is a
    # shallow copy of __dict__ WITHOUT parameters (its state_dict() is empty, the broadcast copies are plain attributes) that runs
    # on its own thread.  A replica therefore never packs and never touches the wrapped module's Engine: it borrows the execution
    # context of ITS device from the wrapped module, under that context's lock.
    def _replicate_for_data_parallel(self):
        replica = super()._replicate_for_data_parallel()
        replica.__dict__["_origin"] = self.__dict__.get("_origin") or self
        return replica

    def _device_context(self, dev):
        """(wrapped module only) the execution context of `dev`, its packed weights in step with the master copy"""
        dev = torch.device(dev)
        with self._contexts_lock:
            ctx = self._contexts.get(dev)
            if ctx is None:
                ctx = self._contexts[dev] = _DeviceContext(None)
        with ctx.lock:
            if not self._loaded:
                raise RuntimeError("no weights loaded: call load_state_dict() first")
            if ctx.eng is None or ctx.version != self._master_version:
                eng = Engine(self.nrows, self.npatches, self.patch_size, self.fov, self._ITERATIVE, precision=self._eng.precision)
                with torch.cuda.device(dev):
                    eng.pack(nn.Module.state_dict(self), dev)
                ctx.eng, ctx.lanes, ctx.version = eng, None, self._master_version
        return ctx

    @contextlib.contextmanager
    def _execution(self, rgb):
        """what a forward runs under: nothing for the module itself; for a DataParallel replica its device's context, locked,
        bound to THIS replica object (a replica's __dict__ is its own, one thread uses it)"""
        origin = self.__dict__.get("_origin")
        if origin is None or not self.__dict__.get("_is_replica", False):
            yield
            return
        if self.training:
            raise NotImplementedError("spherical_fusion is inference-only (eval-mode BatchNorm folded into the weights): call .eval()")
        self._eng.check_input(rgb)
        ctx = origin._device_context(rgb.device)
        with ctx.lock:
            d = self.__dict__
            d["_eng"], d["_lanes"], d["_loaded"], d["_dirty"], d["_pack_version"] = ctx.eng, ctx.lanes, True, False, ctx.version
            try:
                yield
            finally:
                ctx.lanes = d["_lanes"]

    @property
    def precision(self):
        """the arithmetic mode of the convolutions ("f16x3", "f16x1" or "fp32"), fixed at construction"""
        return self._eng.precision

    def state_dict_schema(self):
        return schema(self.npatches, self._ITERATIVE)

    def _master_device(self):
        return self.conv1.weight.device

    def _sync_packed(self, rgb_device):
        """rebuild the packed device buffers if the master copy changed; all lanes (execution contexts) follow"""
        if not self._loaded:
            raise RuntimeError("no weights loaded: call load_state_dict() first")
        dev = self._master_device()
        if dev.type != "cuda":
            raise RuntimeError(f"the model's parameters are on {dev}: move it to an MI355X with .cuda() — there is no CPU path")
        if self._dirty or self._eng.device != dev:
            self._eng.pack(super().state_dict(), dev)
            self._lanes = None                                             # lanes alias the packed weights: rebuild them
            self._pack_version = getattr(self, "_pack_version", 0) + 1     # ... and so do the slots of pipelined()
            self._dirty = False
        if rgb_device != dev:
            hint = ""
            if torch.cuda.device_count() > 1:
                hint = " (move the input to the model's device; nn.DataParallel scatters it per replica, omnifusion_amd/dist.py shards it per process)"
            raise ValueError(f"weights are on {dev}, input on {rgb_device}{hint}")

    def overflowed(self):
        """True if any activation left the range the split-half fp16 format represents (|x| > 65504) since the last call.
        Reads a device flag (synchronises).  The f16x3 path saturates such values instead of producing inf/NaN; rerun with
        OMNI_NET_PRECISION=fp32 for a checkpoint that trips this."""
        return self._eng.read_overflow_flag()

    def graphed(self, example, *args, **kwargs):
        """Capture one forward for inputs shaped like `example` into a hipGraph and return `run(rgb) -> output`.

        The ~150 launches of a forward are stream-ordered, allocation-free inside the library and sync-free once the
        geometry handles exist, so the whole launch sequence replays from one graph launch: at batch 1 the forward is
        launch-bound (2.6 ms eager vs the sum of its kernels), which is what the graph removes.  Outputs live in static
        buffers that the next replay overwrites (clone them to keep them)."""
        static_in = example.clone()
        for _ in range(2):                                   # warm-up: geometry handles, split-K workspace, allocator pools
            self.forward(static_in, *args, **kwargs)
        torch.cuda.synchronize(static_in.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_out = self.forward(static_in, *args, **kwargs)

        def run(rgb):
            static_in.copy_(rgb)
            g.replay()
            return static_out
        run.graph = g
        return run

    def pipelined(self, depth=3, graphs=False):
        """Throughput mode for a STREAM of batches (test.py's loader loop, serving): `run = net.pipelined(2)`, then
        `pending = run(rgb)` enqueues a complete forward — equi2pers, network, blend — on stream k % depth with a private
        execution context and returns at once; `pending.get()` makes the current stream wait for it and returns the output.
        With two forwards in flight one batch's HBM-bound decoder runs beside the next batch's matrix-bound encoder and every
        kernel works on the whole batch (M = B*N patches) instead of a half-batch lane: +10 % panoramas/s at 8 per GPU.
        Results are the bits of a plain call.  graphs=True replays one captured hipGraph per slot instead of enqueueing the ~135 launches
        of a forward from Python: below ~4 panoramas per forward the host is the limit (one panorama per forward: 1170 -> see DESIGN 5b)."""
        return _Pipelined(self, depth, graphs)

    def _check(self, rgb):
        if self.training:
            raise NotImplementedError("spherical_fusion is inference-only (eval-mode BatchNorm folded into the weights): call .eval()")
        self._eng.check_input(rgb)
        if self.__dict__.get("_is_replica", False) and self.__dict__.get("_origin") is not None:
            if self._eng.device != rgb.device:
                raise RuntimeError("a DataParallel replica must run inside _execution()")
            return                                                         # bound to its device's context by _execution()
        self._sync_packed(rgb.device)

    @torch.no_grad()
    def forward(self, rgb, confidence=True):
        with self._execution(rgb):
            return self._forward(rgb, confidence)

    def _forward(self, rgb, confidence):
        self._check(rgb)
        e = self._eng
        bs, _, H, W = rgb.shape
        with torch.cuda.device(rgb.device):
            patches = equi2pers_patches(rgb, self.fov, self.nrows, self.patch_size, layout=_lib.LAYOUT_BNCHW)   # :243
            self._input_read = torch.cuda.current_stream(rgb.device).record_event() if self._want_input_event else None
            a, c = self.network(patches, bs, confidence)                                                        # :245-306
            return e.blend(a, c, (H, W))                                                                        # :307-313

    def network(self, patches, bs, confidence, point_feat=None):
        """planar patches [bs,N,3,P,P] -> (pred * conf, conf) planes [bs,N,1,P,P] (the part of forward between the two resamplers)"""
        e = self._eng
        if self._dirty or e.w is None:
            self._sync_packed(patches.device)
        pf = e.w["point_feat"] if point_feat is None else point_feat
        if bs < 2 * self.LANES or self.LANES < 2:
            return e.network(patches, pf, bs, confidence)
        return self._network_lanes(patches, pf, bs, confidence)

    def _network_lanes(self, patches, pf, bs, confidence):
        e = self._eng
        if self._lanes is None:                                            # reset by _sync_packed whenever the weights were repacked
            # the other lanes' streams must sit on other hardware queues than THIS stream (a fresh torch.cuda.Stream may share its queue: the lanes then
            # run one after the other — round 5 met a process whose forwards took 4.4 instead of 2.5 ms that way); measured, once per packing
            cur0 = torch.cuda.current_stream(patches.device)
            if torch.cuda.is_current_stream_capturing():
                side = [torch.cuda.Stream(device=patches.device) for _ in range(self.LANES - 1)]
            else:
                side = _concurrent_streams(self.LANES, patches.device, first=cur0)[1:]
            self._lanes = [(e, None)] + [(e.lane(), st) for st in side]
        N, P = self.npatches, e.patch_size[0]
        a = torch.empty((bs, N, 1, P, P), dtype=torch.float32, device=patches.device)
        c = torch.empty_like(a) if confidence else None
        cur = torch.cuda.current_stream(patches.device)
        fork = cur.record_event()
        per = (bs + self.LANES - 1) // self.LANES
        per_item = pf.shape[0] == bs * N                                   # iterative model: one feature map per (panorama, patch)
        joins = []
        for k, (eng, stream) in enumerate(self._lanes):
            lo, hi = k * per, min(bs, (k + 1) * per)
            if lo >= hi:
                break
            out = (a[lo:hi], c[lo:hi] if confidence else None)
            pfk = pf[lo * N:hi * N] if per_item else pf
            if stream is None:
                eng.network(patches[lo:hi], pfk, hi - lo, confidence, out=out)
            else:
                stream.wait_event(fork)
                with torch.cuda.stream(stream):
                    eng.network(patches[lo:hi], pfk, hi - lo, confidence, out=out)
                    joins.append(stream.record_event())
        for ev in joins:
            cur.wait_event(ev)
        return a, c
