"""Host input pipeline on the device side of the PCIe link — replaces the per-pixel CPU work of
/root/reference/dataset_loader_stanford.py:42-109 (decoded frame -> cv2.resize INTER_AREA -> /255 -> CHW float32; 16-bit depth ->
metres -> validity mask) and the `rgb.cuda()` of test.py:196.

    rgb   = preprocess_rgb(frames_u8, (512, 1024))               # [B,Hs,Ws,3] uint8 BGR on the GPU -> [B,3,512,1024] float32
    d, m  = preprocess_depth(frames_u16, (512, 1024))            # [B,Hs,Ws] uint16 -> depth [B,1,H,W] float32 (masked), mask uint8

    feeder = DeviceFeeder(batches, (512, 1024))                  # iterable of host uint8 arrays [B,Hs,Ws,3] (decoded by the loader's workers)
    for rgb in feeder:                                           # rgb: device float32 [B,3,H,W], ready on the CURRENT stream
        depth = net(rgb)

What crosses PCIe is the DECODED uint8 frame (1.5 MB per 512x1024 panorama instead of the reference's 6.3 MB of float32: 4.3 GB/s
instead of 17 GB/s at 2 750 panoramas/s).  `DeviceFeeder` keeps `depth` (default 3) pinned staging buffers and device frame buffers
in rotation: the H2D copy of batch k+1 and its preprocess kernel run on a side stream while batch k is in the network; the consumer
stream only waits on an event.  Decoding PNG/EXR files stays with the loader's CPU workers (out of scope: no image codec is part of
the hot path); everything after the decoded frame is on the device.

Training input (the loaders' `Dataset(rotate=True, flip=True, gamma=..., permute_color=...)`, dataset_loader_stanford.py:57-73,
dataset_loader_360d.py:54-71) comes from the same decoded frames, the augmentation folded into the preprocess pass (csrc/omni_augment.hip):

    aug   = draw_augmentation(B, 1024, flip=True, rotate=True, gamma=True)   # the loaders' own draws, item by item: an `Augmentation` (host)
    rgb   = augment_rgb(frames_u8, (512, 1024), aug)             # = preprocess_rgb, then flip / roll / perm / gamma per item — one kernel
    d, m  = augment_depth(frames_u16, (512, 1024), aug)          # = preprocess_depth through the same column map
    lab   = augment(labels_i64, aug)                             # tensors already on the device: [B,C,H,W] of 1/2/4/8-byte elements
    pred  = augment(net(rgb), aug, inverse=True)                 # a prediction back onto the original panorama

    for rgb, depth, mask, aug in TrainFeeder(batches, (512, 1024), flip=True, rotate=True, gamma=False, permute_color=True):
        ...                                                      # batches: (uint8 [B,Hs,Ws,3], uint16 [B,Hs,Ws]) host arrays

The per-item parameters reach the kernels as a table in DEVICE memory (`Augmentation.to(device)`: int32 [B,5] + float32 [B]); in the
feeder it travels in the frames' pinned slot.  Nothing is read back, the calls are capturable, a replayed graph reads the table's
current contents.
"""
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import ptr as _p


def _hw(size):
    return (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))


def preprocess_rgb(frames_u8, size, out=None):
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
        raise ValueError("frames must be a uint8 tensor on an MI355X device; there is no CPU path")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("expected decoded frames [B,Hs,Ws,3] uint8 (BGR, as cv2.imread returns them)")
    H, W = _hw(size)
    f = frames_u8.contiguous()
    B, Hs, Ws, _ = f.shape
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=f.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != f.device or tuple(out.shape) != (B, 3, H, W)
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor [{B},3,{H},{W}] on {f.device} (the kernel writes through its raw pointer)")
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().omni_preprocess_rgb_u8(_p(f), _p(out), B, Hs, Ws, H, W, _lib.stream_of(f)), "preprocess_rgb")
    return out


def preprocess_depth(frames_u16, size, min_depth=0.1, max_depth=8.0):
    if not isinstance(frames_u16, torch.Tensor) or not frames_u16.is_cuda:
        raise ValueError("frames must be a tensor on an MI355X device; there is no CPU path")
    if frames_u16.dtype not in (torch.uint16, torch.int16) or frames_u16.dim() != 3:
        raise ValueError("expected 16-bit depth frames [B,Hs,Ws] (uint16; int16 storage is reinterpreted)")
    H, W = _hw(size)
    f = frames_u16.contiguous()
    B, Hs, Ws = f.shape
    depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=f.device)
    mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=f.device)
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().omni_preprocess_depth_u16(_p(f), _p(depth), _p(mask), B, Hs, Ws, H, W, min_depth, max_depth,
                                                        _lib.stream_of(f)), "preprocess_depth")
    return depth, mask


def _rotation(batches, depth, stage, hand_over):
    """The slot rotation of the feeders: batch k is staged into slot k % depth (`stage(slot, batch)`: pinned copy + asynchronous H2D on the
    side stream) and handed to the consumer (`hand_over(slot)`) once depth-1 batches are in flight ahead of it."""
    pending = []
    k = 0
    for frames in batches:
        stage(k % depth, frames)
        pending.append(k % depth)
        k += 1
        if len(pending) >= depth - 1:                                  # keep depth-1 batches in flight ahead of the consumer
            yield hand_over(pending.pop(0))
    while pending:
        yield hand_over(pending.pop(0))


class DeviceFeeder:
    """Pinned, multi-buffered host -> device staging of decoded frames on a copy stream; /255 + HWC->CHW on the consumer's stream.

    The yielded tensor is a reusable float32 buffer: it is valid until the next batch is requested (stream order on the
    consumer's current stream guarantees that the previous forward has read it before it is overwritten) — clone it to keep it.
    Device footprint: `depth` uint8 frames + one float32 batch (the 256 MB Infinity Cache also holds the network's weights and
    activations: a float32 buffer per slot measurably slows the forward down).

    A consumer that reads the batch on ANOTHER stream (`spherical_fusion.pipelined`) asks for `out_buffers=2` and reports when the
    batch has been read: `feeder.done_with(rgb, pending.input_read)` (the event after equi2pers, the forward's only reader of
    the panoramas) — the buffer is rewritten only after that event."""

    def __init__(self, batches, size, device=None, depth=3, out_buffers=1):
        self.batches, self.size, self.depth = batches, _hw(size), max(2, int(depth))
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.side = torch.cuda.Stream(device=self.device)
        self._slots = None
        self._outs, self._done, self._k, self._nout = None, None, 0, max(1, int(out_buffers))

    def done_with(self, rgb, event):
        """`rgb` (a tensor this feeder yielded) is read by work on another stream that `event` marks the end of"""
        for j, o in enumerate(self._outs):
            if o.data_ptr() == rgb.data_ptr():
                self._done[j] = event
                return
        raise ValueError("not a batch of this feeder")

    def _alloc(self, shape):
        B, Hs, Ws, _ = shape
        H, W = self.size
        self._slots = [{"pin": None, "dev": torch.empty(shape, dtype=torch.uint8, device=self.device),
                        "ready": torch.cuda.Event(), "free": None} for _ in range(self.depth)]
        self._outs = [torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device) for _ in range(self._nout)]
        self._done = [None] * self._nout
        # the frames come from the CURRENT stream's allocator pool and are written on the side stream: a block that work still queued on the
        # current stream writes to (a forward's freed intermediates: the host runs a whole forward ahead) must not take the first copy early
        self.side.wait_stream(torch.cuda.current_stream(self.device))

    def _stage(self, slot, frames):
        s = self._slots[slot]
        if isinstance(frames, torch.Tensor) and frames.is_pinned():
            # a DataLoader(pin_memory=True) batch: already page-locked, copied to the device straight from where the worker put it
            if frames.dtype != torch.uint8 or frames.dim() != 4 or tuple(frames.shape[1:]) != tuple(s["dev"].shape[1:]) or frames.shape[0] > s["dev"].shape[0]:
                raise ValueError("pinned batches must be uint8 [B' <= B,Hs,Ws,3] of one frame size")
            src = frames
        else:
            a = np.ascontiguousarray(frames.numpy() if isinstance(frames, torch.Tensor) else frames)
            if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
                raise ValueError("batches must yield uint8 arrays [B,Hs,Ws,3]")
            if tuple(s["dev"].shape[1:]) != a.shape[1:] or a.shape[0] > s["dev"].shape[0]:
                raise ValueError("all batches of one feeder must have the same frame size and at most the first batch's length")
            if s["pin"] is None:
                s["pin"] = torch.empty(tuple(s["dev"].shape), dtype=torch.uint8).pin_memory()
            if s["free"] is not None:
                s["free"].synchronize()                                # (the previous H2D out of this pinned buffer has been consumed)
            s["pin"].numpy()[:a.shape[0]] = a                          # host memcpy into pinned memory (the worker's hand-over)
            src = s["pin"][:a.shape[0]]
        if s["free"] is not None:
            # the consumer's preprocess has read this slot's device frame — waited for on the HOST (the event is `depth` batches old: it returns at
            # once): a stream-side wait in front of the asynchronous copy makes the runtime hold the copy back (round 5, tools/feed_ab.py: 3593-3893
            # panoramas/s, jittery, with 4 hardware queues and 2650 with 8, against 3904-3966 this way; the GPU-side cost of feeding is 1 %)
            s["free"].synchronize()
        with torch.cuda.stream(self.side):
            s["dev"][:src.shape[0]].copy_(src, non_blocking=True)      # async H2D on the side stream
            s["ready"].record(self.side)
            if src is frames and hasattr(self.batches, "recycle"):     # a producer with a buffer ring (png.PngBatches): the page-locked
                ev = torch.cuda.Event(); ev.record(self.side)          # batch may be decoded into again once this copy has run
                self.batches.recycle(frames, ev)
        s["src"] = src                                                 # keep the host buffer alive until the copy has been ordered
        s["n"] = int(src.shape[0])                                     # (a DataLoader with drop_last=False ends on a shorter batch)

    def __iter__(self):
        def stage(slot, frames):
            if self._slots is None:
                self._alloc(tuple(frames.shape))
            self._stage(slot, frames)
        return _rotation(self.batches, self.depth, stage, self._hand_over)

    def _hand_over(self, slot):
        s = self._slots[slot]
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(s["ready"])                                     # no host synchronisation
        j = self._k % self._nout
        self._k += 1
        if self._done[j] is not None:
            cur.wait_event(self._done[j])                              # a consumer on another stream has finished with this buffer
            self._done[j] = None
        n = s.get("n", s["dev"].shape[0])
        out = self._outs[j][:n]
        preprocess_rgb(s["dev"][:n], self.size, out=out)               # 35 us at 8 x 512x1024; behind the previous forward in stream order
        ev = torch.cuda.Event(); ev.record(cur); s["free"] = ev        # the slot's device frame may be overwritten after this point
        return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Training-time augmentation (csrc/omni_augment.hip): flip, yaw roll, gamma and colour permutation inside the preprocess pass
class Augmentation:
    """Per-item augmentation parameters on the HOST: `flip` [B] (non-zero = mirrored), `dx` [B] (columns rolled to the right, any
    integer: the kernels reduce it modulo W), `perm` [B,3] (out[c] = in[perm[c]], loader channel order) and `gamma` [B] (exponent, > 0;
    1 = none).  `to(device)` packs them into what the kernels read."""

    def __init__(self, flip, dx, perm, gamma=None):
        def ints(v, what):
            t = torch.as_tensor(v)
            if t.device.type != "cpu":
                raise ValueError(f"{what} must be a host tensor (Augmentation.to(device) makes the device table)")
            if t.dtype.is_floating_point or t.dtype.is_complex:
                raise ValueError(f"{what} must hold integers, not {t.dtype}")
            return t.to(torch.int64)
        self.flip, self.dx, self.perm = ints(flip, "flip"), ints(dx, "dx"), ints(perm, "perm")
        B = self.dx.shape[0] if self.dx.dim() == 1 else -1
        g = torch.ones(max(B, 0), dtype=torch.float32) if gamma is None else torch.as_tensor(gamma)
        if g.device.type != "cpu":
            raise ValueError("gamma must be a host tensor (Augmentation.to(device) makes the device table)")
        self.gamma = g.to(torch.float32)
        if B < 0 or tuple(self.flip.shape) != (B,) or tuple(self.perm.shape) != (B, 3) or tuple(self.gamma.shape) != (B,):
            raise ValueError(f"expected flip [B], dx [B], perm [B,3], gamma [B] of one length; got {tuple(self.flip.shape)}, "
                             f"{tuple(self.dx.shape)}, {tuple(self.perm.shape)}, {tuple(self.gamma.shape)}")
        if B and not bool((self.perm.sort(dim=1).values == torch.arange(3)).all()):
            raise ValueError("every row of perm must be a permutation of 0, 1, 2")
        if B and not bool((self.gamma > 0).all() & torch.isfinite(self.gamma).all()):
            raise ValueError("gamma must be finite and > 0")
        if B and int(self.dx.abs().max()) >= 2 ** 31:
            raise ValueError("dx must fit 32 bits")

    def __len__(self):
        return int(self.dx.shape[0])

    def __repr__(self):
        return (f"Augmentation(flip={self.flip.tolist()}, dx={self.dx.tolist()}, perm={self.perm.tolist()}, "
                f"gamma={self.gamma.tolist()})")

    @classmethod
    def identity(cls, B):
        B = int(B)
        return cls(torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.arange(3).repeat(B, 1))

    def pack(self):
        """(int32 [B,5] = flip, dx, perm0, perm1, perm2; float32 [B]) on the host"""
        table = torch.cat([(self.flip != 0).to(torch.int64)[:, None], self.dx[:, None], self.perm], dim=1).to(torch.int32)
        return table.contiguous(), self.gamma.contiguous()

    def to(self, device):
        table, gamma = self.pack()
        return DeviceAugmentation(table.to(device), gamma.to(device), host=self)


class DeviceAugmentation:
    """What the kernels read: `table` int32 [B,5] and `gamma` float32 [B] (or None: no gamma) on one device.  The contents may be
    rewritten in place — also between replays of a captured graph; `host` is the `Augmentation` they were packed from, if any."""
    __slots__ = ("table", "gamma", "host")

    def __init__(self, table, gamma=None, host=None):
        if not isinstance(table, torch.Tensor) or not table.is_cuda or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 5 \
                or not table.is_contiguous():
            raise ValueError("table must be a contiguous int32 tensor [B,5] on an MI355X device")
        if gamma is not None and (not isinstance(gamma, torch.Tensor) or gamma.device != table.device or gamma.dtype != torch.float32
                                  or tuple(gamma.shape) != (table.shape[0],) or not gamma.is_contiguous()):
            raise ValueError(f"gamma must be a contiguous float32 tensor [{table.shape[0]}] on {table.device}")
        self.table, self.gamma, self.host = table, gamma, host

    def __len__(self):
        return int(self.table.shape[0])

    @property
    def device(self):
        return self.table.device


def draw_augmentation(B, width, *, flip=False, rotate=False, gamma=False, permute_color=False, generator=None, np_random=None):
    """The reference loaders' own random draws (dataset_loader_stanford.py:57-73, dataset_loader_360d.py:54-71), item by item, in
    their order: flip coin, roll, gamma (exponent, then coin), permutation (coin, then numpy's permutation).  Only the enabled stages
    draw.  `generator`: a torch.Generator (default: torch's global one); `np_random`: a numpy RandomState / Generator (default: numpy's
    global state) — with the seeds a loader worker would have, the parameters are the loader's."""
    B, W = int(B), int(width)
    if rotate and W < 4:
        raise ValueError("rotate needs width >= 4 (the roll is a multiple of width // 4; the reference divides by zero there)")
    rs = np.random if np_random is None else np_random
    f, d = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
    p, g = torch.arange(3).repeat(B, 1), torch.ones(B, dtype=torch.float32)
    coin = lambda n: torch.randint(n, size=(1,), generator=generator)[0].item()
    for i in range(B):
        if flip:
            f[i] = int(coin(2) == 0)
        if rotate:
            dx = coin(W)
            d[i] = dx // (W // 4) * (W // 4)
        if gamma:
            e = (torch.rand((1,), generator=generator) + 1).numpy()[0]            # float32 in [1, 2)
            if coin(2) == 0:                                                      # the assignment sits inside the `if`: coin 1 = nothing
                g[i] = float(np.float32(1) / e)
        if permute_color:
            if coin(4) == 0:
                p[i] = torch.from_numpy(np.asarray(rs.permutation(3)).astype(np.int64))
    return Augmentation(f, d, p, g)


def _device_aug(aug, B, device):
    if isinstance(aug, Augmentation):
        aug = aug.to(device)
    if not isinstance(aug, DeviceAugmentation):
        raise ValueError("aug must be an Augmentation or what its .to(device) returns")
    if len(aug) != B or aug.device != device:
        raise ValueError(f"aug must hold {B} items on {device} (it holds {len(aug)} on {aug.device})")
    return aug


def augment_rgb(frames_u8, size, aug, out=None):
    """`preprocess_rgb` with the augmentation folded in: [B,Hs,Ws,3] uint8 -> [B,3,H,W] float32, one pass."""
    if not isinstance(frames_u8, torch.Tensor) or not frames_u8.is_cuda:
        raise ValueError("frames must be a uint8 tensor on an MI355X device; there is no CPU path")
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError("expected decoded frames [B,Hs,Ws,3] uint8 (BGR, as cv2.imread returns them)")
    H, W = _hw(size)
    f = frames_u8.contiguous()
    B, Hs, Ws, _ = f.shape
    a = _device_aug(aug, B, f.device)
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=f.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != f.device or tuple(out.shape) != (B, 3, H, W)
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 tensor [{B},3,{H},{W}] on {f.device} (the kernel writes through its raw pointer)")
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().omni_augment_rgb_u8(_p(f), _p(out), _p(a.table), _p(a.gamma), B, Hs, Ws, H, W, _lib.stream_of(f)), "augment_rgb")
    return out


def augment_depth(frames_u16, size, aug, min_depth=0.1, max_depth=8.0, out=None):
    """`preprocess_depth` through the augmentation's column map: depth [B,1,H,W] float32 (masked) and mask uint8.
    `out`: a (depth, mask) pair of contiguous tensors to write into."""
    if not isinstance(frames_u16, torch.Tensor) or not frames_u16.is_cuda:
        raise ValueError("frames must be a tensor on an MI355X device; there is no CPU path")
    if frames_u16.dtype not in (torch.uint16, torch.int16) or frames_u16.dim() != 3:
        raise ValueError("expected 16-bit depth frames [B,Hs,Ws] (uint16; int16 storage is reinterpreted)")
    H, W = _hw(size)
    f = frames_u16.contiguous()
    B, Hs, Ws = f.shape
    a = _device_aug(aug, B, f.device)
    if out is None:
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=f.device)
        mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=f.device)
    else:
        depth, mask = out
        for t, dt in ((depth, torch.float32), (mask, torch.uint8)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != f.device or tuple(t.shape) != (B, 1, H, W) or not t.is_contiguous():
                raise ValueError(f"out must be contiguous (float32, uint8) tensors [{B},1,{H},{W}] on {f.device}")
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().omni_augment_depth_u16(_p(f), _p(depth), _p(mask), _p(a.table), B, Hs, Ws, H, W, min_depth, max_depth,
                                                     _lib.stream_of(f)), "augment_depth")
    return depth, mask


def augment(x, aug, color=False, inverse=False, out=None):
    """The augmentation's index map on a tensor that already lives on the device: [B,C,H,W] (or [B,H,W]) of 1-, 2-, 4- or 8-byte
    elements (float32 depth or images, int64 label maps, uint8 masks), copied as bytes.  color=True (C == 3) also applies the channel
    permutation and, on float32, gamma.  inverse=True applies the inverse column map and no colour: a prediction made on an augmented
    batch lands back on the original panorama (flip / roll test-time averaging)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("x must be a tensor on an MI355X device; there is no CPU path")
    if x.dim() not in (3, 4) or x.element_size() not in (1, 2, 4, 8) or x.dtype.is_complex:
        raise ValueError("expected [B,C,H,W] or [B,H,W] of 1-, 2-, 4- or 8-byte real elements")
    f = x.contiguous()
    B, C, H, W = (f.shape[0], 1, f.shape[1], f.shape[2]) if f.dim() == 3 else f.shape
    if H < 1 or W < 1 or C < 1:
        raise ValueError("expected [B,C,H,W] or [B,H,W] with C, H, W >= 1")
    a = _device_aug(aug, B, f.device)
    color = bool(color) and not inverse
    if color and C != 3:
        raise ValueError(f"color=True needs three channels, got {C}")
    gamma = None
    if color and a.gamma is not None:
        if f.dtype == torch.float32:
            gamma = a.gamma
        elif a.host is None or bool((a.host.gamma != 1).any()):
            raise ValueError(f"gamma needs a float32 tensor, got {f.dtype}")
    if out is None:
        out = torch.empty_like(f)
    elif not isinstance(out, torch.Tensor) or out.dtype != f.dtype or out.device != f.device or out.shape != f.shape or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {f.dtype} tensor {tuple(f.shape)} on {f.device}")
    with torch.cuda.device(f.device):
        _lib.check(_lib.load().omni_augment_planes(_p(f), _p(out), f.element_size(), _p(a.table),
                                                  _p(gamma), B, C, H, W, int(color), int(bool(inverse)),
                                                  _lib.stream_of(f)), "augment")
    return out


class TrainBatch(NamedTuple):
    rgb: torch.Tensor        # [B,3,H,W] float32
    depth: torch.Tensor      # [B,1,H,W] float32, masked
    mask: torch.Tensor       # [B,1,H,W] uint8
    aug: DeviceAugmentation  # the batch's table on the device; .host: the drawn Augmentation


class TrainFeeder:
    """The reference's training batches from decoded frames: `batches` yields (frames_u8 [B,Hs,Ws,3], frames_u16 [B,Hs,Ws]) host arrays;
    every batch draws its augmentation (`draw_augmentation`, width = the network's width: the loader augments after its resize) and the
    feeder yields TrainBatch(rgb, depth, mask, aug) on the CURRENT stream.

    Staging is `DeviceFeeder`'s: `depth` slots in rotation, each ONE pinned buffer (frames, depth frames and the parameter table side by
    side) and its device twin, one asynchronous H2D copy per batch on a side stream, a host-side wait on the slot's `free` event only (it
    is `depth` batches old), no host synchronisation in the steady state.  The yielded tensors are reusable buffers, valid until the next
    batch is requested — clone to keep.  A last batch shorter than the first is handled."""

    def __init__(self, batches, size, *, flip, rotate, gamma, permute_color, device=None, depth=3, generator=None, np_random=None,
                 min_depth=0.1, max_depth=8.0):
        self.batches, self.size, self.depth = batches, _hw(size), max(2, int(depth))
        self.flags = dict(flip=bool(flip), rotate=bool(rotate), gamma=bool(gamma), permute_color=bool(permute_color))
        self.generator, self.np_random = generator, np_random
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.side = torch.cuda.Stream(device=self.device)
        self._slots = None

    def _alloc(self, shape):
        B, Hs, Ws, _ = shape
        H, W = self.size
        up = lambda n: (n + 15) // 16 * 16
        self._shape = (B, Hs, Ws)
        self._o16 = up(B * Hs * Ws * 3)                                # [rgb frames | depth frames | table int32 [B,5] | gamma float32 [B]]
        self._otab = self._o16 + up(B * Hs * Ws * 2)
        self._ogam = self._otab + up(B * 20)
        total = self._ogam + up(B * 4)
        self._slots = [{"pin": torch.empty(total, dtype=torch.uint8).pin_memory(), "dev": torch.empty(total, dtype=torch.uint8, device=self.device),
                        "ready": torch.cuda.Event(), "free": None} for _ in range(self.depth)]
        self._rgb = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        self._depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        self._mask = torch.empty((B, 1, H, W), dtype=torch.uint8, device=self.device)
        self._par = torch.empty(total - self._otab, dtype=torch.uint8, device=self.device)
        self.side.wait_stream(torch.cuda.current_stream(self.device))  # (as DeviceFeeder._alloc: the buffers come from the current stream's pool)

    def _views(self, buf, n):
        B, Hs, Ws = self._shape
        return (buf[:n * Hs * Ws * 3].view(n, Hs, Ws, 3), buf[self._o16:self._o16 + n * Hs * Ws * 2].view(torch.int16).view(n, Hs, Ws),
                buf[self._otab:self._otab + n * 20].view(torch.int32).view(n, 5), buf[self._ogam:self._ogam + n * 4].view(torch.float32))

    def _stage(self, slot, batch):
        rgb, d16 = batch
        rgb = np.ascontiguousarray(rgb.numpy() if isinstance(rgb, torch.Tensor) else rgb)
        d16 = np.ascontiguousarray(d16.numpy() if isinstance(d16, torch.Tensor) else d16)
        if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[3] != 3:
            raise ValueError("batches must yield uint8 arrays [B,Hs,Ws,3]")
        if d16.dtype not in (np.uint16, np.int16) or d16.shape != rgb.shape[:3]:
            raise ValueError("batches must yield 16-bit depth arrays [B,Hs,Ws] of the frames' size")
        if self._slots is None:
            self._alloc(rgb.shape)
        n = rgb.shape[0]
        if rgb.shape[1:3] != self._shape[1:] or n > self._shape[0] or n < 1:
            raise ValueError("all batches of one feeder must have the same frame size and at most the first batch's length")
        aug = draw_augmentation(n, self.size[1], generator=self.generator, np_random=self.np_random, **self.flags)
        table, gam = aug.pack()
        s = self._slots[slot]
        if s["free"] is not None:
            s["free"].synchronize()                                    # (host-side, `depth` batches old: see DeviceFeeder._stage)
        pr, pd, pt, pg = self._views(s["pin"], n)
        pr.numpy()[...] = rgb                                          # host memcpy into pinned memory (the worker's hand-over)
        pd.numpy()[...] = d16.view(np.int16)
        pt.copy_(table); pg.copy_(gam)                                 # the parameter table travels with the frames
        with torch.cuda.stream(self.side):
            s["dev"].copy_(s["pin"], non_blocking=True)                # ONE async H2D per batch (a short batch copies the slot's stale tail too)
            s["ready"].record(self.side)
        s["n"], s["aug"] = n, aug

    def __iter__(self):
        return _rotation(self.batches, self.depth, self._stage, self._hand_over)

    def _hand_over(self, slot):
        s = self._slots[slot]
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(s["ready"])                                     # no host synchronisation
        n = s["n"]
        fr, fd, _, _ = self._views(s["dev"], n)
        # the table leaves the slot with the batch (one small copy in stream order): the consumer may still read it — the inverse map of a
        # prediction — when the side stream refills the slot, which only waits for the kernels below
        self._par.copy_(s["dev"][self._otab:], non_blocking=True)
        k = self._ogam - self._otab
        a = DeviceAugmentation(self._par[:n * 20].view(torch.int32).view(n, 5), self._par[k:k + n * 4].view(torch.float32), host=s["aug"])
        rgb = augment_rgb(fr, self.size, a, out=self._rgb[:n])
        depth, mask = augment_depth(fd, self.size, a, self.min_depth, self.max_depth, out=(self._depth[:n], self._mask[:n]))
        ev = torch.cuda.Event(); ev.record(cur); s["free"] = ev        # the slot may be overwritten after this point
        return TrainBatch(rgb, depth, mask, a)
