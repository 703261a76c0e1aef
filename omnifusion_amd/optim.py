"""AdamW on the device over one flat arena, with the gradient norm and the clip of `clip_grad_norm_` (csrc/omni_optim.hip).

    opt = AdamW(net.parameters(), lr=1e-4, max_grad_norm=0.5)       # replaces optim.AdamW + clip_grad_norm_(net.parameters(), 0.5)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2)   # a torch.optim.Optimizer: the schedulers attach
    loss.backward(); opt.step(); opt.zero_grad()
    opt.grad_norm, opt.skipped_steps, opt.step_count                # device tensors: the fp32 norm before clipping, int64, int64

A step is three launches whatever the number of tensors: one double of g . g per chunk, one block that adds them in a fixed order and
writes the step record (norm, clip factor, per-group decay / step size / bias correction), one update kernel.  Everything that changes from
step to step — the clip factor, the step count, the learning rates — is read from device memory, nothing is read back and nothing
synchronises, so `step()` can be captured in a graph (flat_grads=True) and a replay follows `param_groups[i]['lr']` through the group table.

CONSTRUCTION RE-POINTS `p.data`: every parameter is copied into one fp32 arena (a segment per tensor, each at a multiple of 64 floats) and
`p.data` becomes an as_strided view of it — the same Parameter objects, values, shapes and strides (a channels-last weight stays
channels-last), so modules, `ops.convert` and state-dict keys are unaffected; a tensor that aliased the old storage no longer follows the
parameter.  `exp_avg` and `exp_avg_sq` are two more arenas of the same layout; `state[p]` holds views of them.

Gradients, two modes:
  flat_grads=False  `step()` reads each `p.grad`'s address into the segment table (uploaded when an address changed: pinned slots, no
                    synchronisation).  A parameter without a gradient is skipped, as torch skips it.  A gradient is fp32, on the device,
                    with its parameter's strides, at any 4-byte alignment.  Not capturable (the addresses are read on the host).
  flat_grads=True   every `p.grad` is a view of ONE gradient arena; autograd accumulates into the views in place.  `zero_grad()` is one
                    `zero_()` of the arena and keeps the views — `set_to_none` is ignored — and every parameter steps on every call (a
                    parameter the loss does not reach has a zero gradient: its moments decay and weight decay applies, where torch would
                    leave it alone).  `step()` is capturable; `sync_gradients()` is one all_reduce of the arena.

Differences from `clip_grad_norm_` + `torch.optim.AdamW`: the clip factor multiplies the gradient inside the update, `p.grad`
keeps its unclipped bits; there is ONE step count for all parameters (torch keeps one per parameter, which differs only for a parameter
that had no gradient in some steps); skip_nonfinite=True leaves parameters, moments and the step count untouched when the norm is inf or
NaN and counts the step in `skipped_steps`.  amsgrad, maximize, fp16 / bf16 state and a CPU path do not exist.

`state_dict()` / `load_state_dict()` speak torch.optim.AdamW's format (state[i] = {step, exp_avg, exp_avg_sq}, the same param_groups
keys; max_grad_norm, skip_nonfinite and flat_grads travel in param_groups as extra keys, which torch's loader carries along), so a
checkpoint of either loads into the other.  `state_dict()` reads the step count back (one synchronisation)."""
import torch

from . import _lib, dist as _dist, ops

CHUNK = 4096           # elements per chunk: csrc/omni_optim.hip, OPT_CHUNK
ALIGN = 64             # floats: every segment starts at a multiple
_DEPTH = 4             # pinned staging copies of a table in rotation


def layout(sizes, chunk=CHUNK, align=ALIGN):
    """The arena's layout from the tensors' element counts -> (offsets, total, chunks): segment i occupies [offsets[i], offsets[i] + sizes[i])
    of an arena of `total` floats, every offset a multiple of `align`; `chunks` lists (segment, offset within the segment) of at most `chunk`
    elements each, segment by segment, so that the chunks cover every element exactly once, none straddles two segments and none touches
    the padding.  A pure function of the sizes."""
    offsets, chunks, off = [], [], 0
    for i, n in enumerate(sizes):
        n = int(n)
        if n < 0 or n >= 2 ** 31:
            raise ValueError(f"layout: tensor {i} has {n} elements (0 .. 2^31 - 1)")
        offsets.append(off)
        chunks.extend((i, o) for o in range(0, n, chunk))
        off += -(-n // align) * align
    return offsets, off, chunks


def _dense(t):
    """non-overlapping and dense in some stride order"""
    want = 1
    for stride, size in sorted(zip(t.stride(), t.size())):
        if size == 1:
            continue
        if stride != want:
            return False
        want *= size
    return True


def _same_strides(g, p):
    return g.stride() == p.stride() or all(a == b for a, b, n in zip(g.stride(), p.stride(), p.size()) if n > 1)


class _Table:
    """A small table in device memory with `_DEPTH` pinned host copies in rotation: upload() writes the next pinned copy and starts an
    asynchronous copy on the current stream.  A pinned copy is reused only after the copy out of it has finished — an event wait that in
    practice never waits, so nothing synchronises with the device."""

    def __init__(self, host, device):
        self.dev = torch.empty(host.shape, dtype=host.dtype, device=device)
        self.pins = [torch.empty(host.shape, dtype=host.dtype).pin_memory() for _ in range(_DEPTH)]
        self.events = [None] * _DEPTH
        self.k = 0
        self.upload(host)

    def upload(self, host):
        i = self.k % _DEPTH
        self.k += 1
        if self.events[i] is not None:
            self.events[i].synchronize()
        self.pins[i].copy_(host)
        self.dev.copy_(self.pins[i], non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record()


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's update (decoupled weight decay) on hand-written kernels; see the module's docstring.  `params`: an iterable of
    parameters or of group dicts with their own lr / betas / eps / weight_decay.  max_grad_norm: the max_norm of clip_grad_norm_ (2-norm
    over all gradients), None: no clipping.  Construction re-points `p.data` into the arena."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False, maximize=False,
                 max_grad_norm=None, skip_nonfinite=False, flat_grads=False):
        self._built = False
        if amsgrad or maximize:
            raise ValueError("AdamW: amsgrad and maximize are not built")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"AdamW: max_grad_norm must be None or >= 0 (got {max_grad_norm})")
        # torch.optim.AdamW's own defaults first, so that param_groups carry exactly its keys (whatever this torch version's are)
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        max_grad_norm=None if max_grad_norm is None else float(max_grad_norm), skip_nonfinite=bool(skip_nonfinite),
                        flat_grads=bool(flat_grads))
        super().__init__(params, defaults)                     # (ValueError: a parameter in two groups, an empty list)
        self.max_grad_norm, self.skip_nonfinite, self.flat_grads = defaults["max_grad_norm"], defaults["skip_nonfinite"], defaults["flat_grads"]
        self._params, self._group_of = [], []
        for gi, group in enumerate(self.param_groups):
            self._group_row(group)                             # validates the hyper-parameters
            for p in group["params"]:
                self._params.append(p)
                self._group_of.append(gi)
        if len(self.param_groups) > 256:
            raise ValueError("AdamW: at most 256 parameter groups")
        # every rejection before anything touches the GPU
        for i, p in enumerate(self._params):
            if p.dtype != torch.float32:
                raise ValueError(f"AdamW: parameter {i} is {p.dtype}: fp32 parameters only")
            if not p.is_cuda:
                raise ValueError(f"AdamW: parameter {i} is on {p.device}: parameters live on one MI355X; there is no CPU path")
            if p.device != self._params[0].device:
                raise ValueError(f"AdamW: parameter {i} is on {p.device}, parameter 0 on {self._params[0].device}: one GPU")
            if p.layout != torch.strided or not _dense(p):
                raise ValueError(f"AdamW: parameter {i} (size {tuple(p.shape)}, strides {p.stride()}) is not dense")
        self._device = self._params[0].device
        self._offsets, self._total, chunks = layout([p.numel() for p in self._params])
        if not chunks:
            raise ValueError("AdamW: the parameters have no elements")
        _lib.load()
        with torch.cuda.device(self._device), torch.no_grad():
            self._build(chunks)
        self._built = True

    # ------------------------------------------------------------------------------------------------ construction
    def _group_row(self, group):
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("AdamW: amsgrad and maximize are not built")
        lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        b1, b2 = float(b1), float(b2)
        if not lr >= 0.0 or not eps >= 0.0 or not wd >= 0.0 or not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0:
            raise ValueError(f"AdamW: invalid hyper-parameters lr={lr} betas=({b1}, {b2}) eps={eps} weight_decay={wd}")
        return (lr, b1, b2, eps, wd)

    def _views(self, arena):
        return [torch.as_strided(arena, p.size(), p.stride(), off) for p, off in zip(self._params, self._offsets)]

    def _build(self, chunks):
        dev, n = self._device, self._total
        new = lambda size, dtype=torch.float32: ops._empty((size,), dtype=dtype, device=dev)
        self.params_arena, self.exp_avg, self.exp_avg_sq = new(n).zero_(), new(n).zero_(), new(n).zero_()      # the padding is zero
        self._m_views, self._v_views = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        for p, view in zip(self._params, self._views(self.params_arena)):
            view.copy_(p.data)
            p.data = view
        self.grads_arena = self._g_views = None
        if self.flat_grads:
            self.grads_arena = new(n).zero_()
            self._g_views = self._views(self.grads_arena)
            for p, view in zip(self._params, self._g_views):
                if p.grad is not None:
                    if p.grad.dtype != torch.float32 or p.grad.shape != p.shape:
                        raise ValueError("AdamW: an existing gradient is not its parameter's fp32 shape")
                    view.copy_(p.grad)
                p.grad = view
        nseg = len(self._params)
        self._seg_host = torch.zeros(nseg, 4, dtype=torch.int64)
        self._seg_host[:, 0] = torch.tensor(self._offsets, dtype=torch.int64)
        self._seg_host[:, 1] = torch.tensor([p.numel() for p in self._params], dtype=torch.int64)
        self._seg_host[:, 3] = torch.tensor(self._group_of, dtype=torch.int64)
        self._addrs = [v.data_ptr() for v in self._g_views] if self.flat_grads else [0] * nseg
        self._seg_host[:, 2] = torch.tensor(self._addrs, dtype=torch.int64)
        self._seg = _Table(self._seg_host, dev)
        self._chunks = torch.tensor(chunks, dtype=torch.int32).to(dev)
        self._nchunk = len(chunks)
        self._group_values = [self._group_row(g) for g in self.param_groups]
        self._groups = _Table(torch.tensor(self._group_values, dtype=torch.float64), dev)
        self._partials = new(self._nchunk, torch.float64)
        self._record = new(4 + 8 * len(self.param_groups))
        self._counters = torch.zeros(2, dtype=torch.int64, device=dev)
        self.grad_norm, self.step_count, self.skipped_steps = self._record[0], self._counters[0], self._counters[1]
        self._has_state = [False] * nseg
        # the arguments of the three calls never change: plain integers, no tensor is touched per step
        ptr = lambda t: t.data_ptr()
        self._args_norm = (ptr(self._seg.dev), nseg, ptr(self._chunks), self._nchunk, ptr(self._partials))
        self._args_prep = (ptr(self._partials), self._nchunk, ptr(self._groups.dev), len(self.param_groups),
                           -1.0 if self.max_grad_norm is None else self.max_grad_norm, int(self.skip_nonfinite), ptr(self._record),
                           ptr(self._counters))
        self._args_apply = (ptr(self.params_arena), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self._seg.dev), nseg, ptr(self._chunks),
                            self._nchunk, ptr(self._record), len(self.param_groups))

    def add_param_group(self, param_group):
        if self._built:
            raise ValueError("AdamW: the arena is laid out at construction; parameter groups cannot be added afterwards")
        super().add_param_group(param_group)

    # ------------------------------------------------------------------------------------------------ the step
    def sync_hyperparameters(self):
        """Uploads the group table (lr, betas, eps, weight_decay of every group) where `param_groups` changed since the last upload.
        `step()` calls it; call it yourself before replaying a captured step, which reads the table's current contents."""
        values = [self._group_row(g) for g in self.param_groups]
        if values != self._group_values:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("AdamW: param_groups changed inside a stream capture; call sync_hyperparameters() before capturing")
            with torch.cuda.device(self._device):
                self._groups.upload(torch.tensor(values, dtype=torch.float64))
            self._group_values = values

    def _collect_pointers(self):
        """pointer mode: the gradients' addresses -> the segment table; returns the parameters that step"""
        addrs, stepped = [], []
        for i, p in enumerate(self._params):
            g = p.grad
            if g is None:
                addrs.append(0)
                continue
            if g.dtype != torch.float32 or g.device != self._device or g.layout != torch.strided:
                raise ValueError(f"AdamW: the gradient of parameter {i} must be a dense fp32 tensor on {self._device} (got {g.dtype} on {g.device})")
            if g.shape != p.shape or not _same_strides(g, p):
                raise ValueError(f"AdamW: the gradient of parameter {i} has size {tuple(g.shape)} and strides {g.stride()}, its parameter "
                                 f"{tuple(p.shape)} and {p.stride()}")
            addrs.append(g.data_ptr())
            stepped.append(p)
            if not self._has_state[i]:
                self._init_state(i)
        if addrs != self._addrs:
            self._seg_host[:, 2] = torch.tensor(addrs, dtype=torch.int64)
            self._seg.upload(self._seg_host)
            self._addrs = addrs
        return stepped

    def _check_flat(self):
        """flat mode: every p.grad is still its view of the gradient arena (a gradient set to None gets its view back)"""
        for i, (p, view) in enumerate(zip(self._params, self._g_views)):
            g = p.grad
            if g is not view:
                if g is not None and g.data_ptr() != view.data_ptr():
                    raise ValueError(f"AdamW: flat_grads=True, but the gradient of parameter {i} was replaced by another tensor")
                p.grad = view
            if not self._has_state[i]:
                self._init_state(i)
        return self._params

    def _init_state(self, i):
        self.state[self._params[i]] = {"step": self.step_count, "exp_avg": self._m_views[i], "exp_avg_sq": self._v_views[i]}
        self._has_state[i] = True

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.load()
        with torch.cuda.device(self._device):
            if self.flat_grads:
                stepped = self._check_flat()
            else:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("AdamW: step() reads the gradients' addresses on the host and cannot be captured; use flat_grads=True")
                stepped = self._collect_pointers()
            self.sync_hyperparameters()
            s = torch.cuda.current_stream(self._device).cuda_stream
            _lib.check(L.omni_adamw_grad_sqnorm_f32(*self._args_norm, s), "adamw_grad_sqnorm")
            _lib.check(L.omni_adamw_prepare_f32(*self._args_prep, s), "adamw_prepare")
            _lib.check(L.omni_adamw_apply_f32(*self._args_apply, s), "adamw_apply")
        if stepped:
            torch.autograd.graph.increment_version(stepped)    # a step between a forward and its backward fails in autograd, as torch's does
        return loss

    def zero_grad(self, set_to_none=True):
        """flat_grads=True: one zero_() of the gradient arena; the views stay, `set_to_none` is ignored."""
        if not self.flat_grads:
            return super().zero_grad(set_to_none)
        self.grads_arena.zero_()

    def sync_gradients(self, group=None, average=False):
        """Adds the ranks' gradients in place, between backward() and step().  flat_grads=True: ONE all_reduce(SUM) of the gradient arena, no
        concatenation and no copy back (a gloo group takes dist.sync_gradients' hop through the CPU); otherwise dist.sync_gradients on the
        parameters.  Returns the number of gradients exchanged."""
        if not self.flat_grads:
            return _dist.sync_gradients(self._params, group=group, average=average)
        world = _dist._group_world(group)
        if world == 1:
            return len(self._params)
        dev = _dist._group_device(self._device, group)
        flat = self.grads_arena if dev == self._device else self.grads_arena.to(dev)
        torch.distributed.all_reduce(flat, op=torch.distributed.ReduceOp.SUM, group=group)
        if average:
            flat /= world
        if flat is not self.grads_arena:
            self.grads_arena.copy_(flat)
        return len(self._params)

    # ------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """torch.optim.AdamW's format; `step` is the one step count as a CPU fp32 scalar (read back: one synchronisation), the moments are
        the views of the arenas (torch.save writes each arena once)."""
        sd = super().state_dict()
        step = float(self.step_count.item())
        for entry in sd["state"].values():
            entry["step"] = torch.tensor(step, dtype=torch.float32)
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of torch.optim.AdamW over the same parameters.  The moments are copied into the arenas; a
        parameter without state starts from zero moments; the steps of all entries must agree (there is one step count).  max_grad_norm,
        skip_nonfinite and flat_grads stay as constructed."""
        for group in state_dict["param_groups"]:
            if group.get("amsgrad") or group.get("maximize"):
                raise ValueError("AdamW: amsgrad and maximize are not built")
        super().load_state_dict(state_dict)
        steps = set()
        for i, p in enumerate(self._params):
            entry = self.state.get(p)
            if entry:
                self._m_views[i].copy_(entry["exp_avg"])
                self._v_views[i].copy_(entry["exp_avg_sq"])
                steps.add(int(float(entry["step"])))
                self._has_state[i] = False
                self._init_state(i)
            else:
                self._m_views[i].zero_()
                self._v_views[i].zero_()
                self._has_state[i] = False
                self.state.pop(p, None)
        if len(steps) > 1:
            raise ValueError(f"AdamW: the loaded parameters are at different steps {sorted(steps)}; this optimiser keeps one step count")
        self._counters[0].fill_(steps.pop() if steps else 0)
        for group in self.param_groups:
            group.update(max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite, flat_grads=self.flat_grads)
            for k, v in self.defaults.items():
                group.setdefault(k, v)
        self.sync_hyperparameters()
