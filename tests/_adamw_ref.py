"""The optimiser tests' reference: a float64 restatement of AdamW with clip_grad_norm_'s formula, the segment sizes, the two
parameter groups, seeded parameters, moments and gradients, and torch's own CPU AdamW in float32 and float64, from whose difference the
gate is taken (tests/test_batchnorm_gpu.py's form):

    e32 = max|v32 - v64| / max(1, rms(v64))        torch.optim.AdamW(foreach=False) on the CPU, float32 against float64
    the device must satisfy  err <= 8 . max(e32, 5e-7)

For parameters the compared quantity is (p_after - p_before) / lr unless a test says otherwise, so that an error in the step's direction
is not hidden under |p|; exp_avg and exp_avg_sq are compared directly."""
import functools
import math

import torch

from omnifusion_amd.optim import CHUNK

FACTOR, FLOOR = 8.0, 5e-7
SIZES = [1, 1, 3, 4, 5, 63, 64, 65, 255, 257, 4095, 4096, 4097, 3 * CHUNK + 7]
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)]
GROUP_OF = [i % 2 for i in range(len(SIZES))]                                     # both groups hold small and large tensors
SCALES = [10.0 ** (-6.0 + 7.0 * i / (len(SIZES) - 1)) for i in range(len(SIZES))]  # the gradients' scale per tensor: 1e-6 .. 1e+1
LOADED_STEP = 7

# what each test runs: steps; max_norm (None: no clipping); a factor on every gradient (puts the norm on either side of max_norm); moments
# and step 7 put in through load_state_dict; CosineAnnealingWarmRestarts(T_0=2, T_mult=2) stepped after every optimiser step
CASES = {
    "loaded": dict(steps=1, max_norm=None, gfactor=1.0, loaded=True, sched=False),
    "ten": dict(steps=10, max_norm=None, gfactor=1.0, loaded=False, sched=True),
    "clip_above": dict(steps=1, max_norm=0.5, gfactor=1.0, loaded=True, sched=False),        # norm ~ 1e3
    "clip_below": dict(steps=1, max_norm=0.5, gfactor=1e-4, loaded=True, sched=False),       # norm ~ 0.1
    "six": dict(steps=6, max_norm=None, gfactor=1.0, loaded=False, sched=False),             # the checkpoint tests: 3 + 3 steps
    "four": dict(steps=4, max_norm=None, gfactor=1.0, loaded=False, sched=False),
}


def nerr(got, want):
    """max|v - v64| / max(1, rms(v64))"""
    want = want.double()
    return ((got.double() - want).abs().max() / max(1.0, want.pow(2).mean().sqrt().item())).item()


def params0():
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(n, generator=gen) for n in SIZES]


def moments0():
    """plausible loaded moments: exp_avg of the gradients' scale, exp_avg_sq of its square"""
    gen = torch.Generator().manual_seed(12)
    return ([s * torch.randn(n, generator=gen) for n, s in zip(SIZES, SCALES)],
            [s * s * (0.05 + torch.rand(n, generator=gen)) for n, s in zip(SIZES, SCALES)])


def grads(step, gfactor=1.0):
    gen = torch.Generator().manual_seed(100 + step)
    return [gfactor * s * torch.randn(n, generator=gen) for n, s in zip(SIZES, SCALES)]


def group_dicts(params):
    return [dict(GROUPS[g], params=[p for p, go in zip(params, GROUP_OF) if go == g]) for g in range(len(GROUPS))]


def loaded_state(opt, dtype=torch.float32):
    """a state dict in torch.optim.AdamW's format with moments0() and step 7, for `opt` (indices in group order)"""
    m0, v0 = moments0()
    order = [i for g in range(len(GROUPS)) for i in range(len(SIZES)) if GROUP_OF[i] == g]
    state = {k: {"step": torch.tensor(float(LOADED_STEP)), "exp_avg": m0[i].to(dtype), "exp_avg_sq": v0[i].to(dtype)} for k, i in enumerate(order)}
    return {"state": state, "param_groups": opt.state_dict()["param_groups"]}


class Restatement:
    """AdamW in float64 as the device computes it: ONE step count, the clip factor of clip_grad_norm_ applied inside the update"""

    def __init__(self, params, group_of, groups, max_norm=None):
        self.p = [p.detach().double().clone() for p in params]
        self.m, self.v = [torch.zeros_like(p) for p in self.p], [torch.zeros_like(p) for p in self.p]
        self.group_of, self.groups, self.max_norm, self.t = list(group_of), [dict(g) for g in groups], max_norm, 0

    def step(self, grads):
        """grads: a tensor or None per parameter -> the norm before clipping"""
        norm = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads if g is not None))
        clip = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (norm + 1e-6))
        self.t += 1
        for i, g in enumerate(grads):
            if g is None:
                continue
            h = self.groups[self.group_of[i]]
            lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
            g = g.double() * clip
            self.p[i] *= 1.0 - lr * wd
            self.m[i] += (g - self.m[i]) * (1.0 - b1)
            self.v[i] = self.v[i] * b2 + (1.0 - b2) * g * g
            self.p[i] -= lr / (1.0 - b1 ** self.t) * self.m[i] / (self.v[i].sqrt() / math.sqrt(1.0 - b2 ** self.t) + eps)
        return norm


def run_torch(name, dtype, make=None, after_step=None):
    """torch.optim.AdamW(foreach=False) + clip_grad_norm_ on the CPU in `dtype` over CASES[name] -> {p0, p, m, v: lists in SIZES order, norms,
    lrs: group 0's and 1's learning rate at the LAST step}"""
    c = CASES[name]
    params = [torch.nn.Parameter(p.to(dtype)) for p in params0()]
    opt = torch.optim.AdamW(group_dicts(params), foreach=False)
    if c["loaded"]:
        opt.load_state_dict(loaded_state(opt, dtype))
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=2, T_mult=2) if c["sched"] else None
    norms, lrs = [], None
    for k in range(c["steps"]):
        for p, g in zip(params, grads(k, c["gfactor"])):
            p.grad = g.to(dtype)
        if c["max_norm"] is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(params, c["max_norm"], foreach=False)))
        lrs = [g["lr"] for g in opt.param_groups]
        opt.step()
        if sched is not None:
            sched.step()
    return {"p0": params0(), "p": [p.detach().clone() for p in params], "m": [opt.state[p]["exp_avg"] for p in params],
            "v": [opt.state[p]["exp_avg_sq"] for p in params], "norms": norms, "lrs": lrs}


def quantities(r, direction=True):
    """what the gate compares, each as ONE vector over all tensors: dp = (p - p0) / lr (direction) or p itself, m, v"""
    if direction:
        dp = torch.cat([(p.double() - p0.double()) / GROUPS[g]["lr"] for p, p0, g in zip(r["p"], r["p0"], GROUP_OF)])
    else:
        dp = torch.cat([p.double() for p in r["p"]])
    return {"p": dp, "m": torch.cat([m.double() for m in r["m"]]), "v": torch.cat([v.double() for v in r["v"]])}


@functools.lru_cache(maxsize=None)
def reference(name, direction=True):
    """(float64 run, its quantities, {p, m, v: the gate's right side}) of a case, computed once"""
    r64, r32 = run_torch(name, torch.float64), run_torch(name, torch.float32)
    q64, q32 = quantities(r64, direction), quantities(r32, direction)
    gate = {k: FACTOR * max(nerr(q32[k], q64[k]), FLOOR) for k in q64}
    return r64, q64, gate


def check_gate(name, got, what, direction=True):
    """got: {p0, p, m, v} from the device, on the CPU -> the largest error / gate ratio; prints every error"""
    _, q64, gate = reference(name, direction)
    q = quantities(got, direction)
    worst = 0.0
    for k in ("p", "m", "v"):
        assert not torch.isnan(q[k]).any(), f"{what}: NaN (an unwritten element) in {k}"
        e = nerr(q[k], q64[k])
        label = ("(p - p0) / lr" if direction else "p") if k == "p" else {"m": "exp_avg", "v": "exp_avg_sq"}[k]
        print(f"adamw {name} [{what}] {label}: normalised error {e:.3e}  gate {gate[k]:.3e}  ratio {e / gate[k]:.3f}")
        assert e <= gate[k], f"{what}: {k}: {e:.3e} > {gate[k]:.3e}"
        worst = max(worst, e / gate[k])
    return worst
