"""GPU: what the two masked-mean losses share (csrc/omni_losses.hip) — the serial final and the workspace layout — at the size where an item gets
its 256 blocks and every block wraps: calculate_l1_loss against float64, and the same bits whatever the workspace held before."""
import ctypes

import numpy as np
import pytest
import torch

import _geometry_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_workspace_sizes():
    """header | double part[B][256][2] | float counts[B]: BerHu's header is 64 bytes (the bits of max|gt - pred|), L1 has none; B < 1 counts as 1."""
    from omnifusion_amd import _lib
    lib = _lib.load()
    for B in (0, 1, 2, 7):
        body = (8 * 2 * 256 + 4) * max(B, 1)
        assert lib.omni_l1_workspace_bytes(B) == body and lib.omni_berhu_workspace_bytes(B) == 64 + body


def test_l1_at_the_block_cap_against_float64_and_any_workspace():
    """B = 2, C = 3, 300 x 257: 231 300 elements per item against 256 x 256 threads, so the block cap binds and the grid-stride loop wraps with a ragged
    tail; a [B,1,H,W] and a [B,C,H,W] mask.  The loss within 2e-6 of the float64 restatement (the bound of test_imgrad_and_l1_against_float64_conv2d:
    values in [0, 1), sums in double, one float32 division per item); every gradient element within 1e-6 of the largest one (-(1 / B) (mask / count)
    sign: four float32 roundings, 2.4e-7, count < 2^24 exact).  Then the entries called on a workspace full of NaN: the same bits."""
    from omnifusion_amd import _lib
    from omnifusion_amd.supervision.direct import calculate_l1_loss
    lib = _lib.load()
    B, C, H, W = 2, 3, 300, 257
    rng = np.random.default_rng(2301)
    pred, gt = rng.random((B, C, H, W), dtype=np.float32), rng.random((B, C, H, W), dtype=np.float32)
    p64, g64 = torch.from_numpy(pred).double().requires_grad_(True), torch.from_numpy(gt).double()
    dev = lambda a: torch.from_numpy(a).to(DEV)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    for mask_c in (1, C):
        mask = (rng.random((B, mask_c, H, W)) < 0.6).astype(np.float32)
        ref = gc.l1_loss(p64, g64, torch.from_numpy(mask).double())
        gref, = torch.autograd.grad(ref, p64)
        p, g, m = dev(pred).requires_grad_(True), dev(gt), dev(mask)
        loss = calculate_l1_loss(p, g, m)
        grad, = torch.autograd.grad(loss, p)
        err = abs(float(loss.detach()) - float(ref.detach()))
        gerr = float((grad.double().cpu() - gref).abs().max()) / float(gref.abs().max())
        print(f"mask_c {mask_c}: loss {float(loss.detach()):.9f} float64 {float(ref.detach()):.9f} error {err:.2e}; gradient error {gerr:.2e} of the largest")
        assert err <= 2e-6, (mask_c, err)
        assert gerr <= 1e-6, (mask_c, gerr)

        ws = torch.full((lib.omni_l1_workspace_bytes(B) // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV)
        loss2, grad2, one = torch.empty((), device=DEV), torch.empty_like(grad), torch.ones((), device=DEV)
        pd = p.detach()
        _lib.check(lib.omni_l1_loss_f32(ptr(pd), ptr(g), ptr(m), B, C, H * W, mask_c, ptr(ws), ptr(loss2), _lib.stream_of(pd)), "l1_loss")
        _lib.check(lib.omni_l1_grad_f32(ptr(pd), ptr(g), ptr(m), B, C, H * W, mask_c, ptr(ws), ptr(one), ptr(grad2), _lib.stream_of(pd)), "l1_grad")
        assert torch.equal(loss2, loss.detach()) and torch.equal(grad2, grad), mask_c
        counts = ws.view(torch.float32)[2 * 2 * 256 * B:][:B]                # behind the partials, where the gradient entry looks for them
        assert torch.equal(counts.cpu(), torch.from_numpy(mask.sum(axis=(1, 2, 3), dtype=np.float64).astype(np.float32)))
