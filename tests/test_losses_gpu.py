"""GPU: what the two masked-mean losses share (csrc/omni_losses.hip) — the serial final and the workspace layout — at the size where an item gets
its 256 blocks and every block wraps: calculate_l1_loss against float64, and the same bits whatever the workspace held before.  BerHu's own max
pass, sum kernel and gradient against the float64 restatement of tests/_eval_cases.py (pinned on the CPU by tests/test_eval_cases_cpu.py): at the
block caps, with the maximum of |gt - pred| planted where a wrong max pass would miss it, and on the branch |d| == c."""
import ctypes

import numpy as np
import pytest
import torch

import _eval_cases as ec
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


# ---------------------------------------------------------------------------------------------------------------- BerHu against float64
U24 = ec.U24


def _berhu_raw(pred, gt, mask, wt, grad_out=1.0, fill=None):
    """omni_berhu_loss_f32 + omni_berhu_grad_f32 on a workspace of this test's own -> (loss float32, grad float32 numpy, c float32 (the first word of
    the workspace is the bits of max |gt - pred|), counts float32[B])"""
    from omnifusion_amd import _lib
    lib = _lib.load()
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    p, g, m, w = (torch.from_numpy(np.array(a)).to(DEV) for a in (pred, gt, mask, wt))          # copies: the cases are read-only
    B = pred.shape[0]; per = pred.size // B
    nbytes = lib.omni_berhu_workspace_bytes(B)
    assert nbytes == 64 + (8 * 2 * 256 + 4) * B
    ws = torch.full((nbytes + 4,), 0xFF if fill else 0, dtype=torch.uint8, device=DEV)          # 0xFF bytes: NaN as float and as double
    loss, grad, go = torch.full((), -7.0, device=DEV), torch.full_like(p, -7.0), torch.full((), grad_out, device=DEV)
    _lib.check(lib.omni_berhu_loss_f32(ptr(p), ptr(g), ptr(m), ptr(w), B, per, ptr(ws), ptr(loss), _lib.stream_of(p)), "berhu_loss")
    _lib.check(lib.omni_berhu_grad_f32(ptr(p), ptr(g), ptr(m), ptr(w), B, per, ptr(ws), ptr(go), ptr(grad), _lib.stream_of(p)), "berhu_grad")
    words = ws[:nbytes].cpu().numpy()
    maxbits = words[:4].view(np.float32)[0]
    counts = words[64 + 8 * 2 * 256 * B:].view(np.float32)[:B]
    return loss.cpu().numpy()[()], grad.cpu().numpy(), maxbits / np.float32(5), counts.copy(), maxbits


def _hold_berhu(what, pred, gt, mask, wt, items=None):
    """the loss within 10 * 2^-24 relative of float64; every gradient element (of `items`) within 6 * 2^-24 of its own float64 value and exactly 0
    where the mask is 0 or d = 0; c and the counts exact; the same bits on a workspace full of 0xFF"""
    r = ec.berhu(pred, gt, mask, wt)
    loss, grad, c, counts, _ = _berhu_raw(pred, gt, mask, wt)
    loss2, grad2, c2, counts2, _ = _berhu_raw(pred, gt, mask, wt, fill=True)
    assert loss.tobytes() == loss2.tobytes() and grad.tobytes() == grad2.tobytes() and c.tobytes() == c2.tobytes() and counts.tobytes() == counts2.tobytes(), what
    assert c.tobytes() == r["c"].tobytes(), (what, c, r["c"])
    assert np.array_equal(counts.astype(np.float64), r["counts"]), (what, counts, r["counts"])
    if np.isnan(r["loss"]):
        assert np.isnan(loss), (what, loss)
    else:
        err = abs(float(loss) - r["loss"]) / r["loss"] if r["loss"] else abs(float(loss))
        print(f"{what}: loss {loss:.9g} float64 {r['loss']:.12g} relative error {err:.2e} bound {10 * U24:.2e}")
        assert err <= 10 * U24, (what, err)
    items = range(pred.shape[0]) if items is None else items
    for b in items:
        ref, got = r["grad"][b], grad[b].astype(np.float64)
        if np.isnan(ref).all():
            assert np.isnan(got).all(), (what, b)
            continue
        gerr = np.abs(got - ref)
        rel = float((gerr[ref != 0] / np.abs(ref[ref != 0])).max()) if (ref != 0).any() else 0.0
        print(f"{what}: item {b} gradient relative error {rel:.2e} bound {6 * U24:.2e}")
        assert (gerr <= 6 * U24 * np.abs(ref)).all(), (what, b, rel)
        zero = (np.asarray(mask)[b] == 0) | (r["d"][b] == 0)
        assert (grad[b][zero] == 0).all() and zero.any() == bool((ref == 0).any()), (what, b)
    return r, loss, grad, c


@pytest.mark.parametrize("B,per", ec.BERHU_SIZES)
def test_berhu_against_float64_at_the_launch_edges(B, per):
    """1 x 1, 3 x 255, 3 x 257, 2 x 77 100 (77 100 > 256 x 256: the sum kernel's 256-block cap binds, ragged), 2 x 270 000 (540 000 > 2048 x 256: the
    max pass wraps); masks in {0, 0.5, 1}, weights in [0.5, 2].  The loss carries at most ten float32 roundings against the float64 restatement at
    the same float32 d and c: d * d, c * c, their sum, the division by 2 c (4), * mask, * weight (6), the sums in double, float(sum), sum / count (8),
    the mean over items in double and the final cast (9): 10 * 2^-24 relative, every term being non-negative.  A gradient element carries six:
    g / B, mask * weight, / count, d / c, and two products."""
    _hold_berhu(f"{B} x {per}", *ec.berhu_case(B, per))


@pytest.mark.parametrize("B,per", ec.BERHU_LARGE)
def test_berhu_maximum_found_wherever_it_is(B, per):
    """|gt - pred| = 40 planted in the last element, in an element beyond index 2048 x 256 (reached on a wrapped iteration only), in a masked-out
    element (the maximum is over everything, not over the mask), and in item 1 while item 0 is held to float64: every placement gives c = 8, the
    same bits, read from the first word of the workspace."""
    seen = []
    for placement in ec.BERHU_PLACEMENTS:
        if placement == "beyond_cap" and B * per <= 2048 * 256:
            continue
        r, loss, grad, c = _hold_berhu(f"{B} x {per} {placement}", *ec.berhu_case(B, per, placement), items=(0,) if placement == "item1" else None)
        seen.append(c.tobytes())
        assert c == np.float32(8.0)
    assert len(set(seen)) == 1 and len(seen) >= 3


def test_berhu_on_the_branch_and_in_the_corners():
    """max |d| = 5 so that c = 1: |d| == c takes the linear branch (gradient +-1 * scale), its upper neighbour the quadratic one (d / c), d = 0 gives 0;
    pred == gt everywhere (c = 0): loss 0, gradient 0; an item with an empty mask: the loss is NaN, the other items' gradients are not;
    grad_out = 3: exactly three times the gradient of grad_out = 1 where no product is denormal."""
    B, per = 3, 257
    pred, gt, mask, wt = ec.berhu_case(B, per, None, "planted")
    r, loss, grad, c = _hold_berhu("planted", pred, gt, mask, wt)
    assert c == np.float32(1.0)
    up = np.nextafter(np.float32(1), np.float32(2))
    _, _, _, counts, _ = _berhu_raw(pred, gt, mask, wt)
    for b in range(B):
        scale = -(np.float32(1.0) / np.float32(B)) * (mask[b, 0, 0, 3:10] * wt[b, 0, 0, 3:10] / counts[b])       # the kernel's own float32 sequence
        assert scale.dtype == np.float32
        want = scale * np.array([5.0, 1.0, -1.0, up, -up, 0.0, 1.0], np.float32)
        assert np.array_equal(grad[b, 0, 0, 3:10], want), (b, grad[b, 0, 0, 3:10], want)
    _, grad3, _, _, _ = _berhu_raw(pred, gt, mask, wt, grad_out=3.0)                  # B = 3: grad_out / B = 1 exactly
    g64 = ec.berhu(pred, gt, mask, wt, grad_out=3.0)["grad"]
    assert (np.abs(grad3.astype(np.float64) - g64) <= 6 * U24 * np.abs(g64)).all()

    pred, gt, mask, wt = ec.berhu_case(B, per, None, "equal")
    loss, grad, c, _, _ = _berhu_raw(pred, gt, mask, wt, fill=True)
    assert c == 0 and loss == 0 and (grad == 0).all()

    pred, gt, mask, wt = ec.berhu_case(B, per, None, "empty_item")
    r, loss, grad, c = _hold_berhu("empty item", pred, gt, mask, wt)
    assert np.isnan(loss) and np.isnan(grad[1]).all() and np.isfinite(grad[[0, 2]]).all()


def test_berhu_grad_out_three_is_three_times_grad_out_one():
    """B = 2: grad_out / B is exact for 1 and for 3.  The kernel rounds ((g / B) s) t with s = mask weight / count and t = sign(d) or d / c.  On the
    linear branch t = +-1 and fl(1.5 s) = 3 fl(0.5 s): three times to the bit.  On the quadratic branch fl(fl(1.5 s) t) and 3 fl(fl(0.5 s) t) =
    fl(1.5 fl(s t)) round different products, so 'exactly three times' does not hold there (nor in the reference's autograd); both sit within two
    roundings of 1.5 s t, hence within 4 * 2^-24 relative of each other, and each is held to its own float64 value above."""
    pred, gt, mask, wt = ec.berhu_case(2, 77100)
    r = ec.berhu(pred, gt, mask, wt)
    _, g1, _, _, _ = _berhu_raw(pred, gt, mask, wt, grad_out=1.0)
    _, g3, _, _, _ = _berhu_raw(pred, gt, mask, wt, grad_out=3.0)
    ref = np.float32(3) * g1
    linear = np.abs(r["d"]) <= r["c"]
    err = np.abs(g3.astype(np.float64) - ref.astype(np.float64))
    print(f"grad_out 3 against 3 x grad_out 1: {int((g3 != ref).sum())} of {g3.size} elements differ, all on the quadratic branch: "
          f"{not (g3 != ref)[linear].any()}; max relative {(err[ref != 0] / np.abs(ref[ref != 0])).max():.2e} bound {4 * U24:.2e}")
    assert linear.sum() > 10000 and (~linear).sum() > 10000
    assert np.array_equal(g3[linear], ref[linear])
    assert (err <= 4 * U24 * np.abs(ref.astype(np.float64))).all()
