"""GPU: the input kernels and the point cloud (csrc/omni_io.hip, csrc/omni_area.h through omnifusion_amd/data.py and ply.py) against the
restatements of tests/_eval_cases.py (pinned on the CPU by tests/test_eval_cases_cpu.py).

  equal size       the four-pixel path and the byte path give each other's bits, and those of uint8 / 255 in numpy float32
  integer scales   the bytes of the exact integer restatement (2 x 2 half up, every other scale half to even, ties planted); depth and mask bit-equal
                   to the float32 sequence of the kernel written out in numpy
  depth codes      51 and 4096 masked out, 52 and 4095 kept; depth 0 where the mask is 0
  (70,140)->(30,60) the caps of test_preprocess_vs_restatement_INTER_AREA_UNPINNED against oracle/io_ref.py, which meets them against float64
  point cloud      colours as numpy's (rgb * 255).astype(uint8) for all 256 levels, saturated outside [0, 1]; points within 2e-6 of float64"""
import numpy as np
import pytest
import torch

import _eval_cases as ec
from oracle import io_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)                 # a copy: the cases are read-only


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _rgb_paths(fr):
    """preprocess_rgb at equal size from a 256-byte-aligned source (the four-pixel path where H * W is a multiple of 4) and from the same bytes one
    byte further on (the byte path)"""
    from omnifusion_amd.data import preprocess_rgb
    B, H, W, _ = fr.shape
    aligned = t(fr)
    buf = torch.zeros(fr.size + 1, dtype=torch.uint8, device=DEV)
    buf[1:] = aligned.reshape(-1)
    shifted = buf[1:].view(B, H, W, 3)
    assert aligned.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 1 and shifted.is_contiguous()
    return preprocess_rgb(aligned, (H, W)).cpu().numpy(), preprocess_rgb(shifted, (H, W)).cpu().numpy()


@pytest.mark.parametrize("name", ["quad", "byte", "b2", "levels"])
def test_equal_size_both_paths_give_uint8_over_255(name):
    """(6,10): 60 pixels, the four-pixel path; (5,7): 35 pixels, the byte path; the same frames from a source pointer one byte off: the byte path; B = 2:
    the four-pixel path across the item boundary; 16 x 16 with every byte level in every channel"""
    fr = ec.prep_same_case(name)
    want = (fr.astype(F32) / F32(255)).transpose(0, 3, 1, 2)
    a, b = _rgb_paths(fr)
    assert a.shape == want.shape
    assert np.array_equal(_bits(a), _bits(want)) and np.array_equal(_bits(b), _bits(want))


@pytest.mark.parametrize("fy,fx", ec.PREP_INT_SCALES)
def test_integer_scales_equal_the_integer_restatement(fy, fx):
    from omnifusion_amd.data import preprocess_depth, preprocess_rgb
    fr, dz, (H, W) = ec.prep_int_case(fy, fx)
    got = preprocess_rgb(t(fr), (H, W)).cpu().numpy()
    want = ec.prep_rgb_int(fr, H, W)
    wrong = _bits(got) != _bits(want)
    assert not wrong.any(), (int(wrong.sum()), np.argwhere(wrong)[:4].tolist())
    gd, gm = preprocess_depth(t(dz.view(np.int16)), (H, W))
    rd, rm = ec.prep_depth_int(dz, H, W)
    assert np.array_equal(gm.cpu().numpy(), rm) and np.array_equal(_bits(gd.cpu().numpy()), _bits(rd))


def test_depth_codes_on_either_side_of_the_thresholds():
    from omnifusion_amd.data import preprocess_depth
    codes = ec.DEPTH_CODES
    gd, gm = preprocess_depth(t(codes.view(np.int16)), codes.shape[1:])
    rd, rm = ec.prep_depth_int(codes, *codes.shape[1:])
    gd, gm = gd.cpu().numpy(), gm.cpu().numpy()
    assert codes.ravel().tolist()[1:5] == [51, 52, 4095, 4096] and gm.ravel().tolist() == [0, 0, 1, 1, 0, 0, 1]
    assert np.array_equal(gm, rm) and np.array_equal(_bits(gd), _bits(rd)) and (gd[gm == 0] == 0).all()


def test_fractional_scale_within_the_caps():
    from omnifusion_amd.data import preprocess_depth, preprocess_rgb
    fr, dz = ec.fractional_case()
    H, W = ec.FRACTIONAL[1]
    got = preprocess_rgb(t(fr), (H, W)).cpu().numpy()
    d = np.abs(got - io_ref.preprocess_rgb(fr, H, W))
    gd, gm = preprocess_depth(t(dz.view(np.int16)), (H, W))
    rd, rm = io_ref.preprocess_depth(dz, H, W)
    flip = gm.cpu().numpy() != rm
    derr = np.abs(gd.cpu().numpy() - rd)[~flip].max()
    print(f"(70,140)->(30,60): rgb max {d.max():.3e} share {(d > 1e-6).mean():.2e}; mask flips {flip.mean():.2e}; depth max {derr:.3e}")
    assert d.max() <= ec.RGB_STEP_CAP and (d > 1e-6).mean() <= ec.SHARE_CAP
    assert flip.mean() <= ec.FLIP_CAP and derr <= ec.DEPTH_CAP


def test_pointcloud_levels_and_points_against_float64():
    """B = 3, 5 x 7 (105 vertices: one ragged block): every k / 255 comes back as numpy's (rgb * 255).astype(uint8) has it, -0.1 as 0 and 1.2 as 255;
    the points within 2e-6 (the gate of test_pointcloud_and_ply_golden) of the float64 evaluation; records at a 15-byte stride"""
    from omnifusion_amd.ply import _records, depth_to_pointcloud
    depth, rgb = ec.pointcloud_case()
    pts, col = depth_to_pointcloud(t(depth), t(rgb))
    pts, col = pts.cpu().numpy(), col.cpu().numpy()
    B, _, H, W = depth.shape
    got = col.reshape(B, H, W, 3).transpose(0, 3, 1, 2).ravel()                # back to the order of rgb
    flat = rgb.ravel()
    assert np.array_equal(got[:256], (flat[:256] * 255).astype(np.uint8)) and got[256] == 0 and got[257] == 255
    assert np.array_equal(got[258:], (flat[258:] * 255).astype(np.uint8))
    err = np.abs(pts.astype(np.float64) - ec.pointcloud64(depth)).max()
    print(f"point cloud: max error {err:.3e} against float64, gate 2e-6")
    assert pts.shape == (3, 35, 3) and err <= 2e-6
    rec = _records(t(depth), t(rgb)).cpu().numpy()
    assert rec.shape == (3, 35, 15) and rec.dtype == np.uint8
    raw = rec.tobytes()
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("blue", "u1"), ("green", "u1"), ("red", "u1")])
    a = np.frombuffer(raw, dt)
    assert dt.itemsize == 15 and a.shape == (105,)
    assert np.array_equal(np.stack([a["x"], a["y"], a["z"]], -1).reshape(3, 35, 3).view(np.uint32), pts.view(np.uint32))
    assert np.array_equal(np.stack([a["blue"], a["green"], a["red"]], -1).reshape(3, 35, 3), col)
