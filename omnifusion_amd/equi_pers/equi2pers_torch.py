"""equi2pers — host-side mirror of the reference's equi_pers/equi2pers_torch.py:37, on the device.

    persp = equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w)     # [B,C,H,W] -> [B,C,output_h,N*output_w]

Same name, arguments and values as the reference: N = len(theta) perspective views of the panorama, view k looking at yaw theta[k] and
pitch phi[k] (degrees; theta = phi = 0 is the centre of the image), laid side by side along the width of one tensor.  hFOV is the
field of view along the image HEIGHT and wFOV along its WIDTH (the reference's docstring has them the other way round; its code, and
this one, do not).  Bilinear, zero padding, align_corners=True; the reference's quirks are kept: longitude is scaled
by (W - 1) / W and does not wrap across the +-180 degree seam.

One kernel of libomnifusion_hip.so (csrc/omni_freeview.hip) computes the coordinates of a view pixel once and samples every image
plane with them; no grid tensor exists.  float32 on the GPU only, no CPU path.  These plain mirrors have no backward
(NotImplementedError if the image requires grad): the differentiable operators are equi_pers.differentiable.  `equi2pers_planar` returns the same samples as [B,N,C,output_h,output_w].
"""
from .. import _lib
from . import _freeview


def equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w):
    return _freeview.launch_equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w, _lib.LAYOUT_BCHNW)


def equi2pers_planar(equi_img, hFOV, wFOV, theta, phi, output_h, output_w):
    return _freeview.launch_equi2pers(equi_img, hFOV, wFOV, theta, phi, output_h, output_w, _lib.LAYOUT_BNCHW)
