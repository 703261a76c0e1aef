"""pers2equi — host-side mirror of the reference's equi_pers/pers2equi_torch.py:37, on the device.

    sample_erp, mask = pers2equi(pers_img, hFOV, wFOV, theta, phi, output_h, output_w)
    # pers_img [N,C,h,w], one image per view -> sample_erp [N,C,output_h,output_w], mask [N,1,output_h,output_w] (int64, 0 / 1)

Same name, arguments, values and return types as the reference: view k, looking at yaw theta[k] and pitch phi[k] (degrees) with the
fields of view hFOV (along the height) and wFOV (along the width), is put back onto its own panorama; mask is 1 where the view covers
the pixel (strictly inside the frustum and in front of the camera), and sample_erp is exactly 0 elsewhere.  Bilinear, zero padding,
align_corners=True on the reference's coordinate (y + w_len) / (2 w_len) * w.

One kernel of libomnifusion_hip.so (csrc/omni_freeview.hip); float32 on the GPU only, no CPU path.  This plain mirror has no backward
(NotImplementedError if the views require grad): the differentiable operators are equi_pers.differentiable.  `equi_pers.views_to_erp` merges the views onto ONE panorama without writing the N intermediates.
"""
import torch

from . import _freeview


def pers2equi(pers_img, hFOV, wFOV, theta, phi, output_h, output_w):
    erp, mask = _freeview.launch_pers2equi(pers_img, hFOV, wFOV, theta, phi, output_h, output_w)
    return erp, mask.to(torch.int64)
