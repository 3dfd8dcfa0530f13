"""Drop-in for the reference's models/D2_Net.py: ``D2Net(model_file=None, use_cuda=True)`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score [B,1,H,W], desc [B,512,H/8,W/8])`` (D2_Net.py:84-105), computed by csrc/d2net.hip through libkpb.so: the VGG-16 trunk up to
conv4_3 (three plain 2 x 2 max-pools, no dilation), the soft-detection score -- per image: exp(x / maximum), a 3 x 3 sum whose out-of-map taps count 1, the
ratio to the pixel's channel maximum, the maximum over the 512 channels, divided by the image's sum -- upsampled bilinearly with align_corners=True, and the
L2-normalised pre-ReLU conv4_3 map as 512-channel descriptors at 1/8 resolution, stored channels-last.  H and W must be multiples of 8 (the reference
floor-pools other shapes; that is not built).  As in the reference a pixel without a positive channel turns the whole score map into NaN: no guard is added."""
from .. import weights as _weights
from ._base import HipNet


class D2Net(HipNet):
    ARCH = _weights.ARCH_D2NET

    def __init__(self, model_file=None, use_cuda=True):
        super().__init__()
        self.dim, self.desc_div = 512, 8
        if model_file is not None:      # D2_Net.py:93-97
            import torch
            self.load_state_dict(torch.load(model_file, map_location="cpu")["model"])

    def load_state_dict(self, state_dict, strict=True):
        """Keys the forward does not read are ignored; the ten weight / bias pairs it reads must be there with their shapes (ValueError names the key)."""
        self.load_packed(_weights.pack(_weights.fold_d2net(state_dict), _weights.ARCH_D2NET))
        return "<All keys matched successfully>"


def d2net_random(seed=0) -> "D2Net":
    """D2-Net with seeded random weights (the reference checkpoint weights/d2_tf.pth is not in its tree)."""
    net = D2Net()
    net.load_state_dict(_weights.random_d2net_state_dict(seed))
    return net
