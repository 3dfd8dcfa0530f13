"""Drop-in for the reference's models/disk.py: ``DISK()`` with ``load_state_dict`` / ``eval`` /
``__call__(image) -> (score_map [B,1,H,W], desc_map [B,128,H,W])`` (disk.py:309-313), computed by
csrc/convnet.hip through libkpb.so.  The descriptor map is stored channels-last.  H and W are multiples of
16; 16 x 16 is refused, as the reference's InstanceNorm2d refuses its 1 x 1 bottleneck.

With ``dense_descriptors=False`` the 128-channel map is neither computed nor allocated: the last layer runs its score channel alone (the same bits,
hence the same keypoints) and a ``LazyDescriptors`` handle stands where the map would be; ``brute_force_matcher`` samples it at the keypoints, where the
net evaluates the layer at the <= 4 integer taps of each point, normalises every tap and blends them -- the dense map's samples up to rounding."""
from .. import weights as _weights
from ._base import KeypointOnlyNet


class DISK(KeypointOnlyNet):
    ARCH = _weights.ARCH_DISK

    def __init__(self, desc_dim=128, setup=None, kernel_size=5, dense_descriptors=True):
        if desc_dim != 128 or kernel_size != 5 or setup is not None:
            raise NotImplementedError("this build carries kernels for the default DISK (desc_dim=128, 5x5, thin U-Net)")
        super().__init__(dense_descriptors)
        self.dim, self.desc_div = 128, 1

    def load_state_dict(self, state_dict, strict=True):
        if "extractor" in state_dict:      # model_interface.py:78 passes checkpoint['extractor']; accept both
            state_dict = state_dict["extractor"]
        self.load_packed(_weights.pack(_weights.tensors_disk(state_dict), _weights.ARCH_DISK))
        return "<All keys matched successfully>"


def disk_random(seed=0, dense_descriptors=True) -> "DISK":
    """DISK with seeded random weights (the reference checkpoint disk.pth is not in its tree)."""
    net = DISK(dense_descriptors=dense_descriptors)
    net.load_state_dict(_weights.random_disk_state_dict(seed))
    return net
