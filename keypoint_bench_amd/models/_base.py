"""What every HIP-backed model object shares: `NativeOwner`, the one owner of a packed blob and the native handle(s) made from it on
one device (the extractor nets and LightGlue), and `HipNet`, the torch.nn.Module-shaped surface of the extractor nets
(model_interface.py:43-86 uses load_state_dict / eval / __call__).  `KeypointOnlyNet` adds the mode of the nets that can skip their dense
descriptor map (ALNet, DISK): a `LazyDescriptors` handle stands where the map would be and the matcher samples inside the net."""
import ctypes

import torch

from .._lib import Context, c_void_p, ptr


class NativeOwner:
    """A subclass says how one handle is made (`_create`), how it goes (`_destroy`) and how many there are (`_count`)."""
    LOAD_FIRST = "load_state_dict() / load_packed() must be called before forward"

    def __init__(self):
        self._blob = None
        self._handle = None         # handle 0 (a c_void_p), None while nothing is created
        self._handles = []          # all of them
        self._ctx = None
        self._device = None

    def load_packed(self, blob: bytes):
        """Load an already packed .kpbw blob; the native side is rebuilt at the next use."""
        self._blob = bytes(blob)
        self._release()
        return self

    def _create(self, ctx):
        raise NotImplementedError

    def _destroy(self, lib, handle):
        raise NotImplementedError

    def _count(self):
        return 1

    def _ensure(self, device):
        ctx = Context.get(device)       # every call: the context follows torch's CURRENT stream (torch.cuda.stream(s))
        if self._handle is not None and self._device == device:
            return
        if self._blob is None:
            raise RuntimeError("%s: %s" % (type(self).__name__, self.LOAD_FIRST))
        self._release()
        self._ctx = ctx
        for _ in range(self._count()):      # a create that fails leaves _handle None; what was made before it goes at the next _release
            self._handles.append(self._create(ctx))
        self._handle, self._device = self._handles[0], device

    def _release(self):
        for h in self._handles:
            self._destroy(self._ctx.lib, h)
        self._handle, self._handles = None, []

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


class HipNet(NativeOwner):
    ARCH = 0
    signed_scores = False       # the score map is a raw logit (any sign): detect on it with signed=True (utils/extracter.py), as the pipelines do
    dense_descriptors = True    # forward writes the descriptor map (ALNet and DISK can be built without: the pipelines then sample inside the net)
    tracked_maps = False        # with the optical_flow matcher the tracker follows the net's descriptor maps instead of the frames (model_interface.py:262-272)

    def __init__(self):
        super().__init__()
        self._forward_count = 0
        self.training = False

    # ---- torch.nn.Module surface
    def eval(self):
        self.training = False
        return self

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def parameters(self):
        return iter(())

    def _create(self, ctx):
        h = c_void_p()
        ctx.check(ctx.lib.kpb_net_create(ctx.handle, self.ARCH, self._blob, len(self._blob), ctypes.byref(h)))
        self.dim, self.desc_div = ctx.lib.kpb_net_desc_dim(h), ctx.lib.kpb_net_desc_div(h)
        return h

    def _destroy(self, lib, handle):
        lib.kpb_net_destroy(handle)

    def _run(self, image: torch.Tensor, want_desc=True, slot=0):
        if not image.is_cuda:
            raise RuntimeError("keypoint_bench_amd.%s needs a CUDA/HIP tensor (MI355X); there is no CPU path" % type(self).__name__)
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError("image must be B x 3 x H x W")
        x = image.detach().to(torch.float32).contiguous()
        B, _, H, W = x.shape
        self._ensure(x.device)
        score = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
        desc = None
        if want_desc:
            desc = torch.empty((B, H // self.desc_div, W // self.desc_div, self.dim), dtype=torch.float32, device=x.device)
        self._ctx.check(self._ctx.lib.kpb_net_forward(self._handles[slot], ptr(x), B, H, W, ptr(score), ptr(desc)))
        self._forward_count += 1
        return score, desc

    def forward(self, image):
        score, desc = self._run(image)
        return score, desc.permute(0, 3, 1, 2)     # [B, C, H/div, W/div] view, channels-last storage

    __call__ = forward


class LazyDescriptors:
    """Stands where the dense descriptor map would be; only the matcher ever looks inside it
    (tasks pass desc_map through opaquely: MHA.py:38-39, AUC.py:119-120)."""

    def __init__(self, net, shape, slot, batch_index=0):
        self._net, self.shape, self._b, self._slot = net, torch.Size(shape), batch_index, slot
        self._stamp = net._slot_stamp[slot]

    def detach(self):
        return self

    @property
    def device(self):
        return self._net._device

    def sample(self, pts: torch.Tensor) -> torch.Tensor:
        """Descriptors at pts [N, >=2] (x, y normalised): what grid_sample on the dense map returns."""
        net = self._net
        if self._stamp != net._slot_stamp[self._slot]:
            raise RuntimeError("LazyDescriptors used after %d later forwards of the same net; its features are gone "
                               "(construct the net with dense_descriptors=True to keep maps alive)" % net.KEEP)
        return net._desc_at(pts, self._slot, self._b)


class KeypointOnlyNet(HipNet):
    """A net whose native side answers kpb_net_forward(desc_out_dev = NULL) and kpb_net_desc_at.  With dense_descriptors=False `forward` returns
    (score, LazyDescriptors) and KEEP native nets alternate, each with its own activations."""

    KEEP = 2    # dense_descriptors=False: the features of the last KEEP forwards stay alive (the reference's pattern is
                # forward(img0), forward(img1), then the matcher: model_interface.py:205-212 -> tasks/MHA.py:38-39)

    def __init__(self, dense_descriptors=True):
        super().__init__()
        self.dense_descriptors = bool(dense_descriptors)
        self._slot_stamp = [0] * self.KEEP

    def _count(self):       # keypoint-only mode: KEEP native nets
        return 1 if self.dense_descriptors else self.KEEP

    def forward(self, image: torch.Tensor):
        slot = 0 if self.dense_descriptors else self._forward_count % self.KEEP
        score, desc = self._run(image, self.dense_descriptors, slot)
        self._slot_stamp[slot] = self._forward_count
        if desc is not None:
            return score, desc.permute(0, 3, 1, 2)   # [B, dim, H, W] view, channels-last storage
        B, _, H, W = image.shape
        return score, LazyDescriptors(self, (B, self.dim, H, W), slot)

    __call__ = forward

    def _desc_at(self, pts: torch.Tensor, slot: int = 0, batch_index: int = 0):
        p = pts.detach().to(torch.float32).contiguous()
        n = p.shape[0]
        out = torch.empty((n, self.dim), dtype=torch.float32, device=p.device)
        if n == 0:
            return out
        if batch_index != 0 or self._last_batch() != 1:
            raise NotImplementedError("LazyDescriptors.sample: batch_size 1 only (config/config_MHA.yaml:10); "
                                      "use keypoint_bench_amd.pipeline for batched pairs")
        self._ctx.check(self._ctx.lib.kpb_net_desc_at(self._handles[slot], ptr(p), p.shape[1], n, ptr(None), ptr(out)))
        return out

    def _last_batch(self):
        return 1
