"""The lifecycle of "blob + native handle(s) on one device" (models/_base.py: NativeOwner), which the extractor nets, ALNet's keypoint-only
mode and LightGlue all go through, and the stage methods both pipelines are written on (pipeline.py: _Core).

  reload        a second load_packed / load_state_dict of the same weights drops the handle; the next run makes a new one and gives the same bits
  failed create a blob packed for another architecture is refused at the first forward (KpbError, no handle), and the right blob then works
  stream        a run inside torch.cuda.stream(s) moves the context to s and gives the bits of the default stream
  ALNet         is a HipNet, and says dim / desc_div / dense_descriptors before any device exists
  sequence      SequencePipeline over 4 frames equals PairPipeline (B = 1) on (frame j-1, frame j), frame 0 paired with itself

Everything is compared bit for bit: both sides run the same kernels on the same inputs.  Images are 64 x 96 (the smallest multiple-of-32 shape with more
than one NMS tile column); the LightGlue is the seeded 256-dim matcher of tests/test_gpu_lightglue_counts.py at (33, 31) points."""
import numpy as np
import pytest
import torch

from keypoint_bench_amd import synthetic
from keypoint_bench_amd._lib import KpbError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96
KINDS = ["alike-dense", "alike-sparse", "superpoint", "lightglue"]
NETS = KINDS[:3]


def _image(i=0):
    return torch.from_numpy(synthetic.image_pair(40 + i, H, W)[0][None]).to(DEV)


def _points():
    g = torch.Generator().manual_seed(3)
    return (torch.rand((50, 2), generator=g) * 2 - 1).to(DEV)


def _make(kind):
    if kind == "lightglue":
        from test_gpu_lightglue_counts import FULL, W256, _matcher
        return _matcher(W256, FULL)
    if kind == "superpoint":
        from keypoint_bench_amd.models.SuperPoint import superpoint_random
        return superpoint_random()
    from keypoint_bench_amd.models.ALike import alike_t
    return alike_t(dense_descriptors=(kind == "alike-dense"))


def _go(kind, obj):
    """One run of the object, as host arrays."""
    if kind == "lightglue":
        from test_gpu_lightglue_counts import W256, _run
        pairs, scores, stop = _run(obj, W256, 33, 31)
        return pairs, scores, np.asarray(stop)
    score, desc = obj(_image())
    if kind == "alike-sparse":
        desc = desc.sample(_points())
    return score.cpu().numpy(), desc.cpu().numpy()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_reload_recreates(kind):
    obj = _make(kind)
    first = _go(kind, obj)
    assert obj._handle is not None and first[0].size > 0
    if kind == "lightglue":
        from test_gpu_lightglue_counts import W256
        from keypoint_bench_amd import weights
        dim, _, variant, seed = W256
        obj.load_state_dict(weights.random_lightglue_state_dict(seed, dim, variant))
    else:
        obj.load_packed(obj._blob)
    assert obj._handle is None
    again = _go(kind, obj)
    assert obj._handle is not None
    _same(first, again)


@pytest.mark.parametrize("kind", NETS)
def test_failed_create_leaves_the_object_usable(kind):
    obj = _make(kind)
    right = obj._blob
    wrong = _make("superpoint" if kind != "superpoint" else "alike-dense")._blob
    obj.load_packed(wrong)
    with pytest.raises(KpbError):
        obj(_image())
    assert obj._handle is None
    obj.load_packed(right)
    got = _go(kind, obj)
    assert obj._handle is not None
    _same(got, _go(kind, _make(kind)))


@pytest.mark.parametrize("kind", KINDS)
def test_context_follows_the_current_stream(kind):
    obj = _make(kind)
    default = _go(kind, obj)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        there = _go(kind, obj)
        assert obj._ctx.stream == s.cuda_stream
    _same(default, there)
    back = _go(kind, obj)
    assert obj._ctx.stream == torch.cuda.current_stream(DEV).cuda_stream != s.cuda_stream
    _same(default, back)


def test_alnet_is_a_hipnet():
    from keypoint_bench_amd.models._base import HipNet
    from keypoint_bench_amd.models.ALike import alike_t
    for dense in (True, False):
        net = alike_t(dense_descriptors=dense)
        assert isinstance(net, HipNet)
        assert net._handle is None and net._device is None          # nothing ran
        assert (net.dim, net.desc_div, net.dense_descriptors) == (64, 1, dense)


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "sparse"])
def test_sequence_core_equals_pair_core(dense):
    from keypoint_bench_amd.models.ALike import alike_t
    from keypoint_bench_amd.pipeline import PairPipeline, SequencePipeline
    F = 4
    ep = dict(nms_dist=2, threshold=0.0, border_dist=2, top_k=128, min_score=0.0)
    bf = dict(metric="euclidean", max_distance=5, cross_check=True)
    wide = synthetic.image_pair(7, H, W + 2 * F)[0]                   # frame j: the same scene two columns further on
    frames = torch.from_numpy(np.stack([wide[:, :, 2 * j:2 * j + W] for j in range(F)])).to(DEV).contiguous()
    net = alike_t(dense_descriptors=dense)
    seq = SequencePipeline(net, ep, bf, F, H, W, device=DEV).run(frames, first=True)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (seq.k, seq.pairs, seq.m0, seq.m1)]
    assert got[0].min() > 0
    pair = PairPipeline(net, ep, bf, 1, H, W, device=DEV, place_map=False)
    for j in range(F):
        pair.run(frames[[max(j - 1, 0), j]].contiguous())
        torch.cuda.synchronize()
        k = int(pair.k[0])
        assert k == got[0][j]
        for a, b in zip(got[1:], (pair.pairs, pair.m0, pair.m1)):
            assert a[j, :k].tobytes() == b[0, :k].cpu().numpy().tobytes()
