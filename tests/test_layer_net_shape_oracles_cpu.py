"""The oracles and the bounds of tests/test_gpu_layer_net_shapes.py, checked without a GPU: at every sweep and batch shape the fp32 and float64 chains of R2D2,
SFD2 and D2-Net are finite, SFD2's unsure share stays under its cap, its three stability classes occur, R2D2's maps are constant exactly where every conv8 tap is
padding -- and the shapes and bounds CAN fail: a chain with one edge rule wrong (layer_net_shapes.wrong: a tap bound off by one, replicate for zero padding, a
flipped align_corners, zeros for D2-Net's ones) lies outside the GPU test's bound of the right chain at the shapes the sweep aims at that edge."""
import functools

import numpy as np
import pytest

from layer_net_shapes import (BATCHES, DESC, NETS, SHAPES, UNSURE_CAP, batch_images, constant_per_channel, is_constant, multiplier, oracle, r2d2_atols, r2d2_rule,
                              ratio_rule, sfd2_classes, sid, sweep_image)
from sfd2_fixtures import MARGIN

EVERY = [(n, 1, s) for n in NETS for s in SHAPES[n]] + [(n, b, s) for n in NETS for b, s in BATCHES[n]]


@functools.lru_cache(maxsize=None)
def _both(name, B, shape):
    """(fp32 maps, float64 maps) of the sweep image (B = 1) or of the batch test's B images; computed once, never written to."""
    imgs = sweep_image(*shape) if B == 1 else batch_images(B, *shape)
    return oracle(name, imgs), oracle(name, imgs, double=True)


@pytest.mark.parametrize("name,B,shape", EVERY, ids=sid)
def test_both_oracles_are_finite_and_of_the_documented_shape(name, B, shape):
    H, W = shape
    C, div = DESC[name]
    for s, d, m in _both(name, B, shape):
        assert s.shape == (B, H, W) and d.shape == (B, C, H // div, W // div)
        assert np.isfinite(s).all() and np.isfinite(d).all() and (m is None or np.isfinite(m).all())
    if name == "r2d2":          # all conv8 taps padding <=> min(H, W) <= 8: its output is its bias at every pixel
        for s, d, _ in _both(name, B, shape):
            for i in range(B):
                assert is_constant(s[i]) == constant_per_channel(d[i]) == (min(H, W) <= 8), shape
        if min(H, W) <= 8:
            assert abs(float(_both(name, B, shape)[1][0].max()) - 0.185) < 5e-4


@pytest.mark.parametrize("B,shape", [(1, s) for s in SHAPES["sfd2"]] + BATCHES["sfd2"], ids=sid)
def test_sfd2_unsure_share_stays_under_the_cap(B, shape):
    margin = _both("sfd2", B, shape)[1][2]
    for i in range(B):
        share = float((margin[i] < MARGIN).mean())
        print("sfd2 %dx%d image %d of %d: %.3f %% of the pixels have a float64 margin below %g" % (shape + (i, B, 100 * share, MARGIN)))
        assert share <= UNSURE_CAP


def test_sfd2_sweep_sees_all_three_stability_classes():
    """A score that ignored the class, or mixed two of them up, would pass where only one or two occur."""
    full = [s for s in SHAPES["sfd2"] if set(np.unique(sfd2_classes(sweep_image(*s))).tolist()) == {0, 1, 2}]
    print("sfd2: all three stability classes at", full)
    assert len(full) >= 3 and {(136, 24), (24, 40), (120, 160)} <= set(full)


def _r2d2_fails(shape, kind):
    o32, o64 = _both("r2d2", 1, shape)
    bad = oracle("r2d2", sweep_image(*shape), kind=kind)
    out = []
    for what, i, atol in zip(("score", "desc"), (0, 1), r2d2_atols()):
        e32, e64, e_ref, holds = r2d2_rule(bad[i], o32[i], o64[i], atol)
        print("r2d2 %dx%d, chain with '%s': %s max |wrong - chain32| %.3g (atol %.3g), |wrong - chain64| %.3g against 4 x %.3g: %s"
              % (shape + (kind, what, e32, atol, e64, e_ref, "passes" if holds else "FAILS")))
        out.append(not holds)
    return out


@pytest.mark.parametrize("shape", [(9, 9), (15, 17), (16, 16), (17, 33)], ids=sid)
def test_r2d2_bound_fails_a_tap_bound_off_by_one(shape):
    """(9,9): the only taps inside are conv8's at the four corners, and three of them are in the last row or column; 15 .. 17: the sizes around conv8's reach."""
    assert all(_r2d2_fails(shape, "tap"))


@pytest.mark.parametrize("shape", [(7, 200), (130, 6), (1, 1)], ids=sid)
def test_r2d2_constant_shapes_cannot_see_a_tap_bound_and_the_sweep_does_not_rely_on_them(shape):
    """With min(H, W) <= 8 the maps are conv8's bias whatever the layers below do: these shapes check that NO tap counts, not where the bound lies."""
    assert not any(_r2d2_fails(shape, "tap"))


@pytest.mark.parametrize("shape", [(15, 17), (17, 33), (33, 129), (136, 200)], ids=sid)
def test_r2d2_bound_fails_replicate_padding_in_the_dilated_3x3(shape):
    assert all(_r2d2_fails(shape, "replicate"))


def _ratio_fails(name, shape, kind):
    o32, o64 = _both(name, 1, shape)
    bad = oracle(name, sweep_image(*shape), kind=kind)
    keep = None if name == "d2net" else o64[2] >= MARGIN
    err, ref = ratio_rule(bad[0], o32[0], o64[0], keep)
    M = max(multiplier(name))
    print("%s %dx%d, chain with '%s': score max |wrong - chain64| %.3g = %.3g x ref_err %.3g (M = %d)" % ((name,) + shape + (kind, err, err / ref, ref, M)))
    return err > M * ref


@pytest.mark.parametrize("name,shape", [("sfd2", s) for s in [(8, 264), (200, 8), (24, 8), (24, 40)]] + [("d2net", s) for s in [(8, 136), (200, 8), (8, 16), (24, 40)]], ids=sid)
def test_ratio_bound_fails_a_flipped_align_corners(name, shape):
    """SFD2: the x 4 upsampling of the stability logits (align_corners False); D2-Net: the x 8 upsampling of the score (True).  The strips leave one direction
    with a single source row or column, where only the other direction can tell the two rules apart.  (SFD2's 8 x 136 cannot: the flipped rule moves no pixel with a sure margin to another class
    there; 8 x 264 is the strip one cell high that does.)"""
    assert _ratio_fails(name, shape, "align")


@pytest.mark.parametrize("shape", [(8, 136), (200, 8), (24, 8), (8, 16), (24, 40)], ids=sid)
def test_d2net_ratio_bound_fails_zero_padding_of_the_local_mean(shape):
    """On a strip one cell high or wide six of a window's nine values are padding at every cell."""
    assert _ratio_fails("d2net", shape, "zeros")
