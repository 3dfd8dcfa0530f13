"""The references and the bound of tests/test_gpu_alike_family_shapes.py, checked without a GPU: at every sweep and batch shape the fp32 and float64
references of GoodPoint, LETNet, EdgePoint and ALIKE-l are finite and of the documented shape -- and the bound CAN fail: for each net two references with one rule
wrong (alike_family_shapes.wrong / VARIANTS) miss, at EVERY sweep shape, the bound the GPU test applies -- the per-net bar against the fp32 reference AND
4 x the fp32 reference's own error against the float64 one.  Every wrong variant misses on the descriptor / tracking map, and on the score too, with one
exception that is asserted as such: EdgePoint's score is computed from block 1 alone, so a wrong max-pool leaves it bit for bit what it was."""
import numpy as np
import pytest

from alike_family_shapes import BATCHES, DESC, NETS, SHAPES, VARIANTS, bars, images, oracle, references, rule, sid

EVERY = [(n, 1, s) for n in NETS for s in SHAPES] + [(n, b, s) for n in NETS for b, s in BATCHES]


@pytest.mark.parametrize("name,B,shape", EVERY, ids=sid)
def test_both_references_are_finite_and_of_the_documented_shape(name, B, shape):
    H, W = shape
    C, div = DESC[name]
    r32, r64 = references(name, B, shape)
    for (s, d), dtype in ((r32, np.float32), (r64, np.float64)):
        assert s.shape == (B, H, W) and d.shape == (B, C, H // div, W // div) and s.dtype == d.dtype == dtype
        assert np.isfinite(s).all() and np.isfinite(d).all()
    if name == "edgepoint":             # a signed logit: mostly negative, some positive
        assert float((r64[0] < 0).mean()) > 0.5 and float(r64[0].max()) > 0
    else:                               # a sigmoid
        assert 0.0 < float(r64[0].min()) and float(r64[0].max()) < 1.0
    if B > 1:
        assert not np.array_equal(r64[0][0], r64[0][B - 1])         # (different images)


def test_the_sweep_covers_what_it_is_there_for():
    """A column one tile wide whose coarse maps are 3 x 1 and 5 x 1, a strip whose width is a multiple of neither 64 nor 128, an odd multiple of 32 both ways
    taller than wide and its transpose; the batch of 17 is past the `batch >= 16` switch of the shared trunk."""
    assert all(h % 32 == 0 and w % 32 == 0 and h * w <= 224 * 96 for h, w in SHAPES + [s for _, s in BATCHES])
    assert [(h // 32, w // 32) for h, w in SHAPES[:2]] == [(3, 1), (5, 1)]
    assert SHAPES[2][0] == 32 and SHAPES[2][1] % 64 and SHAPES[2][1] % 128
    assert SHAPES[3] == SHAPES[4][::-1] and SHAPES[3][0] > SHAPES[3][1] and all((v // 32) % 2 for v in SHAPES[3])
    assert sum(h > w for h, w in SHAPES) == 3 and max(b for b, _ in BATCHES) >= 16
    assert all(len(VARIANTS[n]) >= 2 for n in NETS)


@pytest.mark.parametrize("name,kind", [(n, k) for n in NETS for k in VARIANTS[n]])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_the_bound_fails_a_reference_with_one_rule_wrong(shape, name, kind):
    (s32, d32), (s64, d64) = references(name, 1, shape)
    bs, bd = oracle(name, images(1, shape), kind=kind)
    assert np.isfinite(bs).all() and np.isfinite(bd).all()
    held = {}
    for what, got, r32, r64, atol in zip(("score", "map"), (bs[0], bd[0]), (s32[0], d32[0]), (s64[0], d64[0]), bars(name, d32[0])):
        e32, e64, e_ref, holds = rule(got, r32, r64, atol)
        print("%s %dx%d, reference with '%s': %s max |wrong - ref32| %.3g (bar %.3g), |wrong - ref64| %.3g against 4 x %.3g: %s"
              % ((name,) + shape + (kind, what, e32, atol, e64, e_ref, "passes" if holds else "FAILS")))
        held[what] = holds
    assert not held["map"]
    if (name, kind) == ("edgepoint", "pool"):
        assert np.array_equal(bs, s32)          # the score never sees a pool
    else:
        assert not held["score"]

