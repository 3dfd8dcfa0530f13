"""oracle.sample (utils/matcher.py:221-226 restated) on the border, outside the map and on one-row / one-column maps, against the
operation the reference calls: torch.nn.functional.grid_sample(bilinear, align_corners=True, zero padding).  The points and maps are
those tests/test_gpu_match_prefilter.py hands to kpb_sample (tests/match_cases.py).  The two sum the four taps in different order and
un-normalise the coordinate in different order (a last-place difference in x moves a bilinear value continuously, also across a texel
and across the map's edge): atol 2e-6, the bound tests/test_gpu_match.py uses against the reference's own fixtures."""
import numpy as np
import pytest
import torch

import oracle
import match_cases as mc

ATOL = 2e-6


@pytest.mark.parametrize("shape", mc.SAMPLE_MAPS, ids=lambda s: "x".join(map(str, s)))
def test_oracle_sample_equals_grid_sample_on_the_edges(shape):
    d, p = mc.sample_map(*shape), mc.sample_points()
    grid = torch.from_numpy((p - np.float32(0.5)) * np.float32(2.0))[None, None]      # matcher.py:221-222
    want = torch.nn.functional.grid_sample(torch.from_numpy(d)[None], grid, mode="bilinear", align_corners=True, padding_mode="zeros")[0, :, 0].T.numpy()
    got = oracle.sample(d, p)
    hwc = oracle.sample_hwc(np.ascontiguousarray(d.transpose(1, 2, 0)), p)
    assert np.array_equal(got.view(np.uint32), hwc.view(np.uint32))     # strides change addresses only
    print("%s: max |oracle - grid_sample| = %.3g" % (shape, np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)
    C, Hd, Wd = shape
    if Wd > 1 and Hd > 1:       # all four taps off the map: exact zeros; a corner: the texel itself
        assert not got[np.all((p < -1.0 / (min(Hd, Wd) - 1)) | (p > 1 + 1.0 / (min(Hd, Wd) - 1)), axis=1)].any()
    assert np.array_equal(got[0], d[:, 0, 0]) and np.array_equal(got[1], d[:, -1, -1]) and np.array_equal(got[2], d[:, -1, 0]) and np.array_equal(got[3], d[:, 0, -1])
