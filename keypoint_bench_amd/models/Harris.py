"""Drop-in for the reference's models/Harris.py: ``Harris(params)`` with ``eval`` / ``__call__(image) -> (score [B,1,H,W], None)`` (Harris.py:13-22),
computed by csrc/harris.hip through libkpb.so in one kernel: the uint8 plane ``((c0 + c1) + c2) * 255`` (fp32, truncated, low 8 bits kept -- under the
configs' ``gray: false`` the sum reaches 765 and WRAPS, as the reference's ``astype('uint8')`` does), the integer 3 x 3 Sobel, the integer
``block_size`` x ``block_size`` sums of the three products, and the response ``a c - b^2 - k (a + c)^2`` evaluated once in float64: the correctly rounded
value of the formula cv2.cornerHarris approximates in float32, bit-equal to the numpy restatement in tests/harris_fixtures.py.
The reference takes image 0 of the batch only; here every image of the batch gets its map.  The score is SIGNED (edges are negative, flat areas +0):
detect on it with ``detection(score, params, signed=True)``, as the pipelines and the runner do for a net with ``signed_scores``.  There are no weights
and no descriptors (``dim = 0``): the net is ready after construction and feeds detection, the repeatability task and the Lucas-Kanade tracker on the
frames; anything that matches descriptors refuses it.  ksize = 3, block_size 2 .. 6, any finite k, any H, W >= 8."""
from .. import weights as _weights
from ._base import HipNet


class Harris(HipNet):
    ARCH = _weights.ARCH_HARRIS
    signed_scores = True
    dense_descriptors = False

    def __init__(self, params):
        self.params = {k: params[k] for k in ("block_size", "ksize", "k")}      # Harris.py:16-18 reads all three with []
        plan = _weights.harris_plan(self.params)
        super().__init__()
        self.dim, self.desc_div = 0, 1
        self.load_packed(_weights.pack(plan, _weights.ARCH_HARRIS))

    def forward(self, image):
        score, _ = self._run(image, want_desc=False)
        return score, None

    __call__ = forward
