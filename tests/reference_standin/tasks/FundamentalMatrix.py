from utils.extracter import detection  # noqa: F401  (names the shim re-binds)
from utils.matcher import optical_flow_tensor, brute_force_matcher  # noqa: F401
from utils.projection import warp  # noqa: F401
from utils.mvg import fundamental_estimate  # noqa: F401
from models.lightglue import LightGlue  # noqa: F401


def fundamental_matrix_ransac(step, *a, **k):
    raise NotImplementedError("the stand-in has no fundamental-matrix task")


def fundamental_matrix(step, *a, **k):
    raise NotImplementedError("the stand-in has no fundamental-matrix task")
