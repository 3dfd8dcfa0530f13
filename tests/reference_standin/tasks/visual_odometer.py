from utils.extracter import detection  # noqa: F401  (names the shim re-binds)
from utils.matcher import optical_flow_tensor, brute_force_matcher  # noqa: F401
from models.lightglue import LightGlue  # noqa: F401


def visual_odometry(step, *a, **k):
    raise NotImplementedError("the stand-in has no visual-odometry task")
