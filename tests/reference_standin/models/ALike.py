"""ALNet(param): the host forward of ALIKE-t through the project's CPU restatement (oracle/alike_ref.py) on the folded state_dict."""
import torch


class ALNet(object):
    def __init__(self, param):
        self.param, self.t = dict(param), None

    def load_state_dict(self, state_dict, strict=True):
        from keypoint_bench_amd import weights
        self.t = {k: torch.from_numpy(v) for k, v in weights.fold_alike(state_dict).items()}

    def eval(self):
        return self

    def __call__(self, image):
        from oracle import alike_ref
        return alike_ref.alnet_forward(image, self.t)
