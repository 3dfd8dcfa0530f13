"""Drop-in for the reference's tasks/VisualizeTrackingError.py `visualize_tracking_error` (9-51), the task that measures a net whose maps the tensor
Lucas-Kanade tracker follows (LETNet, GoodPoint; any other net is measured on the two images, model_interface.py:233-240): detection in view 0, the
ground-truth warp of the keypoints into view 1, the tracker from map 0 into map 1 started at the warped positions, and the mean distance between where
the tracker ends and where the warp says it should.  Every stage runs on the device (csrc/detect.hip, covis.hip, lk.hip: kpb_lk_track / kpb_track_error).

Left out: the drawing (plot_kps_error and cv2.imwrite, 48-50; OpenCV is absent), as tasks/repeatability.py here omits its overlays.  A matcher type other
than 'optical_flow' raises NotImplementedError: the reference leaves kps1 = None there and fails at the subtraction."""
import torch


def visualize_tracking_error(step, img0, score_map_0, desc_map_0, desc_map_1, params, warp01=None, *, random_angle=None):
    """tasks/VisualizeTrackingError.py:9-51.  desc_map_0 / desc_map_1 [1,3,H,W]: what is tracked (the net's maps, or the two images).  img0: the image the
    task is handed -- its (w - 1, h - 1) scale the warped keypoints (45), whatever the maps' size.  warp01 None or empty: kps0 is tracked onto itself and the
    error is all zeros (33-35, 42-43).  random_angle [n]: the tracker's start angles, one per tracked point (drawn as the reference draws them when missing).
    Returns the reference's dict: track_error (a 0-d tensor: float64 from kpb_track_error -- NaN without keypoints, as torch.mean of an empty tensor -- or the
    fp32 mean of the zeros), kps0 [n,2] (the covisible keypoints; [n,3] without a warp), kps1 [1,n,2] in pixels, kps01 [n,2] or None."""
    from ..utils import matcher
    from ..utils.extracter import detection
    from ..utils.projection import warp
    mp = params["matcher_params"]
    if mp["type"] != "optical_flow":
        raise NotImplementedError("VisualizeTrackingError tracks with matcher type 'optical_flow' (VisualizeTrackingError.py:32); got %r" % (mp["type"],))
    kps0 = detection(score_map_0, params["extractor_params"])                                          # 28
    if not warp01:                                                                                      # 33-35
        kps1 = matcher.optical_flow_tensor(kps0[:, 0:2], kps0[:, 0:2], desc_map_0, desc_map_1, mp["optical_flow_params"], random_angle=random_angle)
        error = torch.zeros(kps0.shape[0], dtype=torch.float32, device=kps0.device)                     # 42-43
        return {"track_error": torch.mean(error), "kps0": kps0, "kps1": kps1, "kps01": None}
    kps0, kps01, _, _ = warp(kps0[:, 0:2], warp01)                                                      # 37
    kps1 = matcher.optical_flow_tensor(kps0, kps01, desc_map_0, desc_map_1, mp["optical_flow_params"], random_angle=random_angle)
    scale = torch.tensor([[img0.shape[3] - 1, img0.shape[2] - 1]], dtype=torch.float32, device=kps1.device)      # 45: the image the task was handed
    _, mean = matcher.track_error(kps01[None], kps1, scale)                                             # 45-46, 51
    return {"track_error": mean[0], "kps0": kps0, "kps1": kps1, "kps01": kps01}


def tracking_error_batch(pipe, items, params, indices=None):
    """The rows [track_error, n_tracked] of the pairs a PairPipeline(track=...) run has just processed: one read-back of B means and B counts."""
    mean, n = pipe.track_mean.cpu().tolist(), pipe.trk["n"].cpu().tolist()
    return [[float(mean[b]), float(n[b])] for b in range(len(items))]
