def fundamental_estimate(pts0, pts1):
    """(F, inliers0, inliers1); with fewer than 8 points there is no estimate."""
    pts0, pts1 = pts0.cpu().numpy(), pts1.cpu().numpy()
    if pts0.shape[0] < 8:
        return None, pts0, pts1
    raise NotImplementedError("the stand-in has no RANSAC")
