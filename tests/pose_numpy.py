"""The relative pose behind a fundamental matrix, stated independently in numpy f64 (include/akaze_hip.h: "relative pose"):
E = K1^T F K0, np.linalg.svd, the four candidates in the library's order, the cheirality expressions, the winner, the kept subset
and the triangulated points -- and the two-view scenes the pose tests use.

One thing an independent decomposition cannot fix on its own: an SVD leaves the joint sign of (u1, v1) -- or of (u2, v2) -- free,
and flipping it exchanges Ra with Rb and t with -t, i.e. renumbers the same four candidates 3, 2, 1, 0.  The library's numbering
follows from the signs its Jacobi rotations leave; np.linalg.svd's from LAPACK's.  numpy_pose therefore takes `like_t`, the
library's +t, and flips (u1, v1) when its own t points the other way.  Everything else -- which rotation goes with which
translation, every count, the winner, the subset, the points -- is then compared as it stands."""
import numpy as np

from test_fundamental_refit_host import _rotation

EPS_RANK = 1e-6  # AKZ_FUNDAMENTAL_REFIT_EPSILON


def camera_matrix(cam):
    fx, fy, cx, cy = cam
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def pose_scene(seed, n, sigma=0.0, outliers=0.0, cams=((1200.0, 1200.0, 960.0, 540.0), (1200.0, 1200.0, 960.0, 540.0))):
    """two_view_scene of tests/test_fundamental_refit_host.py -- the same draws in the same order, so with the default cameras
    the same points -- with a camera (fx, fy, cx, cy) per image, returning the pose as well: a dict with p0, p1 (true), q1
    (observed), out (outlier mask), f (unit norm, p1^T F p0 = 0), r, t (x1 = R x0 + t, NOT normalised), x (the points in camera
    0's frame) and cams."""
    rng = np.random.default_rng(seed)
    k0, k1 = camera_matrix(cams[0]), camera_matrix(cams[1])
    x = np.c_[rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(4, 12, n)]
    r = _rotation(rng.uniform(-0.15, 0.15, 3))
    t = np.array([rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 1), rng.uniform(-0.3, 0.3), rng.uniform(-0.5, 0.5)])
    p0 = x @ k0.T
    p0 = p0[:, :2] / p0[:, 2:]
    p1 = (x @ r.T + t) @ k1.T
    p1 = p1[:, :2] / p1[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    f = np.linalg.inv(k1).T @ tx @ r @ np.linalg.inv(k0)
    f /= np.linalg.norm(f)
    out = rng.uniform(size=n) < outliers
    q1 = p1 + rng.normal(0, sigma, (n, 2))
    ang, dist = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 400, n)
    q1[out] += (np.c_[np.cos(ang), np.sin(ang)] * dist[:, None])[out]
    return dict(p0=p0, p1=p1, q1=q1, out=out, f=f, r=r, t=t, x=x, cams=cams)


def numpy_candidates(f, cam0, cam1, like_t=None):
    """-> (sigma / sigma1, [(R, t)] * 4 in the library's order) or (sigma / sigma1 or zeros, None) without a pose"""
    e = camera_matrix(cam1).T @ np.asarray(f, np.float32).astype(np.float64).reshape(3, 3) @ camera_matrix(cam0)
    u, s, vt = np.linalg.svd(e)
    if not (s[0] > 0.0 and np.isfinite(s[0])):
        return np.zeros(3), None
    if not s[1] > EPS_RANK * s[0]:
        return s / s[0], None
    v1, v2 = vt[0], vt[1]
    u1, u2 = e @ v1 / s[0], e @ v2 / s[1]
    if like_t is not None and np.dot(np.cross(u1, u2), np.asarray(like_t, np.float64)) < 0:
        u1, v1 = -u1, -v1
    u3, v3 = np.cross(u1, u2), np.cross(v1, v2)
    uu, vv = np.c_[u1, u2, u3], np.c_[v1, v2, v3]
    w = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ra, rb, t = uu @ w @ vv.T, uu @ w.T @ vv.T, u3 / np.linalg.norm(u3)
    return s / s[0], [(ra, t), (ra, -t), (rb, t), (rb, -t)]


def rays(p, cam):
    fx, fy, cx, cy = cam
    return np.c_[(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, np.ones(len(p))]


def depths(r, t, a, b):
    """-> det, n0, n1 per match"""
    c = a @ r.T
    cc, bb, cb = (c * c).sum(1), (b * b).sum(1), (c * b).sum(1)
    bt, ct = b @ t, c @ t
    return cc * bb - cb * cb, cb * bt - ct * bb, cc * bt - cb * ct


def in_front(r, t, a, b):
    det, n0, n1 = depths(r, t, a, b)
    return (det > 0) & (n0 > 0) & (n1 > 0)


def numpy_pose(p0, p1, f, cam0, cam1, like_t=None):
    """p0, p1: the matches' coordinates as the library sees them (f32 values).  -> dict(found, sigma, in_front [4], winner, r,
    t, keep (bool mask; all True without a pose), points ([kept, 3] or None))"""
    a, b = rays(np.asarray(p0, np.float64), cam0), rays(np.asarray(p1, np.float64), cam1)
    sigma, cand = numpy_candidates(f, cam0, cam1, like_t)
    res = dict(found=0, sigma=sigma, in_front=np.zeros(4, np.int64), winner=0, r=np.zeros((3, 3)), t=np.zeros(3),
               keep=np.ones(len(a), bool), points=None)
    if cand is None:
        return res
    masks = [in_front(r, t, a, b) for r, t in cand]
    res["in_front"] = np.array([int(m.sum()) for m in masks])
    w = int(np.argmax(res["in_front"]))  # (the first among equals)
    if res["in_front"][w] == 0:
        return res
    r, t = cand[w]
    det, n0, n1 = depths(r, t, a[masks[w]], b[masks[w]])
    l0, l1 = n0 / det, n1 / det
    pts = 0.5 * (l0[:, None] * a[masks[w]] + (l1[:, None] * b[masks[w]] - t) @ r)
    res.update(found=1, winner=w, r=r, t=t, keep=masks[w], points=pts)
    return res
