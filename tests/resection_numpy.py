"""An independent f64 statement of camera resection for the resection tests and tools/resection.py: plain DLT through
numpy.linalg.svd of the 2 n x 12 design matrix itself -- no normal matrix, no Hartley normalisation, no fixed summation order --
then the nearest rotation of the left block.  It shares no code and no order of operations with csrc/akz_resection.hpp; what the
two agree on is the model.  Also the scene maker that every resection test uses."""
import numpy as np

CAMERA = (1400.0, 1400.0, 960.0, 540.0)   # fx, fy, cx, cy
SIZE = (1920.0, 1080.0)


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def project(R, t, points, camera=CAMERA):
    """-> (pixels [n, 2] f64, depth [n]) of f64 points under x_cam = R X + t"""
    fx, fy, cx, cy = camera
    c = np.asarray(points, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    return np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], axis=1), c[:, 2]


def make_scene(seed, n_true=200, n_outliers=50, noise=0.0, camera=CAMERA):
    """A random small rotation (a rotation vector of up to ~0.2 rad), t ~ 0.5, points in a 4 x 2.4 x 6 box 3 to 9 units ahead of
    the camera, f = 1 400, centre (960, 540); points, R and t rounded to f32 BEFORE the pixels are formed from them, pixels
    (+ Gaussian noise of `noise` px) rounded to f32.  The outliers are further points of the box whose pixels are replaced by
    uniform ones over the image; they are shuffled among the true ones.
    -> dict(points [n, 3] f32, pixels [n, 2] f32, camera, R, t (f64 values of the f32 roundings), true [n] bool)"""
    rng = np.random.default_rng(seed)
    n = n_true + n_outliers
    R = rodrigues(rng.uniform(-0.12, 0.12, 3)).astype(np.float32).astype(np.float64)
    t = rng.uniform(-0.5, 0.5, 3).astype(np.float32).astype(np.float64)
    xc = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.2, 1.2, n), rng.uniform(3.0, 9.0, n)], axis=1)
    pts = ((xc - t) @ R).astype(np.float32)          # X = R^T (x_cam - t)
    pix, _ = project(R, t, pts, camera)
    if noise:
        pix = pix + rng.normal(0.0, noise, pix.shape)
    true = np.ones(n, bool)
    true[rng.permutation(n)[:n_outliers]] = False
    pix[~true] = np.stack([rng.uniform(0.0, SIZE[0], n_outliers), rng.uniform(0.0, SIZE[1], n_outliers)], axis=1)
    return dict(points=pts, pixels=pix.astype(np.float32), camera=camera, R=R, t=t, true=true)


def dlt(points, pixels, camera=CAMERA):
    """(R, t, sigma / sigma1) of the DLT over all given correspondences, or None where the left block is singular"""
    fx, fy, cx, cy = camera
    X = np.asarray(points, np.float64)
    a = (np.asarray(pixels, np.float64)[:, 0] - cx) / fx
    b = (np.asarray(pixels, np.float64)[:, 1] - cy) / fy
    Xh = np.concatenate([X, np.ones((len(X), 1))], axis=1)
    Z = np.zeros_like(Xh)
    A = np.concatenate([np.concatenate([Xh, Z, -a[:, None] * Xh], axis=1), np.concatenate([Z, Xh, -b[:, None] * Xh], axis=1)], axis=0)
    P = np.linalg.svd(A)[2][-1].reshape(3, 4)
    if np.linalg.det(P[:, :3]) < 0:
        P = -P
    U, s, Vt = np.linalg.svd(P[:, :3])
    if not s[2] > 1e-6 * s[0]:
        return None
    return U @ Vt, P[:, 3] / s.mean(), s / s[0]


def reprojection_inliers(R, t, points, pixels, eps, camera=CAMERA):
    pix, z = project(R, t, points, camera)
    return (z > 0) & (np.linalg.norm(pix - np.asarray(pixels, np.float64), axis=1) < eps)


def pose_error(R, t, R_ref, t_ref):
    """(the angle of R R_ref^T in radians, |t - t_ref| / |t_ref|)"""
    q = np.asarray(R, np.float64) @ np.asarray(R_ref, np.float64).T
    s = np.linalg.norm([q[2, 1] - q[1, 2], q[0, 2] - q[2, 0], q[1, 0] - q[0, 1]]) / 2.0   # (atan2: arccos cannot see angles below 1e-8)
    return float(np.arctan2(s, (np.trace(q) - 1.0) / 2.0)), float(np.linalg.norm(np.asarray(t, np.float64) - t_ref) / np.linalg.norm(t_ref))
