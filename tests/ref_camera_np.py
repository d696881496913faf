"""Float64 NumPy restatement of the projection under gsplat's camera models and rasterize modes (test helper, small scenes).

Written from the maths, like tests/ref_np.py, and independently of the fp32 operation order of csrc/project.hip:
    ortho:   u = fx x + cx, v = fy y + cy,                               J = [[fx, 0, 0], [0, fy, 0]]
    fisheye: u = fx x theta / rho + cx, v = fy y theta / rho + cy,       rho = |(x, y)|, theta = atan2(rho, z)
             J is the exact Jacobian of that map (1e-7 on rho, on z inside theta and on x^2 guards the optical axis, as gsplat
             does); tests/test_camera_models_cpu.py pins it against central finite differences of fisheye_uv
    pinhole: u = fx x / z + cx with the x/z, y/z clamp of the Jacobian (tests/ref_np.py)
    antialiased: compensation = sqrt(max(0, det(S) / det(S + eps2d I))), opacity x compensation
"""
import numpy as np

from ref_np import quat_to_rot

EPS = 1e-7
MODELS = ("pinhole", "ortho", "fisheye")


def fisheye_uv(p, fx, fy, cx, cy):
    x, y, z = p
    rho = np.hypot(x, y) + EPS
    theta = np.arctan2(rho, z + EPS)
    return np.array([fx * x * theta / rho + cx, fy * y * theta / rho + cy])


def fisheye_jacobian(p, fx, fy):
    x, y, z = p
    rho = np.hypot(x, y) + EPS
    theta = np.arctan2(rho, z + EPS)
    xx, yy, xy = x * x + EPS, y * y, x * y
    r2 = xx + yy
    iR2 = 1.0 / (r2 + z * z)
    a, b = z * iR2 / r2, theta / rho / r2
    return np.array([[fx * (xx * a + yy * b), fx * xy * (a - b), -fx * x * iR2],
                     [fy * xy * (a - b), fy * (yy * a + xx * b), -fy * y * iR2]])


def camera_map(model, p, K, W, H):
    """((u, v), J) of a camera-space point."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    x, y, z = p
    if model == "ortho":
        return np.array([fx * x + cx, fy * y + cy]), np.array([[fx, 0, 0], [0, fy, 0]], np.float64)
    if model == "fisheye":
        return fisheye_uv(p, fx, fy, cx, cy), fisheye_jacobian(p, fx, fy)
    limxp, limxn = (W - cx) / fx + 0.3 * 0.5 * W / fx, cx / fx + 0.3 * 0.5 * W / fx
    limyp, limyn = (H - cy) / fy + 0.3 * 0.5 * H / fy, cy / fy + 0.3 * 0.5 * H / fy
    tx, ty = z * min(limxp, max(-limxn, x / z)), z * min(limyp, max(-limyn, y / z))
    J = np.array([[fx / z, 0, -fx * tx / z ** 2], [0, fy / z, -fy * ty / z ** 2]])
    return np.array([fx * x / z + cx, fy * y / z + cy]), J


def compensation(S2, eps2d):
    """gsplat's antialiasing factor of a 2-D covariance S2 (before the eps2d low-pass)."""
    det_orig = S2[0, 0] * S2[1, 1] - S2[0, 1] ** 2
    det_blur = (S2[0, 0] + eps2d) * (S2[1, 1] + eps2d) - S2[0, 1] ** 2
    return np.sqrt(max(0.0, det_orig / det_blur))


def project(means, quats, scales, opac, viewmat, K, W, H, model="pinhole", antialiased=False, near=0.01, far=1e10,
            eps2d=0.3):
    means, quats, scales, opac = (np.asarray(a, np.float64) for a in (means, quats, scales, opac))
    vm, K = np.asarray(viewmat, np.float64), np.asarray(K, np.float64)
    R, t = vm[:3, :3], vm[:3, 3]
    n = means.shape[0]
    out = dict(ok=np.zeros(n, bool), means2d=np.zeros((n, 2)), conics=np.zeros((n, 3)), depths=np.zeros(n),
               radii=np.zeros(n, np.int64), v1=np.zeros(n), compensations=np.zeros(n), opacities=np.zeros(n))
    for i in range(n):
        mc = R @ means[i] + t
        if mc[2] < near or mc[2] > far:
            continue
        Rq = quat_to_rot(quats[i])
        Sc = R @ (Rq @ np.diag(scales[i] ** 2) @ Rq.T) @ R.T
        (u, v), J = camera_map(model, mc, K, W, H)
        S2 = J @ Sc @ J.T
        comp = compensation(S2, eps2d) if antialiased else 1.0
        S2 = S2 + eps2d * np.eye(2)
        det = np.linalg.det(S2)
        if det <= 0:
            continue
        b = 0.5 * (S2[0, 0] + S2[1, 1])
        v1 = b + np.sqrt(max(0.01, b * b - det))
        radius = int(np.ceil(3 * np.sqrt(v1)))
        if radius <= 0 or u + radius <= 0 or u - radius >= W or v + radius <= 0 or v - radius >= H:
            continue
        Ci = np.linalg.inv(S2)
        out["ok"][i], out["means2d"][i], out["depths"][i], out["radii"][i], out["v1"][i] = True, (u, v), mc[2], radius, v1
        out["conics"][i] = (Ci[0, 0], Ci[0, 1], Ci[1, 1])
        out["compensations"][i] = comp if antialiased else 0.0
        out["opacities"][i] = opac[i] * comp
    return out
