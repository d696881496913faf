// project_grad.h -- the vector-Jacobian product of the projection of ONE Gaussian, in float64.
//
// The function differentiated is projection.project_torch's (k_project's arithmetic as a function: csrc/project.hip), term by term:
//     q / |q| -> R(q);  M = R(q) diag(s);  Sigma = M M^T;  C = R Sigma R^T;  pc = R mean + t;  (u, v, J) of the camera model;
//     S2 = J C J^T;  + eps2d on the diagonal;  conic = inverse of the 2 x 2;  antialiased: o sqrt(det(S2) / det(S2 + eps2d I))
// and the inputs of the product are the six numbers of a v_g2d row: d / d(u, v, conic a, b, c, filed opacity).  The forward is
// recomputed here in double from the stored float32 inputs (the filed float32 conic is not read); out come d / d(mean, quat, scale,
// opacity) and this Gaussian's contribution to d / d(R, t) of the view matrix.
//
// Plain C++: no HIP intrinsic, no header but <math.h>, so that the same text compiles for the device (csrc/project_grad.hip) and for
// the host (tests/project_grad_host.cpp, where it is checked against torch's float64 autograd).  Camera model and rasterize mode are
// template parameters, as in k_project.  The caller decides which rows are visible; nothing is culled here.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GWBP_HD __host__ __device__ inline
#else
#define GWBP_HD inline
#endif

namespace gwbp {

constexpr int kGradPinhole = 0, kGradOrtho = 1, kGradFisheye = 2; // GWBP_CAMERA_*
constexpr double kGradClampMargin = 0.3;                          // project_torch's CLAMP_MARGIN
constexpr double kGradFisheyeEps = 1e-7;                          // project_torch's FISHEYE_EPS

struct ProjView { // the view as gwbp_view stores it, widened
    double R[9], t[3], fx, fy, cx, cy, W, H, eps2d;
};

struct ProjGrad {
    double mean[3], quat[4], scale[3], opacity;
    double R[9], t[3]; // this Gaussian's share of d / d(viewmat[:3, :3]) (row-major) and d / d(viewmat[:3, 3])
};

// v: d / d(u, v, ca, cb, cc, o) of the projected record (a v_g2d row)
template <int CAM, bool AA>
GWBP_HD void project_vjp(const ProjView &V, const double mean[3], const double quat[4], const double scale[3], double opacity,
                         const double v[6], ProjGrad &g)
{
    const double *R = V.R;
    // ---- forward ------------------------------------------------------------------------------------------------------------------
    const double x = R[0] * mean[0] + R[1] * mean[1] + R[2] * mean[2] + V.t[0];
    const double y = R[3] * mean[0] + R[4] * mean[1] + R[5] * mean[2] + V.t[1];
    const double z = R[6] * mean[0] + R[7] * mean[1] + R[8] * mean[2] + V.t[2];
    const double qn = sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
    const double iqn = 1.0 / qn;
    const double qw = quat[0] * iqn, qx = quat[1] * iqn, qy = quat[2] * iqn, qz = quat[3] * iqn;
    double Q[9] = {1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz),     2 * (qx * qz + qw * qy),
                   2 * (qx * qy + qw * qz),     1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx),
                   2 * (qx * qz - qw * qy),     2 * (qy * qz + qw * qx),     1 - 2 * (qx * qx + qy * qy)};
    double M[9], S[9], A[9], C[9]; // M = Q diag(s), S = M M^T, A = R S, C = A R^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = Q[3 * i + j] * scale[j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            S[3 * i + j] = M[3 * i] * M[3 * j] + M[3 * i + 1] * M[3 * j + 1] + M[3 * i + 2] * M[3 * j + 2];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            A[3 * i + j] = R[3 * i] * S[j] + R[3 * i + 1] * S[3 + j] + R[3 * i + 2] * S[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = A[3 * i] * R[3 * j] + A[3 * i + 1] * R[3 * j + 1] + A[3 * i + 2] * R[3 * j + 2];

    double J[6]; // d(u, v) / d(x, y, z), row-major 2 x 3
    // what the camera model keeps for its backward
    double rz = 0, tcx = 0, tcy = 0;                                  // pinhole
    bool free_x = false, free_y = false;                              // pinhole: the clamp of x/z (y/z) does not bind
    double rho = 0, r = 0, theta = 0, xx = 0, yy = 0, xy = 0, r2 = 0, iR2 = 0, fa = 0, fb = 0, fs = 0, zz = 0; // fisheye
    if constexpr (CAM == kGradPinhole) {
        const double tan_x = 0.5 * V.W / V.fx, tan_y = 0.5 * V.H / V.fy;
        const double lim_xp = (V.W - V.cx) / V.fx + kGradClampMargin * tan_x, lim_xn = V.cx / V.fx + kGradClampMargin * tan_x;
        const double lim_yp = (V.H - V.cy) / V.fy + kGradClampMargin * tan_y, lim_yn = V.cy / V.fy + kGradClampMargin * tan_y;
        rz = 1.0 / z;
        const double tx = x * rz, ty = y * rz;
        // torch.clamp passes the gradient where min <= value <= max
        free_x = tx >= -lim_xn && tx <= lim_xp;
        free_y = ty >= -lim_yn && ty <= lim_yp;
        tcx = tx < -lim_xn ? -lim_xn : (tx > lim_xp ? lim_xp : tx);
        tcy = ty < -lim_yn ? -lim_yn : (ty > lim_yp ? lim_yp : ty);
        J[0] = V.fx * rz, J[1] = 0, J[2] = -(V.fx * (z * tcx) * rz * rz);
        J[3] = 0, J[4] = V.fy * rz, J[5] = -(V.fy * (z * tcy) * rz * rz);
    } else if constexpr (CAM == kGradOrtho) {
        J[0] = V.fx, J[1] = 0, J[2] = 0;
        J[3] = 0, J[4] = V.fy, J[5] = 0;
    } else {
        const double eps = kGradFisheyeEps;
        r = sqrt(x * x + y * y);
        rho = r + eps;
        zz = z + eps;
        theta = atan2(rho, zz);
        xx = x * x + eps, yy = y * y, xy = x * y;
        r2 = xx + yy;
        iR2 = 1.0 / (r2 + z * z);
        fa = z * iR2 / r2;
        fb = theta / rho / r2;
        fs = theta / rho;
        J[0] = V.fx * (xx * fa + yy * fb), J[1] = V.fx * xy * (fa - fb), J[2] = -(V.fx * x * iR2);
        J[3] = V.fy * xy * (fa - fb), J[4] = V.fy * (yy * fa + xx * fb), J[5] = -(V.fy * y * iR2);
    }
    double B[6]; // B = J C
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 3; ++j)
            B[3 * i + j] = J[3 * i] * C[j] + J[3 * i + 1] * C[3 + j] + J[3 * i + 2] * C[6 + j];
    const double c00 = B[0] * J[0] + B[1] * J[1] + B[2] * J[2];
    const double c01 = B[0] * J[3] + B[1] * J[4] + B[2] * J[5];
    const double c11 = B[3] * J[3] + B[4] * J[4] + B[5] * J[5];
    const double det_orig = c00 * c11 - c01 * c01;
    const double a00 = c00 + V.eps2d, a11 = c11 + V.eps2d;
    const double det = a00 * a11 - c01 * c01;
    const double idet = 1.0 / det;

    // ---- backward: the opacity and the 2 x 2 ------------------------------------------------------------------------------------
    double v_det_orig = 0, v_det = 0;
    if constexpr (AA) {
        const double ratio = det_orig * idet;
        if (ratio > 0) { // project_torch's select: zero, and no gradient, otherwise
            const double comp = sqrt(ratio);
            g.opacity = v[5] * comp;
            const double v_ratio = v[5] * opacity * 0.5 / comp;
            v_det_orig = v_ratio * idet;
            v_det = -v_ratio * ratio * idet;
        } else {
            g.opacity = 0;
        }
    } else {
        g.opacity = v[5];
    }
    // conic = (a11, -c01, a00) / det
    double v_a00 = v[4] * idet, v_a11 = v[2] * idet, v_c01 = -v[3] * idet;
    v_det -= (v[2] * a11 - v[3] * c01 + v[4] * a00) * idet * idet;
    v_a00 += v_det * a11, v_a11 += v_det * a00, v_c01 -= 2 * c01 * v_det;
    const double g00 = v_a00 + v_det_orig * c11, g11 = v_a11 + v_det_orig * c00;
    const double g01 = 0.5 * (v_c01 - 2 * c01 * v_det_orig); // the symmetric half: S2 is symmetric, c01 read once
    // S2 = J C J^T with G = [[g00, g01], [g01, g11]]:  v_J = 2 G J C = 2 G B,  v_C = J^T G J
    double GJ[6], v_J[6], v_C[9];
    for (int j = 0; j < 3; ++j) {
        GJ[j] = g00 * J[j] + g01 * J[3 + j];
        GJ[3 + j] = g01 * J[j] + g11 * J[3 + j];
        v_J[j] = 2 * (g00 * B[j] + g01 * B[3 + j]);
        v_J[3 + j] = 2 * (g01 * B[j] + g11 * B[3 + j]);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            v_C[3 * i + j] = J[i] * GJ[j] + J[3 + i] * GJ[3 + j];

    // ---- the camera model: (u, v, J) -> pc -----------------------------------------------------------------------------------------
    double v_x = 0, v_y = 0, v_z = 0;
    if constexpr (CAM == kGradPinhole) {
        // u = fx (x rz) + cx;  J00 = fx rz;  J02 = -fx (z c) rz rz with c = clamp(x rz)
        double v_rz = v[0] * V.fx * x + v[1] * V.fy * y + v_J[0] * V.fx + v_J[4] * V.fy;
        v_x = v[0] * V.fx * rz, v_y = v[1] * V.fy * rz;
        v_rz -= 2 * (v_J[2] * V.fx * tcx + v_J[5] * V.fy * tcy) * z * rz;
        v_z = -(v_J[2] * V.fx * tcx + v_J[5] * V.fy * tcy) * rz * rz;
        const double v_cx = -v_J[2] * V.fx * z * rz * rz, v_cy = -v_J[5] * V.fy * z * rz * rz;
        if (free_x)
            v_x += v_cx * rz, v_rz += v_cx * x;
        if (free_y)
            v_y += v_cy * rz, v_rz += v_cy * y;
        v_z -= v_rz * rz * rz;
    } else if constexpr (CAM == kGradOrtho) {
        v_x = v[0] * V.fx, v_y = v[1] * V.fy;
    } else {
        const double jx = V.fx * v_J[0], jy = V.fy * v_J[4], jxy = V.fx * v_J[1] + V.fy * v_J[3];
        const double v_s = v[0] * V.fx * x + v[1] * V.fy * y;
        v_x = v[0] * V.fx * fs - V.fx * v_J[2] * iR2;
        v_y = v[1] * V.fy * fs - V.fy * v_J[5] * iR2;
        double v_iR2 = -V.fx * v_J[2] * x - V.fy * v_J[5] * y;
        double v_xx = jx * fa + jy * fb, v_yy = jx * fb + jy * fa;
        const double v_a = jx * xx + jy * yy + jxy * xy;
        const double v_b = jx * yy + jy * xx - jxy * xy;
        const double v_xy = jxy * (fa - fb);
        double v_theta = v_s / rho + v_b / (rho * r2);
        double v_rho = -v_s * fs / rho - v_b * fb / rho;
        double v_r2 = -v_b * fb / r2 - v_a * fa / r2;
        v_z = v_a * iR2 / r2;
        v_iR2 += v_a * z / r2;
        const double v_den = -v_iR2 * iR2 * iR2;
        v_r2 += v_den;
        v_z += v_den * 2 * z;
        v_xx += v_r2, v_yy += v_r2;
        v_x += 2 * x * v_xx + v_xy * y;
        v_y += 2 * y * v_yy + v_xy * x;
        const double ih = 1.0 / (rho * rho + zz * zz); // theta = atan2(rho, z + eps)
        v_rho += v_theta * zz * ih;
        v_z -= v_theta * rho * ih;
        if (r > 0) // rho = sqrt(x^2 + y^2) + eps: on the axis itself the cone has no gradient; zero is taken
            v_x += v_rho * x / r, v_y += v_rho * y / r;
    }

    // ---- pc = R mean + t;  C = R Sigma R^T -----------------------------------------------------------------------------------------
    const double v_pc[3] = {v_x, v_y, v_z};
    for (int i = 0; i < 3; ++i) {
        g.t[i] = v_pc[i];
        g.mean[i] = R[i] * v_x + R[3 + i] * v_y + R[6 + i] * v_z;
    }
    // v_R = v_pc mean^T + 2 v_C A (v_C symmetric, A = R Sigma);  v_Sigma = R^T v_C R
    double T[9], v_S[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            g.R[3 * i + j] = v_pc[i] * mean[j] + 2 * (v_C[3 * i] * A[j] + v_C[3 * i + 1] * A[3 + j] + v_C[3 * i + 2] * A[6 + j]);
            T[3 * i + j] = v_C[3 * i] * R[j] + v_C[3 * i + 1] * R[3 + j] + v_C[3 * i + 2] * R[6 + j];
        }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            v_S[3 * i + j] = R[i] * T[j] + R[3 + i] * T[3 + j] + R[6 + i] * T[6 + j];
    // Sigma = M M^T: v_M = 2 v_Sigma M;  M = Q diag(s)
    double v_Q[9];
    for (int j = 0; j < 3; ++j)
        g.scale[j] = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double v_M = 2 * (v_S[3 * i] * M[j] + v_S[3 * i + 1] * M[3 + j] + v_S[3 * i + 2] * M[6 + j]);
            v_Q[3 * i + j] = v_M * scale[j];
            g.scale[j] += v_M * Q[3 * i + j];
        }
    // R(q) of the unit quaternion (w, x, y, z), then q / |q|
    const double v_w = 2 * (qx * (v_Q[7] - v_Q[5]) + qy * (v_Q[2] - v_Q[6]) + qz * (v_Q[3] - v_Q[1]));
    const double v_qx = 2 * (-2 * qx * (v_Q[4] + v_Q[8]) + qy * (v_Q[1] + v_Q[3]) + qz * (v_Q[2] + v_Q[6]) + qw * (v_Q[7] - v_Q[5]));
    const double v_qy = 2 * (qx * (v_Q[1] + v_Q[3]) - 2 * qy * (v_Q[0] + v_Q[8]) + qz * (v_Q[5] + v_Q[7]) + qw * (v_Q[2] - v_Q[6]));
    const double v_qz = 2 * (qx * (v_Q[2] + v_Q[6]) + qy * (v_Q[5] + v_Q[7]) - 2 * qz * (v_Q[0] + v_Q[4]) + qw * (v_Q[3] - v_Q[1]));
    const double along = qw * v_w + qx * v_qx + qy * v_qy + qz * v_qz;
    g.quat[0] = (v_w - qw * along) * iqn;
    g.quat[1] = (v_qx - qx * along) * iqn;
    g.quat[2] = (v_qy - qy * along) * iqn;
    g.quat[3] = (v_qz - qz * along) * iqn;
}

// The same product on the values as they are stored: float32 Gaussian, float32 view, float32 v_g2d row, widened on entry.
struct ProjViewF {
    float R[9], t[3], fx, fy, cx, cy;
    int W, H;
    float eps2d;
};

template <int CAM, bool AA>
GWBP_HD void project_vjp_stored(const ProjViewF &Vf, const float *mean, const float *quat, const float *scale, float opacity,
                                const float *v_g2d, ProjGrad &g)
{
    ProjView V;
    for (int i = 0; i < 9; ++i)
        V.R[i] = Vf.R[i];
    for (int i = 0; i < 3; ++i)
        V.t[i] = Vf.t[i];
    V.fx = Vf.fx, V.fy = Vf.fy, V.cx = Vf.cx, V.cy = Vf.cy, V.W = Vf.W, V.H = Vf.H, V.eps2d = Vf.eps2d;
    const double m[3] = {mean[0], mean[1], mean[2]}, q[4] = {quat[0], quat[1], quat[2], quat[3]};
    const double s[3] = {scale[0], scale[1], scale[2]};
    const double v[6] = {v_g2d[0], v_g2d[1], v_g2d[2], v_g2d[3], v_g2d[4], v_g2d[5]};
    project_vjp<CAM, AA>(V, m, q, s, (double)opacity, v, g);
}

} // namespace gwbp
