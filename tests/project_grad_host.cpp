// Host build of csrc/project_grad.h for tests/test_project_grad_cpu.py: the per-Gaussian vjp k_project_bwd evaluates, looped over N
// rows with the kernel's rules -- a hidden row stores zeros, adds nothing to the view sums and is never evaluated -- but with the
// float64 values handed out unrounded, so that the test can hold them against torch's float64 autograd.
#include <stdint.h>

#include "../3dgs-gradient-backprojection_amd/csrc/project_grad.h"

using namespace gwbp;

template <int CAM, bool AA>
static void run(int64_t n, const ProjViewF &V, const float *means, const float *quats, const float *scales, const float *opac,
                const uint8_t *visible, const float *v_g2d, double *v_means, double *v_quats, double *v_scales, double *v_opac,
                double *v_viewmat)
{
    for (int k = 0; k < 12; ++k)
        v_viewmat[k] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        ProjGrad g = {};
        if (visible[i]) {
            project_vjp_stored<CAM, AA>(V, means + 3 * i, quats + 4 * i, scales + 3 * i, opac[i], v_g2d + 6 * i, g);
            for (int k = 0; k < 9; ++k)
                v_viewmat[k] += g.R[k];
            for (int k = 0; k < 3; ++k)
                v_viewmat[9 + k] += g.t[k];
        }
        for (int k = 0; k < 3; ++k)
            v_means[3 * i + k] = g.mean[k], v_scales[3 * i + k] = g.scale[k];
        for (int k = 0; k < 4; ++k)
            v_quats[4 * i + k] = g.quat[k];
        v_opac[i] = g.opacity;
    }
}

// view16: R[9] row-major, t[3], fx, fy, cx, cy.  Returns 0, or -1 for an unknown camera model.
extern "C" int project_grad_host(int64_t n, int camera_model, int antialiased, const float *view16, int width, int height, float eps2d,
                                 const float *means, const float *quats, const float *scales, const float *opac,
                                 const uint8_t *visible, const float *v_g2d, double *v_means, double *v_quats, double *v_scales,
                                 double *v_opac, double *v_viewmat)
{
    ProjViewF V;
    for (int k = 0; k < 9; ++k)
        V.R[k] = view16[k];
    for (int k = 0; k < 3; ++k)
        V.t[k] = view16[9 + k];
    V.fx = view16[12], V.fy = view16[13], V.cx = view16[14], V.cy = view16[15];
    V.W = width, V.H = height, V.eps2d = eps2d;
#define RUN(CAM)                                                                                                                     \
    if (antialiased)                                                                                                                 \
        run<CAM, true>(n, V, means, quats, scales, opac, visible, v_g2d, v_means, v_quats, v_scales, v_opac, v_viewmat);             \
    else                                                                                                                             \
        run<CAM, false>(n, V, means, quats, scales, opac, visible, v_g2d, v_means, v_quats, v_scales, v_opac, v_viewmat);            \
    return 0;
    switch (camera_model) {
    case kGradPinhole: RUN(kGradPinhole)
    case kGradOrtho: RUN(kGradOrtho)
    case kGradFisheye: RUN(kGradFisheye)
    }
#undef RUN
    return -1;
}
