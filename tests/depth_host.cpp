// Host build of csrc/depth_math.h: a stand-alone program (tests/test_depth_loss_cpu.py builds and runs it, once plainly and once under
// -fsanitize=address,undefined) that runs the header's functions over one image, a list of points and a depth map, and writes every
// per-point and per-pixel value, so that the numpy restatement (tests/depth_loss_ref.py) can be held against the SAME text the device
// compiles, bit for bit.  Built with -ffp-contract=off, as the library is.  The corner fetch (which pixel, inside or not) is the
// kernels' rule restated: float comparisons before any conversion.
//
//   depth_host IN OUT
//     IN : int32 H, W, M, kind, float c_points, c_map, then float A[H W], a[H W], points[M][2], g[M], depth_map[H W], weights[H W]
//     OUT: per point float d, t, v_A[4], v_a[4] (zeros for a corner outside the image), then per pixel float t, v_A, v_a (zeros for
//          a pixel that is not valid)
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../3dgs-gradient-backprojection_amd/csrc/depth_math.h"

using namespace gwbp;

static bool read_floats(FILE *f, std::vector<float> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(float), n, f) == n;
}

struct Corner {
    bool in;
    size_t pix;
    float A, a, e;
};

static Corner fetch(const std::vector<float> &A, const std::vector<float> &a, int H, int W, float yf, float xf)
{
    Corner c = {false, 0, 0.0f, 0.0f, 0.0f};
    c.in = yf >= 0.0f && yf < (float)H && xf >= 0.0f && xf < (float)W;
    if (c.in) {
        c.pix = (size_t)(int)yf * (size_t)W + (size_t)(int)xf;
        c.A = A[c.pix], c.a = a[c.pix];
        c.e = depth_expected(c.A, c.a);
    }
    return c;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: depth_host IN OUT\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    int32_t dims[4] = {0, 0, 0, 0};
    float cs[2] = {0.0f, 0.0f};
    int rc = 2;
    std::vector<float> A, a, pts, g, gmap, wmap, out;
    if (fread(dims, sizeof(int32_t), 4, f) == 4 && fread(cs, sizeof(float), 2, f) == 2 && dims[0] >= 1 && dims[0] <= 4096 &&
        dims[1] >= 1 && dims[1] <= 4096 && dims[2] >= 0 && dims[2] <= (1 << 20) && (dims[3] == kDepthDisparity || dims[3] == kDepthDepth)) {
        const int H = dims[0], W = dims[1], M = dims[2], kind = dims[3];
        const size_t P = (size_t)H * (size_t)W;
        if (read_floats(f, A, P) && read_floats(f, a, P) && read_floats(f, pts, 2 * (size_t)M) && read_floats(f, g, (size_t)M) &&
            read_floats(f, gmap, P) && read_floats(f, wmap, P)) {
            out.reserve(10 * (size_t)M + 3 * P);
            for (int i = 0; i < M; ++i) {
                const float x = pts[2 * (size_t)i], y = pts[2 * (size_t)i + 1];
                const float x0 = floorf(x), y0 = floorf(y);
                const Corner c[4] = {fetch(A, a, H, W, y0, x0), fetch(A, a, H, W, y0, x0 + 1.0f), fetch(A, a, H, W, y0 + 1.0f, x0),
                                     fetch(A, a, H, W, y0 + 1.0f, x0 + 1.0f)};
                const DepthSample S = depth_sample(x, y, x0, y0, c[0].e, c[1].e, c[2].e, c[3].e, g[(size_t)i]);
                float v_e[4], v_A[4] = {0.0f, 0.0f, 0.0f, 0.0f}, v_a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                depth_corner_shares(S, depth_sample_grad(S, cs[0]), v_e);
                for (int k = 0; k < 4; ++k)
                    if (c[k].in)
                        depth_expected_grad(c[k].A, c[k].a, v_e[k], v_A[k], v_a[k]);
                out.push_back(S.d), out.push_back(S.t);
                for (int k = 0; k < 4; ++k)
                    out.push_back(v_A[k]);
                for (int k = 0; k < 4; ++k)
                    out.push_back(v_a[k]);
            }
            for (size_t p = 0; p < P; ++p) {
                float t = 0.0f, v_A = 0.0f, v_a = 0.0f;
                if (gmap[p] > 0.0f && wmap[p] > 0.0f) {
                    const float e = depth_expected(A[p], a[p]);
                    t = fabsf(depth_map_residual(kind, e, gmap[p]));
                    depth_expected_grad(A[p], a[p], depth_map_grad(kind, e, gmap[p], wmap[p] * cs[1]), v_A, v_a);
                }
                out.push_back(t), out.push_back(v_A), out.push_back(v_a);
            }
            FILE *o = fopen(argv[2], "wb");
            if (o) {
                rc = out.empty() || fwrite(out.data(), sizeof(float), out.size(), o) == out.size() ? 0 : 2;
                if (fclose(o) != 0)
                    rc = 2;
            }
        }
    }
    fclose(f);
    return rc;
}
