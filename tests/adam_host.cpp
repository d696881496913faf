// Host build of csrc/adam_math.h: a stand-alone program (tests/test_adam_cpu.py builds and runs it, once plainly and once under
// -fsanitize=address,undefined) that runs the header's adam_element over a table for a sequence of gradients and writes what it leaves,
// so that the numpy restatement (tests/adam_ref.py) can be held against the SAME text the device compiles, bit for bit.  Built with
// -ffp-contract=off, as the library is.
//
//   adam_host IN OUT
//     IN : int64 n, int32 steps, int32 0, float64 b1, b2, float eps, float 0, then float step_size[steps], sqrt_bc2[steps] (the caller's,
//          float64 rounded once, as gwbp_adam_step takes them), p[n], m[n], v[n], g[steps][n]
//     OUT: float p[n], m[n], v[n] after the last step
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../3dgs-gradient-backprojection_amd/csrc/adam_math.h"

using namespace gwbp;

static bool read_floats(FILE *f, std::vector<float> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(float), n, f) == n;
}

static bool write_floats(FILE *f, const std::vector<float> &v) { return v.empty() || fwrite(v.data(), sizeof(float), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: adam_host IN OUT\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    int64_t n = 0;
    int32_t steps[2] = {0, 0};
    double betas[2] = {0.0, 0.0};
    float eps[2] = {0.0f, 0.0f};
    int rc = 2;
    std::vector<float> step_size, sqrt_bc2, p, m, v, g;
    if (fread(&n, sizeof n, 1, f) == 1 && fread(steps, sizeof(int32_t), 2, f) == 2 && fread(betas, sizeof(double), 2, f) == 2 &&
        fread(eps, sizeof(float), 2, f) == 2 && n >= 0 && n <= (1 << 24) && steps[0] >= 0 && steps[0] <= 4096) {
        const size_t N = (size_t)n, T = (size_t)steps[0];
        if (read_floats(f, step_size, T) && read_floats(f, sqrt_bc2, T) && read_floats(f, p, N) && read_floats(f, m, N) &&
            read_floats(f, v, N) && read_floats(f, g, T * N)) {
            for (size_t t = 0; t < T; ++t) {
                const AdamScalars S = AdamScalars::make(step_size[t], sqrt_bc2[t], betas[0], betas[1], eps[0]);
                for (size_t i = 0; i < N; ++i)
                    adam_element(p[i], g[t * N + i], m[i], v[i], S);
            }
            FILE *o = fopen(argv[2], "wb");
            if (o) {
                rc = write_floats(o, p) && write_floats(o, m) && write_floats(o, v) ? 0 : 2;
                if (fclose(o) != 0)
                    rc = 2;
            }
        }
    }
    fclose(f);
    return rc;
}
