// Host build of csrc/densify_math.h: a stand-alone program (tests/test_densify_cpu.py builds and runs it) that evaluates the header's
// three functions on the rows of a file and writes what they return, so that the numpy restatement (tests/densify_ref.py) can be held
// against the SAME text the device compiles, bit for bit.  Built with -ffp-contract=off, as the library is.
//
//   densify_host IN OUT
//   IN : int64 n, int32 prune_big, float t_grad, t_small, t_big, t_opa, log16, sx, sy, then float arrays
//        grad2d[n] count[n] scaling[n][3] opacity[n] means[n][3] rotation[n][4] noise[n][3] gx[n] gy[n]
//   OUT: int32 kind[n], float norm[n], float split[n][3] (densify_split of every row), float exps[n][3] (this libm's expf of the
//        scaling: the one place where the restatement may differ, handed back so that it does not)
// It can also be built with -fsanitize=address,undefined and run by hand: it has its own main and reads nothing but its file.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../3dgs-gradient-backprojection_amd/csrc/densify_math.h"

using namespace gwbp;

static bool read_floats(FILE *f, std::vector<float> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(float), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: densify_host IN OUT\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    int64_t n = 0;
    int32_t prune_big = 0;
    float par[7];
    if (fread(&n, sizeof n, 1, f) != 1 || fread(&prune_big, sizeof prune_big, 1, f) != 1 || fread(par, sizeof(float), 7, f) != 7 || n < 0 ||
        n > (1 << 24)) {
        fclose(f);
        return 2;
    }
    const size_t N = (size_t)n;
    std::vector<float> grad2d, count, scaling, opacity, means, rotation, noise, gx, gy;
    const bool ok = read_floats(f, grad2d, N) && read_floats(f, count, N) && read_floats(f, scaling, 3 * N) && read_floats(f, opacity, N) &&
                    read_floats(f, means, 3 * N) && read_floats(f, rotation, 4 * N) && read_floats(f, noise, 3 * N) && read_floats(f, gx, N) &&
                    read_floats(f, gy, N);
    fclose(f);
    if (!ok)
        return 2;
    DensifyThresholds T;
    T.t_grad = par[0], T.t_small = par[1], T.t_big = par[2], T.t_opa = par[3], T.log16 = par[4], T.prune_big = prune_big != 0;
    const float sx = par[5], sy = par[6];
    std::vector<int32_t> kind(N);
    std::vector<float> norm(N), split(3 * N), exps(3 * N);
    for (size_t i = 0; i < N; ++i) {
        kind[i] = densify_kind(grad2d[i], count[i], scaling[3 * i], scaling[3 * i + 1], scaling[3 * i + 2], opacity[i], T);
        norm[i] = densify_norm(gx[i], gy[i], sx, sy);
        densify_split(&means[3 * i], &scaling[3 * i], &rotation[4 * i], &noise[3 * i], &split[3 * i]);
        for (int j = 0; j < 3; ++j)
            exps[3 * i + j] = expf(scaling[3 * i + j]);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    const bool wrote = (N == 0) || (fwrite(kind.data(), sizeof(int32_t), N, o) == N && fwrite(norm.data(), sizeof(float), N, o) == N &&
                                    fwrite(split.data(), sizeof(float), 3 * N, o) == 3 * N && fwrite(exps.data(), sizeof(float), 3 * N, o) == 3 * N);
    fclose(o);
    return wrote ? 0 : 2;
}
