// Host build of csrc/mcmc_math.h: a stand-alone program (tests/test_mcmc_cpu.py builds and runs it, once plainly and once under
// -fsanitize=address,undefined) that evaluates the header's functions on the rows of a file and writes what they return, so that the
// numpy restatement (tests/mcmc_ref.py) can be held against the SAME text the device compiles, bit for bit.  Built with
// -ffp-contract=off, as the library is.
//
//   mcmc_host math IN OUT
//     IN : int64 n, float min_opacity, t_opa, scaler, then opacity[n] scaling[n][3] int32 ratio[n] means[n][3] rotation[n][4] z[n][3]
//     OUT: int64 weight[n] (mcmc_weight), float opacity'[n] scaling'[n][3] (mcmc_relocate), float gate[n], float moved[n][3] (mcmc_noise)
//   mcmc_host libm IN OUT
//     IN : int64 n, int32 op (0 expf, 1 logf, 2 powf), a[n], b[n]          OUT: float out[n]
//     this libm's values: the places where the restatement may differ, handed back so that it does not
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../3dgs-gradient-backprojection_amd/csrc/mcmc_math.h"

using namespace gwbp;

template <typename T> static bool read_array(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T> static bool write_array(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

static int run_math(FILE *f, FILE *o)
{
    int64_t n = 0;
    float par[3];
    if (fread(&n, sizeof n, 1, f) != 1 || fread(par, sizeof(float), 3, f) != 3 || n < 0 || n > (1 << 24))
        return 2;
    const size_t N = (size_t)n;
    std::vector<float> opacity, scaling, means, rotation, z;
    std::vector<int32_t> ratio;
    if (!(read_array(f, opacity, N) && read_array(f, scaling, 3 * N) && read_array(f, ratio, N) && read_array(f, means, 3 * N) &&
          read_array(f, rotation, 4 * N) && read_array(f, z, 3 * N)))
        return 2;
    std::vector<int64_t> weight(N);
    std::vector<float> o_new(N), s_new(3 * N), gate(N), moved(3 * N);
    for (size_t i = 0; i < N; ++i) {
        if (ratio[i] < 1 || ratio[i] > kMcmcMaxRatio)
            return 2;
        weight[i] = mcmc_weight(opacity[i], par[1]);
        mcmc_relocate(opacity[i], &scaling[3 * i], ratio[i], par[0], &o_new[i], &s_new[3 * i]);
        gate[i] = mcmc_gate(opacity[i]);
        mcmc_noise(&means[3 * i], &scaling[3 * i], &rotation[4 * i], opacity[i], &z[3 * i], par[2], &moved[3 * i]);
    }
    return write_array(o, weight) && write_array(o, o_new) && write_array(o, s_new) && write_array(o, gate) && write_array(o, moved) ? 0 : 2;
}

static int run_libm(FILE *f, FILE *o)
{
    int64_t n = 0;
    int32_t op = 0;
    if (fread(&n, sizeof n, 1, f) != 1 || fread(&op, sizeof op, 1, f) != 1 || n < 0 || n > (1 << 26) || op < 0 || op > 2)
        return 2;
    std::vector<float> a, b, out((size_t)n);
    if (!(read_array(f, a, (size_t)n) && read_array(f, b, (size_t)n)))
        return 2;
    for (size_t i = 0; i < (size_t)n; ++i)
        out[i] = op == 0 ? expf(a[i]) : op == 1 ? logf(a[i]) : powf(a[i], b[i]);
    return write_array(o, out) ? 0 : 2;
}

int main(int argc, char **argv)
{
    if (argc != 4 || (strcmp(argv[1], "math") && strcmp(argv[1], "libm"))) {
        fprintf(stderr, "usage: mcmc_host math|libm IN OUT\n");
        return 2;
    }
    FILE *f = fopen(argv[2], "rb");
    if (!f)
        return 2;
    FILE *o = fopen(argv[3], "wb");
    if (!o) {
        fclose(f);
        return 2;
    }
    const int rc = strcmp(argv[1], "math") ? run_libm(f, o) : run_math(f, o);
    fclose(f);
    return fclose(o) == 0 ? rc : 2;
}
