// Stand-alone check of the wide loop's shape rule (hscmp_wide_plan / wide_shape of hscmp_api.hip: host arithmetic, no device) for a
// host-side sanitizer build; run on the CPU.  From the repository root:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_device -O0 \
//         -Xarch_device -g0 -Wno-unused-function -o wide_plan_check hierarchical-sparse-coding_amd/csrc/hscmp_api.hip tools/wide_plan_check.cpp
//   ./wide_plan_check        -> "11200 plans, 0 bad" and no sanitizer report
#include "../include/hscmp.h"
#include <cmath>
#include <cstdio>
int main()
{
    int bad = 0, n = 0;
    const int Ws[] = {8, 12, 16, 20, 32, 40, 64}, Ks[] = {1, 32, 256, 1000}, Bs[] = {1, 16, 17, 4096}, Ts[] = {40, 4096, 65536, 1048576, 16384 * 64 + 64};
    const int nbs[] = {-1, 1, 5, 10, 100000};
    for (int W : Ws) for (int K : Ks) for (int B : Bs) for (int T : Ts) for (int nb : nbs) for (int w = 0; w < 2; ++w) for (int d = 0; d < 2; ++d) {
        hscmp_params p{};
        p.nb_nonzero_coefs = -1; p.nb_blocks = nb; p.tolerance_snr = 20.0; p.tolerance_residual_scale = NAN; p.null_coeff_thres = 1e-16;
        p.eps = 1e-7; p.max_events = 4096; p.max_rounds = 0;
        int32_t out[4] = {-1, -1, -1, -1};
        const int rc = hscmp_wide_plan(K, W, 1, d ? HSCMP_F64 : HSCMP_F32, w, B, T, &p, out);
        ++n;
        if (rc == 0 && (out[0] < out[1] || (out[0] && (out[2] > 16384 || out[3] > 158 * 1024 || d)))) { ++bad; std::printf("bad: K=%d W=%d B=%d T=%d nb=%d\n", K, W, B, T, nb); }
    }
    int32_t out[4];
    bad += hscmp_wide_plan(32, 16, 1, HSCMP_F32, 0, 1, 4096, nullptr, out) == 0;
    bad += hscmp_wide_counters(nullptr, out) == 0;
    std::printf("%d plans, %d bad\n", n, bad);
    return bad != 0;
}
