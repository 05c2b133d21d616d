// tools/bf16_bound_probe.hip -- evidence for the error model of the bound pass (csrc/hscmp_bound.h) on gfx950:
//   1. v_mfma_f32_32x32x16_bf16 forms every bf16 x bf16 product exactly (one non-zero product per output);
//   2. a chain of 12 MFMAs (192 products per output, as one atom group of the bound tile at W = 64) with adversarial
//      operands -- mixed exponents, heavy cancellation -- stays within gamma_192(2^-23) * sum|products| of the exact sum;
//      printed: the largest error in units of 2^-23 * sum|products| (the model allows 192);
//   3. what happens to subnormal bf16 operands and to products / sums below 2^-126.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -o tools/bf16_bound_probe tools/bf16_bound_probe.hip ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int NM = 12;

// a[m][lane][8], b[m][lane][8] bf16 bits; out[lane][16] = the accumulator after NM chained MFMAs from C = 0
__global__ void chain_kernel(const u16x8* a, const u16x8* b, float* out)
{
    const int lane = threadIdx.x;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int m = 0; m < NM; ++m)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[m * 64 + lane]), __builtin_bit_cast(bf16x8, b[m * 64 + lane]), acc, 0, 0, 0);
    for (int r = 0; r < 16; ++r) out[lane * 16 + r] = acc[r];
}

static unsigned short bf(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    return (unsigned short)(u >> 16);
}
static double fb(unsigned short h)
{
    unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return (double)f;
}

struct Run {
    std::vector<unsigned short> A, B;   // [NM][64][8]
    std::vector<float> out;
};

static void run(Run& r)
{
    unsigned short *da, *db;
    float* dout;
    hipMalloc(&da, r.A.size() * 2); hipMalloc(&db, r.B.size() * 2); hipMalloc(&dout, 64 * 16 * 4);
    hipMemcpy(da, r.A.data(), r.A.size() * 2, hipMemcpyHostToDevice);
    hipMemcpy(db, r.B.data(), r.B.size() * 2, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(64), 0, 0, (const u16x8*)da, (const u16x8*)db, dout);
    r.out.resize(64 * 16);
    hipMemcpy(r.out.data(), dout, 64 * 16 * 4, hipMemcpyDeviceToHost);
    hipFree(da); hipFree(db); hipFree(dout);
}

// exact value of output (row i, col j): sum over m, lane half h, element e of A[m][(h<<5)|i][e] * B[m][(h<<5)|j][e]
static void exact(const Run& r, int i, int j, long double& s, long double& sa)
{
    s = 0; sa = 0;
    for (int m = 0; m < NM; ++m)
        for (int h = 0; h < 2; ++h)
            for (int e = 0; e < 8; ++e) {
                const long double p = (long double)fb(r.A[(m * 64 + (h << 5) + i) * 8 + e]) * (long double)fb(r.B[(m * 64 + (h << 5) + j) * 8 + e]);
                s += p; sa += fabsl(p);
            }
}
static float got(const Run& r, int i, int j)
{
    const int h = (i >> 2) & 1, reg = (i & 3) + 4 * (i >> 3);
    return r.out[((h << 5) | j) * 16 + reg];
}

int main()
{
    std::mt19937 g(12345);
    std::uniform_real_distribution<float> U(1.0f, 2.0f);
    // 1. exact products: one non-zero term per output
    {
        int bad = 0, n = 0;
        for (int trial = 0; trial < 20; ++trial) {
            Run r;
            r.A.assign(NM * 64 * 8, 0); r.B.assign(NM * 64 * 8, 0);
            for (int lane = 0; lane < 32; ++lane) {
                r.A[lane * 8] = bf(std::ldexp(U(g), (int)(g() % 120) - 60) * ((g() & 1) ? 1 : -1));
                r.B[lane * 8] = bf(std::ldexp(U(g), (int)(g() % 120) - 60));
            }
            run(r);
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    long double s, sa;
                    exact(r, i, j, s, sa);
                    ++n;
                    if ((long double)got(r, i, j) != s) ++bad;
                }
        }
        printf("1. exact bf16 products: %d of %d outputs differ from the exact product\n", bad, n);
    }
    // 2. accumulation error of 192-product chains, adversarial operands
    {
        double worst = 0.0;
        int n = 0;
        for (int trial = 0; trial < 400; ++trial) {
            Run r;
            r.A.resize(NM * 64 * 8); r.B.resize(NM * 64 * 8);
            const int spread = trial % 4 == 0 ? 2 : trial % 4 == 1 ? 12 : trial % 4 == 2 ? 24 : 40;
            for (size_t q = 0; q < r.A.size(); ++q) {
                r.A[q] = bf(std::ldexp(U(g), (int)(g() % spread) - spread / 2) * ((g() & 1) ? 1 : -1));
                r.B[q] = bf(std::ldexp(U(g), (int)(g() % spread) - spread / 2));
            }
            if (trial % 2) {            // cancellation: the second half of every output's terms negates the first
                for (int m = NM / 2; m < NM; ++m)
                    for (int q = 0; q < 64 * 8; ++q) {
                        r.A[m * 512 + q] = r.A[(m - NM / 2) * 512 + q] ^ 0x8000;
                        r.B[m * 512 + q] = r.B[(m - NM / 2) * 512 + q];
                    }
                r.A[(NM - 1) * 512] ^= 0x0001;  // (not quite zero)
            }
            run(r);
            for (int i = 0; i < 32; ++i)
                for (int j = 0; j < 32; ++j) {
                    long double s, sa;
                    exact(r, i, j, s, sa);
                    const double e = (double)(fabsl((long double)got(r, i, j) - s) / (sa * 0x1p-23L));
                    worst = std::max(worst, e);
                    ++n;
                }
        }
        printf("2. accumulation: %d outputs of 192 products, largest |acc - exact| = %.4f x 2^-23 sum|p| (model: <= 192)\n", n, worst);
    }
    // 3. subnormals
    {
        Run r;
        r.A.assign(NM * 64 * 8, 0); r.B.assign(NM * 64 * 8, 0);
        const float cases[4][2] = {{0x1p-130f, 1.0f}, {0x1p-70f, 0x1p-70f}, {0x1p-63f, 0x1p-63f}, {0x1p-100f, 0x1p-20f}};
        for (int c = 0; c < 4; ++c) { r.A[c * 8] = bf(cases[c][0]); r.B[c * 8] = bf(cases[c][1]); }
        // a sum that cancels below 2^-126: 2^-100 * 1 - (2^-100 - 2^-107) * 1 = 2^-107... scaled to land at 2^-130
        r.A[4 * 8] = bf(0x1p-60f); r.B[4 * 8] = bf(0x1p-60f);
        r.A[4 * 8 + 1] = bf(-0x1.fep-61f); r.B[4 * 8 + 1] = bf(0x1p-60f);
        run(r);
        const char* names[5] = {"subnormal operand 2^-130 x 1", "product 2^-70 x 2^-70 = 2^-140", "product 2^-63 x 2^-63 = 2^-126",
                                "product 2^-100 x 2^-20 = 2^-120", "sum 2^-120 - 0x1.fep-121 = 2^-128"};
        for (int c = 0; c < 5; ++c) {
            long double s, sa;
            exact(r, c, c, s, sa);
            printf("3. %-36s -> %a (exact %La)\n", names[c], got(r, c, c), s);
        }
    }
    return 0;
}
