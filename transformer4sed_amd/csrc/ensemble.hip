// Score-level ensembling for a bank of weight rows (transformer4sed_amd/ensemble.py):
//
//   sed_ensemble_bank    members x_m [n, T_m, C] (m < M <= 8, a device table of pointers) -> out [W, n, T, C] (W <= 64),
//                        out[r] = the combination of the members, each resampled to T frames, under the weight row w[r, :, :]
//
// Frame-rate match: member m at output frame t is read at the half-pixel coordinate of F.interpolate(size=T, mode="linear",
// align_corners=False), found in INTEGERS: num = max((2 t + 1) T_m - T, 0), i0 = num / (2 T), i1 = min(i0 + 1, T_m - 1),
// rem = num - 2 T i0, lambda = float(rem) / float(2 T).  Where rem == 0 or i1 == i0 the value is x[i0] itself (T_m == T: a copy; T_m == 1:
// a broadcast), otherwise v = x[i0] + lambda (x[i1] - x[i0]).
//   mode 0 (arithmetic): y = w_0 v_0, then y = y + w_m v_m for m = 1 .. M - 1; every product and every sum is one fp32 operation rounded
//           to nearest, never fused (__fmul_rn / __fadd_rn / __fsub_rn, and the file is built with -ffp-contract=off): a float32 host
//           restatement in this order gives the same bits.
//   mode 1 (logit mean): y = sigmoid(sum_m w_m logit(clamp(v_m, LO, HI))), LO = 1e-7f, HI = 1 - 1e-7f (the fp32 numbers).  In float64
//           from the loaded fp32 values on, rounded to fp32 once at the end: logit amplifies a rounding of v by 1 / (v (1 - v)), which an
//           fp32 interpolation would turn into errors of 1e-3 for scores within 1e-6 of 1.  Not pinned bit for bit.
//   rounding: dec_scale > 0: y = rintf(y dec_scale) / dec_scale (dec_scale = 10^decimals), three fp32 operations.
//
// Work split: a thread owns one flat (clip, frame, class) element: it loads each member's two neighbours ONCE, keeps the M values in
// registers and produces all W rows from them -- the members are read once for the whole bank, and a wave's W stores each cover 64
// consecutive floats of one output plane.  Consecutive lanes are consecutive FLAT elements (C = 10 rows are not 16-byte aligned).  The
// weights [W, M, C] sit in LDS.  Grid-stride loop over at most ENS_MAX_GRID workgroups; no workgroup waits for another, no atomics,
// nothing kept between launches; every output element is written by one thread.
#include "common.h"

#define ENS_MAX_M 8
#define ENS_MAX_W 64
#define ENS_THREADS 256
#define ENS_MAX_GRID 1024                // workgroups of one launch: one grid pass is ENS_MAX_GRID * ENS_THREADS elements
#define ENS_MAX_WEIGHTS 32768            // W * M * C floats of LDS (128 KB of the CU's 160 KB)

template <int MODE>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_bank_kernel(const float* const* __restrict__ members, const int* __restrict__ Tm,
                                                                    const float* __restrict__ w, float* __restrict__ out, int M, int W,
                                                                    int64_t N, int T, int C, float dec_scale) {
    extern __shared__ __attribute__((aligned(16))) float ens_w[];                    // [W, M, C]
    __shared__ const float* mp[ENS_MAX_M];
    __shared__ int mt[ENS_MAX_M];
    const int tid = threadIdx.x;
    for (int i = tid; i < W * M * C; i += ENS_THREADS) ens_w[i] = w[i];
    if (tid < M) {
        mp[tid] = members[tid];
        const int tm = Tm[tid];
        mt[tid] = tm < 1 ? 1 : tm;
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * ENS_THREADS, T2 = 2 * (int64_t)T;
    const float inv_den = (float)T2;
    for (int64_t e = (int64_t)blockIdx.x * ENS_THREADS + tid; e < N; e += stride) {
        const int64_t r = e / C, b = r / T;
        const int c = (int)(e - r * C), t = (int)(r - b * T);
        float v[ENS_MAX_M];
        double u[ENS_MAX_M];
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) {
            v[m] = 0.f;
            u[m] = 0.0;
            if (m < M) {
                const int tm = mt[m];
                int64_t num = (2 * (int64_t)t + 1) * tm - T;
                num = num < 0 ? 0 : num;
                int64_t i0 = num / T2;
                i0 = i0 > tm - 1 ? tm - 1 : i0;                                      // (holds already for T_m <= T; keeps a bad T_m in bounds)
                const int64_t i1 = i0 + 1 < tm ? i0 + 1 : tm - 1;
                const int64_t rem = num - T2 * i0;
                const float* p = mp[m] + (b * tm) * C + c;
                const float x0 = p[i0 * C];
                if (rem == 0 || i1 == i0) {
                    v[m] = x0;
                    if (MODE == 1) u[m] = (double)x0;
                } else {
                    const float x1 = p[i1 * C];
                    if (MODE == 0) {
                        const float lam = (float)rem / inv_den;
                        v[m] = __fadd_rn(x0, __fmul_rn(lam, __fsub_rn(x1, x0)));
                    } else {
                        u[m] = (double)x0 + ((double)rem / (double)T2) * ((double)x1 - (double)x0);
                    }
                }
                if (MODE == 1) {
                    const double lo = (double)1e-7f, hi = (double)(1.0f - 1e-7f);
                    double q = u[m];
                    q = q < lo ? lo : (q > hi ? hi : q);                            // (a NaN stays a NaN)
                    u[m] = log(q) - log1p(-q);
                }
            }
        }
        for (int row = 0; row < W; ++row) {
            const float* wr = ens_w + (size_t)row * M * C + c;
            float y;
            if (MODE == 0) {
                y = __fmul_rn(wr[0], v[0]);
#pragma unroll
                for (int m = 1; m < ENS_MAX_M; ++m)
                    if (m < M) y = __fadd_rn(y, __fmul_rn(wr[m * C], v[m]));
            } else {
                double z = (double)wr[0] * u[0];
#pragma unroll
                for (int m = 1; m < ENS_MAX_M; ++m)
                    if (m < M) z += (double)wr[m * C] * u[m];
                y = (float)(1.0 / (1.0 + exp(-z)));
            }
            if (dec_scale > 0.f) y = rintf(__fmul_rn(y, dec_scale)) / dec_scale;
            out[(size_t)row * N + e] = y;
        }
    }
}

extern "C" int sed_ensemble_bank(const float* const* members, const int* Tm, const float* w, float* out, int M, int W, int n, int T, int C,
                                 int mode, int decimals, hipStream_t stream) {
    (void)hipGetLastError();
    if (members == nullptr || Tm == nullptr || w == nullptr || out == nullptr) return SED_ERR_ARG;
    if (M < 1 || M > ENS_MAX_M || W < 1 || W > ENS_MAX_W || n < 1 || T < 1 || C < 1 || mode < 0 || mode > 1) return SED_ERR_ARG;
    if (decimals < -1 || decimals > 9) return SED_ERR_ARG;
    if ((int64_t)W * M * C > ENS_MAX_WEIGHTS) return SED_ERR_ARG;
    const int64_t N = (int64_t)n * T * C;
    if (N > ((int64_t)1 << 40)) return SED_ERR_ARG;
    float dec_scale = 0.f;
    if (decimals >= 0) {
        dec_scale = 1.f;
        for (int i = 0; i < decimals; ++i) dec_scale *= 10.f;                       // (exact in fp32 up to 10^10)
    }
    const size_t lds = (size_t)W * M * C * sizeof(float);
    const int grid = grid_for((size_t)N, ENS_THREADS, ENS_MAX_GRID);
    if (mode == 0) {
        static size_t attr = 0;
        if (lds > 65536 && lds > attr) {
            (void)hipFuncSetAttribute((const void*)ensemble_bank_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr = lds;
        }
        hipLaunchKernelGGL(ensemble_bank_kernel<0>, dim3((unsigned)grid), dim3(ENS_THREADS), lds, stream, members, Tm, w, out, M, W, N, T, C,
                           dec_scale);
    } else {
        static size_t attr = 0;
        if (lds > 65536 && lds > attr) {
            (void)hipFuncSetAttribute((const void*)ensemble_bank_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            attr = lds;
        }
        hipLaunchKernelGGL(ensemble_bank_kernel<1>, dim3((unsigned)grid), dim3(ENS_THREADS), lds, stream, members, Tm, w, out, M, W, N, T, C,
                           dec_scale);
    }
    return sed_check_launch();
}
