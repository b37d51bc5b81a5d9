// PMAM tokenizer (full-covariance Gaussian mixture over frame features), gfx950.
//
// Replaces what recipes/desed/pmam/gmm.py and generate_pseudo_label.py get from pycave's GaussianMixture (covariance_type "full"): the
// E-step over every frame.  With Sigma_k = L_k L_k^T the log-density of a frame is  logc_k - 0.5 |L_k^-1 (x - mu_k)|^2, so the hot
// product is, per component, a [N, D] x [D, D] GEMM against the LOWER TRIANGULAR P_k = L_k^-1 followed by a row sum of squares:
//   * sed_gmm_maha          maha[n, k] = sum_j (sum_d X[n, d] P_k[j, d] + b_k[j])^2,  b_k = -P_k mu_k, on v_mfma_f32_32x32x2_f32 (exact fp32
//                           products, fp32 accumulation: in 768 dimensions the term is ~768 and differences of order 1 decide the posterior,
//                           16-bit operands are four orders short).  The whitened row never exists in memory and the d tiles above the
//                           diagonal of P_k are skipped.
//   * sed_gmm_resp          row softmax of logc - 0.5 maha, log-sum-exp, arg-max and per-workgroup column sums (fixed order)
//   * sed_gmm_colsum_reduce the per-workgroup sums -> [K] in a fixed order (no float atomics: N_k is bit-reproducible)
//   * sed_gmm_center_scale  A[n, :] = sqrt(w[n]) (X[n, :] - mu): the operand of the M-step's covariance product A^T A (sed_gemm_f32)
// Only ordinary launches on the caller's stream; a kernel boundary is the only ordering between workgroups.
#include "common.h"
#include "../../include/sed_hip.h"

// ---------------------------------------------------------------------------------------------------------------------
// sed_gmm_maha.  Workgroup = 256 threads = 4 waves, 128 rows of X against one component; wave w owns rows 32 w .. 32 w + 31 and BOTH 32-column
// accumulators of the current 64-wide j tile, so the sum over j of a row stays inside one wave: 16 partial sums per lane carried in
// registers across the j tiles, one butterfly over the 32 column lanes at the end, one store per (n, k).  Tiles of 32 along d are staged
// k-major in LDS (pitch 129 / 65 floats: the scalar writes of a float4 and the 32-lane fragment reads are conflict free, as in
// gemm_f32_kernel of dasm.hip), the next tile's global loads are in flight during the 32 MFMAs of the current one.  The (j tile, d tile)
// walk is one flat sequence: for j tile j0 only d < min(D, j0 + 64) is visited -- P_k is zero above its diagonal by contract.
// Launch geometry: grid = (min(ceil(N / 128), 1024), K); a workgroup strides over the row blocks.
// ---------------------------------------------------------------------------------------------------------------------
#define GM_BM 128
#define GM_BN 64
#define GM_BK 32
#define GM_LDA 129
#define GM_LDB 65
#define GM_MAX_ROW_BLOCKS 1024
typedef __attribute__((ext_vector_type(16))) float gm_f32x16;

template <bool VEC>
__global__ __launch_bounds__(256) void gmm_maha_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ b,
                                                       float* __restrict__ maha, long long N, int D, int K, long long ldx, long long nrb) {
    __shared__ float As[GM_BK * GM_LDA], Bs[GM_BK * GM_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
    const int k = blockIdx.y;
    const float* Pk = P + (size_t)k * D * D;
    const float* bk = b + (size_t)k * D;
    const int l_hi = tid >> 3, l_lo = (tid & 7) * 4;
    for (long long rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
        const long long m0 = rb * GM_BM;
        float4 ra[4], rp[2];
        auto gload = [&](int j0, int k0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long row = m0 + l_hi + 32 * i;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < N) {                                                    // (k0 + l_lo + 3 < D: D is a multiple of the d tile)
                    const float* p = X + row * ldx + k0 + l_lo;
                    if (VEC) v = *reinterpret_cast<const float4*>(p);
                    else { v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3]; }
                }
                ra[i] = v;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int j = j0 + l_hi + 32 * i;
                rp[i] = j < D ? *reinterpret_cast<const float4*>(Pk + (size_t)j * D + k0 + l_lo) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        auto lstore = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = l_hi + 32 * i;
                As[(l_lo + 0) * GM_LDA + r] = ra[i].x; As[(l_lo + 1) * GM_LDA + r] = ra[i].y; As[(l_lo + 2) * GM_LDA + r] = ra[i].z; As[(l_lo + 3) * GM_LDA + r] = ra[i].w;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int r = l_hi + 32 * i;
                Bs[(l_lo + 0) * GM_LDB + r] = rp[i].x; Bs[(l_lo + 1) * GM_LDB + r] = rp[i].y; Bs[(l_lo + 2) * GM_LDB + r] = rp[i].z; Bs[(l_lo + 3) * GM_LDB + r] = rp[i].w;
            }
        };
        float ss[16];
        gm_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { ss[r] = 0.f; acc0[r] = 0.f; acc1[r] = 0.f; }
        const int fa = half * GM_LDA + wave * 32 + col, fb = half * GM_LDB + col;
        int j0 = 0, k0 = 0;
        gload(0, 0);
        while (j0 < D) {
            lstore();
            __syncthreads();
            const int kend = min(D, j0 + GM_BN);
            int nj = j0, nk = k0 + GM_BK;
            if (nk >= kend) { nj = j0 + GM_BN; nk = 0; }
            if (nj < D) gload(nj, nk);
#pragma unroll
            for (int kk = 0; kk < GM_BK; kk += 2) {
                const float a = As[kk * GM_LDA + fa];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk * GM_LDB + fb], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Bs[kk * GM_LDB + fb + 32], acc1, 0, 0, 0);
            }
            __syncthreads();
            if (nk == 0) {                                                        // this j tile is complete: square, add, start the next
                const int ja = j0 + col, jb = ja + 32;
                if (ja < D) {
                    const float bj = bk[ja];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { const float v = acc0[r] + bj; ss[r] += v * v; }
                }
                if (jb < D) {
                    const float bj = bk[jb];
#pragma unroll
                    for (int r = 0; r < 16; ++r) { const float v = acc1[r] + bj; ss[r] += v * v; }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
            }
            j0 = nj; k0 = nk;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = ss[r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);           // (stays inside a 32-lane half: one row per half and register)
            const long long row = m0 + wave * 32 + mfma32_row(r, half);
            if (col == 0 && row < N) maha[row * K + k] = v;
        }
    }
}

extern "C" int sed_gmm_maha(const float* X, const float* P, const float* b, float* maha, int64_t N, int D, int K, int64_t ldx,
                            hipStream_t stream) {
    (void)hipGetLastError();
    if (!X || !P || !b || !maha || N < 1 || D < 32 || D > 768 || (D % 32) || K < 1 || K > 64 || ldx < D) return SED_ERR_ARG;
    if ((uintptr_t)P & 15) return SED_ERR_ARG;
    const long long nrb = (N + GM_BM - 1) / GM_BM;
    const dim3 grid((unsigned)(nrb < GM_MAX_ROW_BLOCKS ? nrb : GM_MAX_ROW_BLOCKS), K);
    const bool vec = !((uintptr_t)X & 15) && !(ldx & 3);
    if (vec) hipLaunchKernelGGL((gmm_maha_kernel<true>), grid, dim3(256), 0, stream, X, P, b, maha, (long long)N, D, K, (long long)ldx, nrb);
    else hipLaunchKernelGGL((gmm_maha_kernel<false>), grid, dim3(256), 0, stream, X, P, b, maha, (long long)N, D, K, (long long)ldx, nrb);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// sed_gmm_resp: one wave per row, lane = component (K <= 64).  Workgroup g, wave w takes rows 4 g + w, + 4 n_blocks, ...: the rows a lane
// adds into its column sum and their order depend only on (N, n_blocks), the four waves are added in wave order through LDS.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_resp_kernel(const float* __restrict__ maha, const float* __restrict__ logc, float* __restrict__ resp,
                                                       float* __restrict__ logp, int* __restrict__ argmax, float* __restrict__ colsum_part,
                                                       long long N, int K) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float lc = lane < K ? logc[lane] : 0.f;
    float csum = 0.f;
    for (long long n = (long long)blockIdx.x * 4 + wave; n < N; n += (long long)gridDim.x * 4) {
        const float s = lane < K ? lc - 0.5f * maha[n * K + lane] : -INFINITY;
        const float m = wave_max(s);
        const float e = lane < K ? expf(s - m) : 0.f;
        const float sum = wave_sum(e);
        const float r = e / sum;
        csum += r;
        if (resp != nullptr && lane < K) resp[n * K + lane] = r;
        if (lane == 0) {
            if (logp != nullptr) logp[n] = m + logf(sum);
        }
        if (argmax != nullptr) {
            const unsigned long long hit = __ballot(s == m);
            if (lane == 0) argmax[n] = hit ? __ffsll((long long)hit) - 1 : 0;
        }
    }
    if (colsum_part == nullptr) return;
    part[wave][lane] = csum;
    __syncthreads();
    if (threadIdx.x < K) colsum_part[(size_t)blockIdx.x * K + threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
}

extern "C" int sed_gmm_resp(const float* maha, const float* logc, float* resp, float* logp, int* argmax, float* colsum_part, int n_blocks,
                            int64_t N, int K, hipStream_t stream) {
    (void)hipGetLastError();
    if (!maha || !logc || N < 1 || K < 1 || K > 64 || n_blocks < 1 || n_blocks > 65535) return SED_ERR_ARG;
    hipLaunchKernelGGL(gmm_resp_kernel, dim3(n_blocks), dim3(256), 0, stream, maha, logc, resp, logp, argmax, colsum_part, (long long)N, K);
    return sed_check_launch();
}

// colsum[k] (+)= sum over the n_blocks partial rows, in double: thread (q = tid / 64, k = tid % 64) adds rows q, q + 4, ..., the four
// quarter sums are added in order
__global__ __launch_bounds__(256) void gmm_colsum_reduce_kernel(const float* __restrict__ part, int n_blocks, int K, double* __restrict__ colsum,
                                                                int accumulate) {
    __shared__ double q4[4][64];
    const int k = threadIdx.x & 63, q = threadIdx.x >> 6;
    double s = 0.0;
    if (k < K)
        for (int i = q; i < n_blocks; i += 4) s += (double)part[(size_t)i * K + k];
    q4[q][k] = s;
    __syncthreads();
    if (threadIdx.x < K) {
        const double t = ((q4[0][k] + q4[1][k]) + q4[2][k]) + q4[3][k];
        colsum[k] = accumulate ? colsum[k] + t : t;
    }
}

extern "C" int sed_gmm_colsum_reduce(const float* colsum_part, int n_blocks, int K, double* colsum, int accumulate, hipStream_t stream) {
    (void)hipGetLastError();
    if (!colsum_part || !colsum || n_blocks < 1 || K < 1 || K > 64) return SED_ERR_ARG;
    hipLaunchKernelGGL(gmm_colsum_reduce_kernel, dim3(1), dim3(256), 0, stream, colsum_part, n_blocks, K, colsum, accumulate);
    return sed_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// sed_gmm_center_scale: A[n, d] = sqrt(w[n w_stride]) (X[n ldx + d] - mu[d]), A packed [N, D]
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_center_scale_kernel(const float* __restrict__ X, const float* __restrict__ mu, const float* __restrict__ w,
                                                               float* __restrict__ A, long long N, int D, long long ldx, long long w_stride) {
    const long long total = N * D;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long n = e / D;
        const int d = (int)(e - n * D);
        A[e] = sqrtf(w[n * w_stride]) * (X[n * ldx + d] - mu[d]);
    }
}

extern "C" int sed_gmm_center_scale(const float* X, const float* mu, const float* w, float* A, int64_t N, int D, int64_t ldx, int64_t w_stride,
                                    hipStream_t stream) {
    (void)hipGetLastError();
    if (!X || !mu || !w || !A || N < 1 || D < 1 || ldx < D || w_stride < 1) return SED_ERR_ARG;
    hipLaunchKernelGGL(gmm_center_scale_kernel, dim3(grid_for((size_t)N * D)), dim3(256), 0, stream, X, mu, w, A, (long long)N, D, (long long)ldx,
                       (long long)w_stride);
    return sed_check_launch();
}
