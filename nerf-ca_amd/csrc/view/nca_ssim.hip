// nca_ssim.hip -- structural similarity of image stacks and the gradient of its sum in the prediction (include/nerfca_hip.h, "ssim"):
// metrics.ssim / compare_sequences and the ssim_weight of drr.fit_volumes.  The value is one pass over the two stacks (plus tile halos); the
// gradient stages its three coefficient maps P, Q, R in the caller's workspace and gathers them -- every pixel is written once by one
// thread, no atomics.  This translation unit keeps its own thread-local error message (nca_ssim_last_error): it shares no state with the
// other sections.  The workspace refusal and the launch epilogue are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_ssim_last_error(void) { return g_err.msg; }

// A workgroup of four waves owns a tile of 16 x 32: window positions in ssim_kernel, pixels in ssim_gather_kernel.  Thread t takes the
// column t & 31 and the rows (t >> 5) and (t >> 5) + 8.  The window length is a template argument, so the weights are kernel arguments
// read at constant indices and every window loop is unrolled.
constexpr int64_t SS_MAX_BLOCKS = (1LL << 32) / 256;
constexpr int SS_TH = 16, SS_TW = 32, SS_BLOCK = 256, SS_WAVES = SS_BLOCK / 64, SS_NPT = SS_TH * SS_TW / SS_BLOCK;
static_assert(SS_TW == 32 && SS_NPT == 2 && SS_BLOCK / SS_TW * SS_NPT == SS_TH, "thread t owns column t & 31 of rows t >> 5 and (t >> 5) + 8");

template <int K>
struct SsimWin {
    double v[K];
};

// COEF = false (nca_ssim): S at the tile's positions -> f64 block sum, one atomic per block; the f32 map when asked for.
// COEF = true (first kernel of nca_ssim_grad): P, Q, R at the tile's positions -> coef f64 [3][N][Hv][Wv].
// The x and y tiles with their K - 1 halo to the right and below are staged in LDS, then the row pass of the five fields for every staged
// row (f64, LDS), then each thread runs the column pass at its own positions.  No thread returns early: the barriers are safe.
template <int K, bool COEF>
__global__ void __launch_bounds__(SS_BLOCK) ssim_kernel(int32_t H, int32_t W, int32_t nbh, int32_t nbw, const float* __restrict__ x, const float* __restrict__ y,
                                                        const double* __restrict__ range, SsimWin<K> w, double k1, double k2, double* __restrict__ sum,
                                                        float* __restrict__ map, double* __restrict__ coef, int64_t plane) {
    constexpr int EH = SS_TH + K - 1, EW = SS_TW + K - 1;
    __shared__ float s_x[EH * EW], s_y[EH * EW];
    __shared__ double s_r[5][EH * SS_TW];
    __shared__ double s_red[SS_WAVES];

    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int32_t bj = (int32_t)(bid % nbw), bi = (int32_t)((bid / nbw) % nbh);
    const int64_t n = bid / ((int64_t)nbw * nbh);
    const int32_t Hv = H - K + 1, Wv = W - K + 1;
    const int32_t i0 = bi * SS_TH, j0 = bj * SS_TW;
    const float* xn = x + n * H * W;
    const float* yn = y + n * H * W;

    for (int idx = tid; idx < EH * EW; idx += SS_BLOCK) {
        const int r = idx / EW, c = idx % EW;
        const int64_t i = (int64_t)i0 + r, j = (int64_t)j0 + c;
        const bool in = i < H && j < W;
        s_x[idx] = in ? xn[i * W + j] : 0.0f;
        s_y[idx] = in ? yn[i * W + j] : 0.0f;
    }
    __syncthreads();
    for (int idx = tid; idx < EH * SS_TW; idx += SS_BLOCK) {          // the row pass: rows of the image, columns of window positions
        const int r = idx / SS_TW, c = idx % SS_TW;
        if ((int64_t)i0 + r < H && (int64_t)j0 + c < Wv) {
            double rx = 0.0, ry = 0.0, rxx = 0.0, ryy = 0.0, rxy = 0.0;
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const double xv = (double)s_x[r * EW + c + b], yv = (double)s_y[r * EW + c + b], wb = w.v[b];
                const double tx = __dmul_rn(wb, xv), ty = __dmul_rn(wb, yv);
                const double txx = __dmul_rn(wb, __dmul_rn(xv, xv)), tyy = __dmul_rn(wb, __dmul_rn(yv, yv)), txy = __dmul_rn(wb, __dmul_rn(xv, yv));
                rx = b ? __dadd_rn(rx, tx) : tx;
                ry = b ? __dadd_rn(ry, ty) : ty;
                rxx = b ? __dadd_rn(rxx, txx) : txx;
                ryy = b ? __dadd_rn(ryy, tyy) : tyy;
                rxy = b ? __dadd_rn(rxy, txy) : txy;
            }
            s_r[0][idx] = rx, s_r[1][idx] = ry, s_r[2][idx] = rxx, s_r[3][idx] = ryy, s_r[4][idx] = rxy;
        }
    }
    __syncthreads();

    const double L = range[n];
    const bool good = L > 0.0 && L <= 1.7976931348623157e308;          // finite and positive (a NaN fails both)
    const double k1L = __dmul_rn(k1, L), k2L = __dmul_rn(k2, L);
    const double C1 = __dmul_rn(k1L, k1L), C2 = __dmul_rn(k2L, k2L);
    const double bad = __longlong_as_double(0x7ff8000000000000LL);
    const int tj = tid & (SS_TW - 1);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < SS_NPT; ++k) {
        const int ti = (tid >> 5) + k * (SS_BLOCK / SS_TW);
        const int64_t i = (int64_t)i0 + ti, j = (int64_t)j0 + tj;
        if (i < Hv && j < Wv) {
            double m[5];
#pragma unroll
            for (int f = 0; f < 5; ++f) {
#pragma unroll
                for (int a = 0; a < K; ++a) {
                    const double t = __dmul_rn(w.v[a], s_r[f][(ti + a) * SS_TW + tj]);
                    m[f] = a ? __dadd_rn(m[f], t) : t;
                }
            }
            const double mx = m[0], my = m[1];
            const double mxx = __dmul_rn(mx, mx), myy = __dmul_rn(my, my), mxy = __dmul_rn(mx, my);
            const double sxx = __dsub_rn(m[2], mxx), syy = __dsub_rn(m[3], myy), sxy = __dsub_rn(m[4], mxy);
            const double a1 = __dadd_rn(__dmul_rn(2.0, mxy), C1), a2 = __dadd_rn(__dmul_rn(2.0, sxy), C2);
            const double b1 = __dadd_rn(__dadd_rn(mxx, myy), C1), b2 = __dadd_rn(__dadd_rn(sxx, syy), C2);
            const double D = __dmul_rn(b1, b2);
            const double S = good ? __ddiv_rn(__dmul_rn(a1, a2), D) : bad;
            const int64_t pos = (n * Hv + i) * Wv + j;
            if constexpr (!COEF) {
                acc = __dadd_rn(acc, S);
                if (map) map[pos] = (float)S;
            } else {
                const double p1 = __ddiv_rn(__dmul_rn(__dmul_rn(2.0, my), __dsub_rn(a2, a1)), D);
                const double p2 = __ddiv_rn(__dmul_rn(__dmul_rn(__dmul_rn(2.0, mx), S), __dsub_rn(b1, b2)), D);
                coef[pos] = good ? __dadd_rn(p1, p2) : bad;
                coef[plane + pos] = -__ddiv_rn(__dmul_rn(2.0, S), b2);
                coef[2 * plane + pos] = good ? __ddiv_rn(__dmul_rn(2.0, a1), D) : bad;
            }
        }
    }

    if constexpr (!COEF) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc = __dadd_rn(acc, __shfl_down(acc, d, 64));
        if ((tid & 63) == 0) s_red[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0) {
            double total = s_red[0];
#pragma unroll
            for (int v = 1; v < SS_WAVES; ++v) total = __dadd_rn(total, s_red[v]);
            atomicAdd(sum + n, total);
        }
    }
}

// Second kernel of nca_ssim_grad: a tile of 16 x 32 PIXELS.  The three coefficient maps at the positions (i - a, j - b) that reach the
// tile -- its K - 1 halo to the left and above -- are staged in LDS (zeros outside [0, Hv) x [0, Wv): never used, the passes skip those
// terms by their indices), then f_M for every staged row, then each thread forms F[P], F[Q], F[R] at its own pixels and writes g.
template <int K>
__global__ void __launch_bounds__(SS_BLOCK) ssim_gather_kernel(int32_t H, int32_t W, int32_t nbh, int32_t nbw, const float* __restrict__ x, const float* __restrict__ y,
                                                               const double* __restrict__ coef, int64_t plane, SsimWin<K> w, const double* __restrict__ scale,
                                                               float* __restrict__ g_x) {
    constexpr int EH = SS_TH + K - 1, EW = SS_TW + K - 1;
    __shared__ double s_m[3][EH * EW];
    __shared__ double s_f[3][EH * SS_TW];

    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int32_t bj = (int32_t)(bid % nbw), bi = (int32_t)((bid / nbw) % nbh);
    const int64_t n = bid / ((int64_t)nbw * nbh);
    const int32_t Hv = H - K + 1, Wv = W - K + 1;
    const int32_t i0 = bi * SS_TH, j0 = bj * SS_TW;
    const double* cn = coef + n * Hv * Wv;

    for (int idx = tid; idx < EH * EW; idx += SS_BLOCK) {
        const int r = idx / EW, c = idx % EW;
        const int64_t pi = (int64_t)i0 - (K - 1) + r, pj = (int64_t)j0 - (K - 1) + c;
        const bool in = pi >= 0 && pi < Hv && pj >= 0 && pj < Wv;
#pragma unroll
        for (int f = 0; f < 3; ++f) s_m[f][idx] = in ? cn[f * plane + pi * Wv + pj] : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < EH * SS_TW; idx += SS_BLOCK) {          // f_M: rows of window positions, columns of pixels
        const int r = idx / SS_TW, c = idx % SS_TW;
        const int64_t pi = (int64_t)i0 - (K - 1) + r, j = (int64_t)j0 + c;
        if (pi >= 0 && pi < Hv && j < W) {
            double fm[3] = {0.0, 0.0, 0.0};
            bool first = true;
#pragma unroll
            for (int b = 0; b < K; ++b) {
                const int64_t pj = j - b;
                if (pj >= 0 && pj < Wv) {
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        const double t = __dmul_rn(w.v[b], s_m[f][r * EW + c + (K - 1) - b]);
                        fm[f] = first ? t : __dadd_rn(fm[f], t);
                    }
                    first = false;
                }
            }
            s_f[0][idx] = fm[0], s_f[1][idx] = fm[1], s_f[2][idx] = fm[2];
        }
    }
    __syncthreads();

    const double sc = scale[n];
    const int tj = tid & (SS_TW - 1);
#pragma unroll
    for (int k = 0; k < SS_NPT; ++k) {
        const int ti = (tid >> 5) + k * (SS_BLOCK / SS_TW);
        const int64_t i = (int64_t)i0 + ti, j = (int64_t)j0 + tj;
        if (i < H && j < W) {
            double F[3] = {0.0, 0.0, 0.0};
            bool first = true;
#pragma unroll
            for (int a = 0; a < K; ++a) {
                const int64_t pi = i - a;
                if (pi >= 0 && pi < Hv) {
#pragma unroll
                    for (int f = 0; f < 3; ++f) {
                        const double t = __dmul_rn(w.v[a], s_f[f][(ti + (K - 1) - a) * SS_TW + tj]);
                        F[f] = first ? t : __dadd_rn(F[f], t);
                    }
                    first = false;
                }
            }
            const int64_t pix = (n * H + i) * W + j;
            const double xv = (double)x[pix], yv = (double)y[pix];
            const double inner = __dadd_rn(__dadd_rn(F[0], __dmul_rn(xv, F[1])), __dmul_rn(yv, F[2]));
            g_x[pix] = (float)__dmul_rn(sc, inner);
        }
    }
}

// The checks both launching entry points share (`win` is a host pointer, read here).  On success *blocks_v / *blocks_p are the tiles of the
// window positions / of the pixels, all images together; the pixels' count is the larger one and is the one held to a launch's limit.
static int ssim_check(const char* who, int32_t N, int32_t H, int32_t W, int32_t K, const double* win, double k1, double k2, int32_t nbv[2], int32_t nbp[2],
                      int64_t* blocks_v, int64_t* blocks_p) {
    if (N <= 0) return g_err.fail(NCA_E_INVALID, "%s: N = %d is not positive", who, (int)N);
    if (H <= 0) return g_err.fail(NCA_E_INVALID, "%s: H = %d is not positive", who, (int)H);
    if (W <= 0) return g_err.fail(NCA_E_INVALID, "%s: W = %d is not positive", who, (int)W);
    if (K < 1 || K > NCA_SSIM_MAX_WIN || K % 2 == 0) return g_err.fail(NCA_E_INVALID, "%s: K = %d is not an odd window length in [1, %d]", who, (int)K, (int)NCA_SSIM_MAX_WIN);
    if (H < K) return g_err.fail(NCA_E_INVALID, "%s: H = %d is smaller than the window, K = %d", who, (int)H, (int)K);
    if (W < K) return g_err.fail(NCA_E_INVALID, "%s: W = %d is smaller than the window, K = %d", who, (int)W, (int)K);
    if (win)
        for (int a = 0; a < K; ++a)
            if (!isfinite(win[a])) return g_err.fail(NCA_E_INVALID, "%s: win[%d] = %g is not finite", who, a, win[a]);
    if (!(isfinite(k1) && k1 > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: k1 = %g is not finite and positive", who, k1);
    if (!(isfinite(k2) && k2 > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: k2 = %g is not finite and positive", who, k2);
    // H W < 2^62 always; the 24 bytes per position of the coefficient maps (and the 4 per pixel) must fit int64
    if ((int64_t)H * W > INT64_MAX / 32 / N) return g_err.fail(NCA_E_INVALID, "%s: %d images of %d x %d pixels overflow int64", who, (int)N, (int)H, (int)W);
    const int32_t Hv = H - K + 1, Wv = W - K + 1;
    nbv[0] = (int32_t)(((int64_t)Hv + SS_TH - 1) / SS_TH), nbv[1] = (int32_t)(((int64_t)Wv + SS_TW - 1) / SS_TW);
    nbp[0] = (int32_t)(((int64_t)H + SS_TH - 1) / SS_TH), nbp[1] = (int32_t)(((int64_t)W + SS_TW - 1) / SS_TW);
    *blocks_v = (int64_t)N * nbv[0] * nbv[1];          // at most the pixel count: no overflow
    *blocks_p = (int64_t)N * nbp[0] * nbp[1];
    // a launch carries at most 2^32 threads (the runtime rejects gridDim.x * blockDim.x beyond that): 2^24 workgroups of 256
    if (*blocks_p > SS_MAX_BLOCKS)
        return g_err.fail(NCA_E_INVALID, "%s: %d images of %d x %d pixels make %lld tiles, more than one launch covers", who, (int)N, (int)H, (int)W, (long long)*blocks_p);
    return NCA_OK;
}

template <int K>
static SsimWin<K> pack_win(const double* win) {
    SsimWin<K> w;
    for (int a = 0; a < K; ++a) w.v[a] = win[a];
    return w;
}

#define SS_DISPATCH(K, BODY) \
    switch (K) {             \
        case 1: { constexpr int KK = 1; BODY; } break;   \
        case 3: { constexpr int KK = 3; BODY; } break;   \
        case 5: { constexpr int KK = 5; BODY; } break;   \
        case 7: { constexpr int KK = 7; BODY; } break;   \
        case 9: { constexpr int KK = 9; BODY; } break;   \
        default: { constexpr int KK = 11; BODY; } break; \
    }

extern "C" int nca_ssim(int32_t N, int32_t H, int32_t W, const float* x, const float* y, const double* range, int32_t K, const double* win, double k1, double k2,
                        double* sum, float* map, void* stream) {
    const char* who = "nca_ssim";
    NCA_REFUSE_NULL(g_err, who, x);
    NCA_REFUSE_NULL(g_err, who, y);
    NCA_REFUSE_NULL(g_err, who, range);
    NCA_REFUSE_NULL(g_err, who, win);
    NCA_REFUSE_NULL(g_err, who, sum);
    int32_t nbv[2], nbp[2];
    int64_t blocks_v, blocks_p;
    const int rc = ssim_check(who, N, H, W, K, win, k1, k2, nbv, nbp, &blocks_v, &blocks_p);
    if (rc != NCA_OK) return rc;
    SS_DISPATCH(K, hipLaunchKernelGGL((ssim_kernel<KK, false>), dim3((unsigned)blocks_v), dim3(SS_BLOCK), 0, (hipStream_t)stream, H, W, nbv[0], nbv[1], x, y, range,
                                      pack_win<KK>(win), k1, k2, sum, map, (double*)nullptr, (int64_t)0));
    return nca_launched(g_err, who);
}

extern "C" size_t nca_ssim_grad_workspace(int32_t N, int32_t H, int32_t W, int32_t K) {
    if (N <= 0 || H <= 0 || W <= 0 || K < 1 || K > NCA_SSIM_MAX_WIN || K % 2 == 0 || H < K || W < K) return 0;
    if ((int64_t)H * W > INT64_MAX / 32 / N) return 0;
    return (size_t)(3 * sizeof(double)) * (size_t)N * (size_t)(H - K + 1) * (size_t)(W - K + 1);
}

extern "C" int nca_ssim_grad(int32_t N, int32_t H, int32_t W, const float* x, const float* y, const double* range, int32_t K, const double* win, double k1, double k2,
                             const double* scale, float* g_x, void* work, size_t work_bytes, void* stream) {
    const char* who = "nca_ssim_grad";
    NCA_REFUSE_NULL(g_err, who, x);
    NCA_REFUSE_NULL(g_err, who, y);
    NCA_REFUSE_NULL(g_err, who, range);
    NCA_REFUSE_NULL(g_err, who, win);
    NCA_REFUSE_NULL(g_err, who, scale);
    NCA_REFUSE_NULL(g_err, who, g_x);
    int32_t nbv[2], nbp[2];
    int64_t blocks_v, blocks_p;
    const int rc = ssim_check(who, N, H, W, K, win, k1, k2, nbv, nbp, &blocks_v, &blocks_p);
    if (rc != NCA_OK) return rc;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_ssim_grad_workspace(N, H, W, K));
    if (rcw != NCA_OK) return rcw;
    const int64_t plane = (int64_t)N * (H - K + 1) * (W - K + 1);
    double* coef = (double*)work;
    SS_DISPATCH(K, {
        const SsimWin<KK> w = pack_win<KK>(win);
        hipLaunchKernelGGL((ssim_kernel<KK, true>), dim3((unsigned)blocks_v), dim3(SS_BLOCK), 0, (hipStream_t)stream, H, W, nbv[0], nbv[1], x, y, range, w, k1, k2,
                           (double*)nullptr, (float*)nullptr, coef, plane);
        hipLaunchKernelGGL((ssim_gather_kernel<KK>), dim3((unsigned)blocks_p), dim3(SS_BLOCK), 0, (hipStream_t)stream, H, W, nbp[0], nbp[1], x, y,
                           (const double*)coef, plane, w, scale, g_x);
    });
    return nca_launched(g_err, who);
}
