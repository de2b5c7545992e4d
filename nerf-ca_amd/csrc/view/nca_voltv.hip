// nca_voltv.hip -- smoothed total variation of voxel volumes in space and along the heart phase (include/nerfca_hip.h, "vol"): the two
// priors drr.fit_volumes adds to its data term, and their gradient (drr.total_variation).  Both kernels are one read of the volumes (plus
// tile halos); the gradient is gathered -- every node is written once by one thread, no atomics -- and writes one f32 per node.  This
// translation unit keeps its own thread-local error message (nca_vol_last_error): it shares no state with the other sections.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdint.h>
#include "../../../include/nerfca_hip.h"

static thread_local char g_vol_err[256] = "";

static int vfail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_vol_err, sizeof(g_vol_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char* nca_vol_last_error(void) { return g_vol_err; }

// A workgroup owns a tile of 4 x 8 x 64 nodes of the grid and marches it through the volumes p = 0 .. n_vol-1.  Wave w of the eight takes the
// rows (j0, j1) = (k, w), k = 0 .. 3, with its 64 lanes along the last (contiguous) axis: 4 nodes per thread.
constexpr int TV_T0 = 4, TV_T1 = 8, TV_T2 = 64;
constexpr int TV_BLOCK = 512, TV_WAVES = TV_BLOCK / 64;
constexpr int TV_NPT = TV_T0 * TV_T1 * TV_T2 / TV_BLOCK;
static_assert(TV_T2 == 64 && TV_WAVES == TV_T1 && TV_NPT == TV_T0, "a wave is one row of the tile: node k of a thread is (k, wave, lane)");

// sqrt(e2 + t t) of one phase pair
__device__ __forceinline__ double tv_mt(double e2, double t) { return __dsqrt_rn(__dadd_rn(e2, __dmul_rn(t, t))); }

// GRAD = false (nca_vol_tv): the x tile and its one-node halo ABOVE are staged in LDS, every thread forms m at its own nodes and sums
//                m - eps_s, and sqrt(eps_t^2 + t^2) - eps_t of the pair (p, p + 1); f64 block sums, one atomic per block and term.
// GRAD = true (nca_vol_tv_grad): the x tile and its one-node halo BELOW AND ABOVE are staged; m is formed ONCE per node of the tile plus its
//                lower halo into LDS (5 x 9 x 65 f64); then each thread gathers the four quotients of its own nodes.  d_a of a lower
//                neighbour is one subtraction and one product of staged values, the same bits whichever thread forms them.
// Marching: the thread keeps x[p] and x[p + 1] at its own nodes in registers (the interior of the next tile is written to LDS from them, only
// the halo is loaded again), and the quotient t / mt of the pair (p - 1, p) in f64, so the phase term reads each volume once; with `cyclic` the
// planes 0 and n_vol - 1 are read a second time for the pair that closes the cycle.  No thread returns early: the barriers are safe.
template <bool GRAD>
__global__ void __launch_bounds__(TV_BLOCK) voltv_kernel(NcaGrid g, const float* __restrict__ vol, int32_t n_vol, int64_t voxels, double eps_s, double eps_t,
                                                         int32_t cyclic, int32_t nb1, int32_t nb2, const double* __restrict__ scale, float* __restrict__ g_vol,
                                                         double* __restrict__ out) {
    constexpr int LO = GRAD ? 1 : 0;                                                  // nodes of halo below the tile
    constexpr int E0 = TV_T0 + 1 + LO, E1 = TV_T1 + 1 + LO, E2 = TV_T2 + 1 + LO;      // the staged x region
    constexpr int M0 = TV_T0 + 1, M1 = TV_T1 + 1, M2 = TV_T2 + 1;                     // tile + lower halo (GRAD)
    __shared__ float s_x[E0 * E1 * E2];
    __shared__ double s_m[GRAD ? M0 * M1 * M2 : 1];
    __shared__ double s_red[2][TV_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);          // the wave's number, known to be uniform
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const double inv0 = g.inv[0], inv1 = g.inv[1], inv2 = g.inv[2];
    const int64_t bid = blockIdx.x;
    const int32_t base2 = (int32_t)(bid % nb2) * TV_T2, base1 = (int32_t)((bid / nb2) % nb1) * TV_T1, base0 = (int32_t)(bid / ((int64_t)nb2 * nb1)) * TV_T0;
    const double es2 = __dmul_rn(eps_s, eps_s), et2 = __dmul_rn(eps_t, eps_t);
    const bool wrap = cyclic != 0 && n_vol >= 2;

    auto X = [&](int a0, int a1, int a2) -> double { return (double)s_x[(a0 * E1 + a1) * E2 + a2]; };
    // m of the node with staged coordinates (a0, a1, a2) and grid indices (i0, i1, i2), all inside the grid
    auto m_at = [&](int a0, int a1, int a2, int64_t i0, int64_t i1, int64_t i2, double& d0, double& d1, double& d2) -> double {
        const double xi = X(a0, a1, a2);
        d0 = i0 < n0 - 1 ? __dmul_rn(__dsub_rn(X(a0 + 1, a1, a2), xi), inv0) : 0.0;
        d1 = i1 < n1 - 1 ? __dmul_rn(__dsub_rn(X(a0, a1 + 1, a2), xi), inv1) : 0.0;
        d2 = i2 < n2 - 1 ? __dmul_rn(__dsub_rn(X(a0, a1, a2 + 1), xi), inv2) : 0.0;
        return __dsqrt_rn(__dadd_rn(es2, __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2))));
    };

    // the thread's own nodes: (j0, j1, j2) = (k, wave, lane)
    const int32_t i2 = base2 + lane;
    const bool ok12 = i2 < n2 && base1 + wave < n1;
    const int64_t off_t = ((int64_t)base0 * n1 + (base1 + wave)) * n2 + i2;
    auto live_at = [&](int k) -> bool { return ok12 && base0 + k < n0; };
    auto off_at = [&](int k) -> int64_t { return off_t + (int64_t)k * n1 * n2; };          // used only where live
    float xc[TV_NPT], xn[TV_NPT];
    double qp[GRAD ? TV_NPT : 1];          // t / mt of the pair that ends at the current volume, 0 where there is none
#pragma unroll
    for (int k = 0; k < TV_NPT; ++k) {
        xn[k] = live_at(k) ? vol[off_at(k)] : 0.0f;
        if constexpr (GRAD) {
            qp[k] = 0.0;
            if (wrap && live_at(k)) {
                const double t = __dsub_rn((double)xn[k], (double)vol[(int64_t)(n_vol - 1) * voxels + off_at(k)]);
                qp[k] = __ddiv_rn(t, tv_mt(et2, t));
            }
        }
    }
    double s0 = 0.0, s1 = 0.0;
    if constexpr (GRAD) s0 = scale[0], s1 = scale[1];
    double acc_s = 0.0, acc_t = 0.0;

    for (int32_t p = 0; p < n_vol; ++p) {
        const bool pair = p + 1 < n_vol || wrap;                                   // the pair (p, p + 1 mod n_vol) exists
        const float* cur = vol + (int64_t)p * voxels;
        const float* nxt = vol + (int64_t)(p + 1 < n_vol ? p + 1 : 0) * voxels;
#pragma unroll
        for (int k = 0; k < TV_NPT; ++k) {
            xc[k] = xn[k];
            if (pair) xn[k] = live_at(k) ? nxt[off_at(k)] : 0.0f;
        }
        __syncthreads();          // the previous volume's readers are done with s_x and s_m
#pragma unroll
        for (int k = 0; k < TV_NPT; ++k) {
            s_x[((k + LO) * E1 + (wave + LO)) * E2 + (lane + LO)] = xc[k];
        }
        for (int idx = tid; idx < E0 * E1 * E2; idx += TV_BLOCK) {                 // the halo: everything staged that is not the tile
            const int a2 = idx % E2, a1 = (idx / E2) % E1, a0 = idx / (E2 * E1);
            if (a0 >= LO && a0 < LO + TV_T0 && a1 >= LO && a1 < LO + TV_T1 && a2 >= LO && a2 < LO + TV_T2) continue;
            const int64_t h0 = (int64_t)base0 - LO + a0, h1 = (int64_t)base1 - LO + a1, h2 = (int64_t)base2 - LO + a2;
            const bool in = h0 >= 0 && h0 < n0 && h1 >= 0 && h1 < n1 && h2 >= 0 && h2 < n2;
            s_x[idx] = in ? cur[(h0 * n1 + h1) * n2 + h2] : 0.0f;
        }
        __syncthreads();
        if constexpr (GRAD) {
            for (int idx = tid; idx < M0 * M1 * M2; idx += TV_BLOCK) {              // m once per node of tile + lower halo
                const int b2 = idx % M2, b1 = (idx / M2) % M1, b0 = idx / (M2 * M1);
                const int64_t h0 = (int64_t)base0 - 1 + b0, h1 = (int64_t)base1 - 1 + b1, h2 = (int64_t)base2 - 1 + b2;
                if (h0 >= 0 && h0 < n0 && h1 >= 0 && h1 < n1 && h2 >= 0 && h2 < n2) {
                    double d0, d1, d2;
                    s_m[idx] = m_at(b0, b1, b2, h0, h1, h2, d0, d1, d2);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < TV_NPT; ++k) {
            if (!live_at(k)) continue;
            const int j0 = k, j1 = wave;
            const int32_t i0 = base0 + j0, i1 = base1 + j1;
            const double t = __dsub_rn((double)xn[k], (double)xc[k]);              // used only where the pair exists
            if constexpr (!GRAD) {
                double d0, d1, d2;
                acc_s = __dadd_rn(acc_s, __dsub_rn(m_at(j0, j1, lane, i0, i1, i2, d0, d1, d2), eps_s));
                if (pair) acc_t = __dadd_rn(acc_t, __dsub_rn(tv_mt(et2, t), eps_t));
            } else {
                const int a0 = j0 + 1, a1 = j1 + 1, a2 = lane + 1;
                auto M = [&](int b0, int b1, int b2) -> double { return s_m[(b0 * M1 + b1) * M2 + b2]; };
                const double xi = X(a0, a1, a2);
                const double d0 = i0 < n0 - 1 ? __dmul_rn(__dsub_rn(X(a0 + 1, a1, a2), xi), inv0) : 0.0;
                const double d1 = i1 < n1 - 1 ? __dmul_rn(__dsub_rn(X(a0, a1 + 1, a2), xi), inv1) : 0.0;
                const double d2 = i2 < n2 - 1 ? __dmul_rn(__dsub_rn(X(a0, a1, a2 + 1), xi), inv2) : 0.0;
                const double num = __dadd_rn(__dadd_rn(__dmul_rn(d0, inv0), __dmul_rn(d1, inv1)), __dmul_rn(d2, inv2));
                const double own = -__ddiv_rn(num, M(a0, a1, a2));
                const double k0 = i0 > 0 ? __ddiv_rn(__dmul_rn(__dmul_rn(__dsub_rn(xi, X(a0 - 1, a1, a2)), inv0), inv0), M(a0 - 1, a1, a2)) : 0.0;
                const double k1 = i1 > 0 ? __ddiv_rn(__dmul_rn(__dmul_rn(__dsub_rn(xi, X(a0, a1 - 1, a2)), inv1), inv1), M(a0, a1 - 1, a2)) : 0.0;
                const double k2 = i2 > 0 ? __ddiv_rn(__dmul_rn(__dmul_rn(__dsub_rn(xi, X(a0, a1, a2 - 1)), inv2), inv2), M(a0, a1, a2 - 1)) : 0.0;
                const double gs = __dadd_rn(__dadd_rn(__dadd_rn(own, k0), k1), k2);
                const double q = pair ? __ddiv_rn(t, tv_mt(et2, t)) : 0.0;
                const double gt = __dadd_rn(-q, qp[k]);
                qp[k] = q;
                g_vol[(int64_t)p * voxels + off_at(k)] = (float)__dadd_rn(__dmul_rn(s0, gs), __dmul_rn(s1, gt));
            }
        }
    }

    if constexpr (!GRAD) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            acc_s = __dadd_rn(acc_s, __shfl_down(acc_s, d, 64));
            acc_t = __dadd_rn(acc_t, __shfl_down(acc_t, d, 64));
        }
        if (lane == 0) s_red[0][wave] = acc_s, s_red[1][wave] = acc_t;
        __syncthreads();
        if (tid < 2) {
            double sum = s_red[tid][0];
#pragma unroll
            for (int w = 1; w < TV_WAVES; ++w) sum = __dadd_rn(sum, s_red[tid][w]);
            atomicAdd(out + tid, sum);
        }
    }
}

// The checks both entry points share; on success *voxels and the blocks per axis are set.
static int vol_check(const char* who, const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, NcaGrid* g,
                     int64_t* voxels, int32_t nb[3]) {
    if (!grid) return vfail(NCA_E_INVALID, "%s: the grid descriptor is NULL", who);
    if (!vol) return vfail(NCA_E_INVALID, "%s: vol is NULL", who);
    if (n_vol <= 0) return vfail(NCA_E_INVALID, "%s: n_vol = %d is not positive", who, (int)n_vol);
    if (cyclic != 0 && cyclic != 1) return vfail(NCA_E_INVALID, "%s: cyclic = %d is neither 0 nor 1", who, (int)cyclic);
    if (!(isfinite(eps_s) && eps_s > 0.0)) return vfail(NCA_E_INVALID, "%s: eps_s = %g is not finite and positive", who, eps_s);
    if (!(isfinite(eps_t) && eps_t > 0.0)) return vfail(NCA_E_INVALID, "%s: eps_t = %g is not finite and positive", who, eps_t);
    *g = *grid;
    if (g->reserved != 0) return vfail(NCA_E_INVALID, "%s: reserved = %d is not 0", who, (int)g->reserved);
    for (int a = 0; a < 3; ++a) {
        if (g->n[a] < 2) return vfail(NCA_E_INVALID, "%s: n[%d] = %d is less than 2 nodes", who, a, (int)g->n[a]);
        if (!isfinite(g->lo[a])) return vfail(NCA_E_INVALID, "%s: lo[%d] = %g is not finite", who, a, g->lo[a]);
        if (!isfinite(g->inv[a])) return vfail(NCA_E_INVALID, "%s: inv[%d] = %g is not finite", who, a, g->inv[a]);
        if (!(g->inv[a] > 0.0)) return vfail(NCA_E_INVALID, "%s: inv[%d] = %g is not positive", who, a, g->inv[a]);
    }
    // n0 n1 < 2^62 always; the bytes of all volumes must fit int64
    const int64_t n01 = (int64_t)g->n[0] * g->n[1];
    if (n01 > (INT64_MAX / 4 / n_vol) / g->n[2])
        return vfail(NCA_E_INVALID, "%s: %d volumes of %d x %d x %d voxels overflow int64", who, (int)n_vol, (int)g->n[0], (int)g->n[1], (int)g->n[2]);
    *voxels = n01 * g->n[2];
    const int tile[3] = {TV_T0, TV_T1, TV_T2};
    for (int a = 0; a < 3; ++a) nb[a] = (int32_t)(((int64_t)g->n[a] + tile[a] - 1) / tile[a]);
    const int64_t blocks = (int64_t)nb[0] * nb[1] * nb[2];          // at most the voxel count: no overflow
    if (blocks > 0x7fffffffLL)
        return vfail(NCA_E_INVALID, "%s: %d x %d x %d voxels make %lld tiles, more than one launch covers", who, (int)g->n[0], (int)g->n[1], (int)g->n[2],
                     (long long)blocks);
    return NCA_OK;
}

extern "C" int nca_vol_tv(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, double* out, void* stream) {
    NcaGrid g;
    int64_t voxels;
    int32_t nb[3];
    if (!out) return vfail(NCA_E_INVALID, "nca_vol_tv: out is NULL");
    const int rc = vol_check("nca_vol_tv", grid, vol, n_vol, eps_s, eps_t, cyclic, &g, &voxels, nb);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((voltv_kernel<false>), dim3((unsigned)((int64_t)nb[0] * nb[1] * nb[2])), dim3(TV_BLOCK), 0, (hipStream_t)stream, g, vol, n_vol, voxels,
                       eps_s, eps_t, cyclic, nb[1], nb[2], (const double*)nullptr, (float*)nullptr, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vfail(NCA_E_HIP, "nca_vol_tv: %s", hipGetErrorString(e));
    return NCA_OK;
}

extern "C" int nca_vol_tv_grad(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, const double* scale,
                               float* g_vol, void* stream) {
    NcaGrid g;
    int64_t voxels;
    int32_t nb[3];
    if (!scale) return vfail(NCA_E_INVALID, "nca_vol_tv_grad: scale is NULL");
    if (!g_vol) return vfail(NCA_E_INVALID, "nca_vol_tv_grad: g_vol is NULL");
    const int rc = vol_check("nca_vol_tv_grad", grid, vol, n_vol, eps_s, eps_t, cyclic, &g, &voxels, nb);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((voltv_kernel<true>), dim3((unsigned)((int64_t)nb[0] * nb[1] * nb[2])), dim3(TV_BLOCK), 0, (hipStream_t)stream, g, vol, n_vol, voxels,
                       eps_s, eps_t, cyclic, nb[1], nb[2], scale, g_vol, (double*)nullptr);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return vfail(NCA_E_HIP, "nca_vol_tv_grad: %s", hipGetErrorString(e));
    return NCA_OK;
}
