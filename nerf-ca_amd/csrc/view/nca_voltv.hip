// nca_voltv.hip -- smoothed total variation of voxel volumes in space and along the heart phase (include/nerfca_hip.h, "vol"): the two
// priors drr.fit_volumes adds to its data term, and their gradient (drr.total_variation).  Both kernels are one read of the volumes (plus
// tile halos); the gradient is gathered -- every node is written once by one thread, no atomics -- and writes one f32 per node.  This
// translation unit keeps its own thread-local error message (nca_vol_last_error): it shares no state with the other sections.  The grid
// checks, the tile count and the tile's indexing are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_vol_last_error(void) { return g_err.msg; }

// A workgroup owns a tile of 4 x 8 x 64 nodes of the grid (nca_view_common.hpp) and marches it through the volumes p = 0 .. n_vol-1.
constexpr int TV_T0 = NCA_TILE0, TV_T1 = NCA_TILE1, TV_T2 = NCA_TILE2;
constexpr int TV_BLOCK = NCA_TILE_BLOCK, TV_WAVES = NCA_TILE_WAVES, TV_NPT = NCA_TILE_NPT;

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
    const NcaTile tile = nca_tile(blockIdx.x, nb1, nb2);
    const int32_t base0 = tile.base0, base1 = tile.base1, base2 = tile.base2;
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
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    const int32_t i2 = nodes.i2;
    float xc[TV_NPT], xn[TV_NPT];
    double qp[GRAD ? TV_NPT : 1];          // t / mt of the pair that ends at the current volume, 0 where there is none
#pragma unroll
    for (int k = 0; k < TV_NPT; ++k) {
        xn[k] = nodes.live(k) ? vol[nodes.off(k)] : 0.0f;
        if constexpr (GRAD) {
            qp[k] = 0.0;
            if (wrap && nodes.live(k)) {
                const double t = __dsub_rn((double)xn[k], (double)vol[(int64_t)(n_vol - 1) * voxels + nodes.off(k)]);
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
            if (pair) xn[k] = nodes.live(k) ? nxt[nodes.off(k)] : 0.0f;
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
            if (!nodes.live(k)) continue;
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
                g_vol[(int64_t)p * voxels + nodes.off(k)] = (float)__dadd_rn(__dmul_rn(s0, gs), __dmul_rn(s1, gt));
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

// The checks both entry points share, after their own pointers; on success *voxels and the tiles per axis are set.
static int vol_check(const char* who, const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, NcaGrid* g,
                     int64_t* voxels, int32_t nb[3], int64_t* tiles) {
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_vol", n_vol);
    if (cyclic != 0 && cyclic != 1) return g_err.fail(NCA_E_INVALID, "%s: cyclic = %d is neither 0 nor 1", who, (int)cyclic);
    if (!(isfinite(eps_s) && eps_s > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: eps_s = %g is not finite and positive", who, eps_s);
    if (!(isfinite(eps_t) && eps_t > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: eps_t = %g is not finite and positive", who, eps_t);
    const int rc = nca_check_grid(g_err, who, grid, n_vol, 4, "volumes", g, voxels);
    return rc != NCA_OK ? rc : nca_count_tiles(g_err, who, *g, 0, nb, tiles);
}

extern "C" int nca_vol_tv(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, double* out, void* stream) {
    const char* who = "nca_vol_tv";
    NcaGrid g;
    int64_t voxels, tiles;
    int32_t nb[3];
    NCA_REFUSE_NULL(g_err, who, out);
    const int rc = vol_check(who, grid, vol, n_vol, eps_s, eps_t, cyclic, &g, &voxels, nb, &tiles);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((voltv_kernel<false>), dim3((unsigned)tiles), dim3(TV_BLOCK), 0, (hipStream_t)stream, g, vol, n_vol, voxels, eps_s, eps_t, cyclic, nb[1],
                       nb[2], (const double*)nullptr, (float*)nullptr, out);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_tv_grad(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, const double* scale,
                               float* g_vol, void* stream) {
    const char* who = "nca_vol_tv_grad";
    NcaGrid g;
    int64_t voxels, tiles;
    int32_t nb[3];
    NCA_REFUSE_NULL(g_err, who, scale);
    NCA_REFUSE_NULL(g_err, who, g_vol);
    const int rc = vol_check(who, grid, vol, n_vol, eps_s, eps_t, cyclic, &g, &voxels, nb, &tiles);
    if (rc != NCA_OK) return rc;
    hipLaunchKernelGGL((voltv_kernel<true>), dim3((unsigned)tiles), dim3(TV_BLOCK), 0, (hipStream_t)stream, g, vol, n_vol, voxels, eps_s, eps_t, cyclic, nb[1],
                       nb[2], scale, g_vol, (double*)nullptr);
    return nca_launched(g_err, who);
}
