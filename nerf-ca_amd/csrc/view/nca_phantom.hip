// nca_phantom.hip -- rasterises a procedural 4-D phantom (include/nerfca_hip.h, "phantom"): per heart phase a table of soft ellipsoids (the
// static thorax, additive) and a table of tapered capsules (the vessels, a maximum) into the f32 grids drr / export / synthetic take.  One
// pass: every node of every phase is written once by one thread, no atomics, the same bits on every run.  This translation unit keeps its
// own thread-local error message (nca_phantom_last_error): it shares no state with the other sections.  The grid checks, the tile count
// and the tile's indexing are nca_view_common.hpp's.
#include <atomic>
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;
static std::atomic<int> g_ph_cull{1};          // the faster of the two as measured by tools/phantom_bench.py

extern "C" const char* nca_phantom_last_error(void) { return g_err.msg; }

// A workgroup owns a tile of 4 x 8 x 64 nodes (nca_view_common.hpp) of one phase.
constexpr int PH_T0 = NCA_TILE0, PH_T1 = NCA_TILE1, PH_T2 = NCA_TILE2;
constexpr int PH_BLOCK = NCA_TILE_BLOCK, PH_WAVES = NCA_TILE_WAVES, PH_NPT = NCA_TILE_NPT;
constexpr int PH_BATCH = NCA_PHANTOM_SEG_BATCH;
constexpr int PH_REC = 9;          // a staged segment: a[3], e[3], ee, ra, rb - ra
static_assert(PH_BATCH == PH_BLOCK, "staging: thread t of the block tests segment t of the batch");

__device__ __forceinline__ double ph_clamp01(double v) { return fmin(fmax(v, 0.0), 1.0); }

// CULL = true: a staged segment whose padded box misses the tile's box is dropped before any node looks at it.  Such a segment has cov == 0
// exactly at every node of the tile and the maximum starts from 0, so the output bits are those of CULL = false.
// No thread returns early: the barriers are safe.  All node indexing is int64.
template <bool CULL>
__global__ void __launch_bounds__(PH_BLOCK) phantom_kernel(NcaGrid g, int64_t voxels, int64_t tiles, int32_t nb1, int32_t nb2, int32_t n_ell,
                                                           const double* __restrict__ ell, int32_t n_seg, const double* __restrict__ seg, double rho_v,
                                                           double edge, float* __restrict__ out) {
    __shared__ double s_seg[PH_BATCH * PH_REC];          // the survivors of one batch, compacted
    __shared__ int s_wcount[PH_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t bid = blockIdx.x;
    const int64_t phase = bid / tiles;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const int32_t base0 = tile.base0, base1 = tile.base1, base2 = tile.base2;
    const double h0 = __ddiv_rn(1.0, g.inv[0]), h1 = __ddiv_rn(1.0, g.inv[1]), h2 = __ddiv_rn(1.0, g.inv[2]);
    auto pos = [](double lo, int32_t i, double h) -> double { return __dadd_rn(lo, __dmul_rn((double)i, h)); };

    // the thread's own nodes: (j0, j1, j2) = (k, wave, lane)
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    const int32_t i1 = nodes.i1, i2 = nodes.i2;
    const double x1 = pos(g.lo[1], i1, h1), x2 = pos(g.lo[2], i2, h2);
    double x0[PH_NPT], best[PH_NPT];
#pragma unroll
    for (int k = 0; k < PH_NPT; ++k) x0[k] = pos(g.lo[0], base0 + k, h0), best[k] = 0.0;

    // the tile's box: positions are monotone in the index, so these are the extremes of what pos() gives inside the tile
    const int32_t last0 = min(base0 + PH_T0, n0) - 1, last1 = min(base1 + PH_T1, n1) - 1, last2 = min(base2 + PH_T2, n2) - 1;
    const double tlo0 = pos(g.lo[0], base0, h0), thi0 = pos(g.lo[0], last0, h0);
    const double tlo1 = pos(g.lo[1], base1, h1), thi1 = pos(g.lo[1], last1, h1);
    const double tlo2 = pos(g.lo[2], base2, h2), thi2 = pos(g.lo[2], last2, h2);
    const double half_edge = __dmul_rn(0.5, edge);
    constexpr double PAD = 1.0 / 1048576.0;          // 2^-20

    const double* segp = seg + phase * (int64_t)n_seg * 8;
    for (int32_t s0 = 0; s0 < n_seg; s0 += PH_BATCH) {
        const int32_t s = s0 + tid;
        bool keep = s < n_seg;
        double a0 = 0, a1 = 0, a2 = 0, b0 = 0, b1 = 0, b2 = 0, ra = 0, rb = 0;
        if (keep) {
            const double* r = segp + (int64_t)s * 8;
            a0 = r[0], a1 = r[1], a2 = r[2], b0 = r[3], b1 = r[4], b2 = r[5], ra = r[6], rb = r[7];
            if constexpr (CULL) {
                // the endpoints' box grown by the reach, padded by a relative 2^-20 of the reach and of the coordinates (which covers every
                // rounding of pos(), of the box itself and of the distance); written so that a NaN keeps the segment
                const double reach = __dadd_rn(fmax(ra, rb), half_edge);
                auto miss = [&](double a, double b, double tlo, double thi) -> bool {
                    const double grow = reach + PAD * (reach + fmax(fabs(a), fabs(b)) + fmax(fabs(tlo), fabs(thi)));
                    return fmin(a, b) - grow > thi || fmax(a, b) + grow < tlo;
                };
                keep = !(miss(a0, b0, tlo0, thi0) || miss(a1, b1, tlo1, thi1) || miss(a2, b2, tlo2, thi2));
            }
        }
        const unsigned long long mask = __ballot(keep);
        __syncthreads();          // the previous batch's readers are done with s_seg and s_wcount
        if (lane == 0) s_wcount[wave] = __popcll(mask);
        __syncthreads();
        int slot = __popcll(mask & ((1ull << lane) - 1ull)), count = 0;
#pragma unroll
        for (int w = 0; w < PH_WAVES; ++w) {
            const int c = s_wcount[w];
            slot += w < wave ? c : 0;
            count += c;
        }
        if (keep) {
            double* rec = s_seg + slot * PH_REC;
            const double e0 = __dsub_rn(b0, a0), e1 = __dsub_rn(b1, a1), e2 = __dsub_rn(b2, a2);
            rec[0] = a0, rec[1] = a1, rec[2] = a2, rec[3] = e0, rec[4] = e1, rec[5] = e2;
            rec[6] = __dadd_rn(__dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)), __dmul_rn(e2, e2));
            rec[7] = ra, rec[8] = __dsub_rn(rb, ra);
        }
        __syncthreads();
        for (int j = 0; j < count; ++j) {          // count is the same in every thread; the records are broadcast reads
            const double* rec = s_seg + j * PH_REC;
            const double e0 = rec[3], e1 = rec[4], e2 = rec[5], ee = rec[6], ra_j = rec[7], dr = rec[8];
            const double q1 = __dsub_rn(x1, rec[1]), q2 = __dsub_rn(x2, rec[2]);
            const double q1e1 = __dmul_rn(q1, e1), q2e2 = __dmul_rn(q2, e2);
#pragma unroll
            for (int k = 0; k < PH_NPT; ++k) {
                const double q0 = __dsub_rn(x0[k], rec[0]);
                const double qe = __dadd_rn(__dadd_rn(__dmul_rn(q0, e0), q1e1), q2e2);
                const double t = ee == 0.0 ? 0.0 : ph_clamp01(__ddiv_rn(qe, ee));
                const double c0 = __dsub_rn(q0, __dmul_rn(t, e0)), c1 = __dsub_rn(q1, __dmul_rn(t, e1)), c2 = __dsub_rn(q2, __dmul_rn(t, e2));
                const double d = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(c0, c0), __dmul_rn(c1, c1)), __dmul_rn(c2, c2)));
                const double r = __dadd_rn(ra_j, __dmul_rn(t, dr));
                const double cov = ph_clamp01(__dadd_rn(0.5, __ddiv_rn(__dsub_rn(r, d), edge)));
                best[k] = fmax(best[k], cov);
            }
        }
    }

    // the ellipsoids: few, every node evaluates all of them in row order (uniform addresses: constant data)
    double bg[PH_NPT];
#pragma unroll
    for (int k = 0; k < PH_NPT; ++k) bg[k] = 0.0;
    const double* ellp = ell + phase * (int64_t)n_ell * 14;
    for (int32_t m = 0; m < n_ell; ++m) {
        const double* r = ellp + (int64_t)m * 14;
        const double u1 = __dsub_rn(x1, r[1]), u2 = __dsub_rn(x2, r[2]);
        const double w = r[12], rho = r[13];
#pragma unroll
        for (int k = 0; k < PH_NPT; ++k) {
            const double u0 = __dsub_rn(x0[k], r[0]);
            const double q0 = __dadd_rn(__dadd_rn(__dmul_rn(r[3], u0), __dmul_rn(r[4], u1)), __dmul_rn(r[5], u2));
            const double q1 = __dadd_rn(__dadd_rn(__dmul_rn(r[6], u0), __dmul_rn(r[7], u1)), __dmul_rn(r[8], u2));
            const double q2 = __dadd_rn(__dadd_rn(__dmul_rn(r[9], u0), __dmul_rn(r[10], u1)), __dmul_rn(r[11], u2));
            const double rad = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(q0, q0), __dmul_rn(q1, q1)), __dmul_rn(q2, q2)));
            const double cov = ph_clamp01(__dadd_rn(0.5, __ddiv_rn(__dsub_rn(1.0, rad), w)));
            bg[k] = __dadd_rn(bg[k], __dmul_rn(rho, cov));
        }
    }

    float* outp = out + phase * voxels;
#pragma unroll
    for (int k = 0; k < PH_NPT; ++k) {
        if (nodes.live(k)) outp[nodes.off(k)] = (float)__dadd_rn(bg[k], __dmul_rn(rho_v, best[k]));
    }
}

extern "C" int nca_phantom_set_cull(int32_t on) {
    if (on != 0 && on != 1) return g_err.fail(NCA_E_INVALID, "nca_phantom_set_cull: on = %d is neither 0 nor 1", (int)on);
    g_ph_cull.store(on);
    return NCA_OK;
}

extern "C" int nca_phantom_get_cull(void) { return g_ph_cull.load(); }

extern "C" int nca_phantom_voxelize(const NcaGrid* grid, int32_t n_phase, int32_t n_ell, const double* ell, int32_t n_seg, const double* seg, double rho_v,
                                    double edge, float* out, void* stream) {
    const char* who = "nca_phantom_voxelize";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, out);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_phase", n_phase);
    if (n_ell < 0) return g_err.fail(NCA_E_INVALID, "%s: n_ell = %d is negative", who, (int)n_ell);
    if (n_seg < 0) return g_err.fail(NCA_E_INVALID, "%s: n_seg = %d is negative", who, (int)n_seg);
    if (n_ell == 0 && n_seg == 0) return g_err.fail(NCA_E_INVALID, "%s: n_ell = 0 and n_seg = 0: there is nothing to rasterise", who);
    if (n_ell > 0 && !ell) return g_err.fail(NCA_E_INVALID, "%s: ell is NULL with n_ell = %d", who, (int)n_ell);
    if (n_seg > 0 && !seg) return g_err.fail(NCA_E_INVALID, "%s: seg is NULL with n_seg = %d", who, (int)n_seg);
    if (!(isfinite(edge) && edge > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: edge = %g is not finite and positive", who, edge);
    if (!isfinite(rho_v)) return g_err.fail(NCA_E_INVALID, "%s: rho_v = %g is not finite", who, rho_v);
    NcaGrid g;
    int64_t voxels, tiles;
    int32_t nb[3];
    int rc = nca_check_grid(g_err, who, grid, n_phase, 4, "phases", &g, &voxels);
    if (rc == NCA_OK) rc = nca_count_tiles(g_err, who, g, n_phase, nb, &tiles);
    if (rc != NCA_OK) return rc;
    const dim3 blocks((unsigned)(tiles * n_phase)), threads(PH_BLOCK);
    if (g_ph_cull.load())
        hipLaunchKernelGGL((phantom_kernel<true>), blocks, threads, 0, (hipStream_t)stream, g, voxels, tiles, nb[1], nb[2], n_ell, ell, n_seg, seg, rho_v, edge, out);
    else
        hipLaunchKernelGGL((phantom_kernel<false>), blocks, threads, 0, (hipStream_t)stream, g, voxels, tiles, nb[1], nb[2], n_ell, ell, n_seg, seg, rho_v, edge, out);
    return nca_launched(g_err, who);
}
