// nca_drr.hip -- cone-beam projection of voxel volumes (include/nerfca_hip.h, "drr"): line integrals of trilinearly interpolated f32
// grids along f64 rays, pix = i0 - sum_s value(o + d z_s) dists_s, the quadrature of the renderer.  What turns a CT / phantom volume
// into training projections (drr.volume_teacher) and an exported 4-D density grid back into images (drr.project_sequence), and its
// adjoint nca_drr_backproject, which scatters pixel gradients back onto the grid (the backward of drr.project_rays, what drr.fit_volumes
// descends by).  This translation unit keeps its own thread-local error message (nca_drr_last_error): it shares no state with nca_api.hip or
// the other sections.  The grid checks are nca_view_common.hpp's; both entry points share drr_check and the loop over groups of volumes.
// The two kernels each place a sample on the grid in their own text, and the two texts must agree bit for bit: a shared routine was tried and
// measured, and every form of it changed the adjoint's instructions ("Where the checks of csrc/view/ live").
#include <atomic>
#include <type_traits>
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_drr_last_error(void) { return g_err.msg; }

constexpr int DRR_BLOCK = 256;
constexpr int DRR_MAX_GROUP = 8;          // volumes one launch keeps accumulators for
constexpr int DRR_DEFAULT_SPLIT = 4;      // the structure tools/drr_bench.py measured as the faster one in every row

static std::atomic<int> g_drr_split{DRR_DEFAULT_SPLIT};

extern "C" int nca_drr_set_split(int32_t split) {
    if (split != 1 && split != 4) return g_err.fail(NCA_E_INVALID, "nca_drr_set_split: split = %d is neither 1 nor 4", (int)split);
    g_drr_split.store(split);
    return NCA_OK;
}

extern "C" int nca_drr_get_split(void) { return g_drr_split.load(); }

// (1 - f) v0 + f v1: two rounded products and one rounded sum
__device__ __forceinline__ double lerp_rn(double omf, double f, double v0, double v1) { return __dadd_rn(__dmul_rn(omf, v0), __dmul_rn(f, v1)); }

// One thread per (ray, part): part j of the K that share a ray marches the samples s = j, j + K, ... in order with one f64 accumulator per
// volume in registers; the K sub-sums are then folded in part order through LDS.  K = 1 is the plain loop over s.  The K parts of a ray sit in
// K different waves of the block (K = 4: wave j of the four is part j of 64 adjacent rays), so in both forms the 64 split of a wave are 64
// adjacent detector pixels (p = w*H + h) at ONE depth step and their gathers fall in a compact block of voxels; K = 4 puts four times the
// waves on the device.  The order of a volume's sum is a function of (S, K) alone: no atomics, nothing depends on the block, the chunk or
// the other volumes of the group.
//
// A sample's indices and weights are computed once and applied to all NV volumes.  A sample with every neighbour inside the grid takes the
// unguarded path (its two last-axis neighbours are adjacent dwords, which the compiler may fetch as one 8-byte load: that needs no
// alignment beyond the dword's on this target); one in the one-cell rim guards each of its eight loads; one outside loads nothing.
template <int NV, int K>
__global__ void __launch_bounds__(DRR_BLOCK) drr_kernel(NcaGrid g, const float* __restrict__ vol, int64_t voxels, int64_t R, int32_t S,
                                                        const double* __restrict__ origins, const double* __restrict__ dirs, const float* __restrict__ z,
                                                        const double* __restrict__ dists, double i0, double* __restrict__ pix) {
    constexpr int RAYS = DRR_BLOCK / K;          // rays of one block
    const int slot = threadIdx.x % RAYS, part = threadIdx.x / RAYS;          // part: which of the K sub-sums of its ray this thread forms
    const int64_t ray = (int64_t)blockIdx.x * RAYS + slot;
    const bool live = ray < R;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    if (live) {
        const double o0 = origins[3 * ray], o1 = origins[3 * ray + 1], o2 = origins[3 * ray + 2];
        const double d0 = dirs[3 * ray], d1 = dirs[3 * ray + 1], d2 = dirs[3 * ray + 2];
        const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
        const int64_t row = n2, slab = (int64_t)n1 * n2;
        for (int32_t s = part; s < S; s += K) {
            const double zz = (double)z[s];
            const double g0 = __dmul_rn(__dsub_rn(__dadd_rn(o0, __dmul_rn(d0, zz)), g.lo[0]), g.inv[0]);
            const double g1 = __dmul_rn(__dsub_rn(__dadd_rn(o1, __dmul_rn(d1, zz)), g.lo[1]), g.inv[1]);
            const double g2 = __dmul_rn(__dsub_rn(__dadd_rn(o2, __dmul_rn(d2, zz)), g.lo[2]), g.inv[2]);
            // outside (-1, n) on any axis (or NaN): every neighbour is outside or has weight 0, the term is exactly 0 -- load nothing
            if (!(g0 > -1.0 && g0 < (double)n0 && g1 > -1.0 && g1 < (double)n1 && g2 > -1.0 && g2 < (double)n2)) continue;
            const double fl0 = floor(g0), fl1 = floor(g1), fl2 = floor(g2);
            const double f0 = __dsub_rn(g0, fl0), f1 = __dsub_rn(g1, fl1), f2 = __dsub_rn(g2, fl2);
            const double m0 = __dsub_rn(1.0, f0), m1 = __dsub_rn(1.0, f1), m2 = __dsub_rn(1.0, f2);
            const int32_t i0a = (int32_t)fl0, i1a = (int32_t)fl1, i2a = (int32_t)fl2;          // each in [-1, n - 1]
            const double w = dists[s];
            const int64_t base = ((int64_t)i0a * n1 + i1a) * n2 + i2a;                          // of neighbour (0,0,0); used only where that is valid
            if (i0a >= 0 && i0a < n0 - 1 && i1a >= 0 && i1a < n1 - 1 && i2a >= 0 && i2a < n2 - 1) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const float* p = vol + (int64_t)v * voxels + base;
                    const double c00 = lerp_rn(m2, f2, (double)p[0], (double)p[1]);
                    const double c01 = lerp_rn(m2, f2, (double)p[row], (double)p[row + 1]);
                    const double c10 = lerp_rn(m2, f2, (double)p[slab], (double)p[slab + 1]);
                    const double c11 = lerp_rn(m2, f2, (double)p[slab + row], (double)p[slab + row + 1]);
                    const double val = lerp_rn(m0, f0, lerp_rn(m1, f1, c00, c01), lerp_rn(m1, f1, c10, c11));
                    acc[v] = __dadd_rn(acc[v], __dmul_rn(val, w));
                }
            } else {
                const bool a0 = i0a >= 0, b0 = i0a + 1 < n0, a1 = i1a >= 0, b1 = i1a + 1 < n1, a2 = i2a >= 0, b2 = i2a + 1 < n2;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const float* p = vol + (int64_t)v * voxels;
                    auto at = [&](bool ok, int64_t off) -> double { return ok ? (double)p[base + off] : 0.0; };
                    const double c00 = lerp_rn(m2, f2, at(a0 && a1 && a2, 0), at(a0 && a1 && b2, 1));
                    const double c01 = lerp_rn(m2, f2, at(a0 && b1 && a2, row), at(a0 && b1 && b2, row + 1));
                    const double c10 = lerp_rn(m2, f2, at(b0 && a1 && a2, slab), at(b0 && a1 && b2, slab + 1));
                    const double c11 = lerp_rn(m2, f2, at(b0 && b1 && a2, slab + row), at(b0 && b1 && b2, slab + row + 1));
                    const double val = lerp_rn(m0, f0, lerp_rn(m1, f1, c00, c01), lerp_rn(m1, f1, c10, c11));
                    acc[v] = __dadd_rn(acc[v], __dmul_rn(val, w));
                }
            }
        }
    }
    // every thread of the block gets here (nothing returned early): the barrier is safe
    if constexpr (K > 1) {
        __shared__ double s_part[K - 1][NV][RAYS];
        if (part > 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) s_part[part - 1][v][slot] = acc[v];
        }
        __syncthreads();
        if (part == 0) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
#pragma unroll
                for (int q = 1; q < K; ++q) acc[v] = __dadd_rn(acc[v], s_part[q - 1][v][slot]);          // ((a0 + a1) + a2) + a3
            }
        }
    }
    if (live && part == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) pix[(int64_t)v * R + ray] = __dsub_rn(i0, acc[v]);
    }
}

// The checks both entry points make after their pointers: the counts, the grid with `node_bytes` bytes per node of a volume, and the f64 per
// ray and volume.  On success *g and *voxels are set.
static int drr_check(const char* who, const NcaGrid* grid, int32_t n_vol, int64_t R, int32_t S, int node_bytes, NcaGrid* g, int64_t* voxels) {
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_vol", n_vol);
    if (R <= 0) return g_err.fail(NCA_E_INVALID, "%s: R = %lld is not positive", who, (long long)R);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "S", S);
    const int rc = nca_check_grid(g_err, who, grid, n_vol, node_bytes, "volumes", g, voxels);
    if (rc != NCA_OK) return rc;
    if (R > INT64_MAX / 8 / n_vol) return g_err.fail(NCA_E_INVALID, "%s: R = %lld rays x %d volumes overflows int64", who, (long long)R, (int)n_vol);
    return NCA_OK;
}

// launch(NV, v0) for groups of NV = 8, 4, 2, 1 volumes that start at volume v0: the kernels keep NV sets of accumulators in registers, and a
// volume's result is the same whatever group it is in.  NV arrives as a std::integral_constant.
template <typename Launch>
static void drr_for_groups(int32_t n_vol, Launch launch) {
    for (int32_t v0 = 0; v0 < n_vol;) {
        const int32_t left = n_vol - v0;
        if (left >= DRR_MAX_GROUP) launch(std::integral_constant<int, DRR_MAX_GROUP>{}, v0), v0 += DRR_MAX_GROUP;
        else if (left >= 4) launch(std::integral_constant<int, 4>{}, v0), v0 += 4;
        else if (left >= 2) launch(std::integral_constant<int, 2>{}, v0), v0 += 2;
        else launch(std::integral_constant<int, 1>{}, v0), v0 += 1;
    }
}

extern "C" int nca_drr_project(const NcaGrid* grid, const float* vol, int32_t n_vol, int64_t R, int32_t S, const double* origins, const double* dirs,
                               const float* z, const double* dists, double i0, double* pix, void* stream) {
    const char* who = "nca_drr_project";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, origins);
    NCA_REFUSE_NULL(g_err, who, dirs);
    NCA_REFUSE_NULL(g_err, who, z);
    NCA_REFUSE_NULL(g_err, who, dists);
    NCA_REFUSE_NULL(g_err, who, pix);
    NcaGrid g;
    int64_t voxels;
    const int rc = drr_check(who, grid, n_vol, R, S, 4, &g, &voxels);
    if (rc != NCA_OK) return rc;
    const int split = g_drr_split.load();
    const int64_t rays_per_block = DRR_BLOCK / split, blocks = (R + rays_per_block - 1) / rays_per_block;
    if (blocks > 0x7fffffffLL) return g_err.fail(NCA_E_INVALID, "%s: R = %lld is more than one launch covers", who, (long long)R);
    const dim3 grd((unsigned)blocks);
    const hipStream_t st = (hipStream_t)stream;
    drr_for_groups(n_vol, [&](auto nv, int32_t v0) {
        constexpr int NV = decltype(nv)::value;
        const float* vp = vol + (int64_t)v0 * voxels;
        double* pp = pix + (int64_t)v0 * R;
        if (split == 4)
            hipLaunchKernelGGL((drr_kernel<NV, 4>), grd, dim3(DRR_BLOCK), 0, st, g, vp, voxels, R, S, origins, dirs, z, dists, i0, pp);
        else
            hipLaunchKernelGGL((drr_kernel<NV, 1>), grd, dim3(DRR_BLOCK), 0, st, g, vp, voxels, R, S, origins, dirs, z, dists, i0, pp);
    });
    return nca_launched(g_err, who);          // once, after the last group
}

// ---- back-projection: the adjoint of nca_drr_project in the volumes ---------------------------------------------------------------------
constexpr int DRR_BACK_PARTS = 4;          // threads that share a ray: part j takes the j-th quarter of the depth steps
constexpr int DRR_DEFAULT_BACK_RUNS = 1;   // the structure tools/drr_grad_bench.py measured as the faster one

static std::atomic<int> g_drr_back_runs{DRR_DEFAULT_BACK_RUNS};

extern "C" int nca_drr_set_backproject_runs(int32_t runs) {
    if (runs != 0 && runs != 1) return g_err.fail(NCA_E_INVALID, "nca_drr_set_backproject_runs: runs = %d is neither 0 nor 1", (int)runs);
    g_drr_back_runs.store(runs);
    return NCA_OK;
}

extern "C" int nca_drr_get_backproject_runs(void) { return g_drr_back_runs.load(); }

// One thread per (ray, part) as in drr_kernel, but part j of the four marches the CONTIGUOUS steps [j ceil(S/4), (j+1) ceil(S/4)): there is no
// cross-thread sum to fold here, the partition only puts four times the waves on the device, and contiguous steps keep a ray's consecutive
// samples (which mostly share a cell) in one thread.  A wave is still 64 adjacent detector pixels at one depth step, so the nodes its 64 lanes
// add into fall in a compact block of voxels.  A sample's indices and its eight weights are computed once and applied to all NV volumes.
//
// RUNS = false: one atomic add per (sample, neighbour, volume).
// RUNS = true:  the thread keeps the 8 NV contributions of its current cell (i0a, i1a, i2a) in registers while consecutive samples stay in that
//               cell, summing them in s order, and adds them to memory when the cell changes and after its last step.
// Both add exactly the contributions of the definition; they differ in the order of a node's sum only.  Interior cells (all eight neighbours are
// nodes) add unguarded, cells in the one-cell rim guard each neighbour, samples outside add nothing.  An early return is safe: no barrier.
template <int NV, bool RUNS>
__global__ void __launch_bounds__(DRR_BLOCK) drr_back_kernel(NcaGrid g, int64_t voxels, int64_t R, int32_t S, const double* __restrict__ origins,
                                                             const double* __restrict__ dirs, const float* __restrict__ z, const double* __restrict__ dists,
                                                             const double* __restrict__ g_pix, double* __restrict__ g_vol) {
    constexpr int RAYS = DRR_BLOCK / DRR_BACK_PARTS;
    const int slot = threadIdx.x % RAYS, part = threadIdx.x / RAYS;
    const int64_t ray = (int64_t)blockIdx.x * RAYS + slot;
    if (ray >= R) return;
    const int32_t per = (S + DRR_BACK_PARTS - 1) / DRR_BACK_PARTS;          // the host refuses an S within 4 of INT32_MAX
    const int64_t s_lo = (int64_t)part * per, s_hi = s_lo + per < S ? s_lo + per : S;
    const double o0 = origins[3 * ray], o1 = origins[3 * ray + 1], o2 = origins[3 * ray + 2];
    const double d0 = dirs[3 * ray], d1 = dirs[3 * ray + 1], d2 = dirs[3 * ray + 2];
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t row = n2, slab = (int64_t)n1 * n2;
    const int64_t off[8] = {0, 1, row, row + 1, slab, slab + 1, slab + row, slab + row + 1};          // neighbour k = 4 a + 2 b + c
    double gp[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) gp[v] = g_pix[(int64_t)v * R + ray];

    // the run of the current cell (RUNS only)
    double acc[RUNS ? NV : 1][8];
    int32_t c0 = 0, c1 = 0, c2 = 0;
    bool open = false;
    auto flush = [&]() {          // the cell (c0, c1, c2), each in [-1, n - 1]: add the run's sums to the neighbours that are nodes
        const int64_t base = ((int64_t)c0 * n1 + c1) * n2 + c2;
        const bool ok0[2] = {c0 >= 0, c0 + 1 < n0}, ok1[2] = {c1 >= 0, c1 + 1 < n1}, ok2[2] = {c2 >= 0, c2 + 1 < n2};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (ok0[k >> 2] && ok1[(k >> 1) & 1] && ok2[k & 1]) {
#pragma unroll
                for (int v = 0; v < (RUNS ? NV : 1); ++v) atomicAdd(g_vol + (int64_t)v * voxels + (base + off[k]), acc[v][k]);
            }
        }
    };

    for (int64_t s = s_lo; s < s_hi; ++s) {
        const double zz = (double)z[s];
        const double g0 = __dmul_rn(__dsub_rn(__dadd_rn(o0, __dmul_rn(d0, zz)), g.lo[0]), g.inv[0]);
        const double g1 = __dmul_rn(__dsub_rn(__dadd_rn(o1, __dmul_rn(d1, zz)), g.lo[1]), g.inv[1]);
        const double g2 = __dmul_rn(__dsub_rn(__dadd_rn(o2, __dmul_rn(d2, zz)), g.lo[2]), g.inv[2]);
        // the forward's test: outside (-1, n) on any axis (or NaN) the sample read nothing, so it adds nothing
        if (!(g0 > -1.0 && g0 < (double)n0 && g1 > -1.0 && g1 < (double)n1 && g2 > -1.0 && g2 < (double)n2)) continue;
        const double fl0 = floor(g0), fl1 = floor(g1), fl2 = floor(g2);
        const double f0 = __dsub_rn(g0, fl0), f1 = __dsub_rn(g1, fl1), f2 = __dsub_rn(g2, fl2);
        const double x0[2] = {__dsub_rn(1.0, f0), f0}, x1[2] = {__dsub_rn(1.0, f1), f1}, x2[2] = {__dsub_rn(1.0, f2), f2};
        const int32_t i0a = (int32_t)fl0, i1a = (int32_t)fl1, i2a = (int32_t)fl2;          // each in [-1, n - 1]
        double w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = __dmul_rn(__dmul_rn(x0[k >> 2], x1[(k >> 1) & 1]), x2[k & 1]);          // (x0 x1) x2
        const double ds = dists[s];
        if constexpr (RUNS) {
            if (!open || i0a != c0 || i1a != c1 || i2a != c2) {
                if (open) flush();
                c0 = i0a, c1 = i1a, c2 = i2a, open = true;
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = -__dmul_rn(gp[v], ds);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[v][k] = __dmul_rn(t, w[k]);
                }
            } else {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = -__dmul_rn(gp[v], ds);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[v][k] = __dadd_rn(acc[v][k], __dmul_rn(t, w[k]));
                }
            }
        } else {
            const int64_t base = ((int64_t)i0a * n1 + i1a) * n2 + i2a;          // of neighbour (0,0,0); used only where that is valid
            if (i0a >= 0 && i0a < n0 - 1 && i1a >= 0 && i1a < n1 - 1 && i2a >= 0 && i2a < n2 - 1) {
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = -__dmul_rn(gp[v], ds);
                    double* p = g_vol + (int64_t)v * voxels + base;
#pragma unroll
                    for (int k = 0; k < 8; ++k) atomicAdd(p + off[k], __dmul_rn(t, w[k]));
                }
            } else {
                const bool ok0[2] = {i0a >= 0, i0a + 1 < n0}, ok1[2] = {i1a >= 0, i1a + 1 < n1}, ok2[2] = {i2a >= 0, i2a + 1 < n2};
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    const double t = -__dmul_rn(gp[v], ds);
                    double* p = g_vol + (int64_t)v * voxels;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (ok0[k >> 2] && ok1[(k >> 1) & 1] && ok2[k & 1]) atomicAdd(p + (base + off[k]), __dmul_rn(t, w[k]));
                }
            }
        }
    }
    if constexpr (RUNS) {
        if (open) flush();
    }
}

extern "C" int nca_drr_backproject(const NcaGrid* grid, int32_t n_vol, int64_t R, int32_t S, const double* origins, const double* dirs, const float* z,
                                   const double* dists, const double* g_pix, double* g_vol, void* stream) {
    const char* who = "nca_drr_backproject";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, origins);
    NCA_REFUSE_NULL(g_err, who, dirs);
    NCA_REFUSE_NULL(g_err, who, z);
    NCA_REFUSE_NULL(g_err, who, dists);
    NCA_REFUSE_NULL(g_err, who, g_pix);
    NCA_REFUSE_NULL(g_err, who, g_vol);
    NcaGrid g;
    int64_t voxels;
    const int rc = drr_check(who, grid, n_vol, R, S, 8, &g, &voxels);          // the gradient volumes are f64
    if (rc != NCA_OK) return rc;
    if (S > INT32_MAX - DRR_BACK_PARTS) return g_err.fail(NCA_E_INVALID, "%s: S = %d is more than one launch covers", who, (int)S);
    const bool runs = g_drr_back_runs.load() != 0;
    const int64_t rays_per_block = DRR_BLOCK / DRR_BACK_PARTS, blocks = (R + rays_per_block - 1) / rays_per_block;
    if (blocks > 0x7fffffffLL) return g_err.fail(NCA_E_INVALID, "%s: R = %lld is more than one launch covers", who, (long long)R);
    const dim3 grd((unsigned)blocks);
    const hipStream_t st = (hipStream_t)stream;
    drr_for_groups(n_vol, [&](auto nv, int32_t v0) {
        constexpr int NV = decltype(nv)::value;
        const double* gp = g_pix + (int64_t)v0 * R;
        double* gv = g_vol + (int64_t)v0 * voxels;
        if (runs)
            hipLaunchKernelGGL((drr_back_kernel<NV, true>), grd, dim3(DRR_BLOCK), 0, st, g, voxels, R, S, origins, dirs, z, dists, gp, gv);
        else
            hipLaunchKernelGGL((drr_back_kernel<NV, false>), grd, dim3(DRR_BLOCK), 0, st, g, voxels, R, S, origins, dirs, z, dists, gp, gv);
    });
    return nca_launched(g_err, who);          // once, after the last group
}
