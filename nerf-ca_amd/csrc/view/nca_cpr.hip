// nca_cpr.hip -- oblique planes and lumen rays through voxel stacks (include/nerfca_hip.h, "cpr"): reformat.cross_sections (the straightened
// and curved-planar reformation along a centreline) and reformat.lumen_profile (the lumen's radius in every direction of a cross-section,
// its area and diameters).
//
// Planes: one thread per output pixel, a workgroup per tile of 16 x 16 pixels of one plane, the lanes along the output's contiguous axis.
// A thread forms its world point, the grid coordinates and, by order, the node, the eight-node cell with its three fractions, or the twelve
// mirrored taps with their twelve weights ONCE, then walks the n_vol volumes with them: the gather of all heart phases costs one coordinate
// set-up, as nca_drr_project marches all phases in one pass.  The three vectors of a plane are the same for a whole workgroup (the
// compiler keeps them in scalar registers).
//
// Lumen: one workgroup per (volume, plane), a thread per ray.  A ray is serial by definition (it ends at its first crossing); the parallelism
// is across rays, planes and volumes.  The unrounded radii go to LDS; after one barrier three threads of three different waves take the
// three ordered sums of the definition (area; minimum and maximum diameter; mean), a fourth writes the status word, which the rays OR
// together in LDS.
//
// Every f64 operation is one rounded operation in the order the header writes it (the intrinsics below, and no contraction in this file);
// every output is written once by one thread, no atomics touch global memory: the same bits on every run.  Every load is of a node of the
// grid: a point that is not inside (0 <= x_a <= n_a - 1, a NaN outside) loads nothing, floor and min keep f_a in 0 .. n_a - 2, and the
// cubic taps are mirrored onto 0 .. n_a - 1.  This translation unit keeps its own thread-local error message (nca_cpr_last_error).
#include "nca_view_common.hpp"

#pragma clang fp contract(off)

static thread_local NcaViewErr g_err;

extern "C" const char* nca_cpr_last_error(void) { return g_err.msg; }

constexpr int CP_TILE = 16, CP_BLOCK = CP_TILE * CP_TILE;
constexpr int64_t CP_MAX_BLOCKS = 0x7fffffffLL;          // what one launch covers
static_assert(CP_BLOCK % 64 == 0, "whole waves");

// ---------------------------------------------------------------------------------------------------------------------- a point on the grid
struct CpPoint {
    double x0, x1, x2;          // grid coordinates
    bool inside;
};

// p_a = (o_a + s * e1_a) + t * e2_a;   x_a = (p_a - lo_a) * inv_a;   inside: 0 <= x_a <= n_a - 1 on every axis
__device__ __forceinline__ CpPoint cp_point(const NcaGrid& g, const double* __restrict__ o, const double* __restrict__ e1, const double* __restrict__ e2, double s, double t) {
    CpPoint p;
    p.x0 = __dmul_rn(__dsub_rn(__dadd_rn(__dadd_rn(o[0], __dmul_rn(s, e1[0])), __dmul_rn(t, e2[0])), g.lo[0]), g.inv[0]);
    p.x1 = __dmul_rn(__dsub_rn(__dadd_rn(__dadd_rn(o[1], __dmul_rn(s, e1[1])), __dmul_rn(t, e2[1])), g.lo[1]), g.inv[1]);
    p.x2 = __dmul_rn(__dsub_rn(__dadd_rn(__dadd_rn(o[2], __dmul_rn(s, e1[2])), __dmul_rn(t, e2[2])), g.lo[2]), g.inv[2]);
    p.inside = p.x0 >= 0.0 && p.x0 <= (double)(g.n[0] - 1) && p.x1 >= 0.0 && p.x1 <= (double)(g.n[1] - 1) && p.x2 >= 0.0 && p.x2 <= (double)(g.n[2] - 1);
    return p;
}

// ORDER 1.  The cell of an inside point: the offset of node (f_0, f_1, f_2) in a volume and the three fractions.
struct CpCell {
    int64_t off;
    double y0, y1, y2;
};

__device__ __forceinline__ double cp_cell_axis(double x, int32_t n, int32_t* f) {
    const double fl = fmin(floor(x), (double)(n - 2));          // 0 <= fl <= n - 2 for an inside x
    *f = (int32_t)fl;
    return __dsub_rn(x, fl);
}

__device__ __forceinline__ CpCell cp_cell(const NcaGrid& g, const CpPoint& p) {
    int32_t f0, f1, f2;
    CpCell c;
    c.y0 = cp_cell_axis(p.x0, g.n[0], &f0);
    c.y1 = cp_cell_axis(p.x1, g.n[1], &f1);
    c.y2 = cp_cell_axis(p.x2, g.n[2], &f2);
    c.off = ((int64_t)f0 * g.n[1] + f1) * g.n[2] + f2;
    return c;
}

// lo + y * (hi - lo)
__device__ __forceinline__ double cp_mix(double lo, double hi, double y) { return __dadd_rn(lo, __dmul_rn(y, __dsub_rn(hi, lo))); }

// the eight nodes of the cell at v: along axis 2, then axis 1, then axis 0.  s1 = n2 and s0 = n1 n2 are the strides of axes 1 and 0
__device__ __forceinline__ double cp_trilinear(const float* __restrict__ v, int64_t s0, int64_t s1, const CpCell& c) {
    const double a00 = cp_mix((double)v[0], (double)v[1], c.y2), a01 = cp_mix((double)v[s1], (double)v[s1 + 1], c.y2);
    const double a10 = cp_mix((double)v[s0], (double)v[s0 + 1], c.y2), a11 = cp_mix((double)v[s0 + s1], (double)v[s0 + s1 + 1], c.y2);
    return cp_mix(cp_mix(a00, a01, c.y1), cp_mix(a10, a11, c.y1), c.y0);
}

// ORDER 3.  The four weights and the four mirrored taps of one axis at cc = x: the expressions of "resample" (zm_cubic of nca_resample.hip,
// with the coordinate given instead of formed from a step).
__device__ __forceinline__ void cp_cubic(double cc, int32_t n, int32_t j[4], double w[4]) {
    const double f = floor(cc);
    const double y = __dsub_rn(cc, f), t = __dsub_rn(1.0, y);
    w[1] = __ddiv_rn(__dadd_rn(__dmul_rn(__dmul_rn(__dmul_rn(y, y), __dsub_rn(y, 2.0)), 3.0), 4.0), 6.0);
    w[2] = __ddiv_rn(__dadd_rn(__dmul_rn(__dmul_rn(__dmul_rn(t, t), __dsub_rn(t, 2.0)), 3.0), 4.0), 6.0);
    w[0] = __ddiv_rn(__dmul_rn(__dmul_rn(t, t), t), 6.0);
    w[3] = __dsub_rn(__dsub_rn(__dsub_rn(1.0, w[0]), w[1]), w[2]);
    const int32_t fi = (int32_t)f, p = 2 * (n - 1);          // 0 <= fi <= n - 1: the taps lie in -1 .. n + 1
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int32_t m = (fi - 1 + k) % p;
        if (m < 0) m += p;
        j[k] = m > n - 1 ? p - m : m;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------- the planes
// Block b owns tile (b % tiles) of plane (b / tiles); thread (ti, tj) = (tid / 16, tid % 16) of it owns pixel (16 tile_i + ti, 16 tile_j + tj).
// A thread past the plane's edge does nothing (no barrier follows).
template <int ORDER>
__global__ void __launch_bounds__(CP_BLOCK) cp_planes_kernel(NcaGrid g, int32_t n_vol, int32_t n_planes, const void* __restrict__ src, const double* __restrict__ origin,
                                                             const double* __restrict__ e1, const double* __restrict__ e2, int32_t nu, int32_t nv, int32_t tiles_v, int32_t tiles,
                                                             double du, double dv, float fill, float* __restrict__ out) {
    const int32_t k = (int32_t)(blockIdx.x / (uint32_t)tiles), tile = (int32_t)(blockIdx.x % (uint32_t)tiles);
    const int32_t i = (tile / tiles_v) * CP_TILE + (int32_t)threadIdx.x / CP_TILE, j = (tile % tiles_v) * CP_TILE + (int32_t)threadIdx.x % CP_TILE;
    if (i >= nu || j >= nv) return;
    const double u = __dmul_rn(__dsub_rn((double)i, __dmul_rn(0.5, (double)(nu - 1))), du);
    const double v = __dmul_rn(__dsub_rn((double)j, __dmul_rn(0.5, (double)(nv - 1))), dv);
    const CpPoint p = cp_point(g, origin + 3 * (int64_t)k, e1 + 3 * (int64_t)k, e2 + 3 * (int64_t)k, u, v);
    const int64_t s1 = g.n[2], s0 = (int64_t)g.n[1] * g.n[2], voxels = s0 * g.n[0];
    const int64_t plane = (int64_t)nu * nv, step = plane * n_planes;          // the output's strides of a plane and of a volume
    float* o = out + ((int64_t)k * plane + (int64_t)i * nv + j);
    if (!p.inside) {
        for (int32_t q = 0; q < n_vol; ++q) o[q * step] = fill;
        return;
    }
    if constexpr (ORDER == 0) {
        const int32_t j0 = (int32_t)floor(__dadd_rn(p.x0, 0.5)), j1 = (int32_t)floor(__dadd_rn(p.x1, 0.5)), j2 = (int32_t)floor(__dadd_rn(p.x2, 0.5));          // x_a <= n_a - 1: on the line
        const float* s = (const float*)src + (j0 * s0 + j1 * s1 + j2);
        for (int32_t q = 0; q < n_vol; ++q) o[q * step] = s[q * voxels];
    } else if constexpr (ORDER == 1) {
        const CpCell c = cp_cell(g, p);
        const float* s = (const float*)src + c.off;
        for (int32_t q = 0; q < n_vol; ++q) o[q * step] = (float)cp_trilinear(s + q * voxels, s0, s1, c);
    } else {
        int32_t j0[4], j1[4], j2[4];
        double w0[4], w1[4], w2[4];
        cp_cubic(p.x0, g.n[0], j0, w0);
        cp_cubic(p.x1, g.n[1], j1, w1);
        cp_cubic(p.x2, g.n[2], j2, w2);
        for (int32_t q = 0; q < n_vol; ++q) {
            const double* c = (const double*)src + q * voxels;
            double acc = 0.0;
#pragma unroll
            for (int k0 = 0; k0 < 4; ++k0) {
#pragma unroll
                for (int k1 = 0; k1 < 4; ++k1) {
                    const double* row = c + (j0[k0] * s0 + j1[k1] * s1);
#pragma unroll
                    for (int k2 = 0; k2 < 4; ++k2) acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(__dmul_rn(row[j2[k2]], w0[k0]), w1[k1]), w2[k2]));
                }
            }
            o[q * step] = (float)acc;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------------------- the lumen
// One ray from the plane's origin: the unrounded radius, and its status bits in *bits.
__device__ __forceinline__ double cp_ray(const NcaGrid& g, const float* __restrict__ vol, int64_t s0, int64_t s1, const double* __restrict__ o, const double* __restrict__ e1,
                                         const double* __restrict__ e2, double dc, double ds, double level, double dr, int32_t n_steps, int* bits) {
    double g_prev = 0.0;
    for (int32_t j = 0; j <= n_steps; ++j) {
        const double rj = __dmul_rn((double)j, dr);
        const CpPoint p = cp_point(g, o, e1, e2, __dmul_rn(rj, dc), __dmul_rn(rj, ds));
        if (!p.inside) {
            *bits = NCA_CPR_STATUS_GRID;
            return j == 0 ? 0.0 : __dmul_rn((double)(j - 1), dr);
        }
        const CpCell c = cp_cell(g, p);
        const double gj = cp_trilinear(vol + c.off, s0, s1, c);
        if (!(gj > level)) {
            if (j == 0) {
                *bits = NCA_CPR_STATUS_CENTRE;
                return 0.0;
            }
            const double t = isfinite(gj) ? __ddiv_rn(__dsub_rn(g_prev, level), __dsub_rn(g_prev, gj)) : 0.0;
            return __dmul_rn(__dadd_rn((double)(j - 1), t), dr);
        }
        g_prev = gj;
    }
    *bits = NCA_CPR_STATUS_OPEN;
    return __dmul_rn((double)n_steps, dr);
}

// Block b owns plane b % n_planes of volume b / n_planes.  Every thread reaches the barrier.
__global__ void __launch_bounds__(CP_BLOCK) cp_lumen_kernel(NcaGrid g, int32_t n_planes, const float* __restrict__ vol, const double* __restrict__ origin, const double* __restrict__ e1,
                                                            const double* __restrict__ e2, int32_t n_ang, const double* __restrict__ dirs, double sin_step, double level, double dr,
                                                            int32_t n_steps, float* __restrict__ radius, double* __restrict__ stats, int32_t* __restrict__ status) {
    __shared__ double s_r[NCA_CPR_MAX_ANGLES];
    __shared__ int s_bits;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, q = b / n_planes, k = b % n_planes;
    const int64_t s1 = g.n[2], s0 = (int64_t)g.n[1] * g.n[2], voxels = s0 * g.n[0];
    if (tid == 0) s_bits = 0;
    __syncthreads();
    int mine = 0;
    for (int32_t a = tid; a < n_ang; a += CP_BLOCK) {
        int bits = 0;
        const double r = cp_ray(g, vol + q * voxels, s0, s1, origin + 3 * k, e1 + 3 * k, e2 + 3 * k, dirs[2 * a], dirs[2 * a + 1], level, dr, n_steps, &bits);
        s_r[a] = r;
        radius[b * n_ang + a] = (float)r;
        mine |= bits;
    }
    if (mine) atomicOr(&s_bits, mine);          // LDS only; an OR has no order
    __syncthreads();
    double* st = stats + 4 * b;
    if (tid == 0) {
        double sum = 0.0;
        for (int32_t a = 0; a < n_ang; ++a) sum = __dadd_rn(sum, __dmul_rn(s_r[a], s_r[a + 1 == n_ang ? 0 : a + 1]));
        st[0] = __dmul_rn(__dmul_rn(0.5, sin_step), sum);
    } else if (tid == 64) {
        const int32_t half = n_ang / 2;
        double lo = __dadd_rn(s_r[0], s_r[half]), hi = lo;
        for (int32_t a = 1; a < half; ++a) {
            const double d = __dadd_rn(s_r[a], s_r[a + half]);
            if (d < lo) lo = d;
            if (d > hi) hi = d;
        }
        st[1] = lo;
        st[2] = hi;
    } else if (tid == 128) {
        double sum = 0.0;
        for (int32_t a = 0; a < n_ang; ++a) sum = __dadd_rn(sum, s_r[a]);
        st[3] = __ddiv_rn(sum, (double)n_ang);
    } else if (tid == 192) {
        status[b] = s_bits;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- the entry points
static int cp_check_step(const char* who, const char* name, double v) {
    if (!isfinite(v)) return g_err.fail(NCA_E_INVALID, "%s: %s = %g is not finite", who, name, v);
    if (!(v > 0.0)) return g_err.fail(NCA_E_INVALID, "%s: %s = %g is not positive", who, name, v);
    return NCA_OK;
}

extern "C" int nca_vol_sample_planes(const NcaGrid* grid, int32_t n_vol, const void* src, int32_t order, int32_t n_planes, const double* origin, const double* e1,
                                     const double* e2, int32_t nu, int32_t nv, double du, double dv, float fill, float* out, void* stream) {
    const char* who = "nca_vol_sample_planes";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, src);
    NCA_REFUSE_NULL(g_err, who, origin);
    NCA_REFUSE_NULL(g_err, who, e1);
    NCA_REFUSE_NULL(g_err, who, e2);
    NCA_REFUSE_NULL(g_err, who, out);
    NcaGrid g;
    int64_t nodes;
    int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 8, "volumes", 0, &g, &nodes);
    if (rc != NCA_OK) return rc;
    if (order != 0 && order != 1 && order != 3) return g_err.fail(NCA_E_UNSUPPORTED, "%s: order = %d is not 0, 1 or 3", who, (int)order);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_planes", n_planes);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "nu", nu);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "nv", nv);
    if ((rc = cp_check_step(who, "du", du)) != NCA_OK) return rc;
    if ((rc = cp_check_step(who, "dv", dv)) != NCA_OK) return rc;
    const int64_t tiles_u = ((int64_t)nu + CP_TILE - 1) / CP_TILE, tiles_v = ((int64_t)nv + CP_TILE - 1) / CP_TILE;
    const int64_t tiles = tiles_u * tiles_v;          // < 2^54
    if (tiles > CP_MAX_BLOCKS / n_planes)
        return g_err.fail(NCA_E_INVALID, "%s: %d planes of %d x %d pixels make %lld x %d tiles, more than one launch covers", who, (int)n_planes, (int)nu, (int)nv,
                          (long long)tiles, (int)n_planes);
    if ((int64_t)nu * nv > (INT64_MAX / 4 / n_vol) / n_planes)
        return g_err.fail(NCA_E_INVALID, "%s: %d volumes of %d planes of %d x %d pixels overflow int64", who, (int)n_vol, (int)n_planes, (int)nu, (int)nv);
    const dim3 blocks((unsigned)(tiles * n_planes)), threads(CP_BLOCK);
    hipStream_t s = (hipStream_t)stream;
    if (order == 0)
        hipLaunchKernelGGL((cp_planes_kernel<0>), blocks, threads, 0, s, g, n_vol, n_planes, src, origin, e1, e2, nu, nv, (int32_t)tiles_v, (int32_t)tiles, du, dv, fill, out);
    else if (order == 1)
        hipLaunchKernelGGL((cp_planes_kernel<1>), blocks, threads, 0, s, g, n_vol, n_planes, src, origin, e1, e2, nu, nv, (int32_t)tiles_v, (int32_t)tiles, du, dv, fill, out);
    else
        hipLaunchKernelGGL((cp_planes_kernel<3>), blocks, threads, 0, s, g, n_vol, n_planes, src, origin, e1, e2, nu, nv, (int32_t)tiles_v, (int32_t)tiles, du, dv, fill, out);
    return nca_launched(g_err, who);
}

extern "C" int nca_vol_lumen(const NcaGrid* grid, int32_t n_vol, const float* vol, int32_t n_planes, const double* origin, const double* e1, const double* e2,
                             int32_t n_ang, const double* dirs, double sin_step, double level, double dr, int32_t n_steps, float* radius, double* stats,
                             int32_t* status, void* stream) {
    const char* who = "nca_vol_lumen";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, origin);
    NCA_REFUSE_NULL(g_err, who, e1);
    NCA_REFUSE_NULL(g_err, who, e2);
    NCA_REFUSE_NULL(g_err, who, dirs);
    NCA_REFUSE_NULL(g_err, who, radius);
    NCA_REFUSE_NULL(g_err, who, stats);
    NCA_REFUSE_NULL(g_err, who, status);
    NcaGrid g;
    int64_t nodes;
    int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 8, "volumes", 0, &g, &nodes);
    if (rc != NCA_OK) return rc;
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_planes", n_planes);
    if (n_ang > NCA_CPR_MAX_ANGLES) return g_err.fail(NCA_E_UNSUPPORTED, "%s: n_ang = %d is more than NCA_CPR_MAX_ANGLES = %d", who, (int)n_ang, (int)NCA_CPR_MAX_ANGLES);
    if (n_ang < 4 || n_ang % 2 != 0) return g_err.fail(NCA_E_INVALID, "%s: n_ang = %d is not an even number of at least 4", who, (int)n_ang);
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "n_steps", n_steps);
    if (!isfinite(sin_step)) return g_err.fail(NCA_E_INVALID, "%s: sin_step = %g is not finite", who, sin_step);
    if (isnan(level)) return g_err.fail(NCA_E_INVALID, "%s: level = %g is not a number", who, level);
    if ((rc = cp_check_step(who, "dr", dr)) != NCA_OK) return rc;
    if ((int64_t)n_planes > CP_MAX_BLOCKS / n_vol)          // at most 2^31 - 1 planes of at most 1024 rays and 32 bytes: no overflow of int64 beside it
        return g_err.fail(NCA_E_INVALID, "%s: %d volumes of %d planes make %lld workgroups, more than one launch covers", who, (int)n_vol, (int)n_planes,
                          (long long)n_vol * n_planes);
    hipLaunchKernelGGL(cp_lumen_kernel, dim3((unsigned)((int64_t)n_vol * n_planes)), dim3(CP_BLOCK), 0, (hipStream_t)stream, g, n_planes, vol, origin, e1, e2, n_ang, dirs,
                       sin_step, level, dr, n_steps, radius, stats, status);
    return nca_launched(g_err, who);
}
