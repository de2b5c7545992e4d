// nca_resample.hip -- the cubic-spline zoom of voxel stacks (include/nerfca_hip.h, "resample"): ccta.spline_filter, ccta.zoom, ccta.resample
// and the resampling of ccta.prepare_ccta; what the reference takes from scipy.ndimage.zoom.
//
// Prefilter: the recursive filter of the cubic B-spline with the mirror boundary, axis by axis in f64, three launches: axis 0 (f32 -> f64),
// then axes 1 and 2 in place in the coefficients.  A line is serial by definition (its initial sum runs over the whole line), so ONE thread
// owns a line and the parallelism is across lines.  A workgroup stages sixteen whole lines in LDS as f64 [len][16] -- along axes 0 and 1 the
// sixteen columns are contiguous in memory, along axis 2 the sixteen rows are one contiguous span that is transposed on the way in -- so
// every global access is a coalesced one and the three sweeps of a line read LDS.  Staging whole lines is what limits an axis to
// NCA_EDT_MAX_AXIS nodes (16 x 512 x 8 bytes are the 64 KiB a workgroup may take); the alternative without a limit, walking the lines in
// memory, reads every node five times per axis instead of once.
//
// Interpolation: one launch, one thread per output node, its lanes along the contiguous axis of the output.  The thread forms the
// coordinate, the four weights and the four mirrored taps of each axis from the step, then sums the 64 products in lexicographic order in
// f64 and rounds once.  No tables.  Order 0 is one tap per axis and a copy.
//
// Every f64 operation is one rounded operation in the order the header writes it (the intrinsics below, and no contraction in this file);
// every node of every stage is written once by one thread: no atomics, the same bits on every run.  This translation unit keeps its own
// thread-local error message (nca_resample_last_error).
#include "nca_view_common.hpp"

#pragma clang fp contract(off)

static thread_local NcaViewErr g_err;

extern "C" const char* nca_resample_last_error(void) { return g_err.msg; }

constexpr int RS_BLOCK = 256;
constexpr int64_t RS_MAX_BLOCKS = (1LL << 32) / RS_BLOCK;          // a launch carries at most 2^32 threads
constexpr int SP_TC = 16;                                          // lines of a tile
static_assert((size_t)NCA_EDT_MAX_AXIS * SP_TC * sizeof(double) <= 65536, "the longest line tile fits the LDS of one workgroup");

// --------------------------------------------------------------------------------------------------------------------------- the prefilter
struct SpConst {
    double z, gain, zn;          // sqrt(3) - 2; (1 - z) (1 - 1 / z); z^(len - 1) by repeated multiplication: all formed on the host
};

// The recursion of one line whose nodes, already multiplied by the gain, lie `stride` apart in LDS.
__device__ __forceinline__ void sp_line(double* s, int stride, int n, const SpConst k) {
    const double z = k.z, zn = k.zn;
    double sum = __dadd_rn(s[0], __dmul_rn(zn, s[(n - 1) * stride]));
    double zi = z;
    for (int i = 1; i <= n - 2; ++i) {
        sum = __dadd_rn(sum, __dmul_rn(zi, __dadd_rn(s[i * stride], __dmul_rn(zn, s[(n - 1 - i) * stride]))));
        zi = __dmul_rn(zi, z);
    }
    double prev = __ddiv_rn(sum, __dsub_rn(1.0, __dmul_rn(zn, zn)));
    s[0] = prev;
    double before = prev;          // c[n - 2] once the loop is done
    for (int i = 1; i <= n - 1; ++i) {
        before = prev;
        prev = __dadd_rn(s[i * stride], __dmul_rn(z, prev));
        s[i * stride] = prev;
    }
    double next = __ddiv_rn(__dmul_rn(__dadd_rn(__dmul_rn(z, before), prev), z), __dsub_rn(__dmul_rn(z, z), 1.0));
    s[(n - 1) * stride] = next;
    for (int i = n - 2; i >= 0; --i) {
        next = __dmul_rn(z, __dsub_rn(next, s[i * stride]));
        s[i * stride] = next;
    }
}

// Along an axis of `len` nodes with `cols` contiguous columns behind it: element (o, j, c) at (o len + j) cols + c.  A block owns sixteen
// consecutive lines of one slab o, staged as f64 [len][16] times the gain; thread t < 16 then owns line t, and all threads write the tile
// back.  `in` may be `out` (axis 1): a tile is read completely before the barrier and no other block touches it.  No thread returns early.
template <typename TI>
__global__ void __launch_bounds__(RS_BLOCK) sp_line_kernel(int32_t len, int64_t cols, int64_t col_tiles, SpConst k, const TI* in, double* out) {
    extern __shared__ double s_c[];          // [len][SP_TC]
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t o = bid / col_tiles, c0 = (bid % col_tiles) * SP_TC;
    const int64_t base = o * len * cols;
    for (int idx = tid; idx < len * SP_TC; idx += RS_BLOCK) {
        const int j = idx / SP_TC;
        const int64_t c = c0 + (idx % SP_TC);
        s_c[idx] = c < cols ? __dmul_rn((double)in[base + (int64_t)j * cols + c], k.gain) : 0.0;
    }
    __syncthreads();
    if (tid < SP_TC && c0 + tid < cols) sp_line(s_c + tid, SP_TC, len, k);
    __syncthreads();
    for (int idx = tid; idx < len * SP_TC; idx += RS_BLOCK) {
        const int j = idx / SP_TC;
        const int64_t c = c0 + (idx % SP_TC);
        if (c < cols) out[base + (int64_t)j * cols + c] = s_c[idx];
    }
}

// Along axis 2, in place: a block owns the rows 16 blockIdx.x .. + 15 of the `rows` = n_vol n0 n1 rows of n2 nodes, one contiguous span
// of memory, staged transposed as f64 [n2][16] times the gain.  A row past the last one is neither staged nor filtered nor written.
__global__ void __launch_bounds__(RS_BLOCK) sp_row_kernel(int64_t rows, int32_t n2, SpConst k, double* c) {
    extern __shared__ double s_c[];          // [n2][SP_TC]
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * SP_TC;
    const int live = (int)(rows - r0 < SP_TC ? rows - r0 : SP_TC);
    double* p = c + r0 * n2;
    const int span = live * n2;          // at most 16 x 512
    for (int idx = tid; idx < span; idx += RS_BLOCK) {
        const int r = idx / n2, i = idx - r * n2;
        s_c[i * SP_TC + r] = __dmul_rn(p[idx], k.gain);
    }
    __syncthreads();
    if (tid < live) sp_line(s_c + tid, SP_TC, n2, k);
    __syncthreads();
    for (int idx = tid; idx < span; idx += RS_BLOCK) {
        const int r = idx / n2, i = idx - r * n2;
        p[idx] = s_c[i * SP_TC + r];
    }
}

// The checks the prefilter, the zoom and its query share: the 8 bytes per node of the coefficients and the 4 of the volume must fit int64.
// `staged`: the prefilter runs (order 3), which stages whole lines and makes three launches of its own.
static int rs_check(const char* who, const NcaGrid* grid, int32_t n_vol, bool staged, NcaGrid* g, int64_t* nodes) {
    const int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 12, "volumes", staged ? NCA_EDT_MAX_AXIS : 0, g, nodes);
    if (rc != NCA_OK || !staged) return rc;
    const int64_t plane = (int64_t)g->n[1] * g->n[2];
    const int64_t blocks_0 = (int64_t)n_vol * ((plane + SP_TC - 1) / SP_TC), blocks_1 = (int64_t)n_vol * g->n[0] * ((g->n[2] + SP_TC - 1) / SP_TC);
    const int64_t blocks_2 = ((int64_t)n_vol * g->n[0] * g->n[1] + SP_TC - 1) / SP_TC;
    return nca_check_launch_blocks(g_err, who, n_vol, *g, blocks_0, blocks_1, blocks_2, RS_MAX_BLOCKS);
}

static SpConst sp_const(int32_t len) {
    const double z = sqrt(3.0) - 2.0;
    const double gain = (1 - z) * (1 - 1 / z);
    double zn = z;
    for (int i = 0; i < len - 2; ++i) zn = zn * z;
    return {z, gain, zn};
}

// the three launches of a checked call
static void sp_launch(const NcaGrid& g, int32_t n_vol, const float* vol, double* coeff, hipStream_t s) {
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t plane = (int64_t)n1 * n2, rows = (int64_t)n_vol * n0 * n1;
    const int64_t tiles_0 = (plane + SP_TC - 1) / SP_TC, tiles_1 = (n2 + SP_TC - 1) / SP_TC;
    hipLaunchKernelGGL((sp_line_kernel<float>), dim3((unsigned)(n_vol * tiles_0)), dim3(RS_BLOCK), (size_t)n0 * SP_TC * sizeof(double), s, n0, plane, tiles_0, sp_const(n0),
                       vol, coeff);
    hipLaunchKernelGGL((sp_line_kernel<double>), dim3((unsigned)((int64_t)n_vol * n0 * tiles_1)), dim3(RS_BLOCK), (size_t)n1 * SP_TC * sizeof(double), s, n1, (int64_t)n2,
                       tiles_1, sp_const(n1), (const double*)coeff, coeff);
    hipLaunchKernelGGL(sp_row_kernel, dim3((unsigned)((rows + SP_TC - 1) / SP_TC)), dim3(RS_BLOCK), (size_t)n2 * SP_TC * sizeof(double), s, rows, n2, sp_const(n2), coeff);
}

extern "C" int nca_vol_spline_filter(const NcaGrid* grid, const float* vol, int32_t n_vol, double* coeff, void* stream) {
    const char* who = "nca_vol_spline_filter";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, coeff);
    if ((const void*)coeff == (const void*)vol) return g_err.fail(NCA_E_INVALID, "%s: coeff is vol: the first launch does not run in place", who);
    NcaGrid g;
    int64_t nodes;
    const int rc = rs_check(who, grid, n_vol, true, &g, &nodes);
    if (rc != NCA_OK) return rc;
    sp_launch(g, n_vol, vol, coeff, (hipStream_t)stream);
    return nca_launched(g_err, who);
}

// ------------------------------------------------------------------------------------------------------------------------ the interpolation
struct ZmAxis {
    int32_t n, m;
    double step;          // (n - 1) / (m - 1), formed on the host
};

// cc = min((double)o step, n - 1)
__device__ __forceinline__ double zm_coord(int32_t o, const ZmAxis a) { return fmin(__dmul_rn((double)o, a.step), (double)(a.n - 1)); }

// the four weights and the four taps f - 1 .. f + 2, mirrored onto the line, of output node o
__device__ __forceinline__ void zm_cubic(int32_t o, const ZmAxis a, int32_t j[4], double w[4]) {
    const double cc = zm_coord(o, a);
    const double f = floor(cc);
    const double y = __dsub_rn(cc, f), t = __dsub_rn(1.0, y);
    w[1] = __ddiv_rn(__dadd_rn(__dmul_rn(__dmul_rn(__dmul_rn(y, y), __dsub_rn(y, 2.0)), 3.0), 4.0), 6.0);
    w[2] = __ddiv_rn(__dadd_rn(__dmul_rn(__dmul_rn(__dmul_rn(t, t), __dsub_rn(t, 2.0)), 3.0), 4.0), 6.0);
    w[0] = __ddiv_rn(__dmul_rn(__dmul_rn(t, t), t), 6.0);
    w[3] = __dsub_rn(__dsub_rn(__dsub_rn(1.0, w[0]), w[1]), w[2]);
    const int32_t fi = (int32_t)f, p = 2 * (a.n - 1);          // 0 <= fi <= n - 1: the taps lie in -1 .. n + 1
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int32_t m = (fi - 1 + k) % p;
        if (m < 0) m += p;
        j[k] = m > a.n - 1 ? p - m : m;
    }
}

// Thread t of the launch owns output node t of the total = n_vol m0 m1 m2; a thread past the last node does nothing.
__global__ void __launch_bounds__(RS_BLOCK) zm_cubic_kernel(ZmAxis a0, ZmAxis a1, ZmAxis a2, int64_t total, const double* __restrict__ c, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int32_t o2 = (int32_t)(t % a2.m), o1 = (int32_t)((t / a2.m) % a1.m), o0 = (int32_t)((t / ((int64_t)a2.m * a1.m)) % a0.m);
    const int64_t v = t / ((int64_t)a2.m * a1.m * a0.m);
    int32_t j0[4], j1[4], j2[4];
    double w0[4], w1[4], w2[4];
    zm_cubic(o0, a0, j0, w0);
    zm_cubic(o1, a1, j1, w1);
    zm_cubic(o2, a2, j2, w2);
    const double* p = c + v * a0.n * a1.n * a2.n;
    double acc = 0.0;
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0) {
#pragma unroll
        for (int k1 = 0; k1 < 4; ++k1) {
            const double* row = p + ((int64_t)j0[k0] * a1.n + j1[k1]) * a2.n;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) acc = __dadd_rn(acc, __dmul_rn(__dmul_rn(__dmul_rn(row[j2[k2]], w0[k0]), w1[k1]), w2[k2]));
        }
    }
    out[t] = (float)acc;
}

__global__ void __launch_bounds__(RS_BLOCK) zm_nearest_kernel(ZmAxis a0, ZmAxis a1, ZmAxis a2, int64_t total, const float* __restrict__ vol, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x;
    if (t >= total) return;
    const int32_t o2 = (int32_t)(t % a2.m), o1 = (int32_t)((t / a2.m) % a1.m), o0 = (int32_t)((t / ((int64_t)a2.m * a1.m)) % a0.m);
    const int64_t v = t / ((int64_t)a2.m * a1.m * a0.m);
    const int32_t j0 = (int32_t)floor(__dadd_rn(zm_coord(o0, a0), 0.5)), j1 = (int32_t)floor(__dadd_rn(zm_coord(o1, a1), 0.5)),
                  j2 = (int32_t)floor(__dadd_rn(zm_coord(o2, a2), 0.5));          // cc <= n - 1, so the tap is on the line
    out[t] = vol[((v * a0.n + j0) * a1.n + j1) * a2.n + j2];
}

static int zm_check_order(const char* who, int32_t order) {
    if (order != 0 && order != 3) return g_err.fail(NCA_E_INVALID, "%s: order = %d is neither 0 nor 3", who, (int)order);
    return NCA_OK;
}

extern "C" size_t nca_vol_zoom_workspace(const NcaGrid* grid_in, int32_t n_vol, int32_t order) {
    const char* who = "nca_vol_zoom_workspace";
    NcaGrid g;
    int64_t nodes;
    if (zm_check_order(who, order) != NCA_OK) return 0;
    if (rs_check(who, grid_in, n_vol, order == 3, &g, &nodes) != NCA_OK) return 0;
    return order == 3 ? ((size_t)nodes * 8 + 255) / 256 * 256 : 0;
}

extern "C" int nca_vol_zoom(const NcaGrid* grid_in, const float* vol, int32_t n_vol, const int32_t m[3], int32_t order, float* out, void* work, size_t work_bytes,
                            void* stream) {
    const char* who = "nca_vol_zoom";
    NCA_REFUSE_NULL_GRID(g_err, who, grid_in);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, m);
    NCA_REFUSE_NULL(g_err, who, out);
    if ((const void*)out == (const void*)vol) return g_err.fail(NCA_E_INVALID, "%s: out is vol: the zoom does not run in place", who);
    const int rco = zm_check_order(who, order);
    if (rco != NCA_OK) return rco;
    NcaGrid g;
    int64_t nodes;
    const int rc = rs_check(who, grid_in, n_vol, order == 3, &g, &nodes);
    if (rc != NCA_OK) return rc;
    for (int a = 0; a < 3; ++a)
        if (m[a] < 2) return g_err.fail(NCA_E_INVALID, "%s: m[%d] = %d is less than 2 nodes", who, a, (int)m[a]);
    const int64_t m01 = (int64_t)m[0] * m[1];          // < 2^62 always
    if (m01 > (INT64_MAX / 4 / n_vol) / m[2])
        return g_err.fail(NCA_E_INVALID, "%s: %d volumes of %d x %d x %d output voxels overflow int64", who, (int)n_vol, (int)m[0], (int)m[1], (int)m[2]);
    const int64_t total = m01 * m[2] * n_vol, blocks = (total + RS_BLOCK - 1) / RS_BLOCK;
    if (blocks > RS_MAX_BLOCKS)
        return g_err.fail(NCA_E_INVALID, "%s: %d volumes of %d x %d x %d output voxels make %lld nodes, more than one launch covers", who, (int)n_vol, (int)m[0], (int)m[1],
                          (int)m[2], (long long)total);
    ZmAxis ax[3];
    for (int a = 0; a < 3; ++a) ax[a] = {g.n[a], m[a], (double)(g.n[a] - 1) / (double)(m[a] - 1)};
    hipStream_t s = (hipStream_t)stream;
    if (order == 3) {
        const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_zoom_workspace(grid_in, n_vol, order));
        if (rcw != NCA_OK) return rcw;
        double* coeff = (double*)work;          // f64 [nodes]
        sp_launch(g, n_vol, vol, coeff, s);
        hipLaunchKernelGGL(zm_cubic_kernel, dim3((unsigned)blocks), dim3(RS_BLOCK), 0, s, ax[0], ax[1], ax[2], total, (const double*)coeff, out);
    } else {
        hipLaunchKernelGGL(zm_nearest_kernel, dim3((unsigned)blocks), dim3(RS_BLOCK), 0, s, ax[0], ax[1], ax[2], total, vol, out);
    }
    return nca_launched(g_err, who);
}
