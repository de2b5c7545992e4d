// nca_filt.hip -- the two filters of the CCTA pipeline (include/nerfca_hip.h, "filt"): ccta.gaussian_filter and ccta.cityblock_distance with the
// dilations, erosions and borders built on it.
//
// Smoothing: a separable, symmetric filter with scipy's `reflect` boundary, three launches with f64 intermediates: axis 0 (f32 -> f64), axis 1
// (f64 -> f64), axis 2 (f64 -> f32, the one rounding).  Each workgroup stages a tile of lines plus its reflected halo in LDS as f64 and sums
// the pairs outermost first.  Along axes 0 and 1 a wave's 64 lanes lie along the contiguous axis; along axis 2 a wave owns one row.  The
// weights travel as a kernel argument: the library never calls exp.
//
// City-block distance: separable, three launches in int32: the distance to the nearest feature of a row (one wave per row, features as
// ballot masks, the idea of nca_edt.hip's row pass), then min_j (|i - j| + f(j)) along axis 1 and along axis 0 by a backward and a forward
// sweep over a line staged in LDS, sixteen threads to a line.  Every node of every stage is written once by one thread: no atomics, the same bits on every run.
//
// This translation unit keeps its own thread-local error message (nca_filt_last_error): it shares no state with the other sections.  The
// grid checks, the workspace refusal and the launch epilogue are nca_view_common.hpp's.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_filt_last_error(void) { return g_err.msg; }

constexpr int FL_BLOCK = 256, FL_WAVES = FL_BLOCK / 64;
constexpr int64_t FL_MAX_BLOCKS = (1LL << 32) / FL_BLOCK;          // a launch carries at most 2^32 threads

// ----------------------------------------------------------------------------------------------------------------------------- smoothing
constexpr int SM_R = NCA_SMOOTH_MAX_RADIUS;
constexpr int SM_TL = 32;                          // nodes along the line of a tile of the axis 0 / axis 1 launches: 8 per wave
constexpr int SM_TC = 64;                          // its columns: one per lane
constexpr int SM_TR = FL_WAVES * 64;               // nodes along the row of a tile of the axis 2 launch: 4 per lane
static_assert((size_t)(SM_TL + 2 * SM_R) * SM_TC * sizeof(double) <= 65536, "the line tile with the largest halo fits the LDS of one workgroup");
static_assert((size_t)FL_WAVES * (SM_TR + 2 * SM_R) * sizeof(double) <= 65536, "so do the four row tiles");
static_assert(SM_TL % FL_WAVES == 0, "a wave takes whole nodes of the line");

struct SmWeights {
    double w[SM_R + 1];          // w[0] the centre
};

// scipy's `reflect` (d c b a | a b c d | d c b a) of any index j onto 0 .. n - 1; the map has period 2 n, so a halo may be longer than the axis
__device__ __forceinline__ int sm_reflect(int j, int n) {
    const int p = 2 * n;
    int m = j % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

// acc = x[c] w[0], then for k = r, r - 1, .., 1: acc += (x[c - k] + x[c + k]) w[k]; every operation one rounded f64 operation.  `s` points at
// the centre, `stride` is the distance of neighbours along the line in LDS.
__device__ __forceinline__ double sm_sum(const double* s, int stride, int r, const SmWeights& W) {
    double acc = __dmul_rn(s[0], W.w[0]);
    for (int k = r; k >= 1; --k) acc = __dadd_rn(acc, __dmul_rn(__dadd_rn(s[-k * stride], s[k * stride]), W.w[k]));
    return acc;
}

// Along an axis of `len` nodes with `cols` contiguous columns behind it: element (o, j, c) at (o len + j) cols + c.  A block owns 64 columns
// and SM_TL nodes of the line of one slab o; it stages the SM_TL + 2 r nodes j0 - r .. j0 + SM_TL + r - 1, reflected, as f64 [.][64] (a
// reflected index is always inside the line, so a tile that hangs over the end stages valid nodes it never uses; a column past the end
// stages 0), then wave w takes the nodes w, w + 4, .. of the tile.  No thread returns before the barrier.
template <typename TI, typename TO>
__global__ void __launch_bounds__(FL_BLOCK) smooth_line_kernel(int32_t len, int64_t cols, int64_t col_tiles, int32_t line_tiles, int32_t r, SmWeights W,
                                                               const TI* __restrict__ in, TO* __restrict__ out) {
    extern __shared__ double s_x[];          // [SM_TL + 2 r][SM_TC]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t ct = bid % col_tiles;
    const int32_t lt = (int32_t)((bid / col_tiles) % line_tiles);
    const int64_t o = bid / (col_tiles * line_tiles);
    const int64_t c = ct * SM_TC + lane;
    const int32_t j0 = lt * SM_TL;
    const int64_t base = o * len * cols;
    const bool live = c < cols;
    const int staged = SM_TL + 2 * r;
    for (int s = wave; s < staged; s += FL_WAVES) {
        const int j = sm_reflect(j0 - r + s, len);
        s_x[s * SM_TC + lane] = live ? (double)in[base + (int64_t)j * cols + c] : 0.0;
    }
    __syncthreads();
    if (live) {
        for (int t = wave; t < SM_TL; t += FL_WAVES) {
            const int j = j0 + t;
            if (j < len) out[base + (int64_t)j * cols + c] = (TO)sm_sum(s_x + (t + r) * SM_TC + lane, SM_TC, r, W);
        }
    }
}

// Along axis 2 (the contiguous one): wave w of a block owns row 4 (blockIdx.x / row_tiles) + w and the SM_TR nodes from i0 = SM_TR
// (blockIdx.x % row_tiles) of it; it stages i0 - r .. i0 + SM_TR + r - 1, reflected, in its own part of LDS, then lane l takes the nodes
// l, l + 64, ..  A wave past the last row stages nothing but takes the barrier.  f64 in, f32 out: the one rounding of the filter.
__global__ void __launch_bounds__(FL_BLOCK) smooth_row_kernel(int64_t rows, int32_t n2, int32_t row_tiles, int32_t r, SmWeights W, const double* __restrict__ in,
                                                              float* __restrict__ out) {
    __shared__ double s_x[FL_WAVES][SM_TR + 2 * SM_R];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t row = (bid / row_tiles) * FL_WAVES + wave;
    const int32_t i0 = (int32_t)(bid % row_tiles) * SM_TR;
    const bool live = row < rows;
    const double* p = in + (live ? row : 0) * n2;
    const int staged = SM_TR + 2 * r;
    if (live)
        for (int s = lane; s < staged; s += 64) s_x[wave][s] = p[sm_reflect(i0 - r + s, n2)];
    __syncthreads();
    if (live) {
        float* q = out + row * n2;
        for (int t = lane; t < SM_TR; t += 64) {
            const int i = i0 + t;
            if (i < n2) q[i] = (float)sm_sum(&s_x[wave][t + r], 1, r, W);
        }
    }
}

// The checks the query and the entry point share: the 16 bytes per node of the workspace and the 4 + 4 of the volumes must fit int64.
static int smooth_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 24, "volumes", 0, g, nodes);
}

extern "C" size_t nca_vol_smooth_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (smooth_check("nca_vol_smooth_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    return ((size_t)nodes * 16 + 255) / 256 * 256;
}

extern "C" int nca_vol_smooth(const NcaGrid* grid, const float* vol, int32_t n_vol, const int32_t radius[3], const double* weights, float* out, void* work,
                              size_t work_bytes, void* stream) {
    const char* who = "nca_vol_smooth";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, radius);
    NCA_REFUSE_NULL(g_err, who, weights);
    NCA_REFUSE_NULL(g_err, who, out);
    if ((const void*)out == (const void*)vol) return g_err.fail(NCA_E_INVALID, "%s: out is vol: the filter does not run in place", who);
    NcaGrid g;
    int64_t nodes;
    const int rc = smooth_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    SmWeights W[3];
    const double* w = weights;
    for (int a = 0; a < 3; ++a) {
        const int32_t r = radius[a];
        if (r < 0) return g_err.fail(NCA_E_INVALID, "%s: radius[%d] = %d is negative", who, a, (int)r);
        if (r > NCA_SMOOTH_MAX_RADIUS)
            return g_err.fail(NCA_E_UNSUPPORTED, "%s: radius[%d] = %d is larger than NCA_SMOOTH_MAX_RADIUS = %d", who, a, (int)r, (int)NCA_SMOOTH_MAX_RADIUS);
        for (int k = 0; k <= SM_R; ++k) W[a].w[k] = 0.0;
        for (int k = 0; k <= r; ++k) {
            if (!isfinite(w[k])) return g_err.fail(NCA_E_INVALID, "%s: weight %d of axis %d = %g is not finite", who, k, a, w[k]);
            if (w[k] < 0.0) return g_err.fail(NCA_E_INVALID, "%s: weight %d of axis %d = %g is negative", who, k, a, w[k]);
            W[a].w[k] = w[k];
        }
        w += r + 1;
    }
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t plane = (int64_t)n1 * n2, rows = (int64_t)n_vol * n0 * n1;
    const int64_t ct0 = (plane + SM_TC - 1) / SM_TC, ct1 = (n2 + SM_TC - 1) / SM_TC;
    const int32_t lt0 = (n0 + SM_TL - 1) / SM_TL, lt1 = (n1 + SM_TL - 1) / SM_TL, rt = (n2 + SM_TR - 1) / SM_TR;
    // at most 2 nodes / 32 of them per block more than nodes / 64 blocks: far below int64
    const int64_t blocks_0 = (int64_t)n_vol * lt0 * ct0, blocks_1 = (int64_t)n_vol * n0 * lt1 * ct1, blocks_2 = (rows + FL_WAVES - 1) / FL_WAVES * rt;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, blocks_0, blocks_1, blocks_2, FL_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_smooth_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    double* a = (double*)work;          // f64 [nodes] after axis 0, then f64 [nodes] after axis 1
    double* b = a + nodes;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((smooth_line_kernel<float, double>), dim3((unsigned)blocks_0), dim3(FL_BLOCK), (size_t)(SM_TL + 2 * radius[0]) * SM_TC * sizeof(double), s, n0, plane,
                       ct0, lt0, radius[0], W[0], vol, a);
    hipLaunchKernelGGL((smooth_line_kernel<double, double>), dim3((unsigned)blocks_1), dim3(FL_BLOCK), (size_t)(SM_TL + 2 * radius[1]) * SM_TC * sizeof(double), s, n1,
                       (int64_t)n2, ct1, lt1, radius[1], W[1], (const double*)a, b);
    hipLaunchKernelGGL(smooth_row_kernel, dim3((unsigned)blocks_2), dim3(FL_BLOCK), 0, s, rows, n2, rt, radius[2], W[2], (const double*)b, out);
    return nca_launched(g_err, who);
}

// ------------------------------------------------------------------------------------------------------------------ city-block distance
constexpr int CB_CHUNKS = NCA_EDT_MAX_AXIS / 64;          // ballot masks of the longest row
constexpr int CB_TC = 16;                                 // columns of a line tile
constexpr int CB_TL = FL_BLOCK / CB_TC;                   // threads that share a line
constexpr int32_t CB_NONE = 0x7fffffff;                   // no feature
static_assert(NCA_EDT_MAX_AXIS % 64 == 0, "a row is whole chunks of 64 nodes");
static_assert((size_t)NCA_EDT_MAX_AXIS * CB_TC * sizeof(int32_t) + CB_TL * CB_TC * sizeof(int32_t) <= 65536, "the longest line tile fits the LDS of one workgroup");
static_assert(CB_TC == 16 && CB_TL == 16, "thread t owns column t & 15 and segment t >> 4 of the line");

// the nodes just outside an axis of n nodes, seen from node i
__device__ __forceinline__ int32_t cb_border(int i, int n) { return min(i + 1, n - i); }

// The row pass.  Wave w of a block owns row 4 blockIdx.x + w of the `rows` = n_vol n0 n1 rows of n2 nodes.  The features of chunk c of the
// row (nodes 64 c .. 64 c + 63) are one ballot mask, kept in LDS; the nearest feature at or before / at or after a node is the highest /
// lowest set bit of the masked word of its own chunk, else of the nearest chunk with any bit on that side.  A wave past the last row loads
// and stores nothing but takes every barrier.
__global__ void __launch_bounds__(FL_BLOCK) cb_row_kernel(int64_t rows, int32_t n2, const float* __restrict__ vol, double threshold, int32_t invert, int32_t border,
                                                          int32_t* __restrict__ gout) {
    __shared__ unsigned long long s_mask[FL_WAVES][CB_CHUNKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t row = (int64_t)blockIdx.x * FL_WAVES + wave;
    const bool live = row < rows;
    const int nch = (n2 + 63) >> 6;
    const float* p = vol + (live ? row : 0) * n2;
    for (int c = 0; c < nch; ++c) {
        const int i2 = c * 64 + lane;
        bool feat = false;
        if (live && i2 < n2) feat = ((double)p[i2] > threshold) != (invert != 0);          // a NaN is not > threshold
        const unsigned long long m = __ballot(feat);
        if (lane == 0) s_mask[wave][c] = m;
    }
    __syncthreads();
    int32_t* q = gout + (live ? row : 0) * n2;
    for (int c = 0; c < nch; ++c) {
        const int i2 = c * 64 + lane;
        const unsigned long long m = s_mask[wave][c];
        const unsigned long long le = m & (~0ull >> (63 - lane)), ge = m & (~0ull << lane);
        int32_t left = CB_NONE, right = CB_NONE;
        if (le) {
            left = lane - (63 - __clzll((long long)le));
        } else {
            for (int cc = c - 1; cc >= 0; --cc) {
                const unsigned long long mm = s_mask[wave][cc];
                if (mm) {
                    left = i2 - (cc * 64 + 63 - __clzll((long long)mm));
                    break;
                }
            }
        }
        if (ge) {
            right = (__ffsll((unsigned long long)ge) - 1) - lane;
        } else {
            for (int cc = c + 1; cc < nch; ++cc) {
                const unsigned long long mm = s_mask[wave][cc];
                if (mm) {
                    right = cc * 64 + (__ffsll((unsigned long long)mm) - 1) - i2;
                    break;
                }
            }
        }
        if (live && i2 < n2) {
            int32_t d = min(left, right);
            if (border) d = min(d, cb_border(i2, n2));
            q[i2] = d;
        }
    }
}

// One step of the separable minimum along an axis of `len` nodes: out(i, c) = min over j of (|i - j| + f(j, c)), and with `border` also of
// min(i + 1, len - i), for the lines c = 0 .. cols - 1 of slab `o`, element (o, j, c) at (o len + j) cols + c.  A block owns 16 consecutive
// lines of one slab, staged in LDS as int32 [len][16] with F = f, or CB_BIG where f is CB_NONE (and for a line past the end).  The minimum is
// the classical two sweeps, exact for |i - j| in integers: backward B(i) = min_{j >= i} (F(j) + j) - i, then forward
// out(i) = min_{j <= i} (B(j) - j) + i.  Sixteen threads share a line: thread t takes line t & 15 and the segment t >> 4 of CB_SEG = ceil(len /
// 16) consecutive nodes, and reads and writes no other node of the tile.  Before each sweep the threads exchange the minimum of their own
// segment (s_red) and every thread folds those of the segments behind it (backward) or before it (forward) into its start value; the border
// is the start value of the last / first segment, a feature at node len / node -1.  A sum that reaches CB_BIG has met no feature: since every
// real distance is below 4 NCA_EDT_MAX_AXIS, the result is CB_BIG exactly there and is written as CB_NONE.  Nothing is ever added to a start
// value that is still CB_NONE: a sweep takes the minimum with its own node first.  No thread returns early: the barriers are safe.
constexpr int32_t CB_BIG = 1 << 29;
static_assert(4 * NCA_EDT_MAX_AXIS < CB_BIG / 2, "distances and indices stay far below CB_BIG");

__global__ void __launch_bounds__(FL_BLOCK) cb_line_kernel(int32_t len, int64_t cols, int64_t col_tiles, int32_t border, const int32_t* __restrict__ in,
                                                           int32_t* __restrict__ out) {
    extern __shared__ int32_t s_f[];                 // [len][CB_TC]
    __shared__ int32_t s_red[CB_TL][CB_TC];          // the minimum of segment s of line c, for the sweep at hand
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t o = bid / col_tiles, c0 = (bid % col_tiles) * CB_TC;
    const int64_t base = o * len * cols;

    for (int idx = tid; idx < len * CB_TC; idx += FL_BLOCK) {
        const int j = idx / CB_TC;
        const int64_t c = c0 + (idx % CB_TC);
        const int32_t f = c < cols ? in[base + (int64_t)j * cols + c] : CB_NONE;
        s_f[idx] = f == CB_NONE ? CB_BIG : f;
    }
    __syncthreads();

    const int tc = tid & (CB_TC - 1), seg = tid / CB_TC;
    const int seg_len = (len + CB_TL - 1) / CB_TL;
    const int j_lo = min(seg * seg_len, len), j_hi = min(j_lo + seg_len, len);          // the thread's own nodes; none when j_lo == len
    int32_t m = CB_NONE;
    for (int j = j_lo; j < j_hi; ++j) m = min(m, s_f[j * CB_TC + tc] + j);
    s_red[seg][tc] = m;
    __syncthreads();

    int32_t run = border ? len : CB_NONE;          // the node just past the end: 0 + len
    for (int s = seg + 1; s < CB_TL; ++s) run = min(run, s_red[s][tc]);
    __syncthreads();                               // every thread has read s_red before it is written again
    m = CB_NONE;
    for (int j = j_hi - 1; j >= j_lo; --j) {
        run = min(run, s_f[j * CB_TC + tc] + j);
        const int32_t b = run - j;
        s_f[j * CB_TC + tc] = b;
        m = min(m, b - j);
    }
    s_red[seg][tc] = m;
    __syncthreads();

    run = border ? 1 : CB_NONE;                    // the node just before the start: 0 - (-1)
    for (int s = 0; s < seg; ++s) run = min(run, s_red[s][tc]);
    const int64_t c = c0 + tc;
    if (c < cols) {
        for (int j = j_lo; j < j_hi; ++j) {
            run = min(run, s_f[j * CB_TC + tc] - j);
            const int32_t d = run + j;
            out[base + (int64_t)j * cols + c] = d >= CB_BIG ? CB_NONE : d;
        }
    }
}

// The checks the query and the entry point share: the 8 bytes per node of the workspace and the 4 + 4 of the volumes must fit int64.
static int cb_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    return nca_check_stack(g_err, who, grid, n_vol, "n_vol", 16, "volumes", NCA_EDT_MAX_AXIS, g, nodes);
}

extern "C" size_t nca_vol_cityblock_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (cb_check("nca_vol_cityblock_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    return ((size_t)nodes * 8 + 255) / 256 * 256;
}

extern "C" int nca_vol_cityblock(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t invert, int32_t border, int32_t* out, void* work,
                                 size_t work_bytes, void* stream) {
    const char* who = "nca_vol_cityblock";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, out);
    if (invert != 0 && invert != 1) return g_err.fail(NCA_E_INVALID, "%s: invert = %d is neither 0 nor 1", who, (int)invert);
    if (border != 0 && border != 1) return g_err.fail(NCA_E_INVALID, "%s: border = %d is neither 0 nor 1", who, (int)border);
    if (threshold != threshold) return g_err.fail(NCA_E_INVALID, "%s: threshold = %g is not a number", who, threshold);
    NcaGrid g;
    int64_t nodes;
    const int rc = cb_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    const int32_t n0 = g.n[0], n1 = g.n[1], n2 = g.n[2];
    const int64_t rows = (int64_t)n_vol * n0 * n1, plane = (int64_t)n1 * n2;
    const int64_t blocks_r = (rows + FL_WAVES - 1) / FL_WAVES;
    const int64_t tiles_1 = (n2 + CB_TC - 1) / CB_TC, blocks_1 = (int64_t)n_vol * n0 * tiles_1;
    const int64_t tiles_0 = (plane + CB_TC - 1) / CB_TC, blocks_0 = (int64_t)n_vol * tiles_0;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, blocks_r, blocks_1, blocks_0, FL_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_cityblock_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    int32_t* gd = (int32_t*)work;          // int32 [nodes] after the row pass, then int32 [nodes] after axis 1
    int32_t* b = gd + nodes;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cb_row_kernel, dim3((unsigned)blocks_r), dim3(FL_BLOCK), 0, s, rows, n2, vol, threshold, invert, border, gd);
    hipLaunchKernelGGL(cb_line_kernel, dim3((unsigned)blocks_1), dim3(FL_BLOCK), (size_t)n1 * CB_TC * sizeof(int32_t), s, n1, (int64_t)n2, tiles_1, border,
                       (const int32_t*)gd, b);
    hipLaunchKernelGGL(cb_line_kernel, dim3((unsigned)blocks_0), dim3(FL_BLOCK), (size_t)n0 * CB_TC * sizeof(int32_t), s, n0, plane, tiles_0, border, (const int32_t*)b,
                       out);
    return nca_launched(g_err, who);
}
