// nca_label.hip -- connected components of thresholded voxel stacks (include/nerfca_hip.h, "label"): metrics.label, component_sizes,
// keep_largest and component_report.
//
// A union-find over the voxel grid whose parent array is `labels` itself.  P[x] is -1 off the mask; on the mask it is the linear index,
// within the volume, of another node of the same component with P[x] <= x.  A node with P[x] == x is a root.  Six launches:
//   1 local    a workgroup per tile of 4 x 8 x 64 nodes (nca_view_common.hpp): the mask bits of the tile go to LDS, a union-find over the
//              tile's 2048 nodes runs in LDS, and every node's parent is written as the global index of its root within the tile, which is
//              the smallest index of its component within the tile (local and global indices have the same order inside a tile).
//   2 seam     every node of the mask unites itself with the forward neighbours that lie in another tile: find both roots, link the larger
//              under the smaller with a returning atomicMin on the larger root's word.  Nothing else writes P in this launch.
//   3 flatten  root[x] = find(x) into the workspace, P only read; the roots (P[x] == x) of every 1024 consecutive nodes are counted.
//   4 scan     one workgroup per volume turns the per-block counts into exclusive offsets in raster order; counts[v] is the total.
//   5 apply    every root gets P[x] = 1 + its rank among the roots of its volume in raster order: its label.
//   6 relabel  every other node of the mask takes the label of its root, the rest 0.  Root words are only read here, the others only
//              written, each by its own thread.
//
// TERMINATION: no workgroup ever waits for another one.  There is no flag, no spin, no look-back and no cooperative launch in this file;
// every loop is one of the two below, and both are bounded by the node count whatever any other thread does and whatever the loads return.
//   find(x):  x <- P[x] while P[x] < x (as unsigned: a negative or larger word ends the loop too).  Every step takes a strictly smaller
//             index, so at most x steps.  This holds for ANY values in P -- stale, torn or wrong ones included.
//   unite(a, b):  a, b <- find(a), find(b); while a != b: with a the larger, old = atomicMin(&P[a], b); if old == a the link is made and
//             the loop ends; otherwise old < a (a larger or negative old ends the loop) and the loop goes on from (find(old), find(b)).
//             max(a, b) is strictly smaller in every round: the new a is at most old < a and b < a already.  At most max(a, b) rounds.
// The loops of the LDS union-find of launch 1 are the same two on indices below 2048.
//
// STALE LOADS: the L2 is per XCD, so a load of P in launch 2 may return an earlier value of the word, whatever its scope.  P[x] only ever
// decreases, only through atomicMin, and every value it ever held is a node of x's component; so a chain of stale parents still ends at a
// node of the component that WAS a root.  Whether it still IS one is never taken from a load: the atomicMin executes at the memory side and
// returns the word's true value, and only `old == a` counts as "a was a root and is now linked".  When old != a the word already pointed to
// old: the atomicMin may have replaced that link by a -> b (when b < old), and the thread that did so goes on to unite old with b, which
// restores it.  The loads of launch 2 are relaxed agent-scope atomic loads: they bypass the L1, which is never refreshed at all.
//
// The result is a function of the mask alone: the components are those of the mask, a component's root is its smallest index (links go
// from larger to smaller only, so the smallest index of a component can never get a parent), and the numbering is by root index.  The
// same bits on every run, whatever order the atomics arrive in.
//
// This translation unit keeps its own thread-local error message (nca_label_last_error): it shares no state with the other sections.
#include "nca_view_common.hpp"

static thread_local NcaViewErr g_err;

extern "C" const char* nca_label_last_error(void) { return g_err.msg; }

constexpr int64_t LB_MAX_NODES = 0x7ffffffeLL;          // a label is a node index plus one in int32
constexpr int64_t LB_MAX_BLOCKS = 0x7fffffffLL;
constexpr int LB_BLOCK = 256, LB_NPT = 4, LB_CHUNK = LB_BLOCK * LB_NPT;          // launches 3, 5 and 6: 1024 consecutive nodes per workgroup
constexpr int LB_TILE_NODES = NCA_TILE0 * NCA_TILE1 * NCA_TILE2;
static_assert(LB_TILE_NODES == 2048 && NCA_TILE1 == 8 && NCA_TILE2 == 64, "a tile-local index is (k << 9) | (wave << 6) | lane");

// ------------------------------------------------------------------------------------------------------------------------ the two loops
__device__ __forceinline__ int32_t lb_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// x <- P[x] while P[x] < x as unsigned: strictly decreasing, at most x steps for any contents of P
__device__ __forceinline__ int32_t lb_find(const int32_t* P, int32_t x) {
    for (;;) {
        const int32_t p = lb_load(P + x);
        if ((uint32_t)p >= (uint32_t)x) return x;
        x = p;
    }
}

// the same on words no other thread writes during the launch: plain loads
__device__ __forceinline__ int32_t lb_find_quiet(const int32_t* __restrict__ P, int32_t x) {
    for (;;) {
        const int32_t p = P[x];
        if ((uint32_t)p >= (uint32_t)x) return x;
        x = p;
    }
}

// max(a, b) is strictly smaller in every round; `old == a` alone says that a was a root
__device__ __forceinline__ void lb_unite(int32_t* P, int32_t a, int32_t b) {
    a = lb_find(P, a);
    b = lb_find(P, b);
    while (a != b) {
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(P + a, b);
        if ((uint32_t)old >= (uint32_t)a) return;          // old == a: linked (a larger or negative word cannot be: it ends the loop as well)
        a = lb_find(P, old);
        b = lb_find(P, b);
    }
}

__device__ __forceinline__ int32_t lb_find_lds(const int32_t* s, int32_t x) {
    for (;;) {
        const int32_t p = __hip_atomic_load(s + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((uint32_t)p >= (uint32_t)x) return x;
        x = p;
    }
}

__device__ __forceinline__ void lb_unite_lds(int32_t* s, int32_t a, int32_t b) {
    a = lb_find_lds(s, a);
    b = lb_find_lds(s, b);
    while (a != b) {
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = atomicMin(s + a, b);
        if ((uint32_t)old >= (uint32_t)a) return;
        a = lb_find_lds(s, old);
        b = lb_find_lds(s, b);
    }
}

// the four row offsets (d0, d1) of a half neighbourhood besides the row itself; backward: negated
__constant__ const int8_t LB_ROW_D0[4] = {0, 1, 1, 1};
__constant__ const int8_t LB_ROW_D1[4] = {1, -1, 0, 1};

// ------------------------------------------------------------------------------------------------------------------------ 1: local pass
// Block b owns tile b % tiles of volume b / tiles.  A wave is a row of 64 nodes along the contiguous axis, so a row's mask is one ballot;
// a node starts with the first node of its run in the row as parent, which makes the links along axis 2.  Then every node of the mask looks
// at the four BACKWARD rows inside the tile.  The node straight across (d2 = 0) is united with unless the pair one lane below is on the
// mask in both rows too: then both pairs lie in the same two runs and that pair makes (or passes on) the link.  The nodes diagonally across
// (d2 = -1, +1) are looked at only where the node straight across is off the mask: otherwise they are in its run.
__global__ void __launch_bounds__(NCA_TILE_BLOCK) label_local_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t tiles, int32_t nb1, int32_t nb2,
                                                                     const float* __restrict__ vol, double threshold, int32_t invert, int32_t conn,
                                                                     int32_t* __restrict__ labels) {
    __shared__ int32_t s_par[LB_TILE_NODES];
    __shared__ unsigned long long s_bits[NCA_TILE0][NCA_TILE1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t vol_off = (bid / tiles) * voxels;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    const bool inv = invert != 0;

#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        bool m = false;
        if (nodes.live(k)) m = ((double)vol[vol_off + nodes.off(k)] > threshold) != inv;
        const unsigned long long bits = __ballot(m);
        if (lane == 0) s_bits[k][wave] = bits;
        const unsigned long long below = ~bits & ((1ull << lane) - 1ull);          // the nodes off the mask below this lane
        const int start = below ? 64 - __clzll((long long)below) : 0;            // one past the highest of them
        s_par[(k << 9) | (wave << 6) | lane] = m ? ((k << 9) | (wave << 6) | start) : -1;
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        const unsigned long long cur = s_bits[k][wave];
        if (!((cur >> lane) & 1ull)) continue;
        const int32_t x = (k << 9) | (wave << 6) | lane;
        for (int r = 0; r < 4; ++r) {
            const int d0 = -LB_ROW_D0[r], d1 = -LB_ROW_D1[r];
            const int nzr = (d0 != 0) + (d1 != 0);
            const int kk = k + d0, ww = wave + d1;
            if (nzr > conn || kk < 0 || ww < 0 || ww >= NCA_TILE1) continue;
            const unsigned long long up = s_bits[kk][ww];
            const int32_t rb = (kk << 9) | (ww << 6);
            if ((up >> lane) & 1ull) {
                if (!(lane > 0 && (((cur & up) >> (lane - 1)) & 1ull))) lb_unite_lds(s_par, x, rb | lane);
            } else if (nzr + 1 <= conn) {
                if (lane > 0 && ((up >> (lane - 1)) & 1ull)) lb_unite_lds(s_par, x, rb | (lane - 1));
                if (lane < 63 && ((up >> (lane + 1)) & 1ull)) lb_unite_lds(s_par, x, rb | (lane + 1));
            }
        }
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < NCA_TILE_NPT; ++k) {
        if (!nodes.live(k)) continue;
        const int32_t x = (k << 9) | (wave << 6) | lane;
        int32_t out = -1;
        if ((s_bits[k][wave] >> lane) & 1ull) {
            const int32_t r = lb_find_lds(s_par, x);
            out = (int32_t)(((int64_t)(tile.base0 + (r >> 9)) * n1 + (tile.base1 + ((r >> 6) & 7))) * n2 + (tile.base2 + (r & 63)));          // below 2^31 - 2
        }
        labels[vol_off + nodes.off(k)] = out;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- 2: seam pass
// The same tiling.  Every node of the mask looks at the FORWARD half of its neighbourhood, (0,0,+1) and the rows (0,+1), (+1,-1), (+1,0),
// (+1,+1), and unites itself with those neighbours that lie in another tile; the pairs inside a tile are launch 1's.  The two economies of
// launch 1 hold here too: straight across, a pair is skipped when the pair one lane below is on the mask in both rows (it lies in the same
// two tiles and the same two runs); diagonally across, only where the node straight across is off the mask (else the diagonal node is in
// that node's run, joined to it by launch 1 or, across a tile face of axis 2, by the (0,0,+1) pair of this launch).
__global__ void __launch_bounds__(NCA_TILE_BLOCK) label_seam_kernel(int32_t n0, int32_t n1, int32_t n2, int64_t voxels, int64_t tiles, int32_t nb1, int32_t nb2,
                                                                    int32_t conn, int32_t* labels) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    int32_t* P = labels + (bid / tiles) * voxels;
    const NcaTile tile = nca_tile(bid % tiles, nb1, nb2);
    const NcaTileNodes nodes = nca_tile_nodes(tile, wave, lane, n0, n1, n2);
    const int32_t i1 = nodes.i1, i2 = nodes.i2;

    for (int k = 0; k < NCA_TILE_NPT; ++k) {          // every branch around a ballot below is uniform over the wave
        const int32_t i0 = tile.base0 + k;
        const bool live = nodes.live(k);
        const int32_t x = live ? (int32_t)nodes.off(k) : 0;
        const bool mx = live && lb_load(P + x) >= 0;          // the sign of a word never changes after launch 1
        if (mx && lane == 63 && i2 + 1 < n2 && lb_load(P + x + 1) >= 0) lb_unite(P, x, x + 1);
        for (int r = 0; r < 4; ++r) {
            const int d0 = LB_ROW_D0[r], d1 = LB_ROW_D1[r];
            const int nzr = (d0 != 0) + (d1 != 0);
            const int32_t j0 = i0 + d0, j1 = i1 + d1;
            if (nzr > conn || j0 >= n0 || j1 < 0 || j1 >= n1) continue;
            const bool row_cross = k + d0 >= NCA_TILE0 || wave + d1 < 0 || wave + d1 >= NCA_TILE1;
            const bool diag = nzr + 1 <= conn;
            if (!row_cross && !diag) continue;
            const int32_t y0 = (int32_t)(((int64_t)j0 * n1 + j1) * n2 + i2);          // the node straight across; inside the grid where i2 < n2
            bool c = false;
            if (mx && (row_cross || lane == 0 || lane == 63)) c = lb_load(P + y0) >= 0;
            if (row_cross) {
                const unsigned long long both = __ballot(mx && c);
                if (mx && c && !(lane > 0 && ((both >> (lane - 1)) & 1ull))) lb_unite(P, x, y0);
            }
            if (diag && mx && !c) {
                if (i2 > 0 && (row_cross || lane == 0) && lb_load(P + y0 - 1) >= 0) lb_unite(P, x, y0 - 1);
                if (i2 + 1 < n2 && (row_cross || lane == 63) && lb_load(P + y0 + 1) >= 0) lb_unite(P, x, y0 + 1);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- 3 .. 6: flatten, scan, apply, relabel
// the sum of `v` over the 256 threads of a workgroup (s: 4 words), returned to all of them
__device__ __forceinline__ int32_t lb_block_sum(int32_t* s, int tid, int32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((tid & 63) == 0) s[tid >> 6] = v;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

// Block b owns the nodes 1024 c .. 1024 c + 1023 of volume v, (v, c) = (b / chunks, b % chunks); thread t the nodes t, t + 256, ...
// root[i] = find(i) on the mask (nothing is written elsewhere: launch 6 does not read it there); part[b] = the roots among the block's nodes.
__global__ void __launch_bounds__(LB_BLOCK) label_flatten_kernel(int64_t voxels, int64_t chunks, const int32_t* __restrict__ labels, int32_t* __restrict__ root,
                                                                 int32_t* __restrict__ part) {
    __shared__ int32_t s[4];
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t base = (bid / chunks) * voxels, c0 = (bid % chunks) * LB_CHUNK;
    const int32_t* __restrict__ P = labels + base;
    int32_t n = 0;
#pragma unroll
    for (int j = 0; j < LB_NPT; ++j) {
        const int64_t i = c0 + j * LB_BLOCK + tid;
        if (i >= voxels) continue;
        const int32_t p = P[i];
        if (p < 0) continue;
        const int32_t r = lb_find_quiet(P, p);
        root[base + i] = r;
        n += r == (int32_t)i;
    }
    n = lb_block_sum(s, tid, n);
    if (tid == 0) part[bid] = n;
}

// Block v turns the `chunks` counts of volume v into exclusive offsets, in place, 256 at a time with a running carry; counts[v] = the total.
__global__ void __launch_bounds__(LB_BLOCK) label_scan_kernel(int64_t chunks, int32_t* __restrict__ part, int32_t* __restrict__ counts) {
    __shared__ int32_t s[LB_BLOCK];
    const int tid = threadIdx.x;
    int32_t* __restrict__ p = part + (int64_t)blockIdx.x * chunks;
    int32_t carry = 0;
    for (int64_t c0 = 0; c0 < chunks; c0 += LB_BLOCK) {
        const int64_t c = c0 + tid;
        const int32_t v = c < chunks ? p[c] : 0;
        s[tid] = v;
        __syncthreads();
        for (int h = 1; h < LB_BLOCK; h <<= 1) {          // inclusive scan
            const int32_t add = tid >= h ? s[tid - h] : 0;
            __syncthreads();
            s[tid] += add;
            __syncthreads();
        }
        if (c < chunks) p[c] = carry + s[tid] - v;
        carry += s[LB_BLOCK - 1];
        __syncthreads();
    }
    if (tid == 0) counts[blockIdx.x] = carry;
}

// The blocks of launch 3.  A root (labels[i] == i) gets labels[i] = 1 + part[b] + the roots before it in the block, in raster order: node
// j * 256 + t of the block comes after every node of the rows below j and after the lanes below t of its own row.
__global__ void __launch_bounds__(LB_BLOCK) label_apply_kernel(int64_t voxels, int64_t chunks, int32_t* __restrict__ labels, const int32_t* __restrict__ part) {
    __shared__ int32_t s_w[LB_NPT][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t bid = blockIdx.x;
    const int64_t base = (bid / chunks) * voxels, c0 = (bid % chunks) * LB_CHUNK;
    bool is_root[LB_NPT];
    int32_t before[LB_NPT];
#pragma unroll
    for (int j = 0; j < LB_NPT; ++j) {
        const int64_t i = c0 + j * LB_BLOCK + tid;
        is_root[j] = i < voxels && labels[base + i] == (int32_t)i;
        const unsigned long long b = __ballot(is_root[j]);
        before[j] = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[j][wave] = __popcll(b);
    }
    __syncthreads();
    int32_t run = part[bid];
#pragma unroll
    for (int j = 0; j < LB_NPT; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w == wave && is_root[j]) labels[base + c0 + j * LB_BLOCK + tid] = 1 + run + before[j];
            run += s_w[j][w];
        }
}

// labels[i] = 0 off the mask, the label of root[i] on it; a root's own word is final already and is only read.
__global__ void __launch_bounds__(LB_BLOCK) label_relabel_kernel(int64_t voxels, int64_t chunks, int32_t* labels, const int32_t* __restrict__ root) {
    const int tid = threadIdx.x;
    const int64_t bid = blockIdx.x;
    const int64_t base = (bid / chunks) * voxels, c0 = (bid % chunks) * LB_CHUNK;
#pragma unroll
    for (int j = 0; j < LB_NPT; ++j) {
        const int64_t i = c0 + j * LB_BLOCK + tid;
        if (i >= voxels) continue;
        if (labels[base + i] < 0) {
            labels[base + i] = 0;
            continue;
        }
        const int32_t r = root[base + i];
        if (r != (int32_t)i) labels[base + i] = labels[base + r];
    }
}

// The checks the query and the entry point share: 4 + 4 bytes per node of vol and labels and 4 of the workspace must fit int64, and a
// volume's node indices plus one must fit int32.
static int label_check(const char* who, const NcaGrid* grid, int32_t n_vol, NcaGrid* g, int64_t* nodes) {
    const int rc = nca_check_stack(g_err, who, grid, n_vol, "n_vol", 16, "volumes", 0, g, nodes);
    if (rc != NCA_OK) return rc;
    if (*nodes / n_vol > LB_MAX_NODES)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: a volume of %d x %d x %d = %lld nodes has more than 2^31 - 2: a label is a node index plus one in int32", who,
                          (int)g->n[0], (int)g->n[1], (int)g->n[2], (long long)(*nodes / n_vol));
    return NCA_OK;
}

static size_t label_root_bytes(int64_t nodes) { return ((size_t)nodes * 4 + 255) / 256 * 256; }

extern "C" size_t nca_vol_label_workspace(const NcaGrid* grid, int32_t n_vol) {
    NcaGrid g;
    int64_t nodes;
    if (label_check("nca_vol_label_workspace", grid, n_vol, &g, &nodes) != NCA_OK) return 0;
    const int64_t chunks = (nodes / n_vol + LB_CHUNK - 1) / LB_CHUNK;
    return label_root_bytes(nodes) + ((size_t)chunks * n_vol * 4 + 255) / 256 * 256;
}

extern "C" int nca_vol_label(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t connectivity, int32_t invert, int32_t* labels,
                             int32_t* counts, void* work, size_t work_bytes, void* stream) {
    const char* who = "nca_vol_label";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, vol);
    NCA_REFUSE_NULL(g_err, who, labels);
    NCA_REFUSE_NULL(g_err, who, counts);
    if ((const void*)labels == (const void*)vol) return g_err.fail(NCA_E_INVALID, "%s: labels is vol: the components are not labelled in place", who);
    if (invert != 0 && invert != 1) return g_err.fail(NCA_E_INVALID, "%s: invert = %d is neither 0 nor 1", who, (int)invert);
    if (threshold != threshold) return g_err.fail(NCA_E_INVALID, "%s: threshold = %g is not a number", who, threshold);
    if (connectivity < 1 || connectivity > 3)
        return g_err.fail(NCA_E_UNSUPPORTED, "%s: connectivity = %d is not 1, 2 or 3 (6, 18 or 26 neighbours)", who, (int)connectivity);
    NcaGrid g;
    int64_t nodes;
    const int rc = label_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    int32_t nb[3];
    int64_t tiles;
    const int rct = nca_count_tiles(g_err, who, g, 0, nb, &tiles);
    if (rct != NCA_OK) return rct;
    const int64_t voxels = nodes / n_vol, chunks = (voxels + LB_CHUNK - 1) / LB_CHUNK;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, tiles * n_vol, chunks * n_vol, 0, LB_MAX_BLOCKS);          // each factor below 2^31
    if (rcb != NCA_OK) return rcb;
    const int rcw = nca_check_workspace(g_err, who, work, work_bytes, nca_vol_label_workspace(grid, n_vol));
    if (rcw != NCA_OK) return rcw;
    int32_t* root = (int32_t*)work;
    int32_t* part = (int32_t*)((char*)work + label_root_bytes(nodes));
    hipStream_t s = (hipStream_t)stream;
    const dim3 tile_grid((unsigned)(tiles * n_vol)), tile_block(NCA_TILE_BLOCK), lin_grid((unsigned)(chunks * n_vol)), lin_block(LB_BLOCK);
    hipLaunchKernelGGL(label_local_kernel, tile_grid, tile_block, 0, s, g.n[0], g.n[1], g.n[2], voxels, tiles, nb[1], nb[2], vol, threshold, invert, connectivity, labels);
    hipLaunchKernelGGL(label_seam_kernel, tile_grid, tile_block, 0, s, g.n[0], g.n[1], g.n[2], voxels, tiles, nb[1], nb[2], connectivity, labels);
    hipLaunchKernelGGL(label_flatten_kernel, lin_grid, lin_block, 0, s, voxels, chunks, (const int32_t*)labels, root, part);
    hipLaunchKernelGGL(label_scan_kernel, dim3((unsigned)n_vol), lin_block, 0, s, chunks, part, counts);
    hipLaunchKernelGGL(label_apply_kernel, lin_grid, lin_block, 0, s, voxels, chunks, labels, (const int32_t*)part);
    hipLaunchKernelGGL(label_relabel_kernel, lin_grid, lin_block, 0, s, voxels, chunks, labels, (const int32_t*)root);
    return nca_launched(g_err, who);
}

// ---------------------------------------------------------------------------------------------------------------------- component sizes
constexpr int SZ_BLOCK = 256, SZ_NPT = 16, SZ_CHUNK = SZ_BLOCK * SZ_NPT, SZ_SLOTS = 256;
constexpr int64_t SZ_MAX_BLOCKS = (1LL << 32) / SZ_BLOCK;          // a launch carries at most 2^32 threads

// Block b owns 4096 consecutive nodes of volume v; a wave reads 64 consecutive nodes at a time.  The first lane of every run of equal labels
// within those 64 adds the run's length to the block's table in LDS: 256 slots, slot = label mod 256, claimed by the first label that
// comes; a label that finds its slot taken by another adds to `sizes` directly.  At the end every claimed slot is one add to `sizes`: one
// add per distinct label and block but for such collisions, however many nodes carry the label.  Integer adds: exact in any order.
__global__ void __launch_bounds__(SZ_BLOCK) label_sizes_kernel(int64_t voxels, int64_t chunks, int32_t cap, const int32_t* __restrict__ labels,
                                                               int32_t* __restrict__ sizes) {
    __shared__ int32_t s_key[SZ_SLOTS], s_cnt[SZ_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t bid = blockIdx.x;
    const int64_t v = bid / chunks, c0 = (bid % chunks) * SZ_CHUNK;
    int32_t* __restrict__ out = sizes + v * cap;
    s_key[tid] = -1;
    s_cnt[tid] = 0;
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < SZ_NPT; ++j) {
        const int64_t i = c0 + j * SZ_BLOCK + tid;
        const int32_t l = i < voxels ? labels[v * voxels + i] : -1;          // -1: past the volume, never counted
        const int32_t prev = __shfl_up(l, 1);
        const bool head = lane == 0 || prev != l;
        const unsigned long long heads = __ballot(head);
        if (!head || l < 0 || l >= cap) continue;
        const unsigned long long above = lane < 63 ? heads >> (lane + 1) : 0ull;
        const int32_t len = above ? __ffsll((long long)above) : 64 - lane;          // up to the next head, or the end of the wave
        const int slot = l & (SZ_SLOTS - 1);
        const int32_t owner = atomicCAS(&s_key[slot], -1, l);
        if (owner == -1 || owner == l)
            atomicAdd(&s_cnt[slot], len);
        else
            atomicAdd(out + l, len);
    }
    __syncthreads();
    if (s_key[tid] >= 0) atomicAdd(out + s_key[tid], s_cnt[tid]);
}

__global__ void label_zero_kernel(int32_t* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = 0;
}

extern "C" int nca_vol_label_sizes(const NcaGrid* grid, const int32_t* labels, int32_t n_vol, int32_t cap, int32_t* sizes, void* stream) {
    const char* who = "nca_vol_label_sizes";
    NCA_REFUSE_NULL_GRID(g_err, who, grid);
    NCA_REFUSE_NULL(g_err, who, labels);
    NCA_REFUSE_NULL(g_err, who, sizes);
    NcaGrid g;
    int64_t nodes;
    const int rc = label_check(who, grid, n_vol, &g, &nodes);
    if (rc != NCA_OK) return rc;
    NCA_REFUSE_NOT_POSITIVE(g_err, who, "cap", cap);
    const int64_t voxels = nodes / n_vol, chunks = (voxels + SZ_CHUNK - 1) / SZ_CHUNK;
    const int rcb = nca_check_launch_blocks(g_err, who, n_vol, g, chunks * n_vol, 0, 0, SZ_MAX_BLOCKS);
    if (rcb != NCA_OK) return rcb;
    hipStream_t s = (hipStream_t)stream;
    // the clear is a KERNEL on the stream, not hipMemsetAsync: a memset node captured into a HIP graph does not replay to what the eager call does
    // (tests/test_graph_replay_gpu.py: the sizes came back on top of what the buffer held)
    const int64_t n_sizes = (int64_t)n_vol * cap, zb = (n_sizes + SZ_BLOCK - 1) / SZ_BLOCK;
    hipLaunchKernelGGL(label_zero_kernel, dim3((unsigned)(zb < 65536 ? zb : 65536)), dim3(SZ_BLOCK), 0, s, sizes, n_sizes);
    const int rcz = nca_launched(g_err, who);
    if (rcz != NCA_OK) return rcz;
    hipLaunchKernelGGL(label_sizes_kernel, dim3((unsigned)(chunks * n_vol)), dim3(SZ_BLOCK), 0, s, voxels, chunks, cap, labels, sizes);
    return nca_launched(g_err, who);
}
