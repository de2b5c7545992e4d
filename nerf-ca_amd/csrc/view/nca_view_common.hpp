// nca_view_common.hpp -- what the translation units of csrc/view/ share (internal; nothing here is exported): the error message of a
// section; for the thirteen grid-taking sections (drr project and backproject, vol, phantom, edt, filt, resample, skel, label, vess, mesh, path, cpr) the refusals of a NULL descriptor
// and of a count that is not positive and the NcaGrid checks, and all of them in order as nca_check_stack (edt, filt, resample, skel, label, vess, mesh, path, cpr; the first five's, mesh's and path's query and
// entry point share them); the count of 4 x 8 x 64 tiles (vol, phantom, skel, label, vess, mesh, path); the largest of three launches' block counts against one launch's limit
// (edt, filt, resample; skel and vess with one count, label, mesh and path with one or two); the workspace refusal (ssim, edt, filt, resample, skel, label, mesh, path); and, for hipcc only, the launch epilogue and
// the tile's indexing on the device.  The Python wrappers' counterpart is nerf-ca_amd/_view.py.  Every text below is part of the library's behaviour: tests and callers
// match on it.
//
// The host part is plain C++17 without HIP types: g++ compiles it on its own, as it does nca_rng.hpp.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif
#include "../../../include/nerfca_hip.h"

static_assert(sizeof(NcaGrid) == 64, "NcaGrid is 64 bytes without padding");

namespace {          // internal linkage: every translation unit has its own copy, the library exports none of it

// The message of the calling thread's last failed call of ONE section.  Each translation unit keeps its own `static thread_local` instance
// behind its own exported nca_*_last_error: the sections share the type, never a buffer.
struct NcaViewErr {
    char msg[256] = "";

    __attribute__((format(printf, 3, 4))) int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        return code;
    }
};

// "<who>: <p> is NULL" for a pointer argument named as the header names it
#define NCA_REFUSE_NULL(err, who, p)                                              \
    do {                                                                          \
        if (!(p)) return (err).fail(NCA_E_INVALID, "%s: " #p " is NULL", who); \
    } while (0)

// "<who>: the grid descriptor is NULL", and "<who>: <name> = <n> is not positive" for an int32 count under the name the header gives it
#define NCA_REFUSE_NULL_GRID(err, who, grid)                                                      \
    do {                                                                                          \
        if (!(grid)) return (err).fail(NCA_E_INVALID, "%s: the grid descriptor is NULL", who); \
    } while (0)
#define NCA_REFUSE_NOT_POSITIVE(err, who, name, n)                                                                   \
    do {                                                                                                             \
        if ((n) <= 0) return (err).fail(NCA_E_INVALID, "%s: %s = %d is not positive", who, name, (int)(n)); \
    } while (0)

// The grid checks, after the caller has refused a NULL `grid` and a `count` (volumes or phases, the `noun`) that is not positive (the two
// macros above, or nca_check_stack, which does all three): reserved,
// then per axis the node count, lo, inv, then that count x n0 n1 n2 nodes of `node_bytes` bytes fit int64.  On success *g is the caller's
// copy of the descriptor and *voxels = n0 n1 n2.
inline int nca_check_grid(NcaViewErr& err, const char* who, const NcaGrid* grid, int32_t count, int node_bytes, const char* noun, NcaGrid* g,
                          int64_t* voxels) {
    *g = *grid;
    if (g->reserved != 0) return err.fail(NCA_E_INVALID, "%s: reserved = %d is not 0", who, (int)g->reserved);
    for (int a = 0; a < 3; ++a) {
        if (g->n[a] < 2) return err.fail(NCA_E_INVALID, "%s: n[%d] = %d is less than 2 nodes", who, a, (int)g->n[a]);
        if (!isfinite(g->lo[a])) return err.fail(NCA_E_INVALID, "%s: lo[%d] = %g is not finite", who, a, g->lo[a]);
        if (!isfinite(g->inv[a])) return err.fail(NCA_E_INVALID, "%s: inv[%d] = %g is not finite", who, a, g->inv[a]);
        if (!(g->inv[a] > 0.0)) return err.fail(NCA_E_INVALID, "%s: inv[%d] = %g is not positive", who, a, g->inv[a]);
    }
    const int64_t n01 = (int64_t)g->n[0] * g->n[1];          // < 2^62 always
    if (n01 > (INT64_MAX / node_bytes / count) / g->n[2])
        return err.fail(NCA_E_INVALID, "%s: %d %s of %d x %d x %d voxels overflow int64", who, (int)count, noun, (int)g->n[0], (int)g->n[1], (int)g->n[2]);
    *voxels = n01 * g->n[2];
    return NCA_OK;
}

// Everything a stack of `count` volumes on one grid is checked for, in this order: the descriptor is not NULL, `count` (named `count_name`
// in the message) is positive, nca_check_grid with `node_bytes` bytes per node, and -- unless max_axis is 0 -- no axis is longer than
// max_axis = NCA_EDT_MAX_AXIS nodes (the kernels that stage whole lines).  On success *g is the caller's copy and *nodes = count n0 n1 n2.
inline int nca_check_stack(NcaViewErr& err, const char* who, const NcaGrid* grid, int32_t count, const char* count_name, int node_bytes, const char* noun,
                           int max_axis, NcaGrid* g, int64_t* nodes) {
    NCA_REFUSE_NULL_GRID(err, who, grid);
    NCA_REFUSE_NOT_POSITIVE(err, who, count_name, count);
    int64_t voxels;
    const int rc = nca_check_grid(err, who, grid, count, node_bytes, noun, g, &voxels);
    if (rc != NCA_OK) return rc;
    for (int a = 0; a < 3 && max_axis; ++a)
        if (g->n[a] > max_axis)
            return err.fail(NCA_E_UNSUPPORTED, "%s: n[%d] = %d is longer than NCA_EDT_MAX_AXIS = %d", who, a, (int)g->n[a], max_axis);
    *nodes = voxels * count;
    return NCA_OK;
}

// The three launches of an entry point make b0, b1 and b2 blocks: refused when the largest is more than `cap`, what one launch covers.
inline int nca_check_launch_blocks(NcaViewErr& err, const char* who, int32_t n_vol, const NcaGrid& g, int64_t b0, int64_t b1, int64_t b2, int64_t cap) {
    const int64_t most = b0 > b1 ? (b0 > b2 ? b0 : b2) : (b1 > b2 ? b1 : b2);
    if (most <= cap) return NCA_OK;
    return err.fail(NCA_E_INVALID, "%s: %d volumes of %d x %d x %d voxels make %lld tiles, more than one launch covers", who, (int)n_vol, (int)g.n[0], (int)g.n[1],
                    (int)g.n[2], (long long)most);
}

// A workgroup of vol and phantom owns a tile of 4 x 8 x 64 nodes.  nb[a] = ceil(n[a] / tile[a]) and *tiles = nb0 nb1 nb2 of a checked
// grid; refused when one launch cannot carry them -- times `phases` where the phase is an outer dimension of the same launch (phantom),
// phases = 0 where there is none (vol).
constexpr int NCA_TILE0 = 4, NCA_TILE1 = 8, NCA_TILE2 = 64;

inline int nca_count_tiles(NcaViewErr& err, const char* who, const NcaGrid& g, int32_t phases, int32_t nb[3], int64_t* tiles) {
    const int tile[3] = {NCA_TILE0, NCA_TILE1, NCA_TILE2};
    for (int a = 0; a < 3; ++a) nb[a] = (int32_t)(((int64_t)g.n[a] + tile[a] - 1) / tile[a]);
    *tiles = (int64_t)nb[0] * nb[1] * nb[2];          // at most the voxel count: no overflow
    if (*tiles <= 0x7fffffffLL / (phases ? phases : 1)) return NCA_OK;
    if (phases)
        return err.fail(NCA_E_INVALID, "%s: %d phases of %d x %d x %d voxels make %lld x %d tiles, more than one launch covers", who, (int)phases, (int)g.n[0],
                        (int)g.n[1], (int)g.n[2], (long long)*tiles, (int)phases);
    return err.fail(NCA_E_INVALID, "%s: %d x %d x %d voxels make %lld tiles, more than one launch covers", who, (int)g.n[0], (int)g.n[1], (int)g.n[2],
                    (long long)*tiles);
}

inline int nca_check_workspace(NcaViewErr& err, const char* who, const void* work, size_t work_bytes, size_t need) {
    if (!work || work_bytes < need)
        return err.fail(NCA_E_WORKSPACE, "%s: the workspace holds %llu bytes%s, %llu are needed", who, (unsigned long long)work_bytes, work ? "" : " (work is NULL)",
                        (unsigned long long)need);
    return NCA_OK;
}

#ifdef __HIPCC__
// After the last launch of an entry point: hipGetLastError once.
inline int nca_launched(NcaViewErr& err, const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return err.fail(NCA_E_HIP, "%s: %s", who, hipGetErrorString(e));
    return NCA_OK;
}

// The tile on the device: eight waves; wave w takes the rows (j0, j1) = (k, w), k = 0 .. 3, with its 64 lanes along the last (contiguous)
// axis, so a thread owns the 4 nodes (k, wave, lane) and every load or store of a wave is a full line.
constexpr int NCA_TILE_BLOCK = 512, NCA_TILE_WAVES = NCA_TILE_BLOCK / 64;
constexpr int NCA_TILE_NPT = NCA_TILE0 * NCA_TILE1 * NCA_TILE2 / NCA_TILE_BLOCK;
static_assert(NCA_TILE2 == 64 && NCA_TILE_WAVES == NCA_TILE1 && NCA_TILE_NPT == NCA_TILE0, "a wave is one row of the tile: node k of a thread is (k, wave, lane)");

// tile t of a grid with nb1 x nb2 tiles per slab of tiles: its first node
struct NcaTile {
    int32_t base0, base1, base2;
};

__device__ __forceinline__ NcaTile nca_tile(int64_t t, int32_t nb1, int32_t nb2) {
    const int32_t base2 = (int32_t)(t % nb2) * NCA_TILE2, base1 = (int32_t)((t / nb2) % nb1) * NCA_TILE1, base0 = (int32_t)(t / ((int64_t)nb2 * nb1)) * NCA_TILE0;
    return {base0, base1, base2};
}

// the thread's own nodes (i0, i1, i2) = (base0 + k, base1 + wave, base2 + lane) of a grid of n0 x n1 x n2 nodes
struct NcaTileNodes {
    int32_t base0, i1, i2, n0, n1, n2;
    bool ok12;          // (i1, i2) is inside the grid
    int64_t off_t;      // the offset of node k = 0

    __device__ __forceinline__ bool live(int k) const { return ok12 && base0 + k < n0; }
    __device__ __forceinline__ int64_t off(int k) const { return off_t + (int64_t)k * n1 * n2; }          // used only where live
};

__device__ __forceinline__ NcaTileNodes nca_tile_nodes(NcaTile t, int wave, int lane, int32_t n0, int32_t n1, int32_t n2) {
    const int32_t i1 = t.base1 + wave, i2 = t.base2 + lane;
    return {t.base0, i1, i2, n0, n1, n2, i2 < n2 && i1 < n1, ((int64_t)t.base0 * n1 + i1) * n2 + i2};
}
#endif
}          // namespace
