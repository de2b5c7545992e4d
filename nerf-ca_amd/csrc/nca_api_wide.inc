// nca_api_wide.inc -- host side of the general kernels (nca_wide.hpp), included by nca_api.hip: planning of a chunk's regions in the caller's
// workspace and the kernel sequence of one net's forward / backward over the chunks.
//
// A chunk is a run of consecutive samples (n = ray * S + sample, or the point index) whose activations fit the workspace: rows padded to a
// multiple of 128, at most 2^18.  Forward results do not depend on the chunking; a backward sums its weight gradients chunk by chunk in
// order, each chunk in `nsplit` position-ordered parts, so the bits of a gradient are a function of (sample count, workspace size) -- run
// to run identical.

static int wide_layout_of(const NcaNet* net, NcaWideLayout* y, int32_t prec) {
    if (!net) return fail(NCA_E_INVALID, "net is NULL");
    if (prec != NCA_PREC_F32)
        return fail(NCA_E_UNSUPPORTED, "bf16 mode runs nets of up to 128 units with 3 -> 1 channels; wider nets and other channel counts run on the general f32 kernels");
    const char* why = "";
    int rc = nca_build_layout_wide(*net, y, &why);
    if (rc != NCA_OK) return fail(rc, "%s", why);
    return NCA_OK;
}
static bool is_wide(const NcaNet* net) { return net && nca_net_is_wide(*net); }

struct WidePlan {
    int64_t chunk;            // rows per chunk (multiple of 128)
    int32_t nsplit;
    int64_t split_stride;     // floats per split of the slab (a split is laid out like the packed image)
    int64_t off_x0, off_h, off_m, off_d, off_slab, off_esum;      // floats from the workspace base; H_j at off_h + j * chunk * F (forward: j & 1), D_i at off_d + i * chunk * F
    int64_t mbits;            // floats of one layer's ReLU bit masks (backward: M_j at off_m + j * mbits, j < NL - 1)
    int64_t bytes;
};
static void wide_plan(const NcaWideLayout& y, int64_t N, bool bwd, int64_t max_bytes, WidePlan* p) {
    const int64_t rows_all = align_up(N, NCA_WIDE_ROWS);
    int64_t chunk = rows_all < (1 << 18) ? rows_all : (1 << 18);
    const int64_t tiles = ((y.F + 127) / 128) * ((y.F + 127) / 128);
    const int64_t want = 512 / tiles > 1 ? 512 / tiles : 1;
    p->split_stride = y.packed_floats;
    for (;;) {
        p->chunk = chunk;
        p->nsplit = (int32_t)(want < chunk / NCA_WIDE_ROWS ? want : chunk / NCA_WIDE_ROWS);
        p->off_x0 = 0;
        p->off_h = chunk * y.K0p;
        p->off_m = p->off_h + chunk * y.F * (bwd ? y.NL : 2);
        p->mbits = (chunk / NCA_WIDE_ROWS) * ((y.F + 127) / 128) * 512;
        p->off_d = p->off_m + (bwd ? (int64_t)(y.NL - 1) * p->mbits : 0);
        p->off_slab = p->off_d + (bwd ? 2 * chunk * y.F : 0);
        p->off_esum = p->off_slab + (bwd ? p->nsplit * p->split_stride : 0);
        p->bytes = align_up((p->off_esum + (bwd ? (int64_t)y.F * y.P : 0)) * 4, 256);
        if (max_bytes <= 0 || p->bytes <= max_bytes || chunk <= NCA_WIDE_ROWS) return;
        chunk = align_up(chunk / 2, NCA_WIDE_ROWS);
    }
}

struct WideBind {
    NcaWideLayout y;
    const float* packed; const float* lat; const float* win; const float* four;
};
static int wide_bind(const NetBind& b, int32_t prec, WideBind* w) {
    int rc = wide_layout_of(b.net, &w->y, prec);
    if (rc) return rc;
    if (!b.packed) return fail(NCA_E_INVALID, "packed weights pointer is NULL");
    if (w->y.T > 0 && !b.params) return fail(NCA_E_INVALID, "dynamic net needs its natural parameters (time latents)");
    if (w->y.enc_mode == NCA_ENC_FOURIER && !b.four) return fail(NCA_E_INVALID, "fourier coefficients are NULL");
    w->packed = static_cast<const float*>(b.packed);
    w->lat = w->y.T > 0 ? b.params + w->y.lat_off : nullptr;
    w->win = b.win;          // (null: unit window)
    w->four = b.four;
    return NCA_OK;
}

// layers 0 .. NL-1 of one chunk; H_j at hbase + (all ? j : j & 1) * chunk * F
static int wide_layers(const WideBind& w, const WidePlan& p, float* ws, int64_t rows, bool all, hipStream_t st) {
    const NcaWideLayout& y = w.y;
    const float* X0 = ws + p.off_x0;
    for (int j = 0; j < y.NL; ++j) {
        const NcaWideLayer& l = y.layer[j];
        float* Hj = ws + p.off_h + (int64_t)(all ? j : (j & 1)) * p.chunk * y.F;
        const float* Hp = j > 0 ? ws + p.off_h + (int64_t)(all ? j - 1 : ((j - 1) & 1)) * p.chunk * y.F : nullptr;
        NcaWideGemmArgs g{};
        if (l.kind == NCA_IN_HID) { g.A[0] = Hp; g.lda[0] = y.F; g.ka[0] = y.F; }
        else { g.A[0] = X0; g.lda[0] = y.K0p; g.ka[0] = y.K0p; }
        if (l.kind == NCA_IN_SKIP) { g.A[1] = Hp; g.lda[1] = y.F; g.ka[1] = y.F; }
        g.B = w.packed + l.pw_off; g.ldb = l.Kp;
        g.C = Hj; g.ldc = y.F;
        g.rows = rows; g.cols = y.F;
        g.bias = w.packed + y.pb_off + (int64_t)j * y.F; g.relu = 1;
        if (all && j < y.NL - 1) g.maskbits = reinterpret_cast<uint32_t*>(ws + p.off_m + (int64_t)j * p.mbits);          // for the dgrad launch that produces D_j
        HIPCHK(nca_launch_wide_gemm(NCA_WG_FWD, g, st));
    }
    return NCA_OK;
}

static void wide_enc_args(const WideBind& w, const NcaWideGeom& geom, const WidePlan& p, float* ws, int64_t n0, int64_t n_valid, int64_t rows, bool onehot, NcaWideEncArgs* e) {
    const NcaWideLayout& y = w.y;
    memset(e, 0, sizeof(*e));
    e->g = geom;
    e->g.C = y.C;
    e->n0 = n0; e->n_valid = n_valid; e->rows = rows;
    e->enc_mode = y.enc_mode; e->L = y.L; e->Kenc = y.Kenc; e->T = y.T; e->P = y.P; e->K0 = y.K0; e->K0p = y.K0p;
    e->onehot = onehot ? 1 : 0;
    e->win = w.win; e->four = w.four;
    e->lat = w.lat;
    e->X0 = ws + p.off_x0;
}

// raw[n][o], n in [0, N)
static int wide_forward(const WideBind& w, const NcaWideGeom& geom, int64_t N, float* raw, void* work, int64_t work_bytes, hipStream_t st) {
    const NcaWideLayout& y = w.y;
    if (y.T > 0 && !geom.phase) return fail(NCA_E_INVALID, "dynamic net needs phase ids");
    WidePlan p;
    wide_plan(y, N, false, work_bytes, &p);
    if (!work || p.bytes > work_bytes) return fail(NCA_E_WORKSPACE, "general kernels: forward workspace %lld < %lld bytes", (long long)work_bytes, (long long)p.bytes);
    float* ws = static_cast<float*>(work);
    Span sp(NCA_K_FWD, st);
    for (int64_t n0 = 0; n0 < N; n0 += p.chunk) {
        const int64_t n_valid = N - n0 < p.chunk ? N - n0 : p.chunk;
        const int64_t rows = align_up(n_valid, NCA_WIDE_ROWS);
        NcaWideEncArgs e;
        wide_enc_args(w, geom, p, ws, n0, n_valid, rows, false, &e);
        HIPCHK(nca_launch_wide_encode(e, st));
        int rc = wide_layers(w, p, ws, rows, false, st);
        if (rc) return rc;
        const float* Hl = ws + p.off_h + (int64_t)((y.NL - 1) & 1) * p.chunk * y.F;
        HIPCHK(nca_launch_wide_head_fwd(n_valid, y.F, y.Cout, Hl, w.packed + y.pwo_off, w.packed + y.pbo_off, raw + n0 * y.Cout, st));
    }
    return NCA_OK;
}

// ---- backward of one chunk, in two halves so that a ray batch can run the compositing chain rule in between (the per-sample raw gradient needs the raw
// fields of BOTH nets): wide_chunk_forward leaves every layer's output of the chunk in the net's region (and the raw field where the caller wants it),
// wide_chunk_backward sweeps back from them and ADDS the chunk's parameter gradient to `grads`
static void wide_plan_rows(const NcaWideLayout& y, int64_t rows, WidePlan* p) {          // the backward regions of a chunk of exactly `rows` rows
    wide_plan(y, rows, true, 0, p);
    if (p->chunk != rows) {          // (more than 2^18 rows: the caller asked for them)
        const int64_t tiles = ((y.F + 127) / 128) * ((y.F + 127) / 128);
        const int64_t want = 512 / tiles > 1 ? 512 / tiles : 1;
        p->chunk = rows;
        p->nsplit = (int32_t)(want < rows / NCA_WIDE_ROWS ? want : rows / NCA_WIDE_ROWS);
        p->off_h = rows * y.K0p;
        p->off_m = p->off_h + rows * y.F * y.NL;
        p->mbits = (rows / NCA_WIDE_ROWS) * ((y.F + 127) / 128) * 512;
        p->off_d = p->off_m + (int64_t)(y.NL - 1) * p->mbits;
        p->off_slab = p->off_d + 2 * rows * y.F;
        p->off_esum = p->off_slab + p->nsplit * p->split_stride;
        p->bytes = align_up((p->off_esum + (int64_t)y.F * y.P) * 4, 256);
    }
}
// (`ws` of the two: the base of the chunk's ACTIVATIONS -- X0 and every H_j, p.off_d floats: the head of a workspace region, or a chunk's block of a forward store)
static int wide_chunk_forward(const WideBind& w, const NcaWideGeom& geom, const WidePlan& p, float* ws, int64_t n0, int64_t n_valid, int64_t rows, float* raw_chunk,
                              hipStream_t st, int span_kind = NCA_K_BWD_DGRAD) {
    const NcaWideLayout& y = w.y;
    Span sp(span_kind, st);
    NcaWideEncArgs e;
    wide_enc_args(w, geom, p, ws, n0, n_valid, rows, true, &e);
    HIPCHK(nca_launch_wide_encode(e, st));
    int rc = wide_layers(w, p, ws, rows, true, st);
    if (rc) return rc;
    if (raw_chunk)
        HIPCHK(nca_launch_wide_head_fwd(n_valid, y.F, y.Cout, ws + p.off_h + (int64_t)(y.NL - 1) * p.chunk * y.F, w.packed + y.pwo_off, w.packed + y.pbo_off, raw_chunk, st));
    return NCA_OK;
}
// `acts`: the chunk's activations (as wide_chunk_forward left them); `scr`: the scratch behind them -- D blocks, split slabs, per-phase sums -- addressed with the
// plan's offsets MINUS p.off_d (scr == acts + p.off_d when both sit in one workspace region)
static int wide_chunk_backward(const WideBind& w, const WidePlan& p, const float* acts, float* scr, int64_t n_valid, int64_t rows, const float* g, float* grads, hipStream_t st) {
    const NcaWideLayout& y = w.y;
    float* slab = scr + (p.off_slab - p.off_d);
    const int nsplit = (int)(p.nsplit < rows / NCA_WIDE_ROWS ? p.nsplit : rows / NCA_WIDE_ROWS);
    const float* X0 = acts + p.off_x0;
    auto H = [&](int j) { return acts + p.off_h + (int64_t)j * p.chunk * y.F; };
    float* D[2] = {scr, scr + p.chunk * y.F};
    int cur = 0;
    {
        Span sp(NCA_K_BWD_DGRAD, st);
        HIPCHK(nca_launch_wide_head_bwd(n_valid, rows, y.F, y.Cout, H(y.NL - 1), w.packed + y.pwo_off, g, D[cur], st));
    }
    {
        Span sp(NCA_K_BWD_WGRAD, st);
        HIPCHK(nca_launch_wide_colsum(n_valid, y.F, y.Cout, H(y.NL - 1), y.F, g, slab + y.pwo_off, p.split_stride, slab + y.pbo_off, nsplit, st));
    }
    for (int j = y.NL - 1; j >= 0; --j) {
        const NcaWideLayer& l = y.layer[j];
        {
            Span sp(NCA_K_BWD_WGRAD, st);
            // dWp_j[f][k] = sum_n D_j[n][f] In_j[n][k]: the encoded part (layer 0, skip layers) and / or the hidden part; the layer's first launch also leaves the
            // bias gradient sum_n D_j[n][f] (the sums of its A operand) in the slabs
            bool bias_done = false;
            for (int part = 0; part < 2; ++part) {
                const bool enc_part = part == 0;
                if (enc_part && l.kind == NCA_IN_HID) continue;
                if (!enc_part && l.kind == NCA_IN_ENC) continue;
                NcaWideGemmArgs gw{};
                gw.A[0] = D[cur]; gw.lda[0] = y.F; gw.ka[0] = rows;
                gw.B = enc_part ? X0 : H(j - 1); gw.ldb = enc_part ? y.K0p : y.F;
                gw.C = slab + l.pw_off + ((!enc_part && l.kind == NCA_IN_SKIP) ? y.K0p : 0); gw.ldc = l.Kp;
                gw.rows = y.F; gw.cols = enc_part ? y.K0p : y.F;
                gw.nsplit = nsplit; gw.split_stride = p.split_stride;
                if (!bias_done) { gw.rowsum = slab + y.pb_off + (int64_t)j * y.F; bias_done = true; }
                HIPCHK(nca_launch_wide_gemm(NCA_WG_WGRAD, gw, st));
            }
        }
        if (j > 0) {
            Span sp(NCA_K_BWD_DGRAD, st);
            NcaWideGemmArgs gd{};
            gd.A[0] = D[cur]; gd.lda[0] = y.F; gd.ka[0] = y.F;
            gd.B = w.packed + l.pw_off + (l.kind == NCA_IN_SKIP ? y.K0p : 0); gd.ldb = l.Kp;
            gd.C = D[1 - cur]; gd.ldc = y.F;
            gd.rows = rows; gd.cols = y.F;
            gd.maskbits = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(acts + p.off_m + (int64_t)(j - 1) * p.mbits));
            HIPCHK(nca_launch_wide_gemm(NCA_WG_DGRAD, gd, st));
            cur = 1 - cur;
        }
    }
    Span sp(NCA_K_BWD_REDUCE, st);
    NcaWideReduceArgs r{};
    r.y = y;
    r.slab = slab; r.split_stride = p.split_stride; r.nsplit = nsplit;
    r.packed = w.packed; r.grads = grads; r.esum = scr + (p.off_esum - p.off_d);
    HIPCHK(nca_launch_wide_reduce(r, st));
    return NCA_OK;
}

// grads (natural, overwritten) from g_raw[n][o]: a batch of points
static int wide_backward(const WideBind& w, const NcaWideGeom& geom, int64_t N, const float* g_raw, float* grads, void* work, int64_t work_bytes, hipStream_t st) {
    const NcaWideLayout& y = w.y;
    if (y.T > 0 && !geom.phase) return fail(NCA_E_INVALID, "dynamic net needs phase ids");
    WidePlan p;
    wide_plan(y, N, true, work_bytes, &p);
    if (!work || p.bytes > work_bytes) return fail(NCA_E_WORKSPACE, "general kernels: backward workspace %lld < %lld bytes", (long long)work_bytes, (long long)p.bytes);
    float* ws = static_cast<float*>(work);
    HIPCHK(nca_launch_wide_zero(grads, y.n_params, st));          // (a kernel, not hipMemsetAsync: nca_wide.hpp)
    for (int64_t n0 = 0; n0 < N; n0 += p.chunk) {
        const int64_t n_valid = N - n0 < p.chunk ? N - n0 : p.chunk;
        const int64_t rows = align_up(n_valid, NCA_WIDE_ROWS);
        int rc = wide_chunk_forward(w, geom, p, ws, n0, n_valid, rows, nullptr, st);
        if (rc) return rc;
        rc = wide_chunk_backward(w, p, ws, ws + p.off_d, n_valid, rows, g_raw + n0 * y.Cout, grads, st);
        if (rc) return rc;
    }
    return NCA_OK;
}

static void rays_to_geom(const NcaRays* r, NcaWideGeom* g) {
    memset(g, 0, sizeof(*g));
    g->mode = NCA_MODE_RAYS;
    g->S = r->S; g->ray_is_f64 = r->ray_is_f64; g->C = 3;
    g->origins = r->origins; g->dirs = r->dirs;
    g->z = r->z; g->zs_r = r->z_stride_r;
    g->phase = r->phase; g->ps_r = r->phase_stride_r; g->ps_s = r->phase_stride_s;
}

// ---- ray batches with a net on the general kernels: every net leaves its RAW field in its sigma buffer (general kernels, or one raw_only launch of
// the fused kernels for a net they cover), then the stand-alone compositing kernel turns raw fields into sigmas and pix in place -- the path nets of
// different width take anyway
static int fused_raw_forward(const NcaRays* rays, int32_t prec, const NetBind& b, float* raw, hipStream_t st) {
    static thread_local NcaFusedArgs one;
    memset(&one, 0, sizeof(one));
    rays_to_args(rays, &one, prec);
    one.nnets = 1;
    int rc = fill_net(b, &one.net[0], prec);
    if (rc) return rc;
    if (one.net[0].lay.T > 0 && !rays->phase) return fail(NCA_E_INVALID, "dynamic net needs phase ids");
    one.ntiles = rays->R * one.nchunk;
    one.raw_only = 1;
    one.raw_out = raw;
    NetBind b1[2] = {b, {}};
    rc = build_stages(&one, b1, false);
    if (rc) return rc;
    const int64_t ngroups = (one.ntiles + NCA_WAVES - 1) / NCA_WAVES;
    const int grid = (int)(ngroups < num_cus() ? ngroups : num_cus());
    if (prec == NCA_PREC_BF16) plan_resident(&one, NCA_KM_FWD);
    Span sp(NCA_K_FWD, st);
    if (prec == NCA_PREC_BF16) HIPCHK(nca_launch_fused_bf16(one.net[0].lay.F, one, false, grid, st));
    else HIPCHK(nca_launch_fused_f32(one.net[0].lay.F, one, false, grid, st));
    return NCA_OK;
}

// runs of whole rays: what a ray batch's backward (and a forward that writes a store) is cut into
struct RayChunks { int64_t rays, rows; WidePlan p[2]; int64_t off[2]; int64_t bytes; };          // rows = align_up(rays * S, 128); off: floats
static int plan_ray_chunks(const NcaWideLayout* lays, const bool* wide, int nn, int64_t R, int32_t S, int64_t budget, RayChunks* rc_) {
    int64_t rays = ((int64_t)1 << 18) / S;
    if (rays < 1) rays = 1;
    if (rays > R) rays = R;
    for (;;) {
        rc_->rays = rays;
        rc_->rows = align_up(rays * S, NCA_WIDE_ROWS);
        int64_t off = 0;
        for (int n = 0; n < nn; ++n) {
            rc_->off[n] = off;
            if (!wide[n]) continue;
            wide_plan_rows(lays[n], rc_->rows, &rc_->p[n]);
            off += rc_->p[n].bytes / 4;
        }
        rc_->bytes = off * 4;
        if (budget <= 0 || rc_->bytes <= budget || rays == 1) return rc_->bytes <= budget || budget <= 0 ? NCA_OK : NCA_E_WORKSPACE;
        rays = (rays + 1) / 2;
    }
}

// ---- the forward STORE of a ray batch whose nets all run on the general kernels: what autograd keeps in the reference (train/run_composite.py:306) -- every layer's
// output of every sample, f32.  Laid out by runs of whole rays (the backward's chunks: min(R, 2^18 / S) rays), per run one activation block per net (X0 | H_0 .. H_{NL-1}, the
// head of a backward region: WidePlan.off_d floats), behind all runs the raw fields f32[R, S] per net.  A backward from it recomputes nothing.
struct GeneralStore { RayChunks ch; int64_t run_stride, n_runs, raw_off, bytes; };          // floats
static bool general_store_plan(const NcaWideLayout* lays, int nn, int64_t R, int32_t S, GeneralStore* gs) {
    bool wide[2] = {true, true};
    if (plan_ray_chunks(lays, wide, nn, R, S, 0, &gs->ch) != NCA_OK) return false;
    gs->run_stride = 0;
    for (int n = 0; n < nn; ++n) gs->run_stride += gs->ch.p[n].off_d;
    gs->n_runs = (R + gs->ch.rays - 1) / gs->ch.rays;
    gs->raw_off = gs->n_runs * gs->run_stride;
    gs->bytes = align_up((gs->raw_off + (int64_t)nn * R * S) * 4, 256);
    return true;
}
static int64_t general_store_bytes(const NcaRays* rays, const NcaNet* const* nets, int nn, int32_t prec) {
    NcaWideLayout lays[2];
    for (int n = 0; n < nn; ++n) {
        if (!is_wide(nets[n])) return 0;          // (a fused-kernel net beside a general one: no store, the backward recomputes)
        int rc = wide_layout_of(nets[n], &lays[n], prec);
        if (rc) return rc;
    }
    GeneralStore gs;
    return general_store_plan(lays, nn, rays->R, rays->S, &gs) ? gs.bytes : 0;
}

static int64_t general_fwd_bytes(const NcaRays* rays, const NcaNet* const* nets, int nn, int32_t prec, int64_t max_bytes) {
    int64_t most = 0;
    for (int n = 0; n < nn; ++n) {
        if (!is_wide(nets[n])) continue;
        NcaWideLayout y;
        int rc = wide_layout_of(nets[n], &y, prec);
        if (rc) return rc;
        WidePlan p;
        wide_plan(y, rays->R * (int64_t)rays->S, false, max_bytes, &p);
        if (p.bytes > most) most = p.bytes;
    }
    return most;
}

static int render_fwd_general(const NcaRays* rays, int32_t prec, const NetBind* binds, int nn, double* pix, float* sig_s, float* sig_d,
                              void* work, int64_t work_bytes, void* store, int64_t store_bytes, hipStream_t st) {
    if (store) {
        // every net on the general kernels: the storing forward of the backward's runs of whole rays, straight into the store (no workspace)
        WideBind wb[2];
        NcaWideLayout lays[2];
        for (int n = 0; n < nn; ++n) {
            if (!is_wide(binds[n].net)) return fail(NCA_E_UNSUPPORTED, "a forward store needs both nets on the fused kernels, or both on the general kernels");
            int rc = wide_bind(binds[n], prec, &wb[n]);
            if (rc) return rc;
            if (wb[n].y.C != 3 || wb[n].y.Cout != 1) return fail(NCA_E_UNSUPPORTED, "a ray batch needs nets with 3 input channels and 1 output channel");
            if (wb[n].y.T > 0 && !rays->phase) return fail(NCA_E_INVALID, "dynamic net needs phase ids");
            lays[n] = wb[n].y;
        }
        if (nn == 2 && wb[0].y.T > 0) return fail(NCA_E_INVALID, "first net of a composite render must be static (T == 0)");
        if (!pix) return fail(NCA_E_UNSUPPORTED, "pix = NULL (ray sums left to the loss kernel) needs both nets on the fused kernels");
        GeneralStore gs;
        if (!general_store_plan(lays, nn, rays->R, rays->S, &gs) || store_bytes < gs.bytes)
            return fail(NCA_E_WORKSPACE, "forward store %lld < %lld bytes", (long long)store_bytes, (long long)gs.bytes);
        NcaWideGeom geom;
        rays_to_geom(rays, &geom);
        NcaPlan pl;
        memset(&pl, 0, sizeof(pl));
        pl.fwd_launches = nn;
        pl.fwd_store_format = NCA_STORE_GENERAL;
        pl.wave_tiles = rays->R * ((rays->S + tile_samples(prec) - 1) / tile_samples(prec));
        publish_plan(pl, true, rays->plan_out);
        float* sb = static_cast<float*>(store);
        float* outs[2] = {sig_s, sig_d};
        const int64_t S = rays->S;
        int64_t run = 0;
        for (int64_t r0 = 0; r0 < rays->R; r0 += gs.ch.rays, ++run) {
            const int64_t nr = rays->R - r0 < gs.ch.rays ? rays->R - r0 : gs.ch.rays;
            const int64_t n0 = r0 * S, n_valid = nr * S, rows = align_up(n_valid, NCA_WIDE_ROWS);
            float* blk = sb + run * gs.run_stride;
            for (int n = 0; n < nn; ++n) {
                int rc = wide_chunk_forward(wb[n], geom, gs.ch.p[n], blk, n0, n_valid, rows, outs[n] + n0, st, NCA_K_FWD);
                if (rc) return rc;
                blk += gs.ch.p[n].off_d;
            }
        }
        // the raw fields stay in the store's tail for the backward's compositing chain rule; the sigma buffers become sigmas in place
        for (int n = 0; n < nn; ++n)
            HIPCHK(nca_launch_wide_copy(sb + gs.raw_off + (int64_t)n * rays->R * S, outs[n], rays->R * S, st));
        int rc = nca_composite_fwd(rays->R, rays->S, rays->act, rays->single_field, rays->scale, sig_s, nn == 2 ? sig_d : nullptr, rays->I0, rays->dists, pix, sig_s,
                                   nn == 2 ? sig_d : nullptr, (void*)st);
        return rc ? rc : NCA_STORE_GENERAL;
    }
    if (!pix) return fail(NCA_E_UNSUPPORTED, "pix = NULL (ray sums left to the loss kernel) needs both nets on the fused kernels");
    float* outs[2] = {sig_s, sig_d};
    NcaWideGeom geom;
    rays_to_geom(rays, &geom);
    NcaPlan pl;
    memset(&pl, 0, sizeof(pl));
    pl.fwd_launches = nn;
    pl.wave_tiles = rays->R * ((rays->S + tile_samples(prec) - 1) / tile_samples(prec));
    publish_plan(pl, true, rays->plan_out);
    for (int n = 0; n < nn; ++n) {
        int rc;
        if (is_wide(binds[n].net)) {
            WideBind w;
            rc = wide_bind(binds[n], prec, &w);
            if (rc) return rc;
            if (w.y.C != 3 || w.y.Cout != 1) return fail(NCA_E_UNSUPPORTED, "a ray batch needs nets with 3 input channels and 1 output channel");
            if (n == 0 && nn == 2 && w.y.T > 0) return fail(NCA_E_INVALID, "first net of a composite render must be static (T == 0)");
            rc = wide_forward(w, geom, rays->R * (int64_t)rays->S, outs[n], work, work_bytes, st);
        } else {
            rc = fused_raw_forward(rays, prec, binds[n], outs[n], st);
        }
        if (rc) return rc;
    }
    return nca_composite_fwd(rays->R, rays->S, rays->act, rays->single_field, rays->scale, sig_s, nn == 2 ? sig_d : nullptr, rays->I0, rays->dists, pix, sig_s,
                             nn == 2 ? sig_d : nullptr, (void*)st);
}

// ---- backward of a ray batch.  Workspace: [regions | raw_s, raw_d, g_raw_s, g_raw_d f32[R, S]].  The batch is cut into runs of whole rays; per run every
// general net runs its storing forward (its layers' outputs stay in ITS region, its raw field goes to raw_*), the compositing chain rule turns the run's
// (g_pix, g_sigma) into per-sample raw gradients, and every general net sweeps back from what it stored -- one recompute, not two.  A fused-kernel net of
// the same batch leaves its raw field for ALL rays first and runs its own backward (recompute) from the finished g_raw_* last, in the regions' place.
static int64_t general_bwd_bytes(const NcaRays* rays, const NcaNet* const* nets, int nn, int32_t prec, int64_t max_bytes) {
    const int64_t extra = 4 * align_up(rays->R * (int64_t)rays->S * 4, 256);
    const int64_t budget = max_bytes > extra ? max_bytes - extra : 1;
    const int ts = tile_samples(prec);
    NcaWideLayout lays[2];
    bool wide[2] = {false, false};
    int64_t most = 0;
    for (int n = 0; n < nn; ++n) {
        wide[n] = is_wide(nets[n]);
        if (wide[n]) {
            int rc = wide_layout_of(nets[n], &lays[n], prec);
            if (rc) return rc;
            // (the raw field of the run-up to the backward: wide_forward in the same region)
        } else {
            NcaLayout lay;
            int rc = layout_of(nets[n], &lay, prec);
            if (rc) return rc;
            BwdPlan bp;
            rc = plan_bwd(&lay, 1, prec, rays->R, (rays->S + ts - 1) / ts, budget, &bp);
            if (rc) return rc;
            if (bp.bytes_total > most) most = bp.bytes_total;
        }
    }
    RayChunks ch;
    plan_ray_chunks(lays, wide, nn, rays->R, rays->S, budget, &ch);          // (over budget only at one ray per run: the size it then needs is what is returned)
    if (ch.bytes > most) most = ch.bytes;
    return most + extra;
}

static int render_bwd_general(const NcaRays* rays, int32_t prec, const NetBind* binds, int nn, const double* g_pix, const float* g_sig_s, const float* g_sig_d,
                              float* const* grads, float* g_depth, void* work, int64_t work_bytes, const void* store, int64_t store_bytes, hipStream_t st) {
    if (g_depth) return fail(NCA_E_UNSUPPORTED, "depth gradients need both nets on the fused kernels");
    if (store) {
        // from the general kernels' forward store: per run of whole rays the compositing chain rule on the stored raw fields, then every net's sweep back from its
        // stored activations -- nothing recomputed.  Workspace: per net the scratch half of a backward region (D blocks, split slabs), and g_raw_s, g_raw_d f32[R, S]
        if ((rays->store_format & NCA_STORE_KIND_MASK) != NCA_STORE_GENERAL) return fail(NCA_E_INVALID, "store_format %d is not a store of the general kernels", rays->store_format);
        WideBind wb[2];
        NcaWideLayout lays[2];
        for (int n = 0; n < nn; ++n) {
            if (!is_wide(binds[n].net)) return fail(NCA_E_INVALID, "a store of the general kernels with a fused-kernel net");
            int rc = wide_bind(binds[n], prec, &wb[n]);
            if (rc) return rc;
            lays[n] = wb[n].y;
            HIPCHK(nca_launch_wide_zero(grads[n], wb[n].y.n_params, st));
        }
        GeneralStore gs;
        if (!general_store_plan(lays, nn, rays->R, rays->S, &gs) || store_bytes < gs.bytes)
            return fail(NCA_E_WORKSPACE, "forward store %lld < %lld bytes", (long long)store_bytes, (long long)gs.bytes);
        const int64_t R = rays->R, S = rays->S;
        const int64_t arr = align_up(R * S * 4, 256);
        int64_t scr_off[2], scr_floats = 0;
        for (int n = 0; n < nn; ++n) { scr_off[n] = scr_floats; scr_floats += gs.ch.p[n].bytes / 4 - gs.ch.p[n].off_d; }
        if (!work || work_bytes < scr_floats * 4 + 2 * arr)
            return fail(NCA_E_WORKSPACE, "general kernels: backward workspace %lld < %lld bytes", (long long)work_bytes, (long long)(scr_floats * 4 + 2 * arr));
        float* ws = static_cast<float*>(work);
        char* tailp = static_cast<char*>(work) + (work_bytes - 2 * arr);
        float* graw[2] = {reinterpret_cast<float*>(tailp), reinterpret_cast<float*>(tailp + arr)};
        const float* sb = static_cast<const float*>(store);
        const float* raw[2] = {sb + gs.raw_off, sb + gs.raw_off + R * S};
        int rc = nca_composite_bwd(R, rays->S, rays->act, rays->single_field, rays->scale, raw[0], nn == 2 ? raw[1] : nullptr, rays->dists, g_pix, g_sig_s, g_sig_d,
                                   graw[0], nn == 2 ? graw[1] : nullptr, (void*)st);
        if (rc) return rc;
        int64_t run = 0;
        for (int64_t r0 = 0; r0 < R; r0 += gs.ch.rays, ++run) {
            const int64_t nr = R - r0 < gs.ch.rays ? R - r0 : gs.ch.rays;
            const int64_t n0 = r0 * S, n_valid = nr * S, rows = align_up(n_valid, NCA_WIDE_ROWS);
            const float* blk = sb + run * gs.run_stride;
            for (int n = 0; n < nn; ++n) {
                rc = wide_chunk_backward(wb[n], gs.ch.p[n], blk, ws + scr_off[n], n_valid, rows, graw[n] + n0, grads[n], st);
                if (rc) return rc;
                blk += gs.ch.p[n].off_d;
            }
        }
        return NCA_OK;
    }
    const int64_t R = rays->R;
    const int32_t S = rays->S;
    const int64_t arr = align_up(R * (int64_t)S * 4, 256);
    if (!work || work_bytes < 4 * arr + 256) return fail(NCA_E_WORKSPACE, "backward workspace too small");
    const int64_t region = work_bytes - 4 * arr;
    char* tailp = static_cast<char*>(work) + region;
    float* raw[2] = {reinterpret_cast<float*>(tailp), reinterpret_cast<float*>(tailp + arr)};
    float* graw[2] = {reinterpret_cast<float*>(tailp + 2 * arr), reinterpret_cast<float*>(tailp + 3 * arr)};
    NcaWideGeom geom;
    rays_to_geom(rays, &geom);
    WideBind wb[2];
    NcaWideLayout lays[2];
    bool wide[2] = {false, false};
    for (int n = 0; n < nn; ++n) {
        wide[n] = is_wide(binds[n].net);
        int rc;
        if (wide[n]) {
            rc = wide_bind(binds[n], prec, &wb[n]);
            if (rc) return rc;
            if (wb[n].y.C != 3 || wb[n].y.Cout != 1) return fail(NCA_E_UNSUPPORTED, "a ray batch needs nets with 3 input channels and 1 output channel");
            if (wb[n].y.T > 0 && !rays->phase) return fail(NCA_E_INVALID, "dynamic net needs phase ids");
            lays[n] = wb[n].y;
            HIPCHK(nca_launch_wide_zero(grads[n], wb[n].y.n_params, st));
        } else {
            rc = fused_raw_forward(rays, prec, binds[n], raw[n], st);
            if (rc) return rc;
        }
    }
    RayChunks ch;
    if (plan_ray_chunks(lays, wide, nn, R, S, region, &ch) != NCA_OK)
        return fail(NCA_E_WORKSPACE, "general kernels: backward workspace %lld < %lld bytes", (long long)work_bytes, (long long)(ch.bytes + 4 * arr));
    float* ws = static_cast<float*>(work);
    for (int64_t r0 = 0; r0 < R; r0 += ch.rays) {
        const int64_t nr = R - r0 < ch.rays ? R - r0 : ch.rays;
        const int64_t n0 = r0 * S, n_valid = nr * S, rows = align_up(n_valid, NCA_WIDE_ROWS);
        for (int n = 0; n < nn; ++n) {
            if (!wide[n]) continue;
            int rc = wide_chunk_forward(wb[n], geom, ch.p[n], ws + ch.off[n], n0, n_valid, rows, raw[n] + n0, st);
            if (rc) return rc;
        }
        int rc = nca_composite_bwd(nr, S, rays->act, rays->single_field, rays->scale, raw[0] + n0, nn == 2 ? raw[1] + n0 : nullptr, rays->dists, g_pix + r0,
                                   g_sig_s ? g_sig_s + n0 : nullptr, g_sig_d ? g_sig_d + n0 : nullptr, graw[0] + n0, nn == 2 ? graw[1] + n0 : nullptr, (void*)st);
        if (rc) return rc;
        for (int n = 0; n < nn; ++n) {
            if (!wide[n]) continue;
            rc = wide_chunk_backward(wb[n], ch.p[n], ws + ch.off[n], ws + ch.off[n] + ch.p[n].off_d, n_valid, rows, graw[n] + n0, grads[n], st);
            if (rc) return rc;
        }
    }
    for (int n = 0; n < nn; ++n) {
        if (wide[n]) continue;
        static thread_local NcaFusedArgs one;
        memset(&one, 0, sizeof(one));
        rays_to_args(rays, &one, prec);
        one.nnets = 1;
        int rc = fill_net(binds[n], &one.net[0], prec);
        if (rc) return rc;
        one.g_raw = graw[n];
        NetBind b1[2] = {binds[n], {}};
        float* g1[2] = {grads[n], nullptr};
        rc = run_bwd(one, prec, b1, R, one.nchunk, g1, work, region, st);
        if (rc) return rc;
    }
    return NCA_OK;
}
