/*
 * nerfca_hip.h -- C ABI of libnerfca_hip.so: the MI355X (gfx950) implementation of NeRF-CA's
 * ray-sampling -> (static + dynamic) MLP -> log-space X-ray compositing path.
 *
 * The reference (kirstenmaas/NeRF-CA @ 2024-10-22) is pure Python/PyTorch and has no FFI of its
 * own; every entry point below therefore names the reference *Python* interface it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host";
 *   - buffers are caller-owned, contiguous, 16-byte aligned; the library allocates nothing that
 *     outlives a call except a small pool of timing events (nca_timing_*) and, per calling thread, one side stream with two events
 *     (NCA_OPT_OVERLAP_CUS: created at the first overlapped backward, never otherwise);
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call returns
 *     without synchronising; no exceptions cross the ABI;
 *   - return value 0 = ok, negative = error (NCA_E_*); nca_last_error() gives the message of the
 *     calling thread's last failure.  Unsupported configurations are errors, never fallbacks.
 *
 * Index bookkeeping (bit-exact with the reference): sample n = r*S + s (ray-major,
 * train/model_helpers.py:118-122), sigma outputs are [R,S] row-major.
 */
#ifndef NERFCA_HIP_H
#define NERFCA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCA_ABI_VERSION 13

enum {
    NCA_OK = 0,
    NCA_E_INVALID = -1,     /* bad argument / inconsistent sizes */
    NCA_E_UNSUPPORTED = -2, /* configuration the kernels do not implement */
    NCA_E_HIP = -3,         /* a HIP runtime call failed */
    NCA_E_WORKSPACE = -4    /* workspace too small */
};

/* positional-encoding families of CPPN.pos_enc / Temporal.pos_enc (model/CPPN.py:112-135) */
enum {
    NCA_ENC_NONE = 0,    /* pos_enc == 'none': features = x                                  */
    NCA_ENC_BANDS = 1,   /* any windowed / plain mode: [x, sin(2^k x), sin(2^k x + pi/2)] * w */
    NCA_ENC_FOURIER = 2  /* 'fourier': [sin(2 pi x g), cos(2 pi x g)]                         */
};

/* output activations of get_activation_func (train/model_helpers.py:63-70) */
enum { NCA_ACT_SIGMOID = 0, NCA_ACT_SOFTPLUS = 1, NCA_ACT_CLAMP = 2 };

/* arithmetic of the MLP contractions */
enum {
    NCA_PREC_F32 = 0, /* parity mode, 1e-5 rel vs the reference: f32 operands and f32 accumulation; the hidden-layer contractions run on
                         the bf16 matrix cores from EXACT three-way bf16 splits of both operands (six v_mfma_f32_32x32x16_bf16 per f32
                         product block: the dropped products are below an f32 FMA chain's own rounding), layer 0 and the output layer on
                         v_mfma_f32_32x32x2_f32 */
    NCA_PREC_BF16 = 1 /* bf16 MFMA operands, f32 accumulate: throughput mode                  */
};

/* One coordinate MLP: model/CPPN.py:6-69 (T == 0) or model/Temporal.py:6-93 (T > 0).
 * Parameters live in ONE flat f32 buffer in nn.Module.parameters() order:
 *   [time_latents P*T]  W0[F,K0] b0[F]  {W_i[F,F] b_i[F]} x n_hidden
 *   [Wskip[F,F+K0] bskip[F]  {W[F,F] b[F]} x (n_late-1)]   Wo[1,F] bo[1]
 * with K0 = enc features + T. */
/* Two families of kernels run a net.  The FUSED kernels keep a sample's activations in registers through the whole net: F = 32, 64 or 128, three
 * input channels, one output channel, both precisions -- every net the reference ships.  The GENERAL kernels (ABI 12) run what those cannot hold --
 * F any multiple of 16 up to 1024 (model/CPPN.py:40-65 takes any num_filters), 1..8 input and output channels -- layer by layer with the
 * activations in HBM: f32 only (v_mfma_f32_32x32x2_f32), a forward store only when EVERY net of the batch is theirs (NCA_STORE_GENERAL), no depth gradients, and a workspace for every call
 * (nca_render_fwd_workspace_nets, nca_mlp_fwd_workspace).  A ray batch may mix the two: each net leaves its raw field, one compositing kernel follows.
 * Their packed image (nca_pack_weights) is [fan-in-padded weights | biases | output layer]. */
typedef struct NcaNet {
    int32_t F;        /* num_filters: 32, 64 or 128 (fused kernels); a multiple of 16 in [16, 1024] (general kernels: F > 128, or see `reserved`) */
    int32_t n_hidden; /* num_early_layers (F->F layers after the input layer) */
    int32_t n_late;   /* num_late_layers (CPPN only; skip connection); both precisions since ABI 11 */
    int32_t enc_mode; /* NCA_ENC_*                                            */
    int32_t L;        /* pos_enc_basis                                        */
    int32_t T;        /* num_time_dim; 0 for the static net                   */
    int32_t P;        /* rows of time_latents (10 in the reference)           */
    int32_t reserved; /* 0 = three input channels, one output channel.  ABI 12: bits 0..7 num_input_channels (0 = 3), bits 8..15
                         num_output_channels (0 = 1), bit 16 (NCA_NET_GENERAL) = run on the general kernels whatever the width;
                         anything but 0 selects the general kernels.  Parameter order with C_out outputs: ... Wo[C_out,F] bo[C_out];
                         encoded width K0 = C (none), C (1 + 2 L) (bands), 2 C L (fourier; coefficients f32[C L]) + T */
} NcaNet;
#define NCA_NET_CHANNELS(c_in, c_out) (((c_in) == 3 ? 0 : (c_in)) | (((c_out) == 1 ? 0 : (c_out)) << 8))
#define NCA_NET_GENERAL 0x10000

/* Per-call planner options (NcaRays.plan_opts): a field that is not NCA_OPT_UNSET replaces the process-wide tunable of the same name
 * (nca_set_option) for THIS call only -- two trainers, or two threads, of one process then do not see each other's settings.  A
 * backward should be given the options of its forward (the store's format travels in NcaRays.store_format either way). */
#define NCA_OPT_UNSET INT64_MIN
typedef struct NcaPlanOpts {
    int64_t stage_fp8;                /* NCA_OPT_STAGE_FP8                */
    int64_t stage_fp8_min_tiles;      /* NCA_OPT_STAGE_FP8_MIN_TILES      */
    int64_t resident_min_tiles;       /* NCA_OPT_RESIDENT_MIN_TILES       */
    int64_t wgrad_rebuild_weight_pct; /* NCA_OPT_WGRAD_REBUILD_WEIGHT_PCT */
    int64_t overlap_cus;              /* NCA_OPT_OVERLAP_CUS (ABI 10)     */
    int64_t bf16_store;               /* NCA_OPT_BF16_STORE (ABI 10)      */
} NcaPlanOpts;
#define NCA_PLAN_OPTS_INIT {NCA_OPT_UNSET, NCA_OPT_UNSET, NCA_OPT_UNSET, NCA_OPT_UNSET, NCA_OPT_UNSET, NCA_OPT_UNSET}   /* "every field unset": a zeroed struct is NOT that (0 is a value of every option) */
struct NcaPlan;

/* A batch of rays and the per-step sampling state: the arguments of
 * obtain_train_predictions_iter / _static (train/model_helpers.py:99-160). */
typedef struct NcaRays {
    int64_t R;              /* rays                                                          */
    int32_t S;              /* samples per ray                                               */
    int32_t ray_is_f64;     /* origins/dirs are double (the real script) or float            */
    const void* origins;    /* [R,3]                                                         */
    const void* dirs;       /* [R,3] (not normalised, train/proj_helpers.py:83)              */
    const int32_t* phase;   /* heart phase ids in [0,P); element (r,s) at r*stride_r+s*stride_s */
    int64_t phase_stride_r;
    int64_t phase_stride_s;
    const float* z;         /* jittered depths: [S] (z_stride_r = 0) or [R,S] (fine pass)    */
    int64_t z_stride_r;
    const double* dists;    /* [S] interval lengths incl. the 1e-10 tail (model_helpers.py:73) */
    const float* I0;        /* [R] initial log-intensities                                   */
    int32_t act;            /* NCA_ACT_*                                                     */
    int32_t single_field;   /* 0: composite (sigma scaled);  1: render_volume_density (one net, sigma un-scaled) */
    float scale;            /* scale_value, 1e-2                                             */
    int32_t store_format;   /* backward from a forward store: the value nca_render_fwd returned when it wrote that store
                               (NCA_STORE_*); ignored by the forward and by a backward without a store */
    const NcaPlanOpts* plan_opts; /* HOST pointer or NULL: per-call planner options (above)                                   */
    struct NcaPlan* plan_out;     /* HOST pointer or NULL: filled with what the planner decided in THIS call (the forward fills
                                     the fwd_* fields and wave_tiles, a backward the rest; the other fields are left as they are) --
                                     the per-caller counterpart of the process-wide nca_last_plan() */
} NcaRays;

/* What a storing forward left in its store (the return value of nca_render_fwd; 0 = it wrote no store).  The backward is told
 * through NcaRays.store_format and lays the store out from THAT, not from the process-wide options, which may have changed in
 * between; a value that does not fit the nets of the call is NCA_E_INVALID. */
enum {
    NCA_STORE_NONE = 0,
    NCA_STORE_F32 = 1,        /* f32 mode: every layer input, ReLU masks, raw outputs                         */
    NCA_STORE_RESERVED2 = 2,  /* (ABI <= 8: bf16 mode with bf16 staging -- retired; never returned, refused by the backward)          */
    NCA_STORE_FP8 = 3,        /* bf16 mode: layer inputs as e4m3, masks of all layers, raw outputs               */
    NCA_STORE_BF16 = 4,       /* bf16 mode with NCA_OPT_STAGE_FP8 = 0 (ABI 10): layer inputs as bf16 fragments, masks of all layers, raw
                                 outputs -- nothing in 8 bits, nothing recomputed: the backward writes bf16 output gradients and the
                                 weight gradient contracts bf16 x bf16                                                */
    NCA_STORE_GENERAL = 5,    /* every net of the batch on the general kernels (ABI 12): X0 and every layer's output of every sample, f32, by runs of whole rays, and the
                                 raw fields -- what autograd keeps in the reference; the backward recomputes nothing                                   */
    NCA_STORE_KIND_MASK = 15,
    NCA_STORE_SHARED_ENC = 16 /* flag: both nets share one stored input block (same encoding vectors)          */
};

int nca_abi_version(void);
const char* nca_last_error(void);

/* ---- parameter bookkeeping ------------------------------------------------------------ */

/* Number of f32 parameters of `net` (== sum(p.numel() for p in module.parameters())). */
int64_t nca_param_count(const NcaNet* net);
/* Bytes of the MFMA-ordered weight image produced by nca_pack_weights. */
int64_t nca_packed_bytes(const NcaNet* net, int32_t prec);
/* Re-order the flat natural parameters into the LDS images the kernels stream
 * (run before every forward: optimisers update the parameters in place). */
int nca_pack_weights(const NcaNet* net, const float* params, void* packed, int32_t prec, void* stream);
/* The same for the two nets of a composite render in ONE launch (ABI 11): at the reference's default batch (1 024 rays x 500 samples,
 * train/composite.txt:25,40) a step is ~0.7 ms and every launch of a few microseconds counts. */
int nca_pack_weights2(const NcaNet* net_a, const float* params_a, void* packed_a,
                      const NcaNet* net_b, const float* params_b, void* packed_b, int32_t prec, void* stream);

/* ---- ray path: replaces obtain_train_predictions_iter/_static + get_predictions_* +
 *      render_volume_density[_composite] (train/model_helpers.py:28-160) ------------------ */

/* Forward.  net_d/packed_d/win_d may be NULL when rays->single_field == 1.
 *   pix   f64[R]    = I0 - sum_s (sigma_s + sigma_d) * dists.  NULL (ABI 11; composite or single-field renders of nets of one width): the
 *         forward leaves only the per-tile ray sums in `work` -- f64[R][nchunk], nchunk = ceil(S / 64) in bf16, ceil(S / 32) in f32 -- and
 *         the caller hands them to nca_loss_fwd_bwd (NcaLoss.ray_part), which forms pix itself: one launch less per step.
 *   sig_s f32[R,S], sig_d f32[R,S]  (activation * scale; un-scaled in single_field mode)
 *   work  scratch of nca_render_fwd_workspace() bytes.
 *   store NULL, or a caller-owned buffer of nca_render_store_bytes() bytes: the forward then also leaves there what the
 *         reference's autograd graph keeps (train/run_composite.py:306) -- f32: every layer input, the ReLU masks and the
 *         raw outputs; bf16: the layer inputs as e4m3, the ReLU masks of every layer and the raw outputs (NCA_OPT_STAGE_FP8 = 0:
 *         no store at all) -- and nca_render_bwd given the same buffer does not recompute the layers.
 *         nca_render_store_bytes() returns 0 where this is not available (nets of different width, nets without a hidden
 *         layer, a general-kernel net beside a fused-kernel one): pass NULL there.  Every net on the general kernels (ABI 12): the store holds
 *         X0, every layer's output and ReLU bit masks by runs of whole rays, and the raw fields, f32 (NCA_STORE_GENERAL).
 * Returns a negative error code, or >= 0: the format of the store it wrote (NCA_STORE_*, 0 = none) -- hand it to the backward
 * in NcaRays.store_format. */
int64_t nca_render_fwd_workspace(const NcaRays* rays);
/* The same when a net of the batch runs on the general kernels (ABI 12): a chunk of activations on top ([rows][K0p + 2 F] floats, at most 2^18 rows,
 * fewer under `max_bytes` > 0).  Equal to nca_render_fwd_workspace() for nets of the fused kernels. */
int64_t nca_render_fwd_workspace_nets(const NcaRays* rays, const NcaNet* net_s, const NcaNet* net_d, int32_t prec, int64_t max_bytes);
int64_t nca_render_store_bytes(const NcaRays* rays, const NcaNet* net_s, const NcaNet* net_d, int32_t prec);
int nca_render_fwd(const NcaRays* rays, int32_t prec,
                   const NcaNet* net_s, const void* packed_s, const float* win_s, const float* four_s,
                   const NcaNet* net_d, const void* packed_d, const float* win_d, const float* four_d,
                   const float* latents_d, /* = params_d (time_latents are its first P*T floats) */
                   double* pix, float* sig_s, float* sig_d, void* work, int64_t work_bytes,
                   void* store, int64_t store_bytes, void* stream);

/* Backward: with recompute (store == NULL), or from the store the forward of the SAME rays, weights and windows left
 * (rays->store_format = that forward's return value).
 * Upstream gradients g_pix f64[R], g_sig_s/g_sig_d f32[R,S] (NULL = 0).
 * Writes (overwrites) grads_s / grads_d, flat f32 in the natural parameter order.
 * `params_*` are the natural flat parameters (needed for the latent gradient).
 * max_bytes: the cap the caller can afford.  With a net on the general kernels max_bytes <= 0 is NOT "no cap" but the smallest plan (one ray per run);
 * a backward from the general forward store (NCA_STORE_GENERAL) takes the scratch of all its rays at once and refuses a workspace sized that way
 * with NCA_E_WORKSPACE: pass a real cap (fused.py: at least 1 MiB). */
int64_t nca_render_bwd_workspace(const NcaRays* rays, const NcaNet* net_s, const NcaNet* net_d, int32_t prec,
                                 int64_t max_bytes);
int nca_render_bwd(const NcaRays* rays, int32_t prec,
                   const NcaNet* net_s, const void* packed_s, const float* win_s, const float* four_s, const float* params_s,
                   const NcaNet* net_d, const void* packed_d, const float* win_d, const float* four_d, const float* params_d,
                   const double* g_pix, const float* g_sig_s, const float* g_sig_d,
                   float* grads_s, float* grads_d, void* work, int64_t work_bytes,
                   const void* store, int64_t store_bytes, void* stream);
/* The same, and d loss / d depth of every sample into g_depth f32[R,S] (NULL: as nca_render_bwd).  The reference's fine pass
 * does not detach its sampled depths: the fine losses reach them through the query point, the positional encoding and the
 * first layer -- and the skip layer, where a net has one -- (train/model_helpers.py:146-148), and through them the coarse
 * nets.  Nets of one width. */
int nca_render_bwd_depth(const NcaRays* rays, int32_t prec,
                   const NcaNet* net_s, const void* packed_s, const float* win_s, const float* four_s, const float* params_s,
                   const NcaNet* net_d, const void* packed_d, const float* win_d, const float* four_d, const float* params_d,
                   const double* g_pix, const float* g_sig_s, const float* g_sig_d,
                   float* grads_s, float* grads_d, float* g_depth, void* work, int64_t work_bytes,
                   const void* store, int64_t store_bytes, void* stream);

/* ---- point path: replaces CPPN.forward / Temporal.forward_composite on arbitrary points
 *      (model/CPPN.py:88-110, model/Temporal.py:138-151) ---------------------------------- */
int nca_mlp_fwd(const NcaNet* net, int32_t prec, const void* packed, const float* win, const float* four,
                const float* params, int64_t N, const float* pts /*[N,3]*/, const int32_t* phase /*[N] or NULL*/,
                float* raw /*[N]*/, void* stream);
/* ABI 12: the forward with a workspace -- what a net on the general kernels needs (nca_mlp_fwd refuses it with NCA_E_WORKSPACE); any other net runs as
 * nca_mlp_fwd and nca_mlp_fwd_workspace returns 0.  pts f32[N, C_in], raw f32[N, C_out]; g_raw / grads of nca_mlp_bwd likewise. */
int64_t nca_mlp_fwd_workspace(const NcaNet* net, int32_t prec, int64_t N, int64_t max_bytes);
int nca_mlp_fwd_ws(const NcaNet* net, int32_t prec, const void* packed, const float* win, const float* four,
                   const float* params, int64_t N, const float* pts, const int32_t* phase, float* raw,
                   void* work, int64_t work_bytes, void* stream);
int64_t nca_mlp_bwd_workspace(const NcaNet* net, int32_t prec, int64_t N, int64_t max_bytes);
/* g_latents: NULL, or f32[N, T] (ABI 9): d loss / d latent INPUT of every point -- what autograd hands back through
 * Temporal.query_time's latent vectors (model/Temporal.py:113-136), one row per point whichever points share a table row; `grads`
 * still carries the table-row sums in its first P*T floats. */
int nca_mlp_bwd(const NcaNet* net, int32_t prec, const void* packed, const float* win, const float* four,
                const float* params, int64_t N, const float* pts, const int32_t* phase, const float* g_raw /*[N]*/,
                float* grads, float* g_latents, void* work, int64_t work_bytes, void* stream);

/* ---- stand-alone compositing of raw fields: render_volume_density_composite / render_volume_density
 *      (train/model_helpers.py:72-97), as the reference's evaluation code calls them
 *      (train/run_composite.py:361, 407-413).  raw_* f32[R,S]; `single_field`, `act`, `scale` as in NcaRays. */
int nca_composite_fwd(int64_t R, int32_t S, int32_t act, int32_t single_field, float scale,
                      const float* raw_s, const float* raw_d, const float* I0, const double* dists,
                      double* pix, float* sig_s, float* sig_d, void* stream);
int nca_composite_bwd(int64_t R, int32_t S, int32_t act, int32_t single_field, float scale,
                      const float* raw_s, const float* raw_d, const double* dists,
                      const double* g_pix, const float* g_sig_s, const float* g_sig_d,
                      float* g_raw_s, float* g_raw_d, void* stream);

/* ---- losses: replaces weighted_MSELoss + compute_losses + the loss assembly and their autograd
 *      (train/model_helpers.py:189-262, 284-288; train/run_composite.py:276-292) ------------------ */
typedef struct NcaLoss {
    int64_t R;               /* rays of this batch (this rank's slice under data parallelism)          */
    int32_t S;
    int32_t use_weighting;   /* entro_use_weighting                                                     */
    double skew;             /* skewness_val                                                            */
    double mask_thre;        /* entro_mask_thre                                                         */
    double weighted_thresh;  /* entro_weighted_thresh                                                   */
    double w_favor, w_dent, w_occl, w_l1;  /* this step's weights (linear_param_decay, run_composite.py:276-279) */
    double inv_R;            /* 1 / GLOBAL ray count: mean-type terms are sums over local rays times this */
    const double* weights_dev; /* NULL, or DEVICE f64[4] = {w_favor, w_dent, w_occl, w_l1} read by the kernels instead of
                                  the four fields above: a captured HIP graph can be replayed with new weights          */
    int32_t unit_mse;        /* 1: the pixel term uses unit weights while the regularisers keep `wpix` -- the fine pass's
                                weighted_pixs_ones (train/run_composite.py:296-299)                                      */
    int32_t reserved;
    double* g_dists;         /* NULL, or DEVICE f64[S]: d loss / d dists -- through the ray sums pix = I0 - sum sigma dists (given the
                                pixel term of THIS call) and through every regulariser that contains sigma * dists.  The reference's
                                fine pass differentiates through the interval lengths of ray 0 (train/model_helpers.py:150); needs the
                                three gradient outputs and `dists_work`                                                    */
    double* dists_work;      /* DEVICE f64[R * S] scratch for g_dists (per-ray contributions, summed over rays in a fixed order) */
    const double* term_grads;/* NULL, or DEVICE f64[11] (ABI 10): TERM-GRADIENT MODE -- the backward of compute_losses as an autograd function
                                (train/model_helpers.py:250-262).  Element i is the upstream gradient of the reference's i-th return value
                                [blendw mean, sigma_s max, sigma_d max, favor, s_entropy, s_sum, d_entropy, d_sum, occl, l1, l2] (the maxima are
                                computed under no_grad there: their entries are ignored); g_sig_s / g_sig_d (and g_dists) then are
                                sum_i term_grads[i] d term_i / d sigma -- every term, not only the six the training loss weights.  There is
                                no pixel term in this mode: pix, gt and g_pix may be NULL (weighted_MSELoss is nca_weighted_sq_err);
                                the four weights above and weights_dev are not read                                                          */
    /* ABI 11 -- a zeroed tail keeps ABI 10 behaviour */
    const double* ray_part;  /* NULL, or DEVICE f64[R][ray_nchunk]: the per-tile ray sums a forward called with pix = NULL left in its workspace;
                                the loss kernel then forms pix[r] = I0[r] - sum_c ray_part[r][c] itself (same order as the forward's own kernel:
                                bit-identical) and, if pix_out is given, stores it.  The `pix` argument of nca_loss_fwd_bwd is then ignored  */
    const float* ray_I0;     /* DEVICE f32[R] (with ray_part)                                                                               */
    double* pix_out;         /* NULL or DEVICE f64[R] (with ray_part)                                                                       */
    int32_t ray_nchunk;
    int32_t reserved2;
    float* terms_f32;        /* NULL, or DEVICE f32[NCA_T_COUNT]: the terms once more, rounded to f32 -- what rides behind the flat gradient in a
                                sharded step's ONE all-reduce (train/run_composite.py:310: the early-stop pair is terms 8 and 5)             */
} NcaLoss;
enum { NCA_T_LOSS = 0, NCA_T_PIXEL, NCA_T_BLENDW, NCA_T_SIG_S_MAX, NCA_T_SIG_D_MAX, NCA_T_FAVOR, NCA_T_S_ENTROPY, NCA_T_S_SUM,
       NCA_T_D_ENTROPY, NCA_T_D_SUM, NCA_T_OCCL, NCA_T_L1, NCA_T_L2, NCA_T_COUNT };
int64_t nca_loss_workspace(int64_t R);
/* terms f64[NCA_T_COUNT]; gradients g_pix f64[R], g_sig_s/g_sig_d f32[R,S] (all three NULL = values only; term-gradient mode: g_pix NULL).
 * pix, gt, wpix are f64[R]; sig_s, sig_d f32[R,S]; dists f64[S]. */
int nca_loss_fwd_bwd(const NcaLoss* desc, const double* pix, const double* gt, const double* wpix,
                     const float* sig_s, const float* sig_d, const double* dists,
                     double* terms, double* g_pix, float* g_sig_s, float* g_sig_d,
                     void* work, int64_t work_bytes, void* stream);

/* ---- the static-only loop's loss (ABI 13): weighted_MSELoss + compute_occl_loss + the loss assembly of train/run_nerf.py:227-230 and their
 *      autograd for ONE field, in one pass per ray (StaticTrainer.step_fused / step_graph / evaluate):
 *        pixel = inv_R sum_r wpix[r] (pix[r] - gt[r])^2
 *        occl  = inv_R sum_r sum_s (double)sigma[r,s] dists[s]
 *        loss  = pixel + w_occl occl
 *        g_pix[r] = 2 wpix[r] (pix[r] - gt[r]) inv_R        g_sigma[r,s] = (float)(w_occl inv_R dists[s])
 *      sigma is the UN-scaled density of render_volume_density (train/model_helpers.py:86-97; NcaRays.single_field).  occl_reg_perc does
 *      not appear: compute_occl_loss (train/model_helpers.py:226-248) ORs an all-ones back mask into the front mask unless use_back is
 *      passed and run_nerf.py:228 never passes it, so the term is the mean ray sum whatever the percentage.  Every sum runs in f64 (sigma
 *      f32, dists f64: the reference's dtype promotion), per-block partials and one finishing block in fixed order: results are
 *      bit-identical run to run and with or without the gradient outputs. */
typedef struct NcaStaticLoss {
    int64_t R;               /* rays of this batch (this rank's slice under data parallelism)          */
    int32_t S;
    int32_t reserved;
    double w_occl;           /* run_args.occl_weight_start (train/run_nerf.py:230): constant over a run */
    double inv_R;            /* 1 / GLOBAL ray count                                                    */
    float* terms_f32;        /* NULL, or DEVICE f32[NCA_ST_COUNT]: the terms once more as f32 (they ride behind the flat gradient in an all-reduce) */
    /* optional, zero = unused: pix formed from the forward's per-tile ray sums, exactly as NcaLoss.ray_part / ray_I0 / ray_nchunk / pix_out */
    const double* ray_part;
    const float* ray_I0;
    double* pix_out;
    int32_t ray_nchunk;
    int32_t reserved2;
} NcaStaticLoss;
enum { NCA_ST_LOSS = 0, NCA_ST_PIXEL, NCA_ST_OCCL, NCA_ST_COUNT = 4 };   /* [3] reserved, written 0 */
int64_t nca_static_loss_workspace(int64_t R);
/* terms f64[NCA_ST_COUNT]; g_pix f64[R] and g_sigma f32[R,S] (both NULL = values only); pix, gt, wpix f64[R] (pix is ignored with
 * desc->ray_part); sigma f32[R,S]; dists f64[S]. */
int nca_static_loss_fwd_bwd(const NcaStaticLoss* desc, const double* pix, const double* gt, const double* wpix,
                            const float* sigma, const double* dists,
                            double* terms, double* g_pix, float* g_sigma,
                            void* work, int64_t work_bytes, void* stream);

/* weighted_MSELoss.forward (train/model_helpers.py:284-288): out[r] = (pred[r] - gt[r])^2 * w[r] (the caller takes the mean,
 * train/run_composite.py:287) and its backward; all arrays of one dtype, f64 (is_f64 = 1: what the real script's f64 ray table gives) or
 * f32; g_pred / g_gt / g_w may each be NULL. */
int nca_weighted_sq_err(int64_t R, int32_t is_f64, const void* pred, const void* gt, const void* w, void* out, void* stream);
int nca_weighted_sq_err_bwd(int64_t R, int32_t is_f64, const void* pred, const void* gt, const void* w, const void* g_out,
                            void* g_pred, void* g_gt, void* g_w, void* stream);

/* ---- fine-pass depths: the sampling half of the hierarchical pass of obtain_train_predictions_iter
 *      (train/model_helpers.py:131-148) with sample_pdf (:162-187): weights = |jump of sigma_s + sigma_d| / batch-wide
 *      max, inverse-transform sampling of n_fine depths per ray from the injected uniform draws u[R, n_fine], and
 *      sort(cat[fine, coarse]).  sig_d may be NULL (single field).  z f32[S] is the coarse depth vector shared by
 *      all rays (ascending); z_all f32[R, S + n_fine].  Needs S >= 3. ------------------------------------ */
int64_t nca_fine_depths_workspace(int64_t R);
int nca_fine_depths(int64_t R, int32_t S, int32_t n_fine, const float* sig_s, const float* sig_d, const float* z,
                    const float* u, float* z_all, void* work, int64_t work_bytes, void* stream);
/* Backward of the three calls above (the reference does not detach the sampled depths, train/model_helpers.py:135-146).
 * nca_fine_depths_bwd: g_tot f32[R,S] = d loss / d (sigma_s + sigma_d) through sample_pdf and the sort with the maximum held
 * fixed; gmax_part f32[R] / cnt_part f32[R] = per-ray parts of d loss / d wmax and of the number of jumps that attain wmax.
 * The caller sums both over rays (and ranks) and passes gmax_each = sum(gmax_part) / count to nca_fine_depths_bwd_max, which
 * adds it to the jumps that attain the maximum (torch.max distributes its gradient evenly over ties). */
int nca_fine_depths_bwd(int64_t R, int32_t S, int32_t n_fine, const float* sig_s, const float* sig_d, const float* z,
                        const float* u, const float* wmax, const float* g_z_all, float* g_tot, float* gmax_part, float* cnt_part,
                        void* stream);
int nca_fine_depths_bwd_max(int64_t R, int32_t S, const float* sig_s, const float* sig_d, const float* wmax, const float* gmax_each,
                            float* g_tot, void* stream);
/*      The same in two stages for a batch that is sharded over ranks: the weights are normalised by the maximum over
 *      the WHOLE batch (model_helpers.py:139), so a rank computes the maximum of its rays into the device scalar
 *      wmax f32[1], all-reduces it (MAX) and samples with the result. */
int nca_fine_weight_max(int64_t R, int32_t S, const float* sig_s, const float* sig_d, float* wmax, void* work, int64_t work_bytes,
                        void* stream);
int nca_fine_depths_given_max(int64_t R, int32_t S, int32_t n_fine, const float* sig_s, const float* sig_d, const float* z,
                              const float* u, const float* wmax, float* z_all, void* stream);

/* ---- per-step batch preparation: the ray gather of train/run_composite.py:262-273 (rays_train[ids] split into origins, directions,
 *      pixel values and loss weights; the rays' heart phases) and randomize_depth + the interval lengths of
 *      train/model_helpers.py:3-12, 73-74, in one launch instead of ~20 small torch kernels.  Bit-exact with the torch ops:
 *      z' = lo + (hi - lo) * t with mid = 0.5 * (z[1:] + z[:-1]) in f32; dists[i] = z'[i+1] - z'[i] (f32 subtraction, widened) and the
 *      1e-10 tail in the ray table's dtype.
 *      table f64[N,4,3] (rows: origin, direction, pixel x3, weight x3); phases i64[N]; ids i64[R].
 *      n_rows = N: an id outside [0, N) does not reach memory -- it is clamped into the table and, if `bad_ids` (device i32[1],
 *      caller-zeroed, may be NULL) is given, counted there; the caller reads the counter when it can afford a synchronisation
 *      (CompositeTrainer.early_stop() / evaluate() do, and raise; bench.py checks at the end of every timed record).  With bad_ids = NULL the
 *      clamping is SILENT: the step trains on row 0 or row N - 1 instead of failing as NumPy's IndexError does in the reference -- pass the
 *      counter.  n_rows <= 0 = unknown: ids are trusted as in ABI <= 8.
 *      Outputs: o, d f64[R,3]; gt, w f64[R]; ph i32[R]; z f32[S]; dists f64[S].  depth / t_rand f32[S].  ------------------------------ */
int nca_prepare_batch(int64_t R, int32_t S, const int64_t* ids, const double* table, const int64_t* phases, int64_t n_rows, int32_t* bad_ids,
                      const float* depth, const float* t_rand,
                      double* o, double* d, double* gt, double* w, int32_t* ph, float* z, double* dists, void* stream);

/* ---- per-step batch sampling and schedules ON THE DEVICE (ABI 11): the importance sampling of train/run_composite.py:250-260
 *      (img_sample_size - n_var ids drawn with replacement from the non-variance rays, n_var from the variance rays, shuffled; or
 *      uniform over the table when var_sample_perc == 0), the stratified depth jitter's uniform draw (train/model_helpers.py:8), the
 *      FreeNeRF band windows (model/CPPN.py:144-159) and the four loss weights (linear_param_decay, train/model_helpers.py:264-269;
 *      train/run_composite.py:276-279) as functions of (seed, iteration): counter-based Philox4x32-10 streams (csrc/nca_rng.hpp), so a rank
 *      draws only ITS slots of the global batch and a captured HIP graph replays a whole training run with NO host work per step -- the
 *      iteration is n_iter + *iter_dev (iter_dev: DEVICE i64[1] or NULL).  The reference's own host draws (NumPy's global generator) are not
 *      reproducible by anyone; what is reproduced is their distribution -- exactly n_var variance slots in a uniformly random arrangement,
 *      i.i.d. uniform draws per slot -- and callers that hold the reference's draws inject them (ids_in / t_rand_in).  ------------------ */
typedef struct NcaSampler {
    uint64_t seed;
    int64_t n_iter;             /* iteration = n_iter + (iter_dev ? *iter_dev : 0)                                        */
    const int64_t* iter_dev;
    int64_t R_global;           /* img_sample_size: slots of the GLOBAL batch (the arrangement is drawn over all of them) */
    int64_t n_var;              /* slots that draw from var_ids (int(var_sample_perc / 100 * img_sample_size)); 0: every slot draws from [0, n_rows) */
    const int64_t* var_ids;     /* DEVICE i64[n_var_ids]     (train/data_helpers.py: var_ray_ids)                          */
    int64_t n_var_ids;
    const int64_t* non_var_ids; /* DEVICE i64[n_non_var_ids]                                                              */
    int64_t n_non_var_ids;
    int64_t n_rows;             /* rows of the ray table                                                                  */
} NcaSampler;
/* ids i64[R] = the ray ids of slots slot0 .. slot0 + R - 1 of the global batch */
int nca_draw_ray_ids(const NcaSampler* s, int64_t slot0, int64_t R, int64_t* ids, void* stream);
/* out f32[n]: uniform [0, 1) draws of stream `stream_id` (2 = the depth jitter; >= 16 free for callers) of the sampler's iteration */
int nca_draw_uniform(const NcaSampler* s, int32_t stream_id, int64_t n, float* out, void* stream);

enum { NCA_WINDOW_NONE = 0, NCA_WINDOW_FREE = 1 };
typedef struct NcaWindowSched {
    int32_t kind;               /* NCA_WINDOW_FREE: update_freq_mask_alpha (model/CPPN.py:144-159) -- bands below the moving pointer 1, the band under
                                   it the fractional part, the rest 1e-8, everything 1 from decay_steps on; bit-identical to the host schedule */
    int32_t L;                  /* pos_enc_basis */
    int32_t window_start;       /* pos_enc_window_start */
    int32_t reserved;
    int64_t decay_steps;        /* *_pos_enc_window_decay_steps */
    float* out;                 /* DEVICE f32[L] */
} NcaWindowSched;
typedef struct NcaWeightSched { double start, end; int64_t steps, delay; } NcaWeightSched;   /* linear_param_decay(iter, start, end, steps, delay) */
typedef struct NcaSchedules {
    int32_t n_windows;          /* 0 .. 4 */
    int32_t reserved;
    NcaWindowSched window[4];
    NcaWeightSched weight[4];   /* favor_s, dynamic entropy, occlusion, l1 (train/run_composite.py:276-279) */
    double* weights_out;        /* NULL or DEVICE f64[4]: NcaLoss.weights_dev of the step */
} NcaSchedules;
/* nca_prepare_batch with everything that changes from step to step made on the device, ONE launch: ids (drawn, or ids_in), the gather, the
 * jitter draw (or t_rand_in) with the jittered depths and interval lengths, the band windows and loss weights of the iteration.
 *   ids_in / t_rand_in  NULL = draw; else the caller's i64[R] / f32[S] (parity tests inject the reference's own draws)
 *   ids_out / t_rand_out  NULL, or where the drawn values are also stored
 *   sched  NULL = no schedules; the other arguments as nca_prepare_batch */
int nca_begin_step(const NcaSampler* s, int64_t slot0, int64_t R, int32_t S, const NcaSchedules* sched,
                   const int64_t* ids_in, const float* t_rand_in,
                   const double* table, const int64_t* phases, int32_t* bad_ids, const float* depth,
                   double* o, double* d, double* gt, double* w, int32_t* ph, float* z, double* dists,
                   int64_t* ids_out, float* t_rand_out, void* stream);

/* ---- optimiser: torch.optim.Adam(lr) + LinearLR(start_factor=1, end_factor, total_iters) of
 *      train/run_composite.py:209-215, 307-308, as one launch over up to NCA_ADAM_MAX_SEG flat buffers.
 *      `step` is DEVICE i64[2] (ABI 11; both zero before the first call): step[0] = optimiser steps taken so far -- the kernel uses
 *      t = step[0] + 1 for the bias corrections and lr = cfg.lr * factor(step[0]) (the scheduler is stepped after the optimiser in the
 *      reference), and the LAST workgroup to finish increments it (step[1] counts the finished workgroups of the launch and is zero again
 *      when it ends: one launch instead of an update and a one-thread tick), so a captured graph replays the whole schedule.
 *      NcaAdam.iter_counter (DEVICE i64[1] or NULL) is incremented with it: the training iteration nca_begin_step reads. -------- */
enum { NCA_ADAM_MAX_SEG = 4 };
typedef struct NcaAdam {
    double lr;               /* base learning rate                                              */
    double beta1, beta2, eps;/* torch defaults 0.9, 0.999, 1e-8; no weight decay, no amsgrad    */
    double lr_end_factor;    /* LinearLR end_factor (1.0 = constant lr)                         */
    int64_t lr_total_iters;  /* LinearLR total_iters                                            */
    int64_t* iter_counter;   /* ABI 11: NULL, or DEVICE i64[1] incremented together with step[0]  */
} NcaAdam;
/* n, params, grads, exp_avg, exp_avg_sq: HOST arrays of n_seg entries (device pointers, f32). */
int nca_adam_step(const NcaAdam* cfg, int32_t n_seg, const int64_t* n, float* const* params, const float* const* grads,
                  float* const* exp_avg, float* const* exp_avg_sq, int64_t* step, void* stream);

/* ---- process-wide tunables: A/B switches of the planner, also the hook with which tests force a kernel path at sizes the
 *      oracle can afford.  Both calls return NCA_OK or NCA_E_INVALID; values persist until changed.  A planner decision that
 *      shapes a forward store is taken ONCE, by the forward, and travels to the backward in NcaRays.store_format. -------------- */
enum {
    NCA_OPT_RESERVED0 = 0,        /* (ABI <= 8: NCA_OPT_ONCHIP_MIN_TILES of the retired bf16-staged backward; get / set return NCA_E_INVALID) */
    NCA_OPT_STAGE_FP8 = 1,        /* bf16 mode: whether the forward may leave a STORE for its backward.  The store is 8-bit staged: the layer
                                     inputs and output gradients that only the weight-gradient kernel reads cross HBM as 8-bit floats (inputs
                                     e4m3, gradients e5m2 scaled by a power of two per 64-sample tile; f32 accumulation; the MLP contractions
                                     themselves stay bf16), the store also holds the raw outputs and the masks of every layer, and the backward
                                     recomputes nothing.  1 = always; 0 = never: nca_render_store_bytes returns 0, a forward that is handed a
                                     store leaves it untouched and returns NCA_STORE_NONE, and the backward recomputes the layers -- bf16
                                     operands everywhere, nothing in 8 bits (BASELINE configs[1] "as written"; the bf16-STAGED store of
                                     ABI <= 8 was retired in round 4: never better in held-out PSNR, 1.75 x slower);
                                     -1 = by batch size: a store when the batch has at least NCA_OPT_STAGE_FP8_MIN_TILES wave tiles.  The
                                     default is -1 with a threshold of 0, i.e. the store is UNCONDITIONAL unless the caller sets one of the
                                     two.  nca_last_plan().stage_fp8 says what ran.  Initial value from NCA_STAGE_FP8 (0 / 1) */
    NCA_OPT_RESIDENT_MIN_TILES = 2, /* bf16 mode: run the fused kernels with ONE net per launch and all of that net's weight images
                                     resident in LDS (no per-layer weight DMA, no workgroup barrier in the tile loop) when the images fit
                                     (width 128: the input layer + 4 hidden layers forward, 4 transposed images backward) and the batch has at least this many 64-sample wave
                                     tiles.  A two-net render then takes two forward launches (the second composites with the first
                                     one's sigma).  0 = always, -1 = never; default 8 * 8 waves * CUs (NCA_RESIDENT=0 -> never,
                                     =force -> always).  Results are bit-identical to the streaming kernels */
    NCA_OPT_STAGE_FP8_MIN_TILES = 3, /* threshold of NCA_OPT_STAGE_FP8 = -1, in 64-sample wave tiles of the whole batch (>= 0; default 0 = always) */
    NCA_OPT_WGRAD_REBUILD_WEIGHT_PCT = 4, /* fp8 staging: the weight-gradient launch is ONE round of one-wave jobs, so its slowest wave is
                                     the launch; the jobs that rebuild their output-gradient block from mask bits take more cycles per
                                     tile than the others and get this many percent of the others' sample splits (100 .. 200; default
                                     115 = the cycle ratio measured on MI355X with round 3's clock-probe build, tools/r03_experiments.sh; initial value from NCA_WGRAD_W).
                                     A constant rather than a calibration at first use: the splits fix the summation order, and with it
                                     the bits of the gradient -- tools/calibrate_wgrad.py times the candidates on a given box */
    NCA_OPT_OVERLAP_CUS = 5,      /* bf16 mode, backward from the 8-bit staged store of a two-net ray batch with resident weight images (the bench path):
                                     the static net's weight-gradient launch (HBM-bound) runs BESIDE the dynamic net's dgrad launch (issue-bound) on
                                     a second stream of the library -- fork and join are events on the caller's stream, so a stream capture records
                                     both branches.  The value is the number of compute units whose wave slots the overlapped weight-gradient launch
                                     is sized for (its one-round grid); the dgrad launch beside it gets the others.  A compute unit holds a workgroup
                                     of EITHER kernel (both take more than half of its LDS), so the two grids add up to the chip whichever is
                                     dispatched first.  The dynamic net's weight gradient follows the join on the whole chip.  0 = off: one
                                     weight-gradient launch for both nets after both dgrad launches (ABI <= 9).  The value fixes the split of the
                                     sample sums, hence the bits of the gradient (run to run they are identical either way).  Initial value from
                                     NCA_OVERLAP_CUS; nca_last_plan().overlap_cus says what ran */
    NCA_OPT_BF16_STORE = 6,       /* bf16 mode, batches for which the 8-bit staged store is off (NCA_OPT_STAGE_FP8 = 0, or below its threshold): 1 (default) =
                                     the forward may still leave a store, with the layer inputs as BF16 fragments (NCA_STORE_BF16; masks of every layer
                                     and raw outputs as in the 8-bit store) -- the backward then recomputes nothing (mode 5), writes bf16 output
                                     gradients and the weight gradient contracts bf16 x bf16: BASELINE configs[1] "as written", nothing in 8 bits;
                                     0 = no store, the backward recomputes the layers (mode 1; also what runs when the caller passes no store).
                                     Initial value from NCA_BF16_STORE */
    NCA_OPT_COUNT
};
int nca_get_option(int32_t opt, int64_t* value);
int nca_set_option(int32_t opt, int64_t value);

/* What the planner decided in the process's last nca_render_fwd and last nca_render_bwd[_depth] / nca_mlp_bwd (bench.py labels
 * its line with it; tests assert the path they mean to exercise).  Process-wide, not per thread: a PyTorch backward runs on the
 * autograd engine's thread. */
typedef struct NcaPlan {
    int32_t fwd_store_format;     /* NCA_STORE_* | flags of the last forward (0: no store)                              */
    int32_t fwd_launches;         /* fused launches of that forward (2: one per net, weight images resident in LDS)     */
    int32_t fwd_resident;         /* 1: resident weight images                                                          */
    int32_t bwd_kernel_mode;      /* 1 recompute, 3 from the f32 store, 5 from the bf16 mode's 8-bit staged store (nothing recomputed) */
    int32_t bwd_resident;
    int32_t bwd_launches_per_chunk; /* fused dgrad launches per ray chunk                                              */
    int32_t bwd_onchip;           /* always 0 (ABI <= 8: the retired bf16-staged backward's on-chip layer)              */
    int32_t stage_fp8;            /* that backward staged 8-bit blocks                                                  */
    int32_t wgrad_jobs, wgrad_splits, wgrad_splits_rebuild;
    int32_t chunks;               /* ray chunks of that backward                                                        */
    int64_t wave_tiles;           /* wave tiles of the whole batch of the last call                                     */
    int32_t overlap_cus;          /* NCA_OPT_OVERLAP_CUS as that backward ran it (0: one weight-gradient launch for both nets)   */
    int32_t overlap_forked;       /* 1: the overlapped launch went to the library's second stream; 0: the same launches in a row on the caller's
                                     (the second stream did not exist yet and the caller's stream was capturing)                  */
    int64_t reserved[3];
} NcaPlan;
int nca_last_plan(NcaPlan* out);
/* Static description of the build: target, ABI, and the timing-experiment mask the kernels were compiled with ("NCA_EXP=0" in
 * every shipped library; the timing-only builds of rounds 2 - 3, whose results are wrong by construction, come from the tag r03-kernels: tools/r03_experiments.sh). */
const char* nca_build_info(void);

/* ---- in-library kernel timing (HIP events on the launch stream), used by bench.py -------- */
enum { NCA_K_PACK = 0, NCA_K_FWD = 1, NCA_K_BWD_DGRAD = 2, NCA_K_BWD_WGRAD = 3, NCA_K_BWD_REDUCE = 4, NCA_K_LOSS = 5, NCA_K_ADAM = 6, NCA_K_COUNT = 7 };
int nca_timing_enable(int32_t on);
/* Synchronises the recorded events and returns accumulated milliseconds and launch count. */
int nca_timing_read(int32_t kind, double* total_ms, int64_t* launches);
int nca_timing_reset(void);

/* ---- view rendering: forward-only inference (export.render_view / render_sequence) --------
 * Rays of ANY C-arm view generated on the device, the composition of two single-field renders into the composite / static / dynamic
 * images of the reference's display block (train/run_composite.py:361, 405-413), and the per-image min / max normalisation it applies
 * before logging.  The static field goes through the render forward above in single-field mode, once per view.  The dynamic field, once per
 * (view, phase), does not (the render forward binds time latents to its second net only): it is the point forward on the chunk's query points,
 * made by the query-point entry below, and the stand-alone compositing kernel in single-field mode.  Purely additive to ABI 13.  These entry points keep their OWN per-thread message: a negative return
 * value is explained by the view-side accessor declared below, not by the library-wide one.  A refused call launches nothing. */

/* One projection.  All f32: that is where train/proj_helpers.py:65-90 (get_ray_values_tigre) rounds. */
typedef struct NcaView {
    float pose[12];            /* rows of the 3x4 [R | t] of source_matrix_tigre([0,0,-DSO], theta, phi, larm), cast to f32 */
    int32_t W, H;              /* nDetector */
    float d_det[2], off_det[2], dsd;
} NcaView;

/* Origins and directions [n,3] of the pixels p = w*H + h in [p0, p0+n) (the order of the reference's flattened [W,H] images):
 * u = (w + .5 - W/2) d_det[0] + off_det[0], v likewise from h, dir = R [u/dsd, v/dsd, 1] (not normalised), origin = t; every operation
 * a rounded f32 one in the host function's order.  out_f64 = 1 writes the same f32 values widened to f64 (the ray table's type, for an
 * f64 pix).  `view` is a host pointer.  NCA_E_INVALID: W or H <= 0, n <= 0, p0 < 0, p0 + n > W*H, a NULL pointer. */
int nca_view_rays(const NcaView* view, int64_t p0, int64_t n, int32_t out_f64, void* origins, void* dirs, void* stream);

/* Query points of a ray chunk: pts f32[R][S][3] = f32(o[r] + d[r] z[s]) as the fused render kernels form them from f64 rays [R,3] (summed
 * in f64, rounded once); z is ONE depth vector f32[S].  The render forward binds time latents to its second
 * net only, so a dynamic net alone cannot run there: it is evaluated on these points through the point forward, once per phase, and the
 * stand-alone compositing kernel in single-field mode turns the raw field into its image.  NCA_E_INVALID: R or S <= 0, a NULL pointer. */
int nca_view_points(int64_t R, int32_t S, const double* origins, const double* dirs, const float* z, float* pts, void* stream);

/* pix_s, pix_d: the two single-field images [n] (f64 when pix_is_f64, else f32), each already I0 - sum(sigma dists scale).
 * pred = f32((pix_s + pix_d) - i0), in f64 in exactly that order; pred_s = f32(pix_s); pred_d = f32(pix_d).
 * pix_d == NULL (a static-only model): pred = pred_s and pred_d is filled with f32(i0). */
int nca_view_compose(int64_t n, double i0, const void* pix_s, const void* pix_d, int32_t pix_is_f64, float* pred, float* pred_s,
                     float* pred_d, void* stream);

/* img [n_img][n] -> minmax [n_img][2] = (min, max) of each image and, when out != NULL, out [n_img][n] = (x - min) / (max - min) in f32
 * (trainer.normalize_image; run_composite.py:405-413).  The one deliberate difference from that expression: a constant image
 * (max == min) gives zeros, not NaN.  A NaN pixel makes min, max and the scaled image NaN, as torch.min / torch.max do there.  No atomics: per-block partials in `work`, one block per image folds them in a fixed order, then
 * the scaling pass -- bit-identical run to run.  The workspace query returns the bytes ONE image of n pixels needs (a positive multiple of
 * 256, non-decreasing in n; NCA_E_INVALID for n <= 0); a call needs n_img times that, else NCA_E_WORKSPACE. */
int64_t nca_image_normalize_workspace(int64_t n);
int nca_image_normalize(int32_t n_img, int64_t n, const float* img, float* out, float* minmax, void* work, int64_t work_bytes, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_view_last_error(void);

/* ---- drr: cone-beam projection of voxel volumes and its adjoint (drr.project_rays / project_sequence / volume_teacher / fit_volumes) --------
 * Line integrals of trilinearly interpolated voxel grids along the rays nca_view_rays writes, by the renderer's quadrature:
 * pix = i0 - sum_s value(o + d z_s) dists_s.  Purely additive to ABI 13.  Like the view section, these entry points keep their OWN
 * per-thread message (the accessor below); a refused call launches nothing and reads no pointer; a launch failure is reported once. */

/* A regular grid of nodes, export.density_volume's linspace(lo, hi, n) on each axis. */
typedef struct NcaGrid {          /* 64 bytes, no implicit padding */
    double lo[3];                 /* position of node 0 on each axis */
    double inv[3];                /* (n-1)/(hi-lo): nodes per unit length, computed by the host in f64 */
    int32_t n[3];                 /* nodes per axis, each >= 2; vol is [n0][n1][n2], last axis fastest */
    int32_t reserved;             /* 0 */
} NcaGrid;

/* vol f32 [n_vol][n0][n1][n2] contiguous, rays f64 [R,3] (nca_view_rays with out_f64 = 1), z f32 [S], dists f64 [S] -> pix f64 [n_vol][R].
 * One sample, every operation a rounded f64 one in this order (no contraction): p_a = o_a + d_a (double)z_s; g_a = (p_a - lo_a) inv_a;
 * i_a = floor(g_a); f_a = g_a - i_a; the eight neighbours (i_a, i_a + 1), one with any index outside [0, n_a - 1] reading as 0, are
 * interpolated as (1 - f) v0 + f v1 along the last axis first, then the middle one, then the first; term = value dists_s.  This is
 * grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) with the coordinate triple reversed.  A sample with a g_a outside
 * (-1, n_a) contributes exactly 0 and loads nothing.  All n_vol volumes are marched in one pass: a sample's indices and weights are computed
 * once per group of up to 8 volumes; each volume's sum is formed in the same order whatever the grouping, so the result does not depend
 * on n_vol, on how a ray set is split into calls, or on the run.  No atomics.  `grid` is a host pointer.
 * NCA_E_INVALID (the message names the value): a NULL pointer; n_vol, R or S <= 0; an n_a < 2; reserved != 0; a non-finite lo or inv;
 * inv_a <= 0; a voxel count that overflows int64. */
int nca_drr_project(const NcaGrid* grid, const float* vol, int32_t n_vol, int64_t R, int32_t S, const double* origins, const double* dirs,
                    const float* z, const double* dists, double i0, double* pix, void* stream);

/* Threads that share one ray (process-wide): 1 = one thread marches all S samples in order; 4 = part j of four takes the samples
 * s = j, j + 4, ... (the four parts of a ray in four waves of one block) and the four sub-sums are folded in part order.  Both are
 * deterministic; they differ from each other in the last bits (the order of the sum).  The default is the faster of the two as measured by
 * tools/drr_bench.py; the other stays for that tool.  set: NCA_E_INVALID for any other value. */
int nca_drr_set_split(int32_t split);
int nca_drr_get_split(void);

/* The adjoint of nca_drr_project in the volumes: g_pix f64 [n_vol][R] (the gradient of a scalar in pix) -> ADDED INTO g_vol f64
 * [n_vol][n0*n1*n2] (the caller zeroes it); rays, z, dists and `grid` as above.  For sample (ray, s), g_a, i_a, f_a and m_a = 1 - f_a are
 * exactly those of nca_drr_project: the same rounded f64 operations, the same skip test g_a in (-1, n_a), never a clamp.  For each of the
 * eight neighbours (a, b, c) in {0,1}^3 whose node (i_0 + a, i_1 + b, i_2 + c) is inside the grid and for each volume v:
 *     w_abc = (x0 x1) x2, where x_k is f_k when the offset on axis k is 1 and m_k when it is 0;
 *     contrib = (-(g_pix[v][ray] dists_s)) w_abc;          g_vol[v][node] += contrib,
 * every product a rounded f64 product in that order.  Neighbours outside the grid contribute nothing and are never addressed; i0 does not
 * enter.  Only the order of a node's sum is undefined: the adds are f64 atomics (one hardware add each, no compare-and-swap loop), so the
 * last bits can differ from run to run.  A sample's indices and weights are computed once per group of up to 8 volumes.  No
 * synchronisation beyond the stream's order: a later kernel on `stream` reads the finished sums.
 * NCA_E_INVALID (the message names the value): the refusals of nca_drr_project, with g_pix and g_vol for vol and pix; an S within 4 of
 * INT32_MAX. */
int nca_drr_backproject(const NcaGrid* grid, int32_t n_vol, int64_t R, int32_t S, const double* origins, const double* dirs, const float* z,
                        const double* dists, const double* g_pix, double* g_vol, void* stream);

/* How nca_drr_backproject adds (process-wide): 0 = one atomic per (sample, neighbour, volume); 1 = a thread sums the contributions of
 * consecutive samples of its ray that stay in one cell in registers and adds them when the cell changes.  They differ in the order of a
 * node's sum only.  The default is the faster of the two as measured by tools/drr_grad_bench.py; the other stays for that tool.
 * set: NCA_E_INVALID for any other value. */
int nca_drr_set_backproject_runs(int32_t runs);
int nca_drr_get_backproject_runs(void);

/* The message of the calling thread's last failed call of this section. */
const char* nca_drr_last_error(void);

/* ---- vol: smoothed total variation of voxel volumes in space and along the heart phase (drr.total_variation / fit_volumes) ---------------
 * The priors of the voxel reconstruction.  Purely additive to ABI 13.  Like the view and drr sections, these entry points keep their OWN
 * per-thread message (the accessor below); a refused call launches nothing and reads no pointer; a launch failure is reported once.
 *
 * vol f32 [n_vol][n0][n1][n2] contiguous on one NcaGrid (lo is validated but unused), each value widened to f64; eps_s, eps_t > 0.  Every
 * operation below is ONE rounded f64 operation in the order written (no contraction).
 * Space, per volume and node i = (i0, i1, i2):
 *     d_a(i) = (x[i + e_a] - x[i]) inv[a] for i_a < n_a - 1, 0 at the last node of axis a (forward differences, no wrap-around);
 *     m(i) = sqrt(eps_s eps_s + ((d_0 d_0 + d_1 d_1) + d_2 d_2));   term(i) = m(i) - eps_s;   space = sum over volumes and nodes;
 *     own = -((d_0(i) inv[0] + d_1(i) inv[1]) + d_2(i) inv[2]) / m(i);   back_a = (d_a(i - e_a) inv[a]) / m(i - e_a) for i_a > 0, else 0;
 *     g_s(i) = ((own + back_0) + back_1) + back_2.
 * Heart phase: the n_vol volumes of one call are one stack.  Pairs (p, p + 1), p = 0 .. n_vol - 2; with cyclic != 0 and n_vol >= 2 also
 * (n_vol - 1, 0) (n_vol == 2 then carries its pair twice); n_vol == 1 has none.  Per pair and node:
 *     t = x[p+1][i] - x[p][i];   mt = sqrt(eps_t eps_t + t t);   term = mt - eps_t;   time = sum over pairs and nodes;
 *     g_t of x[p][i] = (-(t_p / mt_p)) + (t_{p-1} / mt_{p-1}), a pair that does not exist contributing 0.
 * A flat stack has space = time = 0 exactly and a zero gradient.
 * NCA_E_INVALID (the message names the value): a NULL pointer; n_vol <= 0; cyclic not 0 / 1; an eps that is not finite and positive; the
 * grid refusals of nca_drr_project; more tiles (of 4 x 8 x 64 nodes) than one launch covers. */

/* out f64 [2] on the device, ADDED INTO: out[0] += space, out[1] += time.  Only the order of the two sums is free: f64 block sums, then one
 * f64 atomic add per block and term, so the last bits of the two values can differ from run to run. */
int nca_vol_tv(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, double* out, void* stream);

/* g_vol f32 [n_vol][n0*n1*n2], WRITTEN: g_vol[v][i] = (float)(scale[0] g_s + scale[1] g_t), two rounded f64 products, one rounded f64 sum,
 * one rounding to f32.  scale is f64 [2] ON THE DEVICE (a backward pass hands over its upstream gradients without a read-back).  Gathered:
 * every node is written once by one thread, no atomics, the same bits on every run. */
int nca_vol_tv_grad(const NcaGrid* grid, const float* vol, int32_t n_vol, double eps_s, double eps_t, int32_t cyclic, const double* scale,
                    float* g_vol, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_vol_last_error(void);

/* ---- phantom: a procedural 4-D phantom rasterised into voxel grids (phantom.voxelize / make_phantom) -----------------------------------------
 * Soft ellipsoids (a static thorax, additive) and tapered capsules (vessels, a maximum) per heart phase -> out f32 [n_phase][n0][n1][n2] on
 * one NcaGrid, the grids nca_drr_project, nca_vol_tv and export take.  Purely additive to ABI 13.  Like the view, drr and vol sections,
 * these entry points keep their OWN per-thread message (the accessor below); a refused call launches nothing and reads no pointer; a launch
 * failure is reported once.
 *
 * Every operation below is ONE rounded f64 operation in the order written (no contraction).
 * Node i = (i_0, i_1, i_2):   h_a = 1 / inv_a, formed once per axis;   x_a = lo_a + (double)i_a h_a.
 * Ellipsoid row f64 [14] = centre c[3], matrix A[9] (row-major), soft width w > 0, density rho:
 *     u = x - c;   q_k = (A_k0 u_0 + A_k1 u_1) + A_k2 u_2;   r = sqrt((q_0 q_0 + q_1 q_1) + q_2 q_2);
 *     cov = min(max(0.5 + (1 - r) / w, 0), 1);   background = ((0 + rho_0 cov_0) + rho_1 cov_1) + ... in row order (additive: a lung is a
 *     negative rho).
 * Segment row f64 [8] = endpoints a[3], b[3], radii ra, rb >= 0 (a tapered capsule); edge > 0 is one length for the call:
 *     e = b - a;   ee = (e_0 e_0 + e_1 e_1) + e_2 e_2;   q = x - a;   qe = (q_0 e_0 + q_1 e_1) + q_2 e_2;
 *     t = min(max(qe / ee, 0), 1), and t = 0 when ee == 0 (a sphere);   c_k = q_k - t e_k;   d = sqrt((c_0 c_0 + c_1 c_1) + c_2 c_2);
 *     r = ra + t (rb - ra);   cov = min(max(0.5 + (r - d) / edge, 0), 1);   vessels = rho_v max_n cov_n, the maximum starting from 0.
 *     A maximum, not a sum: consecutive segments of a polyline and branch junctions do not double-count, and the order of the rows cannot
 *     change a bit.
 * out[p][i] = (float)(background_p(i) + vessels_p(i)).  Both tables are per phase, on the device: ell f64 [n_phase][n_ell][14] and seg f64
 * [n_phase][n_seg][8]; either count may be 0, not both.  What the tables hold is the caller's responsibility (phantom.voxelize checks it).
 * Every node of every phase is written exactly once by one thread: no atomics, the same bits on every run.  Segments are staged through LDS
 * in batches of NCA_PHANTOM_SEG_BATCH.  `grid` is a host pointer.
 * NCA_E_INVALID (the message names the value): a NULL grid or out; n_phase <= 0; a negative count, or both counts 0; a NULL table whose
 * count is positive; edge not finite and positive; rho_v not finite; the grid refusals of nca_drr_project; more tiles (of 4 x 8 x 64 nodes,
 * times n_phase) than one launch covers. */
enum { NCA_PHANTOM_SEG_BATCH = 512 };
int nca_phantom_voxelize(const NcaGrid* grid, int32_t n_phase, int32_t n_ell, const double* ell, int32_t n_seg, const double* seg,
                         double rho_v, double edge, float* out, void* stream);

/* Culling (process-wide): 1 = a staged segment whose box (its endpoints' box grown by max(ra, rb) + edge / 2, padded by a relative 2^-20)
 * misses the tile's box is dropped before any node of the tile evaluates it; 0 = every node evaluates every segment.  cov is exactly 0 at
 * every node that far from a segment, so both give the same bits.  The default is the faster of the two as measured by
 * tools/phantom_bench.py; the other stays for that tool and the tests.  set: NCA_E_INVALID for any other value. */
int nca_phantom_set_cull(int32_t on);
int nca_phantom_get_cull(void);

/* The message of the calling thread's last failed call of this section. */
const char* nca_phantom_last_error(void);

/* ---- ssim: structural similarity of image stacks and its gradient (metrics.ssim / compare_sequences, ssim_weight of drr.fit_volumes) --------
 * The SSIM of Wang et al. of N image pairs with a separable window, in f64, and the gradient of its sum in the prediction.  Purely additive
 * to ABI 13.  Like the view, drr, vol and phantom sections, these entry points keep their OWN per-thread message (the accessor below); a
 * refused call launches nothing and reads no device pointer; a launch failure is reported once.
 *
 * x (prediction), y (truth): f32 [N][H][W] contiguous on the device.  range: f64 [N] ON THE DEVICE.  win: HOST f64 [K], K odd,
 * 1 <= K <= NCA_SSIM_MAX_WIN, H >= K, W >= K: any weights (the library never calls exp; metrics.gaussian_window makes Wang's window and
 * hands its bits over).  k1, k2 finite and positive.  Every operation below is ONE rounded f64 operation in the order written (the
 * kernels spell each one out: nothing leans on a contraction flag).
 * Per image n:   L = range[n];   C1 = (k1 L)(k1 L);   C2 = (k2 L)(k2 L).  An L that is not finite and positive gives NaN at every position
 *     of that image (value, map and gradient); it is not checked on the host.
 * Per pixel, five fields widened to f64: x, y, xx = x x, yy = y y, xy = x y (products of two f32 values: exact in f64).
 * Statistics at the Hv x Wv = (H - K + 1) x (W - K + 1) window positions (i, j), separable, no padding, for each field v:
 *     r_v(i, j) = (..((win[0] v(i, j)) + win[1] v(i, j + 1)) + ..) + win[K-1] v(i, j + K - 1)          rows i = 0 .. H - 1
 *     m_v(i, j) = (..((win[0] r_v(i, j)) + win[1] r_v(i + 1, j)) + ..) + win[K-1] r_v(i + K - 1, j)
 *     mx = m_x, my = m_y;   sxx = m_xx - mx mx;   syy = m_yy - my my;   sxy = m_xy - mx my;
 *     a1 = 2 (mx my) + C1;   a2 = 2 sxy + C2;   b1 = (mx mx + my my) + C1;   b2 = (sxx + syy) + C2;   D = b1 b2;   S = (a1 a2) / D.
 * x == y makes a1 == b1 and a2 == b2 bit for bit: S is exactly 1.
 * Gradient of sum_p S_p in x (the window moments as variables: d mx = w dx, d m_xx = 2 w x dx, d m_xy = w y dx), per position:
 *     P = ((2 my) (a2 - a1)) / D + (((2 mx) S) (b1 - b2)) / D;   Q = -((2 S) / b2);   R = (2 a1) / D;
 * per pixel (i, j) of the H x W image, with F[M](i, j) = sum_{a,b} win[a] win[b] M(i - a, j - b) formed separably:
 *     f_M(i', j) = sum over b = 0 .. K - 1, increasing, of win[b] M(i', j - b), only the terms with 0 <= j - b < Wv: the first of them
 *                  starts the sum, the others are added in turn (a term outside is SKIPPED, not added as a zero);   rows i' = 0 .. Hv - 1
 *     F[M](i, j) = sum over a = 0 .. K - 1, increasing, of win[a] f_M(i - a, j), only the terms with 0 <= i - a < Hv, in the same way
 *                  (every pixel has at least one term in each pass);
 *     g(i, j) = (float)(scale[n] ((F[P] + x F[Q]) + y F[R])),   x and y the pixel's own values widened.
 * (tests/test_ssim_cpu.py holds these formulas to torch autograd of the conv2d expression in f64: nothing had to be corrected.)
 * NCA_E_INVALID (the message names the value): a NULL pointer (map may be NULL); N, H or W <= 0; K even or outside [1, NCA_SSIM_MAX_WIN];
 * H < K or W < K; a window entry that is not finite; a k that is not finite and positive; N H W beyond what int64 byte offsets carry; more
 * than 2^24 tiles (of 16 x 32 pixels, all images together: 2^32 threads, what one launch covers).  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer. */
enum { NCA_SSIM_MAX_WIN = 11 };

/* sum f64 [N] on the device, ADDED INTO: sum[n] += sum over the Hv Wv positions of S.  Only the order of the sum is free: f64 block sums,
 * then one f64 atomic add per block, so the last bits can differ from run to run.  map, when not NULL: f32 [N][Hv][Wv], WRITTEN,
 * map = (float)S, every position once. */
int nca_ssim(int32_t N, int32_t H, int32_t W, const float* x, const float* y, const double* range, int32_t K, const double* win, double k1,
             double k2, double* sum, float* map, void* stream);

/* The gradient runs as two kernels: the first writes P, Q, R as three f64 maps [3][N][Hv][Wv] into `work`, the second gathers them.  The
 * query returns those bytes (24 N Hv Wv), and 0 for sizes the entry point refuses. */
size_t nca_ssim_grad_workspace(int32_t N, int32_t H, int32_t W, int32_t K);

/* g_x f32 [N][H][W], WRITTEN: every pixel once by one thread.  Gathered, no atomics, the same bits on every run.  scale is f64 [N] ON THE
 * DEVICE (a backward pass hands over its upstream gradients without a read-back). */
int nca_ssim_grad(int32_t N, int32_t H, int32_t W, const float* x, const float* y, const double* range, int32_t K, const double* win, double k1,
                  double k2, const double* scale, float* g_x, void* work, size_t work_bytes, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_ssim_last_error(void);

/* ---- edt: the exact Euclidean distance transform of thresholded voxel stacks (metrics.distance_transform / mask_distances /
 *      centreline_coverage) -----------------------------------------------------------------------------------------------------------------
 * The distance, in world units, from every node of a voxel grid to the nearest node whose value is above (or, inverted, not above) a
 * threshold.  Purely additive to ABI 13.  Like the view, drr, vol, phantom and ssim sections, these entry points keep their OWN per-thread
 * message (the accessor below); a refused call launches nothing and reads no device pointer; a launch failure is reported once.
 *
 * vol f32 [n_vol][n0][n1][n2] contiguous on one NcaGrid (lo is validated but unused).  `grid` is a host pointer.  Every operation below is
 * ONE rounded f64 operation in the order written (the kernels spell each one out: nothing leans on a contraction flag).
 *     h_a = 1 / inv_a;   w_a = h_a h_a, formed once per axis on the host in f64.
 * Node j of volume v is a FEATURE iff ((double)vol[v][j] > threshold) != (invert != 0).  A NaN value is not > threshold: it is a feature
 * only under invert.  A value equal to the threshold is not > threshold.
 * For node i and feature j of the same volume, with the integer offsets d_a = i_a - j_a, their squares formed in int64 and converted
 * exactly:
 *     q(i, j) = w_0 (double)(d_0 d_0) + (w_1 (double)(d_1 d_1) + w_2 (double)(d_2 d_2));
 *     out[v][i] = (float)sqrt(min over the features j of volume v of q(i, j)).
 * A volume without a feature gives +inf at every node; a feature node gets exactly 0.  Every node of every volume is written exactly once
 * by one thread: no atomics, the same bits on every run, and the result of a volume does not depend on n_vol or on its neighbours in the
 * stack.
 * The minimum over all features is the definition; the kernels form it separably -- g = the integer distance to the nearest feature of
 * the row (axis 2), b = min_j1 (w_1 d_1^2 + w_2 g^2), out = sqrt(min_j0 (w_0 d_0^2 + b)) -- which gives the same bits: rounding is monotone
 * and every term is non-negative, so the minimum of the rounded sums is the rounded sum with the minimum (tests/test_edt_cpu.py holds the two
 * forms to each other bit for bit).  For the same reason a search outward from the node's own index stops at the first w_a d_a^2 that is
 * not below the best value so far.
 * The workspace holds b as f64 and g as int32 for every node: 12 bytes per node, rounded up to a multiple of 256.  The query returns it, and
 * 0 for arguments the entry point refuses.
 * NCA_E_INVALID (the message names the value): a NULL grid, vol or out; n_vol <= 0; invert not 0 / 1; a threshold that is NaN; the grid
 * refusals of nca_drr_project; more than 2^24 workgroups in one of the three launches (rows / 4, or tiles of 16 lines: 2^32 threads, what
 * one launch covers).  NCA_E_UNSUPPORTED: an axis longer than NCA_EDT_MAX_AXIS (a line tile of 16 x n_a f64 values is staged in the 64 KiB
 * of LDS a workgroup may take).  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer. */
enum { NCA_EDT_MAX_AXIS = 512 };
size_t nca_vol_edt_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_edt(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t invert, float* out, void* work, size_t work_bytes,
                void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_edt_last_error(void);

/* ---- filt: Gaussian smoothing and the city-block distance of voxel stacks (ccta.gaussian_filter / cityblock_distance / binary_dilation /
 *      binary_erosion / mask_border / vessel_contrast / prepare_ccta, surface=True of metrics.mask_distances) ---------------------------------
 * The two filters the CCTA pipeline of the reference takes from scipy.ndimage: a separable symmetric filter with the `reflect` boundary,
 * and the distance in nodes along the axes (L1) to the nearest node above (or, inverted, not above) a threshold, from which every 6-connected
 * dilation, erosion and mask border follows by a comparison.  Purely additive to ABI 13.  Like the view, drr, vol, phantom, ssim and edt
 * sections, these entry points keep their OWN per-thread message (the accessor below); a refused call launches nothing and reads no device
 * pointer; a launch failure is reported once.  vol is f32 [n_vol][n0][n1][n2] contiguous on the device, on one NcaGrid (`grid` is a host pointer; lo
 * and inv are validated but unused: both filters count in nodes).  Every volume is filtered on its own: its result does not depend on n_vol or on its
 * neighbours in the stack.
 *
 * SMOOTHING.  radius: HOST int32 [3], 0 <= radius[a] <= NCA_SMOOTH_MAX_RADIUS.  weights: HOST f64, the half-weights of axis 0, then of axis
 * 1, then of axis 2, radius[a] + 1 each: w[0] is the centre, w[k] the weight of both nodes k away.  Any finite non-negative numbers (the
 * library never calls exp; ccta.gaussian_weights makes scipy's Gaussian and hands its bits over).  Every operation below is ONE rounded f64
 * operation in the order written (the kernels spell each one out: nothing leans on a contraction flag).
 *     x = (double)vol, exact.  The axes are filtered in the order 0, 1, 2, each on the result of the one before, with that axis's r and w:
 *     y[i] = x[i] w[0];   then for k = r, r - 1, .., 1 (the outermost pair first):   y[i] = y[i] + (x[R(i - k)] + x[R(i + k)]) w[k];
 *     R(j) = m if m < n, else 2 n - 1 - m, with m = j mod 2 n in 0 .. 2 n - 1 (scipy's `reflect`: d c b a | a b c d | d c b a; the map has
 *     period 2 n, so r may exceed the axis).   out = (float)(the result of axis 2): the one rounding to f32.
 * An axis with r = 0 and w[0] = 1 is x 1.0: unchanged.  In this order the result has the bits of
 * scipy.ndimage.gaussian_filter(x.astype(f64), sigma, radius=r, mode="reflect").astype(f32) (tests/test_filt_cpu.py); with the pairs summed
 * innermost first it is 1 ulp off.  Three launches (axis 0: f32 -> f64, axis 1: f64 -> f64, axis 2: f64 -> f32), each staging a tile of
 * lines with its reflected halo in LDS; the two f64 intermediates are the workspace: 16 bytes per node, rounded up to a multiple of 256.  The
 * 40 bytes per node the three launches read and write are what the filter moves.  The tiling sets no limit on an axis.  Every node of every
 * stage is written once by one thread: no atomics, the same bits on every run.  out may NOT alias vol (out == vol is refused; an overlap
 * is not detected).
 * NCA_E_INVALID (the message names the value): a NULL grid, vol, radius, weights or out; out == vol; n_vol <= 0; the grid refusals of
 * nca_drr_project; a negative radius; a weight that is not finite or is negative; more than 2^24 workgroups in one of the three launches.
 * NCA_E_UNSUPPORTED: a radius above NCA_SMOOTH_MAX_RADIUS.  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer.  The
 * query returns 0 for a grid or n_vol the entry point refuses. */
enum { NCA_SMOOTH_MAX_RADIUS = 32 };
size_t nca_vol_smooth_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_smooth(const NcaGrid* grid, const float* vol, int32_t n_vol, const int32_t radius[3], const double* weights, float* out, void* work,
                   size_t work_bytes, void* stream);

/* CITY-BLOCK DISTANCE.  Node j of volume v is a FEATURE iff ((double)vol[v][j] > threshold) != (invert != 0), the rule of nca_vol_edt: a
 * NaN value and a value equal to the threshold are features only under invert.
 *     out[v][i] = min over the features j of volume v of (|i_0 - j_0| + |i_1 - j_1| + |i_2 - j_2|),   an int32 count of nodes;
 *     with border = 1 the nodes just outside the grid are features too: the minimum also runs over min(i_a + 1, n_a - i_a), a = 0, 1, 2.
 * A volume without a feature and without a border gives 0x7fffffff at every node; a feature node gets 0.  Exact in integers; the sentinel is
 * never added to.  Formed separably: g = the distance to the nearest feature of the row (axis 2), b = min_j1 (|i_1 - j_1| + g),
 * out = min_j0 (|i_0 - j_0| + b), each stage with its own axis's border term.  Every node of every stage is written once by one thread: no
 * atomics, the same bits on every run.  With M = (vol > threshold), in scipy.ndimage's terms (6-connected structure, border_value 0):
 *     out <= n             (invert 0, border 0)  is binary_dilation(M, iterations=n);       out itself is distance_transform_cdt(~M, "taxicab");
 *     out > n              (invert 1, border 1)  is binary_erosion(M, iterations=n);         M and out == 1 is M ^ binary_erosion(M), the border.
 * The workspace holds g and b as int32 for every node: 8 bytes per node, rounded up to a multiple of 256.  The query returns it, and 0 for
 * arguments the entry point refuses.
 * NCA_E_INVALID (the message names the value): a NULL grid, vol or out; n_vol <= 0; invert or border not 0 / 1; a threshold that is NaN; the
 * grid refusals of nca_drr_project; more than 2^24 workgroups in one of the three launches (rows / 4, or tiles of 16 lines).
 * NCA_E_UNSUPPORTED: an axis longer than NCA_EDT_MAX_AXIS (a line tile of 16 x n_a int32 values is staged in LDS, and the row pass keeps
 * NCA_EDT_MAX_AXIS / 64 masks per row).  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer. */
size_t nca_vol_cityblock_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_cityblock(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t invert, int32_t border, int32_t* out, void* work,
                      size_t work_bytes, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_filt_last_error(void);

/* ---- resample: the cubic-spline zoom of voxel stacks (ccta.spline_filter / zoom / resample, resample= of ccta.prepare_ccta) ---------------
 * What the reference takes from scipy.ndimage.zoom(x, f, order=3) (mode "constant", prefilter, grid_mode False) to bring a CT and its
 * segmentations to unit spacing (preprocess/preprocess_ccta.py:57-60), and order 0 beside it.  Purely additive to ABI 13.  Like the other
 * view sections these entry points keep their OWN per-thread message (the accessor below); a refused call launches nothing and reads no
 * device pointer; a launch failure is reported once.  vol is f32 [n_vol][n0][n1][n2] contiguous on the device, on one NcaGrid (`grid` is a
 * host pointer; lo and inv are validated but unused: the zoom counts in nodes).  Every volume is resampled on its own.  Every operation below
 * is ONE rounded f64 operation in the order written (the kernels spell each one out: nothing leans on a contraction flag).
 *
 * PREFILTER (order 3).  c = (double)vol, exact.  The axes are taken in the order 0, 1, 2, each on the result of the one before.  On the host,
 * once:  z = sqrt(3.0) - 2.0;   gain = (1 - z) * (1 - 1 / z);   and for a line of n nodes zn = z multiplied by z another n - 2 times (zn = z
 * at n = 2; no pow).  They travel as kernel arguments.  Then, for every line of the axis:
 *     c[i] = c[i] * gain                                     for every i
 *     s = c[0] + zn * c[n-1];   zi = z
 *     for i = 1 .. n-2:   s = s + zi * (c[i] + zn * c[n-1-i]);   zi = zi * z
 *     c[0] = s / (1 - zn * zn)
 *     for i = 1 .. n-1:   c[i] = c[i] + z * c[i-1]
 *     c[n-1] = ((z * c[n-2] + c[n-1]) * z) / (z * z - 1)
 *     for i = n-2 .. 0:   c[i] = z * (c[i+1] - c[i])
 * This is scipy's ni_splines.c for the mirror boundary, which mode "constant" uses for the prefilter.  A line is serial by definition; one
 * thread owns a line and the parallelism is across lines.  Three launches (axis 0: f32 -> f64, axes 1 and 2 in place in coeff), each staging
 * sixteen whole lines in LDS, so an axis has at most NCA_EDT_MAX_AXIS nodes.  nca_vol_spline_filter writes c as f64 [n_vol][n0][n1][n2].
 * Against scipy.ndimage.spline_filter (whose build contracts some of these operations) c is a few f64 units off: at most 2^-44 of the
 * largest |vol| (tests/test_resample_cpu.py measures about 2^-47); the library is held to the definition above bit for bit.
 *
 * INTERPOLATION.  m: HOST int32 [3], the output's nodes per axis, every m[a] >= 2; out is f32 [n_vol][m0][m1][m2].  Per axis, on the host,
 * step_a = (n_a - 1) / (m_a - 1) in f64: end nodes map to end nodes.  For output index o of an axis:
 *     cc = min((double)o * step_a, (double)(n_a - 1))
 * order 3:   f = floor(cc);   y = cc - f;   t = 1 - y;
 *     w1 = (y*y*(y-2)*3+4)/6;   w2 = (t*t*(t-2)*3+4)/6;   w0 = t*t*t/6;   w3 = 1 - w0 - w1 - w2     (each left to right)
 *     the taps f-1 .. f+2, mirrored onto the line: j = M(f - 1 + k), M(i) = q if q <= n-1, else 2(n-1) - q, with q = i mod 2(n-1) in 0 .. 2n-3;
 *     acc = 0;   for k0, k1, k2 in lexicographic order:   acc = acc + ((c[j0][j1][j2] * w_k0) * w_k1) * w_k2;
 *     out = (float)acc: the one rounding to f32.
 * order 0:   one tap floor(cc + 0.5) per axis, no prefilter, out = vol at that node: exact, a NaN or an infinity included.
 * With the coefficients given, order 3 has the bits of scipy.ndimage.zoom(c, f, order=3, prefilter=False) and order 0 those of
 * zoom(x, f, order=0), for every size pair scipy does not overshoot at.  DELIBERATELY NOT scipy's: the min in cc.  Where (m_a - 1) * step_a
 * lands one ulp above n_a - 1 (4 -> 188 nodes, and about 4 % of all pairs), scipy takes the last output plane of that axis for outside the
 * volume and writes 0 into it; here the last output node is the last input node.  Orders 1, 2, 4 and 5, other boundary modes and grid_mode
 * are not offered.
 * nca_vol_zoom at order 3 runs the prefilter into the workspace (8 bytes per input node, rounded up to a multiple of 256) and then one
 * launch with a thread per output node, which forms cc, the weights and the taps from step_a: no tables.  Order 0 is that one launch and
 * needs no workspace (work may be NULL).  Every node of every stage is written once by one thread: no atomics, the same bits on every run.
 * out may NOT alias vol.  The query returns the workspace in bytes (0 at order 0), and 0 for arguments the entry point refuses.
 * NCA_E_INVALID (the message names the value): a NULL grid, vol, coeff, m or out; coeff == vol, out == vol; n_vol <= 0; the grid refusals of
 * nca_drr_project; m[a] < 2; an order other than 0 or 3; output nodes whose bytes overflow int64 or that need more than 2^24 workgroups of
 * 256 threads; more than 2^24 workgroups in one of the prefilter's launches (tiles of 16 lines).  NCA_E_UNSUPPORTED: at order 3 (and for
 * nca_vol_spline_filter) an axis longer than NCA_EDT_MAX_AXIS.  NCA_E_WORKSPACE: at order 3 work is NULL or work_bytes is below the query's
 * answer. */
int nca_vol_spline_filter(const NcaGrid* grid, const float* vol, int32_t n_vol, double* coeff, void* stream);
size_t nca_vol_zoom_workspace(const NcaGrid* grid_in, int32_t n_vol, int32_t order);
int nca_vol_zoom(const NcaGrid* grid_in, const float* vol, int32_t n_vol, const int32_t m[3], int32_t order, float* out, void* work, size_t work_bytes,
                 void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_resample_last_error(void);

/* ---- skel: the soft skeleton of voxel stacks and the sums clDice is made of (metrics.soft_skeleton / cldice) -------------------------------
 * The soft skeleton of Shit et al., "clDice -- a novel topology-preserving loss function for tubular structure segmentation" (CVPR 2021),
 * built from minimum and maximum stencils only, so it is exact in f32 and has the same bits on every run; and the two sums per volume from
 * which the topology precision and sensitivity of clDice follow.  Purely additive to ABI 13.  Like the other view sections these entry
 * points keep their OWN per-thread message (the accessor below); a refused call launches nothing and reads no device pointer; a launch
 * failure is reported once.  vol is f32 [n_vol][n0][n1][n2] contiguous on the device, on one NcaGrid (`grid` is a host pointer; lo and inv
 * are validated but unused: the stencils count in nodes).  Every volume is treated on its own: its result does not depend on n_vol or on
 * its neighbours in the stack.
 *
 * SOFT SKELETON.  Neighbours outside the grid are LEFT OUT (the -inf padding of max_pool3d; not the border_value = 0 of
 * ccta.binary_erosion: a volume that is 1 everywhere has an empty skeleton).
 *     min(a, b) = (b < a) ? b : a;   max(a, b) = (b > a) ? b : a;   relu(x) = (x > 0) ? x : +0
 *     erode(x)[i]  = the minimum over node i and its up to six axis neighbours: a = x[i], then a = min(a, x[i + o]) for the offsets
 *                    o = (-1,0,0), (0,-1,0), (0,0,-1), (0,0,+1), (0,+1,0), (+1,0,0) that stay inside the grid, in this (raster) order;
 *     dilate(x)[i] = the maximum over the up to 27 nodes of the 3 x 3 x 3 box around i: a = x[i], then a = max(a, x[i + o]) for the 26
 *                    offsets o != 0 in raster order, (-1,-1,-1), (-1,-1,0), .., (+1,+1,+1), that stay inside the grid;
 *     open(x) = dilate(erode(x)).
 * The order matters only for a NaN and for the sign of a zero: a NaN at the centre stays, a NaN neighbour is passed over; filling the
 * nodes outside the grid with +inf (erode) and -inf (dilate) is equivalent.  With iterations = K:
 *     E_0 = vol;   S = relu(E_0 - open(E_0));
 *     for j = 1 .. K:   E_j = erode(E_{j-1});   d = relu(E_j - open(E_j));   S = S + relu(d - S * d);
 *     out = S.
 * Every operation is ONE rounded f32 operation in the order written (no fused multiply-add).  For finite input the result equals, as
 * values, the published torch expression with soft_erode = the minimum of three 1-D -max_pool3d(-x) and soft_dilate = max_pool3d(x, 3, 1,
 * 1).  For a binary volume the result is binary and a subset of the volume.
 * K + 1 launches of one kernel: launch j stages a tile of E_j with a halo of two nodes in LDS, forms E_{j+1} on the tile grown by one
 * node, its box maximum, d and the update of S, and writes E_{j+1} and S for the tile's own nodes.  S lives in `out` and is updated in
 * place; the first launch writes every node of it.  E_j and E_{j+1} are the workspace: 8 bytes per node, rounded up to a multiple of 256.
 * The query returns it, and 0 for arguments the entry point refuses.  No atomics: the same bits on every run.  The tiling sets no limit on an
 * axis.  out may NOT alias vol (out == vol is refused; an overlap is not detected).
 * NCA_E_INVALID (the message names the value): a NULL grid, vol or out; out == vol; n_vol <= 0; the grid refusals of nca_drr_project;
 * iterations < 0; more than 2^31 - 1 tiles of 4 x 8 x 64 nodes in the stack (what one launch covers).  NCA_E_UNSUPPORTED: iterations above
 * NCA_SKEL_MAX_ITER.  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer. */
enum { NCA_SKEL_MAX_ITER = 512 };
size_t nca_vol_softskel_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_softskel(const NcaGrid* grid, const float* vol, int32_t n_vol, int32_t iterations, float* out, void* work, size_t work_bytes, void* stream);

/* OVERLAP SUMS.  a, b f32 [n_vol][n0][n1][n2] on the device (they may be the same stack); sums f64 [n_vol][2] on the device:
 *     sums[2 v] = the sum over the nodes i of volume v of (double)a[i] * (double)b[i];     sums[2 v + 1] = the sum of (double)a[i].
 * Each product is exact in f64.  The order of addition is fixed: a workgroup of 256 threads owns 4096 consecutive nodes of one volume,
 * thread t adds the nodes t, t + 256, .. in this order and the workgroup adds its threads in a binary tree; the per-workgroup sums are the
 * workspace (16 bytes per 4096 nodes of a volume, rounded up to a multiple of 256), and a second launch adds them per volume the same way.
 * No atomics: the same bits on every run.  Against the exact sum the result is within N 2^-53 of the sum of the absolute terms, N the
 * nodes of a volume; sums of whole numbers below 2^53 are exact.
 * NCA_E_INVALID: a NULL grid, a, b or sums; n_vol <= 0; the grid refusals of nca_drr_project; more than 2^24 workgroups in the first
 * launch.  NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer.  The query returns 0 for arguments the entry point
 * refuses. */
size_t nca_vol_overlap_sums_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_overlap_sums(const NcaGrid* grid, const float* a, const float* b, int32_t n_vol, double* sums, void* work, size_t work_bytes, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_skel_last_error(void);

/* ---- label: the connected components of thresholded voxel stacks (metrics.label / component_sizes / keep_largest / component_report) --------
 * What scipy.ndimage.label(vol > threshold, generate_binary_structure(3, connectivity)) returns, numbering included, for every volume of a
 * stack; and the node count of every label.  Purely additive to ABI 13.  Like the other view sections these entry points keep their OWN
 * per-thread message (the accessor below); a refused call launches nothing and reads no device pointer; a launch failure is reported once.
 * vol is f32 [n_vol][n0][n1][n2] contiguous on the device, on one NcaGrid (`grid` is a host pointer; lo and inv are validated but unused:
 * neighbourhoods count in nodes).  Every volume is labelled on its own: its result does not depend on n_vol or on its neighbours in the stack.
 *
 * LABEL.  For one volume:
 *     node j is ON THE MASK iff ((double)vol[j] > threshold) != (invert != 0), the rule of nca_vol_edt: a NaN value and a value equal to
 *         the threshold are on the mask only under invert;
 *     two nodes of the mask are NEIGHBOURS iff their indices differ by at most 1 along every axis and along at least one and at most
 *         `connectivity` axes: connectivity 1 / 2 / 3 gives 6 / 18 / 26 neighbours, scipy.ndimage.generate_binary_structure(3, connectivity);
 *     a COMPONENT is a class of the transitive closure of that relation on the mask;
 *     the components are numbered 1 .. count in increasing order of their smallest linear node index (i0 n1 + i1) n2 + i2: first
 *         encounter in raster order, scipy.ndimage.label's numbering;
 *     labels[j] (int32) = the number of j's component on the mask, 0 elsewhere;   counts[v] (int32) = count.
 * The result is a function of the mask alone: the same bits on every run, although the kernels use atomics.
 * Six launches: a union-find in LDS over every tile of 4 x 8 x 64 nodes; the unions across tile faces, edges and corners in global memory
 * (a returning atomicMin links the larger root under the smaller); a read-only flattening that writes every node's root and counts the
 * roots per 1024 nodes; the scan of those counts per volume; the numbering of the roots; the relabelling of every node from its root.  No
 * launch waits for another workgroup and every loop is bounded by the node count (csrc/view/nca_label.hip states why).  No line is staged, so
 * the tiling sets no limit on an axis.  labels may NOT alias vol (labels == vol is refused; an overlap is not detected).
 * The workspace holds the root of every node as int32 and one int32 per 1024 nodes of every volume:
 *     round256(4 n_vol n0 n1 n2) + round256(4 n_vol ceil(n0 n1 n2 / 1024)) bytes,   round256(b) = b rounded up to a multiple of 256.
 * The query returns it, and 0 for arguments the entry point refuses.
 * NCA_E_INVALID (the message names the value): a NULL grid, vol, labels or counts; labels == vol; n_vol <= 0; invert not 0 / 1; a threshold
 * that is NaN; the grid refusals of nca_drr_project; more than 2^31 - 1 tiles of 4 x 8 x 64 nodes in the stack (what one launch covers).
 * NCA_E_UNSUPPORTED: a connectivity other than 1, 2 or 3; a volume of more than 2^31 - 2 nodes (a label is a node index plus one in int32).
 * NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer. */
size_t nca_vol_label_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_label(const NcaGrid* grid, const float* vol, int32_t n_vol, double threshold, int32_t connectivity, int32_t invert, int32_t* labels,
                  int32_t* counts, void* work, size_t work_bytes, void* stream);

/* COMPONENT SIZES.  labels int32 [n_vol][n0][n1][n2] on the device (any labels, nca_vol_label's or not); sizes int32 [n_vol][cap] on the device:
 *     sizes[v cap + l] = the number of nodes of volume v whose label is l, for 0 <= l < cap: entry 0 is the background.
 * A label outside [0, cap) is not counted.  The entry point zeroes `sizes` itself (a fill kernel on the stream: a captured call replays), then one launch: runs of equal
 * labels are merged within a wave, then per workgroup of 4096 nodes in a table of 256 slots in LDS, and every slot is one integer atomicAdd
 * -- exact in any order, the same bits on every run.  No workspace.
 * NCA_E_INVALID: a NULL grid, labels or sizes; n_vol <= 0; cap <= 0; the grid refusals of nca_drr_project; more than 2^24 workgroups.
 * NCA_E_UNSUPPORTED: a volume of more than 2^31 - 2 nodes. */
int nca_vol_label_sizes(const NcaGrid* grid, const int32_t* labels, int32_t n_vol, int32_t cap, int32_t* sizes, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_label_last_error(void);

/* ---- vess: the multi-scale Hessian vesselness of voxel stacks (ccta.hessian_eigenvalues / vesselness) ---------------------------------------
 * The tubeness of Frangi et al., "Multiscale vessel enhancement filtering" (MICCAI 1998), from the eigenvalues of the scale-normalised
 * Hessian of an ALREADY SMOOTHED volume: one call per scale, everything after the Gaussian (nca_vol_smooth) in one launch.  Purely additive
 * to ABI 13.  Like the other view sections these entry points keep their OWN per-thread message (the accessor below); a refused call
 * launches nothing and reads no device pointer; a launch failure is reported once.  s is f32 [n_vol][n0][n1][n2] contiguous on the device,
 * the volume smoothed at sigma, on one NcaGrid (`grid` is a host pointer; lo and inv are validated but unused: everything counts in nodes,
 * so the spacing is taken as isotropic); scale = sigma^2.  Every volume is treated on its own: its result does not depend on n_vol or on
 * its neighbours in the stack.  Every operation below is ONE rounded f64 operation in the order written (no fused multiply-add), so a
 * transcription into any IEEE arithmetic has the same bits up to exp.
 *
 * HESSIAN at node i = (i0, i1, i2), in f64 from the f32 values.  Every index is clamped to [0, n_a - 1] on its own axis (edge replication);
 * e_a is the unit step along axis a:
 *     D_aa = (s[i + e_a] - s[i]) - (s[i] - s[i - e_a]);
 *     D_ab = 0.25 * ((s[i + e_a + e_b] - s[i + e_a - e_b]) - (s[i - e_a + e_b] - s[i - e_a - e_b]))       for a < b;
 *     H = scale * D, the six entries H_00, H_01, H_02, H_11, H_12, H_22.
 * If any of the six is not finite, all three eigenvalues are NaN and the vesselness is +0; the solver is not run.
 *
 * EIGENVALUES.  Cyclic Jacobi on the symmetric a = H: exactly 5 sweeps, each over the pairs (p, q) = (0,1), (0,2), (1,2), r the third index.
 * A pair with a_pq == 0 is skipped.  Otherwise
 *     theta = (a_qq - a_pp) / (2 * a_pq);     t = sgn / (|theta| + sqrt(theta * theta + 1)),  sgn = -1 if theta < 0, else +1;
 *     c = 1 / sqrt(t * t + 1);     s = t * c;
 *     a_pp = a_pp - t * a_pq;     a_qq = a_qq + t * a_pq   (both from the old a_pq);     a_pq = 0;
 *     (a_rp, a_rq) = (c * a_rp - s * a_rq,  s * a_rp + c * a_rq)   (both from the old pair).
 * After 5 sweeps the diagonal is within 2^-49 |H|_F of the eigenvalues (measured against LAPACK on 10^6 matrices: random, nearly
 * degenerate, tube-like, scaled over 10^+-16, small integers).  (x_0, x_1, x_2) = (a_00, a_11, a_22) is then sorted by three
 * compare-and-swaps on the positions (0,1), (1,2), (0,1): x_i and x_j, i < j, change places iff |x_j| < |x_i|, or |x_j| == |x_i| and
 * x_j < x_i.  (l1, l2, l3) = the result: ascending in absolute value, the smaller value first on a tie.  A NaN (an overflow inside the
 * solver) swaps with nothing and is written as the canonical quiet NaN.
 *
 * VESSELNESS of bright tubes (bright = 1).  V = +0 unless l2 < 0 and l3 < 0; then, with c = c[v] of the node's volume,
 *     Ra2 = (l2 * l2) / (l3 * l3);     Rb2 = (l1 * l1) / |l2 * l3|;     S2 = (l1 * l1 + l2 * l2) + l3 * l3;
 *     A = 1 - exp(-Ra2 / (2 * (alpha * alpha)));     B = exp(-Rb2 / (2 * (beta * beta)));     C = 1 - exp(-S2 / (2 * (c * c))),  C = 1 if c == 0;
 *     V = (A * B) * C, rounded once to f32.
 * bright = 0 (dark tubes) takes l2 > 0 and l3 > 0 instead.  Every step above is odd or even in s bit for bit, so that is the bright
 * vesselness of -s -- except at a node where two eigenvalues of opposite sign tie in absolute value, which the tie rule orders the same way
 * for s and -s.  V lies in [0, 1].  c[v] is read on the device and not checked.
 *
 * nca_vol_hessian_eig: eig f32 [n_vol][3][n0][n1][n2] = (l1, l2, l3), each rounded once to f32.
 * nca_vol_hessian_norm_max: norm_max f64 [n_vol] on the device, norm_max[v] = max(+0, the maximum over the nodes of volume v of
 *     S2' = (x1 * x1 + x2 * x2) + x3 * x3,  x_j = l_j rounded to f32 and taken back to f64) -- the S2 of what nca_vol_hessian_eig writes, so
 *     a caller can form the same number from eig.  max(a, b) = (b > a) ? b : a: a NaN is passed over, +inf is kept.  The entry point zeroes
 *     norm_max itself (a fill kernel on the stream: a captured call replays); a workgroup takes the maximum of its tile in a tree and makes one integer atomicMax on the
 *     bit pattern, which orders non-negative doubles as their values do: exact in any order, the same bits on every run.  Frangi's rule is
 *     c = 0.5 sqrt(norm_max).
 * nca_vol_vesselness: out f32 [n_vol][n0][n1][n2], scale_out int32 of the same shape or NULL.  scale_index == 0: every node of out is
 *     written with V and every node of scale_out with 0.  scale_index > 0: out and scale_out are read-modify-write, a node is replaced by
 *     (V, scale_index) only where V > out (the f32 values): over increasing scale_index the result is the maximum over the scales and the
 *     SMALLEST index that attains it.
 * One launch each (norm_max: the fill kernel before it).  A workgroup owns a tile of 4 x 8 x 64 nodes, stages it with a halo of one node in LDS
 * (6 x 10 x 66 f32), and each thread forms the 19-point stencil of its four nodes and runs the solver in registers.  Every node is written
 * once by the thread that owns it.  No workspace.  The tiling sets no limit on an axis.  No output may be s itself (refused; an overlap is
 * not detected).
 * NCA_E_INVALID (the message names the value): a NULL grid, s, eig / norm_max / out or c; an output that is s; n_vol <= 0; the grid
 * refusals of nca_drr_project; a scale, alpha or beta that is not finite and positive; bright not 0 / 1; scale_index < 0; more than
 * 2^31 - 1 tiles of 4 x 8 x 64 nodes in the stack (what one launch covers). */
int nca_vol_hessian_eig(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, float* eig, void* stream);
int nca_vol_hessian_norm_max(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, double* norm_max, void* stream);
int nca_vol_vesselness(const NcaGrid* grid, const float* s, int32_t n_vol, double scale, double alpha, double beta, const double* c, int32_t bright,
                       int32_t scale_index, float* out, int32_t* scale_out, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_vess_last_error(void);

/* ---- mesh: the iso-surfaces of voxel stacks as indexed triangle meshes (mesh.isosurface / export.density_surfaces) ---------------------------
 * Marching tetrahedra on the Kuhn (Freudenthal) split of every grid cell: a 16-case table, no ambiguous case, and a split that is the same in
 * every cell and agrees across cell faces, so the mesh is an oriented closed 2-manifold wherever the surface does not touch a face of the
 * grid.  Purely additive to ABI 13.  Like the other view sections these entry points keep their OWN per-thread message (the accessor below);
 * a refused call launches nothing and reads no device pointer; a launch failure is reported once.  vol is f32 [n_vol][n0][n1][n2] contiguous
 * on the device, on one NcaGrid (`grid` is a host pointer); level is a finite f32.  Every volume is meshed on its own: its result does not
 * depend on n_vol or on its neighbours in the stack, and its vertex indices start at 0.  Every f64 operation below is ONE rounded operation
 * in the order written (no fused multiply-add anywhere), so a transcription into any IEEE arithmetic has the same bits.
 *
 * INSIDE.  Node j is inside iff vol[j] > level as f32: a NaN and a value equal to the level are not.
 * EDGES.  Node i = (i0, i1, i2), linear index (i0 n1 + i1) n2 + i2, OWNS the edges k = 1 .. 7 to i + d_k, d_k = ((k >> 2) & 1, (k >> 1) & 1,
 *     k & 1), whose far end is a node of the grid.  An edge whose ends differ in "inside" is CROSSED and carries exactly one vertex.
 * VERTICES.  With a the owning end, b the far end and v_a, v_b their values taken to f64:
 *     t = ((double)level - v_a) / (v_b - v_a);   t = 0.5 if that is not finite, else min(max(t, 0), 1);
 *     q_x = (double)i_x + t on the axes x with d_x = 1, (double)i_x on the others;   h_x = 1 / inv_x;   vertex_x = (float)(lo_x + q_x * h_x).
 *     The vertices of a volume are numbered by (linear index of the owning node, k) ascending: no vertex twice, no gaps.
 * NORMALS (optional), per vertex.  G_x(i) = (0.5 * ((double)vol[i + e_x] - (double)vol[i - e_x])) * inv_x with both indices clamped to
 *     [0, n_x - 1] (edge replication, as in "vess");   m_x = -(G_x(a) + t * (G_x(b) - G_x(a)));   len = sqrt((m_0 m_0 + m_1 m_1) + m_2 m_2);
 *     normal_x = (float)(m_x / len), or (+0, +0, +0) where len is 0 or not finite.  It points to the outside (down the values).
 * CELLS.  Every node c with c_x + 1 < n_x on all three axes is the base of a cell, numbered by c's linear index.  A cell has six tetrahedra
 *     q = 0 .. 5, one per permutation (a, b, c') of the axes in the order (0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0), with the corners
 *     p0 = c, p1 = p0 + e_a, p2 = p1 + e_b, p3 = p2 + e_c' = c + (1,1,1).  Tetrahedra 1, 2 and 5 (the odd permutations) are mirror images.
 * TRIANGLES.  The edges of a tetrahedron are numbered 0 .. 5 = (p0 p1), (p0 p2), (p0 p3), (p1 p2), (p1 p3), (p2 p3); each is the edge k = the
 *     difference of its ends, owned by its lower end.  With case = sum over the corners p_i inside of 2^i, the triangles are, as edge numbers:
 *         1: 0 1 2      2: 0 4 3      4: 1 3 5      8: 2 5 4       7: 2 4 5      11: 1 5 3      13: 0 3 4      14: 0 2 1
 *         3: 1 2 4, 1 4 3      5: 0 3 5, 0 5 2      6: 0 4 5, 0 5 1      9: 0 1 5, 0 5 4      10: 0 2 5, 0 5 3      12: 1 3 4, 1 4 2
 *     (cases 0 and 15: none; two corners inside: the quadrilateral is split along the diagonal from its lowest-numbered edge).  In an odd
 *     tetrahedron the second and third vertex of every triangle change places.  Every triangle is counter-clockwise seen from the outside,
 *     so the divergence-theorem volume of a bright blob is positive.  The triangles of a volume are ordered by (cell, tetrahedron, position
 *     in the list above); a triangle is three vertex numbers of its volume, int32.  Triangles of zero area (a node exactly at the level gives
 *     t = 0 or 1) are kept: the combinatorics stay those of a manifold.
 *
 * nca_vol_iso_count: totals int64 [n_vol][2] on the device = (vertices, triangles) of every volume, and in the workspace every node's first
 *     vertex and first triangle within its volume and every volume's first of both in the stack.  Five launches: per tile of 4 x 8 x 64 nodes,
 *     staged with the next node on every axis in LDS (5 x 9 x 65 f32), every node's crossing mask and its cell's triangle count as one 16-bit
 *     word; then an exclusive scan per volume in three steps -- the sums of every 1024 consecutive nodes, their scan by one workgroup per
 *     volume (and one workgroup for the stack), and the scan within every 1024 nodes plus that offset.  Offsets within a volume are int32:
 *     a grid with 7 n0 n1 n2 or 12 (n0 - 1)(n1 - 1)(n2 - 1) above 2^31 - 1 is refused.
 * nca_vol_iso_emit: after nca_vol_iso_count on the same arguments and workspace, and after the caller has read totals to size the outputs:
 *     verts f32 [sum V][3], tris int32 [sum T][3], normals f32 [sum V][3] or NULL, the volumes back to back in stack order.  One launch over
 *     the same tiles; every vertex and triangle is written once, by the thread that owns it.  A store is made only below vert_cap vertices
 *     and tri_cap triangles, whatever the workspace holds; verts (and normals) may be NULL when vert_cap is 0, tris when tri_cap is 0, and
 *     with both 0 nothing is launched.
 * No atomics, no workgroup waits for another: the same bits on every run.  The tiling sets no limit on an axis.
 * The workspace, with s = n0 n1 n2 rounded up to a multiple of 4 and round256 as in "label":
 *     round256(2 n_vol s) + 2 round256(4 n_vol s) + round256(8 n_vol ceil(n0 n1 n2 / 1024)) + 2 round256(16 n_vol) bytes.
 * The query returns it, and 0 for arguments the entry points refuse.
 * NCA_E_INVALID (the message names the value): a NULL grid, vol or totals; a negative capacity; NULL verts or tris with a positive capacity;
 * n_vol <= 0; the grid refusals of nca_drr_project; a level that is not finite; more than 2^31 - 1 tiles of 4 x 8 x 64 nodes or runs of 1024
 * nodes in the stack (what one launch covers).
 * NCA_E_UNSUPPORTED: a grid whose worst case overflows the int32 offsets.   NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's
 * answer.  The order: pointers and capacities, n_vol, the grid, the offsets, the level, the workspace, the launch limits. */
size_t nca_vol_iso_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_iso_count(const NcaGrid* grid, const float* vol, int32_t n_vol, float level, int64_t* totals, void* work, size_t work_bytes, void* stream);
int nca_vol_iso_emit(const NcaGrid* grid, const float* vol, int32_t n_vol, float level, const void* work, size_t work_bytes, int64_t vert_cap, int64_t tri_cap,
                     float* verts, int32_t* tris, float* normals, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_mesh_last_error(void);

/* ---- path: geodesic distances under a cost, predecessors, traced paths and ball cover (centreline.geodesic_distance / extract) ---------------
 * Minimal paths on the grid graph of a voxel stack: what the TEASAR centreline loop of centreline.extract runs on.  Purely additive to ABI 13.
 * Like the other view sections these entry points keep their OWN per-thread message (the accessor below); a refused call launches nothing
 * and reads no device pointer; a launch failure is reported once.  Every entry point launches on `stream` and nothing else and reads nothing
 * back.  Every f64 operation below is ONE rounded operation in the order written (no fused multiply-add anywhere: D[u] + w must not be
 * fused), so a transcription into any IEEE arithmetic has the same bits.
 *
 * GRID.  An NcaGrid, checked as nca_check_stack does (no limit on an axis); a volume has at most 2^31 - 2 nodes.  h_a = 1.0 / inv_a in f64.
 * OPEN NODES.  cost is f32 [n_vol][n0][n1][n2].  A node is OPEN when its cost is finite and >= 0; every other node (NaN, +-inf, negative) is
 *     a WALL.
 * NEIGHBOURS.  conn = 1, 2 or 3: the offsets d = (d0, d1, d2) in {-1, 0, 1}^3 with 1 .. conn non-zero components (6, 18 or 26, as in
 *     "label"), enumerated in ascending (d0, d1, d2) order.
 * EDGES.  len(d) = sqrt(((d0 h0)^2 + (d1 h1)^2) + (d2 h2)^2);   w(u, v) = len(d) * (0.5 * ((double)cost[u] + (double)cost[v])), symmetric.
 * DISTANCE.  dist is f64 [n_vol][n0][n1][n2], in/out.  The caller initialises it: 0 at seeds, +inf elsewhere; any non-negative field is
 *     accepted (a run can be resumed, and re-seeded by lowering values).  Walls are written as +inf.  The fixed point is
 *         D[v] = min(D_in[v], min over the open neighbours u of v of fl(D[u] + w(u, v)))   on the open nodes v.
 * SWEEP.  The grid is cut into tiles of 4 x 8 x 64 nodes.  Sweep s reads state s - 1 everywhere and replaces every tile T by the fixed
 *     point of the relaxation restricted to T, the nodes one step outside T frozen at their values of state s - 1.  State s is a function of
 *     the input alone, converged or not.  A tile CHANGED in sweep s when a node of it has another value in state s than in state s - 1
 *     (a wall that held a finite value counts).
 * PREDECESSOR.  pred[v], int32: among the open neighbours u of an open v with D[u] < D[v] strictly, the linear index within the volume of
 *     the one that minimises fl(D[u] + w(u, v)), the first in offset order on a tie; -1 when there is none (seeds, unreachable nodes, walls,
 *     zero-weight plateaus).  Every chain strictly decreases in D: no cycles.
 * TRACE.  From starts[p] follow pred: the nodes go to row p of paths int32 [n_paths][max_len], the tail is filled with -1, lengths[p] is
 *     the number of nodes written.  The walk stops after writing a node whose stop byte is non-zero (status 1; stop is uint8 [voxels] or
 *     NULL), else at a node whose pred word is outside [0, voxels) (status 0), else after max_len nodes (status 2).  A start outside
 *     [0, voxels) writes nothing (status 3; pred holds -1 on a wall as on a seed, so a wall that is a start gives one node and status 0).
 *     Bounded by max_len for ANY contents of pred.
 * BALL COVER.  n_points pairs of a node index (negative or >= voxels: skipped) and an f32 radius r: covered[x] = 1 (uint8, in/out, only ever
 *     set) for every node x of the grid with ((x0 - p0) h0)^2 + ((x1 - p1) h1)^2 + ((x2 - p2) h2)^2 <= (double)r * (double)r, the sum in
 *     axis order, the differences exact.  A NaN radius covers nothing.  All writers write the same value: no atomics.
 *
 * nca_vol_geodesic: `sweeps` >= 1 sweeps, ping-pong between dist and the workspace; the result is in dist whatever the parity of sweeps
 *     (an odd count ends with a copy).  changed int32 [n_vol] on the device: the tiles of that volume that changed in the LAST sweep; 0
 *     means the fixed point is reached.  A workgroup brings its tile to the fixed point in LDS in rounds; it waits for no other workgroup,
 *     and no atomics touch D: the same bits on every run.  With skipping on (nca_path_set_skip, the default) a tile is not run in a sweep
 *     when neither it nor any of its 26 neighbour tiles changed in the sweep before (never in the first sweep of a call): the bits are the
 *     same either way.  The workspace, with round256 as in "label" and tiles = ceil(n0 / 4) ceil(n1 / 8) ceil(n2 / 64):
 *         round256(8 n_vol n0 n1 n2) + 2 round256(n_vol tiles) bytes.   The query returns it, and 0 for arguments the entry point refuses.
 * nca_vol_geodesic_pred: one launch, one thread per node.   nca_vol_trace_paths: one volume, one thread per path.
 * nca_vol_ball_cover: one volume, one workgroup per point over the ball's box clipped to the grid.
 * NCA_E_INVALID (the message names the value): a NULL grid or pointer (stop alone may be NULL); n_vol, sweeps, voxels, n_paths, max_len
 * or n_points <= 0; the grid refusals of nca_drr_project; more than 2^31 - 1 tiles or runs of 256 nodes in the stack (what one launch
 * covers); nca_path_set_skip with a value that is neither 0 nor 1.   NCA_E_UNSUPPORTED: conn outside 1 .. 3; a volume of more than 2^31 - 2
 * nodes.   NCA_E_WORKSPACE: work is NULL or work_bytes is below the query's answer.  The order: pointers, the counts and the grid, conn,
 * sweeps, the workspace, the launch limits, the node count. */
size_t nca_vol_geodesic_workspace(const NcaGrid* grid, int32_t n_vol);
int nca_vol_geodesic(const NcaGrid* grid, int32_t n_vol, const float* cost, double* dist, int32_t conn, int32_t sweeps, int32_t* changed, void* work,
                     size_t work_bytes, void* stream);
int nca_vol_geodesic_pred(const NcaGrid* grid, int32_t n_vol, const float* cost, const double* dist, int32_t conn, int32_t* pred, void* stream);
int nca_vol_trace_paths(int64_t voxels, const int32_t* pred, const uint8_t* stop, int32_t n_paths, const int32_t* starts, int32_t max_len, int32_t* paths,
                        int32_t* lengths, int32_t* status, void* stream);
int nca_vol_ball_cover(const NcaGrid* grid, int32_t n_points, const int32_t* nodes, const float* radius, uint8_t* covered, void* stream);
int nca_path_set_skip(int32_t on);
int nca_path_get_skip(void);

/* The message of the calling thread's last failed call of this section. */
const char* nca_path_last_error(void);

/* ---- cpr: oblique planes and lumen rays through voxel stacks (reformat.cross_sections / lumen_profile) -----------------------------------------
 * The gathers of a curved-planar reformation and of a lumen profile along a centreline: many small planes, or fans of rays in such planes,
 * through a stack of volumes on one NcaGrid.  Purely additive to ABI 13.  Like the other view sections these entry points keep their OWN
 * per-thread message (the accessor below); a refused call launches nothing and reads no device pointer; a launch failure is reported once.
 * Every entry point launches on `stream` and nothing else and reads nothing back.  Every f64 operation below is ONE rounded operation in the
 * order written (no fused multiply-add anywhere; the kernels spell each one out), so a transcription into any IEEE arithmetic has the same
 * bits.  `grid` is a host pointer; every other pointer is on the device.
 *
 * PLANES.  n_planes planes: origin, e1 and e2 are f64 [n_planes][3], in world coordinates.  Nothing checks that e1 and e2 are orthonormal:
 *     they are used as given.
 * WORLD TO GRID.  For a world point p:  x_a = (p_a - lo_a) * inv_a.  The point is INSIDE when 0 <= x_a <= n_a - 1 on all three axes, the
 *     comparisons as written: a NaN coordinate is outside.
 * ORDER 1 (the value g(p) of an inside point in a stack of f32 nodes):  f_a = min(floor(x_a), n_a - 2);   y_a = x_a - f_a;   the eight nodes
 *     (f_0 + a, f_1 + b, f_2 + c), a, b, c in {0, 1}, widened to f64; a pair (lo: offset 0, hi: offset 1) is combined as
 *         lo + y * (hi - lo)                                                       (three operations)
 *     along axis 2 (four pairs, y_2), then along axis 1 (two pairs of those results, y_1), then along axis 0 (y_0).  With y = 0 the result
 *     is lo, and with y = 1 (the last node of an axis, where f = n - 2) it is hi, whenever hi - lo is finite and exact in f64 -- for f32
 *     nodes: whenever both are finite and their exponents lie within 29 of each other -- so a point on a node returns that node's value.
 * ORDER 3 (a stack of f64 coefficients, what nca_vol_spline_filter writes):  per axis cc = x_a, then f, y, t, the weights w0 .. w3, the
 *     mirrored taps j = M(f - 1 + k) and the lexicographic accumulation acc exactly as under INTERPOLATION of the "resample" section.
 *
 * nca_vol_sample_planes: out is f32 [n_vol][n_planes][nu][nv].  Pixel (i, j) of plane k:
 *         u = ((double)i - 0.5 * (double)(nu - 1)) * du;      v = ((double)j - 0.5 * (double)(nv - 1)) * dv;
 *         p_a = (origin[k][a] + u * e1[k][a]) + v * e2[k][a].
 *     A point that is not inside gives `fill` (any f32, its bits kept).  Else, per volume q:
 *     order 0: src is the f32 stack [n_vol][n0][n1][n2]; out = the node floor(x_a + 0.5) per axis: exact, a NaN or an infinity included.
 *     order 1: src is the f32 stack; out = (float)g(p): the one rounding to f32.
 *     order 3: src is the f64 coefficient stack; out = (float)acc.
 *     One thread per pixel, a workgroup per tile of 16 x 16 pixels of one plane.  The coordinates, tap indices and weights of a pixel are
 *     formed once and reused for all n_vol volumes.  Every output is written once by one thread: no atomics, the same bits on every run.
 * nca_vol_lumen: vol is the f32 stack; dirs is f64 [n_ang][2], the host's (cos, sin) of 2 pi a / n_ang, and sin_step the host's
 *     sin(2 pi / n_ang): both are inputs, no transcendental is evaluated on the device.  Ray a of plane k in volume q takes the samples
 *     j = 0 .. n_steps:
 *         r_j = (double)j * dr;   c = r_j * dirs[a][0];   s = r_j * dirs[a][1];   p_a = (origin[k][a] + c * e1[k][a]) + s * e2[k][a];
 *         g_j = g(p), order 1, kept in f64.
 *     The ray ends at the first j at which
 *         the sample is not inside:   r = r_{j-1} (0 at j = 0), status bit 4;   or else
 *         !(g_j > level):   at j = 0   r = 0 and status bit 1 (the centre is not in the lumen);
 *                           at j > 0   t = (g_{j-1} - level) / (g_{j-1} - g_j), t = 0 when g_j is not finite;   r = ((double)(j - 1) + t) * dr.
 *     If no sample ends it:   r = (double)n_steps * dr, status bit 2 (open).
 *     radius f32 [n_vol][n_planes][n_ang] = (float)r.   status int32 [n_vol][n_planes] = the OR of the bits of the plane's rays.
 *     stats f64 [n_vol][n_planes][4], from the unrounded r, every sum starting at 0 and taken in ascending a:
 *         [0] area = (0.5 * sin_step) * sum_a r_a * r_{(a + 1) mod n_ang}             (the polygon through the ray ends)
 *         [1] the minimum and [2] the maximum of D_a = r_a + r_{a + n_ang / 2}, a = 0 .. n_ang / 2 - 1, each starting from D_0 and replaced
 *             when D_a < min (D_a > max) holds
 *         [3] mean = (sum_a r_a) / (double)n_ang.
 *     One workgroup per (volume, plane): a thread per ray (looping when n_ang exceeds the workgroup's 256 threads), the unrounded r in LDS,
 *     the sums by one thread each in the stated order.  No workgroup waits for another and no atomics touch global memory: the same bits
 *     on every run.
 * NCA_E_INVALID (the message names the value): a NULL grid or pointer; n_vol, n_planes, nu, nv or n_steps <= 0; the grid refusals of
 * nca_drr_project (the node count taken at 8 bytes per node); a du, dv or dr that is not finite and positive; a sin_step that is not finite;
 * a NaN level; n_ang odd or below 4; more than 2^31 - 1 workgroups, or outputs whose bytes overflow int64 (what one launch covers).
 * NCA_E_UNSUPPORTED: order outside {0, 1, 3}; n_ang above NCA_CPR_MAX_ANGLES.
 * The order: the pointers as the arguments list them; n_vol and the grid; then order, n_planes, nu, nv, du, dv (planes) or n_planes, n_ang,
 * n_steps, sin_step, level, dr (lumen); the launch limits last. */
enum { NCA_CPR_MAX_ANGLES = 1024, NCA_CPR_STATUS_CENTRE = 1, NCA_CPR_STATUS_OPEN = 2, NCA_CPR_STATUS_GRID = 4 };
int nca_vol_sample_planes(const NcaGrid* grid, int32_t n_vol, const void* src, int32_t order, int32_t n_planes, const double* origin, const double* e1,
                          const double* e2, int32_t nu, int32_t nv, double du, double dv, float fill, float* out, void* stream);
int nca_vol_lumen(const NcaGrid* grid, int32_t n_vol, const float* vol, int32_t n_planes, const double* origin, const double* e1, const double* e2,
                  int32_t n_ang, const double* dirs, double sin_step, double level, double dr, int32_t n_steps, float* radius, double* stats,
                  int32_t* status, void* stream);

/* The message of the calling thread's last failed call of this section. */
const char* nca_cpr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NERFCA_HIP_H */
