/*
 * hlgs.h -- C ABI of libhlgs.so, the MI355X (gfx950) differentiable Gaussian-splat rasterizer
 * with hierarchical level-of-detail selection.
 *
 * Drop-in boundary: every entry point below replaces one native function the reference binds
 * through pybind11 (paths relative to /root/reference):
 *
 *   hlgs_rasterize_forward_prepare/_render  <- RasterizeGaussiansCUDA
 *        submodules/hierarchy-rasterizer/rasterize_points.cu:36-139 (bound as _C.rasterize_gaussians,
 *        ext.cpp:16); split in two phases at the reference's own host sync (rasterizer_impl.cu:330-333)
 *        so that the caller allocates the binning buffer, as the reference's resize lambda did
 *        (rasterize_points.cu:28-34).
 *   hlgs_rasterize_backward[_split]         <- RasterizeGaussiansBackwardCUDA, rasterize_points.cu:141-245
 *   hlgs_mark_visible                       <- CudaRasterizer::Rasterizer::markVisible,
 *        rasterizer_impl.cu:145-157 (called as _C.mark_visible at diff_gaussian_rasterization/__init__.py:174)
 *   hlgs_compute_relocation                 <- ComputeRelocationCUDA, rasterize_points.cu:248-271
 *   hlgs_expand_to_size_dynamic             <- ExpandToSizeDynamic, gaussianhierarchy/torch/torch_interface.cpp:171-194
 *   hlgs_get_interpolation_weights_dynamic  <- GetTsIndexedDynamic, torch_interface.cpp:222-244
 *   hlgs_expand_to_size                     <- ExpandToSize, torch_interface.cpp:148-169
 *   hlgs_get_interpolation_weights          <- GetTsIndexed, torch_interface.cpp:200-220
 *   hlgs_spt_cut_prepare/_finish            <- GetSPTCut, torch_interface.cpp:287-316 (two phases at the
 *        reference's candidate-count sync, runtime_switching.cu:926-931)
 *   hlgs_lod_interp_forward/_backward       <- the Python child/parent lerp of render_post,
 *        gaussian_renderer/__init__.py:304-339 (interp_python=True), and its autograd
 *   hlgs_upper_tree_cut, hlgs_spt_cache_plan, hlgs_copy_rows, hlgs_adam_step, hlgs_spt_build
 *                                           <- the SPT streaming step of train_post.py:323-491, 786-812 and
 *        GaussianModel.build_hierarchical_SPT (scene/gaussian_model.py:184-352), which the reference runs as
 *        Python loops over torch ops
 *   hlgs_adam_update                        <- adamUpdate, submodules/alt-rasterizer/rasterize_points.cu:255-281
 *        (kernel cuda_rasterizer/adam.cu:9-36), bound as _C.adamUpdate (ext.cpp:19)
 *   hlgs_photo_forward/_backward            <- the torch ops between the rasterizer and the loss: the exposure of
 *        render(..., use_trained_exp=True) (gaussian_renderer/__init__.py:139-141), rendered_image.clamp(0, 1) (:142)
 *        and image *= alpha_mask (train_single.py:102-104), with the loss of train_single.py:106-110 and the PSNR
 *        of utils/image_utils.py:17-19
 *   hlgs_mcmc_sample                        <- GaussianModel._sample_alives, scene/gaussian_model.py:1580-1586
 *        (torch.multinomial + bincount, on the CPU with host storage), with the sigmoid probabilities of its callers
 *        relocate_gs (:1614) and add_new_gs (:1714)
 *   hlgs_mcmc_noise                         <- the position noise of train_post.py:868-878 (op_sigmoid,
 *        build_scaling_rotation of utils/general_utils.py:82-114, randn_like, bmm)
 *   hlgs_rng_fill, hlgs_rng_uniform_host    <- the torch generator behind torch.multinomial / torch.randn_like there
 *
 * The alt rasterizer (submodules/alt-rasterizer: RasterizeGaussiansCUDA rasterize_points.cu:44-137 and
 * RasterizeGaussiansBackwardCUDA :138-232) goes through the same rasterizer entry points with
 * variant = HLGS_VARIANT_ALT (see hlgs_raster_args).
 *
 * Conventions: all pointers are device pointers unless a parameter says "host"; float = IEEE fp32,
 * int = int32; every array is dense and contiguous in the reference's layout (means (P,3), rotations
 * (P,4) as [r,x,y,z], shs (P,M,3), view/proj 16 floats, color (3,H,W)).  Nothing is allocated inside
 * the library: the caller passes buffers sized by the *_size() queries.  Work is launched on `stream`
 * (a hipStream_t; NULL = legacy default stream).  Functions return HLGS_OK or an error code;
 * hlgs_last_error() returns the message for the calling thread.
 */
#ifndef HLGS_H
#define HLGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HLGS_OK 0
#define HLGS_ERR_ARG 1
#define HLGS_ERR_DEVICE 2

/* Rasterizer variants (hlgs_raster_args.variant). */
#define HLGS_VARIANT_HIERARCHY 0 /* submodules/hierarchy-rasterizer (diff_gaussian_rasterization) */
#define HLGS_VARIANT_ALT 1       /* submodules/alt-rasterizer (alt_gaussian_rasterization): SH split into dc +
                                    rest, optional antialiasing, eigen-radius tile rect with exact per-tile
                                    culling (rasterizer_impl.cu:52-191), background rendered when nothing is
                                    binned, inverse depth always, and its backward (backward.cu:452-624) */

/* Arguments of one rasterizer call: the tensors RasterizeGaussiansCUDA receives. */
typedef struct hlgs_raster_args {
    int P;            /* Gaussians rasterised: indices.size(0) if non-empty, else means3D rows */
    int P_full;       /* means3D rows (gradients are P_full-sized, rasterize_points.cu:171) */
    int D;            /* active SH degree */
    int M;            /* SH coefficients per Gaussian (sh.size(1)), 0 when colors_precomp is used */
    int W, H;
    const float* bg;             /* 3 */
    const float* means3D;        /* P_full x 3 */
    const float* shs;            /* P_full x M x 3, or NULL */
    const float* colors_precomp; /* P x 3, or NULL */
    const float* opacities;      /* P_full */
    const float* scales;         /* P_full x 3 (activated), or NULL with cov3D_precomp */
    const float* rotations;      /* P_full x 4, or NULL with cov3D_precomp */
    const float* cov3D_precomp;  /* P x 6, or NULL */
    const float* viewmatrix;     /* 16 */
    const float* projmatrix;     /* 16 */
    const float* campos;         /* 3 */
    float scale_modifier, tanfovx, tanfovy;
    const int* indices;          /* in-kernel hierarchy mode (all four non-NULL) or NULL */
    const int* parent_indices;
    const float* ts;
    const int* kids;
    int prefiltered;
    int debug;                   /* synchronise + check after every stage (auxiliary.h:23-30) */
    const float* dc;             /* HLGS_VARIANT_ALT: P x 3 degree-0 SH coefficient; shs then holds the M
                                    higher-order ones (P x M x 3).  NULL otherwise. */
    int antialiasing;            /* EWA opacity compensation; the hierarchy rasterizer always applies it */
    int variant;                 /* HLGS_VARIANT_* */
} hlgs_raster_args;

/* Gradient outputs, all P_full rows; written completely by hlgs_rasterize_backward (no pre-zeroing). */
typedef struct hlgs_grads {
    float* dmean2D;   /* P_full x 3 (z stays 0) */
    float* dcolor;    /* P_full x 3 */
    float* dopacity;  /* P_full */
    float* dmean3D;   /* P_full x 3 */
    float* dcov3D;    /* P_full x 6, or NULL: not written (a caller without cov3D_precomp has nothing to return it for) */
    float* dsh;       /* P_full x M x 3 (may be NULL when M == 0) */
    float* dscale;    /* P_full x 3 */
    float* drot;      /* P_full x 4 */
    float* ddc;       /* HLGS_VARIANT_ALT: P_full x 3, else NULL */
    float* drgb;      /* NULL, or P_full x 3: the colour-factored SH gradient (hlgs_sh_grad_from_colour) -- the SH
                         backward then writes dL/dRGB with the clamp mask applied (zero rows for Gaussians it skips)
                         here instead of dsh / ddc, and still adds its view-direction term to dmean3D */
} hlgs_grads;

const char* hlgs_last_error(void);
const char* hlgs_version(void);

/* ---- rasterizer buffer sizing (bytes) ---- */
size_t hlgs_geom_buffer_size(int P);
size_t hlgs_image_buffer_size(int W, int H);
size_t hlgs_binning_buffer_size(int R);
size_t hlgs_backward_scratch_size(int P, int R);

/* Host-side result of phase 1. */
typedef struct hlgs_frame_info {
    int num_rendered;    /* the reference's num_rendered: Gaussian/tile instances over every tile rect (the alt
                            variant counts its culled instances too); sizes hlgs_backward_scratch_size */
    int max_tile_count;  /* longest per-tile list (selects the binning plan) */
    int rendered;        /* hlgs_rasterize_forward: 1 when phase 2 ran inside the call */
    int num_binned;      /* instances actually binned into the per-tile lists (== num_rendered for the
                            hierarchy rasterizer); sizes hlgs_binning_buffer_size */
    int entry_shift;     /* this frame's point_list entries are (index << entry_shift) | quadrant mask (0: plain
                            indices); the switches are read once when the frame starts (hlgs_set_entry_packing) */
    int drops_empty;     /* 1 if this frame's lists drop the instances whose quadrant mask is 0 (hlgs_set_drop_empty);
                            _prepare sets both and _render runs with them */
} hlgs_frame_info;

/* Phase 1: preprocess + scans.  Writes radii (P), fills geom/img and *info (host).  One host
 * synchronisation, as the reference has (rasterizer_impl.cu:330-331). */
int hlgs_rasterize_forward_prepare(const hlgs_raster_args* a, void* geom, void* img, int* radii,
                                   hlgs_frame_info* info, void* stream);
/* Phase 2: binning (per-tile depth sort) + front-to-back blend.  Every pixel of out_color (3,H,W) and
 * out_invdepth (H,W, or NULL when do_depth is off) is written; seen (P, or NULL for the alt variant) must
 * be zero-initialised by the caller.  With nothing binned this is a no-op for the hierarchy rasterizer
 * (the caller's zeroed output stays 0, not bg: rasterizer_impl.cu:332-333); the alt variant renders bg. */
int hlgs_rasterize_forward_render(const hlgs_raster_args* a, const int* radii, void* geom, void* img,
                                  void* binning, const hlgs_frame_info* info, float* out_color,
                                  float* out_invdepth, int* seen, void* stream);
/* Both phases in one call, with one host synchronisation and no return to the caller between them:
 * prepare, then -- when hlgs_binning_buffer_size(num_rendered) <= binning_bytes -- render into
 * `binning` and set info->rendered = 1.  Otherwise info->rendered = 0 and the caller allocates a
 * binning buffer of the reported size and calls hlgs_rasterize_forward_render.  seen is cleared here;
 * out_color / out_invdepth need no initialisation (with R == 0 they are set to 0).
 * Replaces the forward of RasterizeGaussiansCUDA (rasterize_points.cu:36-139). */
int hlgs_rasterize_forward(const hlgs_raster_args* a, void* geom, void* img, int* radii, void* binning,
                           size_t binning_bytes, hlgs_frame_info* info, float* out_color, float* out_invdepth,
                           int* seen, void* stream);
/* Backward: blend backward (per-tile partial sums, no float atomics) + fused covariance / SH / scale-
 * rotation backward.  dL_dinvdepth may be NULL (rasterize_points.cu:195-201).  R = info.num_rendered. */
int hlgs_rasterize_backward(const hlgs_raster_args* a, const int* radii, const void* geom, const void* img,
                            const void* binning, int R, void* scratch, const float* dL_dcolor,
                            const float* dL_dinvdepth, const hlgs_grads* out, void* stream);
/* hlgs_rasterize_backward with the kernels after the covariance backward (the SH backward, which completes dmean3D,
 * dsh and ddc, and the hierarchy-mode parent mean add) launched on late_stream behind an event on stream, and NOT
 * joined back: dopacity, dscale, drot, dcov3D, dmean2D and dcolor are final in stream order, dmean3D / dsh / ddc in
 * late_stream order.  The caller joins (waits on late_stream) before reading those three.  A view-data-parallel
 * exchange uses it to start the collective over the early gradients while the SH backward runs.
 * late_stream = NULL is hlgs_rasterize_backward. */
int hlgs_rasterize_backward_split(const hlgs_raster_args* a, const int* radii, const void* geom, const void* img,
                                  const void* binning, int R, void* scratch, const float* dL_dcolor,
                                  const float* dL_dinvdepth, const hlgs_grads* out, void* stream, void* late_stream);

/* The averaged SH gradient of a view-data-parallel step, rebuilt from each view's colour gradient.
 * One view's SH gradient is an outer product per Gaussian, dL/dsh[c] = basis_c(dir) * dL/dRGB with the clamp mask
 * applied (computeColorFromSH backward, backward.cu:23-142; alt-rasterizer backward.cu:23-146), so ranks exchange the
 * 3-float dL/dRGB rows (hlgs_grads.drgb) instead of the (D+1)^2 x 3 SH rows, and each rank forms
 *   dsh[p][c - OFF][ch] = scale * sum_v basis_c(normalize(mean_p - campos_v)) * drgb[v][p][ch]
 * in view order v = 0..V-1.  View v's campos (3 floats) and drgb (P x 3) start view_stride floats after view v-1's
 * (an exchange gathers them as one row per rank: [campos, pad | drgb]); means3D: P x 3 (device).  dsh: P x M x 3 holds
 * coefficients OFF..OFF+M-1 (OFF = 1 for HLGS_VARIANT_ALT, whose coefficient 0 goes to ddc: P x 3; OFF = 0 and ddc
 * NULL otherwise); coefficients at or above (D+1)^2 are zero. */
int hlgs_sh_grad_from_colour(int P, int V, int D, int M, int variant, const float* means3D, const float* campos,
                             const float* drgb, int64_t view_stride, float scale, float* dsh, float* ddc, void* stream);

/* z > 0.2 visibility (auxiliary.h:164-189); present is P bytes (bool) */
int hlgs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present, void* stream);
/* MCMC relocation, utils.cu:6-36.  scale_new is 3P floats. */
int hlgs_compute_relocation(int P, const float* opacity_old, const float* scale_old, const int* N,
                            const float* binoms, int n_max, float* opacity_new, float* scale_new, void* stream);

/* ---- MCMC densification (train_post.py:70-75, 707-789, 868-878) ---- */
/* Counter-based random numbers (Philox4x32-10): number `index` of (seed, stream) depends on those three values only --
 * no state, no dependence on the launch, the same on every rank.  counter = (index low, index high, stream, 0), key =
 * (seed low, seed high); of the four output words w0..w3
 *   HLGS_RNG_UNIFORM64: double u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 in [0, 1);
 *   HLGS_RNG_NORMAL32:  float  z = sqrtf(-2 logf(u1)) cosf(2 pi u2), u1 = ((w2 >> 8) + 1) 2^-24 in (0, 1],
 *                       u2 = (w3 >> 8) 2^-24 (Box-Muller, cosine branch).
 * hlgs_rng_fill writes numbers first_index .. first_index + n - 1 to out (device: n doubles or n floats);
 * hlgs_rng_uniform_host writes the same uniforms to host memory and needs no device. */
#define HLGS_RNG_UNIFORM64 0
#define HLGS_RNG_NORMAL32 1
int hlgs_rng_uniform_host(uint64_t seed, uint32_t stream, uint64_t first_index, int64_t n, double* out_host);
int hlgs_rng_fill(int kind, uint64_t seed, uint32_t stream, uint64_t first_index, int64_t n, void* out, void* hip_stream);
/* Opacity-weighted sampling with replacement.  Candidate i < n is storage row alive[i] (alive == NULL: row i) and
 * weighs w_i = 1 / (1 + exp(-x_i)) in float64, x_i the float32 logit at opacity_base + alive[i] * stride_bytes
 * (device memory or pinned host memory: the opacity word of packed host rows is read in place); logits below -103,
 * where float32's sigmoid underflows, weigh exactly 0.  C = the inclusive prefix sum of w, accumulated in float64 in a
 * fixed order.  Draw j < num takes uniform number j of (seed, stream_id) and selects the smallest i with
 * C_i > u_j C_n, so a zero weight is never drawn; sampled[j] = alive[i] and counts (size int32, zeroed here) =
 * bincount(sampled, minlength = size).  The reference's division by sum + eps (:1581) does not change the
 * distribution and is not reproduced, and there is no 16,000,000-candidate subsampling (:1611-1613, :1709-1711).
 * Bit-identical from run to run.  scratch: hlgs_mcmc_sample_scratch_size(n) bytes of device memory; its first
 * 256-byte-aligned address holds HLGS_MCMC_HEADER_BYTES: double C_n, int32 status (bit 0: n == 0 or C_n is 0 or not
 * finite -- nothing was drawn, sampled is -1; bit 1: a drawn row fell outside [0, size)), which the caller reads
 * after the call (no host synchronisation here).  Rows alive[i] must lie inside the opacity storage. */
#define HLGS_MCMC_HEADER_BYTES 16
size_t hlgs_mcmc_sample_scratch_size(int64_t n);
int hlgs_mcmc_sample(int64_t n, const void* opacity_base, int64_t stride_bytes, const int* alive, int64_t num,
                     uint64_t seed, uint32_t stream_id, int* sampled, int* counts, int64_t size, void* scratch,
                     void* hip_stream);
/* The position noise of train_post.py:868-878 over rows first_row <= p < P, in place, one pass:
 *   o = sigmoid(opacity_raw), s = exp(scaling_raw), q = normalize(rotation_raw) (normalised again as build_rotation
 *   does), L = R(q) diag(s), w = 1 / (1 + exp(-100 ((1 - o) - 0.995))), means3D += L L^T (xi w scale),
 * scale = MCMC_Noise_LR * xyz_lr; a row's arithmetic runs in float64 from the float32 inputs and the increment is
 * rounded to float32 once.  xi = noise[3 p + c] (P x 3 floats) when noise is given, else normal number
 * 3 p + c of (seed, stream = step).  The reference runs it after the optimizer step, on the updated parameters. */
int hlgs_mcmc_noise(int64_t P, int64_t first_row, float* means3D, const float* opacity_raw, const float* scaling_raw,
                    const float* rotation_raw, const float* noise, double scale, uint64_t seed, uint32_t step,
                    void* hip_stream);

/* Sparse Adam step of SparseGaussianAdam (alt_gaussian_rasterization/__init__.py:244-271, adam.cu:9-36):
 * for every element p of the N x M parameter whose Gaussian p / M is visible (visible: N bytes),
 * m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, param -= lr m / (sqrt(v) + eps).  No bias correction and
 * no step counter, as the reference. */
int hlgs_adam_update(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const uint8_t* visible,
                     float lr, float b1, float b2, float eps, uint32_t N, uint32_t M, void* stream);

/* ---- adaptive density control of chunk training (train_single.py:144-155; scene/gaussian_model.py:1214-1218,
 *      1249-1345, 1348-1531) ----
 * The reference's own methods cannot be called (add_densification_stats is given two of its three arguments, densify*
 * reads self.nodes, the prune is commented out), so the arithmetic of the cited lines is the contract.  All arrays are
 * float32 device memory unless noted; P rows; rows below protect_rows (the skybox / scaffold prefix) are never
 * selected, pruned or reset.  Nothing here allocates or keeps state. */
/* add_densification_stats (train_single.py:147-148, gaussian_model.py:1527-1530), in place, for the rows with
 * radii > 0: max_radii2D = max(max_radii2D, (float)radii), grad_accum = max(grad_accum, sqrt(gx^2 + gy^2)) of
 * dL_dmean2D (P x 3; the fork's max, not upstream's sum), denom += 1.  Other rows keep their bits. */
int hlgs_density_stats(int64_t P, const float* dL_dmean2D, const int* radii, float* grad_accum, float* denom,
                       float* max_radii2D, void* stream);
/* The masks of densify / densify_and_prune (:1458-1468, :1508, :1512-1514), evaluated in float64 from the float32
 * inputs: o = sigmoid(opacity_raw), g = grad_accum with NaN as 0,
 *   select = g max_radii2D o^(1/5) >= grad_threshold && o > densify_min_opacity && leaf && row >= protect_rows
 *   prune  = o < prune_min_opacity && row >= protect_rows          (prune_min_opacity < 0: all zero)
 * leaf: P bytes or NULL (every row a leaf); select, prune: P bytes each. */
int hlgs_density_select(int64_t P, const float* grad_accum, const float* max_radii2D, const float* opacity_raw,
                        const uint8_t* leaf, double grad_threshold, double densify_min_opacity,
                        double prune_min_opacity, int64_t protect_rows, uint8_t* select, uint8_t* prune, void* stream);
/* The round's plan: in ascending row order the kept rows (not pruned, and not selected when drop_selected) and the
 * selected rows, left in scratch (hlgs_densify_scratch_size(P) bytes of device memory, 256-byte aligned) for
 * hlgs_densify_emit.  prune may be NULL.  counts_host[0] = n_kept, counts_host[1] = n_selected, read back here: the
 * round's only host synchronisation (the caller sizes the output tables from them); pass pinned memory. */
size_t hlgs_densify_scratch_size(int64_t P);
int hlgs_densify_plan(int64_t P, const uint8_t* select, const uint8_t* prune, int drop_selected, void* scratch,
                      int* counts_host, void* stream);
/* Every output table of the round in one launch (_prune_optimizer :1254-1258, :1279-1282; cat_tensors_to_optimizer
 * :1302-1306).  Output row d < n_kept is input row kept[d], bit for bit; output row n_kept + copies j + k is copy k of
 * parent selected[j] (repeat_interleave, :1473, behind torch.cat) -- the reference appends and then prunes, which is
 * the same table because a selected row (o > 0.15) is never pruned (o < 0.005) and a new row's opacity is at least
 * 0.15 / (0.8 copies).  A table's role says what its new rows hold:
 *   HLGS_DENSIFY_COPY     the parent's row, bit for bit (f_dc, f_rest, rotation)
 *   HLGS_DENSIFY_ZERO     zeros (both Adam moments of every parameter, :1302-1303; the statistics)
 *   HLGS_DENSIFY_XYZ      (3 floats)  split: R(q / |q|) (exp(s) * xi) + xyz (:1367-1371); else a copy
 *   HLGS_DENSIFY_SCALING  (3 floats)  shrink: log(exp(s) / (0.8 copies)) (:1474); split: log(exp(s) / (0.7 copies))
 *                                     (:1372); clone: a copy (the reference's log(exp(s)), :1421, is not reproduced)
 *   HLGS_DENSIFY_OPACITY  (1 float)   shrink: logit(sigmoid(x) / (0.8 copies)) (:1478); else a copy
 * A transformed value is computed in float64 from the float32 inputs and rounded once.  xi of new row r = copies j + k,
 * axis c: noise[3 r + c] when noise is given, else normal number 3 r + c of (seed, stream = round).  split needs the
 * XYZ and SCALING tables and rotation (P x 4, the raw quaternions).  At most 32 tables; a table with row_bytes == 0 is
 * skipped; row_bytes is a multiple of 4 and tables are 4-byte aligned (16-byte aligned destinations are written with
 * 16-byte stores).  n_kept and n_selected are the plan's counts; a launch given other counts writes nothing. */
#define HLGS_DENSIFY_CLONE 0
#define HLGS_DENSIFY_SHRINK 1
#define HLGS_DENSIFY_SPLIT 2
#define HLGS_DENSIFY_COPY 0
#define HLGS_DENSIFY_ZERO 1
#define HLGS_DENSIFY_XYZ 2
#define HLGS_DENSIFY_SCALING 3
#define HLGS_DENSIFY_OPACITY 4
typedef struct hlgs_densify_table {
    const void* src;   /* P rows */
    void* dst;         /* n_kept + copies n_selected rows */
    int64_t row_bytes;
    int role;
} hlgs_densify_table;
int hlgs_densify_emit(int T, const hlgs_densify_table* tables, int64_t P, int64_t n_kept, int64_t n_selected,
                      int copies, int mode, const float* rotation, const float* noise, uint64_t seed, uint32_t round,
                      void* scratch, void* stream);
/* reset_opacity (:1214-1218) with replace_tensor_to_optimizer's zeroed moments (:1237-1238), in place, one pass: rows
 * >= protect_rows with sigmoid(opacity_raw) > max_opacity (float64) take (float)logit(max_opacity), every other row
 * keeps its bits (the reference's inverse_sigmoid(sigmoid(x)) round trip destroys very negative logits and is not
 * reproduced); exp_avg and exp_avg_sq (either may be NULL) are zeroed for all rows. */
int hlgs_opacity_reset(int64_t P, int64_t protect_rows, double max_opacity, float* opacity_raw, float* exp_avg,
                       float* exp_avg_sq, void* stream);

/* ---- hierarchical LOD ---- */
size_t hlgs_lod_scratch_size(int N);
/* nodes: N x 6 int32 HierarchyNode rows; viewpoint: device float3; viewdir: host float[3].
 * Writes the first *count entries of render_indices / parent_indices / nodes_for_render_indices
 * (parent_indices is left untouched for roots, runtime_switching.cu:104-107). */
int hlgs_expand_to_size_dynamic(int N, float target_size, const int* nodes, const float* positions,
                                const float* scales, const float* viewpoint, const float* viewdir_host,
                                int* render_indices, int* parent_indices, int* nodes_for_render_indices,
                                void* scratch, int* count, void* stream);
/* viewpoint_host / viewdir_host: host float[3] (torch_interface.cpp:240-241) */
int hlgs_get_interpolation_weights_dynamic(int n, const int* node_indices, float target_size, const int* nodes,
                                           const float* positions, const float* scales,
                                           const float* viewpoint_host, const float* viewdir_host, float* ts,
                                           int* kids, void* stream);
/* static (.hier) variant: nodes N x 7 int32, boxes N x 8 float (minn xyzw, maxx xyzw) */
int hlgs_expand_to_size(int N, float target_size, const int* nodes, const float* boxes, const float* viewpoint,
                        const float* viewdir_host, int* render_indices, int* parent_indices,
                        int* nodes_for_render_indices, void* scratch, int* count, void* stream);
int hlgs_get_interpolation_weights(int n, const int* node_indices, float target_size, const int* nodes,
                                   const float* boxes, const float* viewpoint_host, const float* viewdir_host,
                                   float* ts, int* kids, void* stream);

/* SPT cut (runtime_switching.cu:878-994).  prepare() computes per-SPT candidate intervals into
 * scratch (hlgs_spt_scratch_size(s) bytes) and returns the candidate total in *n_candidates (host);
 * finish() needs work >= hlgs_spt_work_size(n_candidates) bytes and writes the kept Gaussian indices to
 * cut[0..*count) and the exclusive prefix of per-SPT kept counts to counts_prefix (s).  compat != 0
 * reproduces the reference bit for bit (App. A-10 boundary attribution + dropping index 0). */
size_t hlgs_spt_scratch_size(int s);
size_t hlgs_spt_work_size(int n_candidates);
int hlgs_spt_cut_prepare(int s, const int* SPT_starts, const float* SPT_max, const int* SPT_indices,
                         const float* SPT_distances, void* scratch, int* n_candidates, void* stream);
int hlgs_spt_cut_finish(int s, int E, int n_candidates, const int* gaussian_indices, const int* SPT_starts,
                        const float* SPT_min, const int* SPT_indices, const float* SPT_distances, int compat,
                        void* scratch, void* work, int* cut, int* counts_prefix, int* count, void* stream);

/* LOD interpolation (render_post lerp).  M3 = floats of SH per Gaussian (0: no SH).  Outputs have
 * S + n rows: rows [0,S) copy the skybox prefix, row S+i lerps child ridx[i] with parent pidx[i]. */
int hlgs_lod_interp_forward(int S, int n, int M3, const int* ridx, const int* pidx, const float* w,
                            const float* means, const float* scales, const float* rots, const float* opac,
                            const float* shs, float* o_means, float* o_scales, float* o_rots, float* o_opac,
                            float* o_shs, void* stream);
/* Gradient of the lerp (the autograd of render_post's block, gaussian_renderer/__init__.py:304-339) into the
 * P-row gradient arrays d_*: every row is written (zeros where no output row depends on it), so no
 * initialisation is needed; contributions are gathered per node in a fixed order (bitwise deterministic).
 * scratch: hlgs_lod_interp_scratch_size(P, n) bytes.  M3 <= 64. */
size_t hlgs_lod_interp_scratch_size(int P, int n);
int hlgs_lod_interp_backward(int P, int S, int n, int M3, const int* ridx, const int* pidx, const float* w,
                             const float* rots, const float* g_means, const float* g_scales, const float* g_rots,
                             const float* g_opac, const float* g_shs, float* d_means, float* d_scales,
                             float* d_rots, float* d_opac, float* d_shs, void* scratch, void* stream);

/* Morton codes of P positions in the [mn, mx] box (device float3 each): get_morton_indices,
 * gaussianhierarchy/morton.cu:9-58 via torch_interface.cpp:246-260 (used by GaussianModel.sort_morton,
 * scene/gaussian_model.py:570-589). */
int hlgs_morton_codes(int P, const float* xyz, const float* mn, const float* mx, int64_t* codes, void* stream);

/* Mean squared distance to the three nearest other points: simple_knn._C.distCUDA2, imported by
 * scene/gaussian_model.py:21 and used at :848 (create_from_pcd), where the initial scale of every Gaussian is
 * log(sqrt(clamp_min(distCUDA2(xyz), 1e-7))).  xyz: P x 3 device floats; out: P device floats.  For each point i the
 * squared distances d(i, j) = (dx*dx + dy*dy) + dz*dz to all other indices j are taken in float32, every operation
 * rounded on its own (no fma, no |a|^2 + |b|^2 - 2 a.b form); with b0 <= b1 <= b2 the three smallest,
 * out[i] = ((b0 + b1) + b2) / 3.0f.  Coincident points are ordinary neighbours at distance 0.  A missing neighbour
 * (P < 4) counts as +inf, so every output is +inf then.  The result equals the all-pairs scan bit for bit and does not
 * change from run to run.  P == 0 launches nothing.  No host synchronisation; every memory index stays in range for
 * any input bits (outputs of rows with non-finite coordinates are unspecified).
 * scratch: hlgs_knn_scratch_size(P) bytes of device memory, 16-byte aligned.
 * The search works on boxes of HLGS_KNN_BOX Morton-sorted points grouped into super-boxes of HLGS_KNN_SUPER boxes;
 * the radix sort handles HLGS_KNN_SORT_TILE keys per block. */
#define HLGS_KNN_BOX 64
#define HLGS_KNN_SUPER 64
#define HLGS_KNN_SORT_TILE 1024
size_t hlgs_knn_scratch_size(int P);
int hlgs_knn_mean_dist2(int P, const float* xyz, void* scratch, float* out, void* stream);

/* ---- The dynamic hierarchy of N flat Gaussians (the offline GaussianHierarchyCreator, on the device) ----
 * Inputs are activated Gaussians as submodules/gaussianhierarchy/loader.cpp:54-72 leaves them, device float32:
 * xyz N x 3, shs N x sh_floats (any order; rows are only copied and blended), opacity N in (0, 1], scales N x 3
 * (exp of the stored ones), rotations N x 4 (w, x, y, z; normalised inside as loader.cpp:56 does).  N in
 * [1, HLGS_HIER_MAX_N] (2N - 1 node ids are int32) and sh_floats >= 1, else HLGS_ERR_ARG.  Nothing is allocated and
 * nothing is read back; every launch goes to `stream`.
 *
 * hlgs_hier_valid_mask: mask[i] = 1 iff the creator keeps row i (mainHierarchyCreator.cpp:87-152): opacity neither
 *   inf, NaN nor 0, no scale above 10, no NaN in scale, rotation, position or SH.
 *
 * hlgs_hier_build writes the 2N - 1 pre-order rows (row id == node id) of
 *   PointbasedKdTreeGenerator.cpp:16-68  bounds over position -+ 3 max(scale), the first axis of the strictly greatest
 *       extent, the num / 2 members of smallest position[axis] to the left; ties (which nth_element leaves open) by
 *       (position[axis] compared as floats, input row);
 *   ClusterMerger.cpp:23-141  bottom-up, float32 in the reference's order: w_i = opacity_i ((s0 s1 + s0 s2) + s1 s2),
 *       a_i = w_i / (w0 + w1), position and SH row 0 + a0 x0 + a1 x1, cov = sum a_i (cov_i + d_i d_i^T) over the
 *       children's accumulated covariances; eigenvalues ascending (3 x 3 cyclic Jacobi in float64), diagonal bumped by
 *       max(1e-4 m_ii, FLT_EPSILON) while one is exactly 0 (at most 16 times), third eigenvector negated in a
 *       left-handed frame, scale = sqrt|lambda|, rotation = Eigen's quaternion of the eigenvectors, opacity =
 *       (w0 + w1) / surface(scale), not clamped; the root is merged too;
 *   rotation_aligner.cpp:23-115  top-down: every child takes the first of its 24 proper signed axis permutations, in
 *       the loop order (i, j, k, state), whose Frobenius product with the parent's rotation is strictly the greatest
 *       above 0, and its scales are permuted alike; a child with no such candidate is left unchanged;
 *   writer.cpp:99-204  nodes (2N - 1) x 6 int32 {depth, parent (-1 for the root), child_count (2 or 0), first_child
 *       (id + 1 for every node), next_sibling (the right sibling's id for a left child, else 0), max_side_length (the
 *       input row of a leaf, -1 for merged nodes)}; log_scales = log(scale); alpha as is.
 * pos (2N-1) x 3, shs (2N-1) x sh_floats, alpha 2N-1, log_scales (2N-1) x 3, rot (2N-1) x 4 device float32.
 * Results do not change from run to run.  Every memory index stays in range for any input bits.
 * scratch: hlgs_hier_scratch_size(N) bytes of device memory, 256-byte aligned.  Its first word is the status, valid
 * once the stream has passed the call: the caller reads it (the build's one read-back) and treats a non-zero value as
 * an error: HLGS_HIER_STATUS_INVALID a row holds a non-finite value or has opacity 0; _NAN an eigenvalue was NaN (the
 * reference throws); _BUMP an eigenvalue was still 0 after 16 bumps (the reference would go on).
 * A subtree of at most HLGS_HIER_LDS_CAP leaves is finished by one workgroup (its kd levels in LDS, its merge and
 * alignment levels behind barriers); the levels above are one group of launches each.
 * stages: HLGS_HIER_ALL.  For measurement the stages can be run one call each, in order (bit 0 kd top levels, 1 kd in
 * LDS, 2 leaf rows and node table, 3 merge, 4 align, 5 log of the scales); the state between them is in scratch and
 * the outputs. */
#define HLGS_HIER_LDS_CAP 2048
#define HLGS_HIER_MAX_N (1 << 30)
#define HLGS_HIER_ALL 0x3f
#define HLGS_HIER_STATUS_INVALID 1u
#define HLGS_HIER_STATUS_NAN 2u
#define HLGS_HIER_STATUS_BUMP 4u
size_t hlgs_hier_scratch_size(int N);
int hlgs_hier_valid_mask(int N, int sh_floats, const float* xyz, const float* shs, const float* opacity,
                         const float* scales, const float* rotations, unsigned char* mask, void* stream);
int hlgs_hier_build(int N, int sh_floats, const float* xyz, const float* shs, const float* opacity,
                    const float* scales, const float* rotations, float* pos, float* out_shs, float* alpha,
                    float* log_scales, float* rot, int* nodes, void* scratch, int stages, void* stream);

/* ---- Trained chunk hierarchies merged into one scene hierarchy (the offline GaussianHierarchyMerger, on the device) ----
 * K chunk hierarchies in the dynamic layout, as train_post.py saves them (save_hier, scene/gaussian_model.py:1115-1124),
 * and their K chunk centres (center.txt) become one dynamic hierarchy: submodules/gaussianhierarchy
 * hierarchy_explicit_loader.cpp:22-150, mainHierarchyMerger.cpp:94-140 and writer.cpp:99-171, carried over to rows of
 * one Gaussian per node.  Chunk k is n rows of device float32 pos n x 3, shs n x sh_floats, alpha n (activated),
 * log_scales n x 3, rot n x 4 and nodes n x 6 int32 {depth, parent, child_count, first_child, next_sibling,
 * max_side_length}, without skybox rows.  Row 0 is the chunk's root; the other rows are in any order, linked by parent,
 * child_count, first_child and next_sibling (the MCMC round appends and rewires rows, scene/gaussian_model.py
 * :1743-1765); any child count is allowed (the output of a merge is a legal input); first_child of a row with
 * child_count 0 is not read.  centers: K x 3 device float32.
 *
 *   weight (getWeight, hierarchy_explicit_loader.cpp:22-53), float32, every operation rounded on its own: the
 *       position of row 0 is centers[k] (:147); d_j = sqrtf((dx dx + dy dy) + dz dz) to centre j; m = the smallest d_j,
 *       j != k, starting from 1e12f (`if (d < m)`); w = 1 if d_k <= (1.0f - f) m, else 0 if d_k > (1.0f + f) m, else
 *       a d_k + b with a = -1.0f / ((2.0f f) m), b = (1.0f + f) / (2.0f f); f = falloff (0.05 in the reference).
 *       A NaN position gives a NaN weight.
 *   keep  a node iff w > 0 (:106-110).  Its opacity becomes alpha w (one multiply); every other float of the row is
 *       copied bit for bit, the log-scales included: the reference's exp on load and log on write (:84,
 *       writer.cpp:119) is not reproduced.
 *   splice (:112-131)  the children of a dropped node take its place, in order, in the child list of its nearest kept
 *       ancestor.  A kept interior node whose descendants are all dropped stays, with child_count 0.
 *   rows (populateDynamicRec, writer.cpp:99-171)  pre-order, row id == node id, the chunk under the scene root:
 *       depth = 1 + the number of kept proper ancestors; parent = the nearest kept ancestor's id, 0 for the chunk
 *       root; child_count = the spliced children; first_child = id + 1 for every node; next_sibling = the id of the
 *       next child of the same parent, 0 for the last; max_side_length = for a kept node with child_count 0 in its
 *       input, its rank among all such nodes of the output (chunk order, then pre-order: the index into the merged
 *       `gaussians` vector, writer.cpp:123), -1 for every other node.
 *   join (mainHierarchyMerger.cpp:107-136)  row 0 is a new root: depth 0, parent -1, child_count K, first_child 1,
 *       next_sibling 0, max_side_length -1; the chunk roots follow in chunk order, chained by next_sibling.  With a_k
 *       the chunk roots' output opacities: position = sum a_k c_k / max(sum a_k, 1e-12) and SH = the mean of the chunk
 *       roots' SH rows, both summed in chunk order in float64 and rounded once; alpha = max a_k; log-scales =
 *       (float)log((double)root_scale), so that no cut selects it (bounds[3] = 1e9 in the reference); rotation
 *       (1, 0, 0, 0).
 *
 * hlgs_hier_merge_plan (per chunk) validates the links and computes the weights.  scratch: hlgs_hier_merge_scratch_size(n)
 *   bytes of device memory, 256-byte aligned, one per chunk, kept until the chunk's emit has run.  Its first
 *   HLGS_MERGE_HEADER_INTS + HLGS_MERGE_MAX_DEPTH + 1 int32 words are the plan's result, valid once the stream has
 *   passed the call, and the merge's one read-back per chunk: {status, kept nodes, kept input-leaves, 5 x reserved},
 *   then the number of rows at every depth.  status: HLGS_MERGE_STATUS_LINKS the node table is malformed;
 *   HLGS_MERGE_STATUS_ROOT the chunk's root is dropped (a non-finite centre).  The caller treats a non-zero status as
 *   an error.  Validation, by the first kernel and before anything follows a link: depth in [0, HLGS_MERGE_MAX_DEPTH],
 *   child_count in [0, n); for every row but row 0, parent in [0, n), not itself, and depth = the parent's + 1; every
 *   child list walked for child_count members, each in [1, n) and naming that parent; every row but row 0 a member of
 *   exactly one list, row 0 of none.  (Together: the rows form one tree under row 0.)
 * hlgs_hier_merge_emit (per chunk, after the read-back) writes the chunk's kept rows at out_offset .. out_offset + kept
 *   of the outputs (G rows each, 16-byte aligned): kept and level_counts (host, HLGS_MERGE_MAX_DEPTH + 1 entries) as
 *   read back; out_offset = 1 + the kept nodes of the chunks before it; leaf_offset = their kept input-leaves; K the
 *   number of chunks (next_sibling of the last chunk's root is 0).  With a non-zero status in scratch its kernels do
 *   nothing.
 * hlgs_hier_merge_root writes row 0 from the K chunk-root rows chunk_roots[k] (device int32) of the outputs.
 *
 * n in [1, HLGS_MERGE_MAX_N], sh_floats >= 1, else HLGS_ERR_ARG.  Nothing is allocated; every launch goes to `stream`;
 * no host synchronisation.  The tree passes are one launch per depth (data crosses workgroups at launch boundaries
 * only); a child list is walked by one thread.  Results do not change from run to run (no float atomics; integer
 * atomics only where their order does not matter).  Every memory index stays in range for any input bits.
 * stages: HLGS_MERGE_PLAN_ALL / HLGS_MERGE_EMIT_ALL.  For measurement the stages can be run one call each, in order
 * (plan: bit 0 validate, 1 weights; emit: bit 0 depth buckets and bottom-up counts, 1 top-down ids, 2 rows). */
#define HLGS_MERGE_MAX_DEPTH 2047
#define HLGS_MERGE_MAX_N (1 << 30)
#define HLGS_MERGE_HEADER_INTS 8
#define HLGS_MERGE_PLAN_ALL 0x3
#define HLGS_MERGE_EMIT_ALL 0x7
#define HLGS_MERGE_STATUS_LINKS 1u
#define HLGS_MERGE_STATUS_ROOT 2u
size_t hlgs_hier_merge_scratch_size(int n);
int hlgs_hier_merge_plan(int n, int k, int K, const float* centers, const float* pos, const int* nodes, float falloff,
                         void* scratch, int stages, void* stream);
int hlgs_hier_merge_emit(int n, int sh_floats, int k, int K, const float* centers, const float* pos, const float* shs,
                         const float* alpha, const float* log_scales, const float* rot, const int* nodes,
                         const int* level_counts, int kept, int out_offset, int leaf_offset, int G, float* out_pos,
                         float* out_shs, float* out_alpha, float* out_log_scales, float* out_rot, int* out_nodes,
                         void* scratch, int stages, void* stream);
int hlgs_hier_merge_root(int K, int sh_floats, int G, const int* chunk_roots, const float* centers, float root_scale,
                         float* out_pos, float* out_shs, float* out_alpha, float* out_log_scales, float* out_rot,
                         int* out_nodes, void* stream);

/* ---- SPT streaming around the SPT cut (train_post.py:323-491) ---- */
/* Coarse cut of the upper tree (GaussianModel.cut_hierarchy_on_condition with root 0, no upper-tree output,
 * leave_out_of_cut_condition = frustum_cull_spheres: scene/gaussian_model.py:364-404, 67-100, as train_post.py
 * :326-343 calls it).  nodes: N x 6 int32 upper-tree HierarchyNode rows; xyz N x 3; bounds N (sphere radii);
 * min_dist2 N; planes: 4 x 4 floats (nx, ny, nz, d) from extract_frustum_planes; campos 3.  A node survives the
 * cull unless n.p + d + r < 0 for one plane (use_frustum); it is cut if it is a leaf or (use_lod) if not
 * min_dist2 > |campos - p|^2 * distance_multiplier, else its first child and that child's next sibling are
 * visited.  cut (device, N entries) receives the nodes in the reference's order; *count (host) their number.
 * scratch: hlgs_upper_cut_scratch_size(N) bytes.  One host synchronisation (the reference's len()). */
size_t hlgs_upper_cut_scratch_size(int N);
/* The same cut without the host read: the count and an overflow flag land in count_device[0..1] (device memory),
 * for hlgs_spt_cache_plan's n_cut_device, which reads them in its own single host synchronisation. */
int hlgs_upper_tree_cut_device(int N, const int* nodes, const float* xyz, const float* bounds, const float* min_dist2,
                               const float* planes, const float* campos, float distance_multiplier, int use_frustum,
                               int use_lod, void* scratch, int* cut, int* count_device, void* stream);
int hlgs_upper_tree_cut(int N, const int* nodes, const float* xyz, const float* bounds, const float* min_dist2,
                        const float* planes, const float* campos, float distance_multiplier, int use_frustum,
                        int use_lod, void* scratch, int* cut, int* count, void* stream);
/* The cut for a batch of n_views training views (one per rank of a view-data-parallel step): planes
 * n_views x 4 x 4, campos n_views x 3.  A node survives the cull if its sphere reaches into ANY view's frustum, and
 * expands if min_dist2 > min over views |campos_g - p|^2 * distance_multiplier (the nearest camera decides).  With
 * n_views = 1 this is hlgs_upper_tree_cut_device, bit for bit.  Every rank computing it from the same gathered views
 * obtains the same cut (no train_post.py counterpart: the reference trains one view per step). */
int hlgs_upper_tree_cut_views_device(int N, const int* nodes, const float* xyz, const float* bounds,
                                     const float* min_dist2, int n_views, const float* planes, const float* campos,
                                     float distance_multiplier, int use_frustum, int use_lod, void* scratch, int* cut,
                                     int* count_device, void* stream);
/* The same cut from a precomputed walk order (round 5): two launches (every node's state in parallel, then one
 * workgroup that places the surviving nodes) instead of one per level, with the result of
 * hlgs_upper_tree_cut_views_device bit for bit.  order (device): the blob hlgs_upper_tree_order wrote for these
 * nodes, or NULL for the level walk.  Same scratch. */
int hlgs_upper_tree_cut_views_ordered_device(int N, const int* nodes, const void* order, const float* xyz,
                                             const float* bounds, const float* min_dist2, int n_views,
                                             const float* planes, const float* campos, float distance_multiplier,
                                             int use_frustum, int use_lod, void* scratch, int* cut, int* count_device,
                                             void* stream);
/* Host: the walk order of an upper tree (nodes: N x 6 HierarchyNode rows, host memory) into order_host
 * (hlgs_upper_tree_order_size(N) bytes).  Word 3 holds N: the flat cut refuses (count_device[1] = 1) a blob built for
 * another node count.  Word 2 of the blob is 1 when the flat cut can use it: the nodes form a
 * tree as the reference walks it (root 0; first child, then that child's next sibling) with at most 65,535 nodes
 * on it over at most 64 levels; otherwise use the level walk (order = NULL above). */
#define HLGS_CUT_ORDER_HEADER 80       /* words before the per-entry arrays of the order blob */
#define HLGS_CUT_FLAT_MAX_ENTRIES 65535
#define HLGS_CUT_FLAT_MAX_LEVELS 64
size_t hlgs_upper_tree_order_size(int N);
int hlgs_upper_tree_order(int N, const int* nodes_host, void* order_host);
/* SPT construction (GaussianModel.build_hierarchical_SPT + get_min_distance, scene/gaussian_model.py:184-352), host
 * code over host arrays: nodes G x 6 (HierarchyNode), xyz G x 3, log_scales G x 3 (unactivated, as _scaling);
 * root = the hierarchy root (the reference's default root_node 100000 is its skybox size).  The result is an
 * opaque handle: query the sizes, copy into caller buffers (any pointer may be NULL), free.
 *   starts (n_spt + 1), smax / smin / gidx (n_entries): the SPT arrays get_spt_cut_cuda takes;
 *   roots (n_spt): hierarchy ids of the SPT roots; up_nodes (n_upper x 6), up_xyz, up_scaling (n_upper x 3),
 *   min_d2, radii (n_upper): the upper tree (radii only with use_bounding_spheres). */
typedef struct hlgs_spt_result hlgs_spt_result;
int hlgs_spt_build(int G, const int* nodes, const float* xyz, const float* log_scales, int root, float spt_root_volume,
                   float target_granularity, int min_spt_size, int use_bounding_spheres, hlgs_spt_result** out);
int hlgs_spt_result_sizes(const hlgs_spt_result* r, int* n_spt, int* n_entries, int* n_upper);
int hlgs_spt_result_copy(const hlgs_spt_result* r, int* starts, float* smax, float* smin, int* gidx, int* roots,
                         int* up_nodes, float* up_xyz, float* up_scaling, float* min_d2, float* radii);
void hlgs_spt_result_free(hlgs_spt_result* r);
/* The same construction (GaussianModel.build_hierarchical_SPT + get_min_distance, scene/gaussian_model.py:184-345) on
 * the GPU, in two phases around the sizes, which are known only once the walks have ended.
 * hlgs_spt_device_scratch_size(G): bytes of device scratch (256-byte aligned) both calls take, a function of G alone.
 * hlgs_spt_build_device (scene/gaussian_model.py:184-345): nodes G x 6 int32 in device memory; xyz and log_scales rows
 *   of 3 floats every xyz_stride / scale_stride floats (>= 3), in device memory or pinned host memory (the strided
 *   views of a packed host table are read in place and packed into scratch in one pass).  Links are validated before
 *   any is followed (first_child >= G anywhere; next_sibling >= G on a row that is some node's first child); a link
 *   out of range, a node reached twice (a cycle or a shared child) and a first child without a second one return
 *   HLGS_ERR_ARG.  Everything stays in scratch; sizes = {n_spt, n_entries, n_upper}.  host_syncs (may be NULL)
 *   receives the number of read-backs the call made: one after the validation, one per level of the two walks, one
 *   for the number of candidate SPTs and one for the sizes and the error word.
 *   stages: HLGS_SPT_STAGE_ALL; for measurement HLGS_SPT_STAGE_PACK (staging and validation kernels only), then
 *   HLGS_SPT_STAGE_WALK (the rest) on the same scratch.
 * hlgs_spt_emit_device (scene/gaussian_model.py:184-345): writes the ten arrays of hlgs_spt_result_copy, in that
 *   order, into caller-allocated device memory sized from the build's sizes (starts n_spt + 1); radii may be NULL
 *   (no bounding spheres).  nodes and scratch as given to the build, unchanged in between.
 * Integer outputs, up_xyz and up_scaling equal the host build's; the distances differ from it only where the
 * correctly rounded float32 exponential differs from libm's expf. */
#define HLGS_SPT_STAGE_PACK 1
#define HLGS_SPT_STAGE_WALK 2
#define HLGS_SPT_STAGE_ALL 3
#define HLGS_SPT_MAX_G (1 << 30)
size_t hlgs_spt_device_scratch_size(int G);
int hlgs_spt_build_device(int G, const int* nodes, const float* xyz, int64_t xyz_stride, const float* log_scales,
                          int64_t scale_stride, int root, float spt_root_volume, float target_granularity,
                          int min_spt_size, void* scratch, int stages, int* sizes, int* host_syncs, void* stream);
int hlgs_spt_emit_device(int G, const int* nodes, void* scratch, int n_spt, int n_entries, int n_upper, int* starts,
                         float* smax, float* smin, int* gidx, int* roots, int* up_nodes, float* up_xyz,
                         float* up_scaling, float* min_d2, float* radii, void* stream);
/* ---- n-ary mode of the SPT path (opt-in; the entry points above stay the binary path, bit for bit) ----
 * A merged scene hierarchy (hlgs_hier_merge_*) is no binary tree: rows with one child, rows with 3 and more, a root
 * with K children, and leaves whose first_child column holds id + 1.  The _nary entry points take it as it is.
 * The n-ary contract:
 * 1. Child lists.  The children of row v are child_count[v] rows: first_child[v], then next_sibling links.
 *    child_count == 0 means no children, and first_child is then not read (the merger's rule, see
 *    hlgs_hier_merge_emit), so the output of the merger and of hlgs_hier_build goes in unchanged.  Every member must
 *    lie in (root, G) and must be reached once; lists of length 1 are legal.  The rows before the root are the
 *    skybox rows, which carry no hierarchy: their node columns are not read and they are no members, so with root 0
 *    the range is the whole table but the root.  A list is walked for
 *    exactly child_count members, by the thread of its parent.  No kernel follows links in a loop that the table
 *    itself does not bound, and a link is range-checked before it is used as an index.  The builds validate the whole
 *    table before any walk; a violation returns HLGS_ERR_ARG.
 * 2. Walk order: rank-major.  The next frontier is the rank-0 child of every expanding node that has one, in frontier
 *    order, then the rank-1 child of every expanding node that has one, then rank 2, and so on.  On a binary tree
 *    this is the reference's cat(first_children, second_children).  This order defines the cut's order, the SPT
 *    entries' tie order and the flat cut's F*.
 * 3. The upper walk and the cut classify a node as before: culled, leaf (child_count == 0), condition false, expand.
 * 4. SPT walk.  It descends below v iff child_count[v] > 0.  Entries as before: max = the parent's min,
 *    min = min(md(c) + |x_c - centre|, the parent's min); md of a leaf is -1e9 at any level width (the one-element
 *    branch of get_min_distance, -1e6, depends on the per-SPT walk producing a one-node level and is not
 *    reproduced).  An SPT is kept if it has more than min_spt_size entries, sorted by max descending with ties in
 *    walk order; otherwise its entries join the upper tree.
 * 5. Upper-tree rows are sorted by hierarchy id, parent remapped and row 0's parent -1.  first_child is the SPT
 *    number at SPT leaves, whose child_count is set to 0; it is -1 where child_count == 0; otherwise it is remapped.
 *    next_sibling is remapped where it is > 0.  max_side_length is the hierarchy id.  Other rows keep their
 *    child_count, so the cut can walk their lists.  min_distance_squared as before.
 * 6. Bounding radii.  A parent's radius is the max over all its children of (child radius + centre distance); the
 *    last child to arrive computes it.  The max is exact, so the schedule does not show.
 * 7. Binary equivalence.  On a hierarchy that the binary path accepts, n-ary mode returns the binary path's result
 *    bit for bit, floats included.
 * hlgs_spt_build_nary, hlgs_spt_build_device_nary, hlgs_spt_emit_device_nary: arguments, results, scratch and stages
 *   of their binary neighbours.  The device build reads back once after the validation, once per level of the two
 *   walks (the level's children and its longest list in one read), once for the candidates and once for the sizes:
 *   a root with 300 children costs one level, not 300 round trips.
 * hlgs_upper_tree_order_nary: F* over all ranks, preorder positions and subtree ends of the n-ary tree; the blob
 *   layout and the limits (65,535 entries, 64 levels) are those of hlgs_upper_tree_order, and the flat cut takes
 *   either blob (it follows no links).
 * hlgs_upper_tree_cut_views_ordered_device_nary: hlgs_upper_tree_cut_views_ordered_device over child lists; with
 *   order = NULL the n-ary level walk, which runs every level in one workgroup (no waiting between workgroups);
 *   count_device[1] = 1 for a table that is not a tree. */
int hlgs_spt_build_nary(int G, const int* nodes, const float* xyz, const float* log_scales, int root,
                        float spt_root_volume, float target_granularity, int min_spt_size, int use_bounding_spheres,
                        hlgs_spt_result** out);
int hlgs_spt_build_device_nary(int G, const int* nodes, const float* xyz, int64_t xyz_stride, const float* log_scales,
                               int64_t scale_stride, int root, float spt_root_volume, float target_granularity,
                               int min_spt_size, void* scratch, int stages, int* sizes, int* host_syncs, void* stream);
int hlgs_spt_emit_device_nary(int G, const int* nodes, void* scratch, int n_spt, int n_entries, int n_upper,
                              int* starts, float* smax, float* smin, int* gidx, int* roots, int* up_nodes,
                              float* up_xyz, float* up_scaling, float* min_d2, float* radii, void* stream);
int hlgs_upper_tree_order_nary(int N, const int* nodes_host, void* order_host);
int hlgs_upper_tree_cut_views_ordered_device_nary(int N, const int* nodes, const void* order, const float* xyz,
                                                  const float* bounds, const float* min_dist2, int n_views,
                                                  const float* planes, const float* campos,
                                                  float distance_multiplier, int use_frustum, int use_lod,
                                                  void* scratch, int* cut, int* count_device, void* stream);
/* ---- n-ary relocation: the selection of the MCMC round on child lists (opt-in; relocate_gs's pair selection stays
 *      as it is) ----
 * GaussianModel.relocate_gs (scene/gaussian_model.py:1588-1698) is defined on sibling pairs only.  On the hierarchies of
 * the n-ary contract above the selection follows these rules, chosen so that on a hierarchy the binary path accepts
 * they give its selection (contract 7's analogue).  dead: size bytes, non-zero = flagged.
 *   candidate   a row v > sky with child_count 0 that is flagged (the root and inner rows are never candidates; the
 *               rows below sky are not read).
 *   group       per parent p with c children of which k are candidates, in list order.  k == c: the last member stops
 *               being a candidate (:1597-1599), so k = c - 1.  a = c - k survivors.  a == 1: a promote group -- the
 *               survivor s moves into p, and the freed rows are the k dead members in list order, then s (m = k + 1).
 *               a >= 2: an unlink group -- the freed rows are the k dead members in list order (m = k), survivor -1.
 *               Groups with k == 0 or m < 2 are dropped: a single dead child of three or more waits.
 *   order       kept groups ascending by their first freed row; on a binary tree the ascending dead list of
 *               relocate_gs, with (dead, sibling) as the freed pair.
 *   alive       rows >= sky with child_count 0 that are not flagged and are not the survivor of a kept promote group,
 *               ascending: the respawn candidates.
 * hlgs_mcmc_select_scratch_size(size): bytes of device scratch (256-byte aligned) both calls take.
 * hlgs_mcmc_select_count: nodes size x 6 int32 and dead in device memory.  Every row with child_count > 0 walks its own
 *   list for child_count members.  Validation, before a link is used as an index: child_count in [0, size); every member
 *   in (sky, size) and naming the walking row as its parent (so no row is in two lists); the last member's next_sibling
 *   0.  A violation sets HLGS_MCMC_SELECT_STATUS_LINKS and the list is not followed.  counts (4 device int32, valid once
 *   the stream has passed the call -- the selection's one read-back, by the caller): {groups, freed rows, alive,
 *   status}; with a non-zero status the three sizes are 0.
 * hlgs_mcmc_select_emit: nodes, dead and scratch as given to the count, unchanged in between.  group_parent and
 *   group_survivor (groups), group_start (groups + 1: group g's freed rows are free_rows[group_start[g] ..
 *   group_start[g + 1])), free_rows (freed rows) and alive (alive), caller-allocated device int32 arrays sized from
 *   counts.  With a non-zero status its kernel does nothing.
 * size in [0, HLGS_SPT_MAX_G], sky in [0, size], else HLGS_ERR_ARG.  Nothing is allocated, no host synchronisation,
 * every launch goes to `stream`.  A list is walked by one thread.  The result does not depend on the launch shape:
 * integers only, every word written by one thread, the status an OR. */
#define HLGS_MCMC_SELECT_STATUS_LINKS 1u
size_t hlgs_mcmc_select_scratch_size(int size);
int hlgs_mcmc_select_count(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch, int* counts,
                           void* stream);
int hlgs_mcmc_select_emit(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch, int* group_parent,
                          int* group_survivor, int* group_start, int* free_rows, int* alive, void* stream);
/* Row gather dst[i] = src[idx[i]] and scatter dst[idx[i]] = src[i] for n rows of row_bytes (a multiple of 4):
 * the streaming cache's storage[idx].cuda() loads and write-backs (train_post.py:439-488).  src / dst may be
 * pinned host memory (read and written by the GPU over the host link). */
int hlgs_gather_rows(int64_t n, int row_bytes, const int64_t* idx, const void* src, void* dst, void* stream);
int hlgs_scatter_rows(int64_t n, int row_bytes, const int64_t* idx, const void* src, void* dst, void* stream);

/* One bookkeeping pass of train_post.py's SPT cache (the body of the budget loop, :346-430): given the view's
 * coarse cut and the previous step's SPT state, decide which SPTs are reused, which are loaded, and which
 * resident Gaussians stay or are written back.  All arrays are device int32/float32 unless noted. */
typedef struct hlgs_cache_args {
    int n_cut;                         /* coarse cut (hlgs_upper_tree_cut) */
    const int* cut;
    const int* upper_nodes;            /* upper tree, n_upper x 6 */
    const float* upper_xyz;            /* n_upper x 3 */
    const float* campos;               /* 3 */
    float distance_multiplier;         /* SPT distances are |xyz - campos| * distance_multiplier */
    int num_spts;                      /* SPT ids are in [0, num_spts) */
    int m;                             /* prev_SPT_indices / _distances / _counts, m each */
    const int* prev_spt_indices;
    const float* prev_spt_distances;
    const int* prev_spt_counts;
    int R;                             /* len(render_indices) */
    const int* render_indices;
    int n_loaded_prev;                 /* len(load_from_disk_indices) of the previous pass */
    int skybox_points;
    float rtol, atol;                  /* isclose of the reused distances (Reuse_SPT_Tolerarance, 0.05) */
    const int* n_cut_device;           /* NULL, or the [count, overflow] words of hlgs_upper_tree_cut_device: the
                                          cut's length is then read on the device and n_cut is its capacity */
    int n_views;                       /* 0 or 1: campos is one camera; > 1: campos is n_views x 3 and each SPT's
                                          distance is that of the nearest camera (hlgs_upper_tree_cut_views_device) */
} hlgs_cache_args;
typedef struct hlgs_cache_plan {
    int* keep_spt_indices;             /* m: keep_SPT_indices */
    float* keep_spt_distances;         /* m: prev_SPT_distances[SPT_keep_counts_indices] */
    int* keep_spt_counts;              /* m: SPT_counts_new[:n_kept] */
    int* load_spt_indices;             /* n_cut: load_SPT_indices (for hlgs_spt_cut_*) */
    float* load_spt_distances;         /* n_cut */
    int* upper_render;                 /* n_cut: upper_tree_nodes_to_render */
    int* keep_rows;                    /* R: nonzero(keep_gaussians_mask) */
    int* render_kept;                  /* R: render_indices[keep_gaussians_mask] */
    int* write_back_rows;              /* R: nonzero(write_back_mask) */
    int* write_back_indices;           /* R: render_indices[write_back_mask] */
    int n_kept, n_load, n_upper;       /* host outputs: list lengths */
    int n_keep_rows;                   /* R - n_keep_rows rows are written back */
    int prefix;                        /* the prefix the loaded SPTs' counts are shifted by (plus skybox_points) */
} hlgs_cache_plan;
/* scratch: hlgs_spt_cache_scratch_size bytes; one host synchronisation for all the sizes. */
size_t hlgs_spt_cache_scratch_size(int n_cut, int m, int R, int num_spts);
int hlgs_spt_cache_plan(const hlgs_cache_args* a, hlgs_cache_plan* plan, void* scratch, void* stream);
/* dst_t[dst_rows[i]] = src_t[src_rows[i]] for i < n and every table t < T (at most 32); a NULL row list is the
 * identity.  src_rows may be in any order and may repeat; dst_rows entries must be distinct.
 * row_bytes a multiple of 4; src / dst may be pinned host memory.  All of a cache step's parameter
 * and Adam-moment traffic (train_post.py:439-479) in one launch per direction. */
typedef struct hlgs_row_copy {
    const void* src;
    void* dst;
    int64_t row_bytes;
} hlgs_row_copy;
int hlgs_copy_rows(int T, const hlgs_row_copy* tables, int64_t n, const int* src_rows, const int* dst_rows,
                   void* stream);
/* The host legs of the same traffic with packed host storage: host row h (host_row_bytes bytes, a multiple of 64,
 * at most 1024; pinned host memory) holds the T device tables' rows back to back -- table t's row at the sum of the
 * earlier tables' row_bytes -- then zero padding.  tables[t].src is the device table (dst is ignored), float32
 * rows.  to_host != 0: host[host_rows[i]] = (dev_0[dev_rows[i]], dev_1[dev_rows[i]], ..., 0...) -- whole host
 * rows, padding included;  to_host == 0: dev_t[dev_rows[i]] = the table's part of host[host_rows[i]].  NULL row
 * lists are the identity.  Every store or load the GPU issues to host memory covers whole 64-byte lines, where
 * per-tensor host storage takes one 12-180-byte fragment per tensor and row (train_post.py:439-479). */
int hlgs_copy_rows_packed(int T, const hlgs_row_copy* tables, int64_t n, const int* dev_rows, const int* host_rows,
                          void* host, int64_t host_row_bytes, int to_host, void* stream);
/* The load leg of a cache step with rows that are still resident (train_post.py:446-479 after the write-back of
 * :439-444): dst_t[i] = the table's part of host[host_rows[i]] for i < n, except that a host row h with
 * resident_of[h] = r >= 0 is taken from src_t[r] (tables[t].src, the resident table) instead of over the host
 * link -- the step's write-back has just stored the same bits at h.  tables[t].dst is the destination table;
 * resident_of is indexed by host row (NULL: every row from the host). */
int hlgs_load_rows_packed(int T, const hlgs_row_copy* tables, int64_t n, const int* host_rows, const int* resident_of,
                          const void* host, int64_t host_row_bytes, void* stream);
/* Dense Adam step of the cached training loop (train_post.py:786-812: skybox gradient rows zeroed, then
 * OurAdam._single_tensor_adam2, scene/OurAdam.py:357-448, with state step = step) over T (at most 32) tensors in
 * one launch.  The scalars follow torch: lr, betas and eps are the caller's doubles; step_size =
 * lr / (1 - beta1^step) and sqrt(1 - beta2^step) are formed in double, then every tensor op runs in float32. */
typedef struct hlgs_adam_tensor {
    float* param;
    float* grad;                       /* rows < skybox_rows are set to 0 before the update */
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int64_t row_elems;                 /* elements per Gaussian row */
    double lr;
} hlgs_adam_tensor;
int hlgs_adam_step(int T, const hlgs_adam_tensor* tensors, int64_t step, int skybox_rows, double beta1, double beta2,
                   double eps, void* stream);
/* The activations render() reads (scene/gaussian_model.py:44-56: get_opacity = sigmoid(_opacity), get_scaling =
 * exp(_scaling), get_rotation = normalize(_rotation), eps 1e-12) over n resident rows in one pass: opacity_raw n,
 * scaling_raw n x 3, rotation_raw n x 4 (16-byte aligned) -> opacity, scales, rotations (same shapes). */
int hlgs_activate_forward(int64_t n, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
                          float* opacity, float* scales, float* rotations, void* stream);
/* Their gradients in one pass: d_opacity_raw = g (1 - o) o, d_scaling_raw = g s, d_rotation_raw through the norm.
 * opacity / scales are the forward's outputs; any (g, d) pair may be NULL to skip that tensor. */
int hlgs_activate_backward(int64_t n, const float* opacity, const float* scales, const float* rotation_raw,
                           const float* g_opacity, const float* g_scales, const float* g_rotations, float* d_opacity_raw,
                           float* d_scaling_raw, float* d_rotation_raw, void* stream);
/* The same pass with the two regularisers of the MCMC training step (train_post.py:565-576): reg (device, 2 floats) =
 * (opacity_loss, scaling_loss) = (sum_i opacity_i / n, sum_i sum_k scales_ik / n) over the n rows passed in -- the
 * reference's sum(|.|) / len(render_indices); the activated values are positive, and the scaling sum over 3 n values
 * is divided by n as there.  The three activated outputs are bit-identical to hlgs_activate_forward's.  The sums are
 * workgroup partials added in double in a fixed order (no float atomics): reg does not change from run to run.
 * reg and scratch (hlgs_activate_reg_scratch_size(n) bytes) are required; n == 0 writes reg = (0, 0) on the stream and
 * launches no kernel. */
size_t hlgs_activate_reg_scratch_size(int64_t n);
int hlgs_activate_reg_forward(int64_t n, const float* opacity_raw, const float* scaling_raw, const float* rotation_raw,
                              float* opacity, float* scales, float* rotations, float* reg /* device, 2 floats */,
                              void* scratch, void* stream);
/* hlgs_activate_backward with the regularisers' upstream gradients g_reg = (dL/d opacity_loss, dL/d scaling_loss),
 * read on the device: d_opacity_raw = ((g_opacity + g_reg[0] / n) (1 - o)) o, d_scaling_raw = (g_scales + g_reg[1] / n) s.
 * With g_reg non-NULL a NULL g_opacity / g_scales counts as 0, and opacity, scales, d_opacity_raw and d_scaling_raw are
 * required; with g_reg NULL this is hlgs_activate_backward. */
int hlgs_activate_reg_backward(int64_t n, const float* opacity, const float* scales, const float* rotation_raw,
                               const float* g_opacity, const float* g_scales, const float* g_rotations,
                               const float* g_reg /* device, 2 floats, or NULL */,
                               float* d_opacity_raw, float* d_scaling_raw, float* d_rotation_raw, void* stream);

/* ---- photometric losses of the training step (utils/loss_utils.py:17-63, train_single.py:106-121,
 *      train_post.py:558-559 with the un-vendored fused_ssim) ---- */
/* SSIM of C planes of H x W (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2:
 * _ssim, loss_utils.py:44-63).  out (device, 2 floats) = (mean of the SSIM map -- over the interior
 * [5, H-5) x [5, W-5) when valid != 0, fused_ssim padding="valid" --, mean |img1 - img2| = l1_loss).
 * dmaps (C x 3 x H x W, or NULL when no gradient is needed) receives the map's derivatives with respect to the
 * window moments for hlgs_ssim_backward.  scratch: hlgs_ssim_scratch_size bytes. */
size_t hlgs_ssim_scratch_size(int C, int H, int W);
int hlgs_ssim_forward(int C, int H, int W, const float* img1, const float* img2, int valid, float* dmaps,
                      void* scratch, float* out, void* stream);
/* grad_img1 = coef[0] * d(sum of the SSIM map)/d img1 + coef[1] * sign(img1 - img2); coef is a device array so
 * the upstream gradient never needs a host read. */
int hlgs_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* dmaps,
                       const float* coef, float* grad_img1, void* stream);
/* The same two with flags: HLGS_SSIM_VALID (= valid above) and HLGS_SSIM_CLAMP1 -- img1 enters as clamp(img1, 0, 1),
 * the rendered_image.clamp(0, 1) of the reference's renderers (gaussian_renderer/__init__.py:142, 612) folded into
 * the loss: the forward reads the clamped values, the backward gradient passes only where 0 <= img1 <= 1 (torch's
 * clamp backward), so the two clamp kernels of each direction disappear.  Pass the same flags to both. */
#define HLGS_SSIM_VALID 1
#define HLGS_SSIM_CLAMP1 2
int hlgs_ssim_forward_ex(int C, int H, int W, const float* img1, const float* img2, int flags, float* dmaps,
                         void* scratch, float* out, void* stream);
int hlgs_ssim_backward_ex(int C, int H, int W, const float* img1, const float* img2, int flags, const float* dmaps,
                          const float* coef, float* grad_img1, void* stream);
/* The photometric forward and backward of a 3-channel render with what the reference does to it between the rasterizer
 * and the loss applied as the image is loaded -- nothing transformed is stored.  Per pixel p and channel c
 *   t_c  = image_0 E[0][c] + image_1 E[1][c] + image_2 E[2][c] + E[c][3]   (exposure given, else t_c = image_c)
 *   x'_c = m (CLAMP1 ? clamp(t_c, 0, 1) : t_c)                             (alpha_mask given, else m = 1)
 * E (12 device floats, row-major (3, 4)) is the view's trained exposure of render(..., use_trained_exp=True),
 * torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
 * (gaussian_renderer/__init__.py:139-141); the clamp is :142 (flags = HLGS_SSIM_CLAMP1, the only flag accepted);
 * m (H x W) is the alpha mask of train_single.py:102-104 / train_coarse.py:122-125 / render_hierarchy.py:108-112.
 * Zero padding is of x'.  out (device, 5 floats) = (mean SSIM of x' against gt, mean |x' - gt|, mean (x' - gt)^2 of
 * planes 0, 1, 2 -- the PSNR of utils/image_utils.py:17-19 follows from the last three).  dmaps (9 x H x W, or NULL: no
 * gradient maps) as hlgs_ssim_forward's.  scratch: hlgs_photo_scratch_size bytes, for either call.
 * Backward, with gv_c = coef[0] d(sum of the SSIM map)/d x'_c + coef[1] sign(x'_c - gt_c) and
 * g_c = gv_c m [0 <= t_c <= 1 under CLAMP1]:  grad_image_k = sum_c E[k][c] g_c (= g_k without an exposure);
 * grad_exposure (12 floats laid out as E, or NULL: not computed) [k][c] = sum_p image_k g_c, [c][3] = sum_p g_c.
 * No atomics: both gradients are bitwise reproducible.  Pass the same flags, exposure and mask to both calls. */
size_t hlgs_photo_scratch_size(int H, int W);
int hlgs_photo_forward(int H, int W, const float* image, const float* gt, int flags, const float* exposure,
                       const float* alpha_mask, float* dmaps, void* scratch, float* out, void* stream);
int hlgs_photo_backward(int H, int W, const float* image, const float* gt, int flags, const float* exposure,
                        const float* alpha_mask, const float* dmaps, const float* coef, float* grad_image,
                        float* grad_exposure, void* scratch, void* stream);
/* Depth term of train_single.py:111-118: out[0] = mean |(invdepth - mono) * mask| over n values (mask may be
 * NULL); backward grad = coef[0] * sign((invdepth - mono) * mask) * mask. */
size_t hlgs_depth_l1_scratch_size(int64_t n);
int hlgs_depth_l1_forward(int64_t n, const float* invdepth, const float* mono, const float* mask, void* scratch,
                          float* out, void* stream);
int hlgs_depth_l1_backward(int64_t n, const float* invdepth, const float* mono, const float* mask, const float* coef,
                           float* grad, void* stream);

/* ---- hierarchy files and traversal (host code, host buffers; gaussianhierarchy/hierarchy_loader.cpp,
 *      hierarchy_writer.cpp, traversal.cpp -- bound there as load_hierarchy, load_dynamic_hierarchy,
 *      write_hierarchy, write_dynamic_hierarchy, expand_to_target: ext.cpp:16-20) ---- */
#define HLGS_HIER_FULL 0    /* .hier, float32 (hierarchy_writer.cpp:33-57) */
#define HLGS_HIER_HALF 1    /* .hier, binary16 attributes (the default of WriteHierarchy, :58-110) */
#define HLGS_HIER_DYNAMIC 2 /* .dhier (HierarchyNode rows, :113-155) */
typedef struct hlgs_hier_info {
    int format;     /* HLGS_HIER_* */
    int G;          /* Gaussians */
    int N;          /* nodes (.dhier: == G, hierarchy_loader.cpp:185) */
    int sh_degree;  /* .dhier: stored degree (SH rows hold (deg+1)^2 coefficients); .hier: 3 (48 floats) */
} hlgs_hier_info;
/* Sizes of a hierarchy file; dynamic != 0 reads the .dhier header. */
int hlgs_hier_info_read(const char* path, int dynamic, hlgs_hier_info* info);
/* LoadHierarchy (torch_interface.cpp:9-40): pos G x 3, rot G x 4, log_scales G x 3, opacities G, shs G x 48,
 * nodes N x 7 int32 (Node), boxes N x 8 (minn xyzw, maxx xyzw); both the full and the half layout. */
int hlgs_hier_load(const char* path, float* pos, float* rot, float* log_scales, float* opacities, float* shs,
                   int* nodes, float* boxes);
/* WriteHierarchy (torch_interface.cpp:77-104); compressed != 0 writes the binary16 layout (the reference's
 * default) and fails with "Would lose information!" when a node count exceeds 32000. */
int hlgs_hier_write(const char* path, int G, int N, const float* pos, const float* shs, const float* opacities,
                    const float* log_scales, const float* rot, const int* nodes, const float* boxes, int compressed);
/* LoadDynamicHierarchy (torch_interface.cpp:43-74): shs G x (deg+1)^2 x 3, nodes G x 6 int32 (HierarchyNode). */
int hlgs_dhier_load(const char* path, float* pos, float* rot, float* log_scales, float* opacities, float* shs,
                    int* nodes);
/* WriteDynamicHierarchy (torch_interface.cpp:107-133): shs G x (deg+1)^2 x 3, nodes N x 6. */
int hlgs_dhier_write(const char* path, int G, int N, const float* pos, const float* shs, const float* opacities,
                     const float* log_scales, const float* rot, const int* nodes, int sh_degree);
/* ExpandToTarget (torch_interface.cpp:136-146, traversal.cpp:15-39): Gaussian indices of the cut at node depth
 * `target` over N static Nodes (host).  Writes min(count, capacity) entries to out (may be NULL to query). */
int hlgs_expand_to_target(int N, const int* nodes, int target, int* out, int capacity, int* count);

/* ---- inspection (tests): byte offsets of fields inside the caller's buffers, counted from the
 * buffer's first 256-byte-aligned address ---- */
size_t hlgs_binning_point_list_offset(int R);  /* uint32 point_list[R] */
/* point_list entries of a P-Gaussian forward started now are (Gaussian index << shift) | footprint quadrant mask: the
 * shift (a finished frame's own is hlgs_frame_info.entry_shift). */
int hlgs_point_list_entry_shift(int P);
/* The process-wide switches below are atomics, read once when a frame starts: a frame in flight keeps the options it
 * started with (reported in its hlgs_frame_info), so flipping a switch from another thread changes later frames only.
 * 1 if a P-Gaussian forward started now bins no instance whose quadrant mask is 0 (packed entries, dropping on): its tile
 * lists and n_contrib then match the oracle run with drop_empty (oracle/hlgs_oracle.c rect_quad_masks).  0: every
 * instance of the reference's binning (rasterizer_impl.cu:70-115) is listed, and point_list / n_contrib are laid out as
 * the reference lays them out. */
int hlgs_point_list_drops_empty(int P);
/* Tests: on = 0 makes every following frame use plain index entries (the P >= 2^28 path); 1 restores the default. */
void hlgs_set_entry_packing(int on);
/* on = 0: following frames bin every instance, including those whose footprint reaches none of their tile's quadrants
 * (the reference's tile lists and n_contrib; images and gradients are the same either way); 1 (default) drops them. */
void hlgs_set_drop_empty(int on);
/* Tests: the bound on each look-back poll of the fused binning plan (default 2^20 polls, ~0.1 s).  A plan whose
 * look-back times out is re-run with the two-launch plan that needs no inter-block wait; polls = 0 forces that path. */
void hlgs_set_plan_polls(unsigned polls);
size_t hlgs_image_ranges_offset(int W, int H);  /* uint2 ranges[tiles] */
/* uint32 misc[16]: [0] binned instances, [1] longest tile list, [2] record slots, [3] the frame's entry packing (1 when
 * entry_shift != 0), [4] the frame's drops_empty -- written on the device by the frame's binning plan; [5] non-zero when
 * a look-back of the frame's fused plan timed out (hlgs_set_plan_polls) and the frame was planned again by the
 * two-launch plan, which leaves the word set: the count kernel of the next fused plan clears it (LDS-histogram binning
 * only; the other words are not defined) */
size_t hlgs_image_misc_offset(int W, int H);
size_t hlgs_geom_splat_offset(int P);           /* float4 splat[P][4]: x, y, conic a, b | conic c, opacity, r, g |
                                                   b, 1/depth, t, 1/kids | record base, tile x0, y0, width */

/* ---- measurement hooks (bench.py) ---- */
/* Stage timing: every launch of each selected rasterizer stage (bit i of mask = stage i, -1 = all,
 * 0 = off) is bracketed by hipEvents on its launch stream.  hlgs_stage_stats returns, per stage, the
 * mean duration in ms over all launches recorded since the last hlgs_set_stage_timing call and the
 * number of launches (synchronises).  Off by default. */
void hlgs_set_stage_timing(int mask);
int hlgs_stage_count(void);
const char* hlgs_stage_name(int i);
int hlgs_stage_stats(float* mean_ms, int* calls, int max);

#ifdef __cplusplus
}
#endif
#endif
