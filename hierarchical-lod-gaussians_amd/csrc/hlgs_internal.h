// hlgs_internal.h -- buffer layouts and kernel launchers shared by the translation units of libhlgs.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/hlgs.h"

namespace hlgs {

constexpr int kScanItems = 2048;    // elements per scan block (256 threads x 8)
constexpr int kSortCap = 4096;      // largest per-tile list sorted in one LDS pass
constexpr int kWaveSortCap = 1024;  // longest per-tile list sorted in registers by one wave
constexpr size_t kAlign = 256;

// Gaussians per binning block: 4,096 or 1,024 chosen per launch (raster_fwd.hip bin_gauss), on 1,024 threads
constexpr int kBinMaxTiles = 16384; // tile grids up to this use LDS histograms (2 x 64 KiB)

// The blend backward splits each tile's list into up to kBwdSplits + 1 chunks of bwd_chunk_len(count) entries (a
// multiple of the 64-splat batch, at least kBwdChunk) and runs one wave per (tile, chunk), so a launch holds ~3x
// more, shorter waves than tiles.  A chunk that is not the tile's last starts from the per-pixel state the forward
// sampled at the chunk's end (Img::split_state): the transmittance there, and the colour and inverse depth blended
// behind it (final - sampled), which give the back-to-front recursion's accumulators without replaying the back part.
// Chunks of at least 192 entries (round 3; 128 before): a configs[1] tile (~300 entries) then has one boundary instead
// of two, which halves the split state the forward writes (its write traffic was 137 MB per view, 83 MB of it split
// state) at no measured cost (blend pair 538.6-538.9 against 535.2-536.7 us).
constexpr int kBwdChunk = 192;
constexpr int kBwdSplits = 2;
constexpr int kSplitFloats = 4 * 5 * 64;  // per (tile, split): [quadrant][T, dC r, g, b, dD][lane]
__host__ __device__ inline uint32_t bwd_chunk_len(uint32_t cnt)
{
    const uint32_t even = ((cnt + kBwdSplits) / (kBwdSplits + 1) + 63u) & ~63u;
    return even > (uint32_t)kBwdChunk ? even : (uint32_t)kBwdChunk;
}

inline size_t align_up(size_t x) { return (x + kAlign - 1) & ~(kAlign - 1); }
size_t scan_scratch_elems(size_t n);

// Per-Gaussian state written by the forward preprocess and read by the backward
// (the reference's GeometryState, rasterizer_impl.h:29-45).
struct Geom {
    float* depths;            // P
    uint32_t* clamped;        // P, bit c = colour channel c clamped at 0
    float2* means2D;          // P, pixel-space centre
    float* cov3D;             // P x 6
    uint32_t* tiles_touched;  // P
    uint32_t* point_offsets;  // P, inclusive scan of tiles_touched
    int2* rects;              // P, per-axis 3-sigma extent in pixels
    float4* splat;            // P x 4: the blend kernels' per-Gaussian record (see SplatRec)
    uint32_t* qmask;          // P: footprint quadrant masks of the first rect tiles (rect_quad_masks), written by the
                              // preprocess for the visible Gaussians when pack_entries; read by the key scatter
    int pack;                 // FrameOpts::pack of the frame this buffer is carved for (0 when carved without options)
    int drop;                 // FrameOpts::drop: instances whose quadrant mask is 0 are not binned
    uint32_t polls;           // FrameOpts::polls: bound on each look-back poll of the fused plan
    float* sh_jac;            // P x 9: d colour / d view direction (dRGBdx, dRGBdy, dRGBdz), written by k_preprocess_sh
                              // for the visible Gaussians when sh_jac_written(); the SH backward then reads no SH rows
    uint32_t* scan_tmp;
};

// SplatRec, the layout of Geom::splat: the 64-byte per-Gaussian record read by the blend kernels, one half cache
// line per (tile, Gaussian) instance instead of one line per attribute array.
//   [0] x, y, conic.a, conic.b      [1] conic.c, opacity, r, g
//   [2] b, 1/depth, t, 1/num_kids    [3] unused, first tile x | y << 16, rect width (int bits),
//                                        alpha threshold on e2 (alpha_e2_threshold)
// All written by the preprocess.  The Gaussian's record-slot base (the exclusive scan of the rect sizes) is read by
// the blend backward from point_offsets[idx - 1]: writing it into the record after the scan cost the key scatter a
// partial-line write per visible Gaussian.

// Tile-list entries (point_list, and the low word of the sort keys) are idx << kEntryShift | quadrant mask whenever
// the Gaussian count leaves the room (P < 2^28): bit q of the mask says the splat's alpha >= 1/255 footprint reaches
// 8x8 quadrant q of the tile (quad_mask), decided once by the key scatter so that the blends read it instead of
// testing the footprint in every quadrant wave.  Otherwise the entry is idx and the blends test it themselves.
// The low bits do not change the sort order: within a tile the (depth, idx) pairs are already distinct.
// pack_entries(P) is decided on the host (capi.hip; hlgs_set_entry_packing turns it off for tests), once per frame
// (FrameOpts), and reaches the kernels as Geom::pack / their flags argument.
constexpr int kEntryShift = 4;
constexpr int kMiscPack = 3;  // Img::misc word holding the frame's FrameOpts::pack
constexpr int kMiscDrop = 4;  // Img::misc word holding the frame's FrameOpts::drop
constexpr int kMiscFail = 5;  // Img::misc word: a block of the fused plan timed out in its look-back (k_tile_offsets_plan)
constexpr int kMiscDone = 6;  // Img::misc word: blocks of the fused plan done with their ranges
constexpr uint32_t kPlanPolls = 1u << 20;  // default bound on each look-back poll of the fused plan (~0.1 s)
bool pack_entries(int P);
// drop_empty(P): with packed entries, an instance whose quadrant mask is 0 (its footprint reaches none of the tile's
// four 8x8 quadrants, so no pixel of the tile blends it) is not binned: the tile lists, the sort and the blends' staging
// skip it.  Its record slot stays (point_offsets and num_rendered are unchanged) and is never written; k_gauss_bwd
// skips the slots whose mask is 0 (their records would be zero).  On by default; hlgs_set_drop_empty(0) bins every
// instance, so point_list and n_contrib are laid out exactly as the reference's binning lays them out.
bool drop_empty(int P);
// The frame's binning options, read once from the process-wide test switches (atomics, hlgs_set_entry_packing /
// hlgs_set_drop_empty / hlgs_set_plan_polls) when the frame starts; nothing inside a frame reads the switches again,
// so a thread that flips one while another renders changes only later frames.  The plan kernels write pack and drop
// into Img::misc[kMiscPack], [kMiscDrop] and the host reports them in hlgs_frame_info (entry_shift, drops_empty).
struct FrameOpts {
    int pack = 0, drop = 0;
    uint32_t polls = 0;
    uint32_t flags() const { return (uint32_t)pack | (uint32_t)drop << 1; }  // the plan kernels' flags argument
};
FrameOpts frame_opts(int P);
// lds_binning(P, gx, gy): the LDS-histogram binning plan applies (raster_fwd.hip)
bool lds_binning(int P, int gx, int gy);
// Does the forward's preprocess (k_preprocess_sh2) leave Geom::sh_jac for the SH backward?  Same condition as its launch.
inline bool sh_jac_written(const hlgs_raster_args& a)
{
    const int gx = (a.W + 15) / 16, gy = (a.H + 15) / 16;
    return !a.indices && !a.colors_precomp && a.shs && a.M > 0 && a.M <= 16 && lds_binning(a.P, gx, gy);
}
Geom carve_geom(void* base, int P, size_t* total, const FrameOpts& o = FrameOpts());

// Per-pixel / per-tile state (ImageState, rasterizer_impl.h:47-54) plus binning counters.
struct Img {
    float* final_T;        // N
    uint32_t* n_contrib;   // N
    uint2* ranges;         // T: [start, end) into point_list
    uint32_t* tile_count;  // T
    uint32_t* tile_cursor; // T
    uint32_t* misc;        // 16: [0] = binned instances, [1] = longest per-tile list, [2] = record slots (point_offsets[P-1]),
                           // [kMiscPack], [kMiscDrop] = the frame's FrameOpts (the backward reads pack here, not a switch),
                           // [kMiscFail], [kMiscDone]: the fused plan's failure and completion words
    uint32_t* scan_tmp;
    float* split_state;    // T x kBwdSplits x kSplitFloats (see bwd_chunk_len)
};
Img carve_img(void* base, int W, int H, size_t* total);

// Per-instance state (BinningState).  keys = depth_bits << 32 | gaussian index, grouped by tile.
struct Bin {
    uint64_t* keys;
    uint64_t* keys2;
    uint32_t* point_list;  // R, tile-major then front-to-back
};
Bin carve_bin(void* base, int R, size_t* total);

// Backward scratch: one 48-byte gradient record per (tile, Gaussian) instance, stored Gaussian-major at the
// Gaussian's point_offsets slot so the per-Gaussian reduction reads contiguous rows; one slot is three float4s
// (one contiguous write per instance instead of three partial lines in three arrays):
//   rec[3 s]     dmean2D.x, dmean2D.y, dconic.x, dconic.y
//   rec[3 s + 1] dconic.w, dopacity, dcolor.r, dcolor.g
//   rec[3 s + 2] dcolor.b, dinvdepth, -, -
struct BwdScratch {
    float4* rec;
    float* parent_dmean;  // P x 3 (hierarchy mode only)
};
BwdScratch carve_bwd(void* base, int P, int R, size_t* total);

// Buffers the preprocess clears on its way (instead of separate memsets before it): the per-tile counts the
// binning adds into and the caller's `seen` flags.  Null members are skipped.
struct ZeroJob {
    uint32_t* tile_count;
    int T;
    int* seen;
    int P;
};
__device__ __forceinline__ void zero_prelude(const ZeroJob& z, int tid, int nthreads)
{
    if (z.seen)
        for (int i = tid; i < z.P; i += nthreads) z.seen[i] = 0;
    if (z.tile_count)
        for (int i = tid; i < z.T; i += nthreads) z.tile_count[i] = 0;
}

// Non-temporal float4 accesses for streams that pass once and are next touched, if at all, after far more traffic
// than the caches hold: the SH rows the preprocess reads, the direction Jacobians it writes for the backward and the
// SH gradient rows the backward writes.  They do not displace the lines the next kernels read again (the records,
// the tile lists) from L2 and the memory-side cache.
typedef float nt_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_nt(const float4* p)
{
    const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void store_nt(float4* p, const float4& a)
{
    const nt_f4 v = {a.x, a.y, a.z, a.w};
    __builtin_nontemporal_store(v, reinterpret_cast<nt_f4*>(p));
}

// Speculative render (hlgs_rasterize_forward): the render kernels are queued before the host has read
// R and the longest tile list; each exits at once when they exceed what the launch was sized for.
struct Guard {
    const uint32_t* misc;  // Img::misc (R, longest list) or nullptr = no check
    uint32_t cap_R, cap_n;
};
__device__ __forceinline__ bool guard_fail(const Guard& gd)
{
    return gd.misc && (gd.misc[0] > gd.cap_R || gd.misc[1] > gd.cap_n);
}

// Rasterizer stages, in hlgs_stage_name order; stage_mark (capi.hip) times a stage when hlgs_set_stage_timing asks.
enum Stage { ST_PRE = 0, ST_SCAN, ST_RANGES, ST_SCATTER, ST_SORT, ST_BLEND_FWD, ST_BLEND_BWD, ST_GAUSS_BWD,
             ST_COUNT_TILES, ST_COUNT };
void stage_mark(hipStream_t s, int stage, bool begin);

// preprocess.hip
void launch_preprocess(const hlgs_raster_args& a, const Geom& g, int* radii, uint32_t* tile_count, int gx, int gy,
                       const ZeroJob& z, hipStream_t s);
// raster_fwd.hip
uint32_t* bin_histogram(const Img& im, int P, int gx, int gy);
void launch_count_tiles(int P, const int* radii, const Geom& g, const Img& im, int gx, int gy, bool alt,
                        hipStream_t s, uint32_t* hist, bool fused);
// k_plan's words for the host (R, longest list, record slots) in the pinned read-back slot `host`: three 64-bit
// words, each carrying the frame's sequence number in its high half, written by single-copy-atomic 64-bit stores, so
// the host waits until all three carry it and the kernel needs no system-scope release (a write-back of the whole L2).
void launch_plan(int P, const Geom& g, const Img& im, int gx, int gy, uint32_t* host, uint32_t seq, hipStream_t s,
                 bool fused);
void launch_tile_ranges(const Img& im, int T, const uint32_t* point_offsets, int P, uint32_t flags, hipStream_t s);
void launch_binning(const hlgs_raster_args& a, const int* radii, const Geom& g, const Img& im, const Bin& b, int gx,
                    int gy, uint32_t max_count, hipStream_t s, bool timing, Guard gd);
void launch_blend_fwd(const hlgs_raster_args& a, const Geom& g, const Img& im, const Bin& b, int gx, int gy,
                      float* out_color, float* out_invdepth, int* seen, hipStream_t s, Guard gd);
void launch_mark_visible(int P, const float* means, const float* view, uint8_t* present, hipStream_t s);
void launch_relocation(int P, const float* oo, const float* so, const int* N, const float* binoms, int n_max,
                       float* on, float* sn, hipStream_t s);
// raster_bwd.hip
void launch_blend_bwd(const hlgs_raster_args& a, const Geom& g, const Img& im, const Bin& b, const BwdScratch& rs,
                      int gx, int gy, const float* dL_dpix, const float* dL_dinv, hipStream_t s);
// gauss_bwd.hip
void launch_gauss_bwd(const hlgs_raster_args& a, const int* radii, const Geom& g, const BwdScratch& rs,
                      const hlgs_grads& o, bool has_depth, hipStream_t s, hipStream_t late, hipEvent_t ev,
                      const uint32_t* misc);
void launch_sh_from_colour(int P, int V, int D, int M, bool alt, const float* means, const float* campos,
                           const float* drgb, int64_t stride, float scale, float* dsh, float* ddc, hipStream_t s);

// Upper-tree cut (stream.hip).  Per level the frontier (the reference's `stack`) is filtered by the cull;
// leaves go to the cut, then the non-leaves whose LOD condition is false, each group in frontier order; the
// next frontier is the first children of the expanded nodes in order, then their first children's next
// siblings in order (scene/gaussian_model.py:364-404).
constexpr int kCutLevelLaunches = 8;  // wide-level launches queued after the narrow walk (stream.hip)
constexpr int kCutMaxBlocks = 64;      // workgroups of one wide level (all resident at once)
struct CutState {          // the walk's state between k_upper_cut and the k_cut_level launches
    int size, total, parity, overflow;
};
struct CutFlat {           // the flat cut's placement state between k_cut_flat_place and k_cut_flat_write
    uint64_t leaf[1024], stop[1024];            // per thread run: the alive leaves / condition-false nodes
    int2 off[1024];                             // per run: leaves and condition-false nodes before it
    int2 lev[HLGS_CUT_FLAT_MAX_LEVELS + 1];     // per level: (leaves, condition-false nodes) before its first entry
};
struct CutArgs {
    int N;
    const int* nodes;      // N x 6 HierarchyNode rows: 2 child_count, 3 first_child, 4 next_sibling
    const float* xyz;
    const float* bounds;
    const float* min_dist2;
    const float* planes;   // nviews x 4 x (nx, ny, nz, d), normalised as extract_frustum_planes does
    const float* campos;   // nviews x 3
    float dmul;
    int use_frustum, use_lod;
    int nviews;            // >= 1: the cut serves the union of the views (visible in any frustum, LOD of the nearest)
    int* front_a;
    int* front_b;
    int capacity;          // entries of cut
    int* cut;
    int* count;            // [0] = cut size, [1] = overflow flag
    CutState* state;
    unsigned* arrive;      // kCutLevelLaunches arrival counters
    int* level_counts;     // 3 x kCutMaxBlocks
    CutFlat* flat;
};
size_t upper_cut_state_bytes();
void launch_upper_cut(const CutArgs& a, hipStream_t s);
void launch_upper_cut_nary(const CutArgs& a, hipStream_t s);  // child lists, rank-major (hlgs.h)
void launch_upper_cut_flat(const CutArgs& a, const int* order, hipStream_t s);

// SPT cache bookkeeping of one streaming step (stream.hip, train_post.py:346-430)
struct CacheArgs {
    int n_cut;                // the cut's length, or its capacity when n_cut_dev is set
    const int* n_cut_dev;     // [count, overflow] of the device-side upper cut, or NULL
    const int* cut;           // coarse cut of the upper tree
    const int* nodes;         // upper-tree HierarchyNode rows
    const float* xyz;
    const float* campos;      // nviews x 3: an SPT's distance is that of the nearest camera
    int nviews;
    float dmul;
    int num_spts;
    int m;                    // previous step's SPTs
    const int* prev_idx;
    const float* prev_dist;
    const int* prev_counts;
    int R;                    // len(render_indices)
    int tail_end;             // len(render_indices) - len(load_from_disk_indices)
    float rtol, atol;
    // scratch
    int* flag;                // num_spts, zero on entry
    int* spt_idx;             // n_cut
    float* spt_dist;          // n_cut
    int* diff;                // R + 1, zero on entry
    int* sizes;               // device: n_kept, n_load, n_upper, prefix
    // outputs
    int* keep_idx;
    float* keep_dist;
    int* keep_counts;
    int* load_idx;
    float* load_dist;
    int* upper;
};
void launch_cache_lists(const CacheArgs& a, hipStream_t s);
void launch_cache_keep(int R, int sky, const uint32_t* diff_incl, uint32_t* keep, hipStream_t s);
void launch_cache_split(int R, const int* render, const uint32_t* keep_incl, int* keep_rows, int* render_kept,
                        int* wb_rows, int* wb_indices, hipStream_t s);
void launch_rows(bool gather, long n, int row_bytes, const int64_t* idx, const void* src, void* dst, hipStream_t s);
struct RowCopy {
    const void* src;
    void* dst;
    int64_t row_bytes;
    int device_only;          // both sides in device memory: 16-byte accesses at 4-byte alignment are used
};
constexpr int kMaxRowTables = 32;
void launch_rows_multi(int T, const RowCopy* tabs, int64_t n, const int* src_rows, const int* dst_rows,
                       hipStream_t s);
constexpr int kPackSlots = 4;  // packed host rows of up to 4 x 64 words (1 KiB)
void launch_rows_packed(int T, float* const* tabs, const int* words, int64_t n, const int* dev_rows,
                        const int* host_rows, float* host, int hw, bool to_host, hipStream_t s,
                        const float* const* resident = nullptr, const int* resident_of = nullptr);
// optim.hip: one dense Adam step over up to kMaxRowTables tensors (OurAdam._single_tensor_adam2)
struct AdamTensor {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    int64_t row_elems;        // elements per Gaussian row (skybox rows have their gradient zeroed)
    float neg_step_size;      // -lr / (1 - beta1^step)
};
void launch_adam_multi(int T, const AdamTensor* t, int sky, float b1, float a1, float b2, float a2, float bc2_sqrt,
                       float eps, hipStream_t s);
void launch_adam(float* param, const float* grad, float* m, float* v, const uint8_t* vis, float lr, float b1, float b2,
                 float eps, uint32_t N, uint32_t M, hipStream_t s);

// act.hip
void launch_act_fwd(int64_t n, const float* op_raw, const float* sc_raw, const float* rot_raw, float* op, float* sc,
                    float* rot, hipStream_t s);
void launch_act_bwd(int64_t n, const float* op, const float* sc, const float* rot_raw, const float* g_op,
                    const float* g_sc, const float* g_rot, float* d_op, float* d_sc, float* d_rot, hipStream_t s);
// the same with the MCMC regularisers (train_post.py:565-576): reg = (sum op, sum sc) / n through `partial`
// (2 floats per act_reg_blocks(n)); g_reg (device, 2 floats) = their upstream gradients, NULL: the plain backward
int64_t act_reg_blocks(int64_t n);
void launch_act_reg_fwd(int64_t n, const float* op_raw, const float* sc_raw, const float* rot_raw, float* op, float* sc,
                        float* rot, float* reg, float* partial, hipStream_t s);
void launch_act_reg_bwd(int64_t n, const float* op, const float* sc, const float* rot_raw, const float* g_op,
                        const float* g_sc, const float* g_rot, const float* g_reg, float* d_op, float* d_sc,
                        float* d_rot, hipStream_t s);

// loss.hip
// k_reduce_partials, one block: out[k] = s_k * sum_i partial[i * stride + k] for k < stride <= 2, in double, in index order
void launch_reduce_partials(int n, int stride, const float* partial, double s0, double s1, float* out, hipStream_t s);
size_t ssim_partials(int C, int H, int W);
void launch_ssim_forward(int C, int H, int W, const float* img1, const float* img2, int valid, float* abc,
                         float* partial, float* out, hipStream_t s, bool clamp1);
void launch_ssim_backward(int C, int H, int W, const float* img1, const float* img2, const float* abc,
                          const float* coef, float* grad1, hipStream_t s, bool clamp1);
size_t photo_scratch_floats(int H, int W);
void launch_photo_forward(int H, int W, const float* image, const float* gt, const float* expo, const float* amask,
                          float* abc, float* partial, float* out, hipStream_t s, bool clamp1);
void launch_photo_backward(int H, int W, const float* image, const float* gt, const float* expo, const float* amask,
                           const float* abc, const float* coef, float* grad, float* grad_expo, float* partial,
                           hipStream_t s, bool clamp1);
int depth_l1_blocks(long n);
void launch_depth_l1_forward(long n, const float* inv, const float* mono, const float* mask, float* partial,
                             float* out, hipStream_t s);
void launch_depth_l1_backward(long n, const float* inv, const float* mono, const float* mask, const float* coef,
                              float* grad, hipStream_t s);

// lod.hip
void launch_morton(int P, const float* xyz, const float* mn, const float* mx, int64_t* codes, hipStream_t s);
void launch_expand_dynamic(int N, float target, const int* nodes, const float* pos, const float* scales,
                           const float* vp, const float* vd, int* ri, int* pi, int* ni, uint32_t* counts,
                           uint32_t* incl, uint32_t* tmp, hipStream_t s);
void launch_weights_dynamic(int n, const int* idx, float target, const int* nodes, const float* pos,
                            const float* scales, const float* vp, float* ts, int* kids, hipStream_t s);
void launch_expand_static(int N, float target, const int* nodes, const float* boxes, const float* vp, int* ri,
                          int* pi, int* ni, uint32_t* counts, uint32_t* incl, uint32_t* tmp, hipStream_t s);
void launch_weights_static(int n, const int* idx, float target, const int* nodes, const float* boxes,
                           const float* vp, float* ts, int* kids, hipStream_t s);
void launch_spt_prepare(int s_, const int* starts, const float* smax, const int* sidx, const float* sdist,
                        uint32_t* sizes, uint32_t* incl, uint32_t* tmp, hipStream_t s);
void launch_spt_finish(int s_, int E, int n, const int* gidx, const int* starts, const float* smin, const int* sidx,
                       const float* sdist, int compat, const uint32_t* sizes, const uint32_t* incl, uint32_t* counts,
                       uint32_t* counts_incl, uint32_t* tmp_s, int* result, uint32_t* keep, uint32_t* keep_incl,
                       uint32_t* tmp_n, int* cut, int* counts_prefix, hipStream_t s);
void launch_lod_interp_fwd(int S, int n, int M3, const int* ridx, const int* pidx, const float* w, const float* means,
                           const float* scales, const float* rots, const float* opac, const float* shs, float* om,
                           float* osc, float* orot, float* oop, float* osh, hipStream_t s);
size_t lerp_bwd_scratch_elems(int P, int n);
void launch_lod_interp_bwd(int P, int S, int n, int M3, const int* ridx, const int* pidx, const float* w,
                           const float* rots, const float* gm, const float* gsc, const float* grot, const float* gop,
                           const float* gsh, float* dm, float* dsc, float* drot, float* dop, float* dsh, void* scratch,
                           hipStream_t s);

// knn.hip: 3-nearest-neighbour mean squared distance.  A box is kKnnBox consecutive Morton-sorted points (one wave of
// the search), a super-box kKnnSuper consecutive boxes (one lane each in the box test), a sort tile the kKnnSortTile
// keys one block of a radix pass histograms and scatters.
constexpr int kKnnBox = HLGS_KNN_BOX;
constexpr int kKnnSuper = HLGS_KNN_SUPER;
constexpr int kKnnSortTile = HLGS_KNN_SORT_TILE;
static_assert(kKnnBox == 64 && kKnnSuper == 64, "one lane per row of a box and per box of a super-box");
static_assert(kKnnSortTile % 256 == 0, "a sort tile is whole rounds of the histogram's 256 threads");
size_t knn_scratch_bytes(int P);
void launch_knn(int P, const float* xyz, void* scratch, float* out, hipStream_t s);
// The sort of knn.hip on its own: P (key, value) pairs by the full 32-bit key, four stable LSD passes, so equal keys
// keep the order they came in.  hist: radix_hist_elems(P) words, scan_tmp: scan_scratch_elems(radix_hist_elems(P)).
// The result is in keys / vals; the *_tmp arrays are overwritten.
size_t radix_hist_elems(size_t P);
void radix_sort_pairs_u32(uint32_t P, uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp,
                          uint32_t* hist, uint32_t* scan_tmp, hipStream_t s);

// hier_build.hip: the dynamic hierarchy of N activated Gaussians (kd-tree, bottom-up merge, top-down rotation
// alignment, pre-order node table).  A subtree of at most kHierCap leaves is finished by one workgroup.
constexpr int kHierCap = HLGS_HIER_LDS_CAP;
enum HierStage { HB_KD_TOP = 0, HB_KD_LDS, HB_LEAVES, HB_MERGE, HB_ALIGN, HB_FINISH, HB_STAGES };
struct HierIn {
    int N, shf;
    const float *xyz, *shs, *opacity, *scales, *rotations;
};
struct HierOut {
    float *pos, *shs, *alpha, *log_scales, *rot;
    int* nodes;
};
size_t hier_scratch_bytes(int N);
void launch_hier_valid(const HierIn& in, int strict, uint8_t* mask, uint32_t* status, hipStream_t s);
// stages: bit i runs HierStage i (HLGS_HIER_ALL: the build; single bits in order: the same build, stage by stage)
void launch_hier_build(const HierIn& in, const HierOut& out, void* scratch, int stages, hipStream_t s);

// hier_merge.hip: one chunk hierarchy weighted, filtered, spliced and re-linearised under the scene root.  The tree
// passes are one launch per depth; the depths are bucketed from the validated node table.
constexpr int kMergeLevels = HLGS_MERGE_MAX_DEPTH + 1;
struct MergeIn {
    int n, shf;
    const float *pos, *shs, *alpha, *log_scales, *rot;
    const int* nodes;
};
size_t merge_scratch_bytes(int n);
// stages: bit 0 validate, bit 1 weights and counts
void launch_merge_plan(const MergeIn& in, int k, int K, const float* centers, float falloff, void* scratch,
                       int stages, hipStream_t s);
// stages: bit 0 depth buckets and bottom-up, bit 1 top-down, bit 2 rows.  level_counts: host, kMergeLevels entries
void launch_merge_emit(const MergeIn& in, const HierOut& out, int k, const float* centers, const int* level_counts,
                       int kept, int out_offset, int leaf_offset, int last, void* scratch, int stages, hipStream_t s);
void launch_merge_root(int K, int shf, int G, const int* roots, const float* centers, float log_scale,
                       const HierOut& out, hipStream_t s);

// mcmc.hip: opacity-weighted sampling, the position noise and the counter-based numbers of the densification round
constexpr int kMcmcItems = 2048;  // candidates per block of the sampler's float64 prefix sum (256 threads x 8)
size_t mcmc_sample_scratch_bytes(int64_t n);
void launch_mcmc_sample(int64_t n, const void* opacity_base, int64_t stride_bytes, const int* alive, int64_t num,
                        uint64_t seed, uint32_t stream_id, int* sampled, int* counts, int64_t size, void* scratch,
                        hipStream_t s);
void launch_mcmc_noise(int64_t P, int64_t first_row, float* means, const float* op_raw, const float* sc_raw,
                       const float* rot_raw, const float* noise, double scale, uint64_t seed, uint32_t step,
                       hipStream_t s);
void launch_rng_fill(int kind, uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, void* out, hipStream_t s);

// mcmc_nary.hip: the selection of the relocation over child lists (count, read-back by the caller, emit)
size_t mcmc_select_scratch_bytes(int size);
void* mcmc_select_zero_region(void* scratch, int size, size_t* bytes);  // what the caller clears before the count
void launch_mcmc_select_count(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch, int* counts,
                              hipStream_t s);
void launch_mcmc_select_emit(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch,
                             int* group_parent, int* group_survivor, int* group_start, int* free_rows, int* alive,
                             hipStream_t s);

// density.hip: the adaptive density control of chunk training (statistics, selection, plan, emit, opacity reset)
void launch_density_stats(int64_t P, const float* g, const int* radii, float* accum, float* denom, float* maxr,
                          hipStream_t s);
void launch_density_select(int64_t P, const float* accum, const float* maxr, const float* op, const uint8_t* leaf,
                           double thr, double dmin, double pmin, int64_t protect, uint8_t* sel, uint8_t* prune,
                           hipStream_t s);
size_t densify_scratch_bytes(int64_t P);
const int* densify_counts(void* scratch, int64_t P);  // device: [n_kept, n_selected] after launch_densify_plan
void launch_densify_plan(int64_t P, const uint8_t* sel, const uint8_t* prune, int drop_selected, void* scratch,
                         hipStream_t s);
// tables: at most kMaxRowTables, none empty; returns non-zero when the grid would not fit
int launch_densify_emit(int T, const hlgs_densify_table* tables, int64_t P, int64_t n_kept, int64_t n_sel, int copies,
                        int mode, const float* rotation, const float* noise, uint64_t seed, uint32_t round,
                        void* scratch, hipStream_t s);
void launch_opacity_reset(int64_t P, int64_t protect, double cap, float* op, float* m, float* v, hipStream_t s);

// spt_build.hip: the SPTs and the upper tree of a dynamic hierarchy (the device restatement of spt_build.cpp).
// Both return an HLGS_* code (the message set); sizes = {n_spt, n_entries, n_upper}
size_t spt_device_scratch_bytes(int G);
int spt_device_build(int G, const int* nodes, const float* xyz, int64_t xyz_stride, const float* log_scales,
                     int64_t scale_stride, int root, float volume, float tg, int min_size, void* scratch, int stages,
                     int* sizes, int* syncs, bool nary, hipStream_t s);
int spt_device_emit(int G, const int* nodes, void* scratch, int n_spt, int n_entries, int n_upper, int* starts,
                     float* smax, float* smin, int* gidx, int* roots, int* up_nodes, float* up_xyz, float* up_scaling,
                     float* min_d2, float* radii, bool nary, hipStream_t s);

// scan.hip
void scan_inclusive_u32(const uint32_t* in, uint32_t* out, size_t n, uint32_t* tmp, hipStream_t s);

}  // namespace hlgs
