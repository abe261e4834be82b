/*
 * f3dgs.h — C ABI of the MI355X-native differentiable Gaussian rasterizer
 * (libf3dgs_hip.so).
 *
 * This is the drop-in boundary for the one hot path of Feature-3DGS: the
 * tile-based forward/backward rasterizer.  Every entry point below replaces
 * one static method of the reference's C++ class `CudaRasterizer::Rasterizer`
 *   (reference: submodules/diff-gaussian-rasterization-feature/
 *               cuda_rasterizer/rasterizer.h:20-94)
 * which is what the reference's torch binding (rasterize_points.cu:35-236)
 * calls.  Signatures use plain pointers and sizes only: no torch types, no
 * C++ types.  All pointers are DEVICE pointers unless stated otherwise; all
 * float tensors are contiguous fp32; matrices are the 16-float
 * "transposed" matrices the reference passes (scene/cameras.py:55-58), i.e.
 * element (row r, col c) of the mathematical matrix is m[4*c + r].
 *
 * Differences to the reference interface (all deliberate):
 *   - `C` (number of semantic-feature channels) is a RUN-TIME argument.  The
 *     reference bakes it in as the macro NUM_SEMANTIC_CHANNELS
 *     (cuda_rasterizer/config.h:16) and must be recompiled per feature dim.
 *     C == 0 is valid.
 *   - The three `std::function<char*(size_t)>` resize hooks
 *     (rasterizer.h:36-38) become (function pointer, context) pairs.
 *   - Every call takes the HIP stream to enqueue on (the reference uses the
 *     legacy default stream) and returns an int status instead of throwing.
 *   - Optional inputs follow the reference's convention: NULL means "absent"
 *     (forward.cu:204,240; backward.cu:398,402).
 *   - backward() zero-initialises / fully overwrites every output itself; the
 *     caller may pass uninitialised memory (the reference requires zeroed
 *     buffers, rasterize_points.cu:163-173).
 *
 * Alignment: the per-Gaussian kernels read rotations, SH rows and feature
 * rows, and write their gradients, with 16-byte accesses.  `shs`,
 * `rotations`, `semantic_feature`, `dL_dsh`, `dL_drot`, `dL_dconic`,
 * `dL_dsemantic_feature` and `scratch` must therefore be 16-byte aligned
 * (hipMalloc and torch allocations are; a view at an odd storage offset is
 * not).  f3dgs_forward / f3dgs_backward return F3DGS_ERR_INVALID_ARGUMENT for
 * a misaligned pointer; the torch binding copies such a view first.  Image
 * planes may have any alignment (aligned ones take the vector path).
 * The decoder kernels of f3dgs_feature_l1 / f3dgs_feature_decode read the
 * rows of `weight` and the arrays they carve from `scratch` with 16-byte
 * accesses: with a decoder (weight != NULL) both must be 16-byte aligned, and
 * a misaligned one is refused with F3DGS_ERR_INVALID_ARGUMENT before anything
 * is launched.  `feature_map`, `gt`, `bias` and the gradient outputs may have
 * any (float) alignment; an aligned `d_feature_map` takes the vector stores.
 *
 * Status codes: 0 = ok, negative = error; f3dgs_last_error() returns a
 * thread-local human-readable message for the last failing call.
 */
#ifndef F3DGS_H_INCLUDED
#define F3DGS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F3DGS_OK 0
#define F3DGS_ERR_INVALID_ARGUMENT (-1)
#define F3DGS_ERR_HIP (-2)
#define F3DGS_ERR_ALLOC (-3)
#define F3DGS_ERR_UNSUPPORTED (-4)

/* Resize hook: must return a device pointer to at least `nbytes` bytes that
 * stays valid until the matching backward call has completed.  Mirrors
 * `std::function<char*(size_t)>` of rasterizer.h:36-38 /
 * resizeFunctional() of rasterize_points.cu:27-33. */
typedef char* (*f3dgs_resize_fn)(void* ctx, size_t nbytes);

/* Library / ABI version: major*10000 + minor*100 + patch (3.8.0 -> 30800). */
int f3dgs_version(void);

/* Thread-local message of the last error raised on this host thread. */
const char* f3dgs_last_error(void);

/*
 * Process-wide options (no counterpart in the reference).  Each option selects between complete code paths that
 * are exercised by the test suite (tests/test_abi_and_surface.py fails on an option without a test); none removes
 * work.  Defaults are seeded ONCE, at first use of the library, from the environment variable
 * F3DGS_<NAME IN CAPITALS>; afterwards only these calls change them (no launch path reads the environment).
 *   "tile_cull"      1 (default): instances whose 1/255-alpha ellipse misses a tile are never emitted (they
 *                    could not blend at any of its pixels, so outputs are unchanged); 0: the reference's
 *                    bounding-rectangle lists, bit-identical private state (used by the parity tests)
 *   "feature_mfma"   1 (default): feature contraction of the blend kernels on the matrix pipe (exact fp32);
 *                    0: vector pipe only
 *   "profile"        1: per-stage HIP events, see f3dgs_profile_read; 2: only around the two blend kernels
 *   "sort_onesweep"  0 (default): three-kernel radix passes; 1: single-pass radix scatter with decoupled look-back
 *                    (measured slower on MI355X, kept as a tested alternative)
 *   "depth_sort_buckets"  depth sort of more than 16,384 Gaussians: ONE stable pass that cuts the depth keys into up to 2,047
 *                    buckets by (key - smallest alive key) >> shift, then one launch that sorts every bucket inside LDS (four
 *                    launches, two trips through memory) instead of three or four LSD passes (nine or twelve launches): 1 always,
 *                    0 never, -1 (default) for 16,384 < P <= 1,250,000, where it was measured faster.  The lists are the same
 *                    bits either way, for any input: a bucket of more than 8,064 Gaussians (many at one depth) is sorted by
 *                    its workgroup alone in streaming passes - correct, slow; f3dgs_depth_sort_info counts them.  Environment:
 *                    F3DGS_DEPTH_SORT_BUCKETS.  Not with sort_onesweep = 1.
 *   "bwd_pl"         blend backward formulation: 1 pixel-lane kernel (all sums on the matrix pipe), 0 instance-lane
 *                    kernel, -1 (default) by channel count (pixel-lane from the first feature channel on; from five with
 *                    bwd_bf16 = 0)
 *   "bwd_half"       instance-lane blend backward: 1 (default) chunks of 32 instances against two pixel halves,
 *                    0 chunks of 64
 *   "bwd_order"      blend backward: 1 (default) workgroups take the tiles longest walk first
 *   "bwd_bf16"       pixel-lane blend backward: 1 every per-Gaussian sum contracts on bf16 matrix instructions
 *                    (v_mfma_f32_16x16x32_bf16, fp32 accumulation) with each fp32 operand split into two bf16 terms -
 *                    a relative error of a few 1e-6 per product against the 1e-3 tolerance of the gradients; 0: exact-fp32
 *                    matrix instructions (16x slower per multiply-add, and they block the vector pipe of their SIMD);
 *                    -1 (default): by the frame - bf16 while no visible Gaussian is longer than "bwd_bf16_max_ratio" times
 *                    its width (3D scales and screen-space footprint; f3dgs_forward notes per geometry buffer whether
 *                    the frame holds such a Gaussian - against the ratio in force at that call -, f3dgs_backward looks it
 *                    up), otherwise - and when the note is gone - the HYBRID first window: its moment block (the six
 *                    geometric sums) on exact-fp32 matrix instructions, feature and colour blocks on bf16.  The covariance
 *                    chain behind the blend amplifies an error of the MOMENT sums by the square of that ratio
 *                    (measured: the bf16 shape within a third of the gradient bound up to 16, outside it from 32 on);
 *                    a frame replayed from a graph launches both shapes and the frame's word lets one run on the device;
 *                    the later channel windows of wide features (C > 32: feature sums only, nothing amplifies them) stay on
 *                    the bf16 contraction under -1 whatever the first window took
 *   "bwd_bf16_max_ratio"  (default 16) the axis ratio up to which bwd_bf16 = -1 takes the bf16 contraction
 *   "bwd_wide8"      bf16 shape of the pixel-lane blend backward, feature widths above 96: 1 (default) later channel windows of
 *                    up to 128 channels on eight waves per tile (four of them evaluate the blend weights, all eight contract)
 *                    where more than 64 channels remain - half as many re-evaluations of the lists; 0: 64 channels on four
 *   "bwd_m44"        fp32 shape of the pixel-lane blend backward (bwd_bf16 = 0): 1 (default) the colour / depth sums contract on 4 x 4 matrix blocks
 *                    (v_mfma_f32_4x4x1_16B_f32) instead of a 16-column block of which four are used
 *   "bwd_split16"    fp32 shape of the pixel-lane blend backward (bwd_bf16 = 0) with up to 16 feature channels, and its later channel windows of up to 32: 1 (default)
 *                    the column blocks are split over the four waves by quadrants as well (no wave without matrix work, partial
 *                    sums added in the flush), 0 by columns only
 *   "fwd_wide"       blend forward: 1 (default) 128-channel windows where more than 64 channels remain
 *   "fwd_round"      blend forward, matrix shapes of 5..32 channels: list positions a wave tests per round.  64 (default): the hits
 *                    are queued and blended in full chunks of 32; 32: one chunk per round.  Same results bit for bit
 *   "fwd_solo"       blend forward: 1 (default) one 64-thread workgroup per quadrant wave
 *   "sync_free"      0: f3dgs_forward waits for the instance count where the reference does
 *                    (rasterizer_impl.cu:283; here behind the enqueue of the depth sort) and carves the binning buffer for
 *                    exactly that length.  -1 (default): as 1 inside a graph capture, as 0 otherwise (eager, the wait is already
 *                    hidden behind the depth sort: measured, the option changes nothing there).  1: SYNC-FREE FORWARD - the binning buffer is carved for a provision
 *                    ("instance_capacity"), the emit kernel and the tile sort read the count on the device, and the host reads
 *                    it only behind the last launch of the call (it has long been final by then); a frame that found no room
 *                    runs its binning and blend once more with the exact length before the call returns (binning_resize is
 *                    then called a SECOND time in the same forward call, while the first round's kernels may still be in
 *                    flight on the stream: a hook that frees the old buffer must do so in stream order).  Results are
 *                    bit-identical to sync_free = 0.  With sync_free = 1 or -1 the call may also run on a stream that is being
 *                    CAPTURED into a HIP graph (hipStreamBeginCapture / torch.cuda.graph): then nothing is read on the host,
 *                    *num_rendered receives the last count this thread read on the device (at least 1), the blend backward of
 *                    bwd_bf16 = -1 launches both shapes of its first window and the frame's long-axis word lets one of them
 *                    run on the device, and a replayed frame that finds no room is
 *                    VOID: it raises word [4] of f3dgs_forward_counts(), which the owner of the graph checks after a replay
 *                    (and captures again with more room).  Capturing needs one eager forward call on the same host thread and
 *                    device beforehand (pinned count words, a provision); "debug", "profile" and "sort_onesweep" are not
 *                    available inside a capture.
 *   "instance_capacity"  sync_free = 1: entries of the instance lists to provide for; 0 (default): 1.25 x the last count this
 *                    thread read on the device + 4096
 *   "knn_outward"    f3dgs_knn_neighbors: 1 (default) a wave walks the leaves outward from its own (home - 1, home + 1,
 *                    home - 2, ...), 0 in storage order; the lists are the same bits either way
 * Unknown names return F3DGS_ERR_INVALID_ARGUMENT.
 */
int f3dgs_set_option(const char* name, int value);
int f3dgs_get_option(const char* name, int* value /* host pointer, out */);

/* Which contraction the last f3dgs_backward of this PROCESS (any thread: PyTorch runs the backward pass on an autograd thread)
 * ran its blend stage with: 1 the pixel-lane kernel in its two-term bf16 shape, 2 its hybrid shape (first window: feature and
 * colour blocks on bf16, the moment block on exact-fp32 matrix instructions), 3 one of those two chosen ON THE DEVICE by the
 * frame's long-axis word (a frame captured into a graph), 0 an exact-fp32 shape (pixel-lane fp32 or the instance-lane kernel),
 * -1 no backward call yet.  A diagnostic for tests and benchmarks. */
int f3dgs_last_backward_contraction(void);
/* The pinned host words the most recent f3dgs_forward of this THREAD reports its frame in (kernel-written unless said otherwise;
 * NULL before the first call): [0] entries of the instance lists, [1] the reference's num_rendered, [2] != 0: a visible Gaussian
 * has a long axis (option bwd_bf16_max_ratio), [3] entries the binning buffer was carved for (written by the host at enqueue),
 * [4] sticky - an emit wave of a CAPTURED frame found no room (the caller clears it).  They are final once the frame's work has
 * completed (synchronise first); a replayed graph writes the words of the call it was captured from. */
const uint32_t* f3dgs_forward_counts(void);
/* How the calling thread's most recent f3dgs_forward call sorted its Gaussians by depth (read-only; NULL before the first call):
 * [0] the path, F3DGS_DEPTH_SORT_*, [1] bins of the bucket pass in use, the one of the culled Gaussians included, [2] Gaussians a
 * bucket may hold to be sorted inside LDS, [3] the frame's largest bucket, [4] its buckets above [2] ([1 .. 4]: zero on the other
 * paths).  [3] and [4] are written by the frame's kernels: final once its work has completed (synchronise first).  The pointer
 * is good until this thread's next call of this function. */
#define F3DGS_DEPTH_SORT_NONE 0        /* P = 0 */
#define F3DGS_DEPTH_SORT_ONE_LAUNCH 1  /* up to 16,384 Gaussians: one workgroup */
#define F3DGS_DEPTH_SORT_PASSES 2      /* LSD passes of three launches each */
#define F3DGS_DEPTH_SORT_BUCKETS 3     /* option depth_sort_buckets */
#define F3DGS_DEPTH_SORT_LOOKBACK 4    /* option sort_onesweep */
const uint32_t* f3dgs_depth_sort_info(void);
/* ONE view split over several GPUs by tile rows (no counterpart in the reference; SURVEY.md 8(e), "alternative for single huge
 * views"): from this call on the f3dgs_forward calls of this THREAD list and blend only the tiles of rows [tile_row_begin,
 * tile_row_end) of the 16 x 16 tile grid (clipped to the grid; (0, 0) restores the whole view; any other pair with begin >= end
 * is an EMPTY band - the share of a rank beyond the last tile row).  Inside the band the images,
 * final T and n_contrib are bit-identical to the whole view's; outside it the outputs hold the background / zeros.  A Gaussian
 * whose rectangle misses the band is invisible to the call (radius 0, no gradient); *num_rendered counts the band's tiles: over
 * a partition of the rows the counts add up to the whole view's, the element-wise maximum of the radii is the whole view's,
 * and the SUM of the band calls' gradients (each given the upstream gradient of its own rows) is the whole view's gradient -
 * the same all-reduce a view-sharded step ends with (dp.py: band_rows, gather_bands).  The matching f3dgs_backward needs
 * nothing: it reads the band's lists from the forward call's buffers. */
void f3dgs_set_tile_band(int tile_row_begin, int tile_row_end);
/* Host-only diagnostic (no GPU needed): the order in which the blend kernels' workgroups take the tiles of a gx x gy grid when
 * rows [begin, end) are listed - tiles_out[v] = tile of virtual id v (gx * gy entries).  A band is a contiguous run of tile ids,
 * i.e. one XCD's share under the whole-view mapping; with a band the ids are relabelled so that every XCD's run of virtual ids
 * starts with an eighth of the band's tiles.  Returns 1 if the relabelling is on, 0 for the identity (whole view, a band of
 * more than about half the grid, a tiny grid), < 0 on error. */
int f3dgs_debug_band_order(int gx, int gy, int tile_row_begin, int tile_row_end, uint32_t* tiles_out /* host, gx * gy */);
/* Enumeration: the name of option `index` (0, 1, ...), NULL past the end. */
const char* f3dgs_option_name(int index);

/*
 * Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:24-29,
 * rasterizer_impl.cu:141-153): present[i] = (view * p_i).z > 0.2.
 * `present` is a device array of P bytes (0/1).
 */
int f3dgs_mark_visible(
    int P,
    const float* means3D,
    const float* viewmatrix,
    const float* projmatrix,
    uint8_t* present,
    void* stream /* hipStream_t */);

/*
 * Replaces CudaRasterizer::Rasterizer::forward (rasterizer.h:31-62,
 * rasterizer_impl.cu:198-342).
 *
 *   P  number of Gaussians, D active SH degree (0..3), M SH coefficients per
 *      colour channel held by `shs` (0 if absent), C semantic channels.
 *   shs (P,M,3) | colors_precomp (P,3): exactly one non-NULL.
 *   scales (P,3) + rotations (P,4) | cov3D_precomp (P,6): exactly one set.
 *   semantic_feature (P,C) (may be NULL iff C == 0), opacities (P).
 *   out_color (3,H,W), out_feature_map (C,H,W), out_depth (1,H,W), radii (P)
 *   are fully written (radii may be NULL).
 *
 * The three opaque state buffers are sized through the resize hooks and must
 * be handed back unchanged to f3dgs_backward.  Their layout is private to
 * this library.  *num_rendered receives the reference's return value: the
 * number of (tile, Gaussian) instances of the 3-sigma bounding rectangles
 * (rasterizer_impl.cu:279-283).  The private instance lists may be shorter:
 * unless option "tile_cull" is 0, instances whose 1/255-alpha ellipse misses
 * the tile are never emitted (they could not blend at any pixel, so outputs
 * are unchanged).  Reading the counts costs one
 * 8-byte device-to-host copy + stream sync, like rasterizer_impl.cu:283.
 */
int f3dgs_forward(
    f3dgs_resize_fn geometry_resize, void* geometry_ctx,
    f3dgs_resize_fn binning_resize, void* binning_ctx,
    f3dgs_resize_fn image_resize, void* image_ctx,
    int P, int D, int M, int C,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* semantic_feature,
    const float* opacities,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* cam_pos,
    float tan_fovx, float tan_fovy,
    int prefiltered,
    float* out_color,
    float* out_feature_map,
    float* out_depth,
    int* radii,
    int debug,
    void* stream /* hipStream_t */,
    int* num_rendered /* host pointer, out */);

/* Bytes of device scratch f3dgs_backward needs for P Gaussians (the
 * reference cudaMalloc's its scratch inside the call,
 * rasterizer_impl.cu:402-430; here the caller owns it). */
size_t f3dgs_backward_scratch_bytes(int P, int C);

/*
 * Replaces CudaRasterizer::Rasterizer::backward (rasterizer.h:64-94,
 * rasterizer_impl.cu:347-461).
 *
 *   R = num_rendered returned by the matching forward call; geom/binning/
 *   image buffers are the ones that call filled.
 *   dL_dpix (3,H,W), dL_dfeaturepix (C,H,W), dL_depths (1,H,W): upstream
 *   gradients.
 *   Outputs (all fully overwritten): dL_dmean2D (P,3) [x,y in NDC units, z=0],
 *   dL_dopacity (P), dL_dcolor (P,3), dL_dsemantic_feature (P,C),
 *   dL_dmean3D (P,3), dL_dcov3D (P,6), dL_dsh (P,M,3), dL_dscale (P,3),
 *   dL_drot (P,4).  dL_dconic (P,4) and dL_dz (P) are OPTIONAL diagnostics
 *   (NULL = not wanted); the reference allocates but never returns them.
 *   dL_dsh may be NULL iff M == 0; dL_dscale/dL_drot may be NULL iff scales
 *   is NULL.  `scratch` points to f3dgs_backward_scratch_bytes(P, C) bytes.
 */
int f3dgs_backward(
    int P, int D, int M, int C, int R,
    const float* background,
    int width, int height,
    const float* means3D,
    const float* shs,
    const float* colors_precomp,
    const float* semantic_feature,
    const float* scales,
    float scale_modifier,
    const float* rotations,
    const float* cov3D_precomp,
    const float* viewmatrix,
    const float* projmatrix,
    const float* campos,
    float tan_fovx, float tan_fovy,
    const int* radii,
    const char* geom_buffer,
    const char* binning_buffer,
    const char* image_buffer,
    const float* dL_dpix,
    const float* dL_dfeaturepix,
    const float* dL_depths,
    float* dL_dmean2D,
    float* dL_dconic,
    float* dL_dopacity,
    float* dL_dcolor,
    float* dL_dsemantic_feature,
    float* dL_dmean3D,
    float* dL_dcov3D,
    float* dL_dsh,
    float* dL_dscale,
    float* dL_drot,
    float* dL_dz,
    void* scratch,
    int debug,
    void* stream /* hipStream_t */);

/*
 * Fused feature-map loss around the rasterizer (no single counterpart in the reference: it replaces the three
 * PyTorch calls of train.py:99-105 - F.interpolate(bilinear, align_corners=True) to the ground truth's size, the
 * optional 1x1-conv decoder `CNN_decoder` (models/networks.py:107-119) and l1_loss (utils/loss_utils.py:17-18) - and
 * their autograd backward).  feature_map (C,H,W); gt (Cout,Hg,Wg); weight (Cout,C) + bias (Cout) or both NULL for
 * "no decoder" (then Cout must equal C).  Outputs: *loss (device scalar) = mean |decode(resize(feature_map)) - gt|,
 * d_feature_map (C,H,W), d_weight (Cout,C), d_bias (Cout): the gradients of that loss (upstream gradient 1; they
 * scale linearly).  With a decoder C must be 32, 64 or 128 (the contraction runs on the fp32 matrix pipe in
 * 32-channel blocks); other shapes return F3DGS_ERR_UNSUPPORTED.  `scratch`: f3dgs_feature_l1_scratch_bytes(...) bytes.
 * With a decoder `weight` and `scratch` must be 16-byte aligned ("Alignment" above): F3DGS_ERR_INVALID_ARGUMENT otherwise.
 *
 * d_feature_map may be NULL: the dense (C,H,W) gradient - zeros at every pixel the resize does not sample, 8 of 9 when the
 * ground truth is a third of the image - is then not written.  The gradient at the LOSS's resolution stays in `scratch`
 * ((Hg*Wg, C) floats, pixel-major, f3dgs_feature_l1_lowres_grad) for as long as the caller keeps `scratch`, and goes to the
 * blend backward through f3dgs_set_feature_grad_lowres, which applies the transposed resize tile by tile.
 */
size_t f3dgs_feature_l1_scratch_bytes(int C, int Cout, int Hg, int Wg, int has_decoder);
int f3dgs_feature_l1(int C, int H, int W, int Cout, int Hg, int Wg, const float* feature_map, const float* weight,
                     const float* bias, const float* gt, float* loss, float* d_feature_map, float* d_weight,
                     float* d_bias, void* scratch, void* stream /* hipStream_t */);

const float* f3dgs_feature_l1_lowres_grad(int C, int Cout, int Hg, int Wg, int has_decoder, void* scratch);

/*
 * The next f3dgs_backward call of THIS thread takes its feature-map gradient (the argument dL_dfeaturepix of
 * rasterize_points.cu:121 `RasterizeGaussiansBackwardCUDA`) at the resolution of the loss: gx = (Hg*Wg, C) floats,
 * pixel-major, dL/d(resized feature map) as f3dgs_feature_l1 leaves it; `scale`: device scalar multiplied in (the upstream
 * gradient of the loss) or NULL.  The blend backward computes, per tile, what F.interpolate's backward would have written
 * there (same products, same order: bit-identical to the dense path) - it reads Hg*Wg*C floats instead of H*W*C.
 * dL_dfeaturepix of that call may be NULL; if it is not, the two are added.  Needs Hg <= H and Wg <= W (shrinking: at
 * most two output samples per source row / column) and option feature_mfma = 1, else the call returns
 * F3DGS_ERR_UNSUPPORTED.  The setting is consumed by that call whatever it returns - including its early returns (P == 0,
 * an argument error) -; gx == NULL clears it.  The kernel reads exactly the Hg*Wg*C floats of `gx`, nothing beyond them.
 */
int f3dgs_set_feature_grad_lowres(const float* gx, int Hg, int Wg, const float* scale);

/*
 * Fused image loss (the other half of train.py:99-105): (1 - lambda) * l1_loss(image, gt) + lambda * (1 - ssim(image, gt))
 * of utils/loss_utils.py:17-18, :33-63 at window_size 11 (Gaussian window, sigma 1.5, zero padding 5, C1 = 0.01^2,
 * C2 = 0.03^2), forward and backward.  image, gt: N x C x H x W fp32, contiguous (a C x H x W image is N = 1); any
 * N, C, H, W >= 1, images smaller than the window included.  All outputs are device pointers; nothing is read back to the
 * host, no memset is issued and every launch goes to `stream`: both calls may be captured into a graph.  The loss is
 * deterministic (partial sums reduced in a fixed order).
 *
 * f3dgs_image_loss_forward writes *loss, *l1 = mean |image - gt|, *ssim = mean SSIM over all N*C*H*W elements and, if
 * ssim_per_image is not NULL, the N per-image means (size_average=False).  want_grad != 0: it also leaves in `scratch`
 * (f3dgs_image_loss_scratch_bytes(N, C, H, W, want_grad) bytes) the three per-pixel fp32 maps the backward call reads.
 *
 * f3dgs_image_loss_backward writes d_image (N x C x H x W), the gradient with respect to `image` (none is formed for gt) of
 *   mode F3DGS_IMAGE_LOSS_L1_DSSIM        the loss above;                          upstream: one device scalar
 *   mode F3DGS_IMAGE_LOSS_SSIM            the mean SSIM;                           upstream: one device scalar
 *   mode F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE  the N per-image means (a vector output); upstream: N device values
 * times the upstream gradient.  `scratch` is the buffer a want_grad forward call on the same image and gt filled.
 */
#define F3DGS_IMAGE_LOSS_L1_DSSIM 0
#define F3DGS_IMAGE_LOSS_SSIM 1
#define F3DGS_IMAGE_LOSS_SSIM_PER_IMAGE 2
size_t f3dgs_image_loss_scratch_bytes(int N, int C, int H, int W, int want_grad);
int f3dgs_image_loss_forward(int N, int C, int H, int W, const float* image, const float* gt, float lambda_dssim, int want_grad,
                             float* loss, float* l1, float* ssim, float* ssim_per_image, void* scratch, void* stream);
int f3dgs_image_loss_backward(int N, int C, int H, int W, const float* image, const float* gt, float lambda_dssim, int mode,
                              const float* upstream, const void* scratch, float* d_image, void* stream);

/*
 * Image-quality metrics of N rendered views against their ground truth, forward only (the image half of evaluation:
 * metrics.py:71-74 `ssim` and `psnr` per test view, train.py:210-239 `l1_loss` and `psnr`).  Per image n of the N x C x H x W
 * batch, in one launch chain:
 *   l1[n]   = mean |image - gt|                    (utils/loss_utils.py:17-18, per image)
 *   mse[n]  = mean (image - gt)^2                  (utils/image_utils.py:20-21)
 *   psnr[n] = 20 * log10(1 / sqrt(mse[n]))         (utils/image_utils.py:23-25: formed in fp32 from the fp32 mse; identical
 *                                                   images give +inf, as the reference does)
 *   ssim[n] = mean SSIM                            (utils/loss_utils.py:33-63 at window_size 11: the window, padding and
 *                                                   constants of f3dgs_image_loss_forward)
 * Each output is NULL or N floats on the device.  With ssim == NULL the windowed moments are not formed at all.
 * `image` and `gt` choose their format independently:
 *   F3DGS_IMAGE_F32             N x C x H x W fp32, contiguous; with F3DGS_METRICS_QUANTIZE_IMAGE / _GT in `flags` every value v
 *                               is replaced by floor(clamp(v * 255 + 0.5, 0, 255)) / 255 as it is read - the value
 *                               to_tensor(Image.open(...)) gives of the PNG that torchvision's save_image wrote of v
 *                               (render.py:151-152; `mul(255).add_(0.5).clamp_(0, 255)`, the cast to uint8, `div(255)`: the
 *                               same fp32 roundings in the same order; a NaN is cast to 0 and +-inf clamp).  Without the flag
 *                               the values are taken as they are, NaN included.
 *   F3DGS_IMAGE_U8_PLANAR       N x C x H x W uint8; the value is v / 255 (fp32 division, as to_tensor forms it)
 *   F3DGS_IMAGE_U8_INTERLEAVED  N x H x W x C uint8, as PIL hands an image over
 * A quantised fp32 side and the uint8 tensor torch's chain makes of it give bit-identical results.  Any N, C, H, W >= 1, images
 * smaller than the window included; N == 0 is a no-op.  F3DGS_ERR_INVALID_ARGUMENT: bad sizes, an unknown format or flag, a
 * quantize flag on a uint8 side, a NULL image, gt or scratch.  `scratch`: f3dgs_image_metrics_scratch_bytes(N, C, H, W) bytes
 * (three partial sums per 64 x 16 tile; 0 for bad sizes), uninitialised.  Planes of any alignment; rows are read with 16-byte
 * (fp32) or 4-byte (uint8 planar) loads when W % 4 == 0 and the base pointer is aligned to that.  Deterministic (partial sums
 * reduced in a fixed order in fp64, no atomics); nothing is read back to the host, no memset is issued and both launches go
 * to `stream`: capturable.
 */
#define F3DGS_IMAGE_F32 0
#define F3DGS_IMAGE_U8_PLANAR 1
#define F3DGS_IMAGE_U8_INTERLEAVED 2
#define F3DGS_METRICS_QUANTIZE_IMAGE 0x1
#define F3DGS_METRICS_QUANTIZE_GT 0x2
size_t f3dgs_image_metrics_scratch_bytes(int N, int C, int H, int W);
int f3dgs_image_metrics(int N, int C, int H, int W, const void* image, int image_format, const void* gt, int gt_format, int flags,
                        float* l1 /* N */, float* mse /* N */, float* psnr /* N */, float* ssim /* N */, void* scratch,
                        void* stream /* hipStream_t */);

/*
 * Language-guided editing (gaussian_renderer/__init__.py:21-55, calculate_selection_score and
 * calculate_selection_score_delete; render_edit :131-148 calls them for every edited frame): which rows of the (P, C) fp32
 * feature table match the K text embeddings `text` (K x C fp32), in one pass over the table.  Per row f, in the reference's
 * number formats: n = ||f||_2 and f^ = f / n in fp32 (written to normalized_out if that is not NULL; it may alias
 * `features`, the reference's in-place `features /= ...`); f^ and the fp32-normalised text rows rounded to fp16;
 * s_k = f^ . t^_k rounded to fp16; for K > 1 the softmax p over the K scores, every p_k rounded to fp16 (both carried in
 * fp64 and rounded once: the fp16 neighbour of the exact value, which the reference's fp32 evaluations scatter around).  Then, on those fp16 values (pos = the columns of positive_mask, first = first_positive, i.e.
 * positive_ids[0]; q = fp16(sum of p_k over pos); v = p with column `first` replaced by q; m = (argmax_k v_k is in pos),
 * NaN counting as the maximum and the lowest column winning a tie; q2 = fp16(sum of v_k over pos), which counts the
 * positives other than `first` twice, as the reference does):
 *
 *   K = 1 (a threshold is required)      mask = s_0 >= threshold                  score_out = s_0
 *   select, K > 1, has_threshold         mask = q >= threshold                    score_out = q
 *   select, K > 1, no threshold          mask = m                                 score_out = q
 *   delete, K > 1, has_threshold         mask = m or q2 >= threshold              score_out = q2
 *   delete, K > 1, no threshold          mask = m                                 score_out = q
 *
 * A row of zero norm or with a non-finite element has NaN scores: every >= is false and the argmax is column 0.
 * mask_out: P floats, 0 or 1.  score_out: NULL or P floats.  opacity_in / opacity_out (both NULL or both given, P floats,
 * may alias): render_edit's masked fill fused, opacity_out = 0 where the mask is set (F3DGS_EDIT_FILL_UNSELECTED: where
 * it is NOT set, the extraction), opacity_in elsewhere.  `variant` is F3DGS_EDIT_SELECT or F3DGS_EDIT_DELETE, optionally
 * or-ed with F3DGS_EDIT_TEXT_NORMALIZED (the rows of `text` are already t / ||t|| in fp32: the kernel only rounds them)
 * and F3DGS_EDIT_FILL_UNSELECTED.  Limits: K <= F3DGS_EDIT_MAX_TEXTS and K * C <= F3DGS_EDIT_MAX_TEXT_ELEMENTS (the fp16
 * text block lives in 64 KB of LDS); positive_mask non-empty with no bit at or above K and bit first_positive set.
 * Rows are read with 16-byte loads when C % 4 == 0, C <= 2048 and the pointers are 16-byte aligned; anything else takes a
 * slower scalar path.  No scratch, no host read, no memset; one launch on `stream`: capturable.  P = 0 is a no-op.
 */
#define F3DGS_EDIT_SELECT 0
#define F3DGS_EDIT_DELETE 1
#define F3DGS_EDIT_TEXT_NORMALIZED 0x100
#define F3DGS_EDIT_FILL_UNSELECTED 0x200
#define F3DGS_EDIT_MAX_TEXTS 64
#define F3DGS_EDIT_MAX_TEXT_ELEMENTS 32768
int f3dgs_edit_select(int P, int C, int K, const float* features, float* normalized_out, const float* text,
                      uint64_t positive_mask, int first_positive, int variant, int has_threshold, float threshold,
                      float* mask_out, float* score_out, const float* opacity_in, float* opacity_out,
                      void* stream /* hipStream_t */);

/*
 * The contribution pass (no counterpart in the reference, whose only route from a region of a rendered view back to the
 * Gaussians behind it is a backward call with the region as upstream gradient): one more walk over the tile lists of a finished
 * f3dgs_forward call, found in its three state buffers as f3dgs_backward finds them (P, R = num_rendered, width and height of
 * that call; a call made under f3dgs_set_tile_band needs nothing more: tiles outside the band have empty lists).  For pixel p
 * and list position k <= n_contrib[p] the weight is w = alpha * T, formed with the forward's own instruction sequence and the
 * forward's own set of contributors: the pass reproduces the forward's blend weights bit for bit.  Every output is optional,
 * NULL = not wanted, and the work for it is then skipped; at least one must be given.
 *   Per pixel, H x W each, fully written (empty tiles, P == 0 and R == 0 included):
 *     alpha         float   1 - T_final
 *     median_depth  float   the view-space depth of the first blended entry after which T < 0.5; 0 where T never gets there
 *                           (no background on depth, as for the depth image)
 *     ids           int32   the Gaussian of the blended entry of largest weight - the earliest one of an exact tie -, -1 where
 *                           nothing blended
 *     id_weight     float   that entry's weight, or 0
 *   Per Gaussian:
 *     acc           (P, K + 1) floats, ADDED TO (the caller zeroes it once and may accumulate many views): column k < K receives
 *                   the sum over the pixels of w * masks[k][pixel], column K the sum of w.  masks: (K, H, W) floats, any values
 *                   (soft masks), 0 <= K <= F3DGS_CONTRIB_MAX_MASKS; the products are plain fp32.  K = 0: the weight total alone.
 *     wmax          (P) floats, MAX-ED INTO: the largest weight the Gaussian reaches at any pixel.  Weights are >= 0 and the
 *                   maximum is taken on the bit patterns: the buffer must hold non-negative values (zeros to begin with).
 * The sums of `acc` arrive through float atomics in a varying order: like the gradients of f3dgs_backward they are not
 * bit-reproducible between runs.  wmax and every per-pixel output are.  F3DGS_ERR_INVALID_ARGUMENT, before any device work:
 * P < 0, a bad size, K out of range, K > 0 without masks or without acc, a null state buffer while P > 0 (binning_buffer may
 * be NULL when R == 0), every output NULL.  No scratch, no host read, no memset; one launch on `stream`: capturable.
 */
#define F3DGS_CONTRIB_MAX_MASKS 7
int f3dgs_contributions(int P, int R, int width, int height,
                        const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                        int K, const float* masks /* K x H x W */, float* acc /* P x (K + 1) */, float* wmax /* P */,
                        float* alpha, float* median_depth, int* ids, float* id_weight /* H x W each */,
                        void* stream /* hipStream_t */);

/*
 * The label vote: f3dgs_contributions' `acc` over the one-hot masks of an integer label map, for any number of labels, in ONE
 * walk - a pixel has one label, so the (L, H, W) mask stack is never formed and the lists are not walked once per seven masks.
 * `labels` is H x W in the format F3DGS_LABELS_U8, _I32 or _I64 (below; what f3dgs_segment writes is _I64), aligned to its
 * element.  The weights w are those of f3dgs_contributions (the forward's, bit for bit).  With l = labels[p]: if 0 <= l < L -
 * compared on the full-width value - acc[g][l] += w; in every case acc[g][L] += w: a label outside [0, L) belongs to no class
 * but counts in the weight total.  acc: (P, L + 1) floats, ADDED TO (zeroed once by the caller, accumulated over many views),
 * indexed in size_t; float atomics in a varying order, as for f3dgs_contributions.  1 <= L <= F3DGS_LABEL_VOTES_MAX_LABELS.
 * F3DGS_ERR_INVALID_ARGUMENT, before any device work: P < 0, a bad size, L out of range, an unknown format, a NULL or
 * misaligned labels, a NULL acc, a null state buffer while P > 0 (binning_buffer may be NULL when R == 0).  P == 0 or R == 0:
 * returns F3DGS_OK without touching the device.  No scratch, no host read, no memset; one launch on `stream`: capturable.
 */
#define F3DGS_LABEL_VOTES_MAX_LABELS 65536
int f3dgs_label_votes(int P, int R, int width, int height,
                      const char* geom_buffer, const char* binning_buffer, const char* image_buffer,
                      const void* labels /* H x W */, int labels_format /* F3DGS_LABELS_U8 | _I32 | _I64 */, int L,
                      float* acc /* P x (L + 1), ADDED TO */, void* stream /* hipStream_t */);

/*
 * Association of one view's instances with the 3D instances built so far (no counterpart in the reference).  A segmenter such
 * as SAM numbers its masks afresh in every view; these two calls carry the ids of M view masks over to L global instance slots,
 * on dense matrices alone (no tile list is touched).
 *   acc_view  (P, M + 1) floats: what f3dgs_label_votes wrote for this view with L = M (column M: the weight total)
 *   acc       (P, L + 1) floats: the global accumulator, laid out alike (column L: the weight total)
 *   count     a DEVICE int32: the instance slots in use, 0 <= count <= L; updated by the call
 *   dropped   a DEVICE int32, INCREASED by the number of masks that found no free slot
 * f3dgs_instance_associate.  Only Gaussians with acc_view[g][M] > 0 (seen in this view) take part.
 *   3D label  gl[g] = the lowest index of the largest of acc[g][0..L), or -1 when that maximum is <= 0
 *   table     T, (M + 1) x (L + 1) floats, an OUTPUT, fully written: T[m][c] += acc_view[g][m] for m < M with c = gl[g], or c = L
 *             when gl[g] == -1; row M receives max(0, acc_view[g][M] - sum_m acc_view[g][m]), the weight under no mask, formed
 *             per Gaussian in fp32 in ascending m.  Float atomics in a varying order: not bit-reproducible between runs
 *   score     in double from T, for m < M and l < count: row[m] = sum over l < L of T[m][l] (weight on still-unlabelled
 *             Gaussians, column L, does not count against a mask), rowall[m] the same with column L, col[l] = sum over
 *             m <= M of T[m][l] (an instance's weight that no mask covers does count),
 *             iou[m][l] = T[m][l] / ((row[m] + col[l]) - T[m][l]), 0 where the denominator is 0
 *   match     best_label[m] = the lowest l of the largest iou[m][.], -1 when that is 0; best_iou[m] that value (M doubles).  m
 *             claims best_label[m] if best_iou[m] >= iou_thresh; an instance accepts its claimant of largest IoU, the lowest m
 *             among equals: mapping[m] = l
 *   new       every other m with rowall[m] > min_weight takes count, count + 1, ... in ascending m while ids remain below L;
 *             those left over get mapping[m] = -1 and are counted in `dropped`; a mask with rowall[m] <= min_weight gets -1
 *             and is not counted.  The first view (count = 0) is no special case: every mask is new.
 * `scratch`: f3dgs_instance_scratch_bytes(M, L) bytes, 16-byte aligned, uninitialised.  Six launches on `stream` (the table is
 * cleared by a kernel), no host read, no memset, no allocation: capturable.  P == 0 (acc_view and acc may then be NULL): one
 * launch that writes the outputs of an empty table - T = 0, every mask unmatched, count and dropped as they were.
 * f3dgs_instance_merge.  For every Gaussian with acc_view[g][M] > 0: acc[g][mapping[m]] += acc_view[g][m] for every m whose
 * mapping[m] lies in [0, L) (any other entry is ignored), and acc[g][L] += acc_view[g][M].  `mapping` (M int32, device) is
 * associate's or the caller's own; it may repeat a target (two masks joined by hand), then both are added.  An injective mapping
 * gives one plain fp32 add per element: the bits of acc + acc_view; with repeated targets the adds of a row are float atomics.
 * clear_view != 0: the elements of acc_view that were read as non-zero (the total included) are written back as zeros, so that
 * the buffer a vote filled is all zero again for the next view's vote without a memset of the whole of it.  One launch.
 * F3DGS_ERR_INVALID_ARGUMENT, before any device work: P < 0, M outside 1 .. F3DGS_INSTANCE_MAX_MASKS, L outside
 * 1 .. F3DGS_INSTANCE_MAX_INSTANCES, a NULL pointer (acc_view / acc only while P > 0), a misaligned scratch, an iou_thresh or
 * min_weight that is negative or NaN.
 */
#define F3DGS_INSTANCE_MAX_MASKS 1024
#define F3DGS_INSTANCE_MAX_INSTANCES 4096
size_t f3dgs_instance_scratch_bytes(int M, int L);
int f3dgs_instance_associate(int P, int M, int L, const float* acc_view /* P x (M + 1) */, const float* acc /* P x (L + 1) */,
                             double iou_thresh, double min_weight, int32_t* count, int32_t* dropped, int32_t* mapping /* M */,
                             int32_t* best_label /* M */, double* best_iou /* M */, float* table /* (M + 1) x (L + 1) */,
                             void* scratch, void* stream /* hipStream_t */);
int f3dgs_instance_merge(int P, int M, int L, float* acc_view /* P x (M + 1) */, int clear_view, const int32_t* mapping /* M */,
                         float* acc /* P x (L + 1), ADDED TO */, void* stream /* hipStream_t */);

/*
 * Forward-only counterpart (the inference side, render.py:169-171, :137-139, :294-296): the rendered feature map (C,H,W)
 * is resized (bilinear, align_corners=True) to (Hg,Wg) and - if weight / bias are given - decoded by the 1x1 conv into
 * `out` (Cout,Hg,Wg), fp32 or (out_is_half != 0) IEEE fp16 as render.py stores it.  Without a decoder Cout must equal C.
 * With a decoder C must be 32, 64 or 128.  `scratch`: f3dgs_feature_decode_scratch_bytes(...) bytes (0 without a decoder).
 * With a decoder `weight` and `scratch` must be 16-byte aligned ("Alignment" above): F3DGS_ERR_INVALID_ARGUMENT otherwise.
 */
size_t f3dgs_feature_decode_scratch_bytes(int C, int Hg, int Wg, int has_decoder);
int f3dgs_feature_decode(int C, int H, int W, int Cout, int Hg, int Wg, const float* feature_map, const float* weight,
                         const float* bias, void* out, int out_is_half, void* scratch, void* stream);

/*
 * Open-vocabulary segmentation of a rendered view (render.py:168-180 followed by encoders/lseg_encoder/segmentation.py:526-540):
 * the rendered feature map (C,H,W) is resized (bilinear, align_corners=True) to (Hs,Ws), decoded by the 1x1 conv if weight /
 * bias are given (the values of f3dgs_feature_decode, bit for bit), with F3DGS_SEGMENT_ROUND_HALF rounded to IEEE fp16 and back
 * (render.py stores the map as fp16, and that rounding decides labels), and every pixel's Cout-vector D is scored against the
 * K rows of `text` (K x Cout fp32): score_k = (D . t_k / ||t_k||) / ||D||, labels = argmax_k score_k (int64, Hs*Ws), `score`
 * (NULL or Hs*Ws floats) the winning score.  All arithmetic is fp32.  NaN counts as the maximum and the lowest index wins a
 * tie (torch.max): a pixel of zero norm or with a non-finite value gets label 0 and score NaN.  Neither the decoded
 * (Cout,Hs,Ws) map nor the (Hs*Ws,K) logits are ever written to memory.  F3DGS_SEGMENT_TEXT_NORMALIZED: the rows of `text`
 * are already t / ||t|| and are used as they are.  `text` is never modified.
 * With a decoder C must be 32, 64 or 128 and Cout a multiple of 32; without one (weight == bias == NULL) Cout must equal C,
 * any C >= 1, and (Hs,Ws) == (H,W) is no resize at all: every pixel is scored as it is (an already decoded map).
 * 1 <= K <= F3DGS_SEGMENT_MAX_TEXTS.  Other shapes: F3DGS_ERR_UNSUPPORTED.  `scratch`:
 * f3dgs_segment_scratch_bytes(...) bytes (the resized map with a decoder, and the normalised text).  No host read, no memset,
 * no allocation; every launch goes to `stream`: capturable.  Hs * Ws == 0 is a no-op.
 */
#define F3DGS_SEGMENT_ROUND_HALF 0x1
#define F3DGS_SEGMENT_TEXT_NORMALIZED 0x2
#define F3DGS_SEGMENT_MAX_TEXTS 256
size_t f3dgs_segment_scratch_bytes(int C, int Cout, int Hs, int Ws, int K, int has_decoder);
int f3dgs_segment(int C, int H, int W, int Cout, int Hs, int Ws, int K, const float* feature_map, const float* weight,
                  const float* bias, const float* text /* K x Cout */, int flags, int64_t* labels /* Hs*Ws */,
                  float* score /* Hs*Ws or NULL */, void* scratch, void* stream /* hipStream_t */);

/*
 * Segmentation scores of N rendered views (the scoring half of the semantic-segmentation evaluation:
 * encoders/lseg_encoder/segmentation_metric.py:58-108 calculate_accuracy, calculate_accuracy_mask, calculate_iou,
 * calculate_iou_mask, called per view at :818-832), in one launch chain.  `teacher`, `student` and the optional `gt` (NULL: the
 * gt-dependent results are not produced) are N x H x W label maps, contiguous, each in its own format F3DGS_LABELS_U8 (what a
 * label PNG holds), _I32 or _I64 (what f3dgs_segment writes); a base pointer needs the alignment of its element only (a sliced
 * tensor): whole aligned groups of four elements are read by vector loads, the ends of the block element by element.
 * L label slots, 1 <= L <= F3DGS_SEGMENT_MAX_TEXTS.  A pixel is VALID when each of its labels in the maps given lies in [0, L) -
 * compared on the full-width value, before it is narrowed or used as an index; any other pixel counts in `invalid` and in
 * nothing else.  Over the valid pixels of view n, with match := (gt == teacher), all integers:
 *   n_t[i], n_s[i], n_g[i]   teacher == i, student == i, gt == i            n_ts[i]   teacher == i and student == i
 *   m_g[i], m_s[i], m_gs[i]  match and gt == i; match and student == i; match and gt == i and student == i
 *   valid, equal, invalid, matched, correct   valid pixels; teacher == student; pixels left out; match; match and student == gt
 * `counters` (f3dgs_seg_metrics_scratch_bytes(N, L, gt != NULL) bytes, uninitialised, 8-byte aligned; it is cleared by a kernel)
 * holds them after the call: int64 counts[A][N + 1][L] with the arrays in the order n_t, n_s, n_ts (A = 3) and, with gt, n_g,
 * m_g, m_s, m_gs (A = 7), followed by int64 scalars[5][N + 1] in the order valid, equal, invalid, matched, correct (the last two
 * stay 0 without gt).  Row N is the POOLED row: the label-wise sums of the counters over the N views, plus - if given - those of
 * earlier calls, `carry_counts` (A x L) and `carry_scalars` (5), both NULL or both given: a test set of views of several sizes
 * is pooled by chaining its calls.  Per row, views and the pooled one, in fp64:
 *   scores[0][row] accuracy = equal / valid            scores[2][row] accuracy_masked = correct / matched      (0 / 0 = NaN, as
 *   scores[1][row] iou                                 scores[3][row] iou_masked                                the reference)
 *   iou:        the labels ranked by n_t + n_s, descending, THE LOWER LABEL FIRST AMONG EQUAL COUNTS (the reference's argsort
 *               leaves that order open); kept are the first `num_classes` whose count is not zero; iou_i = n_ts / (n_t + n_s -
 *               n_ts); the mean of the kept values that are not NaN, added in rank order, NaN when there is none
 *   iou_masked: ranked by n_g + n_t + n_s; iou_i = m_gs / (m_g + m_s - m_gs), a union of 0 gives NaN and the label is skipped
 *               (np.nanmean)
 * `scores` is [2 K][N + 1], `iou_per_label` [K][N + 1][L] (NaN where the label did not make the cut) and `labels_ranked`
 * [K][N + 1][num_classes] (the kept labels in rank order, padded with -1), K = 2 with gt (second half: the masked ranking), else 1.
 * All three NULL: the counters alone.  1 <= num_classes <= L (the reference: 7).
 * F3DGS_ERR_UNSUPPORTED: L outside 1..256, H W >= 2^31, N > 65536 views in one call.  F3DGS_ERR_INVALID_ARGUMENT: bad sizes, num_classes out of
 * range, an unknown format, a NULL teacher, student or counters, a pointer off its element's alignment, only some of the three
 * outputs or only one carry pointer.  N == 0 is a no-op.  Integer atomics only (32-bit in LDS per workgroup, 64-bit to memory: a
 * pooled row may pass 2^32): two calls give identical bits.  No host read, no memset; three launches on `stream`: may be captured.
 *
 * f3dgs_seg_colorize: the palette pictures of a label map (segmentation.py:547-559).  `labels` N x H x W in any of the three
 * formats, `palette` L x 3 uint8 on the device, `fill` NULL (black) or 3 bytes in HOST memory: the colour of a label outside
 * [0, L).  `out` is uint8 N x H x W' x 3:
 *   F3DGS_SEG_COLOR_MASK   W' = W     palette[label]
 *   F3DGS_SEG_COLOR_BLEND  W' = W     trunc(255 (a img + b mask)), mask = palette / 255, `image` N x 3 x H x W fp32 in [0, 1]
 *   F3DGS_SEG_COLOR_STRIP  W' = 3 W   [trunc(255 img) | blend | mask], the reference's `_vis.png`
 * in the reference's fp32 chain, one rounding per operation and nothing fused: mask = byte / 255.0f, img * a + mask * b,
 * (uint8) clamp(v * 255.0f, 0, 255), truncated.  The reference casts without the clamp: the clamp only defines images outside
 * [0, 1] (NaN gives 0).  `image` may be NULL for the mask.  Errors as above (L: F3DGS_ERR_UNSUPPORTED; an unknown mode or
 * format, a NULL labels, palette, out or needed image: F3DGS_ERR_INVALID_ARGUMENT).  No scratch, no host read, no memset; one
 * launch on `stream`: may be captured.
 */
#define F3DGS_LABELS_U8 0
#define F3DGS_LABELS_I32 1
#define F3DGS_LABELS_I64 2
#define F3DGS_SEG_COLOR_MASK 0
#define F3DGS_SEG_COLOR_BLEND 1
#define F3DGS_SEG_COLOR_STRIP 2
size_t f3dgs_seg_metrics_scratch_bytes(int N, int L, int has_gt);
int f3dgs_seg_metrics(int N, int H, int W, int L, int num_classes, const void* teacher, int teacher_format, const void* student,
                      int student_format, const void* gt /* or NULL */, int gt_format,
                      const int64_t* carry_counts /* A x L or NULL */, const int64_t* carry_scalars /* 5 or NULL */,
                      int64_t* counters, double* scores, double* iou_per_label, int64_t* labels_ranked,
                      void* stream /* hipStream_t */);
int f3dgs_seg_colorize(int N, int H, int W, int L, const void* labels, int labels_format, const unsigned char* palette /* L x 3 */,
                       const float* image /* N x 3 x H x W or NULL */, int mode, float a, float b,
                       const unsigned char* fill /* host, 3 bytes, or NULL */, unsigned char* out, void* stream /* hipStream_t */);

/*
 * SAM mask post-processing: everything between the mask decoder's low-resolution logits and the list of mask records
 * (encoders/sam_encoder/segment_anything: modeling/sam.py:133-162 postprocess_masks, utils/amg.py calculate_stability_score,
 * batched_mask_to_box, is_box_near_crop_edge, uncrop_masks, mask_to_rle_pytorch, automatic_mask_generator.py:295-320; and
 * torchvision's batched_nms).  The networks are not part of this library.
 *
 * f3dgs_sam_masks: `low_res` M x h x w fp32 logits.  Per pixel of the H x W crop the reference's value v: resize h x w -> S x S,
 * keep [:ih, :iw], resize -> H x W, both by PyTorch's upsample_bilinear2d with align_corners = False in fp32, one rounding per
 * operation: scale = (float)in / out, src = max(scale * (dst + 0.5f) - 0.5f, 0), i1 = i0 + (i0 < in - 1),
 * l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d); the two stages stay two fp32 results.  v is never stored.  Per mask m:
 *   counts[m]    = {n_hi, n_lo, area}: the pixels with v > t_hi, v > t_lo, v > t (the caller rounds t + offset and t - offset to fp32)
 *   box[m]       = XYXY min / max of the columns and rows with a set pixel, in the crop's frame; {0, 0, 0, 0} for an empty mask
 *   box_frame[m] = box + (cx0, cy0, cx0, cy0)
 *   stability[m] = (float)n_hi / (float)n_lo, IEEE; 0 / 0 = NaN
 *   packed       M x FW x ceil(FH / 32) words, the mask v > t in the FULL FH x FW frame, column-major: word (x, y / 32) holds rows
 *                32 (y / 32) .. + 31 of column x, bit = row % 32; rows >= FH and everything outside the crop (its origin
 *                (cx0, cy0), its size H x W, inside the frame) are zero.  Every word is written: no clear is needed.
 *   keep[m]      = iou ok and (stability_thresh <= 0 or stability >= stability_thresh) and not (edge_filter and near the crop's
 *                edge): a box coordinate within 20 of the crop's but not within 20 of the frame's (is_box_near_crop_edge)
 *   kept_index   the m with keep[m], ascending, then -1; *kept_count their number
 * iou ok: pred_iou_thresh <= 0 or iou_preds == NULL, or iou_preds[m] > pred_iou_thresh (strict; NaN fails).  A mask that fails
 * is skipped: its workgroups write zero words and return, its counts are 0, its box 0, its stability NaN.
 * `scratch`: f3dgs_sam_masks_scratch_bytes(M) bytes, 4-byte aligned, uninitialised.  Three launches (two for M == 0, which gives
 * *kept_count = 0), integer atomics only: two calls give identical bits.  No host read, no memset: may be captured.
 * F3DGS_ERR_INVALID_ARGUMENT: bad sizes, ih or iw > S, a crop outside the frame, a NULL pointer.  F3DGS_ERR_UNSUPPORTED: M > 65535,
 * a size > 32768, FH FW > 2^30.
 *
 * f3dgs_sam_upscale: the same v for every pixel, stored: `out` M x H x W fp32, or with out_bool bytes v > t (the drop-in for
 * postprocess_masks and the threshold that follows it).  One launch.
 *
 * f3dgs_box_nms: greedy non-maximum suppression of M <= F3DGS_BOX_NMS_MAX boxes GIVEN IN SCORE ORDER (`boxes` M x 4 fp32 XYXY,
 * best first): box j is suppressed when an earlier KEPT box i of the same category (`categories` M int32 or NULL: all one) has
 * IoU > iou_threshold (strict), IoU = inter / (area_i + area_j - inter) in fp32 with an IEEE division, inter from widths clamped
 * at 0, no +1; a NaN quotient (two empty boxes) never suppresses.  `keep` receives the kept positions in score order - order[i]
 * instead of i where `order` (M int32, the sort's permutation) is given - then -1; *count their number.  `scratch`:
 * f3dgs_box_nms_scratch_bytes(M) bytes (the M x ceil(M / 64) suppression words), 8-byte aligned.  Two launches, no host read.
 *
 * f3dgs_mask_rle_count / _emit: the reference's uncompressed RLE of K packed masks (`index` K int32 rows of `packed`, or NULL:
 * rows 0 .. K - 1): runs down the columns, continuing across column ends, a leading 0 where pixel (0, 0) is set.  _count writes
 * lens[k], the number of counts of mask k.  _emit takes `ends`, the INCLUSIVE prefix sums of lens (int64), and writes the counts
 * of mask k to out[ends[k] - lens[k] ..) where they end within `capacity` entries (a mask that does not fit is left out whole:
 * the caller compares ends[K - 1] with capacity).  f3dgs_mask_unpack: K x FH x FW bytes 0 / 1.  One launch each.
 *
 * f3dgs_mask_instance_map: the painter's picture of K packed masks (encoders/sam_encoder/segment.py:57-70 show_anns, which
 * paints the masks in the caller's order, later over earlier): out[y][x] (FH x FW int32, row-major) is the largest j < K whose
 * mask index[j] (mask j without an index; rows may repeat) has bit (x, y) set, -1 where none has.  K == 0 writes all -1 (packed
 * may then be NULL).  One launch, no host read.  F3DGS_ERR_INVALID_ARGUMENT: bad sizes, a NULL out, a NULL packed with K > 0.
 *
 * f3dgs_mask_regions: utils/amg.py remove_small_regions (automatic_mask_generator.py:325-373 calls it twice per mask) of K packed
 * masks (`index` as above; `packed` is only read).  `holes` != 0 labels the background (clear bits of rows < FH), 0 the foreground,
 * with 8-connectivity; a component is small when its area < area_thresh (strict, a double).  `changed`[k] = 1 iff mask k has a
 * small component.  `out` K x FW x ceil(FH / 32) words: with holes the mask OR its small background components (the outer
 * background included); without, the mask without its small components - but where EVERY component is small the largest stays
 * (`changed` is 1 all the same); ties for the largest go to the component whose first pixel comes first in row-major order.
 * Rows >= FH of `out` are zero whatever `packed` holds there.  area[k] = the set pixels of out[k], box[k] (K x 4) its XYXY
 * min / max columns and rows, {0, 0, 0, 0} when empty: both come from the launch that writes the words.
 * No dense label image: the nodes are the maximal vertical runs of the labelled polarity within a column, 16 bytes each, joined
 * by a union-find of integer atomics whose roots are the smallest run of a component; two calls give identical bits.
 * `scratch`: f3dgs_mask_regions_scratch_bytes(K, FW, run_capacity) bytes, 8-byte aligned, uninitialised.  *runs (a HOST int64)
 * receives the number of runs; where it exceeds run_capacity NOTHING is written to out, changed, area or box and the call
 * returns F3DGS_OK: the caller compares and comes again with room (a blob has about 2 runs per column, its background about 2 FW).
 * Seven launches (six for FW == 1), then ONE host read (the total and the error word together: the call synchronises `stream`
 * and cannot be captured).  Every loop is bounded by construction; the walks of the union-find also carry a cap of the number
 * of runs, and a walk that reaches it makes the call return F3DGS_ERR_HIP.  F3DGS_ERR_INVALID_ARGUMENT: bad sizes, area_thresh
 * negative or not finite, a NULL pointer, a misaligned scratch.  F3DGS_ERR_UNSUPPORTED: K > 65535, an edge > 32768,
 * FH FW > 2^30, run_capacity >= 2^31.
 */
#define F3DGS_BOX_NMS_MAX 16384
size_t f3dgs_sam_masks_scratch_bytes(int M);
int f3dgs_sam_masks(int M, int h, int w, int S, int ih, int iw, int H, int W, int FH, int FW, int cx0, int cy0, const float* low_res,
                    const float* iou_preds /* M or NULL */, float pred_iou_thresh, float t, float t_hi, float t_lo,
                    float stability_thresh, int edge_filter, uint32_t* packed, int32_t* counts /* M x 3 */, int32_t* box /* M x 4 */,
                    int32_t* box_frame /* M x 4 */, float* stability, unsigned char* keep, int32_t* kept_index, int32_t* kept_count,
                    void* scratch, void* stream /* hipStream_t */);
int f3dgs_sam_upscale(int M, int h, int w, int S, int ih, int iw, int H, int W, const float* low_res, float t, int out_bool, void* out,
                      void* stream /* hipStream_t */);
size_t f3dgs_box_nms_scratch_bytes(int M);
int f3dgs_box_nms(int M, const float* boxes, const int32_t* categories /* or NULL */, float iou_threshold,
                  const int32_t* order /* or NULL */, int32_t* keep, int32_t* count, void* scratch, void* stream /* hipStream_t */);
int f3dgs_mask_rle_count(int K, int FH, int FW, const uint32_t* packed, const int32_t* index /* or NULL */, int32_t* lens,
                         void* stream /* hipStream_t */);
int f3dgs_mask_rle_emit(int K, int FH, int FW, const uint32_t* packed, const int32_t* index /* or NULL */, const int32_t* lens,
                        const int64_t* ends, int64_t capacity, int32_t* out, void* stream /* hipStream_t */);
int f3dgs_mask_unpack(int K, int FH, int FW, const uint32_t* packed, const int32_t* index /* or NULL */, unsigned char* out,
                      void* stream /* hipStream_t */);
int f3dgs_mask_instance_map(int K, int FH, int FW, const uint32_t* packed, const int32_t* index /* or NULL */,
                            int32_t* out /* FH x FW, row-major */, void* stream /* hipStream_t */);
size_t f3dgs_mask_regions_scratch_bytes(int K, int FW, int64_t run_capacity);
int f3dgs_mask_regions(int K, int FH, int FW, const uint32_t* packed, const int32_t* index /* or NULL */, int holes, double area_thresh,
                       int64_t run_capacity, uint32_t* out, unsigned char* changed, int32_t* area, int32_t* box /* K x 4 */,
                       int64_t* runs /* host */, void* scratch, void* stream /* hipStream_t */);

/*
 * PCA colour image of a feature map (render.py:38-53, feature_visualize_saving), in two calls around a C x C eigenproblem
 * that is the caller's (feature_pca.py solves it with torch.linalg.eigh in float64).  The (C,HW) map is read by kernels only
 * and nothing of size C*HW is allocated.
 * f3dgs_feature_pca_moments: the samples are pixels 0, stride, 2 stride, ... of the flattened map, n = ceil(HW / stride) of
 * them (the reference: stride 3), each divided by max(its L2 norm, 1e-12) in fp32 (F.normalize: a zero pixel stays zero).
 * `mean` (C doubles) receives their mean and `cov` (C x C doubles, symmetric, both triangles written) the covariance
 * sum (x - mean)(x - mean)^T / (n - 1).  The samples are centred BEFORE they are contracted (a first pass forms the mean), the
 * contraction runs on v_mfma_f32_32x32x2_f32 over upper-triangle block pairs with the fp32 accumulator emptied into float64
 * every 256 samples, and all other sums are float64.  No floating-point atomics: two calls give identical bits.
 * `scratch`: f3dgs_feature_pca_scratch_bytes(C, HW, stride) bytes: 4 n for the norms, 8 C per 16384 samples for the partial
 * sums, 12 C, and the float64 partial blocks of the contraction, min(ceil(n / 1024), max(1, 1024 / pairs)) x pairs x 32 KB with
 * pairs = nb (nb + 1) / 2, nb = ceil(C / 64).  That last part follows C, not HW: at most 32 MB up to 2048 channels and 68 MB at
 * 4096 (half of `cov` itself), a few per cent of a map of image size, but MORE than a small map of many channels (C = 512 at
 * 36 x 48: 1.15 MB, the map 3.5 MB, `cov` 2 MB).  "Nothing of size C*HW" is a statement about maps that are larger than C x C.
 * f3dgs_feature_pca_project: t_k(p) = (x_p / max(||x_p||, 1e-12) - mean) . components[k], k = 0, 1, 2, for EVERY pixel p in one
 * pass; `mean` (C floats) and `components` (3 x C floats) are device pointers.  With `lo` / `hi` (device floats, both or
 * neither) `out` (HW x 3 floats, pixel-major) receives clamp((t - lo) / (hi - lo), 0, 1), with both NULL the raw t.
 * C < 3, C > F3DGS_FEATURE_PCA_MAX_CHANNELS, stride < 1, fewer than 3 samples or HW > 2^30: F3DGS_ERR_UNSUPPORTED.  HW == 0 is
 * a no-op.  No host read, no memset, no allocation; every launch goes to `stream`: capturable.
 */
#define F3DGS_FEATURE_PCA_MAX_CHANNELS 4096
size_t f3dgs_feature_pca_scratch_bytes(int C, long long HW, int stride);
int f3dgs_feature_pca_moments(int C, long long HW, int stride, const float* feature_map, double* mean /* C */,
                              double* cov /* C x C */, void* scratch, void* stream /* hipStream_t */);
int f3dgs_feature_pca_project(int C, long long HW, const float* feature_map, const float* mean /* C */,
                              const float* components /* 3 x C */, const float* lo, const float* hi /* device, or both NULL */,
                              float* out /* HW x 3 */, void* stream /* hipStream_t */);

/*
 * The viewer's render modes of a rendered view (utils/image_utils.py:60-161, render_net_image; callers view.py:25 and
 * train.py:164): 'Normal', 'Edge', 'Curvature' and the palette-coloured frame of any one-channel map ('Depth' included).
 * f3dgs_view_normals: depth_to_normal.  Per pixel (y,x) the world points of (y,x), (y+1,x) and (y,x+1) are formed as
 * unproject_depth_map does - X = x / (W-1) * 2 - 1, Y = y / (H-1) * 2 - 1 (pixel indices, not centres), sdepth =
 * (f1 d + f2) / (d + 1e-8) with f1 = proj[2][2], f2 = proj[3][2] of the reference's (transposed) projection_matrix, the row
 * vector (X, Y, sdepth, 1) times `inv_full_proj`, the divide by w - and n = cross(p2 - p1, p3 - p1) / (|.| + 1e-8).  The
 * unprojection and the two differences are FLOAT64 (the reference's float32 chain leaves errors of order 1 on some normals;
 * the judge of this function is the reference's formula in float64), cross product and normalisation float32.  `proj`: 16
 * floats, `inv_full_proj`: 16 DOUBLES, the inverse of full_proj_transform, row-major, both device pointers (view_modes.py:
 * torch.linalg.inv in float64 on the map's device).  Points of row H and column W are the zero vector (the reference pads
 * with zeros): the last row and column are computed against it and the corner pixel's normal is 0.  A depth of 0 is a value
 * like any other.  `out`: H x W x 3 floats, or 3 x H x W with F3DGS_VIEW_NORMALS_CHW; with F3DGS_VIEW_NORMALS_HALF the value
 * written is (n + 1) / 2, the image of the 'Normal' mode.  H == 1 or W == 1 (a division by zero in the reference):
 * F3DGS_ERR_UNSUPPORTED.
 * f3dgs_view_gradient: gradient_map.  image (Cn,H,W), any Cn >= 1; per channel gx, gy with the taps [[-1,0,1],[-2,0,2],
 * [-1,0,1]] / 4 and their transpose, ZEROS outside the image; out (H x W) = sqrt(sum over channels of gx^2 + gy^2).
 * f3dgs_view_curvature: f3dgs_view_gradient of the 3 x H x W, (n + 1) / 2 output of f3dgs_view_normals, bit for bit, in one
 * kernel: the normal image never reaches memory.  (Outside the image that image is 0, not 0.5, as in the reference.)
 * `minmax` of both (NULL, or two floats on the device): receives the minimum and the maximum of `out`.  f3dgs_view_minmax
 * does the same for any field of n floats (a raw depth map).  The values are exactly those of the field (of torch.aminmax)
 * for a field without NaN, -0 reported as +0; integer atomics only: two calls give identical bits.  Each of the three sets
 * the slot to (+inf, -inf) by a one-thread launch in front of its kernel.
 * f3dgs_view_palette: index -> row of `lut` (L x 3 floats, device; the library ships no palette).  F3DGS_VIEW_PALETTE_MINMAX
 * is the reference's `colormap`: idx = rint((v - min) / (max - min) * (L-1)) in float32, halves to even (torch.round; L = 256
 * there); max == min, 0/0 in the reference, gives index 0 everywhere.  F3DGS_VIEW_PALETTE_MAX is render.py:155-161
 * (matplotlib's float call): idx = min(int(v / max * L), L-1), negative values index 0; max == 0 gives index 0.  A NaN
 * indexes 0.  `minmax` is the two-float device slot.  `out_float` (3 x HW, or NULL) receives the colour, `out_u8` (HW x 3
 * bytes, pixel-major, or NULL) what view.py:26 sends: clamp(c, 0, 1) * 255 truncated.  f3dgs_view_bytes is that last step for
 * an image (3 x HW floats) that needs no palette.
 * H * W (HW, n) > 2^30, L < 2, L > F3DGS_VIEW_PALETTE_MAX_ENTRIES: F3DGS_ERR_UNSUPPORTED.  H * W == 0 is a no-op.  No host
 * read, no memset, no allocation; every launch goes to `stream`: capturable.  Workgroups cover F3DGS_VIEW_TILE^2 pixels.
 */
#define F3DGS_VIEW_TILE 16
#define F3DGS_VIEW_NORMALS_CHW 0x1
#define F3DGS_VIEW_NORMALS_HALF 0x2
#define F3DGS_VIEW_PALETTE_MINMAX 0
#define F3DGS_VIEW_PALETTE_MAX 1
#define F3DGS_VIEW_PALETTE_MAX_ENTRIES 4096
int f3dgs_view_normals(int H, int W, const float* depth, const float* proj /* 4 x 4 */, const double* inv_full_proj /* 4 x 4 */,
                       float* out, int flags, void* stream /* hipStream_t */);
int f3dgs_view_gradient(int Cn, int H, int W, const float* image, float* out /* H x W */, float* minmax /* 2, or NULL */,
                        void* stream /* hipStream_t */);
int f3dgs_view_curvature(int H, int W, const float* depth, const float* proj, const double* inv_full_proj, float* out /* H x W */,
                         float* minmax /* 2, or NULL */, void* stream /* hipStream_t */);
int f3dgs_view_minmax(long long n, const float* field, float* minmax /* 2 */, void* stream /* hipStream_t */);
int f3dgs_view_palette(long long HW, const float* field, const float* minmax /* 2 */, const float* lut /* L x 3 */, int L, int mode,
                       float* out_float /* 3 x HW, or NULL */, uint8_t* out_u8 /* HW x 3, or NULL */, void* stream /* hipStream_t */);
int f3dgs_view_bytes(long long HW, const float* image /* 3 x HW */, uint8_t* out_u8 /* HW x 3 */, void* stream /* hipStream_t */);

/*
 * One torch.optim.Adam step (no weight decay, no amsgrad: the reference's configuration,
 * scene/gaussian_model.py:163-178) over one tensor of n floats, in place; `step` is the 1-based step count of that
 * tensor.  param / grad / exp_avg / exp_avg_sq are device pointers.
 */
int f3dgs_adam_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                    double beta2, double eps, int step, void* stream /* hipStream_t */);
/*
 * The same step restricted to the rows (of `width` floats) whose row_mask byte is non-zero: the other rows keep
 * parameter and moments untouched.  An EXTENSION (row f-4's "sparse-aware Adam using radii > 0"), not the reference's
 * optimizer: torch.optim.Adam also moves never-visible Gaussians by their decaying first moment.  row_mask == NULL is
 * f3dgs_adam_step.
 */
int f3dgs_adam_step_rows(size_t n, size_t width, const uint8_t* row_mask, float* param, const float* grad, float* exp_avg,
                         float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int step,
                         void* stream /* hipStream_t */);

/*
 * The same update over SEVERAL tensors in ONE launch (the reference steps the seven per-Gaussian tensors with torch's
 * foreach kernels, scene/gaussian_model.py:163-178): a table of up to F3DGS_ADAM_MAX_TENSORS entries, each with its own
 * learning rate and step count (torch keeps them per parameter); beta1 / beta2 / eps are shared.  `row_mask` (optional,
 * `rows` bytes): the visibility-masked variant of f3dgs_adam_step_rows, applied to every tensor whose `n` is a multiple of `rows`.
 * The table carries no per-tensor flag: with a mask, EVERY entry whose `n` is a whole multiple of `rows` (n = 0 apart) is
 * taken as `rows` rows of n / rows floats, also one that is not per-row data and only happens to have such a length; the
 * others are stepped densely.  A caller who holds such a tensor steps it with f3dgs_adam_step instead (FusedAdam does:
 * it puts a tensor into a masked table only if its first dimension is the mask's length).
 * Errors (F3DGS_ERR_INVALID_ARGUMENT, nothing launched): n_tensors outside 0 .. F3DGS_ADAM_MAX_TENSORS, a null table, an
 * entry with n > 0 and a null pointer or step < 1, a mask with rows == 0.  f3dgs_adam_step[_rows]: a null pointer with
 * n > 0, step < 1, a mask whose width is 0 or does not divide n.
 */
#define F3DGS_ADAM_MAX_TENSORS 16
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    size_t n;        /* elements */
    double lr;
    int step;        /* counts from 1 */
} f3dgs_adam_tensor;
int f3dgs_adam_step_multi(int n_tensors, const f3dgs_adam_tensor* tensors /* host array */, double beta1, double beta2, double eps,
                          const uint8_t* row_mask, size_t rows, void* stream);

/*
 * The capturable optimizer step (ABI 3.24): the same update with step counts, learning rates and the two bias-correction
 * constants held on the DEVICE, so that a launch captured in a HIP graph does the step of the replay it runs in, not of the
 * step it was captured at.  Two launches, in this order on one stream:
 *
 * f3dgs_adam_schedule: one wave; entry k of the table (n > 0) gets
 *   t = *step + 1, stored back to *step (a float32 word, the layout of torch.optim.Adam(capturable=True): exact up to 2^24)
 *   lr = scheduled ? schedule(i) : *lr, where i is the iteration this step belongs to: *iteration + 1 with `advance` != 0 (one
 *        lane then stores i to *iteration, after every entry has read the word), *iteration itself with advance == 0 (the second
 *        table of a step whose first table advanced the word)
 *   consts[k] = { lr, (float)(lr / (1 - beta1^t)), (float)(1 / sqrt(1 - beta2^t)) }: both constants formed in fp64 and rounded
 *        once, as f3dgs_adam_step_multi forms them on the host
 *   schedule(i) = 0 if lr_init == lr_final == 0, otherwise delay * exp(log(lr_init) (1 - u) + log(lr_final) u) with
 *        u = clip(i / max_steps, 0, 1) and delay = lr_delay_mult + (1 - lr_delay_mult) sin(pi/2 clip(i / lr_delay_steps, 0, 1))
 *        for lr_delay_steps > 0, else 1 (the reference's get_expon_lr_func, utils/general_utils.py:29-61), in fp64.
 *   An entry with n == 0 is left alone (step word, consts[k]); a table without any n > 0 launches nothing and advances nothing.
 *   `iteration` may be NULL if no entry is scheduled (advance is then ignored).
 *
 * f3dgs_adam_step_multi_device: f3dgs_adam_step_multi's launch, with entry k's two constants read from consts[k] (what the
 * schedule call wrote for the SAME table); `row_mask` / `rows` as there.  With equal constants it stores the same bits.
 *
 * `consts` holds F3DGS_ADAM_MAX_TENSORS entries of device memory, 8-byte aligned; step / lr / iteration words are device memory
 * too.  No host read, no memset, no allocation, no scratch: everything is enqueued on `stream`.
 * Errors (F3DGS_ERR_INVALID_ARGUMENT, nothing launched): n_tensors outside 0 .. F3DGS_ADAM_MAX_TENSORS, a null table or null
 * `consts` (n_tensors > 0), an entry with n > 0 and a null pointer, a null step word or (not scheduled) a null lr word, a
 * scheduled entry without `iteration`, a schedule with max_steps <= 0, lr_delay_steps < 0, exactly one of lr_init / lr_final
 * zero or either negative (or NaN), beta1 or beta2 outside [0, 1), a mask with rows == 0.
 */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    size_t n;                /* elements */
    float* step;             /* device: steps taken so far, as float32 */
    const double* lr;        /* device: the base rate (read if !scheduled) */
    int scheduled;           /* non-zero: the rate is the schedule below */
    double lr_init, lr_final, lr_delay_mult;
    long long lr_delay_steps, max_steps;
} f3dgs_adam_device_tensor;
typedef struct {
    double lr_now;           /* the rate this step used: for the host to read back */
    float step_size;         /* (float)(lr_now / (1 - beta1^t)) */
    float inv_sqrt_bc2;      /* (float)(1 / sqrt(1 - beta2^t)) */
} f3dgs_adam_consts;
int f3dgs_adam_schedule(int n_tensors, const f3dgs_adam_device_tensor* tensors /* host array */, double beta1, double beta2,
                        long long* iteration /* device, or NULL */, int advance, f3dgs_adam_consts* consts /* device */,
                        void* stream /* hipStream_t */);
int f3dgs_adam_step_multi_device(int n_tensors, const f3dgs_adam_device_tensor* tensors /* host array */, double beta1, double beta2,
                                 double eps, const uint8_t* row_mask, size_t rows, const f3dgs_adam_consts* consts /* device */,
                                 void* stream /* hipStream_t */);

/*
 * The reference's reset_opacity (scene/gaussian_model.py:231-234) IN PLACE, one launch over n elements:
 *   raw = logit(min(sigmoid(raw), cap)), sigmoid(x) = 1 / (1 + expf(-x)) (f3dgs_activate_forward's), logit(x) = logf(x / (1 - x))
 *   (the reference's inverse_sigmoid), fp32; a NaN stays a NaN, as through torch.min
 *   exp_avg = exp_avg_sq = 0 (each may be NULL: no optimizer state yet); a step word is not this call's business
 * The reference builds a new Parameter instead; here the addresses survive, and with them a captured iteration.
 * Errors (F3DGS_ERR_INVALID_ARGUMENT, nothing launched): raw == NULL with n > 0, cap outside (0, 1) or NaN.
 */
int f3dgs_reset_opacity(size_t n, float* raw, float* exp_avg, float* exp_avg_sq, float cap, void* stream /* hipStream_t */);

/*
 * Row movement of one densification (scene/gaussian_model.py:300-431: densify_and_clone, densify_and_split,
 * prune_points and the optimizer-state edits of cat_tensors_to_optimizer / _prune_optimizer) as ONE gather over all
 * per-Gaussian tensors.  Output row j of every tensor comes from source row src_row[j]; kind[j] says how:
 *   0 kept original (row and Adam moments copied), 1 clone (row copied, moments zero),
 *   2 split child (as a clone, but tensors in mode OVERRIDE_CHILD take row override_row[j] of `override_src`:
 *     the child's new xyz and scaling).
 * All pointers are device pointers; `dst` buffers are the caller's (capacity-sized, never the same memory as `src`).
 */
#define F3DGS_DENSIFY_COPY 0            /* parameters: always the source row */
#define F3DGS_DENSIFY_ZERO_NEW 1        /* optimizer moments: source row for kind 0, zeros for kinds 1 and 2 */
#define F3DGS_DENSIFY_OVERRIDE_CHILD 2  /* xyz, scaling: source row for kinds 0/1, override row for kind 2 */
#define F3DGS_DENSIFY_MAX_TENSORS 32
typedef struct f3dgs_densify_tensor {
    const float* src;           /* (n_in, width) */
    float* dst;                 /* (>= n_out, width) */
    const float* override_src;  /* (n_children, width) or NULL */
    int width;                  /* floats per row */
    int mode;                   /* F3DGS_DENSIFY_* */
} f3dgs_densify_tensor;
int f3dgs_densify_gather(size_t n_out, const int32_t* src_row, const uint8_t* kind, const int32_t* override_row, int n_tensors,
                         const f3dgs_densify_tensor* tensors /* host array */, void* stream /* hipStream_t */);

/*
 * The model's front end: what stands between its raw parameters and the op (scene/gaussian_model.py:98-127: the getters
 * get_scaling, get_rotation, get_opacity, get_features that every render() call runs, and what autograd mirrors of them), and the
 * densification statistics behind the op (train.py:132-133, scene/gaussian_model.py:436-438).  Each entry point is ONE launch on
 * `stream`: no host read, no memset, no allocation, no scratch - capturable.  P == 0 returns F3DGS_OK without touching the device.
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: P < 0, M < 1, a NULL input of a group whose output was requested, a
 * misaligned pointer named below.  M > 256: F3DGS_ERR_UNSUPPORTED.  Inputs are contiguous fp32 at any 4-byte alignment.
 *
 * f3dgs_activate_forward: four groups, each optional - a NULL output skips the group, and its inputs may then be NULL.
 *   scales (P,3)     = expf(raw_scaling)
 *   rotations (P,4)  = q / max(sqrt(fp32 sum of squares), 1e-12): F.normalize's formula; it does not rescale, so its overflow
 *                      and underflow are those of the fp32 sum
 *   opacities (P)    = 1 / (1 + expf(-raw_opacity))
 *   shs (P,M,3)      row i = [features_dc row i (3 floats) | features_rest row i (3 (M - 1) floats)]: a copy, bit-exact.  With
 *                      M == 1 features_rest may be NULL.
 *   `rotations` and `shs` must be 16-byte aligned ("Alignment" above: the op reads them with 16-byte loads, and they are written
 *   with 16-byte stores); the split sources are read with consecutive dwords across the wave.
 *
 * f3dgs_activate_backward: every non-NULL output is fully overwritten; a NULL upstream gradient counts as zeros (its saved
 * input may then be NULL).  `scales` and `opacities` are the forward's OUTPUTS, `raw_rotation` its input.
 *   d_raw_scaling  = dL_dscale * scales
 *   d_raw_opacity  = dL_dopacity * opacities * (1 - opacities)
 *   d_raw_rotation: with n = ||raw_rotation|| (fp32, as in the forward): n >= 1e-12: (g - h (h . g)) / n, h = q / n; otherwise
 *                   g / 1e-12 (the clamp was active)
 *   d_features_dc (P,1,3), d_features_rest (P,M-1,3): the two column ranges of dL_dsh, bit-exact; each may be NULL.  dL_dsh is
 *                   read with 16-byte loads and must be 16-byte aligned.
 *
 * f3dgs_densify_stats: for every i with radii[i] > 0
 *   xyz_gradient_accum[i] += sqrt(gx^2 + gy^2), (gx, gy) = dL_dmean2D[i][0..1]; the norm and the sum are formed in fp64 and
 *                            rounded once, so the result is the correctly rounded fp32 sum
 *   denom[i] += 1;  max_radii2D[i] = max(max_radii2D[i], (float)radii[i])
 * and rows with radii <= 0 are untouched.  Each accumulator may be NULL.  dL_dmean2D == NULL means zero gradients: denom and
 * max_radii2D still update (train_step.densification_deltas with `.grad is None`).  The call ADDS into its buffers: the per-view
 * deltas of a data-parallel step are the same call on zeroed buffers.
 */
int f3dgs_activate_forward(int P, int M, const float* raw_scaling /* (P,3) */, const float* raw_rotation /* (P,4) */,
                           const float* raw_opacity /* (P) */, const float* features_dc /* (P,1,3) */,
                           const float* features_rest /* (P,M-1,3) */, float* scales, float* rotations, float* opacities,
                           float* shs, void* stream /* hipStream_t */);
int f3dgs_activate_backward(int P, int M, const float* scales, const float* raw_rotation, const float* opacities,
                            const float* dL_dscale, const float* dL_drot, const float* dL_dopacity, const float* dL_dsh,
                            float* d_raw_scaling, float* d_raw_rotation, float* d_raw_opacity, float* d_features_dc,
                            float* d_features_rest, void* stream /* hipStream_t */);
int f3dgs_densify_stats(int P, const float* dL_dmean2D /* (P,3) or NULL */, const int32_t* radii /* (P) */,
                        float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream /* hipStream_t */);

/*
 * Replaces SimpleKNN::knn / distCUDA2 of the reference's second native module (submodules/simple-knn/
 * simple_knn.cu:45-221, spatial.cu:15-25; caller scene/gaussian_model.py:146): mean_dist2[i] = mean of the squared
 * distances from point i to its three nearest neighbours (exact; a missing neighbour counts as FLT_MAX, as there).
 * points (P,3), mean_dist2 (P) device pointers; `scratch` = f3dgs_knn_scratch_bytes(P) bytes of device memory.
 * Everything is enqueued on `stream`; nothing is read back to the host (the reference synchronises twice).
 */
size_t f3dgs_knn_scratch_bytes(int P);
int f3dgs_knn_mean_dist2(int P, const float* points, float* mean_dist2, void* scratch, void* stream /* hipStream_t */);

/*
 * The K nearest neighbours of every point WITH their indices (no counterpart in the reference, whose search returns the mean
 * distance alone), exact and uniquely defined.  points (P, 3), idx (P, K) int32, dist2 (P, K) float32 or NULL: device pointers.
 * 1 <= K <= F3DGS_KNN_MAX_NEIGHBORS.  Row i holds the K points j != i with the smallest (dist2, j) in LEXICOGRAPHIC order:
 * ascending distance, among equal distances the lower index.  Self is excluded by index, not by distance: a duplicate of
 * point i is its neighbour at distance 0.  Every distance is ((dx*dx) + (dy*dy)) + (dz*dz) with dx = candidate - query in
 * float32, one rounding per operation, so the result is a function of the inputs alone (not of the sort order, the walk order or
 * the lanes).  A slot without a neighbour (P - 1 < K) holds idx = -1 and dist2 = FLT_MAX, f3dgs_knn_mean_dist2's convention.  A
 * point with a NaN or infinite coordinate is nobody's neighbour and has none (its row is all -1); a pair whose distance
 * overflows float32 (is not < inf) is no neighbour pair either.
 * `scratch` = f3dgs_knn_neighbors_scratch_bytes(P, K) bytes of device memory, 16-byte aligned.  P == 0 is a no-op.  P < 0, K
 * out of range, a NULL points / idx / scratch, a misaligned scratch: F3DGS_ERR_INVALID_ARGUMENT before any device work; P > 2^30:
 * F3DGS_ERR_UNSUPPORTED.  No host read, no allocation, no memset; every launch goes to `stream`: capturable.
 *
 * f3dgs_label_mode_filter: one Jacobi step of a weighted mode filter of per-point labels over such lists, ONE launch.  labels
 * (P) int32 (negative: unlabelled; any non-negative value is a label), weight (P) float32 or NULL (1 each), idx (P, K) - the
 * caller's, every entry is bounds-checked -, dist2 (P, K) or NULL, labels_out (P) int32, share_out (P) float32 or NULL.
 * Voters of point i, in this order: i itself, then idx[i, 0 .. K-1].  Voter j votes iff 0 <= j < P, labels[j] >= 0, its weight
 * w > 0 && w < inf, and - for a neighbour - dist2[i, slot] <= max_dist2 (max_dist2 = +inf: no limit, dist2 is not read; a finite
 * max_dist2 with a NULL dist2, a negative or NaN max_dist2: F3DGS_ERR_INVALID_ARGUMENT).  The score of a label is the float32
 * sum of its voters' weights taken in voter order.  The largest score wins; among equal scores labels[i] if it is one of them
 * (whether or not i itself voted), otherwise the smallest label.  labels_out[i] = the winner, -1 with no voter; with fill == 0
 * a point whose own label is negative stays -1.  share_out[i] = the winner's score over the voters' total, one IEEE division; 0
 * where labels_out[i] is -1.  labels_out == labels is refused (F3DGS_ERR_INVALID_ARGUMENT): the step reads the OLD labels
 * only.  A pure function of its inputs: two calls give the same bits.  Capturable like the search.
 */
#define F3DGS_KNN_MAX_NEIGHBORS 16
size_t f3dgs_knn_neighbors_scratch_bytes(int P, int K);
int f3dgs_knn_neighbors(int P, int K, const float* points, int32_t* idx, float* dist2 /* or NULL */, void* scratch,
                        void* stream /* hipStream_t */);
int f3dgs_label_mode_filter(int P, int K, const int32_t* labels, const float* weight /* or NULL */, const int32_t* idx,
                            const float* dist2 /* or NULL */, float max_dist2, int fill, int32_t* labels_out,
                            float* share_out /* or NULL */, void* stream /* hipStream_t */);

/*
 * Connected components of the points over such lists (ABI 3.19; no counterpart in the reference): the lists as a graph.
 * idx (P, K) int32 - the caller's: any integers, every entry is bounds-checked -, dist2 (P, K) float32 or NULL, labels (P) int32
 * or NULL: device pointers.  1 <= K <= F3DGS_KNN_MAX_NEIGHBORS.
 *   Active nodes   node i is active iff labels == NULL or labels[i] >= 0; with labels == NULL every node carries label 0.  An
 *                  inactive node gets root = -1, size = 0, comp = -1.
 *   Directed edge  slot s of row i is an edge i -> j, j = idx[i, s], when 0 <= j < P and j != i, both ends are active and carry the
 *                  same label, and - when max_dist2 < inf - dist2[i, s] <= max_dist2 (a NaN distance gives no edge:
 *                  f3dgs_label_mode_filter's comparison).  A finite max_dist2 with a NULL dist2, a negative or NaN max_dist2:
 *                  F3DGS_ERR_INVALID_ARGUMENT.
 *   Graph          undirected.  mutual == 0: {i, j} is an edge iff i -> j or j -> i.  mutual != 0: iff both, each direction judged
 *                  on its own slot (K more reads per edge, done only when asked).
 *   root, size     (P) int32: root[i] is the smallest index of i's component, size[i] the number of its members - for every member.
 *   comp, comp_root, n_comp   the dense ids, written only when comp is not NULL (comp_root, n_comp and scratch are needed then):
 *                  n_comp (one int32 on the device) the number of components, comp[i] the rank of root[i] among the roots in
 *                  ascending order, comp_root[c] the root of component c for c < n_comp and -1 for n_comp <= c < P.
 *   status         one int32 on the device, always written: 0, non-zero only if a walk of the union-find reached its cap of P steps
 *                  (it cannot, by construction).  This function does not read it.
 * `scratch` = f3dgs_knn_components_scratch_bytes(P, num_labels) bytes of device memory, 8-byte aligned; the same size serves
 * f3dgs_component_filter (num_labels is its table; 0 for this call alone).  P == 0 is a no-op apart from n_comp = 0 (where given) and
 * status = 0.  P < 0, K out of range, a NULL idx / root / size / status, root == size (or any two outputs the same array):
 * F3DGS_ERR_INVALID_ARGUMENT before any device work; P > 2^30: F3DGS_ERR_UNSUPPORTED.  One launch per stage (init, link, flatten and
 * count, spread; for the dense ids a three-launch exclusive prefix over P and one more launch), no workgroup waits for another, no
 * host read, no allocation, no memset node: capturable as one linear graph.  Integers only: two calls give the same bits.
 *
 * f3dgs_component_filter: labels_out[i] = labels[i] (0 for NULL labels) iff i is active, size[i] >= min_size and - with largest !=
 * 0 - i's component is the best of its label: the largest size, among equal sizes the smallest root; a label >= num_labels is
 * nobody's best.  Otherwise labels_out[i] = -1.  root and size are f3dgs_knn_components' for the same labels.  num_labels is used
 * only with largest (a table of num_labels 64-bit words in `scratch`, cleared by a launch; scratch may be NULL without largest).
 * labels_out == labels is allowed: the filter is elementwise in i.  Three launches with largest, one without; capturable.
 *
 * f3dgs_debug_knn_components_shape: f3dgs_knn_components without the dense ids, with the link stage as named - 0: one thread per
 * node, its row in registers; 1: one thread per (node, slot) (what f3dgs_knn_components runs); 2: no link at all, every active
 * node a component (the floor of the other stages).  The same results for 0 and 1.  For measurements and tests.
 */
size_t f3dgs_knn_components_scratch_bytes(int P, int num_labels);
int f3dgs_knn_components(int P, int K, const int32_t* idx, const float* dist2 /* or NULL */, float max_dist2,
                         const int32_t* labels /* or NULL */, int mutual, int32_t* root, int32_t* size, int32_t* comp /* or NULL */,
                         int32_t* comp_root /* or NULL */, int32_t* n_comp /* device, or NULL */, int32_t* status /* device */,
                         void* scratch, void* stream /* hipStream_t */);
int f3dgs_component_filter(int P, const int32_t* labels /* or NULL */, const int32_t* root, const int32_t* size, int min_size,
                           int largest, int num_labels, int32_t* labels_out, void* scratch /* or NULL */,
                           void* stream /* hipStream_t */);
int f3dgs_debug_knn_components_shape(int P, int K, const int32_t* idx, const float* dist2 /* or NULL */, float max_dist2,
                                     const int32_t* labels /* or NULL */, int mutual, int shape, int32_t* root, int32_t* size,
                                     int32_t* status /* device */, void* stream /* hipStream_t */);

/*
 * The two density tests of a point cloud (ABI 3.25; no counterpart in the reference): "fewer than n points within r" and "mean
 * neighbour distance above mean + ratio * std" - what removes a floater that hangs on its object by a thin bridge, or a sparse
 * halo around a dense body, which are ONE component for f3dgs_component_filter.
 *
 * f3dgs_radius_count.  points (P, 3) float32, labels (P) int32 or NULL, count (P) int32: device pointers.  count[i] is the number
 * of points j != i with dist2(i, j) <= radius2, where dist2 = ((dx*dx) + (dy*dy)) + (dz*dz) and dx = p_j - p_i in float32, one
 * rounding per operation: f3dgs_knn_neighbors' distance, so count[i] >= k says what "the k-th entry of row i is <= radius2" says.
 *   labels   j is counted only if labels[j] == labels[i] >= 0 (f3dgs_knn_components' equal-label rule); a query with a negative
 *            label gets 0.  Any int32 may stand there.
 *   finite   a point with a NaN or infinite coordinate has count 0 and is counted by nobody.  A pair of finite points whose distance
 *            overflows float32 is counted only by radius2 = +inf, which is legal and counts every other finite point (of the label).
 *   cap      cap > 0 saturates the result: count[i] = min(true count, cap) - the walk of a lane ends at its cap, which is what
 *            "at least n neighbours" needs; cap == 0: no cap.
 *   self     excluded by index, not by distance: a duplicate of point i is counted, so radius2 = 0 counts the duplicates.
 * The result is an integer function of the inputs alone (not of the sort order, the walk order or the lanes).
 * `scratch` = f3dgs_radius_count_scratch_bytes(P) bytes of device memory, 16-byte aligned (the search's front end and P labels in
 * sorted order).  P == 0 is a no-op.  P < 0, a negative or NaN radius2, cap < 0, a NULL points / count / scratch, a misaligned
 * scratch: F3DGS_ERR_INVALID_ARGUMENT before any device work; P > 2^30: F3DGS_ERR_UNSUPPORTED.  No host read, no allocation, no
 * memset; every launch goes to `stream`: capturable.
 *
 * f3dgs_knn_outliers: statistical outlier removal over the lists of f3dgs_knn_neighbors.  idx (P, K) int32 - the caller's: any
 * integers, every entry is bounds-checked -, dist2 (P, K) float32, labels (P) int32 or NULL, score (P) float32, stats
 * (num_groups x 4) float64, keep (P) bytes: device pointers.  1 <= K <= F3DGS_KNN_MAX_NEIGHBORS, num_groups >= 1, ratio finite
 * and >= 0.
 *   Group      g(i) = labels ? labels[i] : 0 (without labels num_groups must be 1).  Point i is a MEMBER iff 0 <= g(i) < num_groups.
 *   Valid slot slot s of row i is valid iff j = idx[i, s] satisfies 0 <= j < P, j != i and g(j) == g(i), and dist2[i, s] < +inf (a
 *              NaN is not valid; FLT_MAX beside idx -1, the search's empty slot, fails the index test): f3dgs_knn_components' edge.
 *   score[i]   (float)(sum of sqrt((double)dist2[i, s]) over the valid slots in slot order / their number): the mean neighbour
 *              distance in fp64 with the correctly rounded square root, rounded once.  +inf for a point that is no member and for
 *              a member without a valid slot.  (A negative dist2 is not a distance: its score is NaN, which counts as not finite.)
 *   stats[g]   {n, mean, std, threshold} over the members of g with a finite score: n their number, mean = sum score / n, std =
 *              sqrt(sum (score - mean)^2 / (n - 1)) in a second pass about the device's own fp64 mean (the N - 1 form of Open3D and
 *              PCL; 0 for n < 2), threshold = mean + ratio * std.  A group without such a member: four zeros.
 *   keep[i]    1 iff score[i] < +inf and (double)score[i] <= threshold[g(i)], else 0.
 * Every sum is fp64 on the device; the group sums meet in one atomic per distinct group and wave, in a varying order: n, score
 * and - away from a threshold - keep are functions of the inputs alone, mean, std and threshold to the error of an fp64 sum.
 * `scratch` = f3dgs_knn_outliers_scratch_bytes(num_groups) bytes of device memory, 8-byte aligned.  With P == 0 stats is zeroed.
 * P < 0, K or num_groups out of range, num_groups != 1 without labels, a negative or non-finite ratio, a NULL stats / scratch,
 * with P > 0 a NULL idx / dist2 / score / keep, a misaligned scratch: F3DGS_ERR_INVALID_ARGUMENT before any device work; P > 2^30:
 * F3DGS_ERR_UNSUPPORTED.  Four launches (clear; scores and first sums; second sums; thresholds and keep), no workgroup waits for
 * another, no host read, no allocation: capturable.
 */
size_t f3dgs_radius_count_scratch_bytes(int P);
int f3dgs_radius_count(int P, const float* points, float radius2, const int32_t* labels /* or NULL */, int cap, int32_t* count,
                       void* scratch, void* stream /* hipStream_t */);
size_t f3dgs_knn_outliers_scratch_bytes(int num_groups);
int f3dgs_knn_outliers(int P, int K, const int32_t* idx, const float* dist2, const int32_t* labels /* or NULL */, int num_groups,
                       float ratio, float* score /* P */, double* stats /* num_groups x 4 */, uint8_t* keep /* P */, void* scratch,
                       void* stream /* hipStream_t */);

/*
 * Statistics of the Gaussians per group id (ABI 3.20; no counterpart in the reference): what the integers of the label vote, the
 * instance association, the mode filter and the components say about a class, an instance or a component AS A WHOLE.
 *
 * f3dgs_group_stats.  Gaussian i is a MEMBER of group g = groups[i] iff 0 <= g < G, its three coordinates are finite and -
 * with weight != NULL - 0 < weight[i] < inf (the mode filter's voter rule: a NaN weight is no member).  Any integers may stand in
 * `groups`; nothing is read or written out of bounds.  w_i = weight[i], or 1 for a NULL weight; M = sum of w over the members of g.
 *   count         (G) int32   the number of members (exact)
 *   mass          (G)         M
 *   centroid      (G x 3)     sum w x / M
 *   cov           (G x 6)     sum w (x - c)(x - c)^T / M in the order xx xy xz yy yz zz, the population form about the fp64
 *                             centroid c, in a second pass over the points (a one-pass raw-moment form loses about |x|^2 / sigma^2
 *                             of its digits far from the origin); 0 for a single member
 *   aabb          (G x 6)     min x y z, max x y z: the exact minimum and maximum of the members' fp32 coordinates (the weight only
 *                             decides membership), compared through the order-preserving integer map of the bits: -0 < +0
 *   feature_mean  (G x C)     sum w f / M per channel, row i of the features at features + i * feature_stride; a non-finite
 *                             feature element propagates into its channel of its group and is not filtered
 * Every output is optional (NULL: not wanted, its work is skipped - without cov there is no second pass); at least one must be
 * given.  An empty group: count 0, mass 0, zeros in centroid, cov and feature_mean, aabb = (+inf x 3, -inf x 3); P == 0 writes
 * these for every group.  Every sum is accumulated in fp64 (a product of two fp32 values is exact there); every output is the fp64
 * quotient rounded once to fp32.  The sums are gathered with atomics that arrive in a varying order: the float outputs are NOT
 * bit-reproducible between two calls (as `acc` of the contribution pass); count and aabb are.  features: 16-byte row loads when
 * C % 4 == 0, feature_stride % 4 == 0 and the pointer is 16-byte aligned, scalar loads otherwise - the same results.
 * `scratch` = f3dgs_group_stats_scratch_bytes(G, C) bytes of device memory, 8-byte aligned, cleared by a launch of the call.
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: P < 0, G outside [1, F3DGS_GROUP_MAX_GROUPS], C outside [0,
 * F3DGS_GROUP_MAX_CHANNELS], C > 0 without features, feature_mean with C == 0, feature_stride < C, a NULL groups or xyz while
 * P > 0, every output NULL, a scratch that is NULL, misaligned or too small.  No host read, no allocation, no memset node:
 * capturable as one linear graph (three to seven launches).
 *
 * f3dgs_group_merge: unites ADJACENT groups whose mean features agree.  Groups a != b are adjacent iff some slot s of some row i of
 * the neighbour lists is an edge i -> j = idx[i, s] with 0 <= j < P, j != i, groups[i] = a and groups[j] = b both in [0, G), and -
 * for a finite max_dist2 - dist2[i, s] <= max_dist2 (a NaN is no edge: f3dgs_knn_components' rules with "equal labels" turned into
 * "different ids"); with mutual != 0 row j must hold i as well, each judged on its own slot.  Adjacent groups are united iff
 * dot(m_a, m_b) / sqrt(dot(m_a, m_a) * dot(m_b, m_b)) >= min_cos, evaluated in fp64 on the fp32 rows m of feature_mean (G x C); a
 * NaN or a zero norm is no merge.  group_root[g] (G) is the smallest id of g's merged set, for every g in [0, G) - a group nobody
 * belongs to is its own root; groups_out[i] (P; may be `groups`) = group_root[groups[i]], -1 for an id outside [0, G).  status: one
 * int32 on the device, always written: 0, non-zero only if a walk of the union-find reached its cap; never read here.  The result
 * is integers and a function of the inputs alone unless an adjacent pair's cosine lies within rounding of min_cos.
 * `scratch` = f3dgs_group_merge_scratch_bytes(G) bytes (the adjacency is G x G bits), 4-byte aligned, cleared by a launch.
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: P < 0, K outside [1, F3DGS_KNN_MAX_NEIGHBORS], G outside [1,
 * F3DGS_GROUP_MERGE_MAX_GROUPS], C outside [1, F3DGS_GROUP_MAX_CHANNELS], a negative or NaN max_dist2, a NaN min_cos, a NULL
 * feature_mean / group_root / status, a NULL groups / idx / groups_out while P > 0, a finite max_dist2 without dist2, a scratch
 * that is NULL, misaligned or too small; P > 2^30: F3DGS_ERR_UNSUPPORTED.  Five launches, capturable.
 */
#define F3DGS_GROUP_MAX_GROUPS 65536
#define F3DGS_GROUP_MAX_CHANNELS 4096
#define F3DGS_GROUP_MERGE_MAX_GROUPS 4096 /* = F3DGS_INSTANCE_MAX_INSTANCES; the adjacency is G x G bits */
size_t f3dgs_group_stats_scratch_bytes(int G, int C);
int f3dgs_group_stats(int P, int G, int C, const int32_t* groups, const float* xyz, const float* weight /* or NULL */,
                      const float* features /* NULL iff C == 0 */, int64_t feature_stride /* >= C, in elements */,
                      int32_t* count, float* mass, float* centroid, float* cov, float* aabb, float* feature_mean /* each or NULL */,
                      void* scratch, size_t scratch_bytes, void* stream /* hipStream_t */);
size_t f3dgs_group_merge_scratch_bytes(int G);
int f3dgs_group_merge(int P, int K, int G, int C, const int32_t* groups, const int32_t* idx, const float* dist2 /* or NULL */,
                      float max_dist2, int mutual, const float* feature_mean /* G x C */, float min_cos, int32_t* group_root /* G */,
                      int32_t* groups_out /* P, may alias groups */, int32_t* status /* device */, void* scratch,
                      size_t scratch_bytes, void* stream /* hipStream_t */);

/*
 * Object transforms (ABI 3.21; no counterpart in the reference, whose editing stops at delete / extract / recolour): the
 * Gaussians of every group moved, turned and scaled by the group's own similarity transform, every group in the same launch.
 *
 * The table, G rows (1 <= G <= F3DGS_GROUP_MAX_GROUPS) in device memory: quat (G x 4) in the model's order (w, x, y, z), scale
 * (G), translation (G x 3), pivot (G x 3, or NULL: the origin).  The quaternion is normalised in fp64 on the device, R =
 * R(q / |q|) by the rasterizer's formula (preprocess.hip; oracle/torch_oracle.py: _quat_to_rot), and the map of group g is
 *     x' = s R (x - p) + p + t.
 * A row is INVALID iff one of its entries is not finite, |q| is 0 (or not finite), or s <= 0.  status[g] (G, int32, always
 * written): 0 for a valid row, otherwise the first of F3DGS_TRANSFORM_BAD_QUAT (an entry of quat is not finite), _ZERO_QUAT,
 * _BAD_SCALE (not finite), _NONPOSITIVE_SCALE, _BAD_TRANSLATION, _BAD_PIVOT that applies.  The members of an invalid group are
 * treated exactly as non-members.  Gaussian i is TRANSFORMED iff 0 <= groups[i] < G and that row is valid; any integers may stand
 * in `groups` (P, int32).
 *
 * Per-Gaussian inputs, each optional (NULL), at least one; each given input needs its output and the other way round:
 *   xyz        (P x 3)   x' as above
 *   rotations  (P x 4)   the Hamilton product q_T (x) q, q_T the normalised quaternion of the table.  This is exact for the model,
 *                        whose get_rotation normalises.  The rasterizer does NOT normalise (forward.cu:128): fed |q| != 1 it
 *                        builds |q|^2 R + (1 - |q|^2) I, before the transform and after it alike, and that matrix does not turn
 *                        with R.  A caller who hands un-normalised quaternions straight to the rasterizer must normalise first.
 *   scales     (P x 3)   scale_mode F3DGS_TRANSFORM_SCALES_LOG: the model's raw _scaling, + ln s; _LINEAR: activated scales, * s
 *   cov3d      (P x 6)   xx xy xz yy yz zz as cov3D_precomp: s^2 R Sigma R^T
 *   sh_rest    n_rest in {0, 3, 8, 15} coefficients of 3 colours per Gaussian (degree 0 .. 3 without the DC term), row i at
 *              sh_rest + i * sh_stride floats, coefficient k colour c at 3 k + c: the model's _features_rest (P, 15, 3) with
 *              sh_stride = 45, or shs + 3 of a (P, 16, 3) tensor with sh_stride = 48, read (and written) in place.  The
 *              coefficients of band l become D_l(R) c, D_l the (2l + 1)^2 matrix with sum_m c'_m Y_m(R d) = sum_m c_m Y_m(d) for
 *              every unit d in the rasterizer's basis (the constants C1, C2[], C3[] with their signs): a turned object keeps
 *              its view-dependent colour on its own surface.  sh_rest == NULL iff n_rest == 0.
 * DC colour, opacity and semantic features are invariant and are not taken.  A non-finite value of a Gaussian propagates
 * (through the whole band, for a coefficient); there is no per-Gaussian special case.
 *
 * Two forms.  src_rows == NULL: every output has P rows (M is ignored) and may be its input - the same pointer and, for sh_rest,
 * the same stride.  A row that is not transformed is copied unchanged, and where output and input are the same array it is not
 * written at all.  src_rows (M, int32): the GATHER form - output row j is the transform of input row src_rows[j] under that row's
 * group (a copy where it is not transformed), a row of zeros for an index outside [0, P): "a second instance 17 over there" is
 * one call into appended rows.  An output that overlaps an input in any other way is refused.  With P == 0, or M == 0 in the
 * gather form, only status is written.
 *
 * Numerics: one small kernel per call builds, per group and in fp64, s R, p, p + t, q / |q|, ln s, s and D_1, D_2, D_3 (83
 * entries; the recursion of Ivanic and Ruedenberg in the entries of R); the per-Gaussian kernel accumulates every output element
 * as one fp64 chain of fused multiply-adds and rounds once to fp32.  An output that sums n terms t_k lies within
 * ulp32(v) / 2 + 4 n 2^-53 sum|t_k| of its fp64 value v (n = 5 for xyz: the three products, p and t; 4 for rotations, 2 / 1 for
 * scales, 9 for cov3d, 2l + 1 for band l) - wherever the scene lies.  No bit promise beyond "rows that are not transformed are
 * untouched" and "the same inputs give the same outputs" (no atomics).
 * `scratch` = f3dgs_transform_gaussians_scratch_bytes(G) bytes of device memory, 8-byte aligned (the table).
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: P < 0, G outside [1, F3DGS_GROUP_MAX_GROUPS], a NULL quat / scale /
 * translation / status, M < 0 with src_rows, n_rest outside {0, 3, 8, 15} or at odds with sh_rest, an unknown scale_mode, every
 * input NULL, an input without its output or an output without its input, a stride below 3 n_rest, a NULL groups while P > 0,
 * an output that overlaps an input other than in place, a scratch that is NULL, misaligned or too small; P > 2^30:
 * F3DGS_ERR_UNSUPPORTED.  No host read, no allocation, no memset node, no option: two launches, capturable.
 */
#define F3DGS_TRANSFORM_SCALES_LOG 0
#define F3DGS_TRANSFORM_SCALES_LINEAR 1
#define F3DGS_TRANSFORM_BAD_QUAT 1
#define F3DGS_TRANSFORM_ZERO_QUAT 2
#define F3DGS_TRANSFORM_BAD_SCALE 3
#define F3DGS_TRANSFORM_NONPOSITIVE_SCALE 4
#define F3DGS_TRANSFORM_BAD_TRANSLATION 5
#define F3DGS_TRANSFORM_BAD_PIVOT 6
size_t f3dgs_transform_gaussians_scratch_bytes(int G);
int f3dgs_transform_gaussians(int P, int G, const float* quat, const float* scale, const float* translation,
                              const float* pivot /* or NULL */, const int32_t* groups, const int32_t* src_rows /* or NULL */, int M,
                              const float* xyz, const float* rotations, const float* scales /* each or NULL */, int scale_mode,
                              const float* cov3d /* or NULL */, const float* sh_rest /* NULL iff n_rest == 0 */, int n_rest,
                              int64_t sh_stride /* in floats */, float* xyz_out, float* rotations_out, float* scales_out,
                              float* cov3d_out, float* sh_rest_out, int64_t sh_out_stride, int32_t* status /* G */, void* scratch,
                              size_t scratch_bytes, void* stream /* hipStream_t */);

/*
 * Feature codebooks (ABI 3.22; no counterpart in the reference, which stores and writes every semantic feature in full): the two
 * halves of Lloyd's iteration over the per-Gaussian features - vector or product quantisation of the features, and clustering of
 * the Gaussians where no label map and no masks exist.  `features`: P rows of C float32, row i at features + i * feature_stride
 * (feature_stride >= C, in elements; the channel stride is 1): the model's (P, 1, C) tensor, a column slice and a row-strided view
 * are read in place.  `centroids`: (K x C) float32, contiguous.  1 <= K <= F3DGS_CODEBOOK_MAX_CENTROIDS, 1 <= C <=
 * F3DGS_CODEBOOK_MAX_CHANNELS, P >= 0.
 *
 * f3dgs_codebook_assign: codes[i] (P, int32) = the index of the centroid nearest to row i.
 *   L2 (flags == 0)         minimises  score_ik = |c_k|^2 - 2 x_i . c_k
 *   F3DGS_CODEBOOK_COSINE   maximises  x_i . c^_k, c^_k = c_k / |c_k| (a zero centroid: c^_k = 0, it scores 0); score_ik = -x_i . c^_k
 * |c_k|^2 and c^_k are computed per row in fp64 and rounded once to fp32 by a first launch, into `workspace`.  The dot product is
 * ONE fp32 fmaf chain over the channels ascending from 0 (v_mfma_f32_32x32x2_f32: bit for bit such a chain; channels past C are
 * zeros), score = fmaf(-2, dot, |c_k|^2) or -dot: a code is a function of the inputs alone, not of the grid or of P.  The lowest
 * score wins, the lowest k among equal scores.  A score that is not finite never wins: a centroid with a non-finite element, or one
 * whose |c_k|^2 or dot product overflows fp32.  A row with a non-finite element gets code -1, as does every row if no score is
 * finite.  The (P, K) scores are never stored.
 * Optional outputs (NULL: not wanted), all in device memory, none read back:
 *   dist2    (P) float32   sum_c (x_ic - c_kc)^2 of the winner k, or 1 - cos(x_i, c_k) under the cosine metric (cos = 0 where x_i or
 *                          c_k is zero), recomputed for the winner alone in fp64 from the caller's centroids and rounded once; 0
 *                          for code -1
 *   inertia  one double    sum of w_i * dist2_i (the rounded fp32 value) over the rows with a code >= 0 and 0 < w_i < inf (w_i =
 *                          weight[i], 1 for a NULL weight), added in fp64 (a partial sum per 256 rows, then atomics: the last bits
 *                          vary between calls).  The weight excludes a row from this sum and from the update, never from codes.
 *   moved    one int32     the number of rows with codes[i] != prev_codes[i] (needs prev_codes; codes may BE prev_codes)
 * `workspace` = f3dgs_codebook_workspace_bytes(K, C) bytes of device memory, 16-byte aligned: it depends on K and C only.
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: P < 0, K or C outside their limits, unknown flags, feature_stride < C, a NULL
 * centroids, a NULL features or codes while P > 0, moved without prev_codes, a misaligned inertia, a workspace that is NULL,
 * misaligned or too small; P > 2^31 - 129: F3DGS_ERR_UNSUPPORTED.  One to three launches, no host read, no allocation: capturable.
 *
 * f3dgs_codebook_update: centroids[k] (in place) = sum w_i x_i / sum w_i over the rows with codes[i] == k and 0 < w_i < inf, every
 * sum in fp64 (f3dgs_group_stats' accumulation with the codes as ids: the sums meet in a varying order) and the quotient rounded
 * once; with F3DGS_CODEBOOK_COSINE the fp64 mean is divided by its fp64 length before the rounding (a zero mean stays zero).
 * count[k] (K, int32, or NULL) = the number of those rows.  A code outside [0, K) belongs to no centroid.  A centroid without
 * members keeps its row; with F3DGS_CODEBOOK_RESEED_EMPTY it takes the features of row (k * 2654435761 + iteration * 40503) mod P
 * (in uint64) instead - unless P == 0 or that row holds a non-finite element, then it keeps its row.  A non-finite feature of a
 * member propagates into its channel.  `scratch` = f3dgs_codebook_update_scratch_bytes(K, C) bytes, 8-byte aligned, cleared by a
 * launch of the call.  F3DGS_ERR_INVALID_ARGUMENT before any device work: as above, a negative iteration.  Two or three launches,
 * capturable.
 */
#define F3DGS_CODEBOOK_COSINE 1
#define F3DGS_CODEBOOK_RESEED_EMPTY 2
#define F3DGS_CODEBOOK_MAX_CENTROIDS 65536 /* = F3DGS_GROUP_MAX_GROUPS */
#define F3DGS_CODEBOOK_MAX_CHANNELS 4096   /* = F3DGS_GROUP_MAX_CHANNELS */
size_t f3dgs_codebook_workspace_bytes(int K, int C);
int f3dgs_codebook_assign(int P, int K, int C, const float* features, int64_t feature_stride /* >= C, in elements */,
                          const float* centroids /* K x C */, int flags, const int32_t* prev_codes /* or NULL */,
                          const float* weight /* or NULL */, int32_t* codes /* P, may alias prev_codes */, float* dist2, double* inertia,
                          int32_t* moved /* each or NULL */, void* workspace, size_t workspace_bytes, void* stream /* hipStream_t */);
size_t f3dgs_codebook_update_scratch_bytes(int K, int C);
int f3dgs_codebook_update(int P, int K, int C, const float* features, int64_t feature_stride, const int32_t* codes,
                          const float* weight /* or NULL */, int flags, int iteration, float* centroids /* K x C, in place */,
                          int32_t* count /* K, or NULL */, void* scratch, size_t scratch_bytes, void* stream /* hipStream_t */);

/*
 * ---- SAM's prompt encoder and mask decoder (csrc/sam_decoder.hip; forward only) ---------------------------------------
 * From a rendered 256-channel feature map and point / box prompts to the decoder's low-resolution logits and IoU
 * predictions: what the reference's predictor.py:predict_torch gets from `prompt_encoder` and `mask_decoder` before
 * `postprocess_masks`, and what f3dgs_sam_masks takes.  Exactly SAM's decoder: transformer_dim 256, depth 2, 8 heads, MLP 2048,
 * attention downsample rate 2, 4 mask tokens + 1 IoU token, the 4x upscaler and the hypernetwork heads; any other architecture,
 * and the mask prompt (`mask_downscaling`), are not built.  fp32 in, fp32 out; every contraction over a weight matrix on the
 * exact-fp32 matrix instructions; no atomics, every reduction in a fixed order: two calls give the same bits, and a prompt's
 * outputs are the same bits at every batch size and every position in the batch.
 *
 * f3dgs_sam_decoder_pack_weights: `params` is a HOST table of F3DGS_SAM_DECODER_PARAMS device pointers, each a contiguous fp32
 * parameter of the reference's modules in this order (Linear weights (out, in), ConvTranspose2d weights (in, out, 2, 2)):
 *   prompt_encoder:  pe_layer.positional_encoding_gaussian_matrix (2, 128); point_embeddings.0 .. 3.weight; not_a_point_embed.weight;
 *                    no_mask_embed.weight
 *   mask_decoder:    iou_token.weight; mask_tokens.weight (4, 256);
 *                    for layer l = 0, 1 of transformer.layers: self_attn, norm1, cross_attn_token_to_image, norm2, mlp.lin1, mlp.lin2,
 *                    norm3, norm4, cross_attn_image_to_token;
 *                    transformer.final_attn_token_to_image; transformer.norm_final_attn;
 *                    output_upscaling.0 (ConvTranspose2d), .1 (LayerNorm2d), .3 (ConvTranspose2d);
 *                    output_hypernetworks_mlps.0 .. 3, each layers.0 .. 2; iou_prediction_head.layers.0 .. 2
 *   where an attention is q_proj, k_proj, v_proj, out_proj and every module is its weight, then its bias.
 * `packed`: f3dgs_sam_decoder_weights_bytes() bytes, 16-byte aligned, in the kernels' own layout.  One small launch per parameter.
 *
 * f3dgs_sam_decoder_plan (once per feature map): `features` C x h x w, read in place at the given element strides (a view of a
 * larger render works).  Writes into `plan` (f3dgs_sam_decoder_plan_bytes(h, w) bytes, 16-byte aligned) what is the same for
 * every prompt of the image: the token-major embedding + no_mask_embed, the dense positional encoding (cell centres
 * (i + 0.5) / h, (j + 0.5) / w) and layer 0's projections of the image tokens.  Four launches.
 *
 * f3dgs_sam_decoder_predict: B prompts of n_points points each (`coords` B x n_points x 2 fp32 (x, y) in pixels of the
 * input_h x input_w input image; `labels` B x n_points int32: 1 foreground, 0 background, -1 not a point) and, if `boxes` is not
 * NULL, one box each (B x 4 fp32 XYXY).  The tokens of a prompt are [iou, mask 0..3, points..., a pad point if no box is given,
 * box corner 0, box corner 1]: T = 5 + n_points + (boxes ? 2 : 1) <= F3DGS_SAM_DECODER_MAX_TOKENS.  `low_res`: B x n x 4h x 4w
 * fp32 and `iou`: B x n fp32 with n = 3 (masks 1..3) if multimask, else 1 (mask 0); only these are computed.  `scratch`:
 * f3dgs_sam_decoder_scratch_bytes(B, h, w, T) bytes, 16-byte aligned, uninitialised (it holds the prompts' image tokens: B h w
 * KiB and a little).  B == 0 is a no-op.  40 launches, none of them a memset; no host read, no allocation, every launch on
 * `stream`: capturable.
 *
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: a size below its minimum, a NULL or misaligned pointer, a negative stride,
 * no prompt at all, a scratch too small.  F3DGS_ERR_UNSUPPORTED: C != 256, h w > F3DGS_SAM_DECODER_MAX_GRID, T >
 * F3DGS_SAM_DECODER_MAX_TOKENS, B > 65535.  The _bytes functions return 0 for sizes the calls refuse.
 */
#define F3DGS_SAM_DECODER_PARAMS 127
#define F3DGS_SAM_DECODER_MAX_TOKENS 16
#define F3DGS_SAM_DECODER_MAX_GRID 16384
size_t f3dgs_sam_decoder_weights_bytes(void);
int f3dgs_sam_decoder_pack_weights(const float* const* params /* host table of device pointers */, int n_params, float* packed,
                                   void* stream /* hipStream_t */);
size_t f3dgs_sam_decoder_plan_bytes(int h, int w);
int f3dgs_sam_decoder_plan(int C, int h, int w, const float* features, int64_t stride_c, int64_t stride_y, int64_t stride_x /* in elements */,
                           const float* packed, float* plan, void* stream /* hipStream_t */);
size_t f3dgs_sam_decoder_scratch_bytes(int B, int h, int w, int T);
int f3dgs_sam_decoder_predict(int B, int h, int w, int n_points, const float* coords, const int32_t* labels, const float* boxes /* or NULL */,
                              int input_h, int input_w, int multimask, const float* plan, const float* packed, float* low_res, float* iou,
                              void* scratch, size_t scratch_bytes, void* stream /* hipStream_t */);

/*
 * ---- LPIPS, VGG16, version 0.1 (csrc/lpips.hip; forward only) -----------------------------------------------------------
 * The third number of the reference's metrics.py:72-74, as its lpipsPyTorch computes it with net_type 'vgg': the z-score
 * (mean -.030 -.088 -.188, std .458 .448 .450; values as given, no rescaling), torchvision's vgg16().features[0:30] (13
 * convolutions 3x3 pad 1 with bias and ReLU, widths 64 64 | 128 128 | 256 x3 | 512 x3 | 512 x3, a 2x2 max-pool between the
 * blocks), the taps behind relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (C_l = 64, 128, 256, 512, 512 at H, H/2, H/4, H/8, H/16,
 * floor), and per tap  d_l = mean over pixels of sum_c w_l[c] (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2.  fp32 throughout,
 * the contractions of conv1_2 .. conv5_3 on the exact-fp32 matrix instructions in ONE summation order (the accumulator starts
 * at the bias; per chunk of 16 input channels the 144 products (tap; channel pair) are one chain from zero, and the chunk sums
 * are added in chunk order), zeros outside the image: an activation is a function of its 3 x 3 x Cin inputs alone.  No atomics, every reduction in a fixed order: two calls give the same bits, and a pair's
 * outputs are the same bits at every batch size and every position in the batch.  Other networks are not built.
 *
 * f3dgs_lpips_pack_weights: `params` is a HOST table of F3DGS_LPIPS_PARAMS device pointers, each a contiguous fp32 parameter:
 * the 13 convolution weights (Cout, Cin, 3, 3) of features.0 2 5 7 10 12 14 17 19 21 24 26 28, then their 13 biases, then the
 * five heads lin.0 .. 4 (C_l values each, non-negative in the published weights).  `packed`: f3dgs_lpips_weights_bytes() bytes,
 * 16-byte aligned, in the kernels' own layout (59 MB).  One small launch per parameter.
 *
 * f3dgs_lpips_forward: N pairs of 3 x H x W images, H, W >= 16.  A side is read IN PLACE at the given element strides (all
 * >= 0: a channels-last view, a crop of a larger tensor) in its format: F3DGS_LPIPS_F32 (4-byte aligned; with
 * F3DGS_LPIPS_QUANTIZE_X / _Y in `flags` a value v is read as floor(clamp(v * 255 + 0.5, 0, 255)) / 255, what a saved PNG
 * holds of it - f3dgs_image_metrics' rounding) or F3DGS_LPIPS_U8 (value / 255, bit for bit torch's quotient).  `layer_terms`
 * (N x 5 fp32: d_l) and `totals` (N fp32: sum_l d_l) - either may be NULL.  `workspace`: f3dgs_lpips_workspace_bytes(N, H, W)
 * bytes, 16-byte aligned, uninitialised: two activation buffers of 2N x 64 x H x W floats and the fp64 partial sums of the
 * taps.  x and y run as one batch of 2N images: 13 convolution launches, 5 tap launches, 1 final sum.  No host read, no
 * allocation, every launch on `stream`: capturable.  N == 0 is a no-op.
 *
 * f3dgs_lpips_taps: the five un-normalised taps of N images into `taps`, a HOST table of five device pointers (N x C_l x H_l
 * x W_l fp32, contiguous).  `workspace`: f3dgs_lpips_workspace_bytes((N + 1) / 2, H, W) bytes.
 *
 * F3DGS_ERR_INVALID_ARGUMENT before any device work: N < 0, H or W < 16, a NULL or misaligned pointer, a negative stride, an
 * unknown format or flag, a quantize flag on a uint8 side, a workspace too small.  F3DGS_ERR_UNSUPPORTED: more than 65534
 * images or 2^26 pixels an image.  f3dgs_lpips_workspace_bytes returns 0 for sizes the calls refuse.
 */
#define F3DGS_LPIPS_PARAMS 31
#define F3DGS_LPIPS_F32 0
#define F3DGS_LPIPS_U8 1
#define F3DGS_LPIPS_QUANTIZE_X 0x1
#define F3DGS_LPIPS_QUANTIZE_Y 0x2
size_t f3dgs_lpips_weights_bytes(void);
int f3dgs_lpips_pack_weights(const float* const* params /* host table of device pointers */, int n_params, float* packed,
                             void* stream /* hipStream_t */);
size_t f3dgs_lpips_workspace_bytes(int N, int H, int W);
int f3dgs_lpips_forward(int N, int H, int W, const void* x, int x_format, int64_t x_stride_n, int64_t x_stride_c, int64_t x_stride_y,
                        int64_t x_stride_x /* in elements */, const void* y, int y_format, int64_t y_stride_n, int64_t y_stride_c,
                        int64_t y_stride_y, int64_t y_stride_x, int flags, const float* packed, float* layer_terms /* N x 5, or NULL */,
                        float* totals /* N, or NULL */, void* workspace, size_t workspace_bytes, void* stream /* hipStream_t */);
int f3dgs_lpips_taps(int N, int H, int W, const void* image, int format, int64_t stride_n, int64_t stride_c, int64_t stride_y,
                     int64_t stride_x /* in elements */, int quantize, const float* packed,
                     float* const* taps /* host table of five device pointers */, void* workspace, size_t workspace_bytes,
                     void* stream /* hipStream_t */);

/*
 * ---- Side channels of f3dgs_backward: threading contract -----------------------------------------------------------
 * The four setters below and f3dgs_set_feature_grad_lowres change how the f3dgs_backward calls OF THE CALLING HOST THREAD
 * behave.  All five are thread-local: they are invisible to, and unaffected by, any other thread.
 *   - the two callbacks and the accumulate switch are STICKY: they stay armed for every later call of the thread until reset
 *     (NULL / 0).  A caller arms them around exactly the calls it means (dp.py: a `with` block per backward pass);
 *   - f3dgs_set_feature_grad_lowres is ONE-SHOT: it is consumed - and cleared - by the next f3dgs_backward of the thread,
 *     whether that call succeeds or fails.
 * A second trainer in the same process therefore runs on its OWN thread (one thread per device is the supported shape:
 * the instance-count read-back words are kept per (thread, device, stream) as well) and arms its own channels there;
 * nothing needs a lock.  Two trainers that share a thread - interleaving their backward calls on it - must re-arm or
 * clear the channels between calls themselves: the library cannot tell the calls apart.  The process-wide OPTIONS
 * (f3dgs_set_option) are the only state shared between threads; they are read once at the top of each call.
 *
 * Optional notification inside f3dgs_backward (no counterpart in the reference): `fn(ctx, stream)` is called on
 * the calling host thread right after the blend backward has been ENQUEUED on `stream`, i.e. at the point of
 * the stream from which dL_dsemantic_feature is final while the per-Gaussian stage still follows.  A
 * data-parallel caller records an event there and starts the all-reduce of the feature gradient on another
 * stream, overlapping it with the rest of the call.  Thread-local; NULL removes it.
 */
typedef void (*f3dgs_stage_fn)(void* ctx, void* stream /* hipStream_t */);
void f3dgs_set_feature_grad_ready_callback(f3dgs_stage_fn fn, void* ctx);

/*
 * Gradient accumulation across views (no counterpart in the reference, which renders one view per step): with `on` != 0
 * the following f3dgs_backward calls of this host thread ADD their feature gradient into `dL_dsemantic_feature` instead
 * of overwriting it (the blend backward accumulates with atomics anyway: the zero-fill in front of it is skipped).  A
 * caller that renders several views per optimiser step hands in ONE (P, C) buffer, zeroed once, for all of them - no
 * per-view gradient tensor, no per-view zero-fill, no per-view add - and, data parallel, reduces that buffer from inside
 * the LAST view's backward pass (f3dgs_set_feature_grad_ready_callback).  Every other output is overwritten as always.
 * Thread-local; 0 restores the default.
 */
void f3dgs_set_feature_grad_accumulate(int on);

/*
 * Second optional notification inside f3dgs_backward (no counterpart in the reference): with a callback registered the
 * per-Gaussian stage (K8 + K9, R/cuda_rasterizer/backward.cu:145-404 - row-parallel) runs as `chunks` launches over
 * consecutive row ranges, and `fn(ctx, stream, row_begin, row_end)` is called on the calling host thread right after the
 * launch covering Gaussians [row_begin, row_end) has been ENQUEUED: from that point of the stream on, rows
 * [row_begin, row_end) of EVERY per-Gaussian output (dL_dmean3D, dL_dsh, dL_dscale, dL_drot, dL_dopacity, dL_dcolor,
 * dL_dmean2D, dL_dcov3D) are final.  A data-parallel caller starts the all-reduce of those rows (the SH gradient is
 * 48 of the 59 non-feature floats per Gaussian) while the later chunks still run.  Ranges are disjoint, ascending and
 * cover [0, P); row_begin is a multiple of 64.  chunks <= 1: one launch, one call.  Thread-local; NULL removes it.
 */
typedef void (*f3dgs_rows_fn)(void* ctx, void* stream /* hipStream_t */, int row_begin, int row_end);
void f3dgs_set_grad_rows_ready_callback(f3dgs_rows_fn fn, void* ctx, int chunks);

/*
 * Test / profiling hooks (not part of the reference surface).  They expose
 * the private state written by f3dgs_forward so that every stage can be
 * compared with the oracle in isolation.  Each copies `count` elements
 * starting at element 0 into a HOST buffer and synchronises the stream.
 *   what: "rec" (12 floats per Gaussian: mean_x, mean_y, conic a,b,c, opacity, r,g,b, depth, radius bits, pad;
 *         defined only where radii > 0)  "clamped"(u8 bitmask)  "tiles_touched"(u32)  "depth_key"(u32)
 *         "order"(u32 x P, depth order)  "order_counts"(u32 x P: tiles_touched[order[i]] behind a multi-launch depth sort,
 *         the sorted depth keys behind the one-launch sort of up to 16,384 Gaussians)
 *         "counters"(16 x u32: [0] = entries of point_list,
 *         [1] = reference-style num_rendered)  "point_list"(u32 x R)  "tile_sorted"(u32 x R)
 *         "ranges"(uint2 per tile)  "final_T"(float per pixel)  "n_contrib"(u32 per pixel)
 *         "tile_len"(u32 per tile: the largest n_contrib of its pixels)
 */
int f3dgs_debug_read(
    const char* what,
    int P, int C, int R, int width, int height,
    const char* geom_buffer,
    const char* binning_buffer,
    const char* image_buffer,
    void* host_dst, size_t dst_bytes,
    void* stream);

/* Per-stage device-time accounting, active while option "profile" is 1 (seeded from F3DGS_PROFILE).  HIP events are recorded on the call's stream around every stage (no
 * synchronisation inside forward/backward); f3dgs_profile_read waits for the recorded events and
 * returns, per stage name, the accumulated milliseconds and the number of spans since the last
 * f3dgs_profile_reset.  Returns the number of stages written; names[i] are static strings. */
int f3dgs_profile_read(const char** names, double* total_ms, long* calls, int max_stages);
void f3dgs_profile_reset(void);

#ifdef __cplusplus
}
#endif

#endif /* F3DGS_H_INCLUDED */
