/*
 * mvsn_hip.h -- C ABI of libmvsn_hip.so, the MI355X (gfx950) plane-sweep hot path of
 * MultiViewStereoNet.
 *
 * The reference (robustrobotics/multi_view_stereonet) has no native layer: its "kernels" are
 * stock ATen ops called from multi_view_stereonet/multi_view_stereonet.py.  Each entry point
 * below replaces one group of those call sites (cited as file:line into the reference).  A
 * maintainer binds them with ctypes (INTEGRATION.md shows the stub) from inside
 * MultiViewStereoNet.forward().
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into HBM; tensors are dense fp32, row-major in the
 *     index order written next to them (NCHW / NCDHW as in the reference); masks are uint8
 *     (0/1), bit-compatible with torch.bool storage;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); every call only
 *     enqueues work on that stream and never synchronises the device;
 *   - return value: 0 on success, a positive hipError_t, or a negative MVSN_E_* code;
 *     mvsn_last_error() returns a thread-local message for the last non-zero return;
 *   - a "chain" is one (reference image, source view) pair; chains are indexed
 *     n = source * B + image, so n % B is the reference-image index;
 *   - P = rows*cols of the coarsest (1/16) pyramid level, D = number of idepth hypotheses.
 */
#ifndef MVSN_HIP_H
#define MVSN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVSN_ABI_VERSION 7

#define MVSN_E_BADARG (-1)      /* null pointer, non-positive size, unsupported channel count */
#define MVSN_E_TOOLARGE (-2)    /* shape exceeds what the kernel's LDS/global plan supports */
#define MVSN_E_WORKSPACE (-3)   /* workspace pointer null or smaller than the *_workspace_bytes() answer */

typedef void *mvsn_stream_t;

int mvsn_abi_version(void);
const char *mvsn_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Plane-sweep set-up: per chain, the baseline-normalised pose, the D idepth samples, the
 * fronto-parallel homographies at the coarsest level, the incremental homographies
 * H_inc[d] = H[d-1]^-1 H[d] (H_inc[0] = I) and the full-resolution homography of plane 0.
 * Replaces create_idepth_samples (multi_view_stereonet.py:131-165 -> stereo/image_predictor.py:120-209),
 * create_plane_sweep_homographies (:167-194 -> image_predictor.py:400-461), the per-source
 * baseline renormalisation (:566-571) and the per-step torch.inverse/matmul (:281-282).
 *   T_right_in_left (N,4,4)  K_lvl0 (N,4,4)  K_lvl4 (N,4,4)
 *   idepth_samples (N,D)  H_lvl4 (N,D,3,3)  H_inc (N,D,3,3)  H_lvl0_plane0 (N,3,3)  baseline (N)
 * The idepth samples and the three homography outputs carry the bits of the reference's own fp32 evaluation (its
 * per-pixel tensor program and torch.sum's order; torch's CPU inverse of the pose, of the intrinsics and of H[d-1],
 * its 3x3 products: csrc/mvsn_setup.hip, namespace ref32; pinned by tests/golden/g11_incremental_homographies.npz and,
 * for fx != fy, off-centre principal points and pyramids scaled differently in x and y, g12_camera_forms.npz)
 * when the intrinsics are [[fx,0,cx],[0,fy,cy],[0,0,1]]; for any other intrinsics they are a double-precision
 * evaluation rounded once.
 * ------------------------------------------------------------------------------------------- */
int mvsn_plane_sweep_setup(const float *T_right_in_left, const float *K_lvl0, const float *K_lvl4,
                           int n_chains, int rows4, int cols4, int num_idepth_samples,
                           float *idepth_samples, float *H_lvl4, float *H_inc, float *H_lvl0_plane0,
                           float *baseline, mvsn_stream_t stream);
/* The same with the poses and intrinsics as the forward holds them: one (batch, 4, 4) pose tensor per source view
 * (host array of n_sources <= 8 device pointers) and the batch's intrinsics shared by its sources; chain n = s * batch + b.
 * Saves the torch.cat / repeat of :553,:587-592 in front of the launch. */
int mvsn_plane_sweep_setup_sources(const float *const *T_right_in_lefts, int n_sources, const float *K_lvl0,
                                   const float *K_lvl4, int batch, int rows4, int cols4, int num_idepth_samples,
                                   float *idepth_samples, float *H_lvl4, float *H_inc, float *H_lvl0_plane0,
                                   float *baseline, mvsn_stream_t stream);

/* Host only, no device call: the order one chain's outputs are formed in, by the predicate the kernel itself evaluates
 * on that chain's level-0 and level-4 intrinsics (each one row-major 4x4, HOST memory) and the level-4 grid.  Bit 0
 * (value 1): H_lvl0_plane0, H_lvl4 and H_inc in the reference's fp32 order; bit 1 (value 2): the idepth samples too.
 * 3 for every pin-hole K on a level-4 grid of 8 .. 8192 pixels, 1 outside that range, 0 for a K with a shear term or any
 * other entry off [[fx,0,cx],[0,fy,cy],[0,0,1]] (and for null pointers or non-positive sizes). */
int mvsn_plane_sweep_setup_path(const float *K_lvl0_host, const float *K_lvl4_host, int rows4, int cols4);

/* ---------------------------------------------------------------------------------------------
 * Homography warp with bilinear, clamp-to-edge sampling and out-of-image zeroing.
 * Replaces PlaneSweepWarper.forward (multi_view_stereonet.py:205-235) ->
 * HomographyImagePredictor.forward (stereo/image_predictor.py:470-523, grid_sample bilinear /
 * border / align_corners=False).  mask = |nx|>1 or |ny|>1 on the normalised coordinate.
 *   image (B,C,rows,cols)  H (B,n,3,3)  ->  volume (B,C,n,rows,cols)  mask (B,n,rows,cols) u8
 * ------------------------------------------------------------------------------------------- */
int mvsn_homography_warp(const float *image, const float *H, int batch, int channels, int n_planes,
                         int rows, int cols, float *volume, uint8_t *mask, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The fused incremental chain: for every chain, one persistent workgroup keeps the source-view
 * feature map resident on-chip and walks d = 1..D-1: warp the previous plane's features by
 * H_inc[d], warp the coarse source image by H[d], run the FeatureRefiner (conv 35->32, GN,
 * LReLU, residual block, conv 32->32, +features) on fp32 MFMA, and emit the cost-volume slice
 * (not mask) * |left - right| and the mask slice.  Replaces
 * IncrementalFastGeometryAwareFeatureNetwork.forward :270-300 (everything after the plane-0
 * extractor), FeatureRefiner.forward :424-440 and the cost-volume build :553,:587-592.
 *   src_image_lvl4 (N,3,rows,cols)   H_lvl4, H_inc (N,D,3,3)   plane0_features (N,32,rows,cols)
 *   left_features (B,32,rows,cols)   refiner_packed: mvsn_feature_refiner_packed_floats() floats
 *   cost_volume (N,32,D,rows,cols)   mask_volume (N,D,rows,cols) u8
 *   feature_volume: optional (N,32,D,rows,cols) masked source features, or NULL
 *   workspace: mvsn_incremental_cost_volume_workspace_bytes_for() bytes, 16-byte aligned (may be 0 -> NULL allowed)
 *   form: MVSN_CHAIN_AUTO picks per coarse grid and number of chains (mvsn_incremental_cost_volume_form_for tells which);
 *         MVSN_CHAIN_DIRECT = the three 3x3 convolutions as direct implicit GEMMs (any grid up to 2048 px);
 *         MVSN_CHAIN_WINOGRAD = as Winograd F(2x2,3x3) products (fp32 throughout, 2.25x fewer multiplies; even
 *         rows/cols whose planes + one layer of transformed weights fit LDS, e.g. 16x32), MVSN_E_TOOLARGE otherwise.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_CHAIN_AUTO 0
#define MVSN_CHAIN_DIRECT 1
#define MVSN_CHAIN_WINOGRAD 2
#define MVSN_CHAIN_STEPWISE 3 /* one plane per round of full-chip launches (warp, three Winograd convolutions with the
                                 GroupNorm statistics of the producing launch, the residual pass, the cost slice):
                                 for coarse grids whose planes do not fit one CU (30x40, 32x64), any number of chains
                                 (cols % 4 == 0); a selectable form -- since round 5 AUTO stays on the banded form there */
#define MVSN_CHAIN_BANDED 4   /* one chain on SEVERAL workgroups: the coarse plane cut into bands of pixel rows (16x32: 8
                                 bands of 2 rows up to CUs / 8 chains -- every layer split by transform-row half across a
                                 band's waves -- and 4 bands of 4 rows beyond, bit-identical; 30x40: 15 of 2; 32x64: 16 of
                                 2), Winograd arithmetic of
                                 MVSN_CHAIN_WINOGRAD; per step the bands hand each other the new feature rows their
                                 gathers reach into, their GroupNorm sums and one halo row per layer as tagged 8-byte
                                 write-through granules -- no fence, no placement assumption.  For few chains in flight
                                 (batch 1: the reference's loop, test.py:38,197-200): the workgroups of a launch must be
                                 co-resident, so more chains than CUs / bands run as consecutive passes inside the call
                                 (AUTO: one pass on 16x32), and only ONE such call may be in flight per device.
                                 30x40 / 32x64 beyond one pass of the thin bands (17 / 16 chains on 256 CUs): the SLAB
                                 plan -- 3 bands of 10 rows / 4 bands of 8 rows per chain, each a 512-thread workgroup
                                 that keeps its band's activation planes resident in LDS like the plane-resident
                                 Winograd kernel (85 / 64 chains per pass; passes of equal size, or full passes + ONE
                                 thin-band pass for a remainder of at most 17 / 16 chains; four hand-offs per
                                 step; mvsn_incremental_cost_volume_banded_groups tells which plan a call runs).
                                 Needs workspace (..._workspace_bytes_for); the word at
                                 mvsn_incremental_cost_volume_status_offset() inside it is 0 after a clean run. */
size_t mvsn_feature_refiner_packed_floats(void);
/* Pack the ten FeatureRefiner tensors (state_dict order: conv0.{weight,bias}, bn0.{weight,bias},
 * res0.conv1.{weight,bias}, res0.bn1.{weight,bias}, conv_final.{weight,bias}) into the MFMA
 * fragment order the chain kernel streams. */
int mvsn_pack_feature_refiner(const float *conv0_w, const float *conv0_b, const float *bn0_w,
                              const float *bn0_b, const float *res0_w, const float *res0_b,
                              const float *res0_bn_w, const float *res0_bn_b, const float *final_w,
                              const float *final_b, float *packed, mvsn_stream_t stream);
size_t mvsn_incremental_cost_volume_workspace_bytes(int n_chains, int rows, int cols);   /* MVSN_CHAIN_DIRECT: the step's moved
                                                                                             features (always, since ABI 3) + the
                                                                                             activation planes that do not fit LDS */
int mvsn_incremental_cost_volume_form(int rows, int cols);   /* the fused form of this grid: WINOGRAD or DIRECT */
/* Which form a call runs, on what workspace, is decided in ONE place, the library's resolver; the functions below are
 * views of it.  mvsn_incremental_cost_volume_form_for: what MVSN_CHAIN_AUTO resolves to for this many chains on this grid
 * (BANDED, WINOGRAD, STEPWISE or DIRECT) in the entry points that put a repair launch behind a banded call
 * (mvsn_incremental_cost_volume_guarded / _bf16); ..._workspace_bytes_for: the workspace `form` needs for
 * num_idepth_samples planes (AUTO allowed: enough for either entry point).
 * The PLAIN mvsn_incremental_cost_volume has no repair launch, so its AUTO is more conservative: on 30x40 / 32x64 it
 * takes the banded form only while the chains fit ONE thin-band pass (17 / 16 chains on 256 CUs) and the
 * co-residency-free STEPWISE form (DIRECT for cols % 4 != 0) beyond -- the multi-pass slab plan holds the whole device
 * for milliseconds and a time-out without repair would leave NaN in the cost slice.  Ask for MVSN_CHAIN_BANDED (or use
 * the guarded entry) to get the slab plan. */
int mvsn_incremental_cost_volume_form_for(int n_chains, int rows, int cols);
size_t mvsn_incremental_cost_volume_workspace_bytes_for(int n_chains, int num_idepth_samples, int rows, int cols,
                                                        int form);
/* Host only, no device call: the resolver itself (ABI 6).  `form`: the requested form (AUTO allowed); `guarded` != 0: for
 * the entry points with a repair launch (_guarded / _bf16), 0: for the plain one; `coresident_allowed` == 0: AUTO must not
 * pick the banded form, whose workgroups have to be co-resident (several calls in flight on the device, another process
 * holding it) -- it falls back to WINOGRAD, STEPWISE or DIRECT.  An explicit WINOGRAD / STEPWISE request on a grid
 * without that plan is answered with DIRECT and out[6] = 1 (the entry points themselves refuse such a call).
 * out = { form that runs, repair form (0: no repair launch), workspace bytes, repair-workspace bytes, status offset and
 * workgroups per chain (BANDED, else 0), redirected, 0 }.  Returns 1, or 0 when the form has no plan for the grid (the
 * entry points return MVSN_E_TOOLARGE / MVSN_E_BADARG then) or an argument is out of range. */
int mvsn_incremental_cost_volume_resolve(int n_chains, int num_idepth_samples, int rows, int cols, int form,
                                         int coresident_allowed, int guarded, size_t out[8]);
/* MVSN_CHAIN_BANDED only: byte offset, inside the workspace, of the 32-bit status word the launch leaves behind
 * (0 = every inter-workgroup hand-off completed; non-zero = a bounded wait timed out and the outputs are invalid) */
size_t mvsn_incremental_cost_volume_status_offset(int n_chains, int rows, int cols);
/* MVSN_CHAIN_BANDED only: workgroups per chain of the plan a call with this many chains runs (16x32: 8 or 4 thin bands;
 * 30x40 / 32x64: 15 / 16 thin bands, or 3 / 4 slabs with many chains in flight; 0: the grid has no banded plan) */
int mvsn_incremental_cost_volume_banded_groups(int n_chains, int rows, int cols);   /* (ABI 4) */
int mvsn_incremental_cost_volume(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                 const float *plane0_features, const float *left_features,
                                 const float *refiner_packed, int n_chains, int batch,
                                 int num_idepth_samples, int rows, int cols, float *cost_volume,
                                 uint8_t *mask_volume, float *feature_volume, void *workspace,
                                 size_t workspace_bytes, int form, mvsn_stream_t stream);
/* The same call with the small-batch default made safe on a SHARED device (ABI 3).  When `form` resolves to
 * MVSN_CHAIN_BANDED, a second launch follows the banded one(s) on the stream: the single-launch form of the grid (plane-
 * resident Winograd on 16x32, the direct kernel elsewhere) GATED on the banded status word -- its workgroups read the word
 * and return at once when it is 0 (a few microseconds), and recompute cost_volume / mask_volume / feature_volume
 * completely when a hand-off timed out (the banded workgroups were not co-resident).  No host round trip, graph-capturable;
 * the outputs are valid either way.  `repair_workspace`: mvsn_incremental_cost_volume_repair_workspace_bytes() bytes (0 on
 * 16x32).  `sticky_status`: optional two 32-bit words in device-VISIBLE memory (device or pinned host memory; plain
 * system-scope loads / stores by one thread of the repair launch): [0] |= the status of every repaired call, [1] += 1
 * per repair -- never cleared by the library, so a host that looks at it later (or never synchronises per call) still
 * learns that the banded form does not fit this device's load.
 * Other forms: identical to mvsn_incremental_cost_volume.
 * Replaces: the reference's chain loop as above (multi_view_stereonet.py:279-290) -- which has no failure mode to repair. */
size_t mvsn_incremental_cost_volume_repair_workspace_bytes(int n_chains, int rows, int cols);
int mvsn_incremental_cost_volume_guarded(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                         const float *plane0_features, const float *left_features,
                                         const float *refiner_packed, int n_chains, int batch,
                                         int num_idepth_samples, int rows, int cols, float *cost_volume,
                                         uint8_t *mask_volume, float *feature_volume, void *workspace,
                                         size_t workspace_bytes, int form, void *repair_workspace,
                                         size_t repair_workspace_bytes, unsigned *sticky_status, mvsn_stream_t stream);
/* bf16 FEATURE tier (BASELINE config 5's "bf16 features"; reported, never the parity path; ABI 5): the guarded call with
 * the cost volume STORED as bf16 -- `cost_volume_bf16` is (n_chains, 32, D, rows, cols) 2-byte elements, the values the
 * fp32 call writes rounded to nearest-even (v_cvt_pk_bf16_f32): Kernel A's dominant HBM stream halves (SURVEY 8d:
 * config 5 137.5 MB -> ~69 MB per depth map).  mask_volume / feature_volume / workspaces / status as in the guarded
 * call; every form but MVSN_CHAIN_STEPWISE has the variant (MVSN_E_BADARG there: run the fp32 call and convert).
 * Consumer: mvsn_conv_forward_bf16_storage(in_is_bf16 = 1), whose bf16 operand conversion of an fp32 volume yields the
 * same bits -- the stored volume costs the regulariser no accuracy beyond the bf16-operand tier's.
 * Replaces: the cost volume of multi_view_stereonet.py:553,587-592 at config 5's storage precision. */
int mvsn_incremental_cost_volume_bf16(const float *src_image_lvl4, const float *H_lvl4, const float *H_inc,
                                         const float *plane0_features, const float *left_features,
                                         const float *refiner_packed, int n_chains, int batch,
                                         int num_idepth_samples, int rows, int cols, void *cost_volume_bf16,
                                         uint8_t *mask_volume, float *feature_volume, void *workspace,
                                         size_t workspace_bytes, int form, void *repair_workspace,
                                         size_t repair_workspace_bytes, unsigned *sticky_status, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Direct convolution on fp32 MFMA (implicit GEMM, weights = A, activations = B), 2-D or 3-D,
 * C_out in {1..32}, 'same' padding = dilation*(k/2), stride 1 or 2 (2-D only), with
 *   - an optional input transform fused into the tile load:
 *         x = LeakyReLU_0.2(GroupNorm_4(in))                        (in_stats != NULL)
 *         x = in_residual + LeakyReLU_0.2(GroupNorm_4(in))          (in_residual != NULL: a residual
 *             block x + LReLU(GN(conv(x))), utils/resnet.py:93-109, folded into the NEXT layer's load)
 *     and, with out_staged != NULL, x itself written out once (N,C_in,H,W) as a by-product
 *     (2-D 3x3 stride-1 layers only) -- the normalise/activate/add pass never runs on its own;
 *   - bias add, and per-workgroup GroupNorm partials of the OUTPUT (out_partials != NULL) that
 *     mvsn_groupnorm_finalize turns into (mean, rstd) per (sample, group).
 * Replaces every conv2d/conv3d + GroupNorm + LeakyReLU call site of FeatureNetwork (:109-129),
 * CostVolumeFilter (:341-353) and IDepthmapRefiner (:468-484).
 *   in (N,C_in,[D,]H,W)  weight_packed: mvsn_conv_packed_floats() floats  bias (C_out) or NULL
 *   in_stats (N,4,2) mean,rstd   in_gamma,in_beta (C_in)   in_residual, out_staged (N,C_in,H,W)
 *   out (N,C_out,[D,]Ho,Wo)
 *   out_partials (N, R, 4, 3) {count, mean, M2}, R = mvsn_conv_num_tiles() partial records per sample
 *   (one per workgroup tile and wave; written without any workgroup-level synchronisation)
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int n;         /* samples */
  int c_in;      /* input channels (any >= 1) */
  int c_out;     /* 1..32 */
  int depth;     /* 1 for 2-D */
  int rows, cols;/* input spatial size */
  int kd, kh, kw;/* kernel extent; kd = 1 for 2-D */
  int stride;    /* 1 or 2 (rows/cols only) */
  int dilation;  /* rows/cols only */
  int precision; /* MVSN_CONV_FP32, MVSN_CONV_FP32_WINO or MVSN_CONV_BF16X3: arithmetic / algorithm, see below */
} mvsn_conv_desc;

/* Arithmetic of mvsn_conv_forward.
 *   MVSN_CONV_FP32    v_mfma_f32_16x16x4_f32: bit-for-bit an fp32 fmaf chain.
 *   MVSN_CONV_BF16X3  fp32 operands split into bf16 hi + lo, a*b ~= ah*bh + ah*bl + al*bh on
 *                     v_mfma_f32_16x16x32_bf16 with fp32 accumulation (~2^-16 relative per product;
 *                     "3 x bf16 split", the fp32-equivalent tier BASELINE.md section 2 allows).  Only the
 *                     32 -> 32 channel 3x3 / 3x3x3 stride-1 layers (mvsn_conv_bf16x3_supported); weights are
 *                     packed per precision, in_residual / out_staged are not available.
 *   MVSN_CONV_FP32_WINO  the same fp32 MFMA arithmetic on the Winograd F(2x2,3x3) form of the layer: 16
 *                     products per 2x2 outputs and (cin, cout) pair instead of 36; every operand and
 *                     accumulation is fp32, the result differs from MVSN_CONV_FP32 by rounding only (~1e-6
 *                     relative).  2-D 3x3 stride-1 layers with 32 output channels, dilation 1/2/4/8, and the
 *                     3x3x3 32 -> 32 layers (volume form: 2-D Winograd products summed over the depth tap, 12
 *                     multiplies per output instead of 27), cols % 4 == 0 (mvsn_conv_winograd_supported);
 *                     weights are packed per form.  Also the 5x5 stride-2 32 -> 32 layers of the feature extractor
 *                     (multi_view_stereonet.py:78-129), cols % 8 == 0: F(2x2,3x3) on the input's four stride-2 phases,
 *                     392 products per 2x2 outputs and (cin, cout) pair instead of 800; no fused input transform, no
 *                     GroupNorm partials on that form (MVSN_E_BADARG).
 *   MVSN_CONV_BF16    plain bf16 operands (the hi halves only), fp32 accumulation, on the same kernels and packed
 *                     weights as MVSN_CONV_BF16X3: BASELINE config 5's speed tier.  ~2^-9 relative per operand:
 *                     the final depth lands OUTSIDE the 1e-3 parity contract (measured ~2e-3 mean-rel). */
#define MVSN_CONV_FP32 0
#define MVSN_CONV_BF16X3 1
#define MVSN_CONV_FP32_WINO 2
#define MVSN_CONV_BF16 3
int mvsn_conv_bf16x3_supported(const mvsn_conv_desc *desc);
/* bf16 STORAGE on top of MVSN_CONV_BF16 (ABI 4; BASELINE config 5's "bf16 features" for the 3x3x3 regulariser layers,
 * multi_view_stereonet.py:341-353): `in` and / or `out` hold bf16 (same NCDHW element order, two bytes per element) instead
 * of fp32 -- `in_is_bf16` / `out_is_bf16`, at least one set.  Products on the bf16 matrix cores with fp32 accumulation,
 * the biased accumulators rounded to bf16 (RNE) by the storing epilogue; `out_partials` (GroupNorm records) and
 * `in_stats` stay fp32 and are formed from the unrounded accumulators.  desc: kd = 3, precision MVSN_CONV_BF16;
 * weight_packed as for MVSN_CONV_BF16.  A speed tier outside the 1e-3 parity contract (its own asserted budget:
 * tests/test_hip_parity.py); never part of the default path. */
int mvsn_conv_forward_bf16_storage(const mvsn_conv_desc *desc, const void *in, int in_is_bf16,
                                   const float *weight_packed, const float *bias, const float *in_stats,
                                   const float *in_gamma, const float *in_beta, void *out, int out_is_bf16,
                                   float *out_partials, mvsn_stream_t stream);
int mvsn_conv_winograd_supported(const mvsn_conv_desc *desc);

size_t mvsn_conv_packed_floats(const mvsn_conv_desc *desc);
int mvsn_conv_pack_weights(const mvsn_conv_desc *desc, const float *weight, float *packed,
                           mvsn_stream_t stream);
int mvsn_conv_num_tiles(const mvsn_conv_desc *desc);
int mvsn_conv_forward(const mvsn_conv_desc *desc, const float *in, const float *weight_packed,
                      const float *bias, const float *in_stats, const float *in_gamma,
                      const float *in_beta, const float *in_residual, float *out_staged, float *out,
                      float *out_partials, mvsn_stream_t stream);
/* mvsn_conv_forward on an input handed over as up to three channel blocks instead of one tensor: block b is
 * a contiguous (N, block_channels[b], rows, cols) tensor and the layer convolves their channel-wise
 * concatenation (sum of block_channels = desc->c_in) without it ever being assembled.  Replaces the
 * torch.cat([image, features, idepth], 1) in front of every IDepthmapRefiner (multi_view_stereonet.py:466,
 * :602-605).  Winograd form only (desc->precision = MVSN_CONV_FP32_WINO, mvsn_conv_winograd_supported);
 * 1 <= num_blocks <= 3, every block 16-byte aligned. */
int mvsn_conv_forward_blocks(const mvsn_conv_desc *desc, const float *const *in_blocks, const int *block_channels,
                             int num_blocks, const float *weight_packed, const float *bias, float *out,
                             float *out_partials, mvsn_stream_t stream);
/* A normalise / activate / add pass handed over as a job: the arguments of mvsn_groupnorm_lrelu_apply with finalised
 * statistics (stat_tiles = 0). */
typedef struct mvsn_apply_job {
  const float *x, *stats, *gamma, *beta;
  const float *residual, *r_stats, *r_gamma, *r_beta;
  float *out;      /* may alias x */
  int n;           /* samples: (n, 32, spatial) */
  int reverse;     /* 1: the carrying launch walks its tiles, and with them the job, from the end to the beginning
                      (consecutive launches of a pipelined tower alternate, so that each starts on what the one before
                      it touched last: a few per cent of the bytes then come from the memory-side cache); results
                      identical either way */
  long spatial;
} mvsn_apply_job;
/* mvsn_conv_forward (no in_residual / out_staged) AND an independent apply job in one call.  The residual blocks
 * x + LeakyReLU(GroupNorm(conv(x))) (multi_view_stereonet.py:38-48, used :448-474) alternate a convolution bound by the
 * matrix pipe with a pass bound by HBM; with the batch cut in two slices, slice B's convolution can carry slice A's
 * pass in its own launch (the job's 16-byte loads / stores are issued by the convolution's waves between their
 * multiplies).  The job must not depend on this convolution's output, nor the convolution on the job's.  Where the
 * layer's kernel cannot carry it (not a Winograd 32 -> 32 2-D layer, spatial % 256 != 0, job larger than the layer's
 * own output) the job runs as its own launch first: results are bit-identical either way; *carried (may be NULL)
 * says which it was. */
int mvsn_conv_forward_carry(const mvsn_conv_desc *desc, const float *in, const float *weight_packed, const float *bias,
                            const float *in_stats, const float *in_gamma, const float *in_beta, float *out,
                            float *out_partials, const mvsn_apply_job *job, int *carried, mvsn_stream_t stream);
/* partials (N,R,4,3) {count, mean, M2} per record and group (R = mvsn_conv_num_tiles records per sample, passed as
 * `tiles`) -> stats (N,4,2) = {mean, rstd}, eps 1e-5, biased variance; records are 48 bytes, 16-byte aligned */
int mvsn_groupnorm_finalize(const float *partials, int n, int tiles, float *stats, mvsn_stream_t stream);
/* The same statistics with a sample's records cut into up to 16 slices reduced by separate workgroups and added in slice
 * order (ABI 4): for layers that leave MANY records per sample (more than 2048: a level-0 layer of a 1024x512 frame
 * leaves 32768 = 1.5 MB) on FEW samples -- one workgroup per sample then reads megabytes alone.  The number of slices
 * depends on `tiles` only (a sample's statistics do not depend on the batch it travels in; up to 2048 records it is 1 and
 * the call IS mvsn_groupnorm_finalize).  Deterministic; equal to the one-workgroup result up to the rounding of the
 * double-precision sums.  `workspace`: mvsn_groupnorm_finalize_split_workspace_bytes() bytes, 8-byte aligned. */
size_t mvsn_groupnorm_finalize_split_workspace_bytes(int n, int tiles);
int mvsn_groupnorm_finalize_split(const float *partials, int n, int tiles, float *stats, void *workspace,
                                  size_t workspace_bytes, mvsn_stream_t stream);
/* out = [residual +] LeakyReLU_0.2(GroupNorm(x)) on (N,32,spatial); out may alias x.
 * stats: (N,4,2) finalised when stat_tiles == 0, else the producer's records (N,stat_tiles,4,3), finalised by every
 * workgroup of the pass with mvsn_groupnorm_finalize's own code (same bits): the dependent finalize launch in front of
 * the pass disappears -- small batches, where that launch (7 us) costs more than re-reading a few hundred records per
 * workgroup.  mvsn_conv_to1_block takes its in_stats / stat_tiles the same way.
 * residual optional; r_stats set: the residual is itself a raw convolution output (r_gamma, r_beta required), always
 * finalised, out = LeakyReLU(GroupNorm(x)) + LeakyReLU(GroupNorm_r(residual)) -- the first residual block of a refiner
 * (:472-474) when the head's activation x0 = LReLU(GN(conv0)) is never materialised: conv0's raw output feeds block 1's
 * convolution through mvsn_conv_forward's in_stats transform and this call as the residual. */
int mvsn_groupnorm_lrelu_apply(const float *x, const float *stats, int stat_tiles, const float *gamma, const float *beta,
                               const float *residual, const float *r_stats, const float *r_gamma, const float *r_beta,
                               int n, long spatial, float *out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * 32 -> 1 channel 3x3 (kd = 1) or 3x3x3 (kd = 3) convolution, 'same' padding, dilation 1: the last
 * layer of CostVolumeFilter (conv4, :337,:351) and of every IDepthmapRefiner (conv_final, :464,:480).
 * HBM-bound (128 input bytes per output): a tap GEMM P[taps][position] = W[taps x 32] * in[32 x position]
 * on the fp32 matrix cores (every input element is loaded once, 9 or 27 taps on the MFMA row dimension),
 * then a shift-and-add of the tap planes out of LDS.
 * With prior != NULL it also applies the refiner's epilogue (:482 and the gain trick :607-611):
 *     out = relu(prior * fx[n] + conv + bias) / fx[n]
 *   in (N,32,[D,]H,W)  weight (1,32,[3,]3,3) UNPACKED  bias (1) or NULL  prior (N,1,H,W)  fx (N)
 *   out (N,[D,]H,W).  Requires cols % 4 == 0 (mvsn_conv_to1_supported); otherwise use mvsn_conv_forward.
 * ------------------------------------------------------------------------------------------- */
int mvsn_conv_to1_supported(int rows, int cols);
int mvsn_conv_to1(const float *in, const float *weight, const float *bias, const float *prior, const float *fx,
                  int n, int depth, int rows, int cols, int kd, float *out, mvsn_stream_t stream);
/* The 3-D layer on a RAW convolution output: LeakyReLU(GroupNorm(in_raw)) (CostVolumeFilter's bn3 + relu,
 * multi_view_stereonet.py:349-350) is applied while the planes are loaded, so the regulariser's last normalise /
 * activate pass never goes through HBM.   in_raw (N,32,D,H,W)  in_stats (N,4,2)  in_gamma, in_beta (32)  out (N,D,H,W) */
int mvsn_conv_to1_volume_norm(const float *in_raw, const float *in_stats, const float *in_gamma, const float *in_beta,
                              const float *weight, const float *bias, int n, int depth, int rows, int cols, float *out,
                              mvsn_stream_t stream);
/* The same 2-D layer with the tower's LAST residual block folded into its load: the input
 * in_residual + LeakyReLU(GroupNorm(in_raw)) (SimpleBasicBlock, multi_view_stereonet.py:21-38) is formed in
 * registers from the raw output of the block's convolution and the block's input, never written.
 *   in_raw, in_residual (N,32,H,W)  in_stats, stat_tiles: as mvsn_groupnorm_lrelu_apply's stats  in_gamma, in_beta (32)
 *   in_residual may be NULL */
int mvsn_conv_to1_block(const float *in_raw, const float *in_stats, int stat_tiles, const float *in_gamma,
                        const float *in_beta, const float *in_residual, const float *weight, const float *bias,
                        const float *prior, const float *fx, int n, int rows, int cols, float *out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Soft-argmin over the hypothesis axis: out = sum_d softmax(-cost)_d * idepth_d.
 * Replaces extract_idepthmap (multi_view_stereonet.py:486-492).
 *   cost (N,D,P)  idepth_samples (N,D)  ->  idepth (N,P)
 * ------------------------------------------------------------------------------------------- */
int mvsn_soft_argmin(const float *cost, const float *idepth_samples, int n, int num_idepth_samples,
                     int pixels, float *idepth, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-pixel confidence of the soft-argmin (not part of the reference, which keeps the
 * expectation only).  With p = softmax(-cost) over the hypotheses: idx = sum_d p_d * d (in index space),
 * i = clamp(floor(idx), 0, D-1), confidence = p[i-1] + p[i] + p[i+1] + p[i+2], terms outside [0, D-1] left out: the
 * probability mass of the four hypotheses around the estimate (MVSNet's photometric confidence).  A NaN cost gives a
 * NaN confidence in its pixel.
 * mvsn_soft_argmin_confidence: ONE launch in place of mvsn_soft_argmin; its idepth is the same bits.
 *   cost (N,D,P)  idepth_samples (N,D)  ->  idepth, confidence (N,P)
 * mvsn_confidence_fuse_sources: minimum over the sources, chain n = s * batch + b; NaN in any source gives NaN.
 *   confidence (S*B,P)  ->  out (B,P)
 * mvsn_confidence_mask: out = (confidence >= min_confidence) && (valid == NULL || valid) as bytes 0 / 1 -- the `valid`
 * input of mvsn_fusion_consistency; a NaN confidence compares false.   confidence, valid, out: `count` elements
 * mvsn_fusion_gather: out[i] = maps[view[i] * pixels_per_view + pixel[i]] for the `count` points of mvsn_fusion_emit
 * (NaN for an index outside the maps).   maps (n_views, pixels_per_view)  view, pixel (count) int32
 * ------------------------------------------------------------------------------------------- */
int mvsn_soft_argmin_confidence(const float *cost, const float *idepth_samples, int n, int num_idepth_samples,
                                int pixels, float *idepth, float *confidence, mvsn_stream_t stream);
int mvsn_confidence_fuse_sources(const float *confidence, int n_sources, int batch, int pixels, float *out,
                                 mvsn_stream_t stream);
int mvsn_confidence_mask(const float *confidence, const uint8_t *valid, long count, float min_confidence,
                         uint8_t *out, mvsn_stream_t stream);
int mvsn_fusion_gather(const float *maps, const int *view, const int *pixel, int n_views, long pixels_per_view,
                       long count, float *out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The three elementwise steps the flag branches of forward() leave outside the fused kernels:
 *   mvsn_channel_l2_norm      do_cost_volume_filter = False: cost = ||cost_volume||_2 over the channel axis
 *                             (torch.norm(.., dim=1), multi_view_stereonet.py:598).  x (N,C,P) -> out (N,P)
 *   mvsn_idepth_scale         out = prior * fx[n]: the refiner's input channel in the gain trick (:607-611 etc.)
 *   mvsn_refiner_epilogue     out = relu(prior * fx[n] + delta) / fx[n] (:482 + the division that follows), for the
 *                             shapes whose 32 -> 1 layer does not take the fused form of mvsn_conv_to1
 *   prior, delta, out (N,P)   fx (N)
 * ------------------------------------------------------------------------------------------- */
int mvsn_channel_l2_norm(const float *x, int n, int channels, long pixels, float *out, mvsn_stream_t stream);
int mvsn_idepth_scale(const float *prior, const float *fx, int n, long pixels, float *out, mvsn_stream_t stream);
int mvsn_refiner_epilogue(const float *prior, const float *fx, const float *delta, int n, long pixels, float *out,
                          mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Bilinear resize, align_corners=False, to an arbitrary target size (Upsampler :372-380), and
 * the boolean-mask variant float -> bilinear -> (> 0.5) (MaskUpsampler :389-396).
 *   in (N,C,h,w) -> out (N,C,H,W); mask bytes are 0 or 1 (torch.bool)
 * ------------------------------------------------------------------------------------------- */
int mvsn_upsample_bilinear(const float *in, int n, int channels, int rows_in, int cols_in, int rows_out,
                           int cols_out, float *out, mvsn_stream_t stream);
/* upsample_bilinear of a one-channel idepth map plus its per-sample scaled copy out * fx[n] (the refiner's input
 * channel idepth * fx, multi_view_stereonet.py:607-611) in one pass */
int mvsn_upsample_prior(const float *in, const float *fx, int n, int rows_in, int cols_in, int rows_out, int cols_out,
                        float *out, float *out_scaled, mvsn_stream_t stream);
int mvsn_upsample_mask(const uint8_t *in, int n, int channels, int rows_in, int cols_in, int rows_out,
                       int cols_out, uint8_t *out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One level of the ceil-halving area pyramid the forward's inputs are built from
 * (build_image_pyramid, utils/image_utils.py:111-128 = interpolate(mode="area")).
 *   in (N,C,h,w) -> out (N,C,(h+1)/2,(w+1)/2)
 * ------------------------------------------------------------------------------------------- */
int mvsn_area_downsample(const float *in, int n, int channels, int rows_in, int cols_in, float *out,
                         mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input preparation in two launches (multi_view_unpack_batch, multi_view_stereonet_utils.py:541-641):
 * mvsn_image_pyramid: every level of the area pyramid in one pass over the frames, for sizes divisible by
 * 2^(levels-1) (mvsn_image_pyramid_supported; otherwise mvsn_area_downsample level by level).
 *   in (N,C,rows,cols)  out_levels[l-1] -> (N,C,rows>>l,cols>>l), l = 1..levels-1 (HOST array of device pointers)
 * mvsn_prepare_cameras: K pyramid (:575-581: fx*=sx, fy*=sy, cx = sx(cx+0.5)-0.5, cy likewise, sx = w_l/w_0),
 * the source poses and their inverses with the translations divided by the baseline to the FIRST source (:597-604),
 * and that baseline.
 *   K (B,4,4)  T_right_in_left (S,B,4,4) un-normalised  level_sizes_dev: DEVICE int[2*levels] = rows_0, cols_0, rows_1, ...
 *   -> K_pyr (levels,B,4,4)  T_normalised, T_inverse_normalised (S,B,4,4)  baseline (B)
 * ------------------------------------------------------------------------------------------- */
int mvsn_image_pyramid_supported(int rows, int cols, int levels);
int mvsn_image_pyramid(const float *in, int n, int channels, int rows, int cols, int levels, float *const *out_levels,
                       mvsn_stream_t stream);
int mvsn_prepare_cameras(const float *K, const float *T_right_in_left, int batch, int n_sources, int levels,
                         const int *level_sizes_dev, float *K_pyr, float *T_normalised, float *T_inverse_normalised,
                         float *baseline, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-source fusion (multi_view_stereonet.py:615-627): per chain divide by its baseline, mean
 * over the S sources; mask = mean(mask) > 0.5.
 *   raw, refined (S*B,P)  baseline (S*B)  mask (S*B,D,P) u8
 *   -> raw_out, refined_out (B,P)  mask_out (B,D,P) u8
 * `refined_aliases_raw` != 0 reproduces the reference's double division when refiner 4 is off.
 * ------------------------------------------------------------------------------------------- */
int mvsn_fuse_sources(const float *raw, const float *refined, const float *baseline, const uint8_t *mask,
                      int n_sources, int batch, int num_idepth_samples, int pixels, int refined_aliases_raw,
                      float *raw_out, float *refined_out, uint8_t *mask_out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Two-view consistency (the bidirectional path, multi_view_stereonet_utils.py:503-539 with
 * estimate_right_idepthmap, and what its outputs feed in multi_view_stereonet/losses.py).
 *
 * mvsn_idepth_reproject: every pixel (x, y, idepth) of THIS view is lifted to 3-D, moved into the OTHER view and
 * projected: its idepth there, its normalised pixel coordinate there, whether that leaves the image
 * (IDepthmapProjector.forward, stereo/image_predictor.py:538-576), and the other view's idepth map (and optionally a
 * mask, as float, > 0) sampled at that coordinate (grid_sample bilinear / border / align_corners=False,
 * losses.py:59-61, :129-135).  absdiff_partials (optional, batch * mvsn_idepth_reproject_blocks(pixels) floats)
 * receives per-workgroup sums of |sampled - reprojected| for mvsn_occlusion_mask.
 *   K (B,4,4) of this pyramid level   T_other_in_this (B,4,4)   idepth, other_idepth (B,rows,cols)
 *   other_mask (B,rows,cols) u8 or NULL
 *   -> idepth_in_other, other_sampled (B,rows,cols)  other_mask_sampled u8 or NULL  invalid u8  uv (B,rows,cols,2) or NULL
 * mvsn_occlusion_mask: get_occlusion_mask (losses.py:42-82): (sampled - reprojected) > mean|sampled - reprojected|
 * of the image, or invalid.
 * mvsn_masked_l1: loss (+)= mean |a - b| over the elements with neither skip flag set (the two l1_loss terms of
 * left_right_idepthmap_consistency_losses, losses.py:137-157); NaN when nothing is selected, as the reference.
 * ------------------------------------------------------------------------------------------- */
int mvsn_idepth_reproject_blocks(int pixels);
int mvsn_idepth_reproject(const float *K, const float *T_other_in_this, const float *idepth, const float *other_idepth,
                          const uint8_t *other_mask, int batch, int rows, int cols, float *idepth_in_other,
                          float *other_sampled, uint8_t *other_mask_sampled, uint8_t *invalid, float *uv,
                          float *absdiff_partials, mvsn_stream_t stream);
int mvsn_occlusion_mask(const float *idepth_in_other, const float *other_sampled, const uint8_t *invalid,
                        const float *absdiff_partials, int batch, int pixels, uint8_t *mask, mvsn_stream_t stream);
int mvsn_masked_l1(const float *a, const float *b, const uint8_t *skip_a, const uint8_t *skip_b, long n, int accumulate,
                   float *loss, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Plane-resident residual tower on the 16 x 32 coarse grid: ONE persistent workgroup per sample keeps the 32-channel
 * activation planes in LDS and runs  [head conv + GroupNorm + LeakyReLU] -> n_blocks x (x + LReLU(GN(conv3x3_dilated(x))))
 * -> tail  in a single launch.  Replaces, at level 4 of 512 x 256 frames,
 *   - IDepthmapRefiner.forward (multi_view_stereonet.py:468-484) with the gain trick of :607-611
 *     (head over [image 3 | features 32 | prior * fx], dilations 1,2,4,8,1,1, tail_mode 1: relu(prior*fx + conv_final)/fx),
 *   - the residual stack + conv_final of FeatureNetwork.forward (:121-129; no head, tail_mode 0),
 * i.e. the 15-21 launches of mvsn_conv_forward / mvsn_groupnorm_* the launch-per-layer form needs there.
 *   in[b] (n_b, channels[b], 16, 32): up to three channel blocks, sample n reads block b at n % sample_mod[b]
 *   block_scale (optional): block `scale_block` is multiplied by block_scale[n % scale_mod] while it is loaded
 *   weights: the layers' Winograd-transformed weights (mvsn_conv_pack_weights, MVSN_CONV_FP32_WINO) re-ordered per
 *            k-step as [cout tile][xi row][lane][xi column], layer after layer: head (9 k-steps), blocks (8 each),
 *            and for tail_mode 0 the final 32 -> 32 layer
 *   params:  [bias 32 | gamma 32 | beta 32] per layer (head, blocks), then tail_mode 0: bias 32;
 *            tail_mode 1: the 32 -> 1 layer's weight (32 x 9) and bias (1)
 *   out: tail_mode 0 (n, 32, 16, 32); tail_mode 1 (n, 1, 16, 32) with prior (n, 16, 32), fx[n % fx_mod]
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  const float *in[3];
  int channels[3], sample_mod[3];
  const float *block_scale;
  int scale_mod, scale_block;
  int head_chunks, n_blocks;
  int dilation[6];
  const float *weights, *params;
  int tail_mode;
  const float *prior, *fx;
  int fx_mod;
  float *out;
} mvsn_tower_desc;
int mvsn_tower_16x32(const mvsn_tower_desc *desc, int n_samples, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth metrics of a batch on the device: replaces the per-image host loop of test.py:210-235 + get_depth_prediction_metrics
 * (test.py:41-71).  Per image: depth_est = idepth_est / baseline, inverted where positive (:210-214); selected pixels =
 * truth in (min_depth, max_depth) AND estimate in (min_depth, max_depth) (:221,:232); per-pixel values in fp32 as numpy
 * forms them, sums in double in a fixed order.
 *   idepth_est, depth_true (B, pixels) fp32 (depth_true in metric units)   baseline (B)
 *   partials: B * mvsn_depth_metrics_blocks(pixels) * 9 doubles of scratch
 *   rows (B, 9) doubles: {n_truth, n_selected, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3}; NaN metrics when nothing is
 *   selected (numpy's mean of an empty selection); the caller drops images with n_truth == 0 (:223-225).
 * ------------------------------------------------------------------------------------------- */
int mvsn_depth_metrics_blocks(long pixels);
int mvsn_depth_metrics(const float *idepth_est, const float *depth_true, const float *baseline, int batch, long pixels,
                       float min_depth, float max_depth, double *partials, double *rows, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Depth-map fusion: the geometric-consistency filter that follows the network in an MVS pipeline, and the
 * back-projection of the kept pixels into one world-space point cloud (multi_view_stereonet_amd/fusion.py; the
 * semantics are DESIGN.md section 10).  Not part of the reference, which stops at the depth maps.
 *   depth (V,rows,cols) in world units, <= 0 or NaN = no depth, as a candidate and as a tap.  +inf passes "> 0": as a
 *   candidate it can never be confirmed (kept, as inf, only with min_consistent = 0; its point is not finite), as a tap
 *   it makes its slot inconsistent for every pixel whose tap set holds it; a denormal is a depth like any other
 *   valid (V,rows,cols) u8 or NULL (every depth > 0 valid); any non-zero byte is "valid"
 *   K (V,4,4): the top-left 3x3 is used, its bottom row must be (0,0,1) (not checked)   T_cam_in_world (V,4,4)
 *   ref_views (R) int32, neighbours (R,n_slots) int32 view indices or -1 (skip), 1 <= n_slots <= 32; both on the
 *   device and validated by the caller (out-of-range entries are skipped, never dereferenced)
 * mvsn_fusion_consistency: per reference pixel, every neighbour slot in order: lift, move, project, sample the
 *   neighbour's depth bilinearly (all four taps inside, positive, valid), lift again, move back, project; the slot is
 *   consistent when the pixel lands within max_reproj_px and the depth within max_rel_depth relative.
 *   -> fused_depth (R,rows,cols): (depth + sum of consistent depths) / (count + 1) where count >= min_consistent, else 0
 *      count (R,rows,cols) u8   total (1 int64): the number of kept pixels
 *   workspace: mvsn_fusion_workspace_bytes(R, n_slots, rows, cols) bytes, handed on to mvsn_fusion_emit unchanged
 * mvsn_fusion_emit: the kept pixels, ordered by reference then row-major pixel, at [0, total) of
 *   points (total,3) fp32 world   colors (total,3) u8 from images (V,3,rows,cols) in [-1,1], or NULL   view, pixel (total)
 *   capacity = the total read back to the host: that read is the one host synchronisation of a fusion; 0 = no launch.
 * No atomics: every output is a deterministic function of the inputs.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_fusion_workspace_bytes(int n_ref, int n_slots, int rows, int cols);
int mvsn_fusion_consistency(const float *depth, const uint8_t *valid, const float *K, const float *T_cam_in_world,
                            const int *ref_views, const int *neighbours, int n_views, int n_ref, int n_slots, int rows,
                            int cols, float max_reproj_px, float max_rel_depth, int min_consistent, float *fused_depth,
                            uint8_t *count, int64_t *total, void *workspace, size_t workspace_bytes,
                            mvsn_stream_t stream);
int mvsn_fusion_emit(const float *fused_depth, const float *images, const int *ref_views, int n_ref, int rows, int cols,
                     int n_slots, const void *workspace, size_t workspace_bytes, long capacity, float *points,
                     uint8_t *colors, int *view, int *pixel, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Voxel-grid merge of a point cloud (multi_view_stereonet_amd/fusion.py: voxel_merge; the semantics are DESIGN.md
 * section 12): the points of one grid cell become one point.  Per point and axis, in fp32: s = p - origin,
 * t = s * inv_voxel_size, c = floor(t), f = t - c, q = min(65535, (uint)(f * 65536)).  A point with a non-finite
 * coordinate or t is dropped; a finite point needs -2^20 <= c < 2^20 on every axis.  The points of equal (cx, cy, cz)
 * form a voxel; output rows are ordered by the lowest input index of their voxel.
 *   points (n,3) fp32, colors (n,3) u8 or NULL, 1 <= n <= 2^31 - 1; voxel_size and inv_voxel_size = 1 / voxel_size
 *   are both formed by the caller, in fp32
 * mvsn_voxel_assign: hash-grid build, first-point count and scan.
 *   -> result (2 int64): [0] the number of voxels M, [1] status bits (MVSN_VOXEL_STATUS_*; 0 = fine).  Reading the two
 *      words back is the one host synchronisation of a merge.
 *   workspace: mvsn_voxel_workspace_bytes(n) bytes, 16-byte aligned, handed on to mvsn_voxel_merge unchanged: 16 bytes
 *   per table slot (a power of two >= 2 n slots), 4 bytes per point, 12 bytes per 1024 points.
 * mvsn_voxel_merge: rank, accumulate, finalise.  capacity = M as read back (0 = no launch: every point was dropped and
 *   the caller fills `inverse` with -1).  accumulators: capacity * 64 bytes of scratch, 16-byte aligned.
 *   -> out_points (M,3) fp32: (float)(o + (c + (sum q / count + 0.5) / 65536) * voxel_size) in fp64, one rounding per step
 *      out_colors (M,3) u8 or NULL (with colors): (2 sum C + count) / (2 count) in integers   count (M) int32
 *      first (M) int64: the lowest input index among the voxel's points   inverse (n) int64: row of every point, -1 = dropped
 * Integer atomics only (compare-and-swap on an empty key, minimum, sums): every output is a deterministic function of
 * the inputs, whatever order the points arrive in.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_VOXEL_STATUS_RANGE 1   /* a finite point's cell lies outside [-2^20, 2^20): voxel size too small */
#define MVSN_VOXEL_STATUS_TABLE 2   /* a probe sequence visited every slot without finding room (cannot happen
                                       below 2^30 points: the table is at most half full) */
size_t mvsn_voxel_workspace_bytes(long n);
int mvsn_voxel_assign(const float *points, long n, float voxel_size, float inv_voxel_size, float origin_x,
                      float origin_y, float origin_z, int64_t *result, void *workspace, size_t workspace_bytes,
                      mvsn_stream_t stream);
int mvsn_voxel_merge(const float *points, const uint8_t *colors, long n, float voxel_size, float inv_voxel_size,
                     float origin_x, float origin_y, float origin_z, void *workspace, size_t workspace_bytes,
                     long capacity, void *accumulators, float *out_points, uint8_t *out_colors, int *count,
                     int64_t *first, int64_t *inverse, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Oriented normals from depth maps (multi_view_stereonet_amd/fusion.py: depth_normals, point_normals, voxel_normals;
 * the semantics are DESIGN.md section 13).  Pixel (x, y) = (column, row); a pixel is usable when depth > 0 (a NaN is
 * not) and valid is NULL or non-zero; a neighbour p' of a usable p counts when it is inside the image, usable, and
 * |d' - d| <= max_rel_step * d in fp32 (subtract, multiply, compare), the difference finite.
 * mvsn_depth_normals: X = d * K^-1 (x, y, 1) in fp32 (K^-1 formed per view in fp64, rounded once).  The horizontal
 *   tangent t_u is X(x+1,y) - X(x-1,y) when both neighbours count, the one-sided difference when one does; t_v likewise
 *   from (x,y-1), (x,y+1); c = t_v x t_u faces the camera (x right, y down, z forward); c <- R c with R the top-left 3x3
 *   of the view's T_cam_in_world (assumed to be a rotation) when that is given; n = c / |c|.  (0,0,0) where the pixel is
 *   not usable, a tangent has no neighbour, or |c| is zero or not finite.  Every pixel is written.
 *   depth (V,rows,cols)  valid (V,rows,cols) u8 or NULL  K (V,4,4), top-left 3x3 used, bottom row (0,0,1) assumed
 *   T_cam_in_world (V,4,4) or NULL (camera frame)  max_rel_step >= 0, +inf = no step test  ->  normals (V,3,rows,cols)
 * mvsn_normals_gather: out[i, :] = normals[view[i], :, pixel[i]] for the `count` points of mvsn_fusion_emit (NaN for an
 *   index outside the maps; count = 0: no launch).   normals (n_views,3,pixels_per_view)  view, pixel (count) int32
 *   ->  out (count,3)
 * mvsn_voxel_normals: the mean direction of the points of every row of mvsn_voxel_merge.  Per point each component is
 *   clamped to [-1,1] and quantised, q = (int64)rintf(c * 2^20); a point is skipped when inverse[i] lies outside
 *   [0, m), a component is not finite, or q = (0,0,0); the q of a row are summed with 64-bit integer atomics (exact, in
 *   any order); out = (float)(S / sqrt(Sx^2 + Sy^2 + Sz^2)) in fp64, (0,0,0) where S = 0.  m = 0: no launch.
 *   normals (n,3)  inverse (n) int64  accumulators: m * 24 bytes of scratch, 8-byte aligned  ->  out (m,3)
 * Integer atomics only in the third entry, none in the other two: every output is a deterministic function of the inputs.
 * ------------------------------------------------------------------------------------------- */
int mvsn_depth_normals(const float *depth, const uint8_t *valid, const float *K, const float *T_cam_in_world,
                       int n_views, int rows, int cols, float max_rel_step, float *normals, mvsn_stream_t stream);
int mvsn_normals_gather(const float *normals, const int *view, const int *pixel, int n_views, long pixels_per_view,
                        long count, float *out, mvsn_stream_t stream);
int mvsn_voxel_normals(const float *normals, const int64_t *inverse, long n, long m, void *accumulators, float *out,
                       mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fixed-radius nearest neighbour between two unsorted clouds (multi_view_stereonet_amd/fusion.py: cloud_nearest,
 * radius_outlier_mask; metrics.py: cloud_metrics; the semantics are DESIGN.md section 14).  With h = max_dist in fp32,
 * cell = h, inv_cell = 1 / h and r2 = h * h all formed by the caller in fp32: d2(q, p) = (dx dx + dy dy) + dz dz with
 * dx = qx - px ..., every step one fp32 operation; target p is within when d2 <= r2; the nearest is the within-target of
 * least d2, ties to the lowest row.  The result is that of the brute force over every target point, exactly.  A target
 * with a non-finite coordinate is nobody's neighbour; a query with one gets (+inf, -1, 0); a query may lie anywhere.
 * mvsn_cloud_index_build: the target sorted by cell (section 12's grid: cell size h, origin 0) through the hash table.
 *   target (n,3) fp32, 1 <= n <= 2^31 - 1
 *   -> status (1 int64): MVSN_CLOUD_STATUS_* bits, 0 = fine; reading it back is the one host synchronisation of a query
 *   workspace: mvsn_cloud_workspace_bytes(n) bytes, 16-byte aligned, handed on to mvsn_cloud_nearest unchanged: 20
 *   bytes per table slot (a power of two >= 2 n slots: key, population, start, cursor), 20 bytes per point (its slot,
 *   its 16-byte record), 12 bytes per 1024 slots.
 * mvsn_cloud_nearest: one thread per query point walks the records of the cells within reach.
 *   query (nq,3) fp32, 1 <= nq <= 2^31 - 1; n_target as given to the build
 *   -> dist2 (nq) fp32: d2 to the nearest target within max_dist, +inf where none   index (nq) int64: its row, -1
 *      within (nq) int32: the number of targets with d2 <= r2
 * Integer atomics only, in the build (compare-and-swap on an empty key, sums, a cursor whose order of arrival no output
 * depends on): every output is a deterministic function of the inputs.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_CLOUD_STATUS_RANGE 1   /* a finite target's cell lies outside [-2^20, 2^20): max_dist too small */
#define MVSN_CLOUD_STATUS_TABLE 2   /* a probe sequence visited every slot without finding room (cannot happen
                                       below 2^30 points: the table is at most half full) */
size_t mvsn_cloud_workspace_bytes(long n_target);
int mvsn_cloud_index_build(const float *target, long n, float cell, float inv_cell, int64_t *status, void *workspace,
                           size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_cloud_nearest(const float *query, long nq, float inv_cell, float r2, const void *workspace,
                       size_t workspace_bytes, long n_target, float *dist2, int64_t *index, int *within,
                       mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Registration of one cloud to another: Gauss-Newton (ICP) on the residual between a moved source point and its nearest
 * target point (multi_view_stereonet_amd/fusion.py: cloud_register, cloud_register_system; the semantics and every fp32
 * step are DESIGN.md section 20).  The target's index is mvsn_cloud_index_build's (index_workspace, its
 * mvsn_cloud_workspace_bytes(n_target) bytes, inv_cell and r2 as given to mvsn_cloud_nearest): built once, it serves
 * any number of sources.  source (n_source,3), weights (n_source) or NULL, target (n_target,3) as given to the build,
 * target_normals (n_target,3) or NULL, all fp32; 1 <= n_source, n_target <= 2^31 - 1.  T (16 fp32, row-major 4 x 4) maps
 * source coordinates into the target's frame; centre (3 fp32) is the point the rotation update turns about.  T and
 * centre are DEVICE pointers.
 * Per source point, with the pose's twelve numbers rounded once to fp32: p'_a = ((R_a0 x + R_a1 y) + R_a2 z) + t_a; its match is
 *   mvsn_cloud_nearest's of p'; d = p' - target[match]; q = p' - centre.  With target_normals (point-to-plane):
 *   r = (d.x n.x + d.y n.y) + d.z n.z, J = (n, q x n), each product rounded, then one subtraction.  Without
 *   (point-to-point): three rows r = d_a, J_a = (e_a, q x e_a), and sum w r^2 adds w d2 of the query.  The point takes
 *   part iff its row and p' are finite, its weight w (1 without weights) is finite and > 0, a match exists, and in plane
 *   mode the match's normal is finite.  In fp64: H = sum (w J) J^T, b = sum (w J) r, sum w, sum (w r) r, the count,
 *   summed in an order that n_source alone fixes (at most 1024 workgroups, each on blocks of 1024 rows 1024 blocks
 *   apart; no atomics: bitwise reproducible).
 * mvsn_cloud_register_system evaluates that once at T:
 *   H (6,6), b (6), sums (3) = (count, sum w, sum w r^2), all fp64; index (n_source) int64 and residual (n_source)
 *   fp32, both or neither NULL: the matched row and r (plane mode) or d2 (point mode) where the point takes part,
 *   -1 and NaN elsewhere, every row written once.
 * mvsn_cloud_register iterates, iterations (0 to 1000) times: stop with status 1 if count < min_points; scale H to a
 *   unit diagonal and take its Cholesky factor, stop with status 2 at a diagonal entry that is not a positive finite
 *   number, a pivot < min_pivot (inside (0, 1)) or an update that is not finite; solve H (v, omega) = -b and apply
 *   R <- exp([omega]x) R, t <- exp([omega]x) (t - centre) + centre + v to the fp64 pose.  A stopped run keeps its pose.
 *   T_out (16 fp32): the final pose, each number rounded once, T_init's bottom row; history (iterations+1,3) fp64:
 *   (count, sum w, sum w r^2) at the pose before update i, the last row at the final pose; status (1 int32);
 *   information (6,6) fp64: H at the final pose.  iterations + 1 pairs of launches; nothing waits on another workgroup
 *   and nothing is read on the host.
 * workspace: mvsn_cloud_register_workspace_bytes(n_source) bytes (0 for what the entries refuse), 16-byte aligned: the
 *   fp64 pose and a record of 30 doubles per workgroup.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_cloud_register_workspace_bytes(long n_source);
int mvsn_cloud_register_system(const float *source, long n_source, const float *weights, const float *target,
                               const float *target_normals, long n_target, float inv_cell, float r2,
                               const void *index_workspace, size_t index_workspace_bytes, const float *T,
                               const float *centre, void *workspace, size_t workspace_bytes, double *H, double *b,
                               double *sums, int64_t *index, float *residual, mvsn_stream_t stream);
int mvsn_cloud_register(const float *source, long n_source, const float *weights, const float *target,
                        const float *target_normals, long n_target, float inv_cell, float r2,
                        const void *index_workspace, size_t index_workspace_bytes, const float *T_init,
                        const float *centre, int iterations, long min_points, double min_pivot, void *workspace,
                        size_t workspace_bytes, float *T_out, double *history, int *status, double *information,
                        mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Normals of a bare cloud: for every query point the principal axes of the covariance of the support points within the
 * radius (multi_view_stereonet_amd/fusion.py: cloud_normals; the semantics and every step are DESIGN.md section 21).
 * The support's index is mvsn_cloud_index_build's (index_workspace, its mvsn_cloud_workspace_bytes(n_target) bytes;
 * cell = h, inv_cell = 1 / h and r2 = h * h as given to the build and to mvsn_cloud_nearest): built once, it serves any
 * number of query sets.
 *   query (nq,3) fp32, 1 <= nq <= 2^31 - 1; viewpoint (viewpoint_rows,3) fp32 with viewpoint_rows 1 or nq, or NULL with
 *   viewpoint_rows 0; min_neighbours >= 3; min_gap inside [0, 1)
 *   -> normals (nq,3) fp32   eigenvalues (nq,3) fp32 or NULL   count (nq) int32, every element written once
 * A support point is a neighbour exactly when mvsn_cloud_nearest counts it: count is its `within`.  Per neighbour, with
 * d = query - point as the walk forms it: u_a = (int)rintf((d_a * inv_cell) * 2^20), each step one fp32 operation
 * (|u_a| < 2^21); the count n, the three sums S_a of u_a and the six sums S_ab of u_a u_b are exact 64-bit integers.  In
 * fp64, one operation per step: m_a = S_a / n, C_ab = S_ab / n - m_a m_b; six cyclic Jacobi sweeps over the pairs (0,1),
 * (0,2), (1,2) (theta = (C_qq - C_pp) / (2 C_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1),
 * s = t c; a pair whose C_pq is 0 is skipped); the eigenpairs sorted ascending.  eigenvalues = lambda (cell 2^-20)^2 in
 * fp64, rounded once; (0,0,0) where n = 0 or n > 2^20 (the sums could overflow; count stays exact).  normals = the unit
 * eigenvector of lambda_0, rounded once per component, or (0,0,0) where n < min_neighbours, n > 2^20 or
 * lambda_1 - lambda_0 <= min_gap lambda_2.  Its sign: the component of largest magnitude positive (ties to the lowest
 * axis); with a finite viewpoint row v, flipped where (n_x (v_x - q_x) + n_y (v_y - q_y)) + n_z (v_z - q_z) < 0 in fp64
 * and kept canonical where that is 0.  One launch, no atomics: every output is a bitwise-reproducible function of the
 * inputs and does not depend on the order of the support's rows.
 * ------------------------------------------------------------------------------------------- */
int mvsn_cloud_normals(const float *query, long nq, const float *viewpoint, long viewpoint_rows, float cell,
                       float inv_cell, float r2, long min_neighbours, double min_gap, const void *index_workspace,
                       size_t index_workspace_bytes, long n_target, float *normals, float *eigenvalues, int *count,
                       mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The k nearest neighbours between two clouds within a radius, and the statistics of the statistical outlier filter
 * (multi_view_stereonet_amd/fusion.py: cloud_knn, statistical_outlier_mask; the semantics are DESIGN.md section 22).
 * The target's index is mvsn_cloud_index_build's (index_workspace, its mvsn_cloud_workspace_bytes(n_target) bytes; cell,
 * inv_cell and r2 as given to the build and to mvsn_cloud_nearest): built once, it serves any number of query sets.
 * mvsn_cloud_knn: one thread per query point.
 *   query (nq,3) fp32, 1 <= nq <= 2^31 - 1; 1 <= k <= 64; exclude_self 0 or not 0
 *   A target is a candidate exactly when mvsn_cloud_nearest counts it (its fp32 d2 <= r2; a NaN never is) and, with
 *   exclude_self, its row is not the query's row.  The key of a candidate is (uint64(bits of d2) << 32) | row; the result
 *   is the k least keys in ascending order: that of the brute force over every target and a stable sort on (d2, row),
 *   whatever the order of the target's rows in the index.
 *   -> dist2 (nq,k) fp32 and index (nq,k) int64, row-major: slot j the j-th nearest, +inf and -1 from the number of
 *      candidates on   within (nq) int32: the number of candidates   mean (nq) fp64 or NULL:
 *      (sum_j sqrt((double)dist2[j])) / k, summed for j = 0 .. k-1 in that order from 0, one fp64 operation per step; NaN
 *      with fewer than k candidates.  Every element written once.
 *   A query with a non-finite coordinate gets all +inf / -1, within 0 and mean NaN; a non-finite target is nobody's
 *   neighbour; a query may lie anywhere.  mvsn_cloud_knn at k = 1 is mvsn_cloud_nearest bit for bit.
 * mvsn_cloud_mean_stats: mean (n) fp64, 1 <= n <= 2^31 - 1 -> stats (3) fp64 = (count, mu, sigma) over the entries that
 *   are not NaN: mu = (sum m) / count (NaN for count 0), sigma = sqrt((sum (m - mu)^2) / (count - 1)) (0 for count < 2),
 *   two passes.  Both sums in fp64 in an order that n alone fixes (at most 1024 workgroups, each on blocks of 1024 rows
 *   1024 blocks apart, then one workgroup over their records).
 *   workspace: mvsn_cloud_mean_stats_workspace_bytes(n) bytes (0 for what the entry refuses), 16-byte aligned.
 * No atomics, nothing waits on another workgroup, nothing is read on the host: every output is a bitwise-reproducible
 * function of the inputs.
 * ------------------------------------------------------------------------------------------- */
int mvsn_cloud_knn(const float *query, long nq, int k, int exclude_self, float cell, float inv_cell, float r2,
                   const void *index_workspace, size_t index_workspace_bytes, long n_target, float *dist2,
                   int64_t *index, int *within, double *mean, mvsn_stream_t stream);
size_t mvsn_cloud_mean_stats_workspace_bytes(long n);
int mvsn_cloud_mean_stats(const double *mean, long n, void *workspace, size_t workspace_bytes, double *stats,
                          mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Global registration of two clouds: FPFH descriptors, nearest neighbours in descriptor space, RANSAC over the
 * correspondences (multi_view_stereonet_amd/fusion.py: cloud_fpfh, feature_nearest, cloud_ransac, cloud_register_global;
 * the semantics and the exact arithmetic of every step are DESIGN.md section 23).
 * mvsn_cloud_fpfh: points and normals (n,3) fp32, 1 <= n <= 2^31 - 1; the index is mvsn_cloud_index_build's of the points
 *   themselves (index_workspace, its mvsn_cloud_workspace_bytes(n) bytes; cell = radius, inv_cell and r2 as given to the
 *   build); min_neighbours >= 1.  Two launches, one thread per point.
 *   A pair (i, j) counts when mvsn_cloud_nearest counts j for i (fp32 d2 <= r2), j != i, d2 != 0 and both normals are
 *   finite and not (0,0,0).  Its Darboux triple, every step one fp32 operation: e = p_j - p_i, a_i = n_i . e, a_j = n_j . e
 *   ((x + y) + z); the source s is i where |a_i| > |a_j|, j where |a_j| > |a_i|, the lower row at a tie; u = n_s,
 *   l = (p_t - p_s) / sqrt(d2) per component, f2 = u . l, v = u x l, w = u x v, f1 = v . n_t, and f3 the angle of
 *   (u . n_t, w . n_t).  Bins: floor(((f + 1) 11) / 2) clamped to 0 .. 10 for f1 and f2; for f3 the sector of
 *   [-pi, pi] / 11 found by the signs of b_k x (c, s) against the ten inner boundary directions b_k (fp32 literals).
 *   -> spfh (n,33) int32: the counts, f1's 11 bins, then f2's, then f3's   pairs (n) int32: K_i, the number of pairs
 *   -> features (n,33) fp32: with A[b] = sum over the pairs (i, j) with K_j > 0 (n' of them) of
 *      rint(((w 2^20) spfh_j[b]) / K_j), w = r2 / max(d2, r2 2^-20), every step one fp64 operation and the sum an exact
 *      64-bit integer, F[b] = spfh_i[b] / K_i + (A[b] 2^-20) / n' (the second term 0 where n' = 0) in fp64, and each
 *      11-bin block scaled to (F[b] 100) / (sum of the block, from its first bin upwards), rounded to fp32 once.  A row
 *      with K_i < min_neighbours or n' > 2^20 is all zero.  Every element written once.
 * mvsn_cloud_feature_nearest: query (nq,dim) and target (nt,dim) fp32, dim = 33 (anything else: MVSN_E_BADARG),
 *   1 <= nq, nt <= 2^31 - 1.  A row of either side takes part iff its 33 values are finite and not all zero.
 *   d2 = sum_b (q_b - t_b)^2 from b = 0 upwards, one fp32 operation per step; the key of a target is
 *   (uint64(bits of d2) << 32) | row.  -> index (nq) int64 and dist2 (nq) fp32: the least key's row and d2 (ties to the
 *   lowest row), -1 and +inf where the query takes no part or no target does; second_dist2 (nq) fp32: the second least
 *   key's d2, +inf where there is none.  One launch; eight waves share 64 query rows and merge their least keys.
 * mvsn_cloud_feature_mutual: index (nq) int64 into nt rows, back (nt) int64 into nq rows
 *   -> mutual (nq) bytes: 1 where 0 <= index[i] < nt and back[index[i]] == i, else 0.
 * mvsn_cloud_ransac: source (ns,3), target (nt,3) fp32; correspondences (c,2) int64 of (source row, target row), 1 <= ns,
 *   nt, c <= 2^31 - 1; r2 > 0 the squared inlier distance; edge_similarity inside (0, 1]; 1 <= hypotheses <= 2^24 (below:
 *   MVSN_E_BADARG, above: MVSN_E_TOOLARGE); workspace: mvsn_cloud_ransac_workspace_bytes() bytes, 16-byte aligned, cleared
 *   by a memset on the stream.  A correspondence with a row outside its cloud takes no part and is never dereferenced.
 *   Hypothesis h draws j = 0, 1, 2: z = seed + (3 h + j + 1) 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) 0x94D049BB133111EB; z = z ^ z >> 31 (all mod 2^64); the draw is ((z >> 32) c) >> 32.  It is
 *   rejected when two draws coincide, a drawn row lies outside its cloud, a drawn point is not finite, for a pair of
 *   draws min(|ds|^2, |dt|^2) < edge_similarity^2 max(|ds|^2, |dt|^2), a triangle has |a x b|^2 <= 2^-40 |a|^2 |b|^2
 *   (a = p1 - p0, b = p2 - p0), or the pose is not finite.  In fp64, one operation per step: e1 = a / sqrt(|a|^2),
 *   e3 = (e1 x b) / |e1 x b|, e2 = e3 x e1 for both triangles, R_ij = (e1t_i e1s_j + e2t_i e2s_j) + e3t_i e3s_j,
 *   c = ((p0 + p1) + p2) / 3, t = c_t - R c_s.  Its count: the correspondences with |(R s + t) - t_j|^2 <= (double)r2.
 *   The winner has the most inliers, ties to the lowest h.
 *   -> T (16 fp32) and T64 (16 fp64): the winner's pose, row-major 4x4   best (3 int64) = (hypothesis, inliers, status)
 *      inlier (c) bytes: 1 for the winner's inliers.  status 0; 1: fewer than 3 correspondences with both rows inside
 *      and finite; 2: every hypothesis rejected.  With status 1 or 2: T the identity, best = (-1, 0, status), inlier 0.
 *   Two launches and nothing read on the host; the only atomic is a 64-bit integer maximum: every output is a
 *   bitwise-reproducible function of the inputs.
 * ------------------------------------------------------------------------------------------- */
int mvsn_cloud_fpfh(const float *points, const float *normals, long n, float cell, float inv_cell, float r2,
                    long min_neighbours, const void *index_workspace, size_t index_workspace_bytes, int *spfh,
                    int *pairs, float *features, mvsn_stream_t stream);
int mvsn_cloud_feature_nearest(const float *query, long nq, const float *target, long nt, int dim, int64_t *index,
                               float *dist2, float *second_dist2, mvsn_stream_t stream);
int mvsn_cloud_feature_mutual(const int64_t *index, long nq, const int64_t *back, long nt, unsigned char *mutual,
                              mvsn_stream_t stream);
size_t mvsn_cloud_ransac_workspace_bytes(void);
int mvsn_cloud_ransac(const float *source, long ns, const float *target, long nt, const int64_t *correspondences, long c,
                      float r2, double edge_similarity, long hypotheses, unsigned long long seed, void *workspace,
                      size_t workspace_bytes, float *T, double *T64, int64_t *best, unsigned char *inlier,
                      mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dense TSDF volume: depth maps integrated along the viewing rays, and a mesh taken from the volume by Surface Nets
 * (multi_view_stereonet_amd/tsdf.py; the semantics, every fp32 step and the error bounds are DESIGN.md section 15).
 * The state is planar fp32 in the layout (nz,ny,nx), x fastest: sdf_sum = sum w t, weight = sum w, color_sum
 * (3,nz,ny,nx) = sum w rgb or NULL; at most 2^31 - 1 voxels and 2^24 along an axis (rows and cols of the maps too: every
 * index is an exact fp32); the centre of voxel (i,j,k) is origin + voxel_size (i,j,k).
 * mvsn_tsdf_integrate: per voxel centre p and view v in index order, with P_v = K_v T_v^-1 (3x4; fp64, rounded once;
 *   K's bottom row taken to be (0,0,1)): z = P row 2 . (p,1); skip unless z > min_depth; (u, v) = rows 0, 1 over z;
 *   col = floor(u + 0.5), row = floor(v + 0.5), skip unless inside the map; D = depth[v,row,col], skip unless D is finite
 *   and > 0, valid (if given) is non-zero and the weight w (1 without weights) is finite and > 0; sdf = D - z, skip if
 *   sdf < -trunc; t = min(sdf, trunc); sdf_sum = fma(w, t, sdf_sum), weight += w, color_sum = fma(w, rgb, color_sum).
 *   The state is read once and written once whatever n_views is; a voxel no view updates keeps its bits; nothing outside
 *   the maps is read.  One launch, no workspace, no atomics.
 *   depth (V,rows,cols)  valid (V,rows,cols) u8 or NULL  weights (V,rows,cols) or NULL  images (V,3,rows,cols) with
 *   color_sum, or both NULL  K, T_cam_in_world (V,4,4)  1 <= V <= 65535
 * mvsn_tsdf_camera_batch: the number of cameras the integration stages at once (more views loop inside the launch).
 * mvsn_tsdf_classify / mvsn_tsdf_extract: Surface Nets.  A corner is observed when weight >= min_weight (its sdf_sum is
 *   read only then) and inside when d = sdf_sum / weight < 0; cell (i,j,k), i < nx - 1 ..., is active when its 8 corners
 *   are observed and not all of one sign; a grid edge (voxel a, axis) with observed endpoints of different sign emits a
 *   quad when the 4 cells around it exist and are active.  Dims of at least 2 each.
 *   classify (two launches and an 8-byte device copy) -> result (2 int64): [0] the number of vertices M, [1] M + the
 *     number of quads; reading them back is the one host synchronisation of an extraction.
 *   workspace: mvsn_tsdf_workspace_bytes(nx, ny, nz) bytes, 16-byte aligned, handed on to mvsn_tsdf_extract unchanged:
 *     5 bytes per voxel (a code byte, the cell -> row int32 map), 24 bytes per 1024 voxels.
 *   extract (three launches; n_vertices = 0: none) -> vertices (M,3): the mean of the cell's edge crossings
 *     p0 + d0 / (d0 - d1) along the edge, in a fixed edge order; normals (M,3): the normalised sum of the differences of
 *     d along the cell's 4 edges of each axis, (0,0,0) where that is zero or not finite; colors (M,3) u8 with color_sum,
 *     or both NULL; cell (M) int64: the cell's linear index (k ny + j) nx + i, ascending; faces (2 quads,3) int64: two
 *     triangles per quad, counter-clockwise seen from the positive side, ordered by (linear index of a) * 3 + axis.
 * No atomics: every output is a deterministic function of the three state tensors.
 * ------------------------------------------------------------------------------------------- */
int mvsn_tsdf_camera_batch(void);
int mvsn_tsdf_integrate(const float *depth, const uint8_t *valid, const float *weights, const float *images,
                        const float *K, const float *T_cam_in_world, int n_views, int rows, int cols, int nx, int ny,
                        int nz, float voxel_size, float origin_x, float origin_y, float origin_z, float trunc,
                        float min_depth, float *sdf_sum, float *weight, float *color_sum, mvsn_stream_t stream);
size_t mvsn_tsdf_workspace_bytes(int nx, int ny, int nz);
int mvsn_tsdf_classify(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float min_weight,
                       int64_t *result, void *workspace, size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_tsdf_extract(const float *sdf_sum, const float *weight, const float *color_sum, int nx, int ny, int nz,
                      float voxel_size, float origin_x, float origin_y, float origin_z, float min_weight,
                      const void *workspace, size_t workspace_bytes, long n_vertices, long n_quads, float *vertices,
                      float *normals, uint8_t *colors, int64_t *faces, int64_t *cell, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Oriented points into the TSDF volume (tsdf.TSDFVolume.integrate_cloud; the semantics and every step are DESIGN.md
 * section 31): the implicit moving-least-squares distance of the cloud, Hoppe's weighted tangent planes, added to the
 * state of mvsn_tsdf_integrate.  points, normals (n,3) fp32 (normals outwards, used as given), weights (n) fp32 or NULL
 * (1), colors (n,3) u8 with color_sum, or both NULL.  index_workspace is what mvsn_cloud_index_build made over points
 * with cell; inv_cell = 1 / cell and r2 = cell * cell, each formed once in fp32.
 *   Per voxel centre x = origin + (float)i * voxel_size (a multiply, then an add) and every row p within reach, d2 =
 *   (dx dx + dy dy) + dz dz <= r2 of the fp32 differences dx = x - p (mvsn_cloud_nearest's relation), whose point is
 *   finite, whose normal is finite and not (0,0,0) and whose weight w is finite and in (0, 256]:
 *     q = d2 / r2, a = 1 - q, phi = a a, A = rint((phi w) 2^16); s = (dx nx + dy ny) + dz nz,
 *     t = fmin(fmax(s, -trunc), trunc), T = rint((t / trunc) 2^20); every step one fp32 operation.
 *   Exact 64-bit sums per voxel: the count, sum A, sum A T, sum A c per channel.  A voxel with sum A > 0 and at most
 *   2^19 - 1 accepted rows gets, each number formed in fp64 and rounded once: weight += sum A 2^-16, sdf_sum +=
 *   sum A T (trunc 2^-36), color_sum_c += (sum A c 2^-16) / 127.5 - sum A 2^-16; any other voxel keeps its bits.
 *   No byte of the state depends on the order of the rows.  A memset and two launches, no atomics.
 *   workspace: mvsn_tsdf_cloud_workspace_bytes(nx, ny, nz) bytes (0: dims outside the limits), 16-byte aligned: one
 *   flag byte per brick of 8 x 8 x 8 voxels.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_tsdf_cloud_workspace_bytes(int nx, int ny, int nz);
int mvsn_tsdf_cloud_integrate(const float *points, const float *normals, const float *weights, const uint8_t *colors,
                              long n, const void *index_workspace, size_t index_workspace_bytes, float cell,
                              float inv_cell, float r2, int nx, int ny, int nz, float voxel_size, float origin_x,
                              float origin_y, float origin_z, float trunc, float *sdf_sum, float *weight,
                              float *color_sum, void *workspace, size_t workspace_bytes, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ray-cast of the TSDF volume: the surface as cameras (K, T_cam_in_world) see it (tsdf.TSDFVolume.raycast; the
 * semantics, every fp32 step and the error bounds are DESIGN.md section 16).  The state is mvsn_tsdf_integrate's, dims of
 * at least 2 each; K, T_cam_in_world (V,4,4), K's bottom row taken to be (0,0,1); 1 <= V <= 65535, rows, cols <= 2^24,
 * rows * cols <= 2^31 - 1; pixel (x, y) = (column, row), integer at the centre.
 * Per view A = R K^-1 / voxel_size and g0 = (t - origin) / voxel_size (fp64, each number rounded once); per pixel
 *   dir_a = fma(A_a0, x, fma(A_a1, y, A_a2)); sample k >= 1 at t_k = (float)k * step takes part iff min_depth < t_k <=
 *   max_depth (max_depth may be +infinity); g = fma(t_k, dir, g0), cell c = floor(g), in range iff 0 <= c_a <= N_a - 2;
 *   the sample is defined iff it is in range and the 8 corners of c have weight >= min_weight, and its value is the
 *   trilinear interpolant (x, then y, then z, each lerp fma(fr, hi - lo, lo)) of d = sdf_sum / weight.  The hit is the
 *   first k with samples k - 1 and k defined, f_{k-1} >= 0 and f_k < 0: depth = fma(step, f_{k-1} / (f_{k-1} - f_k),
 *   t_{k-1}); a pair with f_{k-1} < 0 <= f_k ends the ray without a hit; an undefined sample resets the pair.  At the hit
 *   point, if its cell is defined: weight_out = the interpolant of weight, colors = that of color_sum / weight, normals =
 *   the normalised analytic gradient of the interpolant of d (world frame, pointing to free space; (0,0,0) where its
 *   length is 0 or not finite).  A pixel without a hit gets zeros in all four maps; every pixel is written once.
 *   depth (V,rows,cols)  normals (V,3,rows,cols)  colors (V,3,rows,cols) with color_sum, or both NULL
 *   weight_out (V,rows,cols)
 *   workspace: mvsn_tsdf_raycast_workspace_bytes(nx, ny, nz) bytes (0 for dims the entry refuses), 16-byte aligned: 4
 *     bytes per voxel, the plane d with a NaN at an unobserved voxel, written by the first of the two launches.
 *   MVSN_E_TOOLARGE when voxel_size |(nx-1,ny-1,nz-1)| / step + 2, the most samples a ray holds inside the box, is
 *   above 2^20.  That count takes T_cam_in_world to be rigid (an orthonormal rotation part, so that depth grows no
 *   faster than metric length); it also bounds the march, so under a T that shrinks lengths the samples of a ray
 *   behind that count are not examined.  Nothing outside the planes is read; no atomics: the outputs are bitwise reproducible, and a view's maps
 *   do not depend on the other views of the call.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_tsdf_raycast_workspace_bytes(int nx, int ny, int nz);
int mvsn_tsdf_raycast(const float *sdf_sum, const float *weight, const float *color_sum, int nx, int ny, int nz,
                      float voxel_size, float origin_x, float origin_y, float origin_z, const float *K,
                      const float *T_cam_in_world, int n_views, int rows, int cols, float min_weight, float min_depth,
                      float max_depth, float step, void *workspace, size_t workspace_bytes, float *depth,
                      float *normals, float *colors, float *weight_out, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Alignment of depth maps to the TSDF volume: Gauss-Newton on the point-to-TSDF residual (tsdf.TSDFVolume.align; the
 * semantics, every fp32 step and the error bounds are DESIGN.md section 17).  The state, K, T_cam_in_world and the limits
 * are mvsn_tsdf_raycast's; depth (V,rows,cols) fp32, valid (V,rows,cols) bytes or NULL, weights (V,rows,cols) fp32 or
 * NULL; 1 <= stride <= 2^24: the pixels with x % stride == 0 and y % stride == 0 are looked at.
 * Per view the camera A, g0 of the ray-cast from the current fp64 pose; per pixel with depth D the grid point
 *   g = fma(D, dir, g0), its cell, fractions, trilinear value f and analytic gradient as in the ray-cast.  The pixel
 *   takes part iff D is finite and > 0, valid is set, its weight w (1 without weights) is finite and > 0, the cell is in
 *   range with its 8 corners at weight >= min_weight, |f| <= band and n = gradient / voxel_size is finite.  Then
 *   r = f / voxel_size, q = g - (N - 1) / 2, J = (n, q x n) in fp32, and in fp64 H = sum w J J^T, b = sum w J r, sum w,
 *   sum w r^2 and the count, summed in an order the launch geometry fixes (no atomics: bitwise reproducible, and a view's
 *   results do not depend on the other views).
 * mvsn_tsdf_align_system evaluates that once at T_cam_in_world:
 *   H (V,6,6), b (V,6), sums (V,3) = (count, sum w, sum w r^2), all fp64; residual (V,rows,cols) fp32 or NULL: r where
 *   the pixel takes part, NaN elsewhere, every pixel written once.
 * mvsn_tsdf_align iterates: iterations (0 to 1000) times, per view: stop with status 1 if count < min_pixels; scale H to
 *   a unit diagonal and take its Cholesky factor, stop with status 2 at a diagonal entry that is not a positive finite
 *   number or a pivot < min_pivot (inside (0, 1)); solve H (v, omega) = -b and apply R <- exp([omega]x) R,
 *   t <- exp([omega]x) (t - cw) + cw + voxel_size v about the volume's centre cw.  A stopped view keeps its pose.
 *   T_out (V,4,4) fp32: the final poses, each number rounded once from the fp64 pose, T_cam_in_world's bottom rows;
 *   history (V,iterations+1,3) fp64: (count, sum w, sum w r^2) at the pose before update i, the last row at the final
 *   pose; status (V) int32: 0, or what stopped the view; information (V,6,6) fp64: H at the final pose.
 *   The launches: the values pass once, then iterations + 1 times the sums and their reduction per view, which solves
 *   in all but the last.  Nothing waits on another workgroup and nothing is read on the host.
 * workspace: mvsn_tsdf_align_workspace_bytes(nx, ny, nz, n_views, rows, cols, stride) bytes (0 for what the entries
 *   refuse), 16-byte aligned: the plane d, the fp64 poses and a record of 30 doubles per workgroup.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_tsdf_align_workspace_bytes(int nx, int ny, int nz, int n_views, int rows, int cols, int stride);
int mvsn_tsdf_align_system(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float voxel_size,
                           float origin_x, float origin_y, float origin_z, const float *depth, const uint8_t *valid,
                           const float *weights, const float *K, const float *T_cam_in_world, int n_views, int rows,
                           int cols, int stride, float min_weight, float band, void *workspace, size_t workspace_bytes,
                           double *H, double *b, double *sums, float *residual, mvsn_stream_t stream);
int mvsn_tsdf_align(const float *sdf_sum, const float *weight, int nx, int ny, int nz, float voxel_size, float origin_x,
                    float origin_y, float origin_z, const float *depth, const uint8_t *valid, const float *weights,
                    const float *K, const float *T_cam_in_world, int n_views, int rows, int cols, int stride,
                    float min_weight, float band, int iterations, long min_pixels, double min_pivot, void *workspace,
                    size_t workspace_bytes, float *T_out, double *history, int *status, double *information,
                    mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Connected components of a triangle mesh, and the mesh of the components one keeps (multi_view_stereonet_amd/mesh.py:
 * mesh_components, filter_mesh; the semantics, the termination and the visibility argument are DESIGN.md section 18).
 * The graph has the n_vertices rows as nodes and the sides of the faces as edges; a face with an index outside
 * [0, n_vertices) takes no part (label -1; the index is never used as an address); a vertex no face uses is a component
 * of its own.  Component ids are dense and ordered by the component's lowest vertex row.
 *   faces (n_faces,3) int64 (NULL with n_faces = 0)   1 <= n_vertices <= 2^31 - 1   0 <= n_faces <= 2^31 - 1
 *   workspace: mvsn_mesh_workspace_bytes(n_vertices, n_faces) bytes (0 for sizes the entries refuse), 16-byte aligned:
 *     a head of 16 bytes, 8 bytes per vertex (parent, and the root -> id map that mvsn_mesh_select reuses as the vertex
 *     row map), 12 bytes per 256 vertices and per 256 faces.
 * mvsn_mesh_components_label (init, hook, flatten, the scan and a 16-byte device copy): a lock-free union-find over
 *   int32 `parent` in the workspace, one thread per face; a root is hooked under a lower root by a compare-and-swap, so
 *   every walk descends and every loop is bounded by n_vertices, whatever the schedule.
 *   -> result (2 int64): [0] the number of components C, [1] status bits (MVSN_MESH_STATUS_*; 0 = fine).  Reading the
 *      two words back is the one host synchronisation of a labelling.
 * mvsn_mesh_components_emit (three launches), on the workspace handed on unchanged, n_components = C as read back
 *   (outside [1, n_vertices] it cannot be this workspace's: MVSN_E_BADARG):
 *   -> vertex_label (n_vertices) int64   face_label (n_faces) int64: the label of the face's first index, or -1
 *      vertex_count, face_count, first (C) int64: the sizes of every component and its lowest vertex row
 * mvsn_mesh_select (count, the scan, rank, an 8-byte device copy): keep (C) bytes, non-zero = the component stays; the
 *   labels as emitted (a label outside [0, C) is dropped).  Needs no labelling in the workspace, and overwrites its map.
 *   -> result (2 int64): [0] the kept vertices M', [1] M' + the kept faces F'; the workspace holds the vertex row map
 *      (int32, -1 for a dropped vertex).
 * mvsn_mesh_compact (two launches; n_vertices_out = 0: none), on select's workspace, with M' and F' as read back:
 *   vertices, normals (n_vertices,3) fp32, copied as bits; colors (n_vertices,3) u8 with out_colors, or both NULL;
 *   cell (n_vertices) int64
 *   -> the rows of the kept vertices and faces in their input order, out_faces renumbered through the row map;
 *      vertex_rows (M'), face_rows (F') int64: the input row of every output row.
 * Integer atomics only (a compare-and-swap on a root, relaxed loads and stores of parent, sums), no float arithmetic:
 * every output is a deterministic function of the inputs, whatever order the faces come in.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_MESH_STATUS_WORKSPACE 1   /* a walk over `parent` ran out of its bound or met a parent above its vertex:
                                          the workspace was overwritten during the call (cannot happen otherwise) */
size_t mvsn_mesh_workspace_bytes(long n_vertices, long n_faces);
int mvsn_mesh_components_label(const int64_t *faces, long n_vertices, long n_faces, int64_t *result, void *workspace,
                               size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_components_emit(const int64_t *faces, long n_vertices, long n_faces, void *workspace,
                              size_t workspace_bytes, long n_components, int64_t *vertex_label, int64_t *face_label,
                              int64_t *vertex_count, int64_t *face_count, int64_t *first, mvsn_stream_t stream);
int mvsn_mesh_select(const int64_t *vertex_label, const int64_t *face_label, const uint8_t *keep, long n_vertices,
                     long n_faces, long n_components, int64_t *result, void *workspace, size_t workspace_bytes,
                     mvsn_stream_t stream);
int mvsn_mesh_compact(const float *vertices, const float *normals, const uint8_t *colors, const int64_t *cell,
                      const int64_t *faces, const int64_t *face_label, const uint8_t *keep, long n_vertices, long n_faces,
                      long n_components, const void *workspace, size_t workspace_bytes, long n_vertices_out,
                      long n_faces_out, float *out_vertices, float *out_normals, uint8_t *out_colors, int64_t *out_cell,
                      int64_t *out_faces, int64_t *vertex_rows, int64_t *face_rows, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Density-based clusters of a cloud: DBSCAN, and with min_points = 1 Euclidean cluster extraction
 * (multi_view_stereonet_amd/fusion.py: cloud_clusters, cloud_cluster_mask; the semantics and the argument are DESIGN.md
 * section 24).  The index is mvsn_cloud_index_build's of the points themselves (index_workspace, its
 * mvsn_cloud_workspace_bytes(n) bytes; inv_cell and r2 as given to the build and to mvsn_cloud_nearest).
 *   points (n,3) fp32, 1 <= n <= 2^31 - 1; min_points >= 1
 *   Row j is a neighbour of row i exactly when mvsn_cloud_nearest of the cloud against itself counts it (fp32 d2 <= r2,
 *   both rows finite; a point is its own neighbour): a relation that is symmetric bit for bit.  A row is core when it is
 *   finite and has at least min_points neighbours.  A cluster is a connected component of the core rows under the
 *   relation; its id is its rank among the clusters ordered by their lowest core row.  A finite row that is not core
 *   joins the cluster of the core neighbour with the least key (uint64(bits of d2) << 32) | row, and is noise (-1)
 *   without one; a row that is not finite is noise.
 *   workspace: mvsn_cloud_cluster_workspace_bytes(n) bytes (0 for sizes the entries refuse), 16-byte aligned: a head of
 *     16 bytes, 8 bytes per point (parent, and the root -> id map), 12 bytes per 256 points.
 * mvsn_cloud_cluster_label (core, hook, flatten, the scan and a 16-byte device copy): one thread per point; the
 *   lock-free union-find of mvsn_mesh_components_label over the core rows, every edge united by its higher row.
 *   -> within (n) int32: mvsn_cloud_nearest's `within` of the cloud against itself, bit for bit   core (n) bytes, 0 or 1
 *      result (2 int64): [0] the number of clusters C, 0 <= C <= n, [1] status bits (MVSN_CLUSTER_STATUS_*; 0 = fine).
 *      Reading the two words back (with the index build's status word) is the one host synchronisation.
 * mvsn_cloud_cluster_emit (rank, labels; labels alone with n_clusters = 0), on both workspaces and `core` handed on
 *   unchanged, n_clusters = C as read back (outside [0, n] it cannot be this workspace's: MVSN_E_BADARG):
 *   -> label (n) int64: the cluster id, -1 for noise   count, core_count, first (C) int64 (may be NULL with C = 0): the
 *      points of every cluster (border points included), its core points, and its lowest core row
 * Integer atomics only (a compare-and-swap on a root, relaxed loads and stores of parent, sums) and no float arithmetic
 * beyond d2: every output is a bitwise-reproducible function of the inputs, whatever order the index holds the points in.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_CLUSTER_STATUS_WORKSPACE 1   /* a walk over `parent` ran out of its bound or met a parent above its row: the
                                             workspace was overwritten during the call (cannot happen otherwise) */
size_t mvsn_cloud_cluster_workspace_bytes(long n);
int mvsn_cloud_cluster_label(const float *points, long n, float inv_cell, float r2, long min_points,
                             const void *index_workspace, size_t index_workspace_bytes, int *within, uint8_t *core,
                             int64_t *result, void *workspace, size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_cloud_cluster_emit(const float *points, long n, float inv_cell, float r2, const void *index_workspace,
                            size_t index_workspace_bytes, const uint8_t *core, void *workspace, size_t workspace_bytes,
                            long n_clusters, int64_t *label, int64_t *count, int64_t *core_count, int64_t *first,
                            mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A cloud rendered into posed cameras (z-buffered depth, the winning row, its colour and normal), and the occlusion test
 * of its points against depth maps (multi_view_stereonet_amd/fusion.py: cloud_render, cloud_visibility, cloud_colorize;
 * the semantics, every fp32 step and the arguments are DESIGN.md section 25).
 *   points (n,3) fp32, 1 <= n <= 2^31 - 1; K, T_cam_in_world (V,4,4), 1 <= V <= 65535; maps of rows x cols pixels, each
 *   at most 2^24 and rows * cols at most 2^31 - 1.  A size outside these limits, a radius outside
 *   0..MVSN_RENDER_MAX_RADIUS, a min_depth or rel_tol that is not a finite number >= 0 or a max_depth that is not > 0
 *   (+inf: no limit) is MVSN_E_BADARG; a workspace that is missing or too small MVSN_E_WORKSPACE; all before any launch.
 *   The camera is mvsn_tsdf_integrate's: P_v = K_v T_v^-1 (3x4; fp64, rounded once; K's bottom row taken to be (0,0,1));
 *   for a point p: z = P row 2 . (p,1); (u, v) = rows 0, 1 over z; c = floor(u + 0.5), r = floor(v + 0.5), every step
 *   one fp32 operation (three nested fused multiply-adds per row).  A point takes part in view v at radius R exactly
 *   when its coordinates and z are finite, min_depth < z <= max_depth, -R <= c < cols + R and -R <= r < rows + R (a NaN
 *   pixel fails; a pixel too large for an int fails, without overflow).
 * mvsn_cloud_render (clear, splat, resolve): per view and pixel the least key (uint64(bits of z) << 32) | row over the
 *   points that take part and whose flat, screen-aligned square |dx|, |dy| <= R around (r, c) holds the pixel: the
 *   nearest point, a tie on z to the lowest row; R = 0 is the exact point render.
 *   workspace: mvsn_cloud_render_workspace_bytes(V, rows, cols) = 8 V rows cols bytes (0 for sizes the entry refuses),
 *     16-byte aligned: one 64-bit key per pixel per view, (V,rows,cols); it may arrive uninitialised.
 *   -> depth (V,rows,cols) fp32: the winner's z, 0 where no point hit   index (V,rows,cols) int64: its row, -1 where none
 *      out_colors (V,3,rows,cols) u8 with colors (n,3) u8, or both NULL   out_normals (V,3,rows,cols) fp32 with normals
 *      (n,3) fp32, or both NULL: the winner's, zeros where none.  Every element of every output is written once.
 *   Integer atomics only (a 64-bit minimum, skipped where a load of the key shows it would change nothing: keys only
 *   decrease, so a stale load can cost an atomic and never drop one): every output is a bitwise-reproducible function of
 *   the inputs, whatever the order of the points and of the atomics.
 * mvsn_cloud_render_camera_batch: the number of cameras both entries stage at once (more views loop inside the launch).
 * mvsn_cloud_visibility (one launch, no workspace, no atomics): point i is visible in view v exactly when it takes part
 *   at R = 0 with max_depth = +inf (so its pixel is inside the map), D = depth[v,r,c] is finite and > 0, and
 *   z <= fma(rel_tol, D, D).  depth is any z-depth map: a render, the network's output, mvsn_tsdf_raycast's.
 *   -> visible (n,V) bytes, 0 or 1   count (n) int32: the views that see the point
 *      values (n,channels) fp32 with maps (V,channels,rows,cols) fp32, 1 <= channels <= 16, or both NULL and channels = 0:
 *      the sum of maps[v,:,r,c] over the visible views in view order (plain fp32 additions onto 0; a sample that is not
 *      finite is added like any other) divided once by (float)count; 0 where count = 0.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_RENDER_MAX_RADIUS 8
size_t mvsn_cloud_render_workspace_bytes(int n_views, int rows, int cols);
int mvsn_cloud_render_camera_batch(void);
int mvsn_cloud_render(const float *points, long n, const uint8_t *colors, const float *normals, const float *K,
                      const float *T_cam_in_world, int n_views, int rows, int cols, int radius, float min_depth,
                      float max_depth, void *workspace, size_t workspace_bytes, float *depth, int64_t *index,
                      uint8_t *out_colors, float *out_normals, mvsn_stream_t stream);
int mvsn_cloud_visibility(const float *points, long n, const float *depth, const float *maps, int channels,
                          const float *K, const float *T_cam_in_world, int n_views, int rows, int cols, float rel_tol,
                          float min_depth, uint8_t *visible, int *count, float *values, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Area-uniform samples of a triangle mesh's surface (multi_view_stereonet_amd/mesh.py: mesh_sample; the semantics and
 * every operation are DESIGN.md section 26).
 *   vertices (n_vertices,3) fp32   faces (n_faces,3) int64   1 <= n_vertices, n_faces, n <= 2^31 - 1
 *   A face with an index outside [0, n_vertices) or a vertex that is not finite takes no part (area 0; its indices are
 *   never used as addresses).  The area of a face is 0.5 sqrt(|(b - a) x (c - a)|^2) in fp64, every step one operation;
 *   with A_max the largest and e = ilogb(A_max), q_f = (uint64) floor(area_f 2^(31 - e)) < 2^32 and
 *   P[f] = q_0 + ... + q_f, an integer scan: a pure function of the mesh.  A face below 2^-31 of the largest has q = 0.
 *   workspace: mvsn_mesh_sample_workspace_bytes(n_faces) bytes (0 for sizes the entries refuse), 16-byte aligned: a head
 *     of 32 bytes, 8 bytes per face (the area, then q, then P, in place), 16 bytes per 256 faces.
 * mvsn_mesh_sample_prefix (the head cleared, area, quantise, the 64-bit scan, prefix, a 16-byte device copy):
 *   -> result (2 int64): [0] P[n_faces - 1], [1] status bits (MVSN_MESH_SAMPLE_STATUS_*; 0 = fine).  Reading the two
 *      words back is the one host synchronisation of a sampling; the workspace holds P.
 * mvsn_mesh_sample_draw (one launch), on the workspace handed on unchanged: sample i draws
 *   z_j = fin(seed + (3 i + j) 0x9E3779B97F4A7C15), j = 1, 2, 3, with splitmix64's finaliser as mvsn_cloud_ransac forms
 *   it; pick = umul64hi(z_1, P[n_faces - 1]); the face is the first f with P[f] > pick; u = (z_2 >> 11) 2^-53,
 *   v = (z_3 >> 11) 2^-53, and (1 - u, 1 - v) in their place where u + v > 1; the weights are ((1 - u) - v, u, v) and the
 *   point a + u (b - a) + v (c - a), in fp64, rounded to fp32 once.
 *   -> points (n,3) fp32   face (n) int64   weights (n,3) fp32
 *      out_normals (n,3) fp32 with normals (n_vertices,3) fp32, or both NULL: the weighted sum of the three vertex
 *      normals in fp64, normalised; (0,0,0) where its length is 0 or not finite
 *      out_colors (n,3) u8 with colors (n_vertices,3) u8, or both NULL: the weighted sum in fp64, floor(x + 0.5),
 *      clamped to [0, 255]
 *   With a total of 0 (the status says so) every face is -1 and everything else 0.
 * Integer atomics only (one 64-bit maximum), integer sums: every output is a bitwise-reproducible function of
 * (vertices, faces, n, seed), and sample i does not depend on n.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_MESH_SAMPLE_STATUS_NO_AREA 1   /* every face has weight 0: there is nothing to draw from */
size_t mvsn_mesh_sample_workspace_bytes(long n_faces);
int mvsn_mesh_sample_prefix(const float *vertices, long n_vertices, const int64_t *faces, long n_faces, int64_t *result,
                            void *workspace, size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_sample_draw(const float *vertices, long n_vertices, const int64_t *faces, long n_faces,
                          const void *workspace, size_t workspace_bytes, long n, uint64_t seed, const float *normals,
                          const uint8_t *colors, float *points, int64_t *face, float *weights, float *out_normals,
                          uint8_t *out_colors, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact point-to-triangle-mesh distance within a radius (multi_view_stereonet_amd/mesh.py: mesh_nearest; the semantics,
 * the distance operation by operation and the proof that the cells visited are enough are DESIGN.md section 26).  The
 * mesh counterpart of mvsn_cloud_nearest: the result is that of the brute force over every (query, face) pair.
 *   query (nq,3), vertices (n_vertices,3) fp32   faces (n_faces,3) int64   1 <= nq, n_vertices, n_faces <= 2^31 - 1
 *   inv_cell = 1 / max_dist and r2 = max_dist^2, each formed once in fp32 by the caller.
 *   A face with an index outside [0, n_vertices) or a vertex that is not finite takes no part (never dereferenced).  The
 *   closest point x of a face to q is formed in fp64 with + - x / and compares alone (the plane's barycentric weights
 *   where all three are >= 0, else the nearest of the three sides in the order (a,b), (b,c), (c,a), ties to the earlier:
 *   a collinear face degenerates to its sides, a face (v,v,v) to the point); x32 = fp32(x) clamped per axis to the
 *   face's box; d2 = (dx dx + dy dy) + dz dz in fp32 of q - x32, mvsn_cloud_nearest's operations; a face is within when
 *   d2 <= r2; the nearest is the least key (uint64(bits of d2) << 32) | row: ties to the lowest row.
 *   The index is mvsn_cloud_index_build's hash grid over (cell, face) pairs: a face goes into every cell of the box
 *   floor(min inv_cell) .. floor(max inv_cell) per axis; a face whose box holds more than
 *   MVSN_MESH_NEAREST_BOX_CELLS cells goes on the list of large faces that every query tests directly.
 * mvsn_mesh_nearest_count (one launch):
 *   -> result (3 int64): [0] the pairs, [1] the large faces, [2] status bits (MVSN_MESH_NEAREST_STATUS_*; 0 = fine).
 *      Reading the three words back is the one host synchronisation of a query: it sizes the workspace.
 *   workspace: mvsn_mesh_nearest_workspace_bytes(pairs, large) bytes (0 for counts above 2^31 - 1), 16-byte aligned: a
 *     head of 16 bytes, 20 bytes per slot of the table (a power of two >= 2 pairs, at least 1024), 4 bytes per pair and
 *     per large face, 12 bytes per 1024 slots.
 * mvsn_mesh_nearest_build (six launches), with the counts as read back.
 * mvsn_mesh_nearest (one launch, one thread per query), on the workspace handed on unchanged:
 *   -> dist2 (nq) fp32, +inf where no face is within   face (nq) int64, -1 where none   point (nq,3) fp32: x32 of the
 *      winner, 0 where none   weights (nq,3) fp32: its barycentric weights, 0 where none   within (nq) int32: the faces
 *      within, each counted once
 *   A query that is not finite gets (+inf, -1, 0, 0, 0); a query may lie anywhere.
 * mvsn_mesh_nearest_box_cells: MVSN_MESH_NEAREST_BOX_CELLS as the library was built with it.
 * Integer atomics only: every output is a bitwise-reproducible function of the inputs, whatever order the faces come in
 * (`face` follows the rows) and whatever order the atomics arrive in.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_MESH_NEAREST_BOX_CELLS 512
#define MVSN_MESH_NEAREST_STATUS_RANGE 1   /* a finite vertex's cell lies outside [-2^20, 2^20): max_dist too small */
int mvsn_mesh_nearest_box_cells(void);
size_t mvsn_mesh_nearest_workspace_bytes(long n_pairs, long n_large);
int mvsn_mesh_nearest_count(const float *vertices, long n_vertices, const int64_t *faces, long n_faces, float inv_cell,
                            int64_t *result, mvsn_stream_t stream);
int mvsn_mesh_nearest_build(const float *vertices, long n_vertices, const int64_t *faces, long n_faces, float inv_cell,
                            long n_pairs, long n_large, void *workspace, size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_nearest(const float *query, long nq, const float *vertices, long n_vertices, const int64_t *faces,
                      long n_faces, float inv_cell, float r2, long n_pairs, long n_large, const void *workspace,
                      size_t workspace_bytes, float *dist2, int64_t *face, float *point, float *weights, int *within,
                      mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A triangle mesh rendered into posed cameras: z-buffered depth, the winning face, its perspective-correct barycentric
 * weights, and the interpolated vertex normal and colour (multi_view_stereonet_amd/mesh.py: mesh_render; the semantics and
 * every operation are DESIGN.md section 27).
 *   vertices (n_vertices,3) fp32   faces (n_faces,3) int64   1 <= n_vertices, n_faces <= 2^31 - 1; K, T_cam_in_world
 *   (V,4,4), 1 <= V <= 65535; maps of rows x cols pixels, each 1..2^15.  A size outside these limits, a min_depth that is
 *   not a finite number >= 0 or a max_depth that is not > 0 (+inf: no limit) is MVSN_E_BADARG; a workspace that is missing
 *   or too small MVSN_E_WORKSPACE; all before any launch.
 *   A face is valid when its three rows lie in [0, n_vertices) and its nine coordinates are finite (otherwise its indices
 *   are never used as addresses).  Each vertex is projected by mvsn_cloud_render's steps on mvsn_tsdf_integrate's camera:
 *   zc = P row 2 . (p,1), (u, v) = rows 0, 1 over zc, every step one fp32 operation; pixel centres are the integers.  A
 *   valid face takes part in view v when every zc is finite and > min_depth and every |u|, |v| <= 2^16 (compared as
 *   floats: a NaN fails); one that does not, although a vertex has zc > min_depth, adds 1 to clipped[v]: there is no
 *   near-plane clipping.  X = rintf(256 u), Y = rintf(256 v) (8 sub-pixel bits, |X|, |Y| <= 2^24); coverage is decided on
 *   these integers alone: A = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0), A = 0 covers nothing, A < 0 swaps vertices 1 and 2 (both
 *   sides are rendered); for the centre (256 c, 256 r) and every directed edge p->q of the oriented face,
 *   E = (Xq-Xp)(256 r - Yp) - (Yq-Yp)(256 c - Xp); the pixel is covered when for all three E > 0, or E = 0 and (dy < 0, or
 *   dy = 0 and dx < 0): of two faces that share an edge exactly one owns a centre on it.  At a covered pixel, in fp64 and
 *   the face's own vertex order: lambda_k = E_k / A (E_k of the edge opposite vertex k), q_k = 1 / zc_k,
 *   S = (lambda_0 q_0 + lambda_1 q_1) + lambda_2 q_2, z = (float)(1 / S); the pixel takes the face when z is finite and
 *   min_depth < z <= max_depth.  Per view and pixel the least key (uint64(bits of z) << 32) | face row wins: the nearest
 *   face, a tie on z to the lowest row.
 * mvsn_mesh_render (clear, raster, resolve):
 *   workspace: mvsn_mesh_render_workspace_bytes(V, rows, cols) = 8 V (rows cols + 1) bytes (0 for sizes the entry refuses),
 *     16-byte aligned: one 64-bit key per pixel per view and one counter per view; it may arrive uninitialised.
 *   -> depth (V,rows,cols) fp32: the winner's z, 0 where no face hit   face (V,rows,cols) int64: its row, -1 where none
 *      weights (V,3,rows,cols) fp32: (float)((lambda_k q_k) / S), 0 where none
 *      out_normals (V,3,rows,cols) fp32 with normals (n_vertices,3) fp32, or both NULL, and out_colors (V,3,rows,cols) u8
 *      with colors (n_vertices,3) u8, or both NULL: mvsn_mesh_sample_draw's interpolation with the fp64 weights before
 *      their rounding; zeros where none   clipped (V) int64.  Every element of every output is written once.
 * mvsn_mesh_render_small_pixels: a face whose clipped box of pixels holds more than this many is rasterised by a whole
 *   wave instead of one thread (a tuning constant: no output depends on it).
 * Integer atomics only (the 64-bit minimum of mvsn_cloud_render with its skip, and a sum): every output is a
 * bitwise-reproducible function of the inputs, whatever the order of the atomics; depth does not depend on the order of
 * the faces.
 * ------------------------------------------------------------------------------------------- */
size_t mvsn_mesh_render_workspace_bytes(int n_views, int rows, int cols);
int mvsn_mesh_render_small_pixels(void);
int mvsn_mesh_render(const float *vertices, long n_vertices, const int64_t *faces, long n_faces, const float *normals,
                     const uint8_t *colors, const float *K, const float *T_cam_in_world, int n_views, int rows, int cols,
                     float min_depth, float max_depth, void *workspace, size_t workspace_bytes, float *depth,
                     int64_t *face, float *weights, float *out_normals, uint8_t *out_colors, int64_t *clipped,
                     mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Simplify a mesh by vertex clustering (multi_view_stereonet_amd/mesh.py: mesh_simplify; the semantics and every
 * operation are DESIGN.md section 28; csrc/mvsn_mesh_simplify.hip).  The vertices of one cell of the grid (voxel_size,
 * origin: mvsn_voxel_assign's cells, step for step) become one vertex; a face is remapped through the clustering and
 * dropped when a corner lies outside [0, n_vertices), is a dropped (non-finite) vertex, or two of its corners share a
 * cluster; of the faces whose remapped triples are equal up to rotation the one with the lowest row stays.
 *   vertices (n_vertices,3) fp32, faces (n_faces,3) int64, normals (n_vertices,3) fp32 or NULL, colors (n_vertices,3) u8
 *   or NULL; 1 <= n_vertices <= 2^31 - 1, 0 <= n_faces <= 2^31 - 1; voxel_size and inv_voxel_size as for the voxel merge
 *   workspace: mvsn_mesh_simplify_workspace_bytes(n_vertices, n_faces) bytes (0 for sizes the entries refuse), 16-byte
 *   aligned, handed from entry to entry unchanged: the voxel merge's workspace, 223 bytes per vertex for the clusters'
 *   sums and rows, 4 bytes per face and per slot of the face table (a power of two >= 2 n_faces slots).
 * mvsn_mesh_simplify_assign: mvsn_voxel_assign on the vertices.
 *   -> result (2 int64): [0] the number of clusters C, [1] status bits (MVSN_VOXEL_STATUS_*; 0 = fine).  The first host read.
 * mvsn_mesh_simplify_mark: clusters = C as read back (> 0).  The vertex side is mvsn_voxel_merge (and, with normals,
 *   mvsn_voxel_normals) into the workspace.  placement 0 = the mean; 1 = the quadric: per face the unit normal n in fp64,
 *   per corner u = (p - origin) / voxel_size - (cell + 0.5) and d = -n.u; n n^T, d n and 1 are quantised to 2^-30 and
 *   summed per cluster with 64-bit integer atomics; x solves (A + lambda k I) x = -b + lambda k u_mean, lambda = 2^-10,
 *   by the closed-form inverse, is clamped to |x| <= 0.5 - 2^-10 per axis, mapped back and rounded to fp32 once.  A
 *   position that voxel_cell does not put into the cluster's own cell is replaced by the first member's position.
 *   drop_unreferenced != 0: a cluster no surviving face uses is not output.
 *   -> result (4 int64): [0] output vertices M', [1] output faces F', [2] status bits (MVSN_MESH_SIMPLIFY_STATUS_*),
 *      [3] the clusters (output or not) whose position fell back to the first member's.  The second host read.
 * mvsn_mesh_simplify_emit: out_vertices_n = M', out_faces_n = F' as read back; normals and colours are written where
 *   the pointer is not NULL and mvsn_mesh_simplify_mark was given the input.
 *   -> out_vertices (M',3) fp32  out_faces (F',3) int64: output rows in the input face's corner order
 *      out_normals (M',3) fp32 or NULL  out_colors (M',3) u8 or NULL  count (M') int32  first (M') int64, ascending
 *      inverse (n_vertices) int64: output row of every input vertex, -1 = none  face_rows (F') int64, ascending
 * Integer atomics only (compare-and-swap on an empty slot, minima, sums): every output is a deterministic function of
 * the inputs, whatever the order of the faces' arrival.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_MESH_SIMPLIFY_STATUS_TABLE 1   /* a probe sequence of the face set visited every slot without finding room
                                               (cannot happen below 2^30 faces: the table is at most half full) */
size_t mvsn_mesh_simplify_workspace_bytes(long n_vertices, long n_faces);
int mvsn_mesh_simplify_assign(const float *vertices, long n_vertices, float voxel_size, float inv_voxel_size,
                              float origin_x, float origin_y, float origin_z, int64_t *result, void *workspace,
                              size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_simplify_mark(const float *vertices, const float *normals, const uint8_t *colors, long n_vertices,
                            const int64_t *faces, long n_faces, float voxel_size, float inv_voxel_size, float origin_x,
                            float origin_y, float origin_z, int placement, int drop_unreferenced, long clusters,
                            int64_t *result, void *workspace, size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_simplify_emit(const int64_t *faces, long n_vertices, long n_faces, long clusters, const void *workspace,
                            size_t workspace_bytes, long out_vertices_n, long out_faces_n, float *out_vertices,
                            int64_t *out_faces, float *out_normals, uint8_t *out_colors, int *count, int64_t *first,
                            int64_t *inverse, int64_t *face_rows, mvsn_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The unique edges of a mesh, smoothing over them, and normals (multi_view_stereonet_amd/mesh.py: mesh_edges,
 * mesh_smooth, mesh_normals; the semantics and every operation are DESIGN.md section 29; csrc/mvsn_mesh_edges.hip,
 * csrc/mvsn_mesh_smooth.hip).
 *
 * Edges.  Side s of face r = (v0, v1, v2) runs from v_s to v_(s+1)%3 and has the index 3 r + s.  A face with an index
 * outside [0, n_vertices) takes no part, nor does a side with equal ends.  An edge is the unordered pair of a side's ends.
 *   faces (n_faces,3) int64; 1 <= n_vertices <= 2^31 - 1, 1 <= n_faces <= (2^31 - 1) / 3 (a side index is an int32)
 *   workspace: mvsn_mesh_edges_workspace_bytes(n_vertices, n_faces) bytes (0 for sizes the entries refuse), 16-byte
 *   aligned, handed from mark to emit unchanged: 24 bytes per slot of the edge table (a power of two >= 6 n_faces
 *   slots, 1024 at least) and 12 bytes per face.
 * mvsn_mesh_edges_mark: every side into the set of packed keys (low << 32) | high; beside the slot the minimum side
 *   index, the count and the winding sum.
 *   -> result (2 int64): [0] the number of edges E, [1] status bits (MVSN_MESH_EDGES_STATUS_*).  The one host read.
 * mvsn_mesh_edges_emit: n_edges = E as read back.
 *   -> edges (E,2) int64 (low, high), in order of first  first (E) int64: the lowest side index that carries the edge
 *      face_count (E) int32: the sides that carry it  winding (E) int32: sides low -> high minus sides high -> low
 *      face_edge (n_faces,3) int64: the edge row of every side, -1 for a side that takes no part
 *      vertex_degree (n_vertices) int32: distinct edges at the vertex
 *      vertex_boundary (n_vertices) u8: 1 where the vertex lies on an edge with face_count 1, else 0
 *
 * mvsn_mesh_smooth: `iterations` steps x <- x + lam L(x) (method 0, laplacian) or pairs of steps with lam, then mu
 * (method 1, taubin), L the uniform Laplacian over `edges` (n_edges,2) int64, in fp64 working positions.  0 < lam <= 1,
 * -2 <= mu < 0, 0 <= iterations <= 10000.  pinned (n_vertices) u8 or NULL: non-zero = the vertex keeps its bits; a
 * vertex with a non-finite coordinate keeps its bits too and its edges contribute to neither end, as do edges with an
 * end outside [0, n_vertices) or with equal ends.  The degree of a vertex is the number of its contributing edges.
 * With span = the largest per-axis extent of the finite vertices = m 2^k, m in [0.5, 1): per edge (a, b) and axis
 * q = rint((x_b - x_a) 2^(30-k)) clamped to +-2^31 goes with 64-bit integer atomics into a's sum and, negated, b's;
 * per free vertex with a degree mean = ((double)sum 2^(k-30)) / (double)degree, x = x + f mean.  Without a finite
 * vertex, or with span 0, out_vertices is the input's bits.  No host read; the steps are launched back to back.
 *   workspace: mvsn_mesh_smooth_workspace_bytes(n_vertices) bytes, 16-byte aligned: 56 bytes per vertex.
 *   -> out_vertices (n_vertices,3) fp32: (float)x, rounded once
 *
 * mvsn_mesh_normals: per face c = (p1 - p0) x (p2 - p0) in fp64 with the lowest row rotated to the front,
 * face_normals = c / |c| and face_area = |c| / 2, zeros for a face with a corner outside [0, n_vertices), a non-finite
 * corner or no area.  Per vertex the direction of the sum of c over its valid faces, summed as integers: with the
 * vertex's largest |component of c| = m 2^e, every face adds rint(c 2^(31-e)); zeros where the sum is zero.
 *   workspace: mvsn_mesh_normals_workspace_bytes(n_vertices) bytes, 16-byte aligned: 32 bytes per vertex.
 *   -> face_normals (n_faces,3) fp32  face_area (n_faces) fp32  vertex_normals (n_vertices,3) fp32
 * Integer atomics only (compare-and-swap on an empty slot, minima, maxima, sums): every output is a deterministic
 * function of the inputs, whatever the order of arrival.
 * ------------------------------------------------------------------------------------------- */
#define MVSN_MESH_EDGES_STATUS_TABLE 1      /* a probe sequence of the edge set visited every slot without finding room
                                               (cannot happen: the table holds at least 3 n_faces slots) */
size_t mvsn_mesh_edges_workspace_bytes(long n_vertices, long n_faces);
int mvsn_mesh_edges_mark(const int64_t *faces, long n_vertices, long n_faces, int64_t *result, void *workspace,
                         size_t workspace_bytes, mvsn_stream_t stream);
int mvsn_mesh_edges_emit(long n_vertices, long n_faces, void *workspace, size_t workspace_bytes, long n_edges,
                         int64_t *edges, int64_t *first, int *face_count, int *winding, int64_t *face_edge,
                         int *vertex_degree, uint8_t *vertex_boundary, mvsn_stream_t stream);
size_t mvsn_mesh_smooth_workspace_bytes(long n_vertices);
int mvsn_mesh_smooth(const float *vertices, long n_vertices, const int64_t *edges, long n_edges, const uint8_t *pinned,
                     int method, long iterations, double lam, double mu, void *workspace, size_t workspace_bytes,
                     float *out_vertices, mvsn_stream_t stream);
size_t mvsn_mesh_normals_workspace_bytes(long n_vertices);
int mvsn_mesh_normals(const float *vertices, long n_vertices, const int64_t *faces, long n_faces, void *workspace,
                      size_t workspace_bytes, float *face_normals, float *face_area, float *vertex_normals,
                      mvsn_stream_t stream);

/* Tensor plumbing of the forward as library calls (so that a whole forward is a replayable list of C calls and nothing
 * else): a device-to-device copy on the stream (the torch.cat / repeat of poses, intrinsics and coarse source images,
 * multi_view_stereonet.py:553,:587-592) and dst[i] = src[i * stride] (the focal lengths K[:, 0, 0], :607). */
int mvsn_copy(void *dst, const void *src, size_t nbytes, mvsn_stream_t stream);
/* `count` independent device-to-device copies, eight per launch, every buffer a plain pointer argument of the kernel (the
 * input / output copies of a replayed forward plan: what torch._foreach_copy_ did with pointers the runtime cannot see) */
int mvsn_copy_many(void *const *dst, const void *const *src, const size_t *nbytes, int count, mvsn_stream_t stream);
/* fx[l * batch + b] = K_pyr[l][b][0][0] for every pyramid level in one launch (K_pyr: host array of `levels` <= 8 device
 * pointers to (batch, 4, 4) intrinsics) */
int mvsn_gather_focal(const float *const *K_pyr, int levels, int batch, float *fx, mvsn_stream_t stream);
int mvsn_gather_strided(const float *src, int count, long stride, float *dst, mvsn_stream_t stream);

/* Test hook for the banded chain (process-wide, 0 = off): bit 1 = the last band of every chain never runs (what a
 * shared device can do to a launch whose workgroups must be co-resident); bits 8.. = log2 of the spin limit of a
 * hand-off (default 2^21).  With it the other bands time out: the status word is set, the cost slice carries a NaN (so
 * the depth maps of that forward are NaN), nothing hangs.  Bit 2 (value 4) pins the 4-band plan on 16x32 (the 8-band
 * half-split plan is compared with it bit for bit); set it before asking for the workspace size. */
int mvsn_debug_set_band_flags(int flags);

/* Test hook: which tiles the dilated 3x3 Winograd layers walk.  0 (default) = row-phase items wherever they take no
 * more work items than the square tiles, 1 = row-phase items on every dilated 2-D layer, 2 = square tiles only.  The
 * outputs and GroupNorm statistics are the same bits either way.  Returns the previous value. */
int mvsn_debug_set_wino_rowphase(int mode);

/* Host only, no device call: the kernel form a Winograd layer (desc->precision = MVSN_CONV_FP32_WINO) runs on, as the
 * launch itself selects it -- `carrying` != 0: for a launch that carries a job (mvsn_conv_forward_carry).  out =
 * { k-steps per step, ring stages, carried units per wave and step, tile form (0 = 16 x 32 tiles, 1 = 10 x 40, 2 =
 * rolling strips, 3 = row-phase items), full-width input transform, bytes of LDS, work items per sample, steps per item }.
 * Returns 1, or 0 when no form of the 3x3 / 3x3x3 kernel runs the layer (the 5x5 stride-2 layer has a fixed plan of its
 * own) or, with `carrying`, when none carries. */
int mvsn_debug_wino_plan(const mvsn_conv_desc *desc, int carrying, int out[8]);

/* Host only, no device call: the kernel form a direct fp32 layer (desc->precision = MVSN_CONV_FP32) runs on, as
 * mvsn_conv_forward itself selects it for a call in `mode` (0 = plain input, 1 = LReLU(GN(in)) folded into the load,
 * 2 = + residual / staged output) with 16-byte aligned tensors and no statistics asked for where that matters (the
 * 3 -> 32 head).  out = { row of the table of forms, kind (0 = register-staged, 1 = LDS-DMA, 2 = the 5x5 stride-2
 * head), pixel tiles per wave (NPT), staged elements per thread and channel (SE; LDS-DMA: pieces per channel, IPC),
 * 16-byte staging (V4), cout tiles (CT), bytes of LDS, tiles per sample }.  Returns the number of rows in the table, or
 * 0 when no direct form runs the layer. */
int mvsn_debug_conv_plan(const mvsn_conv_desc *desc, int mode, int out[8]);

/* Device self-test of the MFMA fragment mapping the conv kernels rely on (A = 16x4, B = 4x16
 * fp32, asymmetric operands); returns 0 when the on-device result matches the scalar product. */
int mvsn_selftest_mfma(mvsn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVSN_HIP_H */
