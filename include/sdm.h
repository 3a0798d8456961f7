/*
 * sdm.h -- C-ABI of the MI355X-native cascaded-regression engine (libsdm_hip.so).
 *
 * The reference (patrikhuber/superviseddescent v0.4.1) is a header-only C++ template library with
 * no FFI of its own; its hot path is reached through duck-typed template concepts
 * (include/superviseddescent/superviseddescent.hpp:85-86,165-166,262-263,323-324).  This header is
 * the boundary a maintainer binds those concepts to: every entry point below names the reference
 * code it stands in for.  Plain C, opaque handle, caller-owned host buffers, library-owned device
 * buffers, one HIP stream per handle, a handle is not thread-safe.
 *
 * Conventions
 *   - all matrices are row-major float32 (CV_32FC1 in the reference), images are single-channel u8
 *   - a parameter row is [x_0..x_{L-1}, y_0..y_{L-1}]          (include/rcr/helpers.hpp:45-55)
 *   - a feature row has F = L*C*C*D + 1 floats, the last one the bias 1.0f
 *                                                              (include/rcr/adaptive_vlhog.hpp:176-183)
 *   - return value: 0 = ok, negative = error (text from sdm_last_error()); nothing throws
 *   - there is NO CPU fallback: without a HIP device every compute entry point returns SDM_ERR_NO_DEVICE
 */
#ifndef SDM_H_
#define SDM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDM_OK 0
#define SDM_ERR_INVALID (-1)       /* bad argument / call order                                      */
#define SDM_ERR_NO_DEVICE (-2)     /* no HIP device, or the device is not gfx950                       */
#define SDM_ERR_HIP (-3)           /* a HIP runtime call failed                                        */
#define SDM_ERR_EMPTY_PATCH (-4)   /* patch_width_half <= 0: cv::resize would throw in the reference   */
#define SDM_ERR_NOT_SPD (-5)       /* regularised Gram matrix not positive definite                    */
#define SDM_ERR_COMM (-6)          /* the installed all-reduce callback failed                         */

#define SDM_VARIANT_DALALTRIGGS 0  /* VlHogVariantDalalTriggs, include/rcr/hog.h:72 */
#define SDM_VARIANT_UOCTTI 1       /* VlHogVariantUoctti */

#define SDM_REG_MANUAL 0           /* Regulariser::RegularisationType::Manual,     regressors.hpp:96 */
#define SDM_REG_MATRIX_NORM 1      /* Regulariser::RegularisationType::MatrixNorm, regressors.hpp:97 */

/* rcr::HoGParam, include/rcr/adaptive_vlhog.hpp:41-60 (same field order as its cereal serialisation).
 * relative_patch_size > 0: the IED-adaptive rcr::HogTransform (adaptive_vlhog.hpp:109-185), feature row = L patches + bias.
 * relative_patch_size == 0: the non-adaptive HogTransform of examples/landmark_detection.cpp:158-269 -- patch_width_half =
 *   num_cells * (cell_size / 2) pixels, ROI not resized (cell_size must be even), NO bias column; the eye index lists
 *   may then be empty (NoNormalisation, superviseddescent.hpp:60-74). */
typedef struct sdm_hog_param {
    int variant;
    int num_cells;
    int cell_size;
    int num_bins;
    float relative_patch_size;
} sdm_hog_param;

typedef struct sdm_ctx sdm_ctx;

/* Timing slots filled when sdm_enable_timing(ctx, 1): accumulated milliseconds and launch counts,
 * measured with HIP events on the handle's stream.  The solver slots mirror the four stages
 * VerbosePartialPivLUSolver prints (include/superviseddescent/verbose_solver.hpp:66-97). */
enum {
    SDM_T_HOG = 0,      /* feature extraction: hog_packed_kernel (hog_fast_kernel / hog_batch_kernel for the shapes it does not serve)   */
    SDM_T_APPLY = 1,    /* detect: desc_kernel<FUSED> + apply_reduce_kernel; otherwise apply_tiled_f16_kernel (apply_tiled_kernel) + apply_reduce_kernel */
    SDM_T_GRAM = 2,     /* "A^T * A" and A^T * b: split_planes_f16_kernel + syrk_tn_split_w4_kernel                                     */
    SDM_T_REG = 3,      /* "AtA + Reg"                                                                                                    */
    SDM_T_FACTOR = 4,   /* "Decomposition" + both substitutions (blocked Cholesky; or the column-pivoted QR)                              */
    SDM_T_BACKSOLVE = 5,/* "solve()" -- 0 since the back substitution runs inside the factorisation's launch sequence                     */
    SDM_T_ALLREDUCE = 6,
    SDM_T_COUNT = 8
};

const char* sdm_last_error(void);
int sdm_device_count(void);                       /* number of usable HIP devices (0 on a CPU box) */

/* Lifetime.  sdm_create fails (NULL) without a gfx950 device. */
sdm_ctx* sdm_create(int device);
void sdm_destroy(sdm_ctx* ctx);
/* Run on a caller-provided hipStream_t (e.g. PyTorch's current stream) instead of the handle's own. */
int sdm_set_stream(sdm_ctx* ctx, void* hip_stream);
int sdm_synchronize(sdm_ctx* ctx);

/* Model geometry: what rcr::HogTransform's constructor (adaptive_vlhog.hpp:92) and
 * InterEyeDistanceNormalisation (include/rcr/model.hpp:90) receive, with the string-keyed landmark
 * ids resolved to 0-based positions.  n_right == 0 && n_left == 0 selects NoNormalisation
 * (superviseddescent.hpp:60-74) -- only valid for paths that never extract HOG features. */
int sdm_set_model_geometry(sdm_ctx* ctx, int num_landmarks, const int* right_eye_idx, int n_right,
                           const int* left_eye_idx, int n_left, int n_levels, const sdm_hog_param* levels);
int sdm_feature_dim(const sdm_ctx* ctx, int level);          /* F of that level, or negative */

/* HOG accumulation mode.  All modes take identical integer decisions (ROI geometry, resized bytes,
 * orientation bins) as the reference; they differ only in how the f32 contributions of one histogram cell
 * are summed:
 *   SDM_HOG_EXACT_ORDER  in the reference's raster order (hog.c:616-617,713-724) -> features bit-identical
 *                        to the reference's CPU path; slow (LDS float atomics retire one lane per 3 cycles)
 *   SDM_HOG_FAST         exact fixed-point sum of the reference's f32 products, rounded to f32 once -> order
 *                        independent, deterministic, within a few ulp of the reference's sequentially rounded sum
 *   SDM_HOG_COLUMNS      (default) separable sum: every pixel column accumulates g*wy in f32 in row order, the
 *                        columns are folded into cells with the wx weights on the matrix cores -> deterministic,
 *                        same error size as FAST (a few ulp of the histogram entries), about 1.2x faster.
 *                        Its lane-packed launch (4 orientations x 5x5 cells, see sdm_debug_set_hog_packing) also takes the
 *                        gradient magnitude from the hardware square root (correctly rounded or one ulp low) and runs the
 *                        block normalisation of hog.c:930-1052 in f32 instead of double: measured against the CPU path
 *                        the features differ by <= 2e-7 absolute (relative L2 8e-8), integer decisions are identical.
 *                        Geometries without a specialised kernel instance run FAST instead.
 * Callers that need the reference's bits select EXACT_ORDER; FAST keeps every double step of the reference. */
#define SDM_HOG_EXACT_ORDER 0
#define SDM_HOG_FAST 1
#define SDM_HOG_COLUMNS 2
int sdm_set_hog_mode(sdm_ctx* ctx, int mode);
/* Which kernel a level runs: *fast_kernel = 1 when the fused S<=64 kernel is used; *fast_bins = the orientation
 * binning method that passed the exhaustive on-device check (511x511 gradients) for that level: 2 = sector count,
 * 1 = un-normalised arg-max, 0 = the reference's normalise-and-score arithmetic. */
int sdm_get_hog_info(sdm_ctx* ctx, int level, int* fast_kernel, int* fast_bins);

/* Images: the `const std::vector<cv::Mat>& images` of HogTransform (adaptive_vlhog.hpp:92,188),
 * single channel u8.  Host images are copied to HBM once.
 *
 * Frame geometry, the same for every image entry point below (tests/test_gpu_frame_geometry.py pins each line):
 *   width, height        any positive int (run: 70 000 columns, 65 600 rows).  stride_bytes: any int >= the row's bytes.
 *   fused pixel kernels  serve a set whose every image has width >= 2, height <= 65 535, stride_bytes <= 2^20 and
 *                        height * stride_bytes <= INT_MAX (run: stride 2^20 under 2 047 rows, a byte offset inside the image of
 *                        2 146 435 135).  One image beyond any of the four sends the WHOLE set to the generic HOG kernel: same
 *                        integer decisions, features within the same tolerance, slower (run: strides 26 843 545 and 26 843 547
 *                        under 80 rows, with faces 175 rows above and below the image).
 *                        A patch may lie partly or wholly outside its image: it reads black there.  With the fused kernels this
 *                        holds while (rows it reaches above or below the image) * stride_bytes < 2^31 -- 2 048 rows at the
 *                        largest stride (run: 2 000 rows), 131 072 rows at a stride of 16 384; a patch further out is not supported.
 *   distance of frames   images of one set may lie anywhere in the device's address space, in any order (run: 2^32 + 2^28 bytes
 *                        apart, the first frame the highest); sdm_set_images_device's image i lies i * height * stride_bytes
 *                        behind the base, in 64 bits (run: above 2^31).
 *   crops, tracker       read the same table with 64-bit offsets; sdm_align_crops_tensor uses 32-bit offsets inside a plane of at
 *                        most INT_MAX bytes (NV12: both planes) and 64-bit ones beyond. */
int sdm_upload_images_u8(sdm_ctx* ctx, const uint8_t* const* images, const int* width, const int* height,
                         const int* stride_bytes, int n_images);
/* The same for 3-channel images in cv::imread's BGR byte order (stride_bytes >= 3 * width): converted to gray ONCE per image
 * on the device, gray = (B*1868 + G*9617 + R*4899 + 8192) >> 14 -- cv::cvtColor(COLOR_BGR2GRAY) of OpenCV 2.4 ... 3.x, which
 * the reference applies to the whole image at every level for every sample (adaptive_vlhog.hpp:114-120).  gray_shift = 15
 * selects the 15-bit weights (3735, 19235, 9798) of later OpenCV releases.  (OpenCV is not in the reference tree: parity
 * unpinned for this step, like cv::resize.) */
int sdm_upload_images_bgr_u8(sdm_ctx* ctx, const uint8_t* const* images, const int* width, const int* height,
                             const int* stride_bytes, int n_images, int gray_shift);
/* Device-resident stack of equally sized images (image i at base + i*height*stride_bytes, a 64-bit product); not copied. */
int sdm_set_images_device(sdm_ctx* ctx, const uint8_t* dev_base, int n_images, int width, int height,
                          int stride_bytes);
/* Frames that are ALREADY on the device -- a hardware decoder's output, torch tensors, regions of a larger frame -- as the image
 * set, each with its own size, pitch, pointer (any alignment) and format.  The call replaces the context's image set: image i is
 * frame i for sdm_set_sample_image_index, sdm_hog_features, sdm_detect_batch, sdm_track_step, sdm_pose_templates_from_landmarks
 * and sdm_align_crops' default source.
 *   one-byte formats (GRAY, NV12)  used IN PLACE: the call neither copies nor reads them, it writes the image table only.  The memory
 *       must stay valid until the image set is replaced (the contract of sdm_set_images_device).  NV12:
 *       data = the Y plane, height rows of stride_bytes; Y is taken as it is (no range expansion), the chroma plane behind it is
 *       never read.
 *   colour formats  converted to gray images the CONTEXT owns, all colour frames of the call in ONE launch on the handle's stream,
 *       with sdm_upload_images_bgr_u8's arithmetic (gray_shift 14 | 15 selects its two weight sets; RGB / RGBA swap the weights
 *       of byte 0 and byte 2; alpha is ignored).  The source is only read and may be released after the call.
 *   mixed sets are allowed: in-place and owned images share the one image table (its base is the lowest address of the set).
 * Argument errors (SDM_ERR_INVALID) change no state and launch nothing -- the previous image set stays the one in use: NULL,
 * n_frames < 1, width or height < 1, stride_bytes < width * bytes per pixel, an unknown format, gray_shift not 14 or 15, and
 * colour frames of 2^31 or more 16-pixel row chunks in one call.  (The frame geometry rule above holds: an image less than 2
 * pixels wide, 65 536+ rows high, of a stride above 2^20 or of more than INT_MAX bytes of height * stride_bytes selects the
 * generic HOG kernel.) */
#define SDM_FRAME_GRAY 0   /* 1 byte per pixel, used in place                                  */
#define SDM_FRAME_BGR  1   /* 3 bytes, cv::imread order                                        */
#define SDM_FRAME_RGB  2
#define SDM_FRAME_BGRA 3   /* 4 bytes, alpha ignored                                           */
#define SDM_FRAME_RGBA 4
#define SDM_FRAME_NV12 5   /* data = the Y plane (height rows of stride_bytes), used in place;
                              the chroma plane behind it is never read; Y is taken as it is    */
#define SDM_FRAME_BGR_PLANAR 16   /* three planes of 1 byte per pixel, B G R: "Planar colour frames" below */
#define SDM_FRAME_RGB_PLANAR 17   /* three planes, R G B                                                    */
#define SDM_FRAME_P010 7   /* as NV12, 16-bit little-endian words, the sample in bits 15..6:
                              "YUV colour description and 10-bit surfaces" below (6 stays
                              free: it has always been refused as an unknown format)           */
#define SDM_FRAME_BASE(f)       ((f) & 0xff)
#define SDM_FRAME_YUV_BT601     0x000    /* matrix, bits 8..11  */
#define SDM_FRAME_YUV_BT709     0x100
#define SDM_FRAME_YUV_BT2020    0x200    /* non-constant luminance */
#define SDM_FRAME_YUV_FULL      0x1000   /* range, bit 12; absent: limited */
typedef struct sdm_frame { const void* data; int width, height, stride_bytes, format; } sdm_frame;
/* YUV colour description and 10-bit surfaces.  The colour description of a YUV frame rides in sdm_frame.format: the base
 * (SDM_FRAME_BASE(format): SDM_FRAME_NV12 or SDM_FRAME_P010) or-ed with one matrix and, for full range, SDM_FRAME_YUV_FULL --
 * SDM_FRAME_NV12 | SDM_FRAME_YUV_BT709 is what a 1080p or 4K decoder delivers, SDM_FRAME_P010 | SDM_FRAME_YUV_BT2020 an HDR stream,
 * SDM_FRAME_NV12 | SDM_FRAME_YUV_FULL a camera or JPEG-derived frame.  Every call that takes an sdm_frame takes these values.
 *   value 5   SDM_FRAME_NV12 with no flag is UNCHANGED on every path: BT.601 limited range with OpenCV's three-decimal constants (the
 *       formulas at sdm_align_crops_tensor and "Pasting crops back into NV12 frames"), bit for bit.  SDM_FRAME_NV12 |
 *       SDM_FRAME_YUV_BT601 IS value 5: an 8-bit BT.601 limited-range frame cannot ask for the derived constants (they differ from
 *       OpenCV's in the fourth digit).  Every other (matrix, range, depth) uses constants derived by the one rule below.
 *   constants   Kr, Kb = (0.299, 0.114) BT.601, (0.2126, 0.0722) BT.709, (0.2627, 0.0593) BT.2020; Kg = 1 - Kr - Kb.  Each integer
 *       constant is floor(c * 2^20 + 0.5) of its real coefficient c, evaluated in double.
 *   decode    d bits (8: NV12, 10: P010).  Limited: ys = 255 / (219 * 2^(d-8)), cs = 255 / (224 * 2^(d-8)), y0 = 16 * 2^(d-8); full:
 *       ys = cs = 255 / (2^d - 1), y0 = 0.  y = max(Y - y0, 0) * CY, u = U - 2^(d-1), v = V - 2^(d-1);
 *       R = clamp255((y + CVR v + 2^19) >> 20), B = clamp255((y + CUB u + 2^19) >> 20), G = clamp255((y - CVG v - CUG u + 2^19) >> 20)
 *       with CY = ys, CVR = 2 (1 - Kr) cs, CUB = 2 (1 - Kb) cs, CVG = 2 Kr (1 - Kr) / Kg cs, CUG = 2 Kb (1 - Kb) / Kg cs, in int32 (every
 *       sum is below 2^31).  BT.709 limited: 1220945 1879825 2215014 558796 223607 at 8 bits, 305236 469956 553753 139699 55902 at 10.
 *   encode    (the pastes, 8 bits)  Y = (YR R + YG G + YB B + (y0 << 20) + 2^19) >> 20 with the coefficients K * (219 / 255 | 1);
 *       U = clamp255((UB B - UG G - UR R + (128 << 20) + 2^19) >> 20) with 0.5, 0.5 Kg / (1 - Kb), 0.5 Kr / (1 - Kb), each times
 *       (224 / 255 | 1); V the same with R in B's place and Kr in Kb's.  BT.709 full: Y 222927 749942 75707, U 524288 404150 120138,
 *       V 524288 476214 48074.
 *   P010      data = the Y plane, height rows of stride_bytes, one 16-bit little-endian word per pixel; the UV plane, (height + 1) / 2
 *       rows of (width + 1) / 2 word pairs, lies behind it or where the second-plane array says.  A tap is word >> 6 (0 ... 1023, the low
 *       six bits are ignored); the bilinear value is (sum of w s + 512) >> 10 at 10 bits for luma and for the UV pair, a luma tap outside
 *       the plane reads 0, a chroma tap 512; the area sums add 10-bit taps.  The 10-bit decode gives the 8-bit (B, G, R); gray weights,
 *       scale and bias, layouts and chroma siting (position / 2) are those of NV12.
 *   gray      channels == 1 from NV12 with any flags is Y as it is; from P010 it is min(255, (Y10 + 2) >> 2) of the bilinear (or averaged)
 *       10-bit luma.  As an image set, NV12 with any flags is read in place; a P010 frame is converted by the colour launch into a
 *       context-owned gray image, min(255, ((word >> 6) + 2) >> 2) per luma word -- its UV plane is never read.
 *   where     sources of sdm_align_crops_tensor[_filtered] and sdm_warp_crops_tensor[_filtered]: NV12 and P010 with flags.  Destinations
 *       of the _nv12 pastes: NV12 with flags.  A P010 destination is refused; so is P010 in sdm_align_crops, as NV12 is.
 *   refused   (SDM_ERR_INVALID, no state changed, nothing launched) a flag on a base that is not NV12 or P010, a matrix field above
 *       0x200, any other set bit; a P010 frame with stride_bytes < 2 * width, a UV row shorter than 4 * ((width + 1) / 2) bytes, or an
 *       odd pointer or stride of either plane.  Offsets inside a plane are 32-bit while height * stride_bytes <= INT_MAX bytes (and
 *       the same for the UV plane), 64-bit beyond. */
int sdm_set_frames_device(sdm_ctx* ctx, const sdm_frame* frames, int n_frames, int gray_shift);
/* Planar colour frames -- 3 x H x W uint8, the layout of torch's decoders, colour transforms and image networks -- as a source and
 * as a destination of every call that takes an sdm_frame.  Nothing is repacked: the image set, the crops, the warps and the pastes
 * address the three planes where they lie.
 *   planes    data is plane 0: height rows of stride_bytes, one byte per pixel, stride_bytes >= width.  Plane c (c = 0, 1, 2) is at
 *       (const uint8_t*)data + c * D with D, the plane distance, a signed 64-bit number of bytes.  The order of the planes is
 *       B, G, R for SDM_FRAME_BGR_PLANAR and R, G, B for SDM_FRAME_RGB_PLANAR.
 *   D         (int64_t)height * stride_bytes by default -- a contiguous 3 x H x W block, the rule NV12 has for its UV plane.  An entry
 *       point with a `chroma` / `dst_chroma` / `planes` array takes the address of plane 1, the SECOND PLANE, as entry i of it: D is
 *       that address minus data, of any sign (a reversed channel view has a negative D); a NULL entry, or a NULL array, is the default.
 *       D == 0 is refused.  So a region x[:, 100:580, 200:840], a frame of an N x 3 x H x W batch and a channel-sliced buffer are all
 *       frames as they are.  Entry points without such an array -- sdm_set_frames_device, sdm_align_paste_tensor[_at][_filtered],
 *       sdm_warp_paste_tensor[_at] -- take planar frames with the default D; the _nv12 forms of the pastes (filter == NULL allowed, any
 *       mix of formats) are the general forms for planar destinations.
 *   values    a planar pixel is the interleaved pixel of the same three bytes: the image set's gray bytes, the crop and warp tensors
 *       (channels == 1: the gray weights applied to the warped (B, G, R)) and the pasted bytes are bit-identical to those of the
 *       SDM_FRAME_BGR / SDM_FRAME_RGB frame that holds the same pixels.  Inside a plane the offsets are those of a one-byte format
 *       (32-bit while height * stride_bytes <= INT_MAX); D is applied to the pointer in 64 bits first.
 *   pastes    one byte of each plane is loaded, blended and stored per owned pixel; the ownership rule, the row order and "never stored
 *       to" hold word for word -- the bytes between the planes and the pitch padding are neither read nor written.  Reading planes
 *       that overlap is harmless; pasting into them is undefined, as pasting into aliasing frames is.
 *   refused   (SDM_ERR_INVALID, no state changed, nothing launched) what is refused of a one-byte-per-pixel frame; D == 0; and
 *       sdm_align_crops, the interleaved u8 form, on a frame list that holds a planar frame (as for NV12: use sdm_align_crops_tensor).
 * sdm_set_frames_device_planes is sdm_set_frames_device with the second planes: planes is NULL or n_frames pointers, entries of frames
 * that are not planar are ignored. */
int sdm_set_frames_device_planes(sdm_ctx* ctx, const sdm_frame* frames, const void* const* planes, int n_frames, int gray_shift);
/* `training_index` of HogTransform::operator() (adaptive_vlhog.hpp:109): sample -> image.
 * idx == NULL means sample i uses image i. */
int sdm_set_sample_image_index(sdm_ctx* ctx, const int* idx, int n_samples);

/* current_x of the cascade loops (superviseddescent.hpp:169, 266, 327): N x 2L */
int sdm_set_x(sdm_ctx* ctx, const float* x_host, int n_samples);
int sdm_get_x(sdm_ctx* ctx, float* x_host);
int sdm_set_x_device(sdm_ctx* ctx, const float* x_dev, int n_samples);  /* device-to-device copy */
int sdm_get_x_device(sdm_ctx* ctx, float* x_dev);

/* One cascade level of feature extraction for all N samples: the thread-pool loop
 * superviseddescent.hpp:173-189 / 269-285 over rcr::HogTransform::operator() (adaptive_vlhog.hpp:109-185).
 * feat_host may be NULL (features stay in HBM for sdm_apply / sdm_gram_rhs). */
int sdm_hog_features(sdm_ctx* ctx, int level, float* feat_host /* N x F or NULL */);
/* Integer decisions of the last sdm_hog_features call: N x (1+2L) ints
 * [patch_width_half, cvRound(x_i).., cvRound(y_i)..]   (adaptive_vlhog.hpp:123,132-133). */
int sdm_get_patch_indices(sdm_ctx* ctx, int* idx_host);

/* LinearRegressor::x of one level (regressors.hpp:383), F x M row-major. */
int sdm_set_regressor(sdm_ctx* ctx, int level, const float* R_host);
int sdm_get_regressor(sdm_ctx* ctx, int level, float* R_host);
/* x <- x - (feat * R_level) .* IED(x): LinearRegressor::predict per row + update
 * (regressors.hpp:377-381, superviseddescent.hpp:209-215 / 294-301 / 337-339). */
int sdm_apply(sdm_ctx* ctx, int level);
/* All levels: SupervisedDescentOptimiser::test (superviseddescent.hpp:262-306) with an empty
 * template, = rcr::detection_model::detect (model.hpp:132-157) for a batch.  x_host may be NULL. */
int sdm_detect_batch(sdm_ctx* ctx, float* x_host);
/* One cascade level of sdm_detect_batch on the current x (the loop body of SupervisedDescentOptimiser::test,
 * superviseddescent.hpp:269-301: projection -> predict -> update): x_{k+1} replaces x_k on the device.  Same launches as
 * sdm_detect_batch, so a level-by-level run (callbacks between the levels, superviseddescent.hpp:303) gives the same bits. */
int sdm_detect_level(sdm_ctx* ctx, int level);

/* Known-template mode (superviseddescent.hpp:195-197, 287-289): when `templates` (n_samples x
 * feature_dim, row n = the known y of sample n) is set, every sdm_hog_features call stores features - templates, which
 * is what sdm_gram_rhs / sdm_apply / sdm_detect_batch then see.  NULL clears it (the RCR case: templates.empty()). */
int sdm_set_templates(sdm_ctx* ctx, const float* templates, int n_samples, int feature_dim);

/* The step before the path: x_n = rcr::align_mean(mean, box_n) (include/rcr/model.hpp:64-76), or
 * align_mean(mean, perturb(box_n, t_n)) (apps/rcr/rcr-train.cpp:130-146, 421-431) when `perturbations` is given,
 * evaluated on the device straight into the state x (replaces sdm_set_x).  mean: 2L floats in the unit box;
 * boxes: N x {x, y, width, height} ints (cv::Rect); perturbations: NULL or N x {translation_x, translation_y, scaling}
 * (the caller draws them: the reference uses N(0, 0.04), N(0, 0.04), N(1, 0.04) from an unseeded std::mt19937).
 * x_host may be NULL. */
int sdm_init_from_boxes(sdm_ctx* ctx, const float* mean, const int* boxes, const float* perturbations, int n_samples,
                        float* x_host);
/* The evaluation after a level: calculate_normalised_landmark_errors (apps/rcr/rcr-train.cpp:200-212) of the
 * current x against the targets of sdm_set_targets: errors[n][i] = ||x_i - x*_i||_2 / IED(x_n); *mean_out = cv::mean
 * of that matrix (what rcr-train prints per cascade level, :457-459).  errors_host (N x L) may be NULL. */
int sdm_normalised_errors(sdm_ctx* ctx, float* errors_host, double* mean_out);

/* Training, one level (superviseddescent.hpp:170-218 with templates.empty()):
 *   sdm_hog_features -> sdm_gram_rhs -> [sdm_allreduce_gram_rhs] -> sdm_solve -> sdm_apply */
int sdm_set_targets(sdm_ctx* ctx, const float* xstar_host, int n_samples);   /* `parameters`, :165 */
/* b = (x - x*) .* norm(x) (:199-205);  G = A^T A, B = A^T b  (regressors.hpp:208,225) */
int sdm_gram_rhs(sdm_ctx* ctx, int level);
/* Sum {G, B} over data-parallel ranks through the installed callback (no-op when none is installed). */
typedef int (*sdm_allreduce_fn)(void* dev_ptr, size_t count_f32, void* hip_stream, void* user);
int sdm_set_allreduce(sdm_ctx* ctx, sdm_allreduce_fn fn, void* user, int world_size);
/* The same exchange through RCCL, called by the library itself: ncclAllReduce(sum, float32, in place) on the handle's stream,
 * so the collective is ordered behind the Gram kernels and before the solve without host synchronisation.  nccl_comm is the
 * caller's ncclComm_t (one rank per process / GPU); nccl_allreduce_fn is the address of ncclAllReduce in the RCCL the caller
 * links (recommended: exactly one RCCL per process), or NULL to let the library find the symbol in the process / load librccl.
 * NULL comm uninstalls.  The reference has no collective (superviseddescent.hpp:170-218 is single-process). */
int sdm_set_allreduce_rccl(sdm_ctx* ctx, void* nccl_comm, void* nccl_allreduce_fn, int world_size);
int sdm_allreduce_gram_rhs(sdm_ctx* ctx);
/* Sharded factorisation of the (already summed and identical) system inside sdm_solve.  The reference solves on one core
 * (regressors.hpp:224-225); replicated on every rank the solve is the serial fraction of data-parallel training.  With sharding
 * installed rank r performs the tile operations of the 128-column tile columns j with j % world_size == r: per 128-column step
 * the owner of the step's column broadcasts <= 4 tiles (its factored diagonal tile + the column's tiles of the open group of 4
 * panel rows), per group of 4 steps the ranks all-gather the group's panel rows; the back substitution stays replicated.
 * The regressor is bit-identical to the replicated solve's for any world_size.  Collectives run on `hip_stream` (the
 * handle's stream) and must be stream-ordered like ncclBroadcast / ncclAllGather; they return 0 on success.
 *   bcast:     `count_f32` floats at dev_ptr, from rank `root` to all
 *   allgather: every rank contributes `count_f32` floats at send_ptr; recv_ptr receives world_size * count_f32, rank-major
 * Passing NULL for both callbacks (or a NULL communicator) restores the replicated solve. */
typedef int (*sdm_bcast_fn)(void* dev_ptr, size_t count_f32, int root, void* hip_stream, void* user);
typedef int (*sdm_allgather_fn)(const void* send_ptr, void* recv_ptr, size_t count_f32, void* hip_stream, void* user);
int sdm_set_solve_sharding(sdm_ctx* ctx, int rank, int world_size, sdm_bcast_fn bcast, sdm_allgather_fn allgather, void* user);
/* The same through RCCL, called by the library itself on the handle's stream; the function addresses may be NULL (looked up as
 * ncclBroadcast / ncclAllGather in the process, then in librccl.so). */
int sdm_set_solve_sharding_rccl(sdm_ctx* ctx, void* nccl_comm, int rank, int world_size, void* nccl_broadcast_fn,
                                void* nccl_allgather_fn);
/* Reduce-scatter form of the exchange (the reference trains in one process: regressors.hpp:208,225 form A^T A / A^T b once; here
 * every rank forms them of ITS rows).  With the factorisation sharded over the same ranks (above) rank r only ever reads the tile
 * columns it owns, so sdm_allreduce_gram_rhs then ships every rank the SUM of its own columns -- tiles grouped by owner, one
 * reduce-scatter of world_size equal chunks: half the ring traffic of the all-reduce -- followed by one all-reduce of F + 1 floats
 * (the summed diagonal and the ranks' shares of ||G||_F^2) through the callback / communicator registered with sdm_set_allreduce*.
 *   reduce_scatter: every rank contributes world_size * count_f32 floats at send_ptr (chunk r destined for rank r); recv_ptr
 *                   receives the element-wise sum over the ranks of this rank's chunk (count_f32 floats); stream-ordered
 * Without it, or with a replicated solve, the exchange stays the all-reduce.  NULL / enable = 0 removes it.
 * From 128 tile columns on (RCR-68) the callback is invoked once per RANGE of tile columns (four ranges), on the handle's second queue,
 * while sdm_gram_rhs' kernel is still multiplying the ranges behind it (round 4: the exchange runs behind the Gram kernel); the sums are
 * those of the one-piece exchange, bit for bit.  sdm_debug_set_option(ctx, "gram_xblocks", 1) keeps the single call. */
typedef int (*sdm_reduce_scatter_fn)(const void* send_ptr, void* recv_ptr, size_t count_f32, void* hip_stream, void* user);
int sdm_set_reduce_scatter(sdm_ctx* ctx, sdm_reduce_scatter_fn fn, void* user);
/* The same through RCCL on the communicator given to sdm_set_allreduce_rccl; the address may be NULL (looked up as ncclReduceScatter). */
int sdm_set_reduce_scatter_rccl(sdm_ctx* ctx, int enable, void* nccl_reduce_scatter_fn);
/* Regulariser::get_matrix (regressors.hpp:126-148) with n_train = the GLOBAL sample count, add to the
 * diagonal (regressors.hpp:215-221), factor and solve (regressors.hpp:224-225; Cholesky instead of
 * PartialPivLU: the regularised Gram matrix is SPD).  Stores R as the level's regressor; R_host may be NULL. */
int sdm_solve(sdm_ctx* ctx, int level, int reg_type, float reg_param, int regularise_last_row,
              long long n_train_global, float* R_host, float* lambda_out);
/* Which of the reference's two solvers sdm_solve / sdm_solve_normal_equations / sdm_train_level run (LinearRegressor<Solver>,
 * regressors.hpp:318):
 *   SDM_SOLVER_CHOLESKY   (default) PartialPivLUSolver's role, regressors.hpp:199-234 -- blocked Cholesky, the SPD system needs no pivoting;
 *   SDM_SOLVER_COLPIV_QR  ColPivHouseholderQRSolver, regressors.hpp:242-306 -- Householder QR with column pivoting of AtA + reg on the
 *                         device (csrc/sdm_qr.hip), x = P R^-1 Q^T (At b); "much MUCH slower" there too (level-2 work, 2 F launches: 0.5 s at F = 8 801), and the
 *                         one that can tell a singular system: sdm_last_rank.  As Eigen's solve() / inverse() the back substitution stops at the last
 *                         nonzero pivot (largest remaining squared column norm below max ||a_j||^2 eps^2 / F * (F - k), or zero) and
 *                         returns zero coefficients for the remaining columns: a singular system gives a finite regressor ("we continued
 *                         learning", regressors.hpp:291).  Always replicated (installed sharding does not concern it; its levels take
 *                         the all-reduce, never the reduce-scatter), F <= 38 400. */
#define SDM_SOLVER_CHOLESKY 0
#define SDM_SOLVER_COLPIV_QR 1
int sdm_set_solver(sdm_ctx* ctx, int solver);
/* Rank of the last column-pivoted QR by Eigen's threshold (|R_kk| > eps * F * max |R_kk|) and the full rank F: what
 * qr_of_AtA.rank() / isInvertible() report at regressors.hpp:288-292 (the caller prints the warning; the library writes nothing to stdout). */
int sdm_last_rank(sdm_ctx* ctx, int* rank, int* full_rank);
/* Stand-alone normal equations for host data (any projection function, not only HOG): what
 * LinearRegressor<Solver>::learn hands to Solver::solve(data, labels, regulariser)
 * (regressors.hpp:199-234, 345-350).  A is n_rows x n_features, b is n_rows x n_outputs (<= 144),
 * R_host receives n_features x n_outputs.  Gram/RHS build, regulariser and Cholesky run on the GPU.
 * Does not need sdm_set_model_geometry. */
int sdm_solve_normal_equations(sdm_ctx* ctx, const float* A_host, int n_rows, int n_features,
                               const float* b_host, int n_outputs, int reg_type, float reg_param,
                               int regularise_last_row, float* R_host, float* lambda_out);
/* The same with the solver named PER CALL (SDM_SOLVER_*): the handle's sdm_set_solver choice is neither read nor changed, so two
 * LinearRegressor<Solver> objects with different solvers can share a handle (what the header layer's PartialPivLUSolver /
 * ColPivHouseholderQRSolver do, regressors.hpp:174-306).  rank / full_rank (either may be NULL) receive what qr_of_AtA.rank() and
 * the matrix order are at regressors.hpp:288-292; with SDM_SOLVER_CHOLESKY a successful solve reports full rank. */
int sdm_solve_normal_equations_with(sdm_ctx* ctx, int solver, const float* A_host, int n_rows, int n_features,
                                    const float* b_host, int n_outputs, int reg_type, float reg_param,
                                    int regularise_last_row, float* R_host, float* lambda_out, int* rank, int* full_rank);
/* Convenience: the four calls above + sdm_apply. */
int sdm_train_level(sdm_ctx* ctx, int level, int reg_type, float reg_param, int regularise_last_row,
                    long long n_train_global);

/* Regulariser sweep of one level: K candidates of the one tuning parameter LinearRegressor has (Regulariser's param,
 * regressors.hpp:126-148; set by hand in the reference, apps/rcr/data/rcr_training_22.cfg) for the price of one feature extraction and
 * one Gram product.  Rows [0, n_fit_rows) of the current samples are the fit rows, rows [n_fit_rows, N) are held out
 * (1 <= n_fit_rows < N, 1 <= K <= 32).  In order:
 *   1. sdm_hog_features(level) and the targets for all N rows;
 *   2. [A^T A | A^T b] over the fit rows only (sdm_gram_rhs' launches with n_fit_rows rows, its bf16 repeat included);
 *   3. the tiles the product wrote are copied beside G; ||G||_F^2 (MatrixNorm) is taken once, from the unregularised matrix;
 *   4. per candidate k: G restored, reg_params[k] added to the diagonal with n = n_train_global > 0 ? n_train_global : n_fit_rows,
 *      factored and solved by sdm_solve's launches (either solver) -- R_k, lambdas[k] and status[k] are what sdm_solve would give on a
 *      context holding the fit rows alone, bit for bit.  status[k] == SDM_ERR_NOT_SPD marks the candidate failed, the sweep goes on;
 *   5. per solved candidate: R_k applied to the current x into scratch rows (sdm_apply's launch; the state x is not touched) and
 *      holdout_err[k] = the mean of sdm_normalised_errors' matrix over the held-out rows, fit_err[k] (may be NULL) over the fit
 *      rows: float32 entries as sdm_normalised_errors computes them, summed in double in a fixed order (two runs: the same bits).  A
 *      failed candidate gets +inf;
 *   6. *best = arg-min of holdout_err, ties to the lowest k; slot `best` becomes the level's regressor (a device copy) and is applied
 *      to all N rows, as sdm_train_level ends.  If every candidate failed: SDM_ERR_NOT_SPD, *best = -1, and x, the level's regressor
 *      and whether it has one stay as before the call.
 * The Gram matrix does not survive the call (sdm_solve afterwards needs sdm_gram_rhs again).  Single rank only: with an all-reduce, a
 * reduce-scatter or solve sharding installed on the handle the call returns SDM_ERR_INVALID (a multi-rank sweep would have to reduce the
 * held-out sums as well).  The passes are timed under SDM_T_REG / SDM_T_FACTOR (scoring: SDM_T_APPLY), the snapshot under SDM_T_GRAM. */
int sdm_train_level_sweep(sdm_ctx* ctx, int level, int reg_type, const float* reg_params, int K, int regularise_last_row,
                          long long n_train_global, int n_fit_rows, double* holdout_err /* K */, double* fit_err /* K or NULL */,
                          float* lambdas /* K */, int* status /* K */, int* best);
/* Candidate k of the last sweep of this handle, F x M row-major like sdm_get_regressor (SDM_ERR_NOT_SPD for a failed candidate;
 * SDM_ERR_INVALID when there is none: no sweep yet, k out of range, or the geometry was changed since). */
int sdm_sweep_get_regressor(sdm_ctx* ctx, int k, float* R_host);

/* Device views for collectives / zero-copy interop (valid until the next allocation-changing call). */
int sdm_gram_device_ptr(sdm_ctx* ctx, void** dev_ptr, size_t* count_f32);
int sdm_x_device_ptr(sdm_ctx* ctx, void** dev_ptr, size_t* count_f32);
/* (Handing out the pointer marks the rows as possibly caller-written: an sdm_apply of this level then runs the f32 matrix-core
 * kernel instead of the float16-piece one, whose 2^12 pre-scale is exact only for |feature| < 16 -- always true of HOG output,
 * not of arbitrary data.  The same holds once templates have been subtracted, sdm_set_templates.) */
int sdm_features_device_ptr(sdm_ctx* ctx, void** dev_ptr, long long* ld, int* n_rows);

/* Profiling. */
int sdm_enable_timing(sdm_ctx* ctx, int on);
int sdm_get_timing(sdm_ctx* ctx, float* ms /* [SDM_T_COUNT] */, int* launches /* [SDM_T_COUNT] */, int reset);

/* Test hooks (used by tests/ to check intermediate integer/byte results bit-exactly). */
int sdm_debug_patch(sdm_ctx* ctx, int level, int sample, int landmark, uint8_t* resized_SxS,
                    uint8_t* bins_SxS, float* hist_2OxCxC, float* desc_P);
/* Instrumented HOG launch (O=4, C=5 geometry only): per-phase shader cycles summed over all waves:
 * [0] geometry/tables [1] histogram clear [2] row loop [3] barrier [4] normalisation [5] output stores, [7] waves. */
int sdm_debug_hog_profile(sdm_ctx* ctx, int level, unsigned long long* out8);
int sdm_debug_gradient_table(sdm_ctx* ctx, int level, float* g_511x511, int* bin_511x511);
/* Development switches by name (A/B handles of kernels kept as fallbacks, test knobs; the list is at the definition in
 * csrc/sdm_capi_debug.hip).  The library reads no environment variable. */
int sdm_debug_set_option(sdm_ctx* ctx, const char* name, int value);
/* The Cholesky's trailing update C -= P^T P on the float16 matrix cores, by itself (unit test of syrk_update_f16_w4_kernel at panel
 * groups of 128 ... 512 rows): P rows x wcols host, C wcols x wcols host in/out (upper 128 x 128 tiles with tile row < wcols_factor / 128). */
int sdm_debug_update_f16(sdm_ctx* ctx, const float* P_host, int rows, int wcols, int wcols_factor, float factor_bound, float* C_host);
/* The first n images (all width x height) of the context-owned single-channel image set, back to the host. */
int sdm_debug_download_images(sdm_ctx* ctx, uint8_t* out, int n, int width, int height);
/* Image i of ANY image set (owned, sdm_set_images_device, sdm_set_frames_device), read through the image table: out receives
 * width x height bytes, dense. */
int sdm_debug_download_image(sdm_ctx* ctx, int i, uint8_t* out);
/* Lane packing of the HOG launch (default on; also sdm_debug_set_option(ctx, "hog_no_pack", 1)): in SDM_HOG_COLUMNS
 * mode a wave walks a GROUP of patches of one sample in passes of 64 pixel columns instead of one patch per wave (a 50-column
 * ROI then fills the wave).  Same integer decisions; a patch cut by a pass boundary sums its cells from two partial folds.
 * Off = one patch (or one landmark pair) per wave, for A/B comparison in tests. */
int sdm_debug_set_hog_packing(sdm_ctx* ctx, int on);
/* How many sdm_gram_rhs launches of this context had to be repeated with three bf16 pieces because an operand left float16's
 * range (the Gram matrix A^T A / A^T b of regressors.hpp:208,225 is formed on the 16-bit matrix cores from two float16 pieces per
 * f32 operand -- float32 accuracy, see csrc/sdm_gram_bf16.hip; the repeat keeps float32's range).  Tests. */
int sdm_debug_gram_fallbacks(sdm_ctx* ctx);
/* How many factorisations of this context ran their trailing updates on the f32 matrix-core kernel because the diagonal of the
 * regularised Gram matrix spanned more than 2^20 (the float16-piece updates of csrc/sdm_gram_bf16.hip share one power-of-two
 * scale per factorisation; PartialPivLUSolver::solve, regressors.hpp:224-225, on arbitrary data).  Tests. */
int sdm_debug_update_fallbacks(sdm_ctx* ctx);
/* The packing plan of a level geometry (host only, no device needed): info5 = {G, P, n_main, Gt, Pt} (G == 0: no packed
 * instance for this geometry); lane_tab [passes][64], wb [passes][64][16], pass_info [passes][4] as documented in
 * superviseddescent_amd/csrc/sdm_kernels.h (HogPlanDev); passes = P + Pt <= max_passes. */
int sdm_debug_hog_plan(int num_cells, int cell_size, int num_bins, int num_landmarks, int* info5, unsigned* lane_tab,
                       float* wb, int* pass_info, int max_passes);
/* cut[num_landmarks]: 1 where the landmark's patch is cut by a pass boundary of that plan (its raw cell histograms arrive in two
 * parts, csrc/sdm_hog_packed.hip CELLS form); host only.  Returns SDM_ERR_INVALID when the geometry has no packed instance. */
int sdm_debug_hog_plan_cut(int num_cells, int cell_size, int num_bins, int num_landmarks, int* cut);
/* columns3[num_landmarks][3] = {cut, jA, jB}: part 0 of the landmark's raw cells holds the cell columns 0 .. jA, part 1 (cut patches)
 * the columns jB .. num_cells - 1; no other (part, column) is written or read, its fold weights are all zero (csrc/sdm_kernels.h:
 * HogPlanHost::cut).  Uncut: {0, num_cells - 1, num_cells}.  Host only; SDM_ERR_INVALID when the geometry has no packed instance. */
int sdm_debug_hog_plan_columns(int num_cells, int cell_size, int num_bins, int num_landmarks, int* columns3);
/* Tests: the band-slot weights {slot 0, slot 1} of the resized-ROI rows d < num_cells * cell_size (hog.c:697-704; zero for the cell
 * rows -1 and num_cells, swapped on odd bands; rows from num_cells * cell_size on are zero) as the one definition of them gives them
 * (csrc/sdm_kernels.h: packed_row_const) -- for the cell sizes with specialised pixel-kernel instances the values the COMPILER
 * evaluated, which are the constants the detect instances multiply by; host only.  SDM_ERR_INVALID unless
 * 1 <= num_cells * cell_size <= 64. */
int sdm_debug_hog_band_weights(int cell_size, int num_cells, float out[64][2]);
/* Tests: the level's table of cv::resize taps as the device built it at sdm_set_model_geometry (csrc/sdm_hog_packed.hip,
 * taps_table_kernel): table[128 half-widths][64 coordinates][8] ints = {s0, c0 | c1 << 16, sy0, sy1, b0 << 12, b1 << 12, carry mask of
 * the row, half-width is one-load eligible}.  info3 = {the level's HOG launch of detect is the raw-cells launch as the context stands
 * (packed plan, SDM_HOG_COLUMNS, descriptor kernel available), that launch is an instance with the one-load row loop, option
 * hog_two_load}.  SDM_ERR_INVALID when the level has no packed plan. */
int sdm_debug_hog_taps(sdm_ctx* ctx, int level, int* table, int* info3);
/* Tests: the level's pair-loop table as the device built it from the same taps (csrc/sdm_hog_packed.hip, pair_taps_table_kernel):
 * table[128 half-widths][64][4] ints = {row d takes its lower source row from the pair's spare (all ones) or from row d - 1's upper row
 * (zero), source row of the spare of pixel rows (2d + 1, 2d + 2) or -1 where the pair needs none, half-width is pair eligible, orphan
 * rows of the patch}.  info2 = {the level's raw-cells launch is an instance with the pair loop, option hog_two_load}.
 * SDM_ERR_INVALID when the level has no packed plan. */
int sdm_debug_hog_pair_taps(sdm_ctx* ctx, int level, int* table, int* info2);
/* Round 4, A/B and tests: which launches the packed default mode uses.  fused != 0 (default; sdm_debug_set_option "detect_unfused" turns it
 * off): sdm_detect_batch runs  pixel kernel -> raw cell histograms -> descriptors x regressor slices on the 16-bit matrix cores
 * (csrc/sdm_desc.hip) -> landmark update, and never writes the N x F feature matrix (LinearRegressor::predict,
 * regressors.hpp:377-381, fused behind HogTransform::operator(), adaptive_vlhog.hpp:109-185) when 2L <= 64 (wider outputs stay on the
 * feature-matrix path, which is faster there; fused == 2 fuses them too).  split_store != 0 (default 0; env
 * option "hog_split_store"): sdm_hog_features / training produce the feature rows through the same raw cells + the store form of
 * that kernel instead of normalising inside the pixel kernel (identical arithmetic, last-bit differences from the summation order
 * of the four clamped block terms). */
int sdm_debug_set_detect_path(sdm_ctx* ctx, int fused, int split_store);

/* Head pose from 2D landmarks: the ModelProjection cascade of the reference's examples/pose_estimation.cpp -- a known-template
 * SupervisedDescentOptimiser (superviseddescent.hpp:195-197, 287-292) over LinearRegressor<> levels (:281-283), NoNormalisation.
 * Its state lives in the handle beside the landmark state, so that a detect batch's landmarks reach it without leaving the device.
 *   parameter row  x = [r_x, r_y, r_z, t_x, t_y, t_z], angles in degrees (deg2rad, :41)
 *   projection     MVP = P * T(t) * R_y * R_x * R_z (:222, rotations :58-98), P the perspective of :142-154 with
 *                  fovy = rad2deg(2 atan2(height, 2 focal)) (:46), aspect = width / height; clip = MVP (X, Y, Z, 1), divide by w,
 *                  viewport (:164-174), u = (x_ss - width/2) / focal, v = (y_ss - height/2) / focal (:232)
 *   feature row    [u_0..u_{K-1}, v_0..v_{K-1}] (F = 2K, no bias column, regressors.hpp:345-350); observed = features - templates;
 *                  x_{k+1} = x_k - observed * R_k (R_k: 2K x 6)
 * Limits (SDM_ERR_INVALID otherwise): 1 <= K <= 64 model points, 6 parameters, levels 0..15, N >= 1. */
/* points: K x 3 model coordinates (the homogeneous w = 1 is implied).  The example uses focal 1800, 1000 x 1000, near 1, far 5000.
 * A different K drops the pose regressors and templates. */
int sdm_pose_set_model(sdm_ctx* ctx, const float* points, int K, float focal, float width, float height, float near_, float far_);
/* current_x of the pose cascade: N x 6 (host, or a device-to-device copy) */
int sdm_pose_set_x(sdm_ctx* ctx, const float* x_host, int n_samples);
int sdm_pose_get_x(sdm_ctx* ctx, float* x_host);
int sdm_pose_set_x_device(sdm_ctx* ctx, const float* x_dev, int n_samples);
/* the known templates y (the observed landmarks, normalised as :327): n_samples x 2K, [u_0..u_{K-1}, v_0..v_{K-1}] */
int sdm_pose_set_templates(sdm_ctx* ctx, const float* templates, int n_samples, int feature_dim);
/* Detect -> pose on the device: the templates of all N rows of the LANDMARK state x (N x 2L pixel coordinates, e.g. after
 * sdm_detect_batch): template[n] = [(x_n[idx_k] - W_n / 2) / focal .., (y_n[idx_k] - H_n / 2) / focal ..] with W_n x H_n the size of
 * row n's image (sdm_set_sample_image_index).  K must equal the pose model's K; 0 <= landmark_index[k] < L. */
int sdm_pose_templates_from_landmarks(sdm_ctx* ctx, const int* landmark_index, int K, float focal);
/* training targets x*: N x 6 for the current rows (`parameters`, superviseddescent.hpp:165) */
int sdm_pose_set_targets(sdm_ctx* ctx, const float* xstar_host, int n_samples);
/* the observed values of the current x: N x 2K (features - templates when templates are set for these rows).  Tests. */
int sdm_pose_features(sdm_ctx* ctx, int level, float* out_host);
/* One training level (superviseddescent.hpp:170-218): projection, b = x - x*, [A|b]^T [A|b] summed in double in a fixed order
 * (bit-identical runs for the same N), Regulariser::get_matrix (regressors.hpp:126-148; lambda as sdm_solve reports it), LU with
 * partial pivoting in double (regressors.hpp:199-234) -- a singular system returns what the factorisation gives, not an error --
 * then x <- x_{k+1} with the regressor of this level (the launch of sdm_pose_test).  R_host (2K x 6) and lambda_out may be NULL. */
int sdm_pose_train_level(sdm_ctx* ctx, int level, int reg_type, float reg_param, int regularise_last_row, float* R_host, float* lambda_out);
/* the regressor of a pose level, 2K x 6 row-major */
int sdm_pose_set_regressor(sdm_ctx* ctx, int level, const float* R_host);
int sdm_pose_get_regressor(sdm_ctx* ctx, int level, float* R_host);
/* Levels first_level .. first_level + n_levels - 1 on all rows in ONE launch (test / predict, superviseddescent.hpp:262-344):
 * a row's result is bit-identical whatever the batch and whether the levels run in one call or one call each. */
int sdm_pose_test(sdm_ctx* ctx, int first_level, int n_levels);

/* Multi-stream face tracking: rcr::detection_model::detect(image, initialisation) (include/rcr/model.hpp:146-157) frame after frame
 * for many faces at once, the loop apps/rcr/rcr-track.cpp:133-177 sketches.  The handle holds a table of `capacity` stream slots in
 * HBM: per slot the landmark row (2L floats, the layout of x), the face box it was started from and a status.  A step runs the
 * cascade of sdm_detect_batch, unchanged, on n rows taken from the slots, and writes the results back into them: a stream's
 * landmarks never leave the device between frames.  Row i of a step belongs to stream ids[i], its image is the current image
 * set's entry for row i (sdm_set_sample_image_index; identity by default) -- several faces in one frame are several streams on
 * the same image.  After a step the current rows x are the step's results in ids order, as after sdm_detect_batch: sdm_get_x,
 * sdm_pose_templates_from_landmarks and the other entry points of the landmark state see them.
 *   init of row i   STARTED slot (sdm_track_start since its last step): align_mean(mean, box), bit-identical to
 *                   sdm_init_from_boxes, so the first step equals sdm_detect_batch from the box;
 *                   SDM_TRACK_INIT_PREVIOUS: the slot's landmarks (detect(image, initialisation));
 *                   SDM_TRACK_INIT_REALIGN: the mean in the enclosing box of the slot's landmarks, float32, every operation rounded:
 *                   x0_j = ((m_j - min m_x) / (max m_x - min m_x)) * (max x - min x) + min x, y the same with the y quantities
 *   lost rule       bit mask of the result row, 0 = tracked (SDM_TRACK_LOST_*):
 *                   NONFINITE  a coordinate is not finite (then no other bit is evaluated)
 *                   SMALL      the enclosing box is narrower or lower than min_size pixels
 *                   OUTSIDE    the box centre ((x0 + x1) * 0.5f, (y0 + y1) * 0.5f) lies outside [0, W) x [0, H) of the row's image
 *                   SCALE      eye landmarks set and max_scale_change > 0: IED(result) > IED(init) * k or IED(result) * k < IED(init),
 *                              in double (get_ied, include/rcr/helpers.hpp:136-160)
 *                   A slot with a non-zero mask becomes LOST: it keeps its last landmarks and is refused by later steps until
 *                   sdm_track_start gives it a new box (rcr-track.cpp's have_face = false -> face detector -> restart).
 * Argument errors (SDM_ERR_INVALID) change no state and launch nothing: no geometry, a level without regressor, tracker not
 * configured, the geometry's L changed since sdm_track_configure, n < 1, an id out of range or repeated within the call, a step
 * on a FREE or LOST slot, templates set (sdm_set_templates), or images that do not cover the n rows. */
#define SDM_TRACK_FREE 0
#define SDM_TRACK_STARTED 1
#define SDM_TRACK_TRACKED 2
#define SDM_TRACK_LOST 3
#define SDM_TRACK_INIT_PREVIOUS 0
#define SDM_TRACK_INIT_REALIGN 1
#define SDM_TRACK_LOST_NONFINITE 1
#define SDM_TRACK_LOST_SMALL 2
#define SDM_TRACK_LOST_OUTSIDE 4
#define SDM_TRACK_LOST_SCALE 8
/* capacity >= 1 slots, all FREE; mean: 2L floats in the unit box (the model's mean, width and height > 0); init_mode
 * SDM_TRACK_INIT_*; min_size >= 0 pixels; max_scale_change >= 0 (0: no scale rule).  Needs the geometry; drops every slot. */
int sdm_track_configure(sdm_ctx* ctx, int capacity, const float* mean, int init_mode, float min_size, float max_scale_change);
/* (Re)start slots from face boxes (n x {x, y, width, height} ints, width and height > 0), whatever their status: STARTED. */
int sdm_track_start(sdm_ctx* ctx, const int* ids, const int* boxes, int n);
/* Slots become FREE (host bookkeeping only, nothing is launched). */
int sdm_track_stop(sdm_ctx* ctx, const int* ids, int n);
/* One frame for n STARTED or TRACKED streams: gather + init -> the cascade of sdm_detect_batch -> commit + lost rule.  One copy
 * of the ids to the device, one of the masks (and of the n x 2L results when landmarks_host is given) back, one synchronise.
 * landmarks_host (n x 2L) and lost_host (n masks) may be NULL.  SDM_ERR_EMPTY_PATCH as sdm_get_x reports it, after the step has
 * been committed. */
int sdm_track_step(sdm_ctx* ctx, const int* ids, int n, float* landmarks_host, int* lost_host);
/* The slots' landmark rows (n x 2L; a STARTED slot gives its align_mean(mean, box)) and statuses (SDM_TRACK_FREE ...); either
 * output may be NULL.  The current rows x are not touched. */
int sdm_track_get(sdm_ctx* ctx, const int* ids, int n, float* landmarks_host, int* status_host);

/* Rolled faces: upright-normalised detect and tracking.  A cascade tolerates the roll its training set held and no more: from a box
 * on a face rolled by 30 degrees an upright-trained cascade ends where it started.  Here every row's face is cut out of its frame
 * as a chip x chip gray image in which it stands upright -- one launch for all rows --, the unchanged cascade of sdm_detect_batch
 * runs on that stack of chips (one image per row), and one small launch maps the result rows back into frame coordinates: after
 * either call below the current rows x are in FRAME coordinates, and sdm_get_x, sdm_align_crops*, sdm_pose_templates_from_landmarks
 * and the tracker's lost rule work on them unchanged.
 *   roll      positive = clockwise on screen (x right, y down): a face with roll t has its eye line, from the subject's right eye to
 *             their left eye (left to right in the image), along (cos t, sin t).
 *   inputs    per row doubles c, s with c^2 + s^2 = 1 and an integer centre (ix, iy); hc = chip / 2 (integer division).
 *   M         chip -> frame, float32, the translations evaluated in double and rounded once:
 *               M00 = c, M01 = -s, M02 = ix - (c hc - s hc);  M10 = s, M11 = c, M12 = iy - (s hc + c hc)
 *   W         frame -> chip (the tracker only): W00 = c, W01 = s, W02 = hc - (c ix + s iy);  W10 = -s, W11 = c, W12 = hc - (c iy - s ix)
 *   points    through a matrix A: ((A00 x + A01 y) + A02, (A10 x + A11 y) + A12) in float32, every operation rounded, nothing contracted.
 *   chip      pixel (column j, row i) is the `sample` rule of sdm_align_crops with M, out_width = out_height = chip, one channel, on the
 *             row's gray context image (sdm_set_sample_image_index; gray and NV12 luma in place, colour as sdm_set_frames_device
 *             converted it): 1/32-pixel positions, (.. + 512) >> 10, a tap outside the frame reads 0.  At roll 0 the chip is a byte copy
 *             of the frame region, at 90, 180 and 270 degrees an exact rotation.  Row n's chip is image n of a stack the context
 *             owns: each chip starts on a 16-byte boundary, row stride (chip + 15) & ~15 (the padding is zero), 64-bit offsets.
 *   detect    box (x, y, w, h) and roll_deg: ix = x + w / 2, iy = y + h / 2 (integer division); c, s on the host in double -- a multiple
 *             of 90 degrees gives exactly 0 / +-1, otherwise cos / sin of (double)roll_deg * pi / 180.  The initialisation is
 *             align_mean(mean, (hc - w / 2, hc - h / 2, w, h)), bit-identical to sdm_init_from_boxes on that box; the cascade runs all
 *             levels on the chips; the result is the rows through M.
 *   tracker   (sdm_track_configure_upright) a STARTED slot behaves as detect, with the roll of sdm_track_start_rolled (sdm_track_start:
 *             roll 0).  A TRACKED slot with landmarks p takes its roll from its eye line: the eye centres as the inter-eye distance
 *             forms them (float32 sums in index order, divided by the count), dx = lx - rx, dy = ly - ry in float32, then in double
 *             n = sqrt(dx^2 + dy^2), c = dx / n, s = dy / n (n == 0 or not finite: c = 1, s = 0); ix = (int)floorf((min x + max x) * 0.5f)
 *             with the float clamped to +-2^20 first, iy likewise.  The row's init is the SDM_TRACK_INIT_REALIGN rule, same arithmetic,
 *             applied to q = W p (whatever init_mode the tracker was configured with).  Behind the cascade and the back-map the commit
 *             and the lost rule run unchanged on the frame-coordinate result, the frames' sizes and the chip-coordinate init (of which
 *             the SCALE rule takes the inter-eye distance).  The first step of a started stream equals sdm_detect_batch_upright.
 *   flags     per row, kept with M until the next upright call (sdm_upright_get):
 *             SDM_UPRIGHT_PARTIAL    a chip corner samples outside [0, W - 1] x [0, H - 1] (the rule of SDM_ALIGN_PARTIAL; informational)
 *             SDM_UPRIGHT_NEAR_EDGE  a result landmark q (chip coordinates, float32) has less than `guard` pixels to the border of the
 *                                    chip: not (qx >= guard, qy >= guard, (chip - 1) - qx >= guard, (chip - 1) - qy >= guard).  Patches
 *                                    may have read black where the frame has pixels: the chip is too small for this face.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: chip outside [32, 1024], guard outside [0, chip / 2), a non-finite
 * roll, a box without area, n < 1, no geometry, a level without regressor, no images, templates set, an image index that does not
 * cover the rows, eye indices missing where a level's patches need them, an upright call before sdm_upright_configure; upright
 * tracking without both eye index sets, without sdm_upright_configure or before sdm_track_configure; and everything sdm_detect_batch
 * and sdm_track_step refuse.  sdm_track_configure itself is unchanged. */
#define SDM_UPRIGHT_PARTIAL 1
#define SDM_UPRIGHT_NEAR_EDGE 2
/* chip in [32, 1024] pixels, guard in [0, chip / 2). */
int sdm_upright_configure(sdm_ctx* ctx, int chip, int guard);
/* mean: 2L floats; boxes: n x {x, y, width, height}; roll_deg: n angles.  One copy in, one synchronise.  x_host (n x 2L, frame
 * coordinates) may be NULL.  SDM_ERR_EMPTY_PATCH as sdm_get_x reports it. */
int sdm_detect_batch_upright(sdm_ctx* ctx, const float* mean, const int* boxes, const float* roll_deg, int n, float* x_host);
/* Of the last upright call (detect or tracker step): matrices_host N x 6 (M00 M01 M02 M10 M11 M12), flags_host N, chips_host
 * N x chip x chip bytes, dense.  Each may be NULL. */
int sdm_upright_get(sdm_ctx* ctx, float* matrices_host, int* flags_host, uint8_t* chips_host);
/* Upright mode of the tracker on (enable != 0) or off.  Needs sdm_track_configure, sdm_upright_configure and both eye index sets.
 * After a later sdm_track_configure with more slots, call it again before the next start or step (they are refused until then). */
int sdm_track_configure_upright(sdm_ctx* ctx, int enable);
/* sdm_track_start with a roll per stream (degrees; the rule of sdm_detect_batch_upright).  Needs upright mode. */
int sdm_track_start_rolled(sdm_ctx* ctx, const int* ids, const int* boxes, const float* roll_deg, int n);

/* Tracking, filtered: a temporal filter on the tracker's output.  A regression cascade's answer jitters by a fraction of a pixel from
 * frame to frame, on a face that does not move too; crops, warps and pastes fitted to the rows carry that jitter on.  The filter is
 * the One-Euro filter (Casiez, Roussel, Vogel 2012): a first-order low-pass whose cut-off rises with the filtered speed -- steady
 * when the face is still, no lag when the head moves --, the speed measured in units of the face's own size, so that one parameter
 * set serves a 60-pixel and a 600-pixel face.  It filters what a step RETURNS, in one launch behind the commit: the slots' landmark
 * rows stay raw, so the next step's initialisation, the lost rule and sdm_track_get are bit-identical to a tracker without it.
 * After sdm_track_step_filtered the current rows x are the FILTERED rows in ids order: sdm_get_x, sdm_align_crops*, sdm_warp_*,
 * the pastes without _at and sdm_pose_templates_from_landmarks work on them.  sdm_upright_get's matrices and flags are those of
 * the raw step.
 *   parameters   min_cutoff > 0 (Hz), beta >= 0 (Hz per face size per second), d_cutoff > 0 (Hz)
 *   state        per slot three rows of 2L floats -- r the previous raw row, d the filtered derivative, f the previous filtered row --
 *                and one int, primed.  sdm_track_configure_filter allocates it, all slots un-primed; sdm_track_start and
 *                sdm_track_start_rolled un-prime the slots they name.
 *   arithmetic   float32, every operation rounded as written, nothing contracted.  Row i of a step with raw result x (frame
 *                coordinates), lost mask m and dt = dt_seconds[i]:
 *                  alpha(fc)  = 1.0f / (1.0f + (1.0f / (6.2831855f * fc)) / dt)
 *                  m != 0     : out = x; primed = 0                        (a lost row passes through, its state is dropped)
 *                  !primed    : r = x; d = 0; f = x; out = x; primed = 1   (first filtered step since start / restart / configure)
 *                  otherwise  : s  = fmaxf(max x - min x, max y - min y) of the row    (min / max are exact in any order)
 *                               w  = s > 0 ? beta / s : 0
 *                               ad = alpha(d_cutoff)
 *                               per coordinate j:
 *                                 v  = (x[j] - r[j]) / dt
 *                                 dn = (ad * v) + ((1.0f - ad) * d[j]);       dn not finite: dn = 0
 *                                 a  = alpha(min_cutoff + w * fabsf(dn))
 *                                 fn = (a * x[j]) + ((1.0f - a) * f[j]);      fn not finite: fn = x[j]
 *                                 r[j] = x[j]; d[j] = dn; f[j] = fn; out[j] = fn
 *   dt           seconds since the stream's last FILTERED step, in [1e-4, 1e4]: the bounds keep v finite for any pixel coordinate.
 *                sdm_track_step never touches the filter's state, whether a filter is configured or not.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched, the slot table, the filter state and the current rows keep their
 * bits: everything sdm_track_step refuses; no filter configured (or OFF) for the step and the get; an unknown mode; min_cutoff or
 * d_cutoff not finite or not > 0; beta not finite or < 0; dt_seconds NULL; a dt outside [1e-4, 1e4] or not finite. */
enum {
    SDM_TRACK_FILTER_OFF = 0,
    SDM_TRACK_FILTER_ONE_EURO = 1       /* the arithmetic above */
};
/* Needs sdm_track_configure; allocates the state for its capacity, all slots un-primed.  mode OFF frees the state (the parameters
 * are not looked at).  A later sdm_track_configure switches the filter off. */
int sdm_track_configure_filter(sdm_ctx* ctx, int mode, float min_cutoff_hz, float beta, float d_cutoff_hz);
/* sdm_track_step, in plain and in upright mode, plus the filter launch: the same copies (the n step times travel with the ids), one
 * synchronise, SDM_ERR_EMPTY_PATCH reported the same way.  landmarks_host receives the raw rows, filtered_host the filtered rows
 * (n x 2L each); landmarks_host, lost_host and filtered_host may be NULL. */
int sdm_track_step_filtered(sdm_ctx* ctx, const int* ids, int n, const float* dt_seconds, float* landmarks_host, int* lost_host,
                            float* filtered_host);
/* The slots' filtered rows f and derivative rows d (n x 2L each) and primed flags (n); an un-primed slot gives zeros and 0.  Each
 * output may be NULL.  Neither the state nor the current rows x are touched. */
int sdm_track_get_filtered(sdm_ctx* ctx, const int* ids, int n, float* filtered_host, float* derivative_host, int* primed_host);

/* Tracking, motion-compensated: a step starts from where the face WAS, and the cascade pulls a shape in only from about as far as its
 * training perturbations reached (a few percent of the face box).  A head turn, a hand-held phone or a slow camera moves a face further
 * between two frames.  With a motion mode configured every step first estimates each tracked stream's translation between its last
 * frame and the new one by block matching on a small chip, and starts the cascade from the shifted landmarks.  Off by default: with no
 * mode configured every call runs the launches it ran before and gives the same bits.  All arithmetic is integer except where stated.
 *   parameters   search S in [1, 16] chip pixels, scale finite in [0.5, 4], min_gain in [0, 255]; the chip side is C = 32.
 *   state        per slot: valid, the grid (k, ox, oy) and a 32 x 32 u8 reference chip.  sdm_track_configure_motion allocates it, all
 *                slots invalid; sdm_track_start and sdm_track_start_rolled invalidate the slots they name.
 *   block mean   B(X, Y, k) = (sum_{u, v < k} g(X + u, Y + v) + k^2 / 2) / k^2 (integer divisions), g the gray byte of the row's context
 *                image in the step's image set (sdm_set_sample_image_index; the image the upright chip reads: gray and NV12 luma in
 *                place, colour and P010 as converted), 0 outside the image.
 *   store        one launch behind the commit, for every row of the step.  Lost mask != 0: valid = 0.  Otherwise, from the committed RAW
 *                row p with x0, x1, y0, y1 the min and max of its coordinates, in float32 with every operation rounded:
 *                  side = fmaxf(x1 - x0, y1 - y0) * scale;  k = min(64, max(1, (int)ceilf(side / 32.0f)))
 *                  cx = (int)floorf((x0 + x1) * 0.5f) with the float clamped to +-2^20 first, cy likewise;  ox = cx - 16 k, oy = cy - 16 k
 *                  chip[j][i] = B(ox + i k, oy + j k, k) for i, j < 32;  valid = 1
 *   search       one launch ahead of the gather, for every row whose slot is TRACKED and valid, in the NEW image of the row:
 *                  cur[j][i] = B(ox - S k + i k, oy - S k + j k, k) for i, j < 32 + 2 S
 *                  SAD(dx, dy) = sum_{i, j < 32} |cur[S + dy + j][S + dx + i] - chip[j][i]| for dx, dy in [-S, S]
 *                  best = the lexicographic minimum of (SAD, dx^2 + dy^2, dy, dx);  zero = SAD(0, 0)
 *                  shift = (dx k, dy k) of best if best.SAD * 256 <= zero * (256 - min_gain), else (0, 0)
 *                Every sum stays below 2^31.  A STARTED slot or one without a valid chip gets the shift (0, 0) and is not searched.
 *   use          the shift is added, as float32 with one rounded add per coordinate, to the slot's landmarks AS THE GATHER READS THEM:
 *                SDM_TRACK_INIT_PREVIOUS, SDM_TRACK_INIT_REALIGN and the upright tracker's p ahead of its roll, centre and W.  The slot
 *                table is not modified; the SCALE rule's init is the shifted init.  With the shift (0, 0) a row's step is bit-identical
 *                to a step without the mode.
 *   filter       sdm_track_step and sdm_track_step_filtered both run the two launches; the store reads the raw rows, the One-Euro state
 *                is not touched by either.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: a parameter outside its range, an unknown mode, a call before
 * sdm_track_configure, sdm_track_get_motion without a mode, an id out of range or named twice.
 * Out of scope: sub-chip-pixel refinement, a rotation or scale search, and any lost rule built on the SAD values -- they are returned so
 * that such a rule can be studied. */
enum {
    SDM_TRACK_MOTION_OFF = 0,
    SDM_TRACK_MOTION_SAD = 1            /* the block matching above */
};
/* Needs sdm_track_configure; allocates the state for its capacity, all slots invalid.  mode OFF frees the state (the parameters are
 * not looked at).  A later sdm_track_configure switches the mode off. */
int sdm_track_configure_motion(sdm_ctx* ctx, int mode, int search, float scale, int min_gain);
/* Of the named slots: motion_host n x 6 ints -- the last step's shift (dx, dy) in pixels, the best SAD, SAD(0, 0), k and whether the
 * row was searched (all 0 when it was not, or never stepped) --, grid_host n x 3 ints (k, ox, oy) and chips_host n x 32 x 32 bytes, zeros
 * where a slot holds no valid chip.  Each may be NULL.  No state is touched. */
int sdm_track_get_motion(sdm_ctx* ctx, const int* ids, int n, int* motion_host, int* grid_host, uint8_t* chips_host);

/* Aligned face crops of the current rows (after sdm_detect_batch, sdm_track_step or sdm_set_x): for every row n of x (N x 2L, what
 * sdm_get_x returns) an out_width x out_height x C u8 crop in which the face stands in a canonical position -- the input of
 * recognition, expression or attribute networks -- without the landmarks or the frames leaving the device.
 *   fit     the least-squares similarity without reflection that maps the row's K landmarks p_k = (x[idx_k], x[L + idx_k]) onto
 *           the template points q_k (crop pixel coordinates), in double: centre both sets, a = sum(p~.q~) / sum|p~|^2,
 *           b = sum(p~x q~y - p~y q~x) / sum|p~|^2, t = q_bar - [[a, -b], [b, a]] p_bar (summation order free).  Its inverse, the crop
 *           -> source matrix M (2 x 3), is [[a, b], [-b, a]] / (a^2 + b^2) with the translation p_bar - [[a, b], [-b, a]] q_bar /
 *           (a^2 + b^2), rounded to float32.
 *   sample  output pixel (column j, row i), integer coordinates at the pixel centres (the cv::warpAffine convention):
 *           sx = (M00 j + M01 i) + M02, sy = (M10 j + M11 i) + M12 in float32, every operation rounded, nothing contracted.
 *           X = floor(sx * 32 + 0.5f) in float32, x0 = X >> 5, fx = X & 31, y the same; per channel
 *           (w00 p(x0, y0) + w10 p(x0 + 1, y0) + w01 p(x0, y0 + 1) + w11 p(x0 + 1, y0 + 1) + 512) >> 10 with w00 = (32 - fx)(32 - fy),
 *           w10 = fx (32 - fy), w01 = (32 - fx) fy, w11 = fx fy.  A tap outside the image reads 0; a non-finite position, or one
 *           with |sx| or |sy| > 2^20, gives 0.  Plain bilinear, no antialiasing: this interleaved u8 form, alpha included, stays
 *           bilinear (sdm_align_crops_tensor_filtered averages a minifying row's footprint).
 *   flags   SDM_ALIGN_DEGENERATE: a selected landmark is not finite, or sum|p~|^2 == 0 -- the crop is all zeros, M six NaNs, and no
 *           other bit is evaluated.  SDM_ALIGN_PARTIAL: a crop corner (column 0 or out_width - 1, row 0 or out_height - 1) samples
 *           outside [0, W - 1] x [0, H - 1] of the row's image, on the float32 positions above.
 *   source  default: the context's own images (single-channel, the ones detect and track read; sizes may differ; rows map to images
 *           through sdm_set_sample_image_index as in detect).  sdm_align_set_source: a stack of n_images equally sized interleaved
 *           u8 images of C in {1, 3, 4} channels, channel order kept (BGR stays BGR) -- e.g. the colour frames whose gray version the
 *           cascade ran on.  In host memory it is copied once, here; in device memory (on_device) it is used in place and must stay
 *           valid while crops are made from it.  base NULL: back to the context's images.
 * Argument errors (SDM_ERR_INVALID) change no state and launch nothing: no geometry (sdm_set_model_geometry), no current rows, K
 * outside [2, L], a landmark index out of range or repeated, a template point not finite or all K template points equal,
 * out_width or out_height outside [1, 1024], out NULL (or, on the device, not 4-byte aligned; 16 when C = 4), channels outside
 * {1, 3, 4}, stride_bytes < width * channels, n_images / width / height < 1, a source that does not cover every row's image index,
 * and an external stack whose width and height are not those of the context image a row maps to.  Every offset is 64-bit. */
#define SDM_ALIGN_DEGENERATE 1
#define SDM_ALIGN_PARTIAL 2
int sdm_align_set_source(sdm_ctx* ctx, const uint8_t* base, int n_images, int width, int height, int stride_bytes, int channels,
                         int on_device);
/* One call for all N current rows: the K indices and the K x 2 template in (one copy), the fit, the warp, the matrices and flags out
 * (one copy), the crops out when out is host memory (out_on_device 0), one stream synchronise.  out: N x out_height x out_width x C
 * bytes, C the source's channels; matrices_host (N x 6: M00 M01 M02 M10 M11 M12) and flags_host (N) may be NULL.  Neither the
 * landmark state, the images nor the tracker's slots are changed. */
int sdm_align_crops(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int out_width, int out_height,
                    uint8_t* out, int out_on_device, float* matrices_host, int* flags_host);

/* Crops as a network's input tensor, straight from frames on the device: one launch behind the fit goes from the frames in place to
 * N x C x H x W (or N x H x W x C) elements of u8, float16 or float32, channel order, mean and std applied.
 *
 * sdm_align_set_source_frames: a frame list as the crop source, used IN PLACE (nothing copied, nothing converted; the memory must stay
 * valid while crops are made from it).  frames: as for sdm_set_frames_device, every format.  chroma: NULL, or n_frames pointers;
 * entry i is the SECOND PLANE of frame i -- the interleaved UV plane of an NV12 frame, plane 1 of a planar colour frame ("Planar colour
 * frames": its plane distance is that address minus data) --, ignored for other formats; a NULL entry, or chroma == NULL, means
 * (const uint8_t*)data + (size_t)height * stride_bytes.  The UV plane has (height + 1) / 2 rows of stride_bytes.
 * n_frames == 0 / frames == NULL: back to the context's images.  Replaces an sdm_align_set_source stack and is replaced by one.
 * Refused (SDM_ERR_INVALID, no state changed): what sdm_set_frames_device refuses of a frame (n_frames < 0, a NULL data pointer, width or
 * height < 1, stride_bytes < width * bytes per pixel, an unknown format), and an NV12 frame with stride_bytes < 2 * ((width + 1) / 2).
 *
 * sdm_align_crops_tensor, for every current row n (rows map to images / frames through sdm_set_sample_image_index; a frame must have the
 * width and height of the context image its row maps to):
 *   1. fit, positions, quantisation, weights, flags   sdm_align_crops', unchanged: the same fit kernel, sx = (M00 j + M01 i) + M02, 1/32-pixel
 *      positions, (... + 512) >> 10, a tap outside the image reads 0, the 2^20 rule, DEGENERATE, PARTIAL.
 *   2. warped pixel by source format
 *        GRAY                      one value g
 *        BGR / RGB / BGRA / RGBA   three values (B, G, R) by byte position; alpha is never read
 *        NV12   Y = the gray warp of the Y plane (sdm_align_crops' bits on that luma).  U, V: warped from the UV plane of
 *               cw = (w + 1) >> 1 by ch = (h + 1) >> 1 byte pairs at cx = sx * 0.5f, cy = sy * 0.5f (exact; chroma co-sited with the even
 *               luma sample), same quantisation and weights; a chroma tap outside [0, cw) x [0, ch) reads 128.  Then BT.601 limited
 *               range in int32, the constants of OpenCV's COLOR_YUV2BGR_NV12: y = max(0, Y - 16) * 1220542,
 *               R = (y + 1673527 (V - 128) + 2^19) >> 20, G = (y - 852492 (V - 128) - 409993 (U - 128) + 2^19) >> 20,
 *               B = (y + 2116026 (U - 128) + 2^19) >> 20, arithmetic shift, clamped to [0, 255].  A position refused by the 2^20 rule
 *               gives (0, 0, 0).
 *        The source is the frame list, else the sdm_align_set_source stack (C = 1: GRAY, 3: BGR, 4: BGRA), else the context's images (GRAY).
 *   3. output channels   channels == 3: a gray source replicates g; a colour source gives (B, G, R) or (R, G, B) by `order`.
 *        channels == 1: a gray source gives g; an NV12 source gives Y as it is (no conversion, the UV plane is not read); the other
 *        colour formats give (B wb + G wg + R wr + (1 << (gray_shift - 1))) >> gray_shift with sdm_upload_images_bgr_u8's weights
 *        (14: 1868, 9617, 4899; 15: 3735, 19235, 9798), applied to the warped values.
 *   4. element   U8: the value v.  F32: (float)v * scale[c] + bias[c], the product rounded, then the sum rounded.  F16: that float32
 *        converted round-to-nearest-even.  c is the OUTPUT channel.
 *   5. layout   NHWC: out[((n H + i) W + j) C + c].  NCHW: out[((n C + c) H + i) W + j].
 *   6. a DEGENERATE row's elements are those of v = 0 (bias[c] for the float dtypes); its M is six NaNs.
 *   7. refused (SDM_ERR_INVALID, no state changed, nothing launched): everything sdm_align_crops refuses; spec NULL; an unknown dtype,
 *      layout or order; channels not 1 or 3; gray_shift not 14 or 15; a non-finite scale or bias with a float dtype; out_dev NULL or not
 *      16-byte aligned.
 * sdm_align_crops on a frame-list source: frames of ONE pixel size (all GRAY, all 3-byte or all 4-byte) give the interleaved warp as for a
 * stack, alpha included; NV12 or mixed pixel sizes are refused (use sdm_align_crops_tensor). */
int sdm_align_set_source_frames(sdm_ctx* ctx, const sdm_frame* frames, const void* const* chroma, int n_frames);

#define SDM_ALIGN_U8         0   /* dtype                                    */
#define SDM_ALIGN_F16        1
#define SDM_ALIGN_F32        2
#define SDM_ALIGN_NHWC       0   /* layout                                   */
#define SDM_ALIGN_NCHW       1
#define SDM_ALIGN_ORDER_BGR  0   /* order of a 3-channel output              */
#define SDM_ALIGN_ORDER_RGB  1
typedef struct sdm_align_tensor {
    int dtype, layout, channels /* 1 or 3 */, order;
    float scale[3], bias[3];      /* float dtypes, per OUTPUT channel; ignored for U8 */
    int gray_shift;               /* 14 | 15: the weights of a colour -> 1 channel output */
} sdm_align_tensor;
/* out_dev: device memory, N * channels * out_height * out_width elements, 16-byte aligned. */
int sdm_align_crops_tensor(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int out_width,
                           int out_height, const sdm_align_tensor* spec, void* out_dev, float* matrices_host, int* flags_host);

/* sdm_align_crops_tensor with area-averaged sampling where a row's similarity minifies: a face 300 to 1000 pixels wide in a 112-pixel crop
 * puts 3 to 9 source pixels under every crop pixel, of which four bilinear taps see a fraction.  Here every output pixel of such a row is
 * the average of S x S bilinear sub-samples spread over its footprint, S chosen per row from the fitted scale, all in the integer arithmetic
 * of the crop path.  One launch for all rows behind the fit kernel; rows with S = 1 run sdm_align_crops_tensor's code and give its bits.
 *   1. unchanged from sdm_align_crops_tensor: the fit, M, the flags (PARTIAL is still judged on the corner pixel CENTRES), the source
 *      rules, the channel, element and layout rules (its items 3 to 6) and its refusals.  Refused in addition: filter NULL, an unknown
 *      mode, max_samples outside [1, 16], min_scale not finite or below 1.  Every refusal returns SDM_ERR_INVALID, changes no state and
 *      launches nothing.
 *   2. S of row n   s2 = M00 M00 + M10 M10 in float32, each operation rounded, nothing contracted.  S = 1 for mode BILINEAR, for
 *      s2 < min_scale * min_scale (float32), for a non-finite s2 and for a DEGENERATE row; otherwise the smallest integer in
 *      [1, max_samples] with (float)(S S) >= s2, and max_samples when there is none.  samples_host[n] = S.
 *   3. sub-sample positions   for u, v in 0 ... S - 1: fj = (float)j + o[u], fi = (float)i + o[v] with o[u] = (float)(2u + 1 - S) /
 *      (float)(2S), a correctly rounded float32 division; then sx = (M00 fj + M01 fi) + M02 and sy likewise: sdm_align_crops' expression
 *      at a fractional (j, i).  S = 1: o = 0, the position of sdm_align_crops.
 *   4. sub-sample value   sdm_align_crops' quantisation to 1/32 pixel, taps and weights, without the final rounding: per byte position
 *      q = w00 p00 + w10 p10 + w01 p01 + w11 p11 <= 255 * 1024.  A tap outside the image reads 0, an NV12 chroma tap outside reads 128.
 *   5. pixel value   v = (sum of q over the S S sub-samples + 512 S S) / (1024 S S), an unsigned integer division; the sum stays below
 *      2^26 + 2^17.  S = 1: (q + 512) >> 10.  If any sub-sample of the pixel is refused by the 2^20 rule the pixel is 0 -- (0, 0, 0) for
 *      NV12 with three output channels.
 *   6. NV12   Y is averaged as in 5; U and V the same way over the same S S sub-samples at cx = sx * 0.5f, cy = sy * 0.5f; the BT.601
 *      conversion is applied once, to the averaged (Y, U, V).  channels == 1 gives the averaged Y as it is, and the UV plane is not read.
 *   7. a colour source to one channel: the gray weights apply to the averaged (B, G, R).
 * samples_host (N) may be NULL; it comes back with the matrices and flags in the same copy. */
#define SDM_ALIGN_FILTER_BILINEAR  0   /* mode                                     */
#define SDM_ALIGN_FILTER_AREA      1
typedef struct sdm_align_filter {
    int   mode;         /* SDM_ALIGN_FILTER_*                                                         */
    int   max_samples;  /* cap on S, the sub-samples per axis: 1 .. 16                                */
    float min_scale;    /* finite, >= 1: rows whose scale^2 < min_scale * min_scale (float32) take S = 1 */
} sdm_align_filter;
int sdm_align_crops_tensor_filtered(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int out_width,
                                    int out_height, const sdm_align_tensor* spec, const sdm_align_filter* filter, void* out_dev,
                                    float* matrices_host, int* flags_host, int* samples_host);

/* Warped faces: the piecewise-affine warp of every current row onto a template shape (the shape-normalised texture of AAM / CLNF
 * pipelines).  The crops above are rigid: one similarity per face, so the landmarks still sit somewhere else in every crop.  Here the
 * template is triangulated over K landmarks and every triangle carries its own affine map, so that every landmark lands on its template
 * point.  Two launches for all rows (the triangles' matrices, the pixels), written as sdm_align_crops_tensor writes its tensor.
 *   mesh     K landmark indices, K template points q_k (crop pixel coordinates, float32), T triangles -- triples (a, b, c) of positions
 *            0 .. K - 1 --, an output size out_width x out_height.  Triangles may overlap, and need not cover the template's hull.
 *   D        of a triangle, in double on the float32 template points, every operation rounded, nothing contracted (this holds for every
 *            expression of this block): u = q_b - q_a, v = q_c - q_a, D = u.x v.y - u.y v.x.  A triangle with D > 0 is called
 *            counter-clockwise here (image coordinates: x right, y down).
 *   labels   out_height x out_width bytes, a function of the mesh alone; the host computes them once, in sdm_warp_set_mesh.  A triangle
 *            with D < 0 has b and c exchanged first (for the labels only).  With x = (double)j, y = (double)i the edge functions are
 *              e0 = (b.x - a.x) (y - a.y) - (b.y - a.y) (x - a.x)
 *              e1 = (c.x - b.x) (y - b.y) - (c.y - b.y) (x - b.x)
 *              e2 = (a.x - c.x) (y - c.y) - (a.y - c.y) (x - c.x)
 *            (two differences, two products, one difference each) and pixel (column j, row i) takes the lowest-numbered triangle t with
 *            e0 >= 0, e1 >= 0 and e2 >= 0 -- also on an edge two triangles share --, or 255 when there is none.
 *   G        per triangle, on the host: G00 = v.y / D, G01 = -v.x / D, G10 = -u.y / D, G11 = u.x / D; q_a is kept beside it.
 *   A_t      per row n and triangle t, from the row's landmarks p_k = (x[idx_k], x[L + idx_k]), in double:
 *              E00 = p_b.x - p_a.x, E01 = p_c.x - p_a.x, E10 = p_b.y - p_a.y, E11 = p_c.y - p_a.y
 *              L_rc = E_r0 G_0c + E_r1 G_1c                    (both products and the sum rounded)
 *              t_r  = p_a[r] - (L_r0 q_a.x + L_r1 q_a.y)       (both products, the sum and the difference rounded)
 *            A_t = (L00, L01, t_0, L10, L11, t_1), each rounded once to float32: M00 M01 M02 M10 M11 M12 of sdm_align_crops, crop -> source.
 *   pixel    (column j, row i) with label t: sx = (A_t00 j + A_t01 i) + A_t02, sy = (A_t10 j + A_t11 i) + A_t12 in float32, every operation
 *            rounded; from that position on it is items 1 to 5 of sdm_align_crops_tensor, unchanged: the 1/32-pixel quantisation, the taps,
 *            the weights, (... + 512) >> 10, the 2^20 rule, the source formats, the channel rules, the element, the layout.  A pixel with
 *            label 255 takes the elements of v = 0 (bias[c] for the float dtypes) and reads no source byte.  Sampling is plain bilinear
 *            here; sdm_warp_crops_tensor_filtered below is this call with the area filter, per triangle and per axis.
 *   flags    per row:
 *            SDM_WARP_DEGENERATE  one of the mesh's K landmarks is not finite: every element is that of v = 0, every matrix of the row is
 *                                 six NaNs, and no other bit is evaluated.
 *            SDM_WARP_PARTIAL     one of the K landmarks lies outside [0, W - 1] x [0, H - 1] of the row's image, compared in float32
 *                                 (informational).
 *            SDM_WARP_FOLDED      for some triangle det(E) = E00 E11 - E01 E10 (double, each operation rounded) is 0 or has the sign
 *                                 opposite to D's: the fitted shape folds over there (informational; the pixels follow the formula).
 *   source   what sdm_align_crops_tensor reads: the sdm_align_set_source_frames list, else the sdm_align_set_source stack, else the
 *            context's images; the same row -> image mapping and the same size rule.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched -- sdm_warp_set_mesh: no geometry, K outside [3, L], an index out of
 * range or repeated, a template point that is not finite, T outside [1, 254], a triangle position outside 0 .. K - 1 or repeated within
 * its triangle, D == 0 or not finite, out_width or out_height outside [1, 1024].  sdm_warp_crops_tensor: no mesh (none set, or
 * sdm_set_model_geometry has changed L since), no current rows, and everything sdm_align_crops_tensor refuses of spec, out_dev and the source.
 * The mesh stays in the context until the next sdm_warp_set_mesh or sdm_destroy. */
#define SDM_WARP_DEGENERATE 1
#define SDM_WARP_PARTIAL 2
#define SDM_WARP_FOLDED 4
#define SDM_WARP_NO_TRIANGLE 255   /* label of a pixel no triangle covers */
/* The Delaunay triangulation of K points (xy: K x 2 float32), host only, no context: the default mesh of the layers above.  triangles
 * receives n_triangles triples of point positions, every one counter-clockwise (D > 0) -- none has zero area.  The same input always gives
 * the same output; of cocircular points any valid choice may come out (an in-circle determinant within 1e-12 of its terms' magnitude
 * counts as zero).  SDM_ERR_INVALID: K < 3 or > 255, a point not finite or given twice, all points on one line, capacity (in triangles;
 * 2K - 5 always suffice) too small. */
int sdm_warp_delaunay(const float* xy, int K, int* triangles, int capacity, int* n_triangles);
int sdm_warp_set_mesh(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, const int* triangles, int T,
                      int out_width, int out_height);
/* the label map of the mesh: out_height x out_width bytes, dense (SDM_ERR_INVALID without a mesh) */
int sdm_warp_get_labels(sdm_ctx* ctx, uint8_t* labels_host);
/* One call for all N current rows.  out_dev: device memory, N * channels * out_height * out_width elements, 16-byte aligned;
 * matrices_host (N x T x 6) and flags_host (N) may be NULL; they come back in one copy, behind one synchronise.  Neither the landmark
 * state, the images, the crop source nor the tracker's slots are changed. */
int sdm_warp_crops_tensor(sdm_ctx* ctx, const sdm_align_tensor* spec, void* out_dev, float* matrices_host, int* flags_host);

/* Warped faces, filtered: sdm_warp_crops_tensor with area-averaged sampling where a triangle's map minifies.  Every triangle has its own
 * affine map: a turned head minifies the near cheek while the far cheek magnifies, and the maps shear, so the sub-sample count is chosen
 * per TRIANGLE and per AXIS.  Every pixel of triangle t is the average of Sx x Sy bilinear sub-samples spread over its footprint, in the
 * integer arithmetic of the crop path, in the same two launches; the filter is sdm_align_crops_tensor_filtered's sdm_align_filter.
 *   1. unchanged from sdm_warp_crops_tensor: the mesh and the label map, G, A_t and its rounding to float32, the flags, the source rules,
 *      the channel, element and layout rules and every refusal.  Refused in addition what sdm_align_crops_tensor_filtered refuses of
 *      filter: NULL, an unknown mode, max_samples outside [1, 16], min_scale not finite or below 1.  Every refusal returns SDM_ERR_INVALID,
 *      changes no state and launches nothing.
 *   2. (Sx, Sy) of row n, triangle t   from the float32 A_t, in float32, each operation rounded, nothing contracted:
 *      cx2 = A00 A00 + A10 A10 (the source step per crop column, squared), cy2 = A01 A01 + A11 A11 (per crop row).  Sx is item 2 of
 *      sdm_align_crops_tensor_filtered applied to cx2, Sy the same rule applied to cy2: 1 for mode BILINEAR, for a DEGENERATE row, for a
 *      value that is not finite or below min_scale * min_scale (float32); otherwise the smallest integer in [1, max_samples] with
 *      (float)(S S) >= value, and max_samples when there is none.  For a similarity Sx = Sy = the rigid call's S.  A FOLDED triangle
 *      follows the formula like any other.  samples_host[(n T + t) 2] = Sx, [(n T + t) 2 + 1] = Sy.
 *   3. sub-samples of pixel (j, i) with label t   all go through the pixel's own A_t, also those whose crop position lies past the
 *      triangle's edge or in unlabelled territory.  For u in 0 ... Sx - 1 and v in 0 ... Sy - 1: fj = (float)j + o_Sx[u],
 *      fi = (float)i + o_Sy[v] with o_S[u] = (float)(2u + 1 - S) / (float)(2S), correctly rounded (the rigid call's offsets); then
 *      sx = (A00 fj + A01 fi) + A02 and sy likewise.
 *   4. value   items 4 to 7 of sdm_align_crops_tensor_filtered with S S replaced by n = Sx Sy <= 256: the sub-samples are un-rounded tap
 *      sums q, v = (sum of q + 512 n) / (1024 n), an unsigned integer division, the sum below 2^26 + 2^17; a pixel with any sub-sample
 *      refused by the 2^20 rule is 0; NV12 averages Y, U and V over the same sub-samples and converts once (channels == 1: the averaged Y,
 *      the UV plane is not read); the gray weights apply to the averaged (B, G, R).
 *   5. a pixel with label 255 takes the elements of v = 0 and reads no source byte, as in sdm_warp_crops_tensor.
 *   6. bit identity   a pixel whose triangle has Sx = Sy = 1 takes exactly the bits sdm_warp_crops_tensor gives it; mode BILINEAR gives
 *      the unfiltered tensor for any rows.
 * Two consequences, both chosen for simplicity and determinism: the MAP is continuous across an edge two triangles share, the sample
 * count is not -- two neighbouring triangles may average over different grids --; and A_t extrapolates up to half a crop pixel past its
 * triangle for the sub-samples of the triangle's border pixels.
 * samples_host (N x T x 2) may be NULL; it comes back with the matrices and flags in the same single copy and synchronise.  The paste
 * direction has the same filter, on W_t: sdm_warp_paste_tensor_filtered ("Pasting warped faces back, filtered"). */
int sdm_warp_crops_tensor_filtered(sdm_ctx* ctx, const sdm_align_tensor* spec, const sdm_align_filter* filter, void* out_dev,
                                   float* matrices_host /* N x T x 6 */, int* flags_host /* N */,
                                   int* samples_host /* N x T x 2: (Sx, Sy) of every triangle; may be NULL */);

/* Pasting crops back: the inverse path of sdm_align_crops_tensor.  A network's output y = net(x) on the crops x -- a restored, swapped,
 * re-lit, blurred or pixelated face -- is warped back through the row's similarity and blended into the frames where they lie on the
 * device, in place, in one launch behind the fit for all rows, in the integer arithmetic of the crop path.  Every float operation is
 * rounded on its own, nothing is contracted.
 *   destination   dst_frames[i].data is WRITTEN in place: the const of sdm_frame, the read-only view of the crop calls, is cast away
 *           here.  Formats GRAY, BGR, RGB, BGRA, RGBA; any pointer alignment, any stride_bytes >= width * bytes per pixel; every offset
 *           is 64-bit.  Row n maps to a frame through sdm_set_sample_image_index (sdm_align_paste_tensor) or image_index
 *           (sdm_align_paste_tensor_at; NULL: row i -> frame i).  In the fit form a frame must have the width and height of the context
 *           image its row maps to (sdm_align_crops_tensor's rule for a frame-list source).  The frames may be the very memory the
 *           context's images or the crop source read in place: that is the caller's business.  in_dev or an opacity map overlapping a
 *           destination frame, and two frame entries that alias each other, are undefined.
 *   M, W    M (crop -> frame) is the fit of sdm_align_crops -- the same kernel, the same M, the same flags -- or row n of matrices_host.
 *           Its inverse W (frame -> crop) is computed from the float32 M in double: d = M00 M11 - M01 M10, W00 = M11 / d, W01 = -M01 / d,
 *           W10 = -M10 / d, W11 = M00 / d, W02 = -(W00 M02 + W01 M12), W12 = -(W10 M02 + W11 M12), each of the six rounded once to
 *           float32.
 *   flags   SDM_ALIGN_DEGENERATE -- the row pastes nothing --: the fit flags it DEGENERATE, an entry of M is not finite, d == 0, or an
 *           entry of W is not finite.  SDM_ALIGN_PARTIAL: the fit's rule on M (a crop corner's pixel centre maps outside
 *           [0, W - 1] x [0, H - 1] of the frame); the _at form evaluates the same rule from M and the frame's size.  Beside an M that
 *           is not finite no other bit is evaluated, as in the fit.
 *   position   frame pixel (column X, row Y), in float32: u = (W00 X + W01 Y) + W02, v = (W10 X + W11 Y) + W12;
 *           U = floor(u * 32 + 0.5f), u0 = U >> 5, fu = U & 31, v the same: sdm_align_crops' quantisation and its four weights out of
 *           1024.  The pixel is IN THE FOOTPRINT of row n when u and v are finite, |u|, |v| <= 2^20, -1 <= u0 <= crop_width - 1 and
 *           -1 <= v0 <= crop_height - 1: at least one tap lies in the crop.
 *   tap     the tensor element of output channel c at (column, row), both clamped into the crop, decoded by dtype.  U8: the byte.
 *           F32: f = e * scale[c] + bias[c], the product rounded, then the sum rounded; F16: converted exactly to float32 first.  Then
 *           p = 0 for a NaN, else rintf(min(max(f, 0), 255)), ties to even.  scale / bias are therefore the INVERSE of the crop call's:
 *           scale = std, bias = mean in 0-255 units.  channels == 3: `order` says which tensor channel is B, G or R; channels == 1: the
 *           one value serves all three.  Layouts as in sdm_align_crops_tensor.
 *   colour  per B, G and R: q = (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10.
 *   opacity the same four weights on the row's opacity map (sdm_align_paste: crop_height x crop_width bytes, one map for all rows or
 *           row n's at n * H * W); a tap outside the crop reads 0; with alpha_dev NULL a tap inside reads 255; a = (... + 512) >> 10.
 *           The crop's border therefore fades over one pixel by itself; a caller's feathered map fades wider.
 *   write   a == 0: no byte of the pixel is written.  Otherwise per destination byte with the old value o:
 *           o' = (a q + (255 - a) o + 127) / 255, an unsigned integer division.  BGR / BGRA: bytes 0, 1, 2 take B, G, R; RGB / RGBA the
 *           reverse; GRAY: from a 3-channel tensor (B wb + G wg + R wr + (1 << (gray_shift - 1))) >> gray_shift of the sampled q with
 *           sdm_upload_images_bgr_u8's weights, from a 1-channel tensor q.  The alpha byte of BGRA / RGBA is neither read nor written:
 *           three bytes are stored.
 *   several rows on one frame   the result is that of pasting the rows one after another in increasing row number, each reading what the
 *           previous one left, whatever the launch order: a pixel is loaded once, every row whose footprint holds it is applied in
 *           registers in row order, and it is stored once.
 *   never stored to, not even with their old value: pitch padding, pixels outside every footprint, pixels whose every a is 0, alpha bytes.
 * NV12 destinations are refused here and taken by sdm_align_paste_tensor_nv12 / _at_nv12 ("Pasting crops back into NV12 frames"
 * below).  These two calls are plain bilinear, as sdm_align_crops is; the
 * antialiasing for a face that is smaller in the frame than in the crop is the filtered form, "Pasting crops back, filtered" below.
 * (The inverse of sdm_warp_crops_tensor is "Pasting warped faces back".)
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: what sdm_align_crops_tensor refuses of landmark_index, template_xy,
 * K, the crop size, spec and the rows' source (fit form); in_dev NULL or not 16-byte aligned; paste NULL; alpha_per_row not 0 or 1;
 * dst_frames NULL or n_frames < 1; what sdm_set_frames_device refuses of a frame; an NV12 frame; a row whose image index is outside
 * [0, n_frames); the size mismatch above; _at form: matrices_host NULL, n_rows < 1, crop_width or crop_height outside [1, 1024]. */
typedef struct sdm_align_paste {
    const uint8_t* alpha_dev;   /* crop-space opacity, u8, device memory; NULL: 255 everywhere inside the crop      */
    int alpha_per_row;          /* 0: one crop_height x crop_width map for all rows; 1: N maps, row n at n * H * W  */
} sdm_align_paste;
/* the current rows: the fit of sdm_align_crops (same kernel, same M, same flags), then the paste.  in_dev: N * channels * crop_height *
 * crop_width elements.  matrices_host (N x 6) and flags_host (N) may be NULL; they come back in one copy behind the call's one
 * synchronise. */
int sdm_align_paste_tensor(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int crop_width, int crop_height,
                           const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste,
                           const sdm_frame* dst_frames, int n_frames, float* matrices_host /* out, N x 6, may be NULL */,
                           int* flags_host /* out, may be NULL */);
/* explicit crop -> frame matrices (what an earlier crop call returned): no landmark state, no geometry, no context images needed -- the
 * network may run on frame t while the tracker has stepped to t + 1 */
int sdm_align_paste_tensor_at(sdm_ctx* ctx, const float* matrices_host /* in, n_rows x 6 */, const int* image_index /* NULL: row i -> frame i */,
                              int n_rows, int crop_width, int crop_height, const sdm_align_tensor* spec, const void* in_dev,
                              const sdm_align_paste* paste, const sdm_frame* dst_frames, int n_frames, int* flags_host);

/* Pasting crops back, filtered: sdm_align_paste_tensor and sdm_align_paste_tensor_at with area-averaged sampling where the crop outsizes
 * the face.  A network that runs at 256 or 512 pixels on a face 60 to 200 pixels wide in the frame puts 9 to 64 tensor elements under
 * every frame pixel, of which four bilinear taps see a fraction: fine texture aliases and shimmers from frame to frame.  Here every frame
 * pixel of such a row takes the average of S x S bilinear sub-samples spread over its footprint in the crop, S chosen per row from W, in
 * the integer arithmetic of the paste; the average is taken BEFORE the blend, of colour and opacity alike.  One launch for all rows
 * behind the prepare stage.  Every rule of "Pasting crops back" that is not restated here holds word for word: M, W, the flags, the
 * decode, the clamped colour taps, opacity 0 outside the crop, the / 255 blend, per-byte stores, the alpha byte never touched, the rows
 * of one frame applied in increasing row number.  NV12 destinations are refused here too (they go through sdm_align_paste_tensor_nv12
 * with this filter, "Pasting crops back into NV12 frames" below); the piecewise-affine paste has its own filtered form, per triangle
 * and per axis ("Pasting warped faces back, filtered").  Every float operation is rounded on its own, nothing is contracted.
 *   S of row n   s2 = W00 W00 + W10 W10 in float32 on the float32 W, each operation rounded: the mirror image of
 *           sdm_align_crops_tensor_filtered, which takes it from M.  S = 1 for mode BILINEAR, for s2 < min_scale * min_scale (float32),
 *           for a non-finite s2 and for a DEGENERATE row; otherwise the smallest integer in [1, max_samples] with (float)(S S) >= s2, and
 *           max_samples when there is none.  samples_host[n] = S.
 *   sub-samples of frame pixel (X, Y), S > 1   for u, v in 0 ... S - 1: fX = (float)X + o[u], fY = (float)Y + o[v], with
 *           o[u] = (float)(2u + 1 - S) / (float)(2S) as in sdm_align_crops_tensor_filtered; the position is (W00 fX + W01 fY) + W02 and
 *           (W10 fX + W11 fY) + W12, quantised as in "Pasting crops back" (2^20 rule, 1/32 pixel).  Per sub-sample the UNROUNDED sums:
 *           per channel w00 p00 + w10 p10 + w01 p01 + w11 p11 with the taps clamped into the crop, and the same weights on the opacity,
 *           where a tap outside the crop reads 0 and, with alpha_dev NULL, a tap inside reads 255.
 *   pixel   q_c = (sum over the S S sub-samples + 512 S S) / (1024 S S) per channel, a the same from the opacity sums: unsigned integer
 *           divisions; the sums stay below 2^26 + 2^17.  Channel order, the gray weights and the blend apply to the averaged q and a
 *           exactly as they do at S = 1.
 *   not touched by a row   a pixel of which any sub-sample is refused by the 2^20 rule; a pixel with a == 0: no byte is written.
 *   result and footprint   the RESULT is the formula above evaluated over the whole frame, row after row.  The kernel's working
 *           footprint of a row with S > 1 is one predicate, used alike for "an earlier row owns this pixel" and "this row is applied
 *           here": the pixel lies in the row's box -- the box of the unfiltered paste one frame pixel wider on each side, |o| < 1/2; an empty box stays empty --
 *           and the float32 position (u, v) of its CENTRE (the expression of "Pasting crops back") satisfies
 *           -1 - du <= u <= crop_width + du and -1 - dv <= v <= crop_height + dv, with du = (|W00| + |W01|) / 2 + 2^-20 mag_u + 9/32,
 *           mag_u = |W00| (width + 1) + |W01| (height + 1) + |W02| (double, rounded once to float32), dv and mag_v the same on the
 *           second row of W.  With mag_u or mag_v >= 2^20, or du or dv >= 2^15, the box alone decides.  The predicate holds every pixel
 *           for which the formula gives a != 0; pixels it holds beyond those get a == 0 and are not written.
 *   S = 1   such a row gives the bits of the unfiltered call, through its footprint and its code.  Rows of different S on one frame
 *           overlap and are applied in row order.  With mode BILINEAR the call writes exactly the bytes of the unfiltered one.
 * Refused in addition to what the unfiltered calls refuse (SDM_ERR_INVALID, no state changed, nothing launched): filter NULL, an unknown
 * mode, max_samples outside [1, 16], min_scale not finite or below 1.  samples_host (one int per row) may be NULL; S comes back in the
 * same copy as the flags. */
int sdm_align_paste_tensor_filtered(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int crop_width,
                                    int crop_height, const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                    const sdm_align_paste* paste, const sdm_frame* dst_frames, int n_frames,
                                    float* matrices_host /* out, N x 6, may be NULL */, int* flags_host /* out, may be NULL */,
                                    int* samples_host /* out, may be NULL */);
int sdm_align_paste_tensor_at_filtered(sdm_ctx* ctx, const float* matrices_host /* in, n_rows x 6 */,
                                       const int* image_index /* NULL: row i -> frame i */, int n_rows, int crop_width, int crop_height,
                                       const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                       const sdm_align_paste* paste, const sdm_frame* dst_frames, int n_frames, int* flags_host,
                                       int* samples_host);

/* Pasting crops back into NV12 frames: sdm_align_paste_tensor[_filtered] and sdm_align_paste_tensor_at[_filtered] for a list of
 * destinations that may hold NV12 frames -- what a hardware decoder delivers and a hardware encoder takes, and what
 * sdm_align_crops_tensor reads in place.  Luma and 4:2:0 chroma are blended where they lie; no plane is converted, nothing outside the
 * faces is re-quantised.  One launch for all rows behind the prepare stage.  Every rule of "Pasting crops back" and "Pasting crops back,
 * filtered" that is not restated here holds word for word.  filter NULL: plain bilinear, S = 1 for every row.
 *   destination   sdm_frame with format SDM_FRAME_NV12: data is the Y plane, height rows of stride_bytes, written in place.  The UV plane
 *           is dst_chroma[i]; with a NULL entry, or dst_chroma == NULL, it is (uint8_t*)data + (size_t)height * stride_bytes, as in
 *           sdm_align_set_source_frames.  It has (height + 1) / 2 rows of stride_bytes and (width + 1) / 2 (U, V) byte pairs per row.
 *           Any pointer alignment; every offset is 64-bit.  The other five formats are accepted in the same list -- a BGR camera and a
 *           decoder surface in one step -- and get exactly the bytes of the calls above, through their per-pixel code; their
 *           dst_chroma entry is ignored.
 *   per luma pixel   (q_B, q_G, q_R) and a are exactly those of the unfiltered paste, or of the filtered paste averaged over S x S
 *           sub-samples: the footprint, the 2^20 rule, S per row and the working footprint are the same.
 *   luma    3-channel tensor: Yq = (269484 q_R + 528482 q_G + 102760 q_B + (16 << 20) + (1 << 19)) >> 20.  1-channel tensor: Yq = q, no
 *           conversion (the mirror of the crop call, which hands out Y as it is for channels == 1), and the UV plane is neither read nor
 *           written.  Y' = (a Yq + (255 - a) Y + 127) / 255; a == 0: the byte is not written.
 *   chroma  3-channel tensor.  Sample (cx, cy) belongs to the pixels X in {2 cx, 2 cx + 1}, Y in {2 cy, 2 cy + 1} that lie inside the
 *           frame; cnt in {4, 2, 1} counts them.  For row n: A = sum of a_i over those pixels, a pixel outside the row's footprint having
 *           a_i = 0.  A == 0: the row leaves the sample alone.  Otherwise per B, G and R: m = (sum of a_i q_i + A / 2) / A, an unsigned
 *           division -- an opacity-weighted mean, so that a half-covered block takes the colour of its covered pixels.  In int32 with an
 *           arithmetic shift, clamped to [0, 255]:
 *               Uq = (460324 m_B - 305135 m_G - 155188 m_R + (128 << 20) + (1 << 19)) >> 20
 *               Vq = (460324 m_R - 385875 m_G -  74448 m_B + (128 << 20) + (1 << 19)) >> 20
 *           a_c = (A + cnt / 2) / cnt.  a_c == 0: neither byte is written.  Otherwise U and V are blended with a_c by the / 255 formula.
 *           The Q20 constants are BT.601 limited range (0.257, 0.504, 0.098; 0.439, 0.291, 0.148; 0.368, 0.071), the counterpart of the
 *           crop call's decode constants; the numbers above are the definition.
 *   several rows on one frame   the result is that of pasting the rows one after another in increasing row number, each reading the luma
 *           and the chroma the previous one left.  On an NV12 frame the unit of ownership is the 2 x 2 block: it is loaded once (up to
 *           four Y bytes, one UV pair) by the lowest-numbered row of the frame whose footprint holds one of its pixels, every row from
 *           that one on is applied in registers in row order, and every changed byte is stored once.
 *   never stored to, not even with their old value: pitch padding of either plane; luma pixels whose every a is 0, even in a block whose
 *           chroma is written; chroma samples whose every a_c is 0; the UV plane for a 1-channel tensor.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: everything the filtered calls refuse, except that an NV12 frame and a
 * NULL filter are accepted; an NV12 frame with stride_bytes < 2 * ((width + 1) / 2).  The fit form's size rule holds against the context
 * image (an NV12 frame set through sdm_set_frames_device is its own luma).  samples_host may be NULL.  The piecewise-affine paste
 * has its NV12 form in sdm_warp_paste_tensor_nv12 / _at_nv12 ("Pasting warped faces back into NV12 frames"). */
int sdm_align_paste_tensor_nv12(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int crop_width, int crop_height,
                                const sdm_align_tensor* spec, const sdm_align_filter* filter /* NULL: plain bilinear */, const void* in_dev,
                                const sdm_align_paste* paste, const sdm_frame* dst_frames,
                                void* const* dst_chroma /* n_frames second planes (NV12: UV, planar: plane 1); NULL, or a NULL entry: behind the first plane */, int n_frames,
                                float* matrices_host /* out, N x 6, may be NULL */, int* flags_host /* out, may be NULL */,
                                int* samples_host /* out, may be NULL */);
int sdm_align_paste_tensor_at_nv12(sdm_ctx* ctx, const float* matrices_host /* in, n_rows x 6 */,
                                   const int* image_index /* NULL: row i -> frame i */, int n_rows, int crop_width, int crop_height,
                                   const sdm_align_tensor* spec, const sdm_align_filter* filter /* NULL: plain bilinear */,
                                   const void* in_dev, const sdm_align_paste* paste, const sdm_frame* dst_frames, void* const* dst_chroma,
                                   int n_frames, int* flags_host, int* samples_host);

/* Pasting warped faces back: the inverse path of sdm_warp_crops_tensor.  A network's output in template space -- a transferred
 * expression, a swapped, re-lit or de-aged texture -- is warped back under the face's own shape, triangle by triangle, and blended into
 * the frames in place: the fit of sdm_warp_crops_tensor, one launch per (row, triangle), one launch for the pixels.  Both forms use the
 * mesh of sdm_warp_set_mesh; the crop is its out_width x out_height.  in_dev, spec, paste and dst_frames mean exactly what they mean for
 * sdm_align_paste_tensor (formats, alignment, pitch, 64-bit offsets, NV12 refused, scale / bias the inverse of the crop call's, the size
 * rule of the fit form, the alpha byte never touched).  Every expression is evaluated as written: double on the float32 inputs where
 * marked, each operation rounded on its own, nothing contracted.
 *   points  p_k, the row's K mesh landmarks as float32: (x[idx_k], x[L + idx_k]) of the current rows (sdm_warp_paste_tensor) or row n of
 *           points_host (sdm_warp_paste_tensor_at).  A_t per triangle is that of "Warped faces": the same code on the same points gives
 *           the same bits in both forms.
 *   flags   the SDM_WARP_* bits.  DEGENERATE: a mesh landmark is not finite; the row pastes nothing and no other bit is evaluated.
 *           PARTIAL: the warp's rule against the destination frame's width and height.  FOLDED: the warp's rule.
 *   box     x0 = floor(min_k p_k.x), x1 = ceil(max_k p_k.x) + 1, y the same, formed in double and clipped to the frame before any
 *           conversion to int.  A pixel outside [x0, x1) x [y0, y1) is outside the row's footprint.
 *   triangle   of frame pixel (column X, row Y).  Per triangle, in double: det E = E00 E11 - E01 E10 (the FOLDED rule's expression).
 *           det E == 0: the triangle covers nothing.  det E < 0: b and c are exchanged, for the edge functions only.  The edge functions
 *           are e0, e1, e2 of the label map with p_a, p_b, p_c in place of the template points and x = (double)X, y = (double)Y.  W_t is
 *           the inverse of the float32 A_t by the formula of "Pasting crops back" (double, each of the six entries rounded once to
 *           float32); a triangle with d == 0 or an entry of W_t that is not finite is skipped as if it were absent.  A triangle has a
 *           box of its own: floor(min(p_a.x, p_b.x, p_c.x)) - 1 <= X < ceil(max(p_a.x, p_b.x, p_c.x)) + 2 and the same in y, in double;
 *           it covers no pixel outside it, whatever the edge functions say.  (With exact arithmetic the box holds every pixel the edge
 *           functions accept, with a pixel to spare.  The rounded edge functions of a needle triangle with a corner far outside the
 *           frame -- 1e9 and beyond -- can be >= 0 many pixels past its corners; the box makes the answer one that every path of the
 *           kernel gives alike.)  The pixel takes the lowest-numbered remaining triangle whose box holds it and with e0 >= 0, e1 >= 0
 *           and e2 >= 0 (a comparison with a NaN is false) -- also on an edge two triangles share, where a folded shape overlaps
 *           itself, and under a FOLDED triangle: such pixels follow the formula.
 *   position   u = (W_t00 X + W_t01 Y) + W_t02, v likewise, in float32, then sdm_align_crops' quantisation.  The pixel is IN THE
 *           FOOTPRINT of the row when it is in the box, has a triangle, u and v are finite with |u|, |v| <= 2^20, and
 *           -1 <= u0 <= crop_width - 1, -1 <= v0 <= crop_height - 1.  (The position of the pixel's one triangle decides: no second
 *           triangle is tried.)
 *   colour  the four taps, their clamping into the crop, the decode and (... + 512) >> 10 of "Pasting crops back", unchanged.
 *   opacity a tap reads 0 when it lies outside the crop OR ITS CROP PIXEL HAS LABEL 255; otherwise the opacity map's byte, or 255 with
 *           alpha_dev NULL; the same weights and rounding.  The hull of the mesh therefore fades over one pixel by itself.  The warp
 *           writes v = 0 outside the hull; the colour taps still read those elements, at the reduced opacity.  A caller who wants them
 *           gone passes a map that fades inside the hull.
 *   write, several rows on one frame, never stored to   those of "Pasting crops back", word for word: the blend divides by 255, a pixel
 *           is loaded once, every row of the frame whose footprint holds it is applied in increasing row number in registers, it is
 *           stored once and only if some opacity was not 0, stores are per byte.
 * NV12 destinations are refused here and taken by sdm_warp_paste_tensor_nv12 / _at_nv12 ("Pasting warped faces back into NV12
 * frames" below, with the block ownership of "Pasting crops back into NV12 frames").
 * These calls are plain bilinear; the antialiasing for a face that is smaller in the frame than its crop is the filtered form,
 * "Pasting warped faces back, filtered" below.  Out of scope, and not half-built: a colour renormalised at the hull's border.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: no mesh (none set, or sdm_set_model_geometry has changed L since);
 * fit form: no current rows, and sdm_warp_crops_tensor's rules on the rows' source sizes; everything sdm_align_paste_tensor refuses of
 * spec, in_dev, paste, dst_frames, n_frames, an NV12 frame, a row's image index or a size mismatch; _at form: points_host NULL or
 * n_rows < 1. */
/* the current rows.  in_dev: N * channels * out_height * out_width elements.  matrices_host (N x T x 6: the A_t bits that
 * sdm_warp_crops_tensor returns) and flags_host (N) may be NULL; they come back behind the call's one synchronise.  Neither the landmark
 * state, the images, the crop source nor the tracker's slots are changed. */
int sdm_warp_paste_tensor(sdm_ctx* ctx, const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste,
                          const sdm_frame* dst_frames, int n_frames, float* matrices_host /* out, N x T x 6, may be NULL */,
                          int* flags_host /* out, may be NULL */);
/* explicit landmarks: the mesh is needed, but no landmark state, no geometry rows and no context images -- the network may run on frame t
 * while the tracker has stepped to t + 1 */
int sdm_warp_paste_tensor_at(sdm_ctx* ctx, const float* points_host /* in, n_rows x K x 2: (x, y) of the mesh's k-th landmark */,
                             const int* image_index /* NULL: row i -> frame i */, int n_rows, const sdm_align_tensor* spec,
                             const void* in_dev, const sdm_align_paste* paste, const sdm_frame* dst_frames, int n_frames, int* flags_host);

/* Pasting warped faces back into NV12 frames: sdm_warp_paste_tensor and sdm_warp_paste_tensor_at for a list of destinations that may
 * hold NV12 frames, which closes decode -> warp -> network -> paste -> encode for the piecewise-affine path without a whole-frame
 * conversion.  The section is a composition of two others and restates nothing else.
 *   per luma pixel   everything is that of "Pasting warped faces back", word for word: the points and the flags (PARTIAL against the
 *           destination's luma width and height), the row's box and the triangle's box, the lowest-numbered triangle and the one
 *           position that decides, the footprint, the four taps, and the opacity that reads 0 outside the crop or on label 255.
 *   destination, luma, chroma, several rows on one frame, never stored to   those of "Pasting crops back into NV12 frames", word for
 *           word, with "the row's footprint" being the mesh footprint: dst_chroma, the 1-channel rule, the opacity-weighted mean over
 *           the block, cnt and a_c, the rows in increasing row number, the 2 x 2 block as the unit of ownership, per-byte stores.
 *   a consequence   a pixel of a block that lies outside the hull or outside the row's box has a_i = 0.  It still counts in cnt: a
 *           block that the hull's edge crosses gets the colour of its covered pixels at an opacity reduced by the uncovered ones.
 *   mixed lists   the other five formats are accepted in the same list and get exactly the bytes of sdm_warp_paste_tensor[_at];
 *           their dst_chroma entry is ignored.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: everything sdm_warp_paste_tensor[_at] refuse, except an NV12
 * frame; an NV12 frame with stride_bytes < 2 * ((width + 1) / 2). */
int sdm_warp_paste_tensor_nv12(sdm_ctx* ctx, const sdm_align_tensor* spec, const void* in_dev, const sdm_align_paste* paste,
                               const sdm_frame* dst_frames,
                               void* const* dst_chroma /* n_frames second planes (NV12: UV, planar: plane 1); NULL, or a NULL entry: behind the first plane */, int n_frames,
                               float* matrices_host /* out, N x T x 6, may be NULL */, int* flags_host /* out, may be NULL */);
int sdm_warp_paste_tensor_at_nv12(sdm_ctx* ctx, const float* points_host /* in, n_rows x K x 2 */,
                                  const int* image_index /* NULL: row i -> frame i */, int n_rows, const sdm_align_tensor* spec,
                                  const void* in_dev, const sdm_align_paste* paste, const sdm_frame* dst_frames, void* const* dst_chroma,
                                  int n_frames, int* flags_host);

/* Pasting warped faces back, filtered: sdm_warp_paste_tensor[_at][_nv12] with area-averaged sampling where a triangle's inverse map
 * minifies.  The networks behind this path run at 256 or 512 pixels in template space and go back onto faces 60 to 200 pixels wide; on a
 * turned head the far cheek's triangles take 8 or more tensor elements per frame pixel along one axis while the near cheek's take 2, so
 * the sub-sample count is chosen per TRIANGLE and per AXIS, as "Warped faces, filtered" does on the way in.  One launch for the pixels
 * behind the fit, the prepare stage and a small stage for the counts; the destination list may mix GRAY, BGR, RGB, BGRA, RGBA and NV12
 * frames, dst_chroma as in the _nv12 calls.  Every rule of "Pasting warped faces back" and "Pasting warped faces back into NV12 frames"
 * that is not restated here holds word for word.  Every float operation is rounded on its own, nothing is contracted.
 *   1. unchanged   the points, A_t, W_t (the inverse of the float32 A_t) and the flags; the row's box and each triangle's box; the
 *      lowest-numbered triangle whose box and edge functions hold the pixel CENTRE; the position of the centre through that one
 *      triangle; and the FOOTPRINT, which is exactly the unfiltered one: the centre lies in the row's box, has a triangle, and its
 *      position is accepted.  The row's box is not widened and there is no second, working footprint: the filter changes what a row
 *      contributes to a pixel it holds, never which pixels it holds.  The ownership rule -- one reader and writer per pixel, per 2 x 2
 *      block on NV12, rows applied in increasing row number -- is the existing one on the existing predicate.
 *   2. (Sx, Sy) of row n, triangle t   from the float32 W_t, in float32, each operation rounded: cx2 = W00 W00 + W10 W10 (the crop step
 *      per frame column, squared), cy2 = W01 W01 + W11 W11 (per frame row).  Sx is the rule of sdm_align_crops_tensor_filtered's S on
 *      cx2, Sy the same rule on cy2: 1 for mode BILINEAR, for a DEGENERATE row, for a triangle that is skipped or covers nothing
 *      (det E == 0, d == 0, an entry of W_t not finite, or a row whose box is empty), for a value that is not finite or below
 *      min_scale * min_scale (float32); otherwise the smallest integer in [1, max_samples] with (float)(S S) >= value, and max_samples
 *      when there is none.  samples_host[(n T + t) 2] = Sx, [(n T + t) 2 + 1] = Sy.  For a row whose points are a similarity of the
 *      template, Sx = Sy = the S of the rigid filtered paste.
 *   3. sub-samples of frame pixel (X, Y) whose triangle is t   for u in 0 ... Sx - 1 and v in 0 ... Sy - 1: fX = (float)X + o_Sx[u],
 *      fY = (float)Y + o_Sy[v] with the offsets of sdm_align_crops_tensor_filtered.  All go through the pixel's own W_t, also those
 *      whose frame position lies past the triangle's edge: (W00 fX + W01 fY) + W02, v likewise; each is quantised as in "Pasting crops
 *      back" (the 2^20 rule, 1/32 pixel) and gives the UNROUNDED weighted sums per channel (taps clamped into the crop) and of the
 *      opacity, where a tap reads 0 outside the crop OR ON A CROP PIXEL WITH LABEL 255, otherwise the map's byte, or 255 without a map.
 *   4. pixel   with n = Sx Sy <= 256: q_c = (sum + 512 n) / (1024 n) per channel, a the same on the opacity sums, unsigned integer
 *      divisions; the sums stay below 2^26 + 2^17.  Channel order, the gray weights, the / 255 blend, the NV12 luma and chroma formulas
 *      and the block's opacity-weighted mean apply to the averaged q and a exactly as they do at n = 1.  A pixel of which any
 *      sub-sample is refused by the 2^20 rule gets a = 0 from that row.
 *   5. bit identity   a pixel whose triangle has Sx = Sy = 1 takes exactly the bytes of the unfiltered call; mode BILINEAR writes
 *      exactly the bytes of sdm_warp_paste_tensor[_at] on lists without NV12 frames and of sdm_warp_paste_tensor[_at]_nv12 on lists
 *      with them.
 *   6. consequences   the MAP is continuous across an edge two triangles share, the sample count is not; W_t extrapolates up to half a
 *      frame pixel past its triangle; the hull's border is now antialiased from the inside -- a border pixel's sub-samples that land
 *      on label 255 count with opacity 0 --; a frame pixel whose centre lies outside the hull is still never touched.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: everything the _nv12 forms of the warped paste refuse; filter NULL,
 * an unknown mode, max_samples outside [1, 16], min_scale not finite or below 1.  samples_host (N x T x 2) may be NULL; it comes back
 * in the same copy as the flags.  Out of scope: widening the footprint beyond pixels whose centre lies in the hull. */
int sdm_warp_paste_tensor_filtered(sdm_ctx* ctx, const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                   const sdm_align_paste* paste, const sdm_frame* dst_frames, void* const* dst_chroma, int n_frames,
                                   float* matrices_host /* N x T x 6, may be NULL */, int* flags_host /* may be NULL */,
                                   int* samples_host /* N x T x 2, may be NULL */);
int sdm_warp_paste_tensor_at_filtered(sdm_ctx* ctx, const float* points_host, const int* image_index, int n_rows,
                                      const sdm_align_tensor* spec, const sdm_align_filter* filter, const void* in_dev,
                                      const sdm_align_paste* paste, const sdm_frame* dst_frames, void* const* dst_chroma, int n_frames,
                                      int* flags_host, int* samples_host);

/* Landmark region masks: from the current rows, one crop_height x crop_width uint8 opacity map per row, in CROP space, on the device --
 * polygons over named landmarks (or the convex hull of a set of landmarks), minus holes, grown and feathered.  The bytes are what
 * sdm_align_paste.alpha_dev with alpha_per_row = 1 takes: "paste only inside the face outline", "the mouth only", "everything but the
 * eyes", or a per-face prior channel of a network.  Two launches behind the fit for all rows (the vertices, the pixels).  Every float
 * operation is float32 and rounded on its own, nothing is contracted, except where double is named; division and square root are
 * correctly rounded.
 *   fit, W   the fit is that of sdm_align_crops: the same kernel, the same M, the same flags (the _at form: row n of matrices_host, and no
 *           PARTIAL is evaluated -- it knows no frame).  W (frame -> crop) is the inverse of the float32 M computed as in "Pasting
 *           crops back".  SDM_ALIGN_DEGENERATE as there: the fit flags it, an entry of M is not finite, d == 0, or an entry of W is not
 *           finite; the row's map is all zeros.
 *   region   a list of 1 to 8 polygons.  Polygon g has sizes[g] landmark indices into [0, L), 3 <= sizes[g] <= 128, one polygon after the
 *           other in vertex_index; their sum P is at most 256.  The last n_holes polygons are holes, 0 <= n_holes < n_polygons.  Bit g of
 *           hull_bits makes polygon g the convex hull of its points.  |grow| <= 1024, 0 <= feather <= 1024.
 *   vertices   p_k = (x[i_k], x[L + i_k]) of the row (the _at form: row n of points_host, P points in the polygons' order);
 *           q_k = ((W00 px + W01 py) + W02, (W10 px + W11 py) + W12).  A row that is not DEGENERATE and has a q that is not finite or
 *           has |qx| or |qy| > 2^20 gets an all-zero map and SDM_REGION_NONFINITE.
 *   hull    the q sorted by (x, then y), comparisons exact, exact duplicates dropped; Andrew's monotone chain with
 *           turn(o, a, b) = sign of (double)(ax - ox) * (double)(by - oy) - (double)(ay - oy) * (double)(bx - ox), the four differences
 *           taken in float32 first (the products are exact in double: the sign is exact); pop while the turn is <= 0; the lower chain,
 *           then the upper chain.  One or two vertices may remain (all points equal, or all collinear): the rules below hold for m >= 1.
 *   signed distance of crop pixel (column c, row r) to a polygon q_0 ... q_{m-1}: P = ((float)c, (float)r), D2 = +inf, wn = 0; for
 *           k = 0 ... m - 1 with a = q_k, b = q_{(k + 1) mod m}:
 *               ex = bx - ax; ey = by - ay; wx = Px - ax; wy = Py - ay;  ee = (ex ex) + (ey ey)
 *               t  = ee > 0 ? fminf(fmaxf(((wx ex) + (wy ey)) / ee, 0), 1) : 0
 *               dx = wx - (t ex); dy = wy - (t ey);  D2 = fminf(D2, (dx dx) + (dy dy));  cr = (ex wy) - (ey wx)
 *               if (ay <= Py) { if (by > Py && cr > 0) ++wn; } else if (by <= Py && cr < 0) --wn;
 *           sd = sqrtf(D2), negated when wn != 0: the non-zero winding rule (a closed mouth's folded inner-lip polygon stays filled).
 *   map     s = +inf; every polygon that is no hole: s = fminf(s, sd); every hole, in order: s = fmaxf(s, -sd); wr = fmaxf(feather, 1.0f);
 *           a = 0.5f + ((grow - s) / wr), clamped to [0, 1]; byte = rintf(a * 255.0f).  The ramp is centred on the contour moved outwards
 *           by grow; feather 0 is a one-pixel antialiased edge.
 *   out_dev   N * crop_height * crop_width bytes, dense, 16-byte aligned, row n at n * crop_height * crop_width.  Nothing else is written.
 * Refused with SDM_ERR_INVALID, no state changed, nothing launched: what sdm_align_crops_tensor refuses of landmark_index, template_xy,
 * K, the crop size and the rows (fit form); region NULL, sizes NULL, counts, sizes, P or n_holes outside the ranges above; a hull bit at
 * or beyond n_polygons; vertex_index NULL or an index outside [0, L); grow or feather not finite or outside their ranges; out_dev NULL
 * or not 16-byte aligned; _at form: matrices_host or points_host NULL, n_rows < 1, crop_width or crop_height outside [1, 1024]. */
#define SDM_REGION_NONFINITE 16
typedef struct sdm_region_mask {
    const int* sizes;           /* n_polygons vertex counts, the holes last                                          */
    int n_polygons, n_holes;
    unsigned hull_bits;         /* bit g: polygon g is the convex hull of its points                                 */
    float grow, feather;        /* crop pixels                                                                       */
} sdm_region_mask;
/* the current rows.  matrices_host (N x 6) and flags_host (N) may be NULL; they come back in one copy behind the call's one synchronise. */
int sdm_align_region_mask(sdm_ctx* ctx, const int* landmark_index, const float* template_xy, int K, int crop_width, int crop_height,
                          const int* vertex_index /* P */, const sdm_region_mask* region, uint8_t* out_dev,
                          float* matrices_host /* N x 6, may be NULL */, int* flags_host /* may be NULL */);
/* explicit matrices (what an earlier crop call returned) and frame-space points: no landmark state, no geometry, no images needed */
int sdm_align_region_mask_at(sdm_ctx* ctx, const float* matrices_host /* n_rows x 6 */, const float* points_host /* n_rows x P x 2, frame */,
                             int n_rows, int crop_width, int crop_height, const sdm_region_mask* region, uint8_t* out_dev,
                             int* flags_host /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* SDM_H_ */
