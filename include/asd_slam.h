/*
 * asd_slam.h -- C ABI of libasdhip: the MI355X (gfx950) implementation of ASD-SLAM's
 * per-frame front-end and local-BA hot path.
 *
 * The reference has no plugin / FFI layer: the hot path is reached through C++ methods
 * of libvslam with OpenCV types in every signature.  This header is the
 * flat-array boundary drawn INSIDE those methods; each entry point cites the reference
 * code it replaces (paths relative to the reference root, src/vslam/...).
 * INTEGRATION.md shows the adapter a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C types, caller-owned buffers, row-major, no torch / OpenCV types;
 *   - every call returns ASD_OK (0) or a negative asd_status; asd_last_error(ctx)
 *     returns a human readable message for the last failure on that context;
 *   - one asd_ctx = one HIP device + one HIP stream; a ctx is not thread-safe,
 *     different ctxs may be used from different threads / processes;
 *   - "host" pointers are ordinary CPU memory.  Results that the next stage consumes
 *     (pyramid, descriptors, grid) also stay resident in HBM inside the ctx;
 *   - there is NO CPU fallback: without a usable HIP device asd_ctx_create fails with
 *     ASD_ERR_NO_DEVICE.
 */
#ifndef ASD_SLAM_H
#define ASD_SLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASD_DESC_DIM 128      /* ORBmatcher.cc:1638 assumes exactly 128 columns          */
#define ASD_PATCH 32          /* ORBextractor.cc:1115 Rect(x-16,y-16,32,32)               */
#define ASD_MAX_LEVELS 16
#define ASD_GRID_COLS 64      /* Frame.h:37  FRAME_GRID_COLS                              */
#define ASD_GRID_ROWS 48      /* Frame.h:38  FRAME_GRID_ROWS                              */
#define ASD_HISTO_LENGTH 30   /* ORBmatcher.cc:39                                         */

typedef enum asd_status {
  ASD_OK = 0,
  ASD_ERR_INVALID = -1,     /* bad argument (null pointer, size out of range)             */
  ASD_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at create              */
  ASD_ERR_HIP = -3,         /* a HIP call or kernel failed                                */
  ASD_ERR_NO_WEIGHTS = -4,  /* asd_load_weights was not called                            */
  ASD_ERR_CAPACITY = -5,    /* input exceeds the capacity given at asd_ctx_create         */
  ASD_ERR_NUMERIC = -6,     /* solver breakdown (non positive definite system)            */
  ASD_ERR_RANGE = -7        /* ASDNet (two-piece fp16 operand form): an activation left fp16's range, the
                               descriptors of this call are not valid (see asd_asdnet_pieces)            */
} asd_status;

typedef struct asd_ctx asd_ctx;

/* Replaces the ORBextractor constructor arguments (ORBextractor.cc:452-456; values given
 * in Tracking.cc:77-85) plus device selection. */
typedef struct asd_config {
  int32_t n_features;     /* --feature_count, 2000                                        */
  float   scale_factor;   /* --feature_scale_factor, 1.2                                  */
  int32_t n_levels;       /* --feature_level, 8                                           */
  int32_t ini_th_fast;    /* 20 (Tracking.cc:80)                                          */
  int32_t min_th_fast;    /* 7  (Tracking.cc:81)                                          */
  int32_t max_width;      /* largest image the ctx will see                               */
  int32_t max_height;
  int32_t max_patches;    /* capacity of asd_describe / extract (>= 2*n_features: init)   */
  int32_t device;         /* HIP device ordinal                                           */
} asd_config;

/* cv::KeyPoint as produced by ExtractDesc (ORBextractor.cc:887-898,1236-1242). */
typedef struct asd_keypoint {
  float   x, y;       /* level-0 pixel coordinates (pt * mvScaleFactor[octave])           */
  float   size;       /* (int)(31 * scale[octave]) stored as float                        */
  float   angle;      /* IC_Angle, degrees in [0,360)                                     */
  float   response;   /* FAST score                                                       */
  int32_t octave;
} asd_keypoint;

/* ---- context ------------------------------------------------------------------------ */
int asd_ctx_create(const asd_config* cfg, asd_ctx** out);
int asd_ctx_destroy(asd_ctx* ctx);
/* (ctx == NULL: the message of the calling thread's last asd_bow_score, the one failing call that has no context) */
const char* asd_last_error(const asd_ctx* ctx);
const char* asd_version(void);

/* Scale tables of the extractor: ORBextractor.cc:459-492 (mvScaleFactor, mvLevelSigma2,
 * their inverses, mnFeaturesPerLevel).  Each output holds n_levels entries; any may be
 * NULL. */
int asd_get_scale_tables(const asd_ctx* ctx, float* scale, float* inv_scale, float* sigma2,
                         float* inv_sigma2, int32_t* features_per_level);

/* ---- ASDNet descriptor (E6) --------------------------------------------------------- */
/* Replaces torch::jit::load of bestmodel_c.pt (ORBextractor.cc:457-458).  Takes the 7
 * conv weights in torch layout [cout][cin][kh][kw] and the 7 BatchNorm running
 * mean/var vectors (affine=False, eps as given) of ASDNet.py:334-356; BN is folded into
 * the conv on upload. */
int asd_load_weights(asd_ctx* ctx, const float* const conv_w[7], const float* const bn_mean[7],
                     const float* const bn_var[7], float bn_eps);

/* Replaces computeSIFTDescriptors' forward pass (ORBextractor.cc:1125-1132 ->
 * ASDNet.forward, ASDNet.py:360-370): n u8 patches [n][32][32] -> n unit-norm
 * descriptors [n][128] f32.  Both pointers are host memory. */
int asd_describe(asd_ctx* ctx, const uint8_t* patches, int32_t n, float* desc);

/* Same, device resident: d_patches / d_desc are HIP device pointers; no copies and no
 * synchronisation -- the work is enqueued on the ctx stream (used by bench + extract). */
int asd_describe_device(asd_ctx* ctx, const uint8_t* d_patches, int32_t n, float* d_desc);

/* ---- extractor (E1-E7) -------------------------------------------------------------- */
/* Replaces ORBextractor::ExtractDesc(image, mask, keypoints, descriptors, use_orb=false)
 * (ORBextractor.cc:1137-1249): pyramid, FAST + quadtree, orientation, blur, patch gather,
 * ASDNet.  kps / desc have room for max_patches entries; *n_out receives the count.
 * n_features_override > 0 replaces cfg.n_features for this call (the reference keeps a
 * second extractor with 2*nFeatures for initialisation, Tracking.cc:85). */
int asd_extract(asd_ctx* ctx, const uint8_t* image, int32_t width, int32_t height, int32_t stride,
                int32_t n_features_override, asd_keypoint* kps, float* desc, int32_t* n_out);

/* Same with the image already resident in HBM (d_image = HIP device pointer, row stride in
 * bytes): what a camera driver with a device-side ring buffer, or bench.py, calls. */
int asd_extract_device(asd_ctx* ctx, const uint8_t* d_image, int32_t width, int32_t height, int32_t stride,
                       int32_t n_features_override, asd_keypoint* kps, float* desc, int32_t* n_out);

/* Pipelined extraction.  ExtractDesc of frame t+1 does not depend on the tracking of frame t, and a
 * replay reads its images from disk (Examples/Monocular/kitti.cc:116-155), so they can overlap:
 * asd_extract_submit queues an extraction for a worker thread with its own HIP streams and returns at
 * once; asd_extract_wait blocks until the OLDEST outstanding submission has finished and hands back the
 * same results asd_extract would.  Up to ASD_EXTRACT_QUEUE submissions may be outstanding; the worker runs
 * the front half (pyramid .. patch gather) of the next queued frame underneath the ASDNet pass of the
 * previous one.  `image` must stay valid until its wait.  While submissions are outstanding the worker owns the
 * shared front-end and ASDNet buffers: asd_extract*, asd_describe*, asd_get_level_image / asd_get_raw_corners / asd_get_patches and
 * asd_stereo_match return ASD_ERR_INVALID ("... submission(s) outstanding") instead of racing with it.  If the
 * extractor's streams / buffers cannot be created the call fails and the next submit starts over.  The device-resident
 * descriptors of a waited frame (asd_frame_set with desc == NULL) stay valid for two further submissions. */
#define ASD_EXTRACT_QUEUE 3
int asd_extract_submit(asd_ctx* ctx, const uint8_t* image, int32_t device_resident, int32_t width,
                       int32_t height, int32_t stride, int32_t n_features_override);
int asd_extract_wait(asd_ctx* ctx, asd_keypoint* kps, float* desc, int32_t* n_out);
/* Same without the copy: *kps / *desc point into the library's own result buffers of that submission (the
 * descriptors sit in pinned host memory) and stay valid until two further submissions have been made -- e.g. to
 * wrap them as the Frame's mvKeys / mDescriptors (cv::Mat header over foreign data) for the frame's lifetime in
 * the tracker, which is two frames. */
int asd_extract_wait_view(asd_ctx* ctx, const asd_keypoint** kps, const float** desc, int32_t* n_out);
/* The lifetime of a view, checkable: asd_extract_last_view returns the id of the view handed out by the most recent
 * asd_extract_wait / asd_extract_wait_view (ids count submissions from 0), and asd_extract_view_valid(ctx, id) is 1 as long
 * as no later submission has been given that view's buffers -- exactly: while fewer than ASD_EXTRACT_QUEUE + 2 submissions
 * have been made after the one the view belongs to -- and 0 afterwards (or for an id that was never handed out).  A caller
 * that keeps a view across frames (mCurrentFrame / mLastFrame) can assert this where it dereferences it. */
uint64_t asd_extract_last_view(const asd_ctx* ctx);
int32_t asd_extract_view_valid(asd_ctx* ctx, uint64_t view_id);

/* Intermediate products of the last asd_extract, for tests and for callers that read
 * ORBextractor::mvImagePyramid (ORBextractor.h:87).  Level images are returned WITHOUT
 * the 19 px border.  blurred != 0 selects the GaussianBlur'ed copy
 * (ORBextractor.cc:1226-1227). */
int asd_get_level_size(const asd_ctx* ctx, int32_t level, int32_t* width, int32_t* height);
int asd_get_level_image(asd_ctx* ctx, int32_t level, int32_t blurred, uint8_t* out);
/* Raw FAST corners of a level before the quadtree (ORBextractor.cc:858-876), in the
 * reference's vToDistributeKeys order; coordinates are relative to minBorder (16). */
int asd_get_raw_corners(asd_ctx* ctx, int32_t level, int32_t capacity, float* x, float* y,
                        float* response, int32_t* n_out);
/* The 32x32 patches the last asd_extract / asd_extract_device gathered for ASDNet (ORBextractor.cc:1113-1115: the
 * blurred level, keypoint at [16][16]), in keypoint order: out[min(n, capacity)][32][32], *n_out = min(n, capacity).
 * A later asd_describe overwrites them, after which *n_out = 0 until the next extraction; refused while submissions are outstanding, like the calls above. */
int asd_get_patches(asd_ctx* ctx, int32_t capacity, uint8_t* out, int32_t* n_out);

/* ---- undistortion in front of the extractor (Tracking.cc:104,125) -------------------
 * Tracking::GrabImageMonocular and Tracking::Loc call cv::undistort(im, mImGray, mK, mDistCoef) on every image
 * and build the Frame with distCoefZero.  K = (fx, fy, cx, cy) and dist = (k1, k2, p1, p2) as the CV_32F mK /
 * mDistCoef hold them (Tracking.cc:59-72).
 * asd_undistort_map writes the map pair OpenCV 3.2.0's cv::undistort builds internally (newCameraMatrix empty:
 * initUndistortRectifyMap in stripes of min(max(1, 4096 / width), height) rows, CV_16SC2 + CV_16UC1):
 * xy[height][width][2] = integer source (x, y), frac[height][width] = (y fraction) * 32 + (x fraction), in 1/32 px.
 * Host only: needs no context and no device.  dist == NULL means zero coefficients. */
int asd_undistort_map(const float K[4], const float dist[4], int32_t width, int32_t height, int16_t* xy, uint16_t* frac);
/* Builds that map once and keeps it in HBM: from then on every extraction (asd_extract, asd_extract_device,
 * asd_extract_submit; device, pinned and pageable sources) runs on the undistorted image -- remap INTER_LINEAR,
 * BORDER_CONSTANT 0, integer-exact, as level 0 of the pyramid (asd_get_level_image(0, 0) returns it) -- and an
 * extraction of another size returns ASD_ERR_INVALID.  dist == NULL or four zero coefficients clear the map (no extra
 * launch).  ASD_ERR_CAPACITY above max_width / max_height; ASD_ERR_INVALID while submissions of asd_extract_submit are
 * outstanding. */
int asd_set_undistortion(asd_ctx* ctx, const float K[4], const float dist[4], int32_t width, int32_t height);
/* cv::undistort itself on the context's map, result into host memory dst (row stride dst_stride): for callers that
 * need the image (a viewer, the right image of a stereo pair).  src is a device pointer if device_resident != 0, else
 * host memory (pinned or pageable).  ASD_ERR_INVALID without a map or for another size. */
int asd_undistort(asd_ctx* ctx, const uint8_t* src, int32_t device_resident, int32_t width, int32_t height, int32_t stride,
                  uint8_t* dst, int32_t dst_stride);

/* ---- frames, grid (G1) and matchers (M0-M2, M4 init, M5) ----------------------------- */
/* A frame slot keeps what the reference keeps in Frame: undistorted keypoints
 * (mvKeysUn), descriptors (mDescriptors) and the 64x48 grid (Frame.cc:123-138), all
 * resident in HBM.  Slots are small integers in [0, ASD_MAX_FRAMES). */
#define ASD_MAX_FRAMES 64   /* (round 4: a keyframe and its 20 + 5 x 20 covisible neighbours resident for the batched per-keyframe stage) */
/* Replaces Frame::Frame(...) bookkeeping after ExtractORB: UndistortKeyPoints is the
 * identity for zero distortion (Frame.cc:298-304), image bounds (Frame.cc:351-357),
 * AssignFeaturesToGrid (Frame.cc:123-138).  desc may be NULL to adopt the descriptors of
 * the last asd_extract without a round trip. */
int asd_frame_set(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, const float* desc,
                  int32_t n, float min_x, float max_x, float min_y, float max_y);

/* Replaces Frame::GetFeaturesInArea (Frame.cc:219-274): indices in reference order. */
int asd_frame_features_in_area(asd_ctx* ctx, int32_t slot, float x, float y, float r,
                               int32_t min_level, int32_t max_level, int32_t capacity,
                               int32_t* idx_out, int32_t* n_out);

/* M0: ORBmatcher::DescriptorDistance (ORBmatcher.cc:1629-1650) for every pair, in the
 * reference's summation order (sequential f32, no FMA): out[na][nb].  Also the kernel of
 * MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:271-338). */
int asd_dist_matrix(asd_ctx* ctx, const float* a, int32_t na, const float* b, int32_t nb, float* out);

/* M5: MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:271-338) for one map point:
 * n observations' descriptors [n][128] -> index of the descriptor with the least median
 * distance to the others. */
int asd_distinctive_descriptor(asd_ctx* ctx, const float* desc, int32_t n, int32_t* best_idx);
/* The same for many map points in one call (LocalMapping::ProcessNewKeyFrame / SearchInNeighbors update hundreds
 * per keyframe, LocalMapping.cc:245, 535, 628): set s holds the observation descriptors
 * desc[set_start[s] .. set_start[s+1]) (row-major [.][128], set_start[0] = 0); best_idx[s] = index inside set s. */
int asd_distinctive_descriptor_batch(asd_ctx* ctx, int32_t n_sets, const int32_t* set_start, const float* desc,
                                     int32_t* best_idx);

/* M1: ORBmatcher::SearchByProjection(Frame& cur, const Frame& last, th, bMono=true)
 * (ORBmatcher.cc:1318-1452).  Inputs mirror what the method reads:
 *   last frame: slot_last (keypoint octave/angle), per keypoint i: has_mp[i] (mvpMapPoints[i]
 *   != NULL && !mvbOutlier[i]), world position Xw[i][3] (f32, MapPoint::GetWorldPos) and
 *   the map point's descriptor mp_desc[i][128] (MapPoint::GetDescriptor);
 *   cur frame: slot_cur, pose Tcw[16] f32 row-major 4x4, intrinsics K = fx,fy,cx,cy.
 * Output: match_cur[n_cur] = index i of the last-frame keypoint whose map point was
 * written into CurrentFrame.mvpMapPoints[j], or -1; *n_matches = the method's return
 * value.  cur.mvpMapPoints is taken as all-NULL on entry (Tracking.cc:670).
 * check_orientation mirrors mbCheckOrientation.
 * mp_obs_positive[i] (NULL = all non-zero): MapPoint::Observations() > 0 of last-frame map point i.  A current keypoint
 * that received a map point WITHOUT observations earlier in the same call is not skipped by later map points
 * (ORBmatcher.cc:1392-1395) and may be overwritten; each write counts in the return value and enters the rotation
 * histogram, exactly as in the reference (a keypoint written twice can be removed -- and subtracted -- twice). */
int asd_match_project_frame(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last,
                            const uint8_t* has_mp, const float* Xw, const float* mp_desc,
                            const float* Tcw, const float* K, float th, int32_t check_orientation,
                            int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive);

/* M2: ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>&, th)
 * (ORBmatcher.cc:44-122) after Frame::isInFrustum (Frame.cc:160-217) has filled the
 * tracking fields.  Per map point m: in_view[m] (mbTrackInView && !isBad), proj[m] = (u,v),
 * level[m] = mnTrackScaleLevel, view_cos[m], desc[m][128].  occupied[j] != 0 marks current
 * keypoints that already hold a map point with Observations()>0 on entry.
 * Output: match_cur[n_cur] = map point index m written to F.mvpMapPoints[j] or -1 (entries
 * occupied on entry stay -1); *n_matches = reference return value
 * (counts each match twice, ORBmatcher.cc:116-117).
 * mp_obs_positive[m] (NULL = all non-zero): Observations() > 0 of map point m; a keypoint given a map point without
 * observations earlier in this call stays available to later map points (ORBmatcher.cc:86-88). */
int asd_match_project_points(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view,
                             const float* proj, const int32_t* level, const float* view_cos,
                             const float* desc, const uint8_t* occupied, float th, float nn_ratio,
                             int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive);

/* Device-resident descriptor bank.  The reference reads MapPoint::GetDescriptor() for every query of
 * every frame (ORBmatcher.cc:72, :1371) but only rewrites it once per keyframe
 * (MapPoint::ComputeDistinctiveDescriptors, MapPoint.cc:330-337).  An integration that gives each
 * MapPoint a bank row uploads a descriptor when it changes and passes row ids per frame instead of
 * 512-byte descriptors: asd_match_project_frame_bank / asd_match_project_points_bank are
 * asd_match_project_frame / _points with `rows` in place of the descriptor table.
 * Rows: both banks (this one and the attribute bank of asd_mpbank_put) grow on demand, from 16384 rows, to hold every row written;
 * first_row + n is summed in 64 bits and may not exceed ASD_BANK_MAX_ROWS (ASD_ERR_CAPACITY, asd_last_error names the limit; nothing
 * is allocated or enqueued then).  A negative first_row or n is ASD_ERR_INVALID.  Growth waits for EVERY stream of the context -- the
 * second stream of an asd_prep_async bracket included -- before the old rows are carried over, so no row written earlier is lost,
 * whichever stream its write was enqueued on. */
#define ASD_BANK_MAX_ROWS (1 << 22) /* 2 GiB of descriptors */
int asd_bank_put(asd_ctx* ctx, int32_t first_row, int32_t n, const float* desc);
/* bank[first_row + i] = descriptor of keypoint i of frame `slot`, i in [0, n): device to device */
int asd_bank_put_from_frame(asd_ctx* ctx, int32_t slot, int32_t first_row, int32_t n);
int asd_match_project_frame_bank(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last,
                                 const uint8_t* has_mp, const float* Xw, const int32_t* mp_rows,
                                 const float* Tcw, const float* K, float th, int32_t check_orientation,
                                 int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive);
int asd_match_project_points_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view,
                                  const float* proj, const int32_t* level, const float* view_cos,
                                  const int32_t* rows, const uint8_t* occupied, float th, float nn_ratio,
                                  int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive);

/* Fused tracking chains: the numeric bodies of Tracking::TrackWithMotionModel (Tracking.cc:664-723) and Tracking::TrackLocalMap
 * (:725-736 with the matcher call of SearchLocalPoints, :803-851) as ONE submission each -- search, claim replay, edge assembly
 * and Optimizer::PoseOptimization enqueued back to back on the device, one synchronisation at the end (the separate calls
 * cost two host round trips).  Results are bit-identical to calling the matcher and asd_pose_optimize one after the other.
 *
 * asd_track_motion_model = asd_match_project_frame (same arguments) followed by PoseOptimization over the matches: keypoint j
 * with match_cur[j] = i >= 0 contributes the edge (Xw[i], keypoint j, invSigma2 of its octave: Optimizer.cc:272-310), edges in
 * keypoint order.  pose7 in = SE3Quat of the predicted Tcw (Tracking.cc:672), out = the optimised pose; outlier[n_cur] =
 * mvbOutlier (0 where the keypoint has no match); *n_inliers = nInitialCorrespondences - nBad.  The caller keeps the
 * control flow: the nmatches < 20 retry with 2*th (:681-685) is a second call, the outlier discard (:695-714) a loop over
 * `outlier`.  Fewer than 3 matches: pose7 untouched, *n_inliers = 0 (Optimizer.cc:323-324). */
int asd_track_motion_model(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw,
                           const float* mp_desc, const float* Tcw, const float* K, float th, int32_t check_orientation,
                           const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur, int32_t* n_matches,
                           uint8_t* outlier, int32_t* n_inliers);
int asd_track_motion_model_bank(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw,
                                const int32_t* mp_rows, const float* Tcw, const float* K, float th, int32_t check_orientation,
                                const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur, int32_t* n_matches,
                                uint8_t* outlier, int32_t* n_inliers);
/* asd_track_local_map = asd_match_project_points (same arguments) followed by PoseOptimization over ALL map points of the
 * frame: keypoint j contributes an edge if occupied[j] != 0 (it held a map point on entry: world position cur_Xw[j][3]) or
 * match_cur[j] = m >= 0 (world position mp_Xw[m][3]).  mp_Xw[n_mp][3] / cur_Xw[n_cur][3] are f32 world positions
 * (MapPoint::GetWorldPos); the other outputs as above. */
int asd_track_local_map(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj,
                        const int32_t* level, const float* view_cos, const float* desc, const float* mp_Xw,
                        const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio,
                        const uint8_t* mp_obs_positive, const float* K, double* pose7, int32_t* match_cur,
                        int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers);
int asd_track_local_map_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj,
                             const int32_t* level, const float* view_cos, const int32_t* rows, const float* mp_Xw,
                             const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio,
                             const uint8_t* mp_obs_positive, const float* K, double* pose7, int32_t* match_cur,
                             int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers);

/* The same with Tracking::SearchLocalPoints' frustum loop (Tracking.cc:817-835) on the device as well: the map points are given
 * as for asd_frustum (position, normal, raw mfMinDistance / mfMaxDistance) together with the frame pose Tcw they are projected
 * with; isInFrustum, PredictScale (the level by comparison with thresholds derived from the host's logf: same value as libm's)
 * and the search windows are computed on the device, then asd_track_local_map's chain runs.  Xw doubles as the position
 * table of the new matches' edges. */
int asd_track_local_points(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const float* Xw, const float* normal,
                           const float* min_dist, const float* max_dist, const float* desc, const float* Tcw, const float* K,
                           float viewing_cos_limit, const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio,
                           const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur, int32_t* n_matches,
                           uint8_t* outlier, int32_t* n_inliers);
int asd_track_local_points_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const float* Xw, const float* normal,
                                const float* min_dist, const float* max_dist, const int32_t* rows, const float* Tcw,
                                const float* K, float viewing_cos_limit, const uint8_t* occupied, const float* cur_Xw, float th,
                                float nn_ratio, const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur,
                                int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers);

/* asd_track_local_points_bank with the map points named by ROW of both banks (descriptor bank + the attribute bank below: position, normal,
 * distance range as asd_mpbank_put stored them): Tracking::SearchLocalPoints' loop (Tracking.cc:817-835) walks mvpLocalMapPoints, whose
 * attributes change once per keyframe (UpdateNormalAndDepth) -- per frame the host then names the points it selected (4 bytes each) instead
 * of gathering and uploading 36 bytes per point.  Results as asd_track_local_points_bank on the same attributes, bit for bit.  n_mp >= 1;
 * sizes beyond the device replay return ASD_ERR_CAPACITY (use the _bank form).  Honours asd_track_async / asd_track_finish. */
int asd_track_local_points_rows(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const int32_t* rows, const float* Tcw, const float* K,
                                float viewing_cos_limit, const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio,
                                const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier,
                                int32_t* n_inliers);

/* Map-point attribute bank, the companion of the descriptor bank (same row ids): MapPoint::mWorldPos, mNormalVector,
 * mfMinDistance, mfMaxDistance (MapPoint.cc:60-77, 340-391; rewritten by UpdateNormalAndDepth once per keyframe, read by
 * Frame::isInFrustum for every local map point of every frame, Frame.cc:160-217).  Xw[n][3], normal[n][3], min_dist[n],
 * max_dist[n] (raw values: isInFrustum's 0.8 / 1.2 factors are applied by the kernels).  The arrays are consumed on return. */
int asd_mpbank_put(asd_ctx* ctx, int32_t first_row, int32_t n, const float* Xw, const float* normal, const float* min_dist,
                   const float* max_dist);

/* Both tracking stages of a frame as ONE submission -- an OPTIONAL form with a precondition the reference's Tracking does not
 * meet in general; the form that binds to Tracking.cc as it stands is the two-call one (asd_track_motion_model_bank -> host ->
 * asd_track_local_points_bank), and that is what bench.py's `value` is measured on.
 * What it does: asd_track_motion_model_bank, then -- on the device, where the host of the two-call form sits -- what Tracking
 * does between the stages: matches PoseOptimization marked as outliers are dropped (Tracking.cc:695-714), the optimised pose
 * becomes the frame's pose (Frame::SetPose, Frame.cc:150-158), the map points the motion-model stage matched -- kept, or
 * dropped as outliers (both carry mnLastFrameSeen = this frame: :705-707, :811-823) -- are left out of the local-map search;
 * then asd_track_local_points_bank over the remaining candidates, from the motion-model stage's pose and kept matches.
 * The precondition: the reference selects mvpLocalMapPoints BETWEEN the stages (Tracking::UpdateLocalMap, Tracking.cc:730 ->
 * :871-879: UpdateLocalKeyFrames :907-1000 votes over the matches the motion-model stage has just made, UpdateLocalPoints
 * :881-905 collects those keyframes' points).  This call has no place for that decision: the local map is passed as a list
 * known BEFORE the frame is tracked -- n_cand rows of the attribute + descriptor bank (cand_rows), and per keypoint of the last
 * frame the candidate index of the map point it holds (last_cand[i], -1 = not among the candidates; NULL = none is).  Results
 * equal the reference's only when that list IS the set UpdateLocalMap would select: localisation against a fixed map whose
 * local set the caller fixes per frame, or a caller that deliberately tracks against the previous frame's local map (one
 * frame of lag in the keyframe vote).  Any other superset lets the local-map stage match points the reference would not have
 * searched.  Given the same candidate list the results are those of the two calls bit for bit (match2[j] is a CANDIDATE index).
 * pose7: in = SE3Quat of the predicted pose, out = the local-map stage's optimum; pose1 = the motion-model stage's.  The
 * control flow stays with the caller as before: if the motion-model stage made too few matches (nmatches < 20,
 * Tracking.cc:681-685) it discards match2 / pose7 and runs the retry with the separate calls.  Sizes beyond the one-submission
 * form (more than 4096 last-frame points, more than 32768 candidates, frames beyond the
 * solver's LDS form) return ASD_ERR_CAPACITY: use the two calls.  Honours asd_track_async / asd_track_finish.
 * (asd_update_local_map makes that decision on the device from a resident table: running it between the two stages inside this call, which
 * would meet the precondition, is left to a later change.) */
typedef struct asd_track_frame_args {
  int32_t slot_cur, slot_last;
  const uint8_t* has_mp;            /* [n_last] motion-model stage: as asd_track_motion_model_bank */
  const float* Xw_last;             /* [n_last][3] */
  const int32_t* last_rows;         /* [n_last] descriptor-bank rows */
  const int32_t* last_cand;         /* [n_last] or NULL */
  const uint8_t* last_obs_positive; /* [n_last] or NULL */
  const float* Tcw;                 /* [16] predicted pose the motion-model search projects with */
  float th;                         /* its window factor (15 mono, Tracking.cc:676-680) */
  int32_t check_orientation;
  int32_t n_cand;                   /* local-map stage: as asd_track_local_points_bank, attributes from the bank */
  const int32_t* cand_rows;         /* [n_cand] rows of the attribute and descriptor banks */
  const uint8_t* cand_obs_positive; /* [n_cand] or NULL */
  float viewing_cos_limit, th_local, nn_ratio;
  const float* K;                   /* fx fy cx cy */
  double* pose7;                    /* [7] in / out */
  double* pose1;                    /* [7] out */
  int32_t *match1, *n_matches1; uint8_t* outlier1; int32_t* n_inliers1;   /* [n_cur] tables, as the stage calls return them */
  int32_t *match2, *n_matches2; uint8_t* outlier2; int32_t* n_inliers2;
} asd_track_frame_args;
int asd_track_frame(asd_ctx* ctx, const asd_track_frame_args* args);

/* Frame construction beside the stages in flight.  Between asd_prep_async(ctx, 1) and asd_prep_async(ctx, 0) the device
 * work of asd_frame_set, asd_bank_put_from_frame and asd_mpbank_put is enqueued on a second stream of the context instead of
 * behind the outstanding asd_track_* stage (the reference's Frame constructor runs before the frame is tracked, not after the
 * previous one: Tracking.cc:96-118); closing the bracket orders everything enqueued on the context AFTERWARDS behind it.  The
 * caller guarantees what ordering on one stream gave for free: nothing written inside the bracket (the frame slot, the bank
 * rows) is read by a stage still in flight.
 * What the bracket does NOT order: opening it does not put the second stream behind work already enqueued on the context's stream.
 * A frame slot written OUTSIDE a bracket must therefore be complete -- some call that waits for the context's stream (a matcher or
 * asd_track_* call run to completion, asd_track_finish, asd_bank_put, asd_extract_device) or for work ordered behind the slot's copies
 * (asd_extract_wait* of a submission made after the asd_frame_set: submissions wait for the adoption copy) has returned since -- before
 * a call inside a bracket reads it (asd_bank_put_from_frame's source slot).  The host loop of host/track_loop.cpp behaves this way:
 * the only frame it sets outside a bracket is the first of a run, and the bracket that reads that slot first takes the next frame's
 * extraction, submitted or run after it. */
int asd_prep_async(asd_ctx* ctx, int32_t on);

/* Split-phase execution of the asd_track_* calls.  asd_track_async(ctx) arms the NEXT asd_track_motion_model[_bank] /
 * asd_track_local_map[_bank] / asd_track_local_points[_bank] call on this context: it returns as soon as its work is enqueued
 * -- every INPUT array has been consumed by then and may be reused, the OUTPUT arrays (pose7, match_cur, n_matches,
 * outlier, n_inliers) must stay valid -- and asd_track_finish(ctx) waits for the device, fills the outputs and returns the
 * status the synchronous call would have returned (same results bit for bit: same kernels, same order).  The host work of
 * the next frame that does not depend on this result -- Frame construction in the reference: asd_extract_wait[_view],
 * asd_frame_set on ANOTHER slot, asd_extract_submit, asd_bank_put*, and asd_local_ba_submit / _wait / _poll -- may run in
 * between (it is enqueued behind the chain on the context's stream); any other call that uses the matcher or the pose solver
 * returns ASD_ERR_INVALID until asd_track_finish.  An armed call that fails returns its error and leaves nothing outstanding;
 * asd_track_finish with nothing outstanding is ASD_ERR_INVALID. */
int asd_track_async(asd_ctx* ctx);
int asd_track_finish(asd_ctx* ctx);

/* Frame::isInFrustum (Frame.cc:160-217) + MapPoint::PredictScale (MapPoint.cc:438-453) for
 * n map points: Xw[n][3], normal[n][3] (GetNormal), min_dist[n] / max_dist[n] = the map
 * point's raw mfMinDistance / mfMaxDistance (the 0.8 / 1.2 invariance factors of
 * MapPoint.cc:409-419 are applied inside).  Outputs as consumed by M2.  Runs on the host:
 * a few thousand points x ~50 flops, and PredictScale's logf must match libm bit for bit. */
int asd_frustum(asd_ctx* ctx, int32_t slot_cur, int32_t n, const float* Xw, const float* normal,
                const float* min_dist, const float* max_dist, const float* Tcw, const float* K,
                float viewing_cos_limit, uint8_t* in_view, float* proj, int32_t* level, float* view_cos);

/* M4 (bootstrap only): ORBmatcher::SearchForInitialization (ORBmatcher.cc:416-531).
 * prev_matched[n1][2] in/out (vbPrevMatched), matches12[n1] out (index in frame 2 or -1). */
int asd_match_init(asd_ctx* ctx, int32_t slot1, int32_t slot2, float* prev_matched, int32_t window,
                   float nn_ratio, int32_t check_orientation, int32_t* matches12, int32_t* n_matches);

/* DBoW2::FeatureVector of a frame (node id at `levelsup` = 4 -> keypoint indices; Frame::ComputeBoW,
 * Frame.cc:289-296), as produced by asd_compute_bow below or by the caller's own DBoW2.
 * node_id ascending (std::map order), start has n_nodes+1 entries into idx. */
typedef struct asd_feature_vector {
  int32_t n_nodes;
  const int32_t* node_id;
  const int32_t* start;
  const int32_t* idx;
} asd_feature_vector;

/* ---- relocalisation / loop-closing variants of the projection searches ----
 * Flat-array forms of the remaining ORBmatcher overloads.  min_dist / max_dist are the raw mfMinDistance /
 * mfMaxDistance (the 0.8 / 1.2 factors of Get{Min,Max}DistanceInvariance are applied inside), K = fx fy cx cy,
 * poses row-major 4x4 f32.  Pointer-graph side effects stay with the caller. */

/* ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, float th,
 * float ORBdist) (ORBmatcher.cc:1455-1582, Tracking::Relocalization).  Arrays over pKF's keypoints (n_kf):
 * valid[i] = pMP && !isBad() && !sAlreadyFound.count(pMP); kf_angle[i] = pKF->mvKeysUn[i].angle;
 * occupied[j] = CurrentFrame.mvpMapPoints[j] != NULL on entry.  match_cur[j] = i (pKF's map point assigned to the
 * current frame's keypoint j) or -1; *n_matches = return value. */
int asd_match_project_keyframe(asd_ctx* ctx, int32_t slot_cur, int32_t n_kf, const uint8_t* valid, const float* Xw,
                               const float* min_dist, const float* max_dist, const float* desc, const float* kf_angle,
                               const uint8_t* occupied, const float* Tcw, const float* K, float th, float orb_dist,
                               int32_t check_orientation, int32_t* match_cur, int32_t* n_matches);

/* ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
 * vector<MapPoint*>& vpMatched, int th) (:300-413, LoopClosing).  valid[i] = !isBad() && !spAlreadyFound.count(pMP).
 * matched_kp[j] in/out over pKF's keypoints: -1 = vpMatched[j] is NULL, anything else = occupied on entry; the call
 * writes the index i of the point it assigns.  *n_matches = return value. */
int asd_match_project_sim3(asd_ctx* ctx, int32_t slot_kf, const float* Scw, int32_t n_mp, const uint8_t* valid,
                           const float* Xw, const float* normal, const float* min_dist, const float* max_dist,
                           const float* desc, const float* K, int32_t th, int32_t* matched_kp, int32_t* n_matches);

/* ORBmatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
 * vector<MapPoint*>& vpReplacePoint) (:963-1086), search half like asd_fuse_search (no chi2 gate in this overload). */
int asd_fuse_search_sim3(asd_ctx* ctx, int32_t slot_kf, const float* Scw, int32_t n_mp, const uint8_t* valid,
                         const float* Xw, const float* normal, const float* min_dist, const float* max_dist,
                         const float* desc, const float* K, float th, int32_t* best_idx, float* best_dist);

/* ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1090-1314).  Arrays over each keyframe's
 * keypoints: has[i] = map point present, not bad and not already matched (vbAlreadyMatched1/2); T1w / T2w the
 * keyframe poses; R12 row-major 3x3, t12[3].  match12[i1] = i2 for mutually consistent pairs, else -1. */
int asd_match_sim3(asd_ctx* ctx, int32_t slot1, int32_t slot2, const uint8_t* has1, const uint8_t* has2, const float* Xw1,
                   const float* Xw2, const float* min_dist1, const float* max_dist1, const float* min_dist2,
                   const float* max_dist2, const float* desc1, const float* desc2, const float* T1w, const float* T2w,
                   float s12, const float* R12, const float* t12, const float* K, float th, int32_t* match12,
                   int32_t* n_matches);

/* ---- vocabulary ----
 * ORBVocabulary = TemplatedVocabulary<FSift::TDescriptor, FSift> (ORBVocabulary.h:34).  The tree is handed
 * over as flat arrays indexed by DBoW2 node id (0 = root, as in m_nodes): children of node i are
 * child_ids[child_start[i] .. child_start[i+1]) in m_nodes[i].children order (= file order,
 * TemplatedVocabulary.h:1455-1497), weight[i] = m_nodes[i].weight, word_id[i] = m_nodes[i].word_id for
 * leaves and -1 for inner nodes, desc[i] = m_nodes[i].descriptor (128 f32; row 0 unused).
 * weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY; scoring: 0 L1, 1 L2, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA,
 * 5 DOT_PRODUCT (BowVector.h enums).  ASD_ERR_INVALID unless the arrays describe a tree rooted at 0 whose
 * leaves all carry a word id; ASD_ERR_CAPACITY for a branching factor above 64. */
int asd_voc_load(asd_ctx* ctx, int32_t n_nodes, int32_t k, int32_t L, int32_t weighting, int32_t scoring,
                 const int32_t* child_start, const int32_t* child_ids, const double* weight,
                 const int32_t* word_id, const float* desc);
/* TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup) (TemplatedVocabulary.h:1219-1260)
 * for n descriptors: desc != NULL -> host descriptors [n][128]; desc == NULL -> the descriptors resident in
 * frame slot `slot` (n must equal the slot's keypoint count).  Any of word / node / weight may be NULL.
 * A leaf met above level L - levelsup reports itself as node (the reference leaves *nid unset there). */
int asd_bow_descend(asd_ctx* ctx, int32_t slot, const float* desc, int32_t n, int32_t levelsup, int32_t* word,
                    int32_t* node, double* weight);
/* Frame::ComputeBoW (Frame.cc:289-296) = transform(features, BowVector, FeatureVector, levelsup)
 * (TemplatedVocabulary.h:1125-1197).  Outputs (caller-owned, capacity n, fv_start n+1): BowVector as
 * (bow_id ascending, bow_val) with *n_words entries, FeatureVector as CSR over *n_fv_nodes nodes in the
 * asd_feature_vector layout. */
int asd_compute_bow(asd_ctx* ctx, int32_t slot, const float* desc, int32_t n, int32_t levelsup, int32_t* bow_id,
                    double* bow_val, int32_t* n_words, int32_t* fv_node, int32_t* fv_start, int32_t* fv_idx,
                    int32_t* n_fv_nodes);

/* M3: ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)
 * (ORBmatcher.cc:156-297): slot_kf / slot_f hold the two frames, has_mp_kf[i] = pKF has a good map
 * point at keypoint i.  Output match_f[n_f] = keypoint index in pKF whose map point was assigned
 * to F's keypoint, or -1; *n_matches = return value. */
int asd_match_bow(asd_ctx* ctx, int32_t slot_kf, int32_t slot_f, const asd_feature_vector* fv_kf,
                  const asd_feature_vector* fv_f, const uint8_t* has_mp_kf, float nn_ratio,
                  int32_t check_orientation, int32_t* match_f, int32_t* n_matches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (ORBmatcher.cc:533-666), the
 * loop-closing overload (LoopClosing.cc:304): slot1 / slot2 hold the two keyframes, has_mp1/2[i] = the keyframe has a map point at
 * keypoint i that is not bad.  It differs from the KF-Frame overload above in that a candidate of keyframe 2 needs a map point and
 * must not have been taken yet (vbMatched2, claimed in the reference's visiting order), in the strict threshold bestDist1 < TH_LOW
 * (:609; the other overload has <=, :231), and in that the orientation histogram holds keyframe 1's indices.
 * Output match12[n1] = keypoint index in keyframe 2 whose map point vpMatches12[i1] is, or -1; *n_matches = return value. */
int asd_match_bow_kf(asd_ctx* ctx, int32_t slot1, int32_t slot2, const asd_feature_vector* fv1, const asd_feature_vector* fv2,
                     const uint8_t* has_mp1, const uint8_t* has_mp2, float nn_ratio, int32_t check_orientation,
                     int32_t* match12, int32_t* n_matches);

/* M4: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo=false)
 * (ORBmatcher.cc:669-822): has_mp1 / has_mp2 mark keypoints that already hold a map point,
 * F12[9] row-major f32 fundamental matrix, epipole (ex, ey) of camera 1 in image 2 as computed at
 * :675-683, sigma2 level table of pKF2 comes from the ctx.  Output matches12[n1] = index in
 * KF2 or -1; *n_matches = return value. */
int asd_match_triangulate(asd_ctx* ctx, int32_t slot1, int32_t slot2, const asd_feature_vector* fv1,
                          const asd_feature_vector* fv2, const uint8_t* has_mp1, const uint8_t* has_mp2,
                          const float* F12, float ex, float ey, int32_t check_orientation,
                          int32_t* matches12, int32_t* n_matches);

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th) (ORBmatcher.cc:825-960),
 * search half: for every candidate map point (valid[i] = pMP && !isBad() && !IsInKeyFrame(pKF)) project into
 * the keyframe, apply the depth / viewing-angle / scale gates, search the window and return the keypoint
 * with the smallest descriptor distance among those passing the level and 5.99-chi2 gates.  best_idx[i] = -1
 * when nothing qualifies (bestDist > TH_LOW).  The side effects (Replace / AddObservation / AddMapPoint,
 * :938-956) are asd_fuse_apply over the resident observation table, which takes best_idx as it is returned
 * here (this call, asd_fuse_search_batch, asd_fuse_search_sim3); a caller that keeps its own observation
 * lists performs them itself in map point order (host/fuse_apply.hpp).  They do not influence the search.
 * min_dist / max_dist are the raw mfMinDistance / mfMaxDistance like asd_frustum. */
int asd_fuse_search(asd_ctx* ctx, int32_t slot_kf, int32_t n_mp, const uint8_t* valid, const float* Xw,
                    const float* normal, const float* min_dist, const float* max_dist, const float* desc,
                    const float* Tcw, const float* K, float th, int32_t* best_idx, float* best_dist);

/* LocalMapping::CreateNewMapPoints, per-match body (LocalMapping.cc:386-523, monocular branch): for each
 * match (idx1[i] in frame slot1 = current keyframe, idx2[i] in slot2 = neighbour) run the parallax gate
 * (0 < cos < 0.9998), the linear triangulation (4x4 SVD, :432-450), cheirality in both cameras, the 5.991
 * reprojection gates and the scale-consistency gate (ratioFactor = 1.5*scaleFactor).  ok[i] = 1 and x3D[i]
 * = the new point when the reference would create a MapPoint, else ok[i] = 0 and x3D[i] = 0.  The caller
 * keeps the pointer-graph part (new MapPoint, AddObservation, ComputeDistinctiveDescriptors ->
 * asd_distinctive_descriptor, UpdateNormalAndDepth, :527-542).  Tcw row-major 4x4 f32, K = fx fy cx cy. */
int asd_triangulate_pairs(asd_ctx* ctx, int32_t slot1, int32_t slot2, int32_t n_pairs, const int32_t* idx1,
                          const int32_t* idx2, const float* Tcw1, const float* Tcw2, const float* K1,
                          const float* K2, float* x3D, uint8_t* ok, int32_t* n_ok);
/* ---- the per-keyframe work in front of LocalBA, batched (LocalMapping::DoMapping, LocalMapping.cc:59-113) ----
 * CreateNewMapPoints (:299-545) runs SearchForTriangulation + the per-match triangulation against nn = 20 covisible keyframes,
 * SearchInNeighbors (:557-636) runs Fuse against 20 + second neighbours both ways: 40-100 matcher calls per keyframe, each a
 * few hundred microseconds as a call of its own.  The batch entry points take all of them in ONE submission: one upload, one
 * launch chain, one synchronisation.  What makes that legitimate: inside one call the searches do not feed each other --
 * vbMatched2 is never set in SearchForTriangulation (ORBmatcher.cc:685, :730), Fuse's Replace / AddObservation side effects
 * never enter the search (:938-956) -- and the only coupling BETWEEN the reference's consecutive calls is a filter the caller
 * applies when it walks the results in the reference's order: a keypoint of the current keyframe that an earlier neighbour
 * already gave a map point is skipped for later neighbours (pKF1->GetMapPoint(idx1), ORBmatcher.cc:708-712 after
 * LocalMapping.cc:527-533), a map point an earlier Fuse replaced is bad for later ones (:846-850).  Every result equals the
 * per-pair call's (asd_match_triangulate + asd_triangulate_pairs, asd_fuse_search) bit for bit. */

/* The keyframe's DBoW2::FeatureVector resident beside its descriptors (slot must hold the frame): node ids ascending. */
int asd_frame_set_bow(asd_ctx* ctx, int32_t slot, const asd_feature_vector* fv);

typedef struct asd_kf_neighbor {
  int32_t slot;              /* frame slot of the neighbour keyframe (asd_frame_set + asd_frame_set_bow done) */
  const uint8_t* has_mp;     /* [n_keypoints of that slot] it already holds a map point there */
  float F12[9];              /* fundamental matrix, current keyframe -> neighbour (LocalMapping.cc:638-655), row-major f32 */
  float ex, ey;              /* epipole of the current camera in the neighbour's image (ORBmatcher.cc:675-683) */
  float Tcw[16];             /* the neighbour's pose */
  float K[4];                /* its intrinsics fx fy cx cy */
} asd_kf_neighbor;
/* SearchForTriangulation (check_orientation = false, as LocalMapping.cc:370 calls it) + the per-match triangulation body for
 * every neighbour: matches12[b][i] = keypoint of neighbour b matched to keypoint i of the current keyframe or -1 (has_mp_cur
 * as at entry: see above), x3D[b][i][3] / ok[b][i] as asd_triangulate_pairs returns them for that pair (0 where no match).
 * Arrays are [n_nb][n_cur] row-major. */
int asd_create_map_points_batch(asd_ctx* ctx, int32_t slot_cur, const uint8_t* has_mp_cur, const float* Tcw_cur, const float* K_cur,
                                int32_t n_nb, const asd_kf_neighbor* nb, int32_t* matches12, int32_t* n_matches, float* x3D, uint8_t* ok);

typedef struct asd_fuse_call {
  int32_t slot_kf;           /* target keyframe */
  int32_t first, n;          /* its candidate map points: rows [first, first + n) of the tables below */
  float Tcw[16];
  float K[4];
} asd_fuse_call;
/* asd_fuse_search for n_calls (keyframe, map point list) pairs over shared tables (valid, Xw, normal, min_dist, max_dist,
 * and the map points' descriptors: desc [n_total][128], or desc == NULL and desc_rows [n_total] = rows of the descriptor bank --
 * 4 bytes per point uploaded instead of 512); best_idx / best_dist [n_total] as asd_fuse_search returns them per call. */
int asd_fuse_search_batch(asd_ctx* ctx, int32_t n_calls, const asd_fuse_call* calls, int32_t n_total, const uint8_t* valid, const float* Xw,
                          const float* normal, const float* min_dist, const float* max_dist, const float* desc, const int32_t* desc_rows,
                          float th, int32_t* best_idx, float* best_dist);

/* vt.row(3) of cv::SVD::compute(A, w, u, vt, MODIFY_A|FULL_UV) for n row-major 4x4 f32 matrices
 * (the call at LocalMapping.cc:440); v is [n][4].  Exposed for the parity tests of the SVD itself. */
int asd_svd4_null(asd_ctx* ctx, int32_t n, const float* A, float* v);

/* ---- stereo association (dead code in the reference: no stereo Frame constructor survives) ----
 * Frame::ComputeStereoMatches (Frame.cc:360-535).  The reference keeps two extractors (mpORBextractorLeft / Right,
 * Frame.h), hence two contexts here: extract the left image on ctx_left and the right image on ctx_right (same size,
 * same device), put mvKeys + mDescriptors and mvKeysRight + mDescriptorsRight into two frame slots of ctx_left, then
 * call this before the next extraction overwrites either pyramid.  u_right[N] / depth[N] = mvuRight / mvDepth (-1 =
 * no stereo match); *n_matched = matches that survive the 1.5 * 1.4 * median SAD filter (:517-531).
 * mb = baseline in metres, mbf = baseline * fx. */
/* asd_frame_set(desc == NULL) with the descriptors of src's last extraction instead of ctx's own (both contexts on one device): the
 * right frame of a stereo pair, extracted by its own context, put into a slot of the left one for asd_stereo_match. */
int asd_frame_set_from_ctx(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, int32_t n, float min_x, float max_x, float min_y,
                           float max_y, asd_ctx* src);
/* With the pipelined extractor (asd_extract_submit / asd_extract_wait*) the shared pyramid of a context holds a LATER frame by the
 * time both extractions of a stereo pair have been waited for: asd_extract_keep_pyramid(ctx, 1) makes every submission keep its own
 * copy of its pyramid (one device-to-device copy in the front half), and asd_stereo_match then reads the copies of the submissions
 * waited for last on the two contexts -- valid as long as their descriptors are (two further submissions).  Inside an
 * asd_prep_async bracket of ctx_left the call runs on that context's second stream, beside tracking stages in flight. */
int asd_extract_keep_pyramid(asd_ctx* ctx, int32_t on);
/* Read-ahead extraction on hold: while on != 0 the extractor's workers enqueue no further ASDNet forward (front halves continue, forwards
 * already enqueued finish).  For a caller that runs LocalMapping::DoMapping in line (Tracking.cc:797 -> LocalMapping.cc:59-113): the extractor
 * is told to stand back for the length of asd_local_ba and makes the time up beside the tracking stages.  asd_extract_wait[_view] on a
 * submission that is held ends the hold (it could not return otherwise). */
int asd_extract_hold(asd_ctx* ctx, int32_t on);
int asd_stereo_match(asd_ctx* ctx_left, asd_ctx* ctx_right, int32_t slot_left, int32_t slot_right, float mb, float mbf,
                     float* u_right, float* depth, int32_t* n_matched);

/* ---- optimizer (P1, B1-B5, C1) ------------------------------------------------------- */
/* Optimizer::PoseOptimization (Optimizer.cc:239-413) on g2o's EdgeSE3ProjectXYZOnlyPose
 * (types_six_dof_expmap.h:194-222, .cpp:372-394) with Levenberg
 * (optimization_algorithm_levenberg.cpp:61-189).
 *   pose7: in/out (qx,qy,qz,qw,tx,ty,tz) f64, world->camera, as Converter::toSE3Quat
 *   produces from the f32 Tcw (Converter.cc:37-47);
 *   Xw[n][3], obs[n][2], inv_sigma2[n] as f64 (values are f32-representable);
 *   outlier[n] out (mvbOutlier); *n_inliers = nInitialCorrespondences - nBad. */
int asd_pose_optimize(asd_ctx* ctx, double* pose7, int32_t n, const double* Xw, const double* obs,
                      const double* inv_sigma2, const double* K, uint8_t* outlier, int32_t* n_inliers);

typedef struct asd_ba_problem {
  int32_t n_poses;          /* local + fixed keyframes, ordered by ascending KF id        */
  int32_t n_points;         /* local map points, ordered by ascending MP id               */
  int32_t n_edges;          /* in the reference's insertion order (Optimizer.cc:534-593)  */
  double*        poses;     /* [n_poses][7] in/out (qx,qy,qz,qw,tx,ty,tz)                 */
  const uint8_t* fixed;     /* [n_poses] vSE3->setFixed (Optimizer.cc:490,505)            */
  double*        points;    /* [n_points][3] in/out                                       */
  const int32_t* e_point;   /* [n_edges] point index                                      */
  const int32_t* e_pose;    /* [n_edges] pose index                                       */
  const double*  e_obs;     /* [n_edges][2] kpUn.pt                                       */
  const double*  e_info;    /* [n_edges] information scale (invSigma2, x10 global map)    */
  double K[4];              /* fx, fy, cx, cy                                             */
  int32_t its_first;        /* 5  (Optimizer.cc:602)                                      */
  int32_t its_second;       /* 10 (Optimizer.cc:648)                                      */
} asd_ba_problem;

typedef struct asd_ba_result {
  double*  edge_chi2;        /* [n_edges] final e->chi2()                                 */
  uint8_t* edge_depth_pos;   /* [n_edges] final e->isDepthPositive()                      */
  uint8_t* edge_outlier1;    /* [n_edges] moved to level 1 after the first round          */
  double   chi2_first;       /* active robust chi2 after optimize(its_first)              */
  double   chi2_second;      /* active chi2 after optimize(its_second)                    */
  int32_t  iters_first;      /* LM iterations actually run, as g2o's optimize() returns   */
  int32_t  iters_second;     /* them: -1 for a round without an active vertex (every edge */
                             /* gated out after the first round), no trial, nothing moves  */
} asd_ba_result;

/* Numeric core of Optimizer::LocalBundleAdjustment (Optimizer.cc:484-650): BlockSolver_6_3
 * (block_solver.hpp:354-604) + LinearSolverDense + Levenberg + Huber(sqrt 5.991), two
 * rounds with the chi2 > 5.991 || depth <= 0 gating in between.  The caller applies the
 * erase policy (Optimizer.cc:652-700) from edge_chi2 / edge_depth_pos. */
int asd_local_ba(asd_ctx* ctx, asd_ba_problem* problem, asd_ba_result* result);
/* The same computation on an OPTIONAL lane of the library -- not the reference's order.  In this reference LocalBundleAdjustment
 * runs in line: Tracking::CreateNewKeyFrame -> LocalMapping::DoMapping (Tracking.cc:797, LocalMapping.cc:59-113, the call at
 * :89); there is no mapping thread (LocalMapping::Run, :120, is never started), so frame t+1 is tracked against the map that
 * the keyframe's LocalBA has already rewritten: that is asd_local_ba above.  These entry points offer upstream ORB-SLAM2's
 * concurrent arrangement to an integrator who wants it: _submit hands the problem to a worker thread that runs it on a HIP
 * stream of its own and returns at once; the tracking entry points (asd_extract*, asd_frame_set, asd_match_*, asd_track_*,
 * asd_pose_optimize) may be called meanwhile -- the frames tracked meanwhile read the PRE-BA map, so poses depart from the
 * reference's.  *problem, *result and every array they point to belong to the library until _wait
 * returns; _wait blocks until the run has finished and returns ITS status (results bit-identical to asd_local_ba:
 * same kernels, same order).  One run at a time: a second _submit before _wait, asd_local_ba while a run is outstanding
 * and _wait with nothing submitted return ASD_ERR_INVALID.  asd_local_ba_poll: 0 = idle, 1 = running, 2 = finished and
 * waiting to be collected.  Aborting a run (mbAbortBA) is not offered: a run is ~4 ms. */
int asd_local_ba_submit(asd_ctx* ctx, asd_ba_problem* problem, asd_ba_result* result);
int asd_local_ba_wait(asd_ctx* ctx);
int asd_local_ba_poll(asd_ctx* ctx);

/* ---- full bundle adjustment ------------------------------------------------------------ */
typedef struct asd_gba_problem {
  int32_t n_poses;          /* keyframes, ordered by ascending KF id (Optimizer.cc:72-89)          */
  int32_t n_points;         /* map points, ordered by ascending MP id (:96-107)                    */
  int32_t n_edges;          /* in the caller's insertion order (:112-151: grouped by point)        */
  double*        poses;     /* [n_poses][7] in/out (qx,qy,qz,qw,tx,ty,tz)                          */
  const uint8_t* fixed;     /* [n_poses] vSE3->setFixed(pKF->mnId == 0) (:84); any mask is honoured */
  double*        points;    /* [n_points][3] in/out                                                */
  const int32_t* e_point;   /* [n_edges] point index                                               */
  const int32_t* e_pose;    /* [n_edges] pose index                                                */
  const double*  e_obs;     /* [n_edges][2] kpUn.pt (:121-125)                                     */
  const double*  e_info;    /* [n_edges] invSigma2 (:133-134)                                      */
  double K[4];              /* fx, fy, cx, cy                                                      */
  int32_t n_iterations;     /* nIterations (:173)                                                  */
  int32_t robust;           /* bRobust (:136-141): 1 = Huber, delta = (float)sqrt(5.99) (:91 --    */
                            /* NOT LocalBA's 5.991); 0 = no kernel                                 */
  const volatile int32_t* stop;   /* pbStopFlag (:66-67); NULL = none                              */
} asd_gba_problem;

typedef struct asd_gba_result {
  double*  edge_chi2;       /* [n_edges] e->chi2() of the stored errors                            */
  double   chi2;            /* activeRobustChi2() of the stored errors, as asd_local_ba reports it */
  int32_t  iterations;      /* what g2o's optimize() returns: iterations run, -1 without an active */
                            /* vertex (no edge)                                                    */
  int32_t  trials;          /* solves, accepted and rejected                                       */
} asd_gba_result;

/* Numeric core of Optimizer::BundleAdjustment (Optimizer.cc:51-237; GlobalBundleAdjustemnt, :43-48, only collects its vectors):
 * the graph of :57-162, then ONE round, initializeOptimization(); optimize(n_iterations) (:172-173) -- Levenberg with g2o's schedule
 * (optimization_algorithm_levenberg.cpp:61-189), no outlier gating, no levels.  The caller of Tracking::CreateInitialMapMonocular
 * (Tracking.cc:472-570: GlobalBundleAdjustemnt(mpMap, 20) behind Initializer::Initialize) and of
 * LoopClosing::RunGlobalBundleAdjustment needs nothing else from g2o.  Poses and points are written in place.
 *   - A point without an edge is legal (the reference removes such a vertex, :153-157) and comes back untouched; so does a free pose
 *     without an edge (its quaternion normalised, as SE3Quat's constructor does for every pose).
 *   - n_edges == 0: iterations = -1, nothing moves (sparse_optimizer.cpp:356-359).  Edges but no free pose among their keyframes:
 *     ASD_ERR_INVALID -- the reference does not return, it stops on an assertion of BlockSolver::resize (block_solver.hpp:75).
 *   - stop: read by the HOST before each chunk of four Levenberg trials is enqueued, never by the device.  Set on entry: the call is
 *     that of n_iterations = 0 -- iterations = 0, the estimates as given (quaternions normalised), chi2 / edge_chi2 of the errors at
 *     them.  Set later: the trials already enqueued finish, the iteration in progress is abandoned, the last ACCEPTED estimate
 *     comes back with the errors at it and the iterations completed so far.  (g2o looks at the flag in front of every iteration,
 *     sparse_optimizer.cpp:376; this reference is single-threaded, so there the flag cannot change during a call.)
 *   - The reduced pose system (n = 6 x free poses with an edge) is solved densely in f64.  Up to ASD_GBA_TILED_FROM - 1 such poses
 *     by LocalBA's single-workgroup solvers; from there on by a tiled Cholesky over the whole chip (csrc/gba.hip: tiles of 96 rows =
 *     16 pose blocks, the trailing update on v_mfma_f64_16x16x4_f64).  Environment ASD_GBA_SOLVE=tiled|single, read at
 *     asd_ctx_create, forces one form.  A pivot that is not positive fails the trial's solve: the trial is rejected and lambda grows,
 *     which is what g2o does when LinearSolverEigen / LinearSolverDense report a failed factorisation (linear_solver_eigen.h:
 *     105-110: solve() returns false when the LLT did not succeed; optimization_algorithm_levenberg.cpp:126-127 sets tempChi to the
 *     largest double, rho < 0).
 *   - Pinned against the reference's g2o with its own solver (BlockSolverX + LinearSolverEigen) in tests/test_gba.py: iterations
 *     and trials per iteration exact, the estimates within 4 x S, S = the distance between three reference runs (two roundings of
 *     the sparse solver and the dense one; tests/golden/make_gba_golden.py).
 * Limits (ASD_ERR_CAPACITY beyond them, asd_last_error says which): ASD_GBA_MAX_FREE_POSES free poses, ASD_GBA_MAX_EDGES edges,
 * ASD_GBA_MAX_POINTS points.  The partial-sum limit of asd_local_ba's control does not apply.
 * ASD_ERR_INVALID while a run of asd_local_ba_submit or a call started with asd_track_async is outstanding: they share the
 * solver's device buffers.  asd_local_ba before and after returns the bits it returns without this call. */
#define ASD_GBA_MAX_FREE_POSES 2048
#define ASD_GBA_MAX_EDGES (4 * 1024 * 1024)
#define ASD_GBA_MAX_POINTS (2 * 1024 * 1024)
#define ASD_GBA_TILED_FROM 40
int asd_bundle_adjustment(asd_ctx* ctx, asd_gba_problem* problem, asd_gba_result* result);
/* Test aid: the forms of the context's last asd_bundle_adjustment.  out = {dense solve: 0 = k_ba_solve_lds, 1 = k_ba_chol_lds,
 * 2 = k_ba_chol (the single-workgroup solvers, by size as in asd_debug_local_ba_forms), 3 = the tiled Cholesky, -1 = none (no edge);
 * nPf, nLa, Ea: free poses, landmarks and edges of the active structure; tiles per side of the tiled form (ceil(nPf / 16)), 0 for
 * the other forms}.  All -1 before any call. */
int32_t asd_debug_gba_forms(const asd_ctx* ctx, int32_t out[5]);
/* Test aid: the trials (solves, accepted and rejected) each iteration of the context's last asd_bundle_adjustment took, as g2o's
 * levenbergIteration() reports them behind an iteration.  Writes min(cap, iterations) values, -1 behind them; returns the number
 * of iterations recorded (0 before any call, and for a call that ran none). */
int32_t asd_debug_gba_trials(const asd_ctx* ctx, int32_t* out, int32_t cap);
/* Test aid: ONE dense symmetric positive-definite solve A x = b in f64 by the kernel every optimiser ends in, launched as the
 * production call sites launch it (tests/test_dense_solve.py).  form: 0 = k_ba_solve_lds (n = 6 x 1 .. 30 pose blocks; A is packed
 * on the host the way k_ba_schur leaves it), 1 = k_ba_chol_lds (6 x 1 .. 32), 2 = k_ba_chol (6 x 1 .. ASD_GBA_MAX_FREE_POSES),
 * 3 = the tiled Cholesky with its trailing update on f64 MFMA, 4 = the same on plain FMA (any n up to 7 x ASD_GBA_MAX_FREE_POSES).
 * A: host, row-major n x n, the lower triangle is the matrix.  b: [n].  done_in / chol_ok_in: what the kernels find in the
 * Levenberg state's `done` and `chol_ok` (done_in != 0: every kernel returns at once).  x_out [n]: uploaded as given, comes back
 * as the kernel left it.  L_out: null, or [n][n] -- forms 2 .. 4: the matrix as the kernel left it (L in the lower triangle);
 * forms 0 and 1 keep theirs in LDS and do not write it.  *chol_ok_out: the flag afterwards (0: a pivot was not positive; the call
 * still returns ASD_OK).  ASD_ERR_INVALID for a size the form does not take and while a run of asd_local_ba_submit is outstanding.
 * Allocates per call; not for a hot path. */
int32_t asd_debug_dense_solve(asd_ctx* ctx, int32_t form, int32_t n, const double* A, const double* b, int32_t done_in,
                              int32_t chol_ok_in, double* L_out, double* x_out, int32_t* chol_ok_out);
/* Test aid: ONE call of one fp64 primitive of csrc/se3.h / csrc/sim3_math.h per item (tests/test_prims.py).  in: host, n items of
 * the op's input width; out: host, n items of its output width (doubles, in the order of the function's arguments; a Pose7 is
 * qx qy qz qw tx ty tz, a Sim3d is qx qy qz qw tx ty tz s, matrices are row-major).  One launch of a 64-thread-per-block kernel on
 * the context's stream, one lane per item, then a synchronise.
 *   op                              in                                            out
 *    0 asd_rsqrt                     1  x                                          1
 *    1 quat_normalize                4  x y z w                                    4  x y z w
 *    2 quat_rotate                   7  qx qy qz qw, v[3]                          3
 *    3 pose_map                     10  Pose7, X[3]                                3
 *    4 pose_oplus                   13  Pose7, u[6] = (omega, upsilon)             7  Pose7
 *    5 rot_to_quat_eigen             9  R                                          4  x y z w
 *    6 huber                         2  e2, delta                                  2  rho0, rho1
 *    7 jac_pose                      5  x y z fx fy                               12  J
 *    8 s3_exp<false>   9 <true>      7  u = (omega, upsilon, sigma)                8  Sim3d
 *   10 s3_log                        8  Sim3d                                      7
 *   11 s3_mul<false>  12 <true>     16  Sim3d a, Sim3d b                           8  Sim3d
 *   13 s3_inverse                    8  Sim3d                                      8  Sim3d
 *   14 s3_map                       11  Sim3d, v[3]                                3
 *   15 s3_oplus<false> 16 <true>    16  Sim3d est, u[7], fix_scale (0 or not)      8  Sim3d
 *   17 s3_quat_of_rot<false> 18 <true> 9  R                                        4  x y z w
 *   19 s3_rot_of_quat                8  Sim3d (the quaternion is read)             9  R
 *   20 s3_lu_solve3                 12  W, t[3]                                    3
 *   21 s3_edge_error                24  Sim3d C, Si, Sj                            7
 *   22 s3_project_error             17  Sim3d, X Y Z, ou ov, fx fy cx cy           2
 *   23 s3_chi2                       3  e0 e1 inv_sigma2                           1
 *   24 s3_solve7                    57  H[49], lambda, b[7]                        8  ok (1 or 0), x[7]
 * flags: ASD_PRIM_HOST -- run on the host instead, through the same header functions (ctx may then be NULL; no device is touched);
 * ASD_PRIM_FUSED_BUILD -- the instantiation compiled with the flags of ba.o / gba.o (contraction allowed) instead of
 * -ffp-contract=off; it holds ops 0 .. 7 only.  ASD_ERR_INVALID for an unknown op or flag bit, n < 0 and null pointers; n = 0
 * returns ASD_OK and launches nothing.  Allocates per call; not for a hot path. */
enum {
  ASD_PRIM_RSQRT = 0, ASD_PRIM_QUAT_NORMALIZE, ASD_PRIM_QUAT_ROTATE, ASD_PRIM_POSE_MAP, ASD_PRIM_POSE_OPLUS, ASD_PRIM_ROT_TO_QUAT_EIGEN,
  ASD_PRIM_HUBER, ASD_PRIM_JAC_POSE, ASD_PRIM_SE3_OPS,
  ASD_PRIM_S3_EXP = ASD_PRIM_SE3_OPS, ASD_PRIM_S3_EXP_EIGEN, ASD_PRIM_S3_LOG, ASD_PRIM_S3_MUL, ASD_PRIM_S3_MUL_EIGEN, ASD_PRIM_S3_INVERSE,
  ASD_PRIM_S3_MAP, ASD_PRIM_S3_OPLUS, ASD_PRIM_S3_OPLUS_EIGEN, ASD_PRIM_S3_QUAT_OF_ROT, ASD_PRIM_S3_QUAT_OF_ROT_EIGEN,
  ASD_PRIM_S3_ROT_OF_QUAT, ASD_PRIM_S3_LU_SOLVE3, ASD_PRIM_S3_EDGE_ERROR, ASD_PRIM_S3_PROJECT_ERROR, ASD_PRIM_S3_CHI2, ASD_PRIM_S3_SOLVE7,
  ASD_PRIM_OPS
};
#define ASD_PRIM_HOST 1
#define ASD_PRIM_FUSED_BUILD 2
int32_t asd_debug_prim(asd_ctx* ctx, int32_t op, int32_t flags, int32_t n, const double* in, double* out);

/* ---- essential graph (Sim3 pose graph of a loop closure) --------------------------------- */
typedef struct asd_essgraph_problem {
  int32_t n_kf;             /* keyframes, ordered by ascending mnId (Optimizer.cc:765-800)                          */
  int32_t n_edges;          /* in the caller's insertion order (:808-939)                                          */
  double*        sim3;      /* [n_kf][8] in/out (qx,qy,qz,qw,tx,ty,tz,s).  On entry vScw: CorrectedSim3 where the   */
                            /* keyframe has one, else (Rcw, tcw, 1) (:774-788)                                     */
  const uint8_t* fixed;     /* [n_kf] pKF == pLoopKF (:790); any mask is honoured                                  */
  const int32_t* e_i;       /* [n_edges] row of vertex 0 (:827)                                                    */
  const int32_t* e_j;       /* [n_edges] row of vertex 1 (:826)                                                    */
  const double*  e_meas;    /* [n_edges][8] Sji (:823, :870, :897, :928); the information is the identity (:805)   */
  int32_t fix_scale;        /* bFixScale (:795)                                                                    */
  int32_t n_iterations;     /* the reference: 20 (:943)                                                            */
  /* optional tail (:947-999) */
  float*         Tcw_out;   /* [n_kf][16] or NULL: [R t/s; 0 1] as float, row major (:957-963)                     */
  int32_t n_mp;             /* map points to correct (0: none)                                                     */
  const int32_t* mp_ref;    /* [n_mp] row of the keyframe the point is corrected through: the caller applies the   */
                            /* mnCorrectedByKF rule of :976-985                                                    */
  float*         mp_Xw;     /* [n_mp][3] in/out: correctedSwr.map(Srw.map(X)) in f64, stored as float (:988-996)   */
} asd_essgraph_problem;

typedef struct asd_essgraph_result {
  double*  edge_chi2;       /* [n_edges] e->chi2() of the stored errors                                            */
  double   chi2;            /* activeChi2() of the stored errors                                                   */
  int32_t  iterations;      /* what g2o's optimize() returns: iterations run, -1 without an active vertex (no edge) */
  int32_t  trials;          /* solves, accepted and rejected                                                       */
} asd_essgraph_result;

/* Numeric core of Optimizer::OptimizeEssentialGraph (Optimizer.cc:737-1000), which LoopClosing::CorrectLoop calls at
 * LoopClosing.cc:587: a VertexSim3Expmap per keyframe, an EdgeSim3 per edge, initializeOptimization(); optimize(n_iterations), then
 * the pose recovery and the map-point correction.  Which edges there are and what they measure (:808-939) is the caller's part
 * (host/asd_adapters.hpp: asd::Optimizer::OptimizeEssentialGraph); with this call nothing in the reference's Tracking, LocalMapping
 * or LoopClosing needs g2o.
 *   - Error: EdgeSim3::computeError, log(C * S_i * S_j^-1) (types_seven_dof_expmap.h:106-114), f64.
 *   - Jacobians: g2o's numeric ones (base_binary_edge.hpp:130-206): central differences, delta = 1e-9, through oplusImpl =
 *     Sim3(update) * estimate with update[6] = 0 under fix_scale (types_seven_dof_expmap.h:60-69).  No Jacobian for a fixed vertex.
 *   - Levenberg: setUserLambdaInit(1e-16) (:750) and g2o's schedule (optimization_algorithm_levenberg.cpp:61-189); no robust kernel,
 *     no stop flag.  The system of the free vertices that have an edge (n = 7 x their number) is factored densely in f64 by the
 *     tiled Cholesky of asd_bundle_adjustment (csrc/gba.hip) at every size; a pivot that is not positive rejects the trial.
 *   - A keyframe without an edge is not an active vertex and comes back untouched (the Sim3 constructors of the reference, sim3.h:
 *     59-67, store the quaternion as given: no vertex is renormalised on entry).  Fixed vertices come back untouched as well.
 *   - n_edges == 0: iterations = -1, nothing moves (sparse_optimizer.cpp:356-359); the tail still runs, with the entry estimates.
 *     Edges but no free vertex among them: ASD_ERR_INVALID.  An edge naming a row outside [0, n_kf), or i == j: ASD_ERR_INVALID.
 *     Duplicate (i, j) pairs are legal and both count (the reference produces them when a spanning-tree or loop edge coincides with
 *     a LoopConnections edge: sInsertedEdges only guards the covisibility edges).
 *   - chi2 / edge_chi2 are those of the stored errors, i.e. of the last computeActiveErrors: after a run that ended on a rejected
 *     trial, the rejected trial's (the estimates are the accepted ones).  n_iterations = 0: the errors at the entry estimates.
 *   - Everything is f64 without float atomics: two calls on one problem return the same bits.
 *   - Pinned against the reference's g2o (BlockSolver_7_3 + LinearSolverEigen) in tests/test_essgraph.py: iterations and trials per
 *     iteration exact, the estimates within 4 x S (tests/golden/make_essgraph_golden.py).
 * Limits (ASD_ERR_CAPACITY beyond them, asd_last_error says which): ASD_ESSGRAPH_MAX_KEYFRAMES keyframes, ASD_ESSGRAPH_MAX_EDGES
 * edges, ASD_ESSGRAPH_MAX_POINTS map points, ASD_ESSGRAPH_MAX_ITERATIONS iterations (a count below 0 is taken as 0).  ASD_ERR_INVALID while a run of asd_local_ba_submit or a call started with
 * asd_track_async is outstanding.  asd_local_ba and asd_bundle_adjustment before and after return the bits they return without
 * this call. */
#define ASD_ESSGRAPH_MAX_KEYFRAMES 2048
#define ASD_ESSGRAPH_MAX_EDGES (64 * 1024)
#define ASD_ESSGRAPH_MAX_POINTS (4 * 1024 * 1024)
#define ASD_ESSGRAPH_MAX_ITERATIONS 1000
int asd_optimize_essential_graph(asd_ctx* ctx, asd_essgraph_problem* problem, asd_essgraph_result* result);
/* Test aid: the structure of the context's last asd_optimize_essential_graph.  out = {active vertices (keyframes with an edge, fixed
 * ones included), free active vertices (n / 7), active edges, tiles per side of the Cholesky (ceil(n / 96), 0 without a solve)}.
 * All -1 before any call. */
int32_t asd_debug_essgraph_forms(const asd_ctx* ctx, int32_t out[4]);
/* Test aid: the trials each iteration of the context's last asd_optimize_essential_graph took, as asd_debug_gba_trials. */
int32_t asd_debug_essgraph_trials(const asd_ctx* ctx, int32_t* out, int32_t cap);

/* Converter::toSE3Quat / toCvMat (Converter.cc:37-71): f32 4x4 <-> f64 quaternion + t. */
int asd_tcw_to_pose7(const float* Tcw16, double* pose7);
int asd_pose7_to_tcw(const double* pose7, float* Tcw16);

/* ---- instrumentation ----------------------------------------------------------------- */
/* Device-side duration of the kernels enqueued by the most recent call of the named stage,
 * measured with hipEvents on the ctx stream.  stage: "asdnet", "extract", "match", "ba", "sim3" (asd_optimize_sim3),
 * "sim3_ransac" (both kernels of asd_sim3_ransac, its upload included), "pnp_ransac" (likewise for asd_pnp_ransac), "initializer" (likewise for asd_initialize; "initializer_hyp": its upload and k_init_hyp alone),
 * "kfdb" (the scoring pass of the last asd_kfdb_score / asd_kfdb_query_*, its upload included), "essgraph" (asd_optimize_essential_graph:
 * every kernel of the call, the tail included; the host's looks at the Levenberg state lie inside). */
int asd_last_stage_ms(const asd_ctx* ctx, const char* stage, float* ms);
/* Per-kernel device time of the ASDNet forward, accumulated with hipEvents recorded on the ctx
 * stream between the layer launches of every forward while enabled.  layer 0 = input_norm+conv1,
 * 1..5 = conv2..conv6 (MFMA implicit GEMM), 6 = 8x8 conv (split-K GEMM), 7 = reduce+L2Norm. */
int asd_profile_enable(asd_ctx* ctx, int32_t on);
int asd_profile_get(asd_ctx* ctx, int32_t layer, double* total_ms, int32_t* calls, int64_t* patches);
/* Which ASDNet layers run on the split-operand kernels: bit 0 = conv2 ... bit 4 = conv6, bit 5 = the 8x8 conv.
 * Both kernel families compute in f32: the split kernels write every f32 operand exactly as the sum of three bf16 terms
 * and accumulate the six significant cross products in f32 on the bf16 matrix pipe (error at the level of the f32 MFMA chain,
 * see asdnet.hip); the others use v_mfma_f32_32x32x2_f32.  Chosen at asd_ctx_create: environment ASD_ASDNET_MATH=f32 clears
 * every bit; default all layers split (0x3f). */
int32_t asd_asdnet_split_mask(const asd_ctx* ctx);
/* How the split-operand 3x3 conv kernels carry an f32 operand (chosen at asd_ctx_create by ASD_ASDNET_MATH):
 *   2  ("f16x2", the default; "split" is an alias)  x 2^k = h + l with two fp16 terms (22 significant bits), the three products
 *      l h, h l, h h accumulated in f32 on the f16 matrix pipe; against a float64 forward the descriptors are as close as those
 *      of the f32 MFMA chain (tests/test_asdnet.py).  Activations must stay below 4094 in magnitude (BatchNorm keeps them O(1)).
 *      Two guards: asd_load_weights runs a calibration batch (64 synthetic patches: noise, edges, checkerboards, ramps, dots)
 *      and, if any layer's largest activation leaves less than a factor two of headroom (> 2048), switches this context to
 *      the three-piece form below (asd_asdnet_pieces then reports 3, asd_last_error says why); and a descriptor that comes out
 *      non-finite at run time raises a device flag: asd_describe / asd_extract* / asd_extract_wait* return ASD_ERR_RANGE for
 *      that call (asd_describe_device, which does not synchronise, reports it from the next asd_sync) -- the reference's f32
 *      libtorch path (ORBextractor.cc:1127-1132) has no such failure mode, so it is an error here, never a silent NaN.
 *   3  ("bf16x3")  exact sum of three bf16 terms, six products; no range restriction; 1.35x the ASDNet time of the default. */
int32_t asd_asdnet_pieces(const asd_ctx* ctx);
/* what the calibration pass of the last asd_load_weights found ("" = nothing to report; non-empty when it switched the context to
 * the three-piece form).  A note on a successful call: asd_last_error is not touched by it. */
const char* asd_calibration_note(const asd_ctx* ctx);
/* Raw handles for harnesses that keep inputs resident (bench.py): the ctx stream
 * (hipStream_t) and device scratch. */
void* asd_ctx_stream(asd_ctx* ctx);
int asd_device_alloc(asd_ctx* ctx, uint64_t bytes, void** dptr);
int asd_device_free(asd_ctx* ctx, void* dptr);
/* page-locked host memory (an image buffer handed to asd_extract_submit(device_resident = 0) from here is copied by the front
 * half's stream without a staging pass) */
int asd_host_alloc(asd_ctx* ctx, uint64_t bytes, void** hptr);
int asd_host_free(asd_ctx* ctx, void* hptr);
int asd_memcpy_h2d(asd_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int asd_memcpy_d2h(asd_ctx* ctx, void* dst, const void* src, uint64_t bytes);
int asd_sync(asd_ctx* ctx);
/* Test aid: MapPoint::PredictScale (MapPoint.cc:438-453) is evaluated on the device by comparing the distance ratio with
 * per-level thresholds derived from the host's logf at asd_ctx_create; this sweeps EVERY float in [lo, hi] and returns the
 * number of ratios for which the comparison rule and ceil(logf(r) / logf(scaleFactor)) (clamped) disagree (expected 0). */
int32_t asd_debug_level_sweep(const asd_ctx* ctx, float lo, float hi, int64_t* n_checked);
/* Test aid: which forms the last asd_local_ba (or the run collected by asd_local_ba_wait; not valid while a run is outstanding)
 * took in each of its two rounds.  out[round] = {dense solve of the reduced pose system: 0 = k_ba_solve_lds (nPf <= 30),
 * 1 = k_ba_chol_lds (31-32), 2 = k_ba_chol (>= 33), -1 = none (no free pose with an active edge); active structure:
 * 0 = built on the device, 1 = built on the host; nPf, nLa, Ea: free poses, landmarks and edges of the active structure}.
 * The structure is built once, for round 0: round 1 runs over it with its level-1 edges masked, so its values repeat round 0's.
 * All -1 before any run, and for a round that did not start. */
int32_t asd_debug_local_ba_forms(const asd_ctx* ctx, int32_t out[2][5]);
/* Test aid: how the Levenberg rounds of the last asd_local_ba (or of the run collected by asd_local_ba_wait; not valid while a
 * run is outstanding) went.  out[round] = {iterations done (the round's iters_first / iters_second), trials (solves, accepted
 * and rejected), trial blocks enqueued (the blocks behind the round's end are no-ops), length of the first chunk of blocks
 * (the trials the same round of the context's previous LocalBA took, else its_first / its_second; 0 when no block ran)}.
 * Read from host-side bookkeeping: it adds no work to a run.  All -1 before any run, and for a round that did not start. */
int32_t asd_debug_local_ba_lm(const asd_ctx* ctx, int32_t out[2][4]);
/* Test aid: what the solver of the context's last asd_pose_optimize did.  out[0] = the edge store it took (2 = compact LDS,
 * 1 = full f64 LDS, 0 = global memory; -1 for a call with fewer than 3 edges, which runs no solver), then ten values per round
 * of Optimizer.cc:335-403, out[1 + 10 r + k]: {state: 0 = ran, 1 = not run because the previous re-classification changed no flag
 * (the round would repeat the one before it), -1 = not reached (fewer than 10 edges); active edges; Levenberg iterations; trials
 * (solves, accepted and rejected); passes over the edges; passes that re-evaluated the current pose after an iteration that ended
 * on a rejected trial without ending the round; trials whose 6x6 system was not positive definite; nBad of the re-classification;
 * 1 if the round ended on a rejected trial (the re-classification then reads the inliers' errors at the rejected pose);
 * iterations that rejected a trial and were followed by another iteration}.  A round that was not run reports the numbers of the
 * round it repeats; a round that was not reached reports -1 throughout.  Written by one thread of the stand-alone solver behind
 * the outlier flags of the block the call copies back anyway; the fused tracking chains (asd_track_*) do not write it and do not
 * change it.  All -1 before any run. */
#define ASD_POSE_OPT_DEBUG_INTS 41
int32_t asd_debug_pose_opt(const asd_ctx* ctx, int32_t out[ASD_POSE_OPT_DEBUG_INTS]);
/* Optimizer::OptimizeSim3 (Optimizer.cc:1002-1194) on g2o's VertexSim3Expmap, EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ
 * (types_seven_dof_expmap.h:48-193) with their NUMERIC Jacobians (base_binary_edge.hpp:130-206, delta = 1e-9), Levenberg as in
 * asd_pose_optimize: optimize(5) over all 2 n edges, pairs with chi2 > th2 on either edge dropped (the errors as the round's last
 * evaluation left them, :1146), optimize(nBad > 0 ? 10 : 5) over the rest, final count.
 *  sim3[8]  in/out  qx qy qz qw tx ty tz s  (g2oS12), f64
 *  n pairs (<= 65535) = the correspondences the reference adds edges for (:1065-1131), in ascending i:
 *  P1c[n][3] = R1w*P3D1w + t1w, P2c[n][3] likewise (f64, f32-representable), obs1/obs2[n][2] = mvKeysUn pt,
 *  inv_sigma2_1/2[n], K1[4], K2[4] = fx fy cx cy, th2 (10 in the reference, LoopClosing.cc:362), fix_scale.
 *  keep[n] out: 1 = vpMatches1[idx] still set on return; *n_in = return value.
 * Where nCorrespondences - nBad < 10 after the first round (:1164) the reference returns 0 in front of :1191: *n_in = 0, keep
 * carries the first round's drops and sim3 is NOT written.  n == 0 is that case (g2o's optimize() returns -1 on the empty graph).
 * The result is one bit pattern over repeated calls.  Against the reference's own g2o it agrees as far as two builds of that g2o
 * agree with each other (tests/golden/make_sim3_golden.py): the numeric Jacobians put the noise floor near 1e-7, not 1e-8. */
int asd_optimize_sim3(asd_ctx* ctx, double* sim3, int32_t n, const double* P1c, const double* P2c, const double* obs1,
                      const double* obs2, const double* inv_sigma2_1, const double* inv_sigma2_2, const double* K1,
                      const double* K2, float th2, int32_t fix_scale, uint8_t* keep, int32_t* n_in);
/* Test aid: what the context's last asd_optimize_sim3 did.  out[4 r + k], r = round 0 / 1: {active edges, Levenberg iterations
 * (optimize()'s return value: -1 with no active edge), trials (solves, accepted and rejected), 1 if the round's last trial was
 * rejected}, -1 throughout for a second round that did not run; out[8] = nBad of the first re-classification, out[9] = the second
 * round's iteration cap (5 or 10, :1158-1162; chosen in front of the early return), out[10] = 1 on the early return of :1165,
 * out[11] = n.  Written by one thread into the block the call copies back anyway.  All -1 before any run. */
#define ASD_SIM3_OPT_DEBUG_INTS 12
int32_t asd_debug_optimize_sim3(const asd_ctx* ctx, int32_t out[ASD_SIM3_OPT_DEBUG_INTS]);
/* Sim3Solver (src/vslam/src/Sim3Solver.cc): the RANSAC loop of Sim3Solver::iterate (:140-207) for a batch of solvers, the hypotheses of
 * every solver in parallel.  One problem = one Sim3Solver and one iterate() call on it:
 *  in      n                       N = mvX3Dc1.size(), the correspondences the constructor gathered (:62-103)
 *          X1c[n][3], X2c[n][3]    mvX3Dc1 / mvX3Dc2 = Rcw * Xw + tcw per keyframe (:94-98), f32
 *          max_err1[n], max_err2[n] mvnMaxError1 / 2: 9.210 * sigma2 of the keypoint's level (:87-88) as the caller's vectors hold it -- the
 *                                  reference's are vector<size_t> (Sim3Solver.h:78-79), so it compares with the integer part (:356)
 *          K1[4], K2[4]            fx fy cx cy of mK1 / mK2 (:105-106)
 *          fix_scale               mbFixScale (:292, :311)
 *          min_inliers             mRansacMinInliers (:118)
 *          n_iter                  the iterations this call may run: min(nIterations, mRansacMaxIts - mnIterations) (:158)
 *          draws[n_iter][3]        draws[k][i] = what RandomInt(0, n - 1 - i) returned for draw i of iteration k (:168); the swap-with-back
 *                                  bookkeeping of vAvailableIndices (:163-177) is done by the device
 *  in/out  best_inliers            mnBestInliers (:183-186)
 *  out     best_updated            1 when an iteration of this call took over the best model (:183); only then are written
 *          R12[9], t12[3], s12,    mBestRotation, mBestTranslation, mBestScale, mBestT12 (:187-190), row major
 *          T12[16]
 *          found                   1 when iterate() returns a model (:192-199), 0 when it returns cv::Mat() (:206)
 *          iterations_done         how many of the n_iter supplied iterations the reference would have run: k + 1 when iteration k
 *                                  returns, n_iter otherwise -- what the caller adds to mnIterations, and 3 x that many draws were consumed
 *          n_inliers               nInliers (:194), 0 unless found
 *          inliers[n]              mvbInliersi of the returned iteration (:195-197, indexed by correspondence: the caller maps through
 *                                  mvnIndices1), all 0 unless found (:143)
 * A problem with n < min_inliers runs nothing (:146-150): found = 0, iterations_done = 0 and nothing else of it is written.
 * The model of an iteration (ComputeSim3, :226-337) is evaluated in f64 from the f32 points -- centroids, M = Pr2 * Pr1^T, Horn's N (:251-260),
 * its top eigenvector by cyclic Jacobi, the rotation directly from that unit quaternion (the reference's atan2 / angle-axis / cv::Rodrigues
 * chain, :274-284, gives the same rotation for either sign of the eigenvector), scale (:292-311), translation (:316), T12 and T21 (:321-336) --
 * and every output is rounded to f32 once, since the reference keeps them as CV_32F.  It is the reference's formula, not cv::eigen's bits:
 * an entry is within 0.5 ulp + 32 * eps64 * cond of the exact value, cond = |N|_2 / (lambda1 - lambda2) (tests/sim3solver_ref.py).
 * CheckInliers / Project (:340-403) and FromCameraToImage (:405-423) run in un-fused f32 in the reference's operation order on those f32
 * matrices; a non-finite model or projection is never an inlier (both comparisons of :356 are false), as in the reference.
 * Limits (ASD_ERR_CAPACITY beyond them): ASD_SIM3_RANSAC_MAX_N correspondences per problem, ASD_SIM3_RANSAC_MAX_PROBLEMS problems per call,
 * ASD_SIM3_RANSAC_MAX_HYPOTHESES iterations per call summed over its problems.  ASD_ERR_INVALID: a draw outside [0, n - 1 - i], n < 3 in a
 * problem that has iterations to run, a null array, negative n / n_iter; asd_last_error names the problem.  Two kernel launches and one
 * synchronisation per call, no atomics: a call is one bit pattern.  Legal wherever asd_optimize_sim3 is. */
#define ASD_SIM3_RANSAC_MAX_N 8192
#define ASD_SIM3_RANSAC_MAX_PROBLEMS 64
#define ASD_SIM3_RANSAC_MAX_HYPOTHESES 4096
typedef struct asd_sim3_ransac_problem {
  int32_t n;
  const float* X1c;
  const float* X2c;
  const float* max_err1;
  const float* max_err2;
  float K1[4], K2[4];
  int32_t fix_scale, min_inliers, n_iter;
  const int32_t* draws;
  int32_t best_inliers;
  int32_t best_updated;
  float R12[9], t12[3], s12, T12[16];
  int32_t found, iterations_done, n_inliers;
  uint8_t* inliers;
} asd_sim3_ransac_problem;
int asd_sim3_ransac(asd_ctx* ctx, int32_t n_problems, asd_sim3_ransac_problem* problems);
/* Sim3Solver::SetRansacParameters (:114-138), the value it leaves in mRansacMaxIts: epsilon = (float)min_inliers / n as a float,
 * pow(epsilon, 3) and both log() in double, ceil, the conversion to int (a value that does not fit an int -- epsilon = 0 or > 1 -- converts
 * as x86-64 does, to INT_MIN), max(1, min(., max_iterations)); 1 iteration when min_inliers == n (:130-131).  Host only, no context. */
int32_t asd_sim3_ransac_max_iterations(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations);
/* Test aid: one iteration of the context's last asd_sim3_ransac: the three sampled correspondences (:163-177), mnInliersi (:346-363),
 * mT12i / mT21i / ms12i as f32 (:308-336) and the f64 unit quaternion (w x y z) the rotation was made from.  Copied back with the
 * block the call reads anyway.  ASD_ERR_INVALID for a (problem, hypothesis) the last call did not run. */
typedef struct asd_sim3_ransac_debug {
  int32_t idx[3];
  int32_t count;
  float T12[16], T21[16], s;
  double q[4];
} asd_sim3_ransac_debug;
int32_t asd_debug_sim3_ransac(const asd_ctx* ctx, int32_t problem, int32_t hypothesis, asd_sim3_ransac_debug* out);
/* PnPsolver (src/vslam/src/PnPsolver.cc): the EPnP RANSAC loop of PnPsolver::iterate (:165-258) for a batch of solvers, the hypotheses of
 * every solver in parallel -- the step of Tracking::Relocalization (Tracking.cc:1156-1174) between SearchByBoW and PoseOptimization.  One
 * problem = one PnPsolver and one iterate() call on it:
 *  in      n                       N = mvP2D.size(), the correspondences the constructor gathered (:67-101, :129)
 *          P3Dw[n][3]              mvP3Dw (:93), f32
 *          P2D[n][2]               mvP2D = mvKeysUn[i].pt (:89), f32
 *          max_err[n]              mvMaxError = mvSigma2[i] * th2, the product taken in f32 (:156)
 *          K[4]                    fu fv uc vc (:104-107)
 *          min_inliers             mRansacMinInliers AFTER SetRansacParameters (:139; asd_pnp_ransac_parameters)
 *          n_iter                  the iterations this call may run.  The loop condition of :182 joins its two limits with OR, so a call that
 *                                  does not return a refined model runs max(nIterations, mRansacMaxIts - mnIterations) iterations
 *          draws[n_iter][4]        draws[k][i] = what RandomInt(0, n - 1 - i) returned for draw i of iteration k (:193); the swap-with-back
 *                                  bookkeeping of vAvailableIndices (:188-201) is done by the device.  The minimal set is ASD_PNP_MIN_SET = 4,
 *                                  the only value the reference passes (Tracking.cc:1141)
 *  in/out  best_inliers            mnBestInliers (:212-215)
 *  out     best_updated            1 when an iteration of this call took over the best model (:212); only then are written
 *          best_Tcw[16]            mBestTcw (:217-223), row major
 *          best_mask[n]            mvbBestInliers (:214), by correspondence
 *          found                   1 when iterate() returns the refined model (:226-236)
 *          iterations_done         k + 1 when iteration k returns, n_iter otherwise: what the caller adds to mnIterations; 4 x that many
 *                                  draws were consumed
 *          n_inliers               mnRefinedInliers (:228), 0 unless found
 *          Tcw[16]                 mRefinedTcw (:294-300), written only when found
 *          inliers[n]              mvbRefinedInliers (:229-234, by correspondence: the caller maps through mvKeyPointIndices), all 0 unless found
 * A problem with n < min_inliers runs nothing (:173-177): found = 0, iterations_done = 0 and nothing else of it is written.
 * The rule over the iterations is a literal sequential run of :182-257: an iteration with mnInliersi >= min_inliers (:209) that beats
 * best_inliers (:212, strict) becomes the best model and Refine (:260-305) runs on its inlier set; Refine is a function of mvbBestInliers
 * alone, so the calls the reference repeats on an unchanged set (:226 for an iteration that passes :209 without beating the best) are known to
 * fail and are not run; a Refine with more than min_inliers inliers (:292, strict) ends the call.  What :241-255 does afterwards (bNoMore,
 * returning mBestTcw) is the caller's (asd::PnPsolver, host/asd_adapters.hpp).  So is one case the rule above leaves out: a best model that
 * comes in with best_inliers is taken to be one whose Refine failed, which holds unless the caller iterates a solver again AFTER it returned
 * its refined model; the reference then returns the same refined model at the next iteration that passes :209 without beating the best one,
 * and asd::PnPsolver::End restores that from the iteration counts (asd_debug_pnp_ransac).
 * The model (compute_pose, :477-525) is EPnP in f64 from the f32 inputs widened: control points by PCA (:375-409), barycentric coordinates
 * (:411-434), M^T M (:436-451, :492), its four smallest eigenvectors, L_6x10 / rho (:760-810), the three approximations (:667-758) each followed
 * by five Gauss-Newton steps (:840-950), R and t by Procrustes (:569-627) with the reference's sign rule (:636-649, the first correspondence
 * only) and determinant fix (:618-622, row 2 of R), the candidate of least reprojection error with strict < from candidate 1 (:518-520).
 * Where the reference calls OpenCV's legacy C API the library states its own rules; they are the formula, not OpenCV's bits:
 *  - cvSVD of the symmetric matrices (:400, :493) is a cyclic Jacobi eigen-decomposition; the eigenvalues are ordered and the vectors are
 *    orthonormal to rounding.  With four correspondences M^T M has a four-dimensional null space and EPnP's result depends on the basis the
 *    solver returns for it: the pose of a minimal set is not a function of the input alone, in the reference as here.
 *  - cvInvert(CV_SVD) (:421) and cvSolve(CV_SVD) (:681, :712, :746) are the pseudo-inverse and the minimum-norm least-squares solution by a
 *    one-sided Jacobi SVD; singular values at or below 2 * DBL_EPSILON * (sum of the singular values) count as zero.
 *  - cvSVD of ABt (:608): the same SVD; the left vector of a zero singular value is the cross product of the other two left vectors.
 *  - qr_solve on a zero column (:887-891) returns without writing X in the reference, and gauss_newton then adds an indeterminate x
 *    (uninitialised on the first pass): the one place the reference's behaviour is undefined.  The library's rule is x = 0 for that step.
 * CheckInliers (:308-339) is the reference's mixed arithmetic without fusing: Xc, Yc = the f64 expression over the f64 pose and the f32 point
 * rounded to f32, invZc = 1 / (f64 sum) rounded to f32, ue = uc + fu * Xc * invZc in f64, distX = P2D.x - ue rounded to f32, error2 in f32,
 * compared < with max_err.  A non-finite pose or projection is never an inlier.  best_Tcw / Tcw are the f64 R, t rounded to f32 once, last row
 * 0 0 0 1.
 * Limits (ASD_ERR_CAPACITY beyond them): ASD_PNP_RANSAC_MAX_N correspondences per problem, ASD_PNP_RANSAC_MAX_PROBLEMS problems per call,
 * ASD_PNP_RANSAC_MAX_HYPOTHESES iterations per call summed over its problems.  ASD_ERR_INVALID: a draw outside [0, n - 1 - i], n < 4 in a
 * problem that has iterations to run, a null array, negative n / n_iter; asd_last_error names the problem.  Two kernel launches and one
 * synchronisation per call, no atomics, reductions of one fixed shape: a call is one bit pattern.  Legal wherever asd_sim3_ransac is. */
#define ASD_PNP_MIN_SET 4
#define ASD_PNP_RANSAC_MAX_N 8192
#define ASD_PNP_RANSAC_MAX_PROBLEMS 64
#define ASD_PNP_RANSAC_MAX_HYPOTHESES 4096
typedef struct asd_pnp_ransac_problem {
  int32_t n;
  const float* P3Dw;
  const float* P2D;
  const float* max_err;
  float K[4];
  int32_t min_inliers;
  int32_t n_iter;
  const int32_t* draws;
  int32_t best_inliers;
  int32_t best_updated;
  float best_Tcw[16];
  uint8_t* best_mask;
  int32_t found, iterations_done, n_inliers;
  float Tcw[16];
  uint8_t* inliers;
} asd_pnp_ransac_problem;
int asd_pnp_ransac(asd_ctx* ctx, int32_t n_problems, asd_pnp_ransac_problem* problems);
/* PnPsolver::SetRansacParameters (:121-152) in the reference's types: int nMinInliers = N * (float)epsilon, raised to min_inliers and to
 * min_set (:134-139) -> *min_inliers_out; epsilon = max(epsilon, (float)nMinInliers / N) as a float (:141-142); 1 iteration when
 * nMinInliers == N, else ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in double (:147-150); *max_its_out = max(1, min(.,
 * max_iterations)) (:152).  A value that does not fit an int converts as x86-64 does, to INT_MIN (as asd_sim3_ransac_max_iterations).
 * Host only, no context. */
int asd_pnp_ransac_parameters(int32_t n, double probability, int32_t min_inliers, int32_t max_iterations, int32_t min_set, float epsilon,
                              int32_t* min_inliers_out, int32_t* max_its_out);
/* Test aid: one compute_pose of the context's last asd_pnp_ransac.  which >= 0: iteration `which`; which = -1 - r: the r-th Refine the walk
 * ran (r < n_refines).  idx = the four sampled correspondences (:188-201; -1 for a Refine), hypothesis = the iteration (for a Refine: the one
 * whose inlier set it refined), count = mnInliersi of the CheckInliers behind it, n_refines = how many Refines the problem's walk ran, then in
 * f64: R (row major), t, the control points cws (:375-409), the four basis vectors v (ut rows 11, 10, 9, 8 of :493) with their eigenvalues
 * (ascending), rep_errors of candidates 1-3 (:508-516), the chosen N (:518-520) and its betas after gauss_newton.  Copied back with the
 * block the call reads anyway.  ASD_ERR_INVALID for a (problem, which) the last call did not run. */
typedef struct asd_pnp_ransac_debug {
  int32_t idx[4];
  int32_t count, n_refines, N, hypothesis;
  double R[9], t[3], cws[12], v[48], eig[4], rep_errors[3], betas[4];
} asd_pnp_ransac_debug;
int32_t asd_debug_pnp_ransac(const asd_ctx* ctx, int32_t problem, int32_t which, asd_pnp_ransac_debug* out);
/* Initializer (src/vslam/src/Initializer.cc): Initializer::Initialize (:43-120) for a batch of frame pairs -- the step of
 * Tracking::MonocularInitialization (Tracking.cc:385-438, Initializer(frame, 1.0, 200)) between SearchForInitialization (asd_match_init) and
 * the first map.  GlobalBundleAdjustemnt(20) on the two-keyframe map, which the reference runs next, is asd_bundle_adjustment.  One problem
 * = one Initialize call:
 *  in      n1, keys1[n1][2]        mvKeys1 = the reference frame's mvKeysUn pt (:37), f32
 *          n2, keys2[n2][2]        mvKeys2 = the current frame's mvKeysUn pt (:49), f32
 *          matches12[n1]           vMatches12: the keypoint of frame 2 matched to keypoint i of frame 1, -1 for none.  mvMatches12 (:55-64) is
 *                                  built by the library in index order
 *          K[4]                    fx fy cx cy of mK (:35)
 *          sigma                   mSigma (:39); mSigma2 = sigma * sigma in f32 (:40)
 *          n_iter                  mMaxIterations (:41)
 *          draws[n_iter][8]        draws[k][j] = what RandomInt(0, N - 1 - j) returned for draw j of iteration k (:93); the swap-with-back
 *                                  bookkeeping of vAvailableIndices (:88-100) is done by the device
 *          min_parallax,           what Initialize passes to ReconstructH / ReconstructF: 1 and 50 in the reference (:115-117)
 *          min_triangulated
 *  out     n_matches               N = mvMatches12.size() (:66)
 *          SH, SF                  the scores FindHomography / FindFundamental leave (:164-169, :215-220)
 *          model                   0 = ReconstructH was called, 1 = ReconstructF (:113-116): RH = SH / (SH + SF) in f32, compared as a double
 *                                  with 0.40; a NaN (SH = SF = 0) goes to F, as in the reference
 *          ok                      what Initialize returns
 *          R21[9], t21[3]          row major, f32; written only when ok
 *          P3D[n1][3],             vP3D / vbTriangulated, indexed by the keypoint of frame 1 (CheckRT :850-851, :931-935): zero / 0 for a
 *          triangulated[n1]        keypoint whose match is not one of the winning hypothesis' good points; written only when ok
 *          H21[9], F21[9]          the best models of :166 and :217, f32; each is written only when an iteration of its model scored above 0
 *          inliers_H[n_matches],   vbMatchesInliers of :167 and :218, by match (the k-th match is the k-th keypoint of frame 1 that has one);
 *          inliers_F[n_matches]    always written, all 0 for a model no iteration of which scored above 0
 * When ok == 0 nothing is written to R21, t21, P3D and triangulated (the reference leaves vP3D / vbTriangulated alone and R21 / t21 empty).
 * A problem in which no iteration of the chosen model scores above 0 makes the reference read an empty H21 / F21; the library's rule is
 * ok = 0.
 *
 * Arithmetic.  Every cv::Mat the reference stores as CV_32F is f32 here.  Where it leaves the evaluation to OpenCV the library states its
 * own rules; they are the formula, not OpenCV's bits:
 *  - a matrix product is evaluated in f64 on the widened elements, the terms of an element added in index order, and rounded to f32 once
 *    when stored; a chain runs left to right as written (T2inv * Hn * T1 is two products and two roundings).  A scalar in front of a chain
 *    (s * U * Rp * Vt, :638) scales the first matrix first (one rounding); R * p3dC1 + t (:903) and K * [R | t] (:866) are one sum per element
 *    with the addend last; -R.t() * t (:868) is the negated product.  t / cv::norm(t) (:648, :957) divides each element by the f64 norm.
 *  - inv() (:133, :160, :595) is the adjugate over the determinant in f64, rounded once; a zero determinant gives the zero matrix, as
 *    cv::invert leaves it.  determinant and norm are f64 on the widened elements; dot and norm return double to the expression around them.
 *  - scalar float expressions (:604-627, :662-665, all of CheckHomography, CheckFundamental, CheckRT and Normalize) are the reference's
 *    C++ literally, un-fused, with the types C++ gives them: th = (float)5.991, invSigmaSquare = (float)(1.0 / (double)(sigma * sigma)),
 *    1.0 / x divides in double and rounds once, comparisons with 0.99998 / 1.0000001 / 0.40 / 0.7 / 0.75 / 0.9 are made in double, sqrt of a
 *    float is the f32 square root.  The score is the sequential f32 sum over the matches in order, test 1 before test 2 of each match.
 *  - the null vector of A (ComputeH21 :229-264, 16 x 9; ComputeF21 :279-303, 8 x 9; every entry the f32 product the reference forms) is the
 *    right singular vector of the smallest singular value by a one-sided Jacobi in f64 on the widened entries, of unit norm to rounding, then
 *    rounded to f32.  For F, A has 8 rows and that singular value is zero.  The SIGN is the library's choice -- the component of largest
 *    magnitude (the first of equal ones) is positive: H21i, H12i and F21i change sign with it, and so does the order of the motion hypotheses;
 *    the scores, the masks and the outcome of ReconstructF do not (CheckHomography and CheckFundamental are homogeneous of degree 0 in the
 *    model, E21's singular vectors are defined up to sign either way).
 *  - the 3 x 3 SVDs (Fpre :305, E21 :954, A = invK * H21 * K :599): the same Jacobi in f64 on the widened elements; V is the product of the
 *    rotations applied to the identity, u_j = (A v_j) / w_j, and the sign of each pair is set so that the component of v_j of largest magnitude
 *    (the first of equal ones) is positive; a u_j whose w_j is at or below 2 * DBL_EPSILON * (w_0 + w_1
 *    + w_2) is the cross product of the other two; the triplets are ordered by descending w (the first of equal ones first); U, w and Vt are
 *    then rounded to f32.  ReconstructH's eight hypotheses are ordered by the signs of U and V (:621-628 pair x1, x3 with fixed signs), so
 *    their ORDER, and with it which of two hypotheses tied for best is kept (:717, strict), depends on this convention.
 *  - Triangulate (:774-787) is asd_svd4_null's computation (OpenCV 3.2.0's JacobiSVDImpl_ on the 4 x 4 f32 matrix, rows formed as
 *    x * P.row(2) - P.row(0) by asd_triangulate_pairs' rule) and x3D = vt.row(3)[0..2] * (float)(1.0 / vt.row(3)[3]) + 0.0f.
 *  - parallax (:940-943): vCosParallax[min(50, size - 1)] of the sorted list is selected by rank (-0 and +0 rank as equal; a NaN cosine,
 *    for which the reference's sort is undefined, orders after every number); parallax = (float)(acos((double)cos) * 180 / CV_PI).
 * Limits (ASD_ERR_CAPACITY beyond them): ASD_INIT_MAX_KEYS keypoints per frame, ASD_INIT_MAX_ITERATIONS iterations per problem,
 * ASD_INIT_MAX_PROBLEMS problems per call.  ASD_ERR_INVALID: N < 8 (the reference's sampling is undefined; Tracking.cc:428 never goes below
 * 100), a draw outside [0, N - 1 - j], a match index outside [-1, n2), a null array, negative n1 / n2, n_iter < 1; asd_last_error names the
 * problem.  Two kernel launches (k_init_hyp: one workgroup per problem, iteration and model; k_init_reconstruct: one per problem) and one
 * synchronisation per call, no atomics, every reduction of one fixed shape: a call is one bit pattern.  Timer: "initializer".  Legal wherever
 * asd_pnp_ransac is. */
#define ASD_INIT_MAX_KEYS 8192
#define ASD_INIT_MAX_ITERATIONS 1024
#define ASD_INIT_MAX_PROBLEMS 8
typedef struct asd_initializer_problem {
  int32_t n1;
  const float* keys1;
  int32_t n2;
  const float* keys2;
  const int32_t* matches12;
  float K[4];
  float sigma;
  int32_t n_iter;
  const int32_t* draws;
  float min_parallax;
  int32_t min_triangulated;
  int32_t n_matches;
  float SH, SF;
  int32_t model, ok;
  float R21[9], t21[3];
  float* P3D;
  uint8_t* triangulated;
  float H21[9], F21[9];
  uint8_t* inliers_H;
  uint8_t* inliers_F;
} asd_initializer_problem;
int asd_initialize(asd_ctx* ctx, int32_t n_problems, asd_initializer_problem* problems);
/* Initializer::Normalize (:791-837) in the reference's f32 order: the means and the mean absolute deviations are sequential f32 sums over
 * ALL n keys (the frame's, not only the matched ones), sX = (float)(1.0 / meanDevX); pts_out[n][2] = vNormalizedPoints, T_out[9] = T row
 * major.  asd_initialize normalises with this function on the host, in front of its upload.  n == 0 gives the reference's 0 / 0.  Host only,
 * no context. */
int asd_initializer_normalize(int32_t n, const float* keys, float* pts_out, float* T_out);
/* Test aid: the context's last asd_initialize.
 *  which = 2 k + m, 0 <= k < n_iter, m = 0 (H) / 1 (F): iteration k of that model.  idx = the eight sampled matches (:88-100), nullv = the
 *    unit null vector in f64, for F also U, w, Vt of the rank-2 step (:305) in f64 (w descending, before the rounding to f32), M1 = H21i or F21i,
 *    M2 = H12i (H only), score, and mask (when not NULL: [n_matches] bytes) = vbCurrentInliers.
 *  which = -1: the reconstruction.  U, w, Vt = the 3 x 3 decomposition (:599 or :954) in f64; best_H / best_F = the iterations the walks kept
 *    (-1: none scored above 0); n_inliers = N of :485-488 / :586-589; n_hyp = 8 / 4 motion hypotheses, or 0 where none was checked (:607-611,
 *    or no model); R, t, n_good, parallax and cos_sel (the selected cosine, NaN when n_good = 0) of each; winner = the hypothesis returned or
 *    -1; second_good (H path).
 *  which = -2 - h: the same, and points (when not NULL: [n_matches][3] f32) = hypothesis h's triangulated points by match, NaN where the
 *    point was never triangulated (the match is not in the inlier set), flags (when not NULL: [n_matches] bytes): bit 0 = counted in nGood
 *    (:930-932), bit 1 = vbGood (:934-935).
 * ASD_ERR_INVALID for a (problem, which) the last call did not run. */
typedef struct asd_initializer_debug {
  int32_t idx[8];
  double nullv[9], U[9], w[3], Vt[9];
  float M1[9], M2[9], score;
  int32_t best_H, best_F, n_inliers, n_hyp, winner, second_good;
  float R[8][9], t[8][3], parallax[8], cos_sel[8];
  int32_t n_good[8];
  uint8_t* mask;
  float* points;
  uint8_t* flags;
} asd_initializer_debug;
int32_t asd_debug_initialize(const asd_ctx* ctx, int32_t problem, int32_t which, asd_initializer_debug* out);
/* ---- keyframe database and BoW score ------------------------------------------------------
 * TemplatedVocabulary::score (TemplatedVocabulary.h:1264-1269) -> L1Scoring / L2Scoring / DotProductScoring::score
 * (src/dbow2/DBoW2/ScoringObject.cpp:23-68, :73-120, :271-311) of two BowVectors given as (word id strictly ascending, value).  Host
 * only: no context, no device (like asd_undistort_map).  scoring = asd_voc_load's enum: 0 L1, 1 L2, 5 DOT_PRODUCT; 2 CHI_SQUARE, 3 KL
 * and 4 BHATTACHARYYA are not offered (ASD_ERR_INVALID; asd_last_error(NULL) says so) -- KL needs log(), which the device cannot
 * match bit for bit.  v1 = (id1, val1) is score()'s first argument.  The sum is the reference's chain: f64, one term per common word in
 * ascending word order, no FMA; two L1 vectors without a common word score -0.0 (-score / 2.0).  Ids that are not strictly ascending:
 * ASD_ERR_INVALID. */
int asd_bow_score(int32_t scoring, int32_t n1, const int32_t* id1, const double* val1, int32_t n2, const int32_t* id2,
                  const double* val2, double* score);

/* KeyFrameDatabase (src/vslam/src/KeyFrameDatabase.cc), one per context: the keyframes' BowVectors live in HBM and every query is one
 * brute-force scoring pass over them (kfdb.hip).  All calls run on the context's stream with buffers of their own: they are legal
 * while submissions of asd_extract_submit are outstanding and while an asd_track_* call is armed; they add no stream.
 *
 * asd_kfdb_clear   the constructor / clear() (:34-38, :72-76): empties the database and sets the scoring every later call uses
 *                  (0 | 1 | 5; -1 = the loaded vocabulary's, ASD_ERR_INVALID when none is loaded).  A context starts with an empty L1 database.
 * asd_kfdb_add     add() (:41-47).  kf = the caller's keyframe id (mnId, any int32 >= 0); global_map = KeyFrame::GetGlobalMapFlag().
 *                  An id already present is ASD_ERR_INVALID (the reference would list the keyframe twice; that is not reproduced).
 *                  An empty BowVector is a legal entry that no query ever finds.
 * asd_kfdb_erase   erase() (:49-70).  An unknown id is ASD_OK (the reference's loop finds nothing).  It invalidates the state a
 *                  query left for asd_kfdb_select.
 * asd_kfdb_score   mpVoc->score(query, entry) as f64 for the n named entries: the body of DetectLoop's minScore loop
 *                  (LoopClosing.cc:154-168; the caller casts to float and takes the minimum).  An unknown id is ASD_ERR_INVALID.
 *                  Changes no per-entry state.
 *
 * Per-entry state, kept between queries like the reference's KeyFrame fields: mnLoopQuery / mnLoopWords / mLoopScore,
 * mnRelocQuery / mnRelocWords / mRelocScore, the global-map flag and an add sequence number.  Two deliberate differences:
 * every query stamps with a fresh number, so the coincidences of the reference's initial values mnLoopQuery(0) / mnRelocQuery(-1) with
 * a keyframe of id 0 / a frame of id -1 are not reproduced; and mLoopScore / mRelocScore, which the reference never initialises
 * (KeyFrame.cc:150, :181), start at 0.0f. */
int asd_kfdb_clear(asd_ctx* ctx, int32_t scoring);
int asd_kfdb_add(asd_ctx* ctx, int32_t kf, int32_t n_words, const int32_t* bow_id, const double* bow_val, int32_t global_map);
int asd_kfdb_erase(asd_ctx* ctx, int32_t kf);
int asd_kfdb_score(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t n, const int32_t* kfs, double* score);
/* KeyFrameDatabase::DetectLoopCandidates (:80-204) and ::DetectRelocalizationCandidates (:206-322), each in two calls, because
 * GetBestCovisibilityKeyFrames(10) is pointer-graph state of the caller and which keyframes need it is known only after scoring.
 *
 * asd_kfdb_query_loop   :85-149.  connected = pKF->GetConnectedKeyFrames() as ids (ids not in the database are ignored): they never
 *   enter lKFsSharingWords.  minCommonWords = (int)(maxCommonWords * 0.6f) (this fork; upstream 0.8f), gate mnLoopWords > minCommonWords;
 *   mLoopScore is stored for every keyframe that passes the gate, in front of the si >= min_score and only_global_map tests (:142-147).
 *   Output: lScoreAndMatch as (scored_kf, scored_score = float si) in the reference's list order, *n_scored entries.
 * asd_kfdb_query_reloc  :208-266.  only_global_map is applied in front of the list (:229): a keyframe that is not global-map is
 *   stamped and has its words counted but is never scored.  minCommonWords = (int)(max * 0.8f).
 * asd_kfdb_select       the covisibility accumulation and the retain filter (:153-203 for mode 0, :271-321 for mode 1) over the state
 *   the last query of that mode left.  neigh[n_scored][10] = GetBestCovisibilityKeyFrames(10) of scored_kf[i] as ids, -1 padded; ids
 *   that are not in the database are legal (keyframes whose query stamp does not match).  Loop: a neighbour counts when this query
 *   stamped it and its words are > minCommonWords (:167), bestAccScore starts at min_score, retain is > 0.55f * bestAccScore (this fork;
 *   upstream 0.75f).  Reloc: only the stamp is checked (:286), so a neighbour that shares a word but was not scored by this query
 *   contributes the score an earlier reloc query left on it (0.0f when there was none); bestAccScore starts at 0, retain is
 *   > 0.75f * bestAccScore.  All in f32.  Output: vpLoopCandidates / vpRelocCandidates as ids in the reference's order (duplicates
 *   dropped, first occurrence kept).  n_scored == 0 gives *n_cand = 0; an n_scored that is not the last query's (or an
 *   asd_kfdb_erase since that query) is ASD_ERR_INVALID.
 * ASD_ERR_CAPACITY when `capacity` is too small (*n_scored / *n_cand then hold the count needed; a query may simply be repeated) and
 * for a query of more than 13653 words (the query vector is staged in LDS). */
int asd_kfdb_query_loop(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t n_connected,
                        const int32_t* connected, float min_score, int32_t only_global_map, int32_t capacity, int32_t* scored_kf,
                        float* scored_score, int32_t* n_scored);
int asd_kfdb_query_reloc(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t only_global_map,
                         int32_t capacity, int32_t* scored_kf, float* scored_score, int32_t* n_scored);
int asd_kfdb_select(asd_ctx* ctx, int32_t mode, int32_t n_scored, const int32_t* neigh, int32_t capacity, int32_t* cand,
                    int32_t* n_cand);
/* Test aids.  asd_debug_kfdb: out = {live entries, live words, entry capacity, word capacity, number of arena growths}.
 * asd_debug_kfdb_entry: out = {stamped by the last loop query, loop words, stamped by the last reloc query, reloc words},
 * score = {loop score, reloc score}; ASD_ERR_INVALID for an id that is not in the database. */
int32_t asd_debug_kfdb(asd_ctx* ctx, int64_t out[5]);
int32_t asd_debug_kfdb_entry(asd_ctx* ctx, int32_t kf, int32_t out[4], float score[2]);
/* ---- observation table and the local map ---------------------------------------------------
 * The third resident table, one per context (localmap.hip), beside the descriptor / attribute banks and the keyframe database: which
 * keyframe observes which map point.  It is keyframe-major: every live keyframe (kf = the caller's mnId, any int32 >= 0) has a row of n
 * int32 entries, entry idx = the bank row of the map point the keyframe observes at keypoint idx, or -1 -- KeyFrame::mvpMapPoints in the
 * row numbering of asd_bank_put* / asd_mpbank_put.
 * PRECONDITION, not checked: the table mirrors MapPoint::mObservations -- entry (kf, idx) = r exactly when point r has the observation
 * kf -> idx, so a point occurs at most once in a keyframe's row.  EVERY TABLE ENTRY COUNTS: a row that names a point twice gives that
 * keyframe two votes per keypoint of the frame that holds the point.
 *
 * asd_map_put        create or replace a keyframe's row (KeyFrame construction; n <= 65536).  Links and bad flag of a replaced row stay.
 * asd_map_set        change single entries: KeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch, i.e. the keyframe side of
 *                    MapPoint::AddObservation / EraseObservation / Replace (KeyFrame.cc:436-459, MapPoint.cc:110-142, :206-244).  Applied
 *                    in the order given.  An unknown keyframe or an idx outside its row is ASD_ERR_INVALID.
 * asd_map_erase      the keyframe leaves the table with its links and flag (KeyFrame::SetBadFlag's erase, KeyFrame.cc:723-815).  An
 *                    unknown id is ASD_OK.
 * asd_map_clear      empties the table and frees its storage.
 * asd_map_kf_links   cov[n_cov <= 10] = GetBestCovisibilityKeyFrames(10) as ids in its order, children = GetChilds() as ids strictly
 *                    ascending, parent = GetParent()'s id or -1.  The ids may name keyframes that are not, or no longer, in the table:
 *                    such a keyframe contributes no points and counts as not bad, exactly as a keyframe would that the host still holds
 *                    a pointer to.  kf itself must be in the table (ASD_ERR_INVALID).
 * asd_map_kf_bad     KeyFrame::isBad() of a keyframe in the table (ASD_ERR_INVALID for an unknown id).
 * asd_map_point_bad  MapPoint::isBad() for n bank rows, one byte per row; rows never named are not bad.
 *
 * Storage starts small and grows; at least 16384 live keyframes (the limit is 262144) of up to 65536 entries and bank rows below 2^28 are
 * taken, ASD_ERR_CAPACITY with a message beyond.  All work runs on the context's stream and every call returns with its own work drained.
 * The calls are legal while submissions of asd_extract_submit are outstanding.  While an asd_track_* call armed with asd_track_async is
 * unfinished EVERY call of this section returns ASD_ERR_INVALID: asd_track_local_points_map reads the search list and the banks on that
 * stream, and no ordering between a table change and the stage in flight is promised -- asd_track_finish first. */
int asd_map_put(asd_ctx* ctx, int32_t kf, int32_t n, const int32_t* rows);
int asd_map_set(asd_ctx* ctx, int32_t kf, int32_t count, const int32_t* idx, const int32_t* rows);
int asd_map_erase(asd_ctx* ctx, int32_t kf);
int asd_map_clear(asd_ctx* ctx);
int asd_map_kf_links(asd_ctx* ctx, int32_t kf, int32_t n_cov, const int32_t* cov, int32_t n_children, const int32_t* children,
                     int32_t parent);
int asd_map_kf_bad(asd_ctx* ctx, int32_t kf, int32_t flag);
int asd_map_point_bad(asd_ctx* ctx, int32_t n, const int32_t* rows, int32_t flag);

/* Tracking::UpdateLocalMap (Tracking.cc:871-879 = UpdateLocalKeyFrames :907-1015 + UpdateLocalPoints :881-905) and the skip loop of
 * SearchLocalPoints (:827-841) as one call over the table.  The reference is restated literally with ONE rule where it iterates in
 * pointer order: every walk over a std::map<KeyFrame*, ...> or std::set<KeyFrame*> (keyframeCounter, GetChilds()) is in ASCENDING
 * KEYFRAME ID (the quadtree's pointer-order tie is documented the same way).
 *   in   cur_rows[n_cur]   mCurrentFrame.mvpMapPoints as bank rows after the motion-model stage's outlier drop, -1 = none
 *        seen_rows[n_seen] further rows that carry mnLastFrameSeen == this frame: the dropped outliers' points (:705-707)
 *        prev_kfs[n_prev]  the caller's current mvpLocalKeyFrames, used only when nobody votes
 *        max_kfs           80 (:961); at most 1000
 *   out  local_kfs / n_local_kfs  mvpLocalKeyFrames;  ref_kf  pKFmax, or -1 when nobody voted (mpReferenceKF then stays, :1010-1014)
 *        local_rows / n_local     mvpLocalMapPoints, in order
 *        search_rows / n_search   the sub-list SearchLocalPoints does not skip, in order
 * Votes (:910-927): every keypoint of the frame whose point is not bad gives one vote to every keyframe that observes the point -- per
 * keypoint, a point the frame holds twice votes twice; bad points do not vote (the caller nulls them itself).  List (:939-954): the voted
 * keyframes in ascending id, bad ones skipped; pKFmax = the first with a strictly larger count (the lowest id among the maxima, never a bad
 * keyframe).  Expansion (:958-1008): over the voted keyframes only (the end iterator is taken before anything is appended), stopped when the
 * list holds more than max_kfs entries at the top of an iteration; per keyframe the first not-bad, not-yet-included covisible, then the
 * first such child, then the parent (no bad test, :997-1006) if not yet included -- and adding a parent ENDS the expansion (the break at
 * :1004 leaves the outer loop).  Nobody voted (:929-930): the list is prev_kfs unchanged.  Points (:885-903): the local keyframes in list
 * order, their entries in ascending keypoint index, a point taken at its first occurrence unless it is bad; a bad keyframe in prev_kfs still
 * contributes.  Search list: local_rows without the rows named in cur_rows (>= 0) or seen_rows, order kept.
 * Capacities are the caller's.  When one is too small the call returns ASD_ERR_CAPACITY with ALL counts set to what is needed, and may
 * simply be repeated.  Both lists also stay on the device for asd_track_local_points_map (after ASD_OK only).  Results are identical from
 * run to run.  ASD_ERR_CAPACITY also when the local keyframes' rows together exceed 2^31 - 2^24 entries. */
typedef struct asd_local_map_args {
  int32_t n_cur;  const int32_t* cur_rows;
  int32_t n_seen; const int32_t* seen_rows;
  int32_t n_prev; const int32_t* prev_kfs;
  int32_t max_kfs;
  int32_t kf_capacity;     int32_t* local_kfs;   int32_t n_local_kfs; int32_t ref_kf;
  int32_t row_capacity;    int32_t* local_rows;  int32_t n_local;
  int32_t search_capacity; int32_t* search_rows; int32_t n_search;
} asd_local_map_args;
int asd_update_local_map(asd_ctx* ctx, asd_local_map_args* args);

/* asd_track_local_points_rows over the search_rows that the last asd_update_local_map of this context left on the device: TrackLocalMap's
 * body (Tracking.cc:725-736) without a row upload.  Same stage, same results bit for bit as the _rows call given the returned list;
 * match_cur[j] indexes search_rows.  ASD_ERR_INVALID when there is no such list, when any asd_map_* call has changed the table since, or
 * when n_search == 0; asd_track_local_points_rows' own ASD_ERR_CAPACITY beyond the device replay.  Honours asd_track_async / _finish. */
int asd_track_local_points_map(asd_ctx* ctx, int32_t slot_cur, const float* Tcw, const float* K, float viewing_cos_limit,
                               const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive,
                               double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers);

/* KFcounter of KeyFrame::UpdateConnections (KeyFrame.cc:541-573) for a keyframe in the table: for every OTHER keyframe the number of the
 * keyframe's not-bad points that it observes too (the vote pass of asd_update_local_map with the keyframe's own row as the frame).  The
 * keyframe itself is excluded (:561), bad keyframes are not (as in the reference).  Keyframes with a count > 0 come back in ascending id;
 * ASD_ERR_CAPACITY with *n = the count needed when `capacity` is too small. */
int asd_map_shared_counts(asd_ctx* ctx, int32_t kf, int32_t capacity, int32_t* kfs, int32_t* counts, int32_t* n);

/* ---- LocalMapping::KeyFrameCulling and MapPoint::Observations() over the table ----
 * asd_map_put_octaves sets mvKeysUn[idx].octave for every keypoint of a keyframe that is in the table: n must equal the row's length and
 * every value must be < ASD_MAX_LEVELS, anything else is ASD_ERR_INVALID.  The octaves are the keypoints', not the point list's: they
 * follow the row through growth and compaction, an asd_map_put that replaces the row with the same n keeps them, one with another n drops
 * them, asd_map_erase and asd_map_clear drop them, asd_map_set does not touch them.  Setting them does not invalidate the search list of
 * asd_track_local_points_map. */
int asd_map_put_octaves(asd_ctx* ctx, int32_t kf, int32_t n, const uint8_t* octave);

/* LocalMapping::KeyFrameCulling (LocalMapping.cc:739-809), the monocular path, stated literally -- including what pKF->SetBadFlag() inside
 * the loop does to the observations the NEXT candidates are judged by (KeyFrame.cc:739-741 -> MapPoint::EraseObservation, MapPoint.cc:
 * 119-142 -> MapPoint::SetBadFlag, :180-197).  Per candidate, in list order:
 *   skipped (decision 3, counts 0) when bit0 of its flag is set or its id is 0 (:751-754);
 *   for every entry idx whose point r is >= 0 and not bad: nMPs++; if Observations(r) > 3 and at least 3 OTHER keyframes observe r at an
 *   octave <= octave(kf, idx) + 1: nRedundantObservations++.  Observations(r) = the number of table entries that name r;
 *   culled when nRedundantObservations > 0.9 nMPs (decided as 10 nR > 9 nM, the same for every row the table takes; nMPs == 0 never culls);
 *   a culled candidate with bit1 (mbNotErase) gets decision 2 and changes nothing (KeyFrame.cc:729-733);
 *   otherwise (decision 1) its observations leave the counts before the next candidate is examined, in ascending keypoint index; a point
 *   whose count thereby reaches <= 2 becomes bad at that moment, is appended to bad_rows, loses all its observations and counts in no later
 *   candidate's nMPs.  (A point that is flagged bad and still has entries -- a state the reference does not have -- counts nowhere, is not
 *   reported again, and keeps its entries in other rows.)
 * apply = 1 leaves the table as these calls would: for every decision-1 keyframe asd_map_kf_bad(kf, 1) and every entry of its row -1; for
 * every row of bad_rows asd_map_point_bad(row, 1) and its remaining entries in all other rows -1.  The keyframe keeps its slot, links and
 * octaves (asd_map_erase stays the caller's step).  When that changed anything the search list of asd_track_local_points_map is invalid.
 * apply = 0 changes nothing.
 * ASD_ERR_INVALID: a candidate that is not in the table or occurs twice; any live keyframe without octaves (asd_last_error names one).
 * ASD_ERR_CAPACITY: more than 4096 candidates; candidates' rows of more than 2^26 entries together; bad_capacity too small -- n_bad then
 * holds the count needed, the table is untouched whatever apply says, and the call may be repeated.  Results are identical from run to run. */
typedef struct asd_kf_culling_args {
  int32_t n_cand; const int32_t* cand;      /* GetVectorCovisibleKeyFrames() as ids, in its order                    */
  const uint8_t* cand_flags;                /* per candidate: bit0 = GetGlobalMapFlag() (:751), bit1 = mbNotErase    */
  int32_t apply;                            /* 0: decisions only, the table is left as it was                        */
  uint8_t* decision;                        /* [n_cand] 0 kept, 1 SetBadFlag took effect, 2 mbToBeErased only, 3 skipped (:751-754) */
  int32_t* n_mps; int32_t* n_redundant;     /* [n_cand] nMPs, nRedundantObservations as the reference had them at the test (0 when skipped) */
  int32_t bad_capacity; int32_t* bad_rows; int32_t n_bad;  /* points that EraseObservation turned bad, in the order it happened */
} asd_kf_culling_args;
int asd_keyframe_culling(asd_ctx* ctx, asd_kf_culling_args* args);

/* MapPoint::Observations() (nObs, MapPoint.cc:110-117) for n bank rows: counts[i] = the number of table entries that name rows[i].  The
 * bad byte is not consulted; a row never named gives 0.  Changes neither the table nor the search list. */
int asd_map_observations(asd_ctx* ctx, int32_t n, const int32_t* rows, int32_t* counts);

/* ---- MapPoint::UpdateNormalAndDepth over the tables ----
 * asd_map_kf_centers sets KeyFrame::GetCameraCenter() (Ow, f32, as KeyFrame::SetPose leaves it, KeyFrame.cc:221-235) for n keyframes
 * that are in the table.  The library does not recompute it from Tcw.  An unknown keyframe is ASD_ERR_INVALID and nothing is written; a
 * keyframe named twice takes the last value.  The centre belongs to the keyframe's slot: it follows table growth, an asd_map_put that
 * replaces the row keeps it (whatever n), asd_map_erase and asd_map_clear drop it.  Setting centres does not invalidate the search list of
 * asd_track_local_points_map. */
int asd_map_kf_centers(asd_ctx* ctx, int32_t n, const int32_t* kfs, const float* Ow /*[n][3]*/);

/* MapPoint::UpdateNormalAndDepth (MapPoint.cc:361-407) for n points at once, over the observation table, the centres above, the octaves of
 * asd_map_put_octaves and the attribute bank, whose rows it rewrites in place -- the caller uploads no normals and no ranges.
 * Xw non-NULL is the write-back form, MapPoint::SetWorldPos directly in front of the update (Optimizer.cc:728-731, :225-227, :995-998,
 * LoopClosing.cc:518-520): Xw[i] becomes the row's position first, whatever the point's status (SetWorldPos has no bad test either).
 * Per point, with Pos = the row's position in the attribute bank (f32):
 *   status 0  updated: the row's normal, min_dist and max_dist are rewritten;
 *          1  the point is flagged bad (asd_map_point_bad; :369): normal and range untouched;
 *          2  no table entry names the row (:381) -- a row beyond the row tables included: untouched;
 *          3  ref_kf[i] is not in the table, or its row does not name the point: untouched.  The reference cannot reach this state
 *             (MapPoint::EraseObservation re-seats mpRefKF); what it would do there -- std::map::operator[] inserting index 0 and reading
 *             keypoint 0's octave (:397) -- is NOT restated.
 * The tests apply in this order.  The observers of a point are ALL table entries that name it, no bad-keyframe test, as mObservations is
 * walked (:386-393), in ASCENDING KEYFRAME ID (the section's standing rule for pointer-order walks).  level = the octave of ref_kf's entry
 * for the point; scaleFactor[] and nLevels are the context's own (asd_get_scale_tables); an octave >= nLevels (the reference would read
 * past mvScaleFactors) takes the factor 0.  The reference leaves the arithmetic to OpenCV; the library's rule is
 *   d      = Pos - Ow_kf                                              f32, per component
 *   nrm    = sqrt(((double)dx*dx + (double)dy*dy) + (double)dz*dz)    f64 (the products are exact)
 *   unit_k = (float)((double)d_k * (1.0 / nrm))
 *   normal = normal + unit                                            f32, one observer after the other in ascending keyframe id, from zero
 *   mNormalVector_k = (float)((double)normal_k * (1.0 / (double)n_obs))
 *   dist          = (float)nrm  with kf = ref_kf
 *   mfMaxDistance = dist * scaleFactor[level]                         one f32 product
 *   mfMinDistance = mfMaxDistance / scaleFactor[nLevels - 1]          one correctly rounded f32 division
 * A point that sits on a camera centre follows IEEE arithmetic (inf / NaN), as the reference would; it is not an error.
 * normal / min_dist / max_dist (each may be NULL) return what the bank holds for the rows after the call, for every status.
 * ASD_ERR_INVALID (asd_last_error names the culprit): a row < 0 or beyond the attribute bank's capacity (its position was never put);
 * a row named twice; any live keyframe without octaves or without a centre; an open asd_prep_async bracket or an unfinished call armed with
 * asd_track_async (the attribute bank may be written on the second stream: asd_debug_bank_get's conditions).  ASD_ERR_CAPACITY: more than
 * 2^20 points per call, or more than 2^30 observations of the requested points together.  n == 0 is ASD_OK.  On any error neither bank nor
 * table is changed.  The call runs on the context's stream and returns drained; results are identical from run to run; it changes neither
 * the table nor its version: the search list of asd_track_local_points_map stays valid and the next stage reads the new attributes. */
typedef struct asd_normal_depth_args {
  int32_t n; const int32_t* rows;      /* bank rows of the points, distinct                                   */
  const int32_t* ref_kf;               /* [n] mpRefKF->mnId                                                   */
  const float* Xw;                     /* [n][3] or NULL: MapPoint::SetWorldPos in front of the update        */
  float* normal; float* min_dist; float* max_dist;   /* [n][3], [n], [n], each may be NULL: what the bank now holds */
  uint8_t* status;                     /* [n] or NULL                                                         */
} asd_normal_depth_args;
int asd_update_normal_and_depth(asd_ctx* ctx, asd_normal_depth_args* args);

/* The rule above for ONE point on the host, without a context or a device (the kernel's own functions, csrc/normal_depth.h): Ow[n_obs][3]
 * = the observers' centres in walk order, ref = the index of the reference keyframe among them, scale_level = scaleFactor[level],
 * scale_top = scaleFactor[nLevels - 1].  ASD_ERR_INVALID for n_obs < 1, ref outside [0, n_obs) or a NULL pointer.  It also gives a caller
 * the MapPoint constructor's normal (MapPoint.cc:60-77) for free. */
int asd_normal_and_depth_point(int32_t n_obs, const float* Ow /*[n_obs][3], in walk order*/, int32_t ref /*index into Ow*/,
                               const float* Pos, float scale_level, float scale_top, float normal[3], float* min_dist, float* max_dist);

/* ---- Optimizer::LocalBundleAdjustment over the table: the graph and the erase policy ----
 * asd_local_ba_graph is Optimizer.cc:418-467 and the structure of :484-593 for keyframe kf (which must be in the table) and
 * neigh[n_neigh <= 4096] = GetVectorCovisibleKeyFrames() as ids in its order (the full vector: the table's 10 links do not hold it).  An id
 * that is not in the table is legal: it counts as not bad and contributes no points.  Every walk over mObservations is in ASCENDING
 * KEYFRAME ID (the section's standing rule); an observer of a point is any table entry that names it.
 *   local_kfs / n_local_kfs   lLocalKeyFrames: kf, then the neighbours that are not bad, in the order given (:420-431)
 *   local_rows / n_points     lLocalMapPoints: the local keyframes in list order, their entries in ascending keypoint index, a point taken
 *                             at its first occurrence unless it is -1 or flagged bad (:435-449)
 *   fixed_kfs / n_fixed       lFixedCameras: local_rows in order, each point's observers in ascending id, an observer taken at its first
 *                             occurrence when it is neither local nor bad (:453-467)
 *   pose_kfs, pose_fixed / n_poses   local and fixed keyframes together in ascending id -- asd_ba_problem's pose order; pose_fixed = 1 for
 *                             the members of lFixedCameras (the caller ORs in mnId == 0 || GetGlobalMapFlag(), :490).  A local keyframe
 *                             without any edge is listed all the same: asd_local_ba accepts idle vertices.
 *   point_rank[n_points]      the index of local_rows[i] among the local rows sorted ascending -- asd_ba_problem's point order.  It equals
 *                             ascending mnId when the caller hands out bank rows in creation order; a caller that does not renumbers.
 *   e_* / n_edges             the edges in the reference's insertion order (:534-593): the points in local_rows order, each point's observers
 *                             in ascending id, bad keyframes skipped (:556).  e_point = the point's point_rank, e_pose = the index into
 *                             pose_kfs, e_kf = the keyframe id, e_idx = the keypoint index (mit->second), e_octave = mvKeysUn[e_idx].octave
 *                             from the octave plane.  e_obs (mvKeysUn[e_idx].pt) and e_info (inv_sigma2[e_octave], x 10 for a global-map
 *                             point) are the caller's to fill.
 *   Xw[n_points][3]           optional (NULL = skip): the points' positions from the attribute bank in point_rank order, widened to f64
 *                             (Converter::toVector3d).  When asked for, the bank conditions of asd_update_normal_and_depth apply: the rows lie
 *                             inside the bank's capacity, no asd_prep_async bracket is open.
 * Capacities are the caller's.  When one is too small the call returns ASD_ERR_CAPACITY with ALL counts set to what is needed; it changes
 * nothing and may simply be repeated.  ASD_ERR_INVALID: kf not in the table; a duplicate id, a negative id or kf itself in neigh; any
 * live keyframe without octaves.  ASD_ERR_CAPACITY also when the local keyframes' rows together exceed asd_update_local_map's bound, or
 * the local points (2^20) or their observations together (2^30) asd_update_normal_and_depth's.  The call runs on the context's stream,
 * returns drained and undoes every mark it set; it changes neither the table nor its version (the search list stays valid); results
 * are identical from run to run.  After ASD_OK the graph stays resident for asd_local_ba_apply -- the points' observer segments and the
 * edge -> entry map -- until any asd_map_* call changes the table. */
typedef struct asd_ba_graph_args {
  int32_t kf; int32_t n_neigh; const int32_t* neigh;
  int32_t kf_capacity;    int32_t* local_kfs;  int32_t n_local_kfs;
  int32_t point_capacity; int32_t* local_rows; int32_t* point_rank; int32_t n_points;
  int32_t fixed_capacity; int32_t* fixed_kfs;  int32_t n_fixed;
  int32_t pose_capacity;  int32_t* pose_kfs;   uint8_t* pose_fixed; int32_t n_poses;
  int32_t edge_capacity;  int32_t* e_point; int32_t* e_pose; int32_t* e_kf; int32_t* e_idx; uint8_t* e_octave; int32_t n_edges;
  double* Xw;
} asd_ba_graph_args;
int asd_local_ba_graph(asd_ctx* ctx, asd_ba_graph_args* args);

/* The erase policy of Optimizer.cc:652-697 over the resident graph: erase[n_edges] = one byte per edge of the last asd_local_ba_graph,
 * chi2 > 5.991 || !isDepthPositive as the caller read it from asd_ba_result; n_points = that graph's.  The reference erases one pair after
 * the other (KeyFrame::EraseMapPointMatch + MapPoint::EraseObservation, MapPoint.cc:119-142): a point whose nObs reaches <= 2 turns bad on
 * the spot and loses ALL its entries (SetBadFlag, :180-197), later pairs of that point are no-ops.  The edges are grouped by point, so
 * this has a closed form, which is what the device evaluates: left = Observations(r) - flagged edges of r, where Observations counts
 * every table entry that names r, the bad keyframes' included; the point turns bad exactly when it has a flagged edge and left <= 2.
 *   n_erased              the observations EraseObservation itself removed (the pairs that were not no-ops)
 *   bad_rows / n_bad      the points that turned bad, in local_rows order (= the order it happened); bad_capacity too small is
 *                         ASD_ERR_CAPACITY with n_bad and n_erased set, nothing changed, and the call may be repeated
 *   new_ref[n_points]     in local_rows order: the lowest remaining observer id for a point that lost an observation and did not turn
 *                         bad, -1 otherwise.  mpRefKF is re-seated only when its own observation goes and ends at the lowest id among the
 *                         observers finally left: the caller assigns new_ref when the point's mpRefKF was among its erased keyframes.
 * apply = 1 leaves the table as the reference leaves the map: every flagged edge's entry -1, every entry of a point that turned bad -1 in
 * every row (through the resident segments), that point's bad byte set.  When a flagged edge exists the table's version is bumped and the
 * search list of asd_track_local_points_map is invalid; without one nothing changes.  apply = 1 consumes the graph either way; apply = 0
 * changes nothing and keeps it.  ASD_ERR_INVALID, the table untouched: no resident graph; the table has changed since the graph call;
 * n_edges or n_points differ from the graph's; an unfinished call armed with asd_track_async. */
typedef struct asd_ba_apply_args {
  int32_t n_edges; const uint8_t* erase;
  int32_t apply;
  int32_t n_erased;
  int32_t bad_capacity; int32_t* bad_rows; int32_t n_bad;
  int32_t n_points; int32_t* new_ref;
} asd_ba_apply_args;
int asd_local_ba_apply(asd_ctx* ctx, asd_ba_apply_args* args);

/* ---- ORBmatcher::Fuse's side effects and MapPoint::Replace over the table ----
 * asd_fuse_apply is the half of Fuse that asd_fuse_search* leave out: what the reference does with bestIdx, in its order, with every
 * Replace seen by the candidates behind it.  cand[n] are the candidates as bank rows in the caller's list order (-1 = null pointer),
 * best_idx[n] the keypoint of kf the search chose (-1 = bestDist > TH_LOW or not searched).  A candidate with cand < 0 or best_idx < 0
 * takes no step (action 0).  Observations(r) = the number of table entries that name r (the section's standing precondition: a point at
 * most once per row); a row no entry has ever named counts 0 -- a point created this keyframe.
 *   mode 0  Fuse(pKF, vpMapPoints, th), ORBmatcher.cc:842-957: at its turn a candidate that is flagged bad or that kf's row names AT THAT
 *           MOMENT is skipped (:849, action 7); then :939-955 literally -- an empty entry takes the candidate (AddObservation + AddMapPoint),
 *           an entry whose point is flagged bad does nothing, otherwise Observations(pMPinKF) > Observations(pMP) (strict) decides who is
 *           replaced.
 *   mode 1  Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :986-1083 followed by SearchAndFuse's loop, LoopClosing.cc:619-627.  Pass 1, in
 *           order: the gate is "flagged bad, or named by kf's row AT ENTRY" (spAlreadyFound is a snapshot); an empty entry takes the
 *           candidate; an occupied entry whose point is not bad is noted as vpReplacePoint[i] (it may be a candidate pass 1 put there).
 *           Pass 2, in order: vpReplacePoint[i]->Replace(vpPoints[i]) with no test at all.  A point noted twice goes through Replace
 *           twice; the second time its observations are gone (n_moved = n_dropped = 0) and it is reported with action 3 all the same: the
 *           host owes mpReplaced and the found / visible transfer for it.
 *   mode 2  the loop fusion of CorrectLoop, LoopClosing.cc:540-555: cand[i] = mvpCurrentMatchedPoints[i], best_idx[i] = i.  An occupied
 *           entry gives pCurMP->Replace(pLoopMP) with no bad test and no comparison, an empty entry takes the point.
 * MapPoint::Replace(L -> W), MapPoint.cc:206-244: L == W is a no-op; otherwise L is flagged bad and loses every entry: for each of L's
 * observations (k, idx), the entry becomes W when no entry of keyframe k names W (Observations(W) grows by one), and -1 otherwise.  The
 * keyframes of one point are distinct, so the result does not depend on the order of that walk and no ordering rule is needed.  W may be a
 * point that is itself flagged bad (modes 1 and 2 have no test): it receives the entries all the same, as in the reference.
 *   action  0 no step;  1 observation added at an empty entry;  2 the candidate was replaced by the keyframe's point (mode 0);
 *           3 the keyframe's point was replaced by the candidate;  4 the entry's point is flagged bad: nothing happens, nFused still counts
 *           (:942, :1073);  5 Replace of a point by itself (mode 2);  6 mode 2 only: the entry is empty but the candidate already observes
 *           kf elsewhere -- the reference's AddObservation is a no-op there while AddMapPoint would write a second entry; the table cannot
 *           hold that state and it is NOT restated: the step is skipped;  7 skipped at its turn by the gate.
 *   other   pMPinKF as the walk met it (bank row), -1 = the entry was empty / no step
 *   obs_cand, obs_other   Observations() of the two directly in front of the step (mode 1, action 3: in front of pass 2's Replace); 0
 *           where there is no step (actions 0 and 7) and for the missing side of actions 1 and 6
 *   n_moved, n_dropped    Replace: observations re-seated on the winner / erased because the winner is already in that keyframe
 *   n_fused the number of actions 1 .. 5 in every mode.  Modes 0 and 1: nFused as the reference counts it (:956, :1080).  Mode 2: the steps
 *           the loop of :540-555 took, the self-Replace of action 5 INCLUDED (the reference calls Replace there, which returns at once);
 *           the skipped step of action 6 is not counted.  Written only when the call returns ASD_OK.
 * From action and other the host derives, in order, the (loser, winner) pairs for mpReplaced / IncreaseFound / IncreaseVisible and the
 * winners whose ComputeDistinctiveDescriptors is due.
 * apply = 1 leaves the table as the reference leaves the map: every moved, dropped or added entry rewritten, every loser's bad byte set,
 * and -- when an action 1, 2 or 3 occurred -- the version bumped, so the search list of asd_track_local_points_map is invalid.  Without
 * such an action the table keeps its version.  apply = 0 changes nothing.  Results are identical from run to run.
 * ASD_ERR_INVALID (asd_last_error names the culprit): kf is not in the table; a best_idx outside kf's row; a candidate row >= 0 named
 * twice; a row >= 2^28 or < -1; an unknown mode; an unfinished call armed with asd_track_async.  ASD_ERR_CAPACITY: n > 2^20, or more than
 * 2^30 observations of the involved points together.  On any error the table is untouched.  Neither octaves nor centres are needed.  The
 * call runs on the context's stream and returns drained. */
typedef struct asd_fuse_apply_args {
  int32_t kf;                      /* pKF: must be in the table                                                          */
  int32_t mode;                    /* 0, 1, 2: above                                                                     */
  int32_t n; const int32_t* cand;  /* the candidates as bank rows, in the caller's list order; -1 = null pointer         */
  const int32_t* best_idx;         /* [n] keypoint of kf the search chose, -1 = none                                     */
  int32_t apply;                   /* 0: outcomes only, the table is left as it was                                      */
  uint8_t* action;                 /* [n] outcome codes above                                                            */
  int32_t* other;                  /* [n] pMPinKF as the walk met it (bank row), -1 = the entry was empty / no step      */
  int32_t* obs_cand; int32_t* obs_other;   /* [n] Observations() of the two in front of the step                         */
  int32_t* n_moved; int32_t* n_dropped;    /* [n] Replace: observations re-seated on the winner / erased                 */
  int32_t n_fused;                 /* out: nFused as the reference counts it                                             */
} asd_fuse_apply_args;
int asd_fuse_apply(asd_ctx* ctx, asd_fuse_apply_args* args);

/* KeyFrame::GetMapPointMatches(): the row of keyframe kf as it stands, rows[*n].  ASD_ERR_CAPACITY with *n = the row's length when
 * `capacity` is too small, ASD_ERR_INVALID for an unknown kf.  Changes neither the table nor its version. */
int asd_map_get(asd_ctx* ctx, int32_t kf, int32_t capacity, int32_t* rows, int32_t* n);

/* The points of n_kfs keyframes: the keyframes in the order given, their entries in ascending keypoint index, a point taken at its first
 * occurrence unless it is -1 or flagged bad -- the rule of UpdateLocalPoints, i.e. vpFuseCandidates of SearchInNeighbors (LocalMapping.cc:
 * 599-615) and the gathering loop of mvpLoopMapPoints in ComputeSim3.  An id that is not in the table contributes nothing; an id named
 * twice is ASD_ERR_INVALID; ASD_ERR_CAPACITY with *n = the count needed when `capacity` is too small.  Changes neither the table nor its
 * version. */
int asd_map_points(asd_ctx* ctx, int32_t n_kfs, const int32_t* kfs, int32_t capacity, int32_t* rows, int32_t* n);

/* Test aid: out = {live keyframes, live entries, slot capacity, arena capacity, row-table capacity, growths of the slot table, of the arena,
 * of the row tables}. */
int32_t asd_debug_map(asd_ctx* ctx, int64_t out[8]);

/* Test aid: rows [first_row, first_row + n) of the descriptor bank (desc[n][128], or NULL) and of the attribute bank (attr[n][8] = Xw,
 * normal, min_dist, max_dist as asd_mpbank_put stored them, or NULL), read as a consumer reads them: the copies are enqueued on the
 * context's stream and that stream alone is waited for -- NOT the second stream of asd_prep_async, so a bracket that does not order its
 * writes shows.  ASD_ERR_INVALID for rows outside the respective bank's capacity, while a bracket is open and while a call started with
 * asd_track_async is outstanding.  A row never written holds whatever the allocation held. */
int32_t asd_debug_bank_get(asd_ctx* ctx, int32_t first_row, int32_t n, float* desc, float* attr);

/* Runs `reps` back-to-back repetitions of the ASDNet forward on resident buffers and
 * returns the average per-repetition device time (hipEvents on the ctx stream). */
int asd_describe_timed(asd_ctx* ctx, const uint8_t* d_patches, int32_t n, float* d_desc,
                       int32_t reps, float* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* ASD_SLAM_H */
