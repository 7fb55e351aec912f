/*
 * ysmr_hip.h -- C ABI of libysmr_hip.so: the MI355X (gfx950) implementation of YSMR's per-frame
 * detect-and-link hot path.  Plain pointers and sizes only; every pointer named *_dev is a HIP
 * device pointer owned by the caller (e.g. torch.Tensor.data_ptr()); `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  No entry point allocates on the per-frame path
 * (ysmr_tracker_create/destroy own the tracker state).  Every function returns 0 (YSMR_OK) or a
 * YSMR_ERR_* code and never throws -- mirroring the reference's "log + return None" convention
 * (ysmr/track_eval.py:50-77, ysmr/main.py:92-95); ysmr_last_error() gives the message.
 *
 * Reference interfaces replaced (files under /root/reference):
 *   ysmr_unpack_dib_batch cv2.VideoCapture.read (uncompressed AVI frames)   ysmr/track_eval.py:159
 *   ysmr_mjpeg_decode_batch cv2.VideoCapture.read (Motion-JPEG AVI frames)  ysmr/track_eval.py:159
 *   ysmr_annotate_batch   cv2.putText + cv2.circle + cv2.VideoWriter.write   ysmr/track_eval.py:1423-1449
 *   ysmr_view_*           cv2.drawContours + cv2.putText + cv2.circle of the window 'display video analysis' opens, into a file
 *                         ysmr/track_eval.py:306-325, 353-362
 *   ysmr_mjpeg_batch      cv2.VideoWriter.write with fourcc 'MJPG' ('save video fourcc codec')   ysmr/track_eval.py:1400-1449
 *   ysmr_threshold_batch  cv2.cvtColor + cv2.GaussianBlur + 2 x cv2.adaptiveThreshold
 *                         ysmr/track_eval.py:180-208
 *   ysmr_mean_threshold_batch  cv2.cvtColor + cv2.GaussianBlur + cv2.meanStdDev + threshold_list
 *                         moving average + cv2.threshold   ysmr/track_eval.py:180-182, 219-253
 *   ysmr_components_batch scipy binary_propagation + cv2.findContours + cv2.minAreaRect +
 *                         reshape_result   ysmr/track_eval.py:211-303, ysmr/helper_file.py:1336-1347
 *   ysmr_detect_batch     both of the above in one call
 *   ysmr_luminosity_batch cv2.boxPoints + cv2.fillPoly + cv2.mean per contour ('include luminosity in tracking
 *                         calculation')   ysmr/track_eval.py:290-300
 *   ysmr_tracker_*        CentroidTracker.__init__/update   ysmr/tracker.py:37-71, 93-230
 *                         (ysmr_tracker_dimensions / _update3 / _run3 / _peek3: the same with (x, y, luminosity)
 *                         centroids, tracker.py:111, 151)
 *                         GaussianSumFIR.correct/predict    ysmr/gsff.py:204-347
 *                         row emission                      ysmr/track_eval.py:313-316
 *   ysmr_gsff_gains       GaussianSumFIR.generate_n_i/compute_lsf_gain  ysmr/gsff.py:87-153
 *   ysmr_rows_sort        sort_list (order by TRACK_ID, POSITION_T)  ysmr/helper_file.py:1538-1574
 *   ysmr_select_tracks    select_tracks + find_good_tracks   ysmr/track_eval.py:408-843
 *   ysmr_evaluate_tracks  evaluate_tracks (statistics, not the plots)  ysmr/track_eval.py:846-1318
 *   ysmr_plot_*           large_xy_plot, rose_graph, angle_distribution_plot   ysmr/plot_functions.py:29-257
 *   ysmr_violin_*,        violin_plot and the categories of evaluate_tracks    ysmr/plot_functions.py:260-370,
 *   ysmr_plot_violins                                                          ysmr/track_eval.py:1151-1303
 *   ysmr_rows_columns,    save_list text + get_data (pandas.read_csv) + save_df_to_csv
 *   ysmr_rows_format_csv  ysmr/helper_file.py:1403-1478, 860-905, 1366-1400  (host functions)
 *   ysmr_csv_parse_typed  get_data (pandas.read_csv with the dtype annotate_video passes) for an `*_analysed.csv`
 *                         ysmr/helper_file.py:860-905, ysmr/track_eval.py:1354-1369
 *   ysmr_marks_build,     the table's rows looked up frame by frame (curr_frame_data, one mark per row)
 *   ysmr_marks_workspace_bytes   ysmr/track_eval.py:1419-1447
 */
#ifndef YSMR_HIP_H
#define YSMR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YSMR_OK            0
#define YSMR_ERR_ARG       1   /* bad argument (null pointer, size, unsupported option) */
#define YSMR_ERR_HIP       2   /* a HIP runtime call failed */
#define YSMR_ERR_CAPACITY  3   /* a fixed-capacity buffer would overflow (tracks, workspace) */
#define YSMR_ERR_STATE     4   /* handle used in the wrong state */

/* 15 still: ysmr_annotate_batch with its mark struct, and later the ysmr_plot_*, ysmr_mjpeg_*, ysmr_violin_*, ysmr_mjpeg_decode_*, ysmr_view_*, ysmr_csv_*, ysmr_table_*, ysmr_marks_* and ysmr_xlsx_* functions, were ADDED under this number
 * -- no existing entry point, struct or constant changed, so every caller written against 15 keeps working; only a caller
 * of a new function needs a library that has it (the loader reports a missing symbol by name). */
#define YSMR_ABI_VERSION   15

/* per-frame detection status bits (status_dev) */
#define YSMR_DET_OVERFLOW  1   /* more components than max_det: detections truncated */
#define YSMR_DET_ARENA     2   /* geometry scratch arena exhausted: some rectangles missing */
#define YSMR_DET_STALLED   4   /* an internal grid barrier timed out: this call's outputs are undefined; the next call on
                                 the same buffers clears everything and is valid again */

/* cv_flavour: which OpenCV the a1 / a6 arithmetic follows.  opencv-contrib-python is an unpinned third-party
 * dependency of the reference (setup.py:29, "openCV v3 or v4"); two of its results changed between releases:
 *   0                     OpenCV >= 4.5.1: 15-bit BGR2GRAY coefficients; cv::minAreaRect angle in (0, 90] (the
 *                         restated hull order + rotating calipers produce [0, 90]: an axis-aligned box is
 *                         reported with angle 90, or 0, whichever of its equal-area sides is visited last)
 *   YSMR_CV_ANGLE_PRE451  OpenCV < 4.5.1: the same rectangle with its angle in [-90, 0) and width / height named
 *                         the other way round (angle 90 becomes -90 with the sides as they are)
 *   YSMR_CV_GRAY_3X       OpenCV 3.x: 14-bit BGR2GRAY coefficients (1868 / 9617 / 4899); no effect on gray input
 * (upstream-recollection, like the rest of the cv2 restatement: the image half is parity-unpinned) */
#define YSMR_CV_ANGLE_PRE451 1
#define YSMR_CV_GRAY_3X      2
/* A scheduling hint carried in the same argument (results are the same bytes with or without it): the caller runs the
 * one-launch link (ysmr_tracker_run with capacity and max_det <= 2048 or so) on another stream while this call's kernels
 * execute.  ysmr_threshold_batch then takes the float32-chain kernel, whose resident grid leaves registers and LDS on
 * every compute unit, and ysmr_components_batch launches k_windows / k_geometry with the smaller resident grids that
 * leave the link's workgroups their 59 KB of LDS per unit (detection alone is ~8 % slower that way). */
#define YSMR_BESIDE_LINK     4
/* ... and the hint for a handle that links a whole batch with one launch (ysmr_tracker_batched): that launch holds ONE
 * compute unit for the length of the batch.  The matrix-pipe threshold kernel, which gives every compute unit one
 * workgroup, then cuts its rows for 248 workgroups (31 on each of the 8 XCDs) instead of 256 -- whichever XCD the link sits
 * on, none gets a workgroup it cannot place before another has finished (same bytes). */
#define YSMR_BESIDE_BATCH_LINK 8
/* ... and for the two-launch link of large tables (k_link + k_track, 4K: 5000 tracks): its launches want a fat workgroup and
 * thousands of waves placed every ~30 us, so the matrix-pipe threshold kernel keeps to 160 of the 256 compute units (round 5's
 * kernel at 3840 x 2160: 24.2 k frames/s end to end on 128 or 160 workgroups, 23.7 k on 192, 21.9 k on 248 -- and a threshold
 * fraction of 0.13 / 0.16 / 0.19 / 0.23, profiles/r05_sweep_4k_thr_grid.log; same bytes). */
#define YSMR_BESIDE_SPLIT_LINK 16
#define YSMR_CV_FLAVOUR_MASK 31

/* One output row: a live track in one frame (ysmr/track_eval.py:313-316,
 * CSV columns TRACK_ID,POSITION_T,POSITION_X,POSITION_Y,WIDTH,HEIGHT,DEGREES_ANGLE). */
typedef struct ysmr_row {
    int32_t frame;        /* POSITION_T */
    int32_t track_id;     /* TRACK_ID */
    double  x, y;         /* POSITION_X/Y: GSFF-filtered (or raw when GSFF is disabled) */
    float   w, h, angle;  /* WIDTH, HEIGHT, DEGREES_ANGLE; all 0 while the track is "disappeared" */
    int32_t disappeared;  /* consecutive frames without a detection (0 = matched this frame) */
} ysmr_row;

typedef struct ysmr_tracker ysmr_tracker; /* opaque; bound to one device + used from one thread */

int         ysmr_abi_version(void);
const char *ysmr_last_error(void);        /* message of the calling thread's last failing call */

/* ---- frame ingest: f1 ------------------------------------------------------------------- */

/* What cv2.VideoCapture.read() (ysmr/track_eval.py:159) does to a frame of an UNCOMPRESSED AVI once it has its bytes:
 * DIB rows are stored bottom-up (bottom_up = 1) with a stride padded to 4 bytes; 8-bit frames with a palette that
 * is not the gray ramp are expanded to BGR.  raw_dev: u8 [n_frames][raw_frame_bytes], the 'movi' chunk bodies as
 * they are in the file; bytes_per_pixel 1 or 3; palette_dev: NULL, or u8 [256][3] (B, G, R) for 1-byte pixels.
 * frames_dev: u8 [n_frames][height][width][channels], channels = 3 with a palette, else bytes_per_pixel -- the
 * layout ysmr_threshold_batch / ysmr_detect_batch read; 4-byte aligned. */
int ysmr_unpack_dib_batch(void *stream, const uint8_t *raw_dev, int n_frames, size_t raw_frame_bytes, int height,
                          int width, int bytes_per_pixel, int row_stride, int bottom_up,
                          const uint8_t *palette_dev, uint8_t *frames_dev);

/* HOST function: n bytes of the open file `fd`, from `offset` on, into `dst` (e.g. the pinned staging buffer of a frame
 * feed) by `threads` positional reads side by side (<= 0: 8).  What cap.read() does for an uncompressed file, a batch of
 * frames at a time (ysmr/track_eval.py:159). */
int ysmr_file_read(int fd, void *dst, size_t n, long long offset, int threads);

/* ---- annotated output video ------------------------------------------------------------- */

/* One mark of the annotated video (ysmr/track_eval.py:1423-1447): a track's position in one frame, truncated to
 * integers, its id, and how it is drawn -- style 0: (B, G, R) = (0, 255, 0); style 1 (not moving): (15, 165, 253);
 * style 2 (turn point): (255, 255, 255) and a dot of radius 1 instead of a single pixel.  16 bytes. */
typedef struct {
    int32_t  x, y;
    uint32_t track_id;
    uint32_t style;
} ysmr_mark;

/* What cv2.putText + cv2.circle + cv2.VideoWriter.write (ysmr/track_eval.py:1435-1449) do to a batch of frames, for an
 * uncompressed 24-bit stream.  frames_dev: u8 [n_frames][height][width][channels], channels 1 (gray: B = G = R) or 3
 * (B, G, R).  The marks of frame i are marks_dev[first_dev[i] .. first_dev[i + 1]), in table order (first_dev: int64
 * [n_frames + 1], non-decreasing; it may point into a longer array, first_dev[0] need not be 0); first_dev = NULL: no
 * marks, the frames are only packed.  Every frame is painted as a sequential painter would: mark by mark, the id's
 * decimal digits (5 x 7 pixels each, 6 apart, top-left corner at (x - 10, y - 16)) and then the dot at (x, y), later
 * paint over earlier, pixels outside the frame dropped.  out_dev: n_frames stored DIB frames, out_frame_bytes apart
 * (>= out_stride * height), rows out_stride bytes apart (a multiple of 4, >= 3 * width; the bytes behind a row's
 * pixels are zeroed), the last row first if bottom_up.  out_dev 4-byte aligned. */
int ysmr_annotate_batch(void *stream, const uint8_t *frames_dev, int n_frames, int height, int width, int channels,
                        const ysmr_mark *marks_dev, const int64_t *first_dev,
                        uint8_t *out_dev, int out_stride, size_t out_frame_bytes, int bottom_up);

/* ---- detection view ---------------------------------------------------------------------- */

/* ADDED under ABI 15 (see above).  What the window "... unfiltered possible detections" of track_bacteria shows
 * (ysmr/track_eval.py:306-325, 353-362), as stored DIB frames: the frame with every detection's box outlined in blue and
 * every live track's id and centroid in green.  PIXEL RULE (the project's own; the cv2 half is parity-unpinned, like
 * ysmr_luminosity_batch's): the frame expanded to B, G, R, then two layers, later over earlier --
 *   boxes   for every detection d < det_count[frame] the closed outline of np.intp(cv2.boxPoints(rect)), the corners
 *           ysmr_luminosity_batch reports in corners_dev: the four 8-connected lines corner i-1 -> corner i, each walked from
 *           its left end, pixels outside the frame dropped and nothing clipped beforehand, (B, G, R) = (255, 0, 0); a box
 *           whose corners coincide paints that pixel (cv2.drawContours with thickness <= 1 and LINE_8, as recollected);
 *   tracks  for every row of the frame the id's decimal digits and the single-pixel dot at (int(x), int(y)), truncated
 *           toward zero: exactly style 0 of ysmr_annotate_batch, (0, 255, 0).  Rows of "disappeared" tracks are painted
 *           too (upstream goes through objects.items(), which holds them); a row whose position is not finite is not.
 * Upstream's "FPS: n" lettering is not drawn.  The work per outline is bounded by the frame's size, wherever the corners
 * are (they are moved to +-2^20 at most).
 *
 * ysmr_view_boxes_batch packs the frames exactly as ysmr_annotate_batch does with first_dev = NULL (same arguments, same
 * layout, same zeroed row padding) and paints the box layer; det_dev / det_count_dev / max_det as ysmr_detect_batch leaves
 * them (the cv_flavour angle is already in the detections).
 * ysmr_view_tracks_batch paints the track layer into such frames, later on the same stream or behind an event: the rows
 * rows_dev[*row_begin_dev .. *row_end_dev) -- two DEVICE integers, e.g. the row counter of ysmr_tracker_run copied before
 * and after the batch's link, so that no host synchronisation is needed; the range is cut to [0, rows_capacity) -- in any
 * order; a row goes into frame row.frame - first_frame_index and is skipped if that is outside [0, n_frames).
 * ysmr_view_batch_host: HOST function, both layers on host arrays with the same pixel-deciding code (row_begin / row_end
 * are values here; rows_host may be NULL if there are none). */
int ysmr_view_boxes_batch(void *stream, const uint8_t *frames_dev, int n_frames, int height, int width, int channels,
                          const float *det_dev, const int32_t *det_count_dev, int max_det,
                          uint8_t *out_dev, int out_stride, size_t out_frame_bytes, int bottom_up);
int ysmr_view_tracks_batch(void *stream, const ysmr_row *rows_dev, int64_t rows_capacity, const int64_t *row_begin_dev,
                           const int64_t *row_end_dev, int32_t first_frame_index, int n_frames, int height, int width,
                           uint8_t *dib_dev, int stride, size_t frame_bytes, int bottom_up);
int ysmr_view_batch_host(const uint8_t *frames_host, int n_frames, int height, int width, int channels,
                         const float *det_host, const int32_t *det_count_host, int max_det,
                         const ysmr_row *rows_host, int64_t row_begin, int64_t row_end, int32_t first_frame_index,
                         uint8_t *out_host, int out_stride, size_t out_frame_bytes, int bottom_up);

/* ---- threshold view ---------------------------------------------------------------------- */

/* ADDED under ABI 15 (see above).  What the windows 'threshold' (the final mask behind binary_propagation,
 * ysmr/track_eval.py:271) and 'Adaptive double threshold markers' (:210) of track_bacteria show, and a composite of both over
 * the frame, as stored DIB frames laid out as ysmr_annotate_batch's (out_stride a multiple of 4 and >= 3 * width, the bytes
 * behind a row's pixels zeroed, out_frame_bytes >= out_stride * height, out_dev 4-byte aligned, the last row first if
 * bottom_up; bytes between two frames are not touched).  cls_dev / mask_dev: u8 [n_frames][height][width], contiguous, as
 * ysmr_detect_batch leaves them (cls bit 0 thresh, bit 1 markers, other bits ignored; mask != 0: kept).  PIXEL RULE, (B, G, R):
 *   mode 0 (mask)     255, 255, 255 where mask != 0, else 0, 0, 0;
 *   mode 1 (markers)  255, 255, 255 where bit 1 of cls is set, else 0, 0, 0 (mask_dev may be NULL);
 *   mode 2 (classes)  the first that holds: mask != 0 and bit 1 set (0, 0, 255); mask != 0 (0, 255, 255); bit 0 set
 *                     (255, 0, 0) -- passed the low threshold, dropped by the hysteresis --; else the frame's own pixel
 *                     (gray g: g, g, g).  A function of (cls & 3, mask != 0) alone, total.
 * frames_dev: u8 [n_frames][height][width][channels], channels 1 or 3; read in mode 2 only and may be NULL otherwise.
 * YSMR_ERR_ARG, nothing launched or written: NULL cls or out, NULL mask in modes 0 and 2, NULL frames in mode 2, channels
 * outside {1, 3}, a mode outside 0 .. 2, a layout that breaks the conditions above.
 * ysmr_thrview_batch_host: HOST function, the same on host arrays with the same pixel-deciding code. */
int ysmr_thrview_batch(void *stream, const uint8_t *frames_dev, const uint8_t *cls_dev, const uint8_t *mask_dev,
                       int n_frames, int height, int width, int channels, int mode,
                       uint8_t *out_dev, int out_stride, size_t out_frame_bytes, int bottom_up);
int ysmr_thrview_batch_host(const uint8_t *frames_host, const uint8_t *cls_host, const uint8_t *mask_host,
                            int n_frames, int height, int width, int channels, int mode,
                            uint8_t *out_host, int out_stride, size_t out_frame_bytes, int bottom_up);

/* ---- frame ingest: Motion-JPEG ------------------------------------------------------------------ */

/* ADDED under ABI 15 (see above).  bits of status_dev[i] of ysmr_mjpeg_decode_batch */
#define YSMR_MJPEGD_UNSUPPORTED 1  /* not baseline SOF0 / 8 bit / one interleaved scan of all components, sampling other than
                                      the call's, geometry other than the call's, APP14 present, > 1 SOS, arithmetic coding */
#define YSMR_MJPEGD_CORRUPT     2  /* a code that no table holds, a coefficient index past 63, an entropy segment that ends
                                      before its MCUs, a missing or out-of-sequence RSTn, no SOS / SOF / DQT the scan needs */

/* Bytes of scratch ysmr_mjpeg_decode_batch needs (mostly the quantised coefficients, 2 bytes per sample of the padded
 * planes, and for three components the decoded planes, 1 byte per sample).  0 for arguments it refuses. */
size_t ysmr_mjpeg_decode_workspace_bytes(int n_frames, int height, int width, int channels, int sampling);

/* What cv2.VideoCapture.read does with a Motion-JPEG AVI, for a batch of '00dc' chunk bodies as they are in the file, back
 * to back: JPEG i is chunks_dev[offsets_dev[i] .. offsets_dev[i + 1]); bytes behind its EOI are ignored.  sampling: 0 = one
 * component (channels 1), 1 = 4:4:4, 2 = 4:2:2 (2 x 1), 3 = 4:2:0 (2 x 2) (channels 3: B, G, R).  frames_dev: u8
 * [n_frames][height][width][channels], the layout ysmr_threshold_batch reads, byte for byte what libjpeg-turbo's default
 * decode (accurate integer IDCT, fancy upsampling) delivers.  status_dev[i] = 0, or YSMR_MJPEGD_* bits for a frame outside
 * the supported subset or damaged: such a frame's pixels are undefined, inside its own height * width * channels bytes
 * and nowhere else, and no read leaves its own chunk.  Asynchronous on `stream`.  workspace_dev: 256-byte aligned,
 * workspace_bytes >= ysmr_mjpeg_decode_workspace_bytes(...); no state is kept in it and nothing found in it is used. */
int    ysmr_mjpeg_decode_batch(void *stream, const uint8_t *chunks_dev, const int64_t *offsets_dev, int n_frames,
                               int height, int width, int channels, int sampling,
                               void *workspace_dev, size_t workspace_bytes,
                               uint8_t *frames_dev, int32_t *status_dev /* [n_frames] */);

/* ADDED under ABI 15 (see above).  ysmr_mjpeg_decode_batch for files WITHOUT restart markers -- what cameras, ffmpeg, OpenCV and
 * Pillow write.  ysmr_mjpeg_decode_batch gives a lane to each restart interval, so such a frame is one lane's work there; here
 * its entropy data is cut into subsequences of fixed size that are decoded side by side, every one from an assumed state first
 * and again from its predecessor's exit state until no entry state changes, which makes the result EXACT for every stream (a
 * decoder started at a wrong bit falls into step with the code after a few symbols; one that never does costs time only).  A
 * frame WITH a restart interval is decoded as ysmr_mjpeg_decode_batch decodes it.  Same supported subset, same status bits, same
 * bytes in frames_dev, same rules for the workspace and for what is read and written.
 * max_chunk_bytes: an upper bound of offsets_dev[i + 1] - offsets_dev[i] over the call, 1 .. 2^27 - 1 (the host knows the chunk
 * sizes, the offsets live on the device); it sizes the workspace, and a frame with a longer chunk is flagged
 * YSMR_MJPEGD_CORRUPT. */
size_t ysmr_mjpeg_decode_sync_workspace_bytes(int n_frames, int height, int width, int channels, int sampling,
                                              int max_chunk_bytes);   /* 0 for arguments the call refuses */
int    ysmr_mjpeg_decode_batch_sync(void *stream, const uint8_t *chunks_dev, const int64_t *offsets_dev, int n_frames,
                                    int height, int width, int channels, int sampling, int max_chunk_bytes,
                                    void *workspace_dev, size_t workspace_bytes,
                                    uint8_t *frames_dev, int32_t *status_dev /* [n_frames] */);
/* The two compile-time constants of it: bytes of a subsequence, subsequences a workgroup takes at a time (tests build streams
 * that cross these boundaries).  Either pointer may be NULL. */
void   ysmr_mjpeg_decode_sync_geometry(int *subsequence_bytes, int *subsequences_per_pass);

/* ---- frame ingest: TIFF stacks ------------------------------------------------------------------- */

/* ADDED under ABI 15 (see above).  bits of status_dev[i] of ysmr_tiff_decode_batch: what any strip of frame i met */
#define YSMR_TIFFD_BAD_CODE 1   /* LZW: a code above the next free entry (after a Clear: any code above 255 but Clear and EOI),
                                   or a 3839th data code without a Clear, for which the table has no room */
#define YSMR_TIFFD_SHORT    2   /* the strip's data (or an LZW EOI) ends before the strip's rows are full */
#define YSMR_TIFFD_OVERRUN  4   /* PackBits: a run that would pass the end of the strip */
#define YSMR_TIFFD_OLD_LZW  8   /* LZW: the body begins 0x00, then an odd byte -- the old LSB-first variant (libtiff's test) */
#define YSMR_TIFFD_TABLE    16  /* a row of strips_dev outside the call's geometry: nothing of it was read or written */

/* Bytes of scratch ysmr_tiff_decode_batch needs for n_frames frames cut into strips of rows_per_strip rows (the last one of
 * a frame shorter where the height is no multiple) whose bodies are body_bytes bytes together.  0 for what the call refuses:
 * n_frames, height or width not positive; channels not 1 or 3; compression not 1 (none), 5 (LZW) or 32773 (PackBits);
 * predictor not 1 or 2; photometric not 0 or 1 (one channel) or 2 (three); rows_per_strip not 1 .. height; body_bytes, the
 * bytes of a frame or the number of strips beyond 2^31 - 1. */
size_t ysmr_tiff_decode_workspace_bytes(int n_frames, int height, int width, int channels, int compression, int predictor,
                                        int photometric, int rows_per_strip, long long body_bytes);

/* The strips of n_frames pages of a TIFF stack, as they are stored, to frames: strips_dev is int32 [n_strips][5] = (frame,
 * first row, rows, offset of the body in bodies_dev, bytes of the body); n_strips / n_frames strips of equal height (but for
 * the last) tile a frame.  A body may begin at ANY byte; no byte outside [offset, offset + bytes) is read, and a strip
 * writes its own rows * width * channels bytes of its frame and nothing else.  compression 5 is LZW as TIFF 6.0 defines and
 * libtiff decodes it (MSB first, 9 .. 12 bits, the width grows one code early; a stream without a leading Clear starts from
 * the cleared table; decoding ends at EOI or when the strip is full), 32773 PackBits, 1 none.  Then predictor 2 (a running
 * sum mod 256 along a row, per channel), photometric 0 (inverted) and 2 (R, G, B stored, B, G, R delivered).  frames_out: u8
 * [n_frames][height][width][channels], the layout ysmr_threshold_batch reads.  status_dev[i] = 0 or YSMR_TIFFD_* bits; a
 * flagged frame's pixels are undefined, inside its own bytes.  Asynchronous on `stream`.  workspace_dev: 256-byte aligned,
 * workspace_bytes >= ysmr_tiff_decode_workspace_bytes(...); afterwards it holds an int32 per strip, that strip's bits. */
int    ysmr_tiff_decode_batch(void *stream, const uint8_t *bodies_dev, const int32_t *strips_dev, int n_strips, int n_frames,
                              int height, int width, int channels, int compression, int predictor, int photometric,
                              void *workspace_dev, size_t workspace_bytes,
                              uint8_t *frames_out, int32_t *status_dev /* [n_frames] */);

/* ---- annotated output video as Motion-JPEG --------------------------------------------------- */

/* bit of *status_dev of ysmr_mjpeg_batch */
#define YSMR_MJPEG_OVERFLOW 1   /* offsets_dev[n_frames] > out_capacity: the chunks that end inside the capacity are complete */

/* Bytes of scratch ysmr_mjpeg_batch needs for this geometry (about 16 per pixel of the padded frames: the quantised
 * coefficients and a bit buffer with room for the worst case, 26 bits per coefficient).  0 for a geometry it refuses. */
size_t ysmr_mjpeg_workspace_bytes(int n_frames, int height, int width);

/* What cv2.VideoWriter.write does with fourcc 'MJPG', for a batch of frames as ysmr_annotate_batch leaves them.  dib_dev:
 * n_frames stored 24-bit DIB frames, frame_bytes apart (>= stride * height), rows stride bytes apart (a multiple of 4,
 * >= 3 * width), B, G, R per pixel, the last row first if bottom_up.  Every frame becomes one baseline sequential JPEG
 * (SOF0, 8 bits, Y Cb Cr all sampled 1 x 1): SOI, APP0 'AVI1', one DQT with tables 0 and 1 (T.81 Annex K.1 scaled by
 * quality 1 .. 100 as libjpeg does), SOF0, four DHT (the typical tables of Annex K.3), DRI = ceil(width / 8), SOS, data,
 * EOI; one MCU row is one restart interval.  Integer arithmetic only from pixel to byte -- 16-bit fixed-point JFIF colour,
 * the edges repeated up to a multiple of 8, a 16-bit matrix DCT, quantisation rounding half away from zero, AC clamped to
 * +-1023 and DC to [-1024, 1023] -- so the bytes are exactly those of the model in tests/jpeg_model.py, and they do not
 * depend on scheduling.
 * out_dev receives finished AVI chunks back to back: '00dc', the JPEG's size (little-endian u32), the JPEG, one zero byte
 * if that size is odd; chunk i begins at out_dev + offsets_dev[i] (offsets_dev: int64 [n_frames + 1], offsets_dev[0] = 0).
 * offsets_dev is exact whether or not the batch fits: if offsets_dev[n_frames] > out_capacity, *status_dev =
 * YSMR_MJPEG_OVERFLOW, no byte at or beyond out_capacity is written and the chunks that end inside it are complete (call
 * again with a buffer of offsets_dev[n_frames] bytes); otherwise *status_dev = 0.  height, width <= 65535.
 * workspace_dev: 256-byte aligned, workspace_bytes >= ysmr_mjpeg_workspace_bytes(...); no state is kept in it. */
int ysmr_mjpeg_batch(void *stream, const uint8_t *dib_dev, int n_frames, int height, int width,
                     int stride, size_t frame_bytes, int bottom_up, int quality,
                     void *workspace_dev, size_t workspace_bytes,
                     uint8_t *out_dev, size_t out_capacity, int64_t *offsets_dev, int32_t *status_dev);

/* ADDED under ABI 15 (see above).  ysmr_mjpeg_batch with two choices; ysmr_mjpeg_batch is this call with sampling = 1 and
 * huffman = 0, and ysmr_mjpeg_workspace_bytes the workspace of that mode.  Arguments, chunks, offsets_dev, status_dev and the
 * capacity contract are those of ysmr_mjpeg_batch; anything else than the values named here is YSMR_ERR_ARG.
 * sampling (the codes of ysmr_mjpeg_decode_batch): 1 = 4:4:4, 2 = 4:2:2 (luminance sampled 2 x 1), 3 = 4:2:0 (2 x 2).  The MCU
 * is 8 h x 8 v pixels, the frame's edges repeated up to a multiple of it; its blocks are the h v luminance blocks row by row,
 * then Cb, then Cr (T.81 A.2.3); SOF0 says 0x11 / 0x21 / 0x22 for Y and 0x11 for Cb and Cr; one MCU row is one restart
 * interval, DRI = ceil(width / 8 h).  Cb and Cr are downsampled as libjpeg does, on the clamped 0 .. 255 samples of the
 * padded frame: 2 x 1 by (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... along the output row, 2 x 2 by
 * (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ...  4:2:0 has half the blocks of 4:4:4, and about half its workspace.
 * huffman: 0 = the typical tables of Annex K.3; 1 = four tables built for every frame from that frame's own symbol counts
 * (ZRL and EOB included): code lengths by the rule of ysmr_png_code_lengths with a limit of 16 bits over the alphabet
 * {pseudo-symbol with the count 1, symbol 0, symbol 1, ...} -- the pseudo-symbol of T.81 K.2 comes first, so it is the lightest
 * of all and has a longest code; leaving it out leaves the code of all 1-bits unused --, canonical codes by length, then by
 * symbol; each DHT segment lists only the symbols the frame uses, so the header's length varies from frame to frame.  The
 * coefficients are those of huffman = 0: only the bits differ.  The counts are integer sums: two calls give the same bytes.
 * At most 65535 frames per call.  tests/jpeg_sampled_model.py is the specification of every byte. */
size_t ysmr_mjpeg_encode_workspace_bytes(int n_frames, int height, int width, int sampling, int huffman);
int ysmr_mjpeg_encode_batch(void *stream, const uint8_t *dib_dev, int n_frames, int height, int width,
                            int stride, size_t frame_bytes, int bottom_up, int quality, int sampling, int huffman,
                            void *workspace_dev, size_t workspace_bytes,
                            uint8_t *out_dev, size_t out_capacity, int64_t *offsets_dev, int32_t *status_dev);

/* ---- detection: a1-a6 ------------------------------------------------------------------- */

/* Bytes of scratch ysmr_detect_batch needs for this geometry. */
size_t ysmr_detect_workspace_bytes(int batch, int height, int width, int max_det);

/* Call once after allocating a workspace, again if the output buffers used with it were written by anyone else,
 * and after a detection call that returned an error.  The workspace keeps a record of where the previous
 * ysmr_components_batch / ysmr_detect_batch call may have written the label map and the mask (a word per 32-pixel
 * row segment, left by the labelling kernel); when the next call gets the same labels_dev / mask_dev, batch,
 * geometry and max_det it zeroes the two maps there -- and only where that call does not write them again -- instead
 * of the whole maps.  A workspace whose first 256 bytes are zero (this call) makes the next call clear everything. */
int ysmr_detect_workspace_init(void *stream, void *workspace_dev, size_t workspace_bytes);

/* a1-a3 fused.  frames_dev: u8 [batch][height][width][channels], channels 1 (gray) or 3 (BGR).
 * cls_dev: u8 [batch][height][width] (allocation rounded up to a multiple of 16 bytes):
 *   bit0 = `thresh`  (1st adaptiveThreshold call), bit1 = `markers` (2nd call).
 * inv = 0: THRESH_BINARY (bit set iff s - mean > t); inv = 1: THRESH_BINARY_INV (s - mean <= t).
 * use_high = 0 reproduces "adaptive double threshold = 0": bit1 mirrors bit0. */
int ysmr_threshold_batch(void *stream, const uint8_t *frames_dev, int batch, int height, int width,
                         int channels, int inv, int t_low, int t_high, int use_high,
                         uint8_t *cls_dev, int cv_flavour);

/* Fault injection for the library's own test of YSMR_DET_STALLED, through the workspace the caller owns (there is no
 * process-wide switch): a workspace whose header word at byte offset YSMR_WS_FAULT_OFFSET holds
 * YSMR_WS_FAULT_RESIDUE_STALL makes the NEXT ysmr_components_batch / ysmr_detect_batch call on THAT workspace behave as if
 * one workgroup of its barrier kernel never became resident -- the barrier times out (quickly), every frame's status gets
 * YSMR_DET_STALLED and the call returns; the call clears the word.  ysmr_detect_workspace_init clears it too. */
#define YSMR_WS_FAULT_OFFSET        32
#define YSMR_WS_FAULT_RESIDUE_STALL 0xFA17057Au

/* Measurement aid: the NEXT ysmr_threshold_batch / _variant call of this host thread hands the two HIP events (hipEvent_t
 * created with timing enabled; either may be NULL) to its kernel dispatch (hipExtLaunchKernel), which sets them to the
 * kernel's own start and end on the device -- hipEventElapsedTime between them is the duration a kernel trace reports.
 * Events recorded on the stream before and after the call also count the dispatch gaps on both sides (~10 us of a
 * 100 us kernel).  Not used by the mean-gray call. */
int ysmr_threshold_timing(void *start_event, void *stop_event);
/* How many workgroups the matrix-pipe threshold kernel cuts a batch's rows for under these hints (256: one per compute
 * unit; 248 beside the one-launch batch link; 160 beside the two-launch link) -- what a caller needs to size its batches:
 * with as many frames per batch as workgroups (of one panel each: frames up to 1232 columns wide) every workgroup takes ONE
 * whole frame and starts one item, where 256 frames on 248 workgroups start two (the kernel is 5 % faster per frame that way:
 * 0.344 instead of 0.327 of the roofline, profiles/r05_batch_248.log).  ABI 14.  No reference counterpart (the reference
 * thresholds frame by frame, track_eval.py:180-208). */
int ysmr_threshold_workgroups(int cv_flavour);

/* The same call with the kernel named (test and measurement aid; the results are the same bytes whichever is taken).
 * Gray frames of at least 18 rows and 64 columns (width a multiple of 4) are served by a kernel that evaluates the
 * Gaussian mean on the matrix pipe to within 1/512, decides every pixel that is farther than that from both levels
 * and re-evaluates the rest with cv2's float32 arithmetic (csrc/thr_mfma.hip); everything else, and BGR input, by the
 * kernels that run that arithmetic for every pixel (csrc/detect.hip: k_threshold_strip, k_threshold).
 * variant 0: as ysmr_threshold_batch; 1: the float32-chain kernels only; 2: the matrix-pipe kernel deciding every
 * pixel farther than 1/2048 from the levels (a quarter of the shipped margin: any wrong byte says that the margin is
 * being used up; diagnostic); 3: the matrix-pipe kernel with every pixel sent through its exact path (diagnostic).  2 and 3 fail for geometries that kernel does
 * not serve. */
int ysmr_threshold_batch_variant(void *stream, const uint8_t *frames_dev, int batch, int height, int width,
                                 int channels, int inv, int t_low, int t_high, int use_high,
                                 uint8_t *cls_dev, int cv_flavour, int variant);

/* The mean-gray threshold branch, taken by the reference when 'adaptive double threshold' < 0
 * (ysmr/track_eval.py:219-253): replaces cv2.meanStdDev(gray), the 5 s moving average of
 * mean +- stddev +- offset kept in `threshold_list`, and cv2.threshold(blurred, int(average)).
 *   inv      0: white bacteria on dark background (THRESH_BINARY,  level = mean + stddev + offset)
 *            1: dark on bright              (THRESH_BINARY_INV, level = mean - stddev - offset)
 *   offset   settings['threshold offset for detection'] as it stands at track_eval.py:222-229,
 *            i.e. already negated for inv = 1 (track_eval.py:132)
 *   window   longest list the average is taken over = floor(5 * fps) + 1 (the list is trimmed
 *            AFTER the average, when it is longer than 5 * fps: track_eval.py:239-242)
 *   state_dev  ysmr_mean_threshold_state_bytes(window) bytes, 8-byte aligned; all zero = empty
 *            list (start of a video); carries the list from one call to the next
 *   stats_dev  f64 [batch][4] out: mean, stddev, this frame's level, averaged integer level
 *   levels_dev i32 [batch] out: the level each frame was compared with (clamped to [-1, 256])
 *   cls_dev    u8 [batch][H][W] out: 3 where the blurred pixel is foreground, else 0 -- the class
 *            map ysmr_components_batch expects (every foreground pixel is its own marker: this
 *            branch has no binary_propagation step) */
size_t ysmr_mean_threshold_state_bytes(int window);
int ysmr_mean_threshold_batch(void *stream, const uint8_t *frames_dev, int batch, int height, int width,
                              int channels, int inv, double offset, int window, void *state_dev,
                              double *stats_dev, int32_t *levels_dev, uint8_t *cls_dev, int cv_flavour);

/* a4-a6 from a class map already in HBM (written by ysmr_threshold_batch or by the caller):
 * hysteresis + labelling + RETR_EXTERNAL ordering + minAreaRect.  Same outputs as
 * ysmr_detect_batch; cls_dev is read and its bit2 is written. */
int ysmr_components_batch(void *stream, int batch, int height, int width, void *workspace_dev,
                          size_t workspace_bytes, uint8_t *cls_dev, uint8_t *mask_dev,
                          int32_t *labels_dev, int32_t *det_count_dev, float *det_dev,
                          int32_t *anchors_dev, int max_det, int32_t *status_dev, int cv_flavour);

/* a1-a6 = ysmr_threshold_batch followed by ysmr_components_batch.  Outputs (all device):
 *   cls_dev     u8  [batch][H][W]  class map as above (bit2 is used internally as a flag)
 *   mask_dev    u8  [batch][H][W]  final mask {0,255} == binary_propagation(markers, mask=thresh)
 *                                  (may be NULL)
 *   labels_dev  i32 [batch][H][W]  0 = background, else 1 + raster index of the first pixel of
 *                                  the 8-connected component of the final mask (required: it is
 *                                  also the union-find array)
 *   det_count_dev i32 [batch]      detections per frame (<= max_det written)
 *   det_dev     f32 [batch][max_det][5]  cx, cy, w, h, angle_deg of cv2.minAreaRect, in
 *                                  cv2.findContours(RETR_EXTERNAL) order (reverse raster order
 *                                  of first pixels; components nested in a hole are skipped)
 *   anchors_dev i32 [batch][max_det]  raster index of each detection's first pixel (may be NULL)
 *   status_dev  i32 [batch]        YSMR_DET_* bits
 */
int ysmr_detect_batch(void *stream, const uint8_t *frames_dev, int batch, int height, int width,
                      int channels, int inv, int t_low, int t_high, int use_high,
                      void *workspace_dev, size_t workspace_bytes, uint8_t *cls_dev,
                      uint8_t *mask_dev, int32_t *labels_dev, int32_t *det_count_dev,
                      float *det_dev, int32_t *anchors_dev, int max_det, int32_t *status_dev,
                      int cv_flavour);

/* ---- luminosity: the third tracking coordinate ------------------------------------------------------ */

/* What the reference's frame loop does per contour when 'include luminosity in tracking calculation' is set
 * (ysmr/track_eval.py:290-300): box = np.intp(cv2.boxPoints(rect)), cv2.fillPoly(mask, [box], 255) on an empty mask,
 * cv2.mean(gray, mask)[0] / 100 -- the mean gray value under the detection's min-area rectangle, as the third coordinate
 * the tracker links with.  One launch for a batch; the mask is never stored (csrc/luminosity.hip).
 *   frames_dev    u8 [batch][height][width][channels], the frames the threshold call read (4-byte aligned; at most 2^24
 *                 pixels per frame).  channels 3: the gray value is the fixed-point BGR2GRAY of the threshold kernels,
 *                 YSMR_CV_GRAY_3X in cv_flavour honoured; the other cv_flavour bits are ignored
 *   det_dev, det_count_dev   as ysmr_components_batch / ysmr_detect_batch leave them: the five values are used as they
 *                 stand (the angle convention of cv_flavour is already in them)
 *   lum_dev       f64 [batch][max_det]  mean / 100; 0.0 for a box that covers no pixel of the frame.  Entries past
 *                 det_count[b] are left UNTOUCHED (as are those of the three arrays below)
 *   sum_dev, count_dev   u32 [batch][max_det], each may be NULL: the integers the value was made from -- the sum of the gray
 *                 values under the filled box and the number of its pixels inside the frame
 *   corners_dev   i32 [batch][max_det][4][2] (x, y), may be NULL, 16-byte aligned: np.intp(boxPoints(rect)); a coordinate
 *                 beyond +-2^20 is moved there
 * The fill is OpenCV's (upstream recollection, parity-unpinned like the rest of the image half): the four
 * edges as 8-connected lines drawn left to right plus the edge table's scanline spans in 16.16 fixed point, clipped to the
 * frame.  A rectangle of size (0, 0) fills its own pixel. */
int ysmr_luminosity_batch(void *stream, const uint8_t *frames_dev, int batch, int height, int width, int channels,
                          const float *det_dev, const int32_t *det_count_dev, int max_det, int cv_flavour, double *lum_dev,
                          uint32_t *sum_dev, uint32_t *count_dev, int32_t *corners_dev);
/* HOST function: the same arithmetic -- the code that decides a pixel is shared with the kernel -- on host arrays, a
 * detection at a time.  What the CPU tests compare with the NumPy model where no GPU is present; cos / sin are the host's
 * there and the device's in the kernel (both rounded to float32 before use, as cv2.boxPoints does). */
int ysmr_luminosity_batch_host(const uint8_t *frames_host, int batch, int height, int width, int channels,
                               const float *det_host, const int32_t *det_count_host, int max_det, int cv_flavour,
                               double *lum_host, uint32_t *sum_host, uint32_t *count_host, int32_t *corners_host);

/* ---- linking: a7-a19 -------------------------------------------------------------------- */

/* Horizon sizes n_i (gsff.py:87-109) and rows 0/1 of each least-squares gain (gsff.py:111-153,
 * closed form of the default constant-velocity model).  n_max <= 0 means "None -> fps".
 * n_i_out: n_f ints.  gains_out (may be NULL): for filter i, 2 rows x 2*n_i[i] doubles, filters
 * concatenated.  Returns YSMR_ERR_ARG for horizons that are not strictly increasing and >= 1. */
int ysmr_gsff_gains(double fps, int n_min, double n_max, int n_f, int32_t *n_i_out,
                    double *gains_out);

/* CentroidTracker(max_disappeared, fps, n_min, n_max, n_f, use_gsff).  capacity = maximum number
 * of simultaneously live tracks, max_det = maximum detections per frame.  gains_host may be NULL
 * (closed form) or point to host memory laid out as ysmr_gsff_gains() writes it. */
int ysmr_tracker_create(double max_disappeared, double fps, int n_min, double n_max, int n_f,
                        int use_gsff, int capacity, int max_det, const double *gains_host,
                        ysmr_tracker **out);
int ysmr_tracker_destroy(ysmr_tracker *t);
int ysmr_tracker_reset(ysmr_tracker *t, void *stream);

/* A handle links (x, y) centroids (2, the default) or (x, y, third) centroids (3: the reference's
 * input_centroids of width 3, tracker.py:111 -- the third coordinate is the luminosity of ysmr_luminosity_batch).  The
 * distance is sqrt(dx*dx + dy*dy + dl*dl) in float64, summed in that order; claims, ageing, ids, registration order and the
 * rows are the 2-D handle's (rows carry x and y).  Set before the handle's first frame:
 *   YSMR_ERR_ARG    dimensions other than 2 or 3; 3 on a handle created with use_gsff = 1 (the reference has no such mode: its
 *                   filter bank is built for (x, y) and CentroidTracker.update raises on the first frame)
 *   YSMR_ERR_STATE  a frame has been linked since the handle was created or last reset
 * ysmr_tracker_reset keeps the dimension.  A 3-D handle is driven by ysmr_tracker_update3 / ysmr_tracker_run3 /
 * ysmr_tracker_peek3 -- ysmr_tracker_update and ysmr_tracker_run return YSMR_ERR_STATE on it, as the three do on a 2-D
 * handle.  It links with one launch per frame (k_frame), or two (k_link + k_track) where a 2-D handle of that capacity and
 * max_det would, and finds every row minimum by the all-pairs search: the grid searches and the one-launch batch link are
 * two-dimensional by construction, so ysmr_tracker_batched is 0 and ysmr_tracker_prepare a no-op for it -- except that
 * ysmr_tracker_link_mode(t, 2) asks for the 3-D batch link (below): ysmr_tracker_batched then answers 1 for a handle that
 * link serves, and its binning is prepared with ysmr_tracker_prepare3 (ysmr_tracker_prepare stays a no-op).  Without a
 * filter bank the position of a track is the last point it claimed, all three coordinates; a lost track keeps it. */
int ysmr_tracker_dimensions(ysmr_tracker *t, int dimensions);

/* One CentroidTracker.update(rects).  det_dev: [m][5] = cx, cy, w, h, angle; f32 as written by
 * ysmr_detect_batch (det_is_f64 = 0) or f64 (det_is_f64 = 1; for callers holding float64
 * centroids, like the reference's input_centroids, tracker.py:111).  m >= 0: detection count known
 * on the host; m < 0: read it from *m_dev (device i32, clamped to max_det).
 * Outputs (device, each may be NULL):
 *   rows_dev      ysmr_row [capacity]  one row per live track after the update, ascending id
 *   n_rows_dev    i32                  number of rows
 *   claim_col_dev i32 [capacity]       for each track row BEFORE the update (ascending id):
 *                                      claimed detection column or -1
 *   n_before_dev  i32                  number of tracks before the update
 *   new_cols_dev  i32 [max_det]        detection columns registered as new tracks, in id order
 *   n_new_dev     i32
 */
int ysmr_tracker_update(ysmr_tracker *t, void *stream, const void *det_dev, int det_is_f64, int m,
                        const int32_t *m_dev, int32_t frame_index, ysmr_row *rows_dev,
                        int32_t *n_rows_dev, int32_t *claim_col_dev, int32_t *n_before_dev,
                        int32_t *new_cols_dev, int32_t *n_new_dev);

/* ysmr_tracker_update for a 3-D handle: third_dev f64 [m], the third coordinate of each detection. */
int ysmr_tracker_update3(ysmr_tracker *t, void *stream, const void *det_dev, int det_is_f64, const double *third_dev, int m,
                         const int32_t *m_dev, int32_t frame_index, ysmr_row *rows_dev, int32_t *n_rows_dev,
                         int32_t *claim_col_dev, int32_t *n_before_dev, int32_t *new_cols_dev, int32_t *n_new_dev);

/* The frame loop of track_bacteria for `batch` consecutive frames whose detections are already
 * on the device: det_dev f32 [batch][max_det][5], det_count_dev i32 [batch] -- the WHOLE array, batch x max_det x 5 floats
 * whatever the counts are: the batch link reads the box of a frame's slot 0 for lanes that claim nothing, also where the
 * frame's count is 0, and uses nothing of it.  Rows are appended
 * to rows_dev (capacity rows_capacity) starting at *row_count_dev, which is advanced; rows of a
 * frame are contiguous and in ascending id order.  Overflow sets *row_count_dev past capacity
 * (rows beyond capacity are dropped); the host checks after synchronising. */
/* 1 when the handle links with one launch per frame (k_frame), else 0 */
int ysmr_tracker_fused(ysmr_tracker *t);

/* How ysmr_tracker_run links a batch.  A handle whose configuration allows it -- tracking.ini's defaults do: up to three
 * filters with horizons of at most 31 frames, capacity <= 768 (a track per lane of one 768-thread workgroup), max_det <= 2456
 * -- links a whole batch with ONE launch
 * (one workgroup, a track per lane, the filter state in registers from the first frame to the last, the measurement
 * history in a ring in HBM); every other handle,
 * and ysmr_tracker_update, run one launch (or two, for large tables) per frame.  The two paths emit the same frames, ids,
 * counters, boxes and row order; the filtered positions agree within the parity tolerance (1e-9 px on well-conditioned rows),
 * not bit for bit: the batch launch keeps running window sums and one reciprocal for the three weights where the per-frame
 * kernels evaluate the FIR and three divisions.
 *   ysmr_tracker_batched    1 when ysmr_tracker_run takes the one-launch-per-batch path, else 0
 *   ysmr_tracker_link_mode  mode 0: the library's choice (default); 1: one launch per frame even where a batch launch
 *                           would serve (measurement and tests).  Takes effect with the next call; the track table is
 *                           carried over.
 *                           2: as 0, and a 3-D handle whose configuration allows it -- linked with one launch per frame,
 *                           capacity <= 768, max_det small enough for the kernel's LDS (2048 is) -- also links a batch of
 *                           ysmr_tracker_run3 with ONE launch (k_batch3: the same workgroup without a filter bank, the third
 *                           coordinate in the distances and in the stored point).  ysmr_tracker_batched then answers 1 for
 *                           it; every other 3-D handle keeps the per-frame link, and on a 2-D handle mode 2 is mode 0.  The
 *                           memory the 3-D batch link needs is allocated by the first such call.  Both paths of a 3-D
 *                           handle emit the same rows and keep the same points, bit for bit (no filter is involved). */
int ysmr_tracker_batched(ysmr_tracker *t);
int ysmr_tracker_link_mode(ysmr_tracker *t, int mode);

/* Optional, for a handle that links a batch with one launch (a no-op for every other): that launch reads each frame's
 * detections binned into a uniform grid of cells, which ysmr_tracker_run works out in a launch of its own in front of the
 * link.  A caller that detects batch b+1 on one stream while batch b is linked on another can take that launch off the
 * link's chain: call this on the DETECTION stream behind the call that writes det_dev / det_count_dev (up to 256 frames),
 * then ysmr_tracker_run with the same det_dev, det_count_dev and batch on the link stream once it has waited for the
 * detection stream as it must anyway.  slot (0 or 1) names which of two internal blocks to fill: a block must not be
 * prepared again before the ysmr_tracker_run that uses it has executed (two detectors taking turns use their own number).
 * The binning holds for the bytes det_dev held when it executed and is used by ONE ysmr_tracker_run; rewrite the
 * detections and you call it again. */
int ysmr_tracker_prepare(ysmr_tracker *t, void *stream, const float *det_dev, const int32_t *det_count_dev, int batch,
                         int slot);
/* ... for a 3-D handle (ysmr_tracker_prepare is a no-op on one; this returns YSMR_ERR_STATE on a 2-D handle, like the
 * other 3-D calls): the same contract and the same two slots, with third_dev f64 [batch][max_det] binned beside the
 * centres; good for ONE ysmr_tracker_run3 with the same det_dev, third_dev, det_count_dev and batch.  A no-op unless
 * ysmr_tracker_batched. */
int ysmr_tracker_prepare3(ysmr_tracker *t, void *stream, const float *det_dev, const double *third_dev,
                          const int32_t *det_count_dev, int batch, int slot);

int ysmr_tracker_run(ysmr_tracker *t, void *stream, const float *det_dev,
                     const int32_t *det_count_dev, int batch, int32_t first_frame_index,
                     ysmr_row *rows_dev, int64_t rows_capacity, int64_t *row_count_dev);
/* ... for a 3-D handle: third_dev f64 [batch][max_det], as ysmr_luminosity_batch writes it (slots at or beyond a frame's
 * count are never read).  One launch per frame, or per batch in link mode 2 (above). */
int ysmr_tracker_run3(ysmr_tracker *t, void *stream, const float *det_dev, const double *third_dev,
                      const int32_t *det_count_dev, int batch, int32_t first_frame_index, ysmr_row *rows_dev,
                      int64_t rows_capacity, int64_t *row_count_dev);

/* Current track table in id order: ids i32 [capacity], positions f64 [capacity][2] (the
 * CentroidTracker.objects values: GSFF predictions, or raw centroids without GSFF), disappeared
 * counters, count.  Device outputs, each may be NULL. */
int ysmr_tracker_peek(ysmr_tracker *t, void *stream, int32_t *ids_dev, double *xy_dev,
                      int32_t *disappeared_dev, int32_t *n_dev);
/* ... of a 3-D handle, with third_dev f64 [capacity]: each track's third coordinate, in the same order. */
int ysmr_tracker_peek3(ysmr_tracker *t, void *stream, int32_t *ids_dev, double *xy_dev, double *third_dev,
                       int32_t *disappeared_dev, int32_t *n_dev);

/* Host-visible counters (synchronises the stream): live tracks, next id, sticky error bits. */
int ysmr_tracker_info(ysmr_tracker *t, void *stream, int32_t *n_tracks, int32_t *next_id,
                      int32_t *error_bits);

/* ---- output: a19, f2 --------------------------------------------------------------------- */

/* Order rows by (TRACK_ID, POSITION_T): what sort_list does to the csv after tracking
 * (helper_file.py:1538-1574, called at track_eval.py:393).  rows_dev and sorted_dev are distinct
 * device arrays of n_rows rows; (track_id, frame) pairs are unique, so the order is total.
 * On return the first uint32 of the workspace reports which ordering ran: 0, the table had the tracker's shape (ids
 * below n_rows, every track with one row in every frame from its first to its last) and each row was put at
 * offset[id] + frame - first_frame[id] without a sort, sorted_dev is complete; 1, any other table, ordered by the stable
 * radix sort of (track_id << 32 | frame) (equal pairs keep their input order), which may still be running on `stream`. */
size_t ysmr_rows_sort_workspace_bytes(long long n_rows);
int    ysmr_rows_sort(void *stream, const ysmr_row *rows_dev, long long n_rows, void *workspace_dev,
                      size_t workspace_bytes, ysmr_row *sorted_dev);

/* HOST function (no GPU involved): the csv text of `rows_host` exactly as the reference's final
 * file has it -- header of save_list (helper_file.py:1451), one line per row, numbers printed the
 * way DataFrame.to_csv prints uint32 / float64 columns (shortest repr; WIDTH, HEIGHT and
 * DEGREES_ANGLE are the float32 values widened to float64, 0.0 for disappeared tracks;
 * helper_file.py:1366-1400, 881-889).  out_capacity >= ysmr_rows_csv_bound(n_rows, with_header);
 * threads <= 0: one per hardware thread. */
size_t ysmr_rows_csv_bound(long long n_rows, int with_header);
int    ysmr_rows_format_csv(const ysmr_row *rows_host, long long n_rows, int with_header, int via_pandas,
                            int threads, char *out, size_t out_capacity, size_t *out_length);

/* HOST function: the same text written to `path` (created or truncated), every formatting thread writing its own
 * piece at its place in the file; *out_length (may be NULL) receives the number of bytes. */
int    ysmr_rows_write_csv(const ysmr_row *rows_host, long long n_rows, int with_header, int via_pandas,
                           int threads, const char *path, size_t *out_length);
/* ... and, in the same pass, the seven DataFrame columns of ysmr_rows_columns below (ABI 11): the values the text is
 * printed from are the values pandas would read back from it, worked out once for both consumers. */
int    ysmr_rows_write_csv_columns(const ysmr_row *rows_host, long long n_rows, int with_header, int via_pandas,
                                   int threads, const char *path, size_t *out_length, uint32_t *track_id, uint32_t *t,
                                   double *x, double *y, double *w, double *h, double *angle);

/* DEVICE function (ABI 15): the same csv text and the same seven columns worked out ON THE DEVICE from rows that are already there
 * in order (ysmr_rows_sort's output) -- a thread prints a row (shortest round-trip digits by Burger & Dybvig's free-format
 * algorithm in 128-bit fixed point, CPython's layout, pandas' float converter, csrc/fmt.h), a scan places the rows, a second
 * launch packs them behind the header.  Asynchronous on `stream`.  csv_capacity >= ysmr_rows_csv_bound(n_rows, with_header);
 * *csv_length_dev receives the number of bytes; *unserved_dev counts the rows that hold a value the device form does not print
 * (NaN, infinities, |v| outside 2^-20 .. 2^24 other than zero: not something a track produces) -- if it is not 0 the text and
 * columns are incomplete and the caller takes ysmr_rows_write_csv_columns for the table.  Byte for byte and bit for bit what
 * that host function gives otherwise (track_eval.py:393, helper_file.py:1403-1478, 860-905, 1366-1400). */
size_t ysmr_rows_format_device_workspace_bytes(long long n_rows);
int    ysmr_rows_format_device(void *stream, const ysmr_row *rows_dev, long long n_rows, int with_header, int via_pandas,
                               void *workspace_dev, size_t workspace_bytes, char *csv_dev, size_t csv_capacity,
                               unsigned long long *csv_length_dev, uint32_t *track_id_dev, uint32_t *t_dev, double *x_dev,
                               double *y_dev, double *w_dev, double *h_dev, double *angle_dev, uint32_t *unserved_dev);
/* HOST function: the device form's arithmetic (csrc/fmt.h) run on the host a row at a time -- what the CPU tests compare with
 * ysmr_rows_format_csv (std::to_chars) on millions of values.  columns5: five arrays of n_rows doubles, one behind the other
 * (may be NULL); *unserved as above (such rows are left out of the text). */
int    ysmr_rows_format_csv_devicelike(const ysmr_row *rows_host, long long n_rows, int with_header, int via_pandas, char *out,
                                       size_t out_capacity, size_t *out_length, double *columns5, long long *unserved);

/* DEVICE functions (added under ABI 15): the reading direction -- the text of a `*_list.csv` / `*_selected_data.csv` that is in
 * device memory -> the seven columns helper_file.get_data returns (pandas.read_csv with upstream's dtype and usecols,
 * helper_file.py:860-905), bit for bit.  csrc/csv_parse.h states what is served: a header line (read by the HOST, which passes
 * the number of columns and the position of each of TRACK_ID, POSITION_T, POSITION_X, POSITION_Y, WIDTH, HEIGHT, DEGREES_ANGLE
 * in it), then lines of exactly that many fields; integers of 1 .. 10 digits up to 2^32 - 1; floats
 * -?digits(.digits)?([eE][+-]?digits)? read as pandas' precise_xstrtod reads them, with a final decimal exponent in
 * -325 .. 308.  Nothing else is guessed at: it is flagged or counted, and the caller reads the file with pandas.
 *
 * ysmr_csv_index: one pass with 16-byte loads (newline bit map, counts by popcount, flags), a prefix sum, one pass that writes
 * the byte offset of every line start into the workspace.  Asynchronous on `stream`.  text_dev: 16-byte aligned, n_bytes in
 * 1 .. 2^31 - 257 (bytes behind n_bytes are never read).  *n_lines_dev: the lines of the file, the header and a last line
 * without '\n' included.  *flags_dev: 1 a '"', 2 a '\r', 4 a NUL or a byte >= 0x80 (get_data's text-mode read of such a file
 * is the host's business), 8 more lines than a served file of n_bytes can hold -- any of them: not served.
 * ysmr_csv_workspace_bytes: 0 for what is refused (0 bytes, more than the 32-bit offsets hold, arithmetic that does not fit).
 *
 * ysmr_csv_parse: a line per lane, the lines of a workgroup staged into LDS with 16-byte loads; a line that reaches beyond the
 * staged span (ysmr_csv_geometry) is PARSED FROM GLOBAL MEMORY, it is not counted unserved.  Same text_dev, n_bytes and
 * workspace as the index call before it; n_rows <= *n_lines_dev - 1 (rows beyond what the index found are counted unserved
 * and not read).  wanted[7]: the seven positions, distinct, below n_columns (7 .. 4096).  *unserved_dev (zeroed by the call):
 * rows that are not served; no value of such a row is written.
 *
 * ysmr_csv_order: sort_list (helper_file.py:1538-1574) -- the rows ordered by (TRACK_ID, POSITION_T), equal pairs in file
 * order as DataFrame.sort_values leaves them: a stable radix sort of key and row number, then a gather of the seven columns
 * into the (distinct) outputs.  Upstream's "rough check" (sort only when rows 0 .. 5 hold pairwise distinct ids) is the
 * caller's, on six downloaded ids.
 *
 * ysmr_csv_geometry: bytes of text per workgroup of the index pass, lines per workgroup of the parse, bytes of a workgroup's
 * lines held in LDS (counted from the 16-byte boundary at or before its first line).
 *
 * ysmr_csv_parse_devicelike: a HOST function, the same arithmetic (csrc/csv_parse.h) a line at a time on text in host memory,
 * header line included (it is skipped); what the CPU tests compare with pandas.  *n_rows: the lines behind the header (more
 * than row_capacity: YSMR_ERR_CAPACITY); *unserved and *flags as above. */
size_t ysmr_csv_workspace_bytes(size_t n_bytes);
int    ysmr_csv_index(void *stream, const char *text_dev, size_t n_bytes, void *workspace_dev, size_t workspace_bytes,
                      uint32_t *n_lines_dev, uint32_t *flags_dev);
int    ysmr_csv_parse(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                      int n_columns, const int32_t *wanted, long long n_rows, uint32_t *track_id_dev, uint32_t *t_dev,
                      double *x_dev, double *y_dev, double *w_dev, double *h_dev, double *angle_dev, uint32_t *unserved_dev);
size_t ysmr_csv_order_workspace_bytes(long long n_rows);
int    ysmr_csv_order(void *stream, long long n_rows, const uint32_t *track_id_dev, const uint32_t *t_dev, const double *x_dev,
                      const double *y_dev, const double *w_dev, const double *h_dev, const double *angle_dev,
                      void *workspace_dev, size_t workspace_bytes, uint32_t *track_id_out, uint32_t *t_out, double *x_out,
                      double *y_out, double *w_out, double *h_out, double *angle_out);
void   ysmr_csv_geometry(int *index_chunk_bytes, int *rows_per_group, int *staged_span_bytes);
int    ysmr_csv_parse_devicelike(const char *text_host, size_t n_bytes, int n_columns, const int32_t *wanted,
                                 long long row_capacity, uint32_t *track_id, uint32_t *t, double *x, double *y, double *w,
                                 double *h, double *angle, long long *n_rows, long long *unserved, uint32_t *flags);

/* DEVICE functions (added under ABI 15): the writing direction for ANY table of typed columns -- what
 * DataFrame.to_csv(index=False) writes with '\n' line ends (helper_file.py:1366-1400, save_df_to_csv: `<name>_selected_data.csv`,
 * `<name>_analysed.csv`), byte for byte, from columns that are in device memory.  The header's bytes are written as given; each
 * row is a line of n_columns (1 .. 16) fields separated by ',' and ended by '\n'.  Integers are plain decimals; a float64 is its
 * repr (shortest round-trip digits, CPython's layout) for EVERY finite value, 0.0 / -0.0, inf / -inf, and NaN is the empty field.
 * (A NaN that is its line's only field is written "", as the csv module quotes a line that would be empty.)
 * The widest fields are 10 / 20 / 11 / 4 / 24 bytes for the five types.
 *
 * ysmr_table_csv_bound: header_bytes + n_rows x the sum of (width + 1).  0 for what is refused: a negative count, no or more than
 * 16 columns, an unknown type, arithmetic beyond size_t, a bound above 2^32 - 1 (the scans are 32-bit).  Nothing is truncated.
 * ysmr_table_format_workspace_bytes: 0 for the same; 256 for n_rows = 0.
 *
 * ysmr_table_format_device: asynchronous on `stream`, no host synchronisation inside.  columns: a HOST array whose data pointers
 * are DEVICE pointers to n_rows values each; header_host: host memory (may be NULL with header_bytes = 0).  csv_capacity >=
 * the bound, else YSMR_ERR_CAPACITY and nothing is launched; *csv_length_dev receives the bytes written, *wide_cells_dev the
 * number of float64 cells outside 0 and 2^-20 <= |v| < 2^24 (finite): those are printed by a kernel of their own (k_table_wide,
 * multi-word integers) into side slots and copied by the row printer, whose steady path prints everything else once, a row per
 * lane, staged in LDS and sent out compacted.  The text depends on the input alone (no ordering comes from atomics).
 *
 * ysmr_table_format_geometry: rows per workgroup of the row printer, and the largest staging in LDS (sixteen float64 columns;
 * a table's own is rows_per_group x its longest line rounded up to 4).
 *
 * ysmr_table_format_devicelike: a HOST function, the same arithmetic (csrc/fmt.h) a row at a time on columns in host memory;
 * what the CPU tests compare with pandas.  ysmr_fmt_f64_text: a HOST function, n float64 fields into 24-byte slots (zero filled
 * behind the text) with their lengths; printer 0: the fast printer (length 255 for a value it declines), 1: the wide printer
 * for every finite non-zero value, 2: the writer's choice between the two. */
#define YSMR_COL_U32 0
#define YSMR_COL_I64 1
#define YSMR_COL_I32 2
#define YSMR_COL_I8  3
#define YSMR_COL_F64 4
typedef struct { const void *data; int32_t type; int32_t reserved; } ysmr_table_column;
size_t ysmr_table_csv_bound(long long n_rows, int n_columns, const ysmr_table_column *columns, size_t header_bytes);
size_t ysmr_table_format_workspace_bytes(long long n_rows, int n_columns, const ysmr_table_column *columns);
int    ysmr_table_format_device(void *stream, long long n_rows, int n_columns, const ysmr_table_column *columns,
                                const char *header_host, size_t header_bytes, void *workspace_dev, size_t workspace_bytes,
                                char *csv_dev, size_t csv_capacity, unsigned long long *csv_length_dev, uint32_t *wide_cells_dev);
void   ysmr_table_format_geometry(int *rows_per_group, int *staged_bytes);
int    ysmr_table_format_devicelike(long long n_rows, int n_columns, const ysmr_table_column *columns, const char *header,
                                    size_t header_bytes, char *out, size_t out_capacity, size_t *out_length, long long *wide_cells);
int    ysmr_fmt_f64_text(const double *values, long long n, int printer, char *slots, uint8_t *lengths);

/* DEVICE functions (added under ABI 15): the reading direction for 1 .. 16 TYPED columns -- what
 * pandas.read_csv(usecols, dtype) gives for the columns of an `*_analysed.csv` that annotate_video reads (track_eval.py:1321-1472),
 * bit for bit.  ysmr_csv_parse_typed runs behind the same ysmr_csv_index call as ysmr_csv_parse, with the same text, workspace,
 * staged span and line-per-lane layout (a line beyond the staged span is parsed from global memory); ysmr_csv_parse and its
 * arguments are as they were.  fields: a HOST array of n_fields (1 .. 16) entries; data: DEVICE pointers to n_rows values of the
 * type, aligned to it (HOST pointers for the _devicelike twin); type: one of YSMR_COL_*; column: the position of the column in the
 * header, all distinct and below n_columns (1 .. 4096); flags: 0, or YSMR_CSV_EMPTY_IS_NAN on a YSMR_COL_F64 field.
 * Served (csrc/csv_parse.h): lines of exactly n_columns fields, fields that are not wanted skipped whatever they hold;
 *   U32  1 .. 10 digits, value <= 2^32 - 1;     I64  -?digits, 1 .. 18 digits;
 *   I32, I8  -?digits (at most 18 behind leading zeros), the value inside the type;
 *   F64  as ysmr_csv_parse reads it; with YSMR_CSV_EMPTY_IS_NAN an empty field is served too and is the quiet NaN pandas gives
 *        (0x7FF8000000000000).
 * Anything else -- nan, NA, inf, "+1", "1.", a blank, an empty integer field, a value out of range, too few or too many fields --
 * makes the row unserved: it is counted in *unserved_dev (zeroed by the call), no value of it is written, and the caller reads
 * the file with pandas.  No byte at or behind n_bytes is read; nothing is written outside n_rows values per field.
 * ysmr_csv_parse_typed_devicelike: a HOST function, the same text (csrc/csv_parse.h) a line at a time, header line skipped. */
#define YSMR_CSV_EMPTY_IS_NAN 1
typedef struct { void *data; int32_t type; int32_t column; int32_t flags; int32_t reserved; } ysmr_csv_field;
int    ysmr_csv_parse_typed(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                            int n_columns, int n_fields, const ysmr_csv_field *fields, long long n_rows, uint32_t *unserved_dev);
int    ysmr_csv_parse_typed_devicelike(const char *text_host, size_t n_bytes, int n_columns, int n_fields, const ysmr_csv_field *fields,
                                       long long row_capacity, long long *n_rows, long long *unserved, uint32_t *flags);

/* DEVICE functions (added under ABI 15): the collated workbook (helper_file.py:92-137 upstream, collate_results_csv_to_xlsx: a
 * sheet per `*statistics.csv`, DataFrame.to_excel) -- the kinds of a csv file's columns and a sheet's rows as SpreadsheetML.
 *
 * ysmr_csv_column_kinds runs behind the same ysmr_csv_index call as the two parsers, with the same text, workspace, staged span
 * and line-per-lane layout.  kinds_dev: 17 words, zeroed by the call.  Word c < n_columns (1 .. 16) ORs over the n_rows lines
 * behind the header YSMR_KIND_NOT_INT (a field that is not -?[0-9]{1,18}), YSMR_KIND_NOT_NUMBER (a field that is neither empty
 * nor a float64 field ysmr_csv_parse_typed serves; a run of more than 18 digits with no '.' or exponent sets it too) and
 * YSMR_KIND_EMPTY; word 16 holds YSMR_KIND_BAD_LINE for an empty line or one whose field count is not n_columns.  A ballot per
 * bit, then one atomic OR per wave and column: two runs give the same words.  No bit: pandas.read_csv makes the column int64
 * (YSMR_COL_I64); only NOT_INT / EMPTY: float64 with NaN for the empty fields (YSMR_COL_F64, YSMR_CSV_EMPTY_IS_NAN); anything
 * else is not guessed at: the caller reads the file with pandas.  ysmr_csv_column_kinds_devicelike: a HOST function, the same
 * text (csrc/csv_parse.h) a line at a time; *n_rows: the lines behind the header, *flags: as the index pass sets them.
 *
 * ysmr_xlsx_sheet_device: the n_rows rows of 1 .. 16 typed columns (DEVICE pointers in a HOST array, as for
 * ysmr_table_format_device) as <row r="N">, a cell per value and </row> (csrc/xlsx_row.h), between prefix_host and suffix_host,
 * which are written as given (the XML head, <sheetData> and the header row; the closing tags).  Table row 0 is sheet row
 * first_row; with_index: column A holds the table's row number in cell style 1 and the columns follow from B, else they start at
 * A.  Every cell carries its reference (letters A .. Q, rows of 1 .. 7 digits); integers are plain decimals, a float64 the text
 * ysmr_table_format_device prints for it, for every finite value; a NaN cell is not written at all (a row of only NaN is its
 * <row>, its index cell, </row>); an infinity is the string cell <c r="B7" t="str"><v>inf</v></c>.  Asynchronous on `stream`, no
 * host synchronisation inside; *xml_length_dev receives the bytes written, *wide_cells_dev the float64 cells printed by the
 * wide printer; nothing is written at or behind xml_dev + the length.  A row per lane printed once into LDS, the workgroup's
 * text compacted there and sent out in 16-byte stores, a prefix sum over the pieces, a packing launch: the text depends on the
 * input alone.  Refused (YSMR_ERR_ARG, nothing launched): a column count outside 1 .. 16, an unknown type, first_row < 1 or
 * first_row + n_rows - 1 > 1048576; (YSMR_ERR_CAPACITY, nothing launched) a bound above 2^32 - 1, xml_capacity below the bound,
 * workspace_bytes below ysmr_xlsx_sheet_workspace_bytes.  Nothing is truncated.
 * ysmr_xlsx_sheet_bound: prefix_bytes + n_rows x the longest row + suffix_bytes, the longest row being that of the declared types'
 * widest values under the digits of the table's last sheet row and last row number; 0 for what is refused.
 * ysmr_xlsx_sheet_workspace_bytes: 0 for the same (the suffix waits in the workspace: never 0 for what is served).
 * ysmr_xlsx_sheet_geometry: rows per workgroup of the row printer, its largest staging in LDS, and the longest row there is
 * (sixteen float64 columns behind the index).  ysmr_xlsx_sheet_devicelike: a HOST function, the same text a row at a time on
 * columns in host memory. */
#define YSMR_KIND_NOT_INT    1
#define YSMR_KIND_NOT_NUMBER 2
#define YSMR_KIND_EMPTY      4
#define YSMR_KIND_BAD_LINE   1
int    ysmr_csv_column_kinds(void *stream, const char *text_dev, size_t n_bytes, const void *workspace_dev, size_t workspace_bytes,
                             int n_columns, long long n_rows, uint32_t *kinds_dev /* 17 */);
int    ysmr_csv_column_kinds_devicelike(const char *text_host, size_t n_bytes, int n_columns, uint32_t *kinds /* 17 */,
                                        long long *n_rows, uint32_t *flags);
size_t ysmr_xlsx_sheet_bound(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row, int with_index,
                             size_t prefix_bytes, size_t suffix_bytes);
size_t ysmr_xlsx_sheet_workspace_bytes(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row,
                                       int with_index, size_t suffix_bytes);
void   ysmr_xlsx_sheet_geometry(int *rows_per_group, int *staged_bytes, int *max_row_bytes);
int    ysmr_xlsx_sheet_device(void *stream, long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row,
                              int with_index, const char *prefix_host, size_t prefix_bytes, const char *suffix_host,
                              size_t suffix_bytes, void *workspace_dev, size_t workspace_bytes, char *xml_dev, size_t xml_capacity,
                              unsigned long long *xml_length_dev, uint32_t *wide_cells_dev);
int    ysmr_xlsx_sheet_devicelike(long long n_rows, int n_columns, const ysmr_table_column *columns, long long first_row,
                                  int with_index, const char *prefix, size_t prefix_bytes, const char *suffix, size_t suffix_bytes,
                                  char *out, size_t out_capacity, size_t *out_length, long long *wide_cells);

/* DEVICE functions (added under ABI 15): the marks of a whole annotated video from the columns of the evaluated table --
 * annotate.build_marks on the device, the same bytes.  A row is kept if x and y are finite, 0 <= t < n_frames and (with
 * phenotype_dev) phenotype == subtype; its mark is x, y truncated toward zero and clipped to int32, the 32 bits of the id, style 1
 * where moving == 0, else 2 where turn_points == 1, else 0 (csrc/marks_rule.h).  marks_dev [n_rows]: the marks ordered by frame
 * and inside a frame in TABLE order, the entries behind the last mark zeroed; first_dev [n_frames + 1]: first[i] = the marks of
 * the frames below i -- what ysmr_annotate_batch takes.  Table order is get_data's: sort_rule 0 file order, 1 the table sorted by
 * (TRACK_ID, POSITION_T) with equal pairs in file order, 2 the latter exactly when rows 0 .. 5 (all rows of a shorter table) hold
 * pairwise distinct ids -- upstream's rough check, made on the device.  One stable radix sort of the 64-bit key (t << 32 | id)
 * -- (t << 32) for file order -- with the row number as payload, a gather and a binary search per frame: no atomics, two calls
 * give the same bytes; asynchronous on `stream`, no host synchronisation inside.
 * ysmr_marks_workspace_bytes: 0 for what is refused (n_rows outside 0 .. 2^31 - 1, n_frames outside 1 .. 2^31 - 2). */
size_t ysmr_marks_workspace_bytes(long long n_rows, int n_frames);
int    ysmr_marks_build(void *stream, long long n_rows, const uint32_t *track_id_dev, const int64_t *t_dev, const double *x_dev,
                        const double *y_dev, const int8_t *moving_dev, const int8_t *turn_points_dev,
                        const double *phenotype_dev /* NULL: every subtype */, int subtype, int n_frames, int sort_rule,
                        void *workspace_dev, size_t workspace_bytes, ysmr_mark *marks_dev /* n_rows */, int64_t *first_dev /* n_frames + 1 */);

/* HOST functions (ABI 13): the same csv and columns worked out WHILE the video runs.  Rows go in as the link emits them -- any
 * number of ysmr_rows_stream_push calls with host rows in any order; a call copies its rows and returns, the stream's threads
 * format them meanwhile -- and ysmr_rows_stream_finish orders what has been pushed by (TRACK_ID, POSITION_T) (a row's place is
 * offset[id] + frame - first_frame[id] for the tracker's tables, whose ids are never reused and whose tracks have a row in every
 * frame of their life; any other table is sorted), writes the csv to `path` (NULL: no file) and fills the seven columns (all
 * NULL: none): byte for byte what ysmr_rows_sort + ysmr_rows_write_csv_columns give for the same rows (track_eval.py:393,
 * helper_file.py:1538-1574).  One handle per video, used from one thread at a time. */
typedef struct ysmr_rows_stream ysmr_rows_stream;
int    ysmr_rows_stream_create(int threads, int via_pandas, ysmr_rows_stream **out);
int    ysmr_rows_stream_push(ysmr_rows_stream *s, const ysmr_row *rows_host, long long n_rows);
long long ysmr_rows_stream_count(ysmr_rows_stream *s);   /* rows pushed so far (-1: NULL handle) */
int    ysmr_rows_stream_finish(ysmr_rows_stream *s, int with_header, const char *path, size_t *out_length,
                               uint32_t *track_id, uint32_t *t, double *x, double *y, double *w, double *h, double *angle);
int    ysmr_rows_stream_destroy(ysmr_rows_stream *s);

/* HOST function: the seven DataFrame columns (dtypes of helper_file.py:881-889).
 * via_pandas (here and above): the reference does not keep the tracker's float64 values, it prints
 * them and reads the text back with pandas.read_csv (helper_file.py:860-905), whose default float
 * converter returns about one value in five 1 ulp off.  via_pandas = 1 applies that same text ->
 * double conversion (restated from pandas' precise_xstrtod), so that the DataFrame and the csv equal
 * the reference's; via_pandas = 0 keeps the exact values. */
int    ysmr_rows_columns(const ysmr_row *rows_host, long long n_rows, int via_pandas, uint32_t *track_id,
                         uint32_t *t, double *x, double *y, double *w, double *h, double *angle);

/* ---- selection: select_tracks / find_good_tracks (ysmr/track_eval.py:408-843) ------------------ */

/* Settings of the selection, as get_configs() stores them (ysmr/helper_file.py:776-788) and as
 * select_tracks() derives them (track_eval.py:574-583). */
typedef struct ysmr_select_params {
    double  area_lo, area_hi;        /* 'extreme area outliers lower / upper end in px*px' */
    double  area_factor;             /* 'exclude measurement when above x times average area' (0 = off) */
    double  q_area;                  /* 'percent quantiles excluded area' / 100 (<= 0: no area bounds) */
    double  motility_stop_fraction;  /* 'stop excluding motility outliers if total count above percent' / 100 */
    double  max_empty_ratio;         /* 'maximal empty frames in %' / 100 + 1 */
    double  ratio_min, ratio_max;    /* 'average width/height ratio min. / max.' */
    double  edge_fraction;           /* 'percent of screen edges to exclude' / 100 */
    int32_t min_length_frames;       /* int(round(fps) * 'minimal length in seconds') */
    int32_t limit_frames;            /* int(round(fps) * 'limit track length to x seconds'); 0 = off */
    int32_t limit_exact;             /* 'limit track length exactly' */
    int32_t omit_motility;           /* 'try to omit motility outliers' */
    int32_t max_holes;               /* 'maximal consecutive holes' */
    int32_t max_recursion;           /* 'maximal recursion depth' */
    int32_t frame_height, frame_width;
} ysmr_select_params;

#define YSMR_SELECT_OK                0   /* rows_selected rows were written */
#define YSMR_SELECT_TOO_SHORT         1   /* fewer rows than min_length_frames (track_eval.py:612-619) */
#define YSMR_SELECT_TOO_SHORT_CLEANED 2   /* ... after the clean-up (track_eval.py:676-684) */
#define YSMR_SELECT_NONE              3   /* no acceptable track (track_eval.py:817-820) */

/* What the reference logs along the way (track_eval.py:686-691, 707-708, 721-723, 799-815). */
typedef struct ysmr_select_summary {
    int32_t   status;                /* YSMR_SELECT_* */
    int32_t   outliers_used;         /* 0: distance-outlier exclusion off (setting, or too many outliers) */
    long long rows_before, tracks_before, rows_after, tracks_after;
    double    area_lo, area_hi;      /* area quantiles (-1 / inf when q_area <= 0) */
    double    q1_dist, q3_dist, dist_fence;
    long long dist_outliers;
    long long kick_reasons[9];       /* tracks per lowest reached rejection stage; [0] = passed */
    long long good_tracks, rows_selected;
} ysmr_select_summary;

/* The table must be ordered by (TRACK_ID, POSITION_T) -- what ysmr_rows_sort / sort_list produce --
 * and hold the values the reference's DataFrame holds (ysmr_rows_columns with via_pandas = 1).
 * Outputs: sel_row_dev[i] = row of the input table, sel_index_dev[i] = its index in the cleaned table
 * (the 'index' column of the reference's result), i < summary->rows_selected, in table order; both
 * need room for n_rows entries.  Synchronous: returns when the result is complete.
 * summary is host memory.  Parity note: means follow numpy's pairwise summation, the median pandas'
 * median_linear, quantiles numpy's 'linear' method (what pandas 2.x / numpy 2.x execute). */
size_t ysmr_select_workspace_bytes(long long n_rows, int max_recursion);
int    ysmr_select_tracks(void *stream, long long n_rows, const uint32_t *track_id_dev, const uint32_t *t_dev,
                          const double *x_dev, const double *y_dev, const double *w_dev, const double *h_dev,
                          const ysmr_select_params *params, void *workspace_dev, size_t workspace_bytes,
                          int64_t *sel_row_dev, int64_t *sel_index_dev, ysmr_select_summary *summary);

/* ---- per-track statistics of the selected tracks: evaluate_tracks, ysmr/track_eval.py:846-1318 ---- */

typedef struct ysmr_evaluate_params {
    double pixel_per_micrometre;   /* settings['pixel per micrometre'] */
    double fps;
    double min_turn_angle;         /* settings['minimal angle in degrees for turning point'] */
    int32_t angle_lag;             /* settings['compare angle between n frames'] */
    int32_t reach_lag;             /* int(round(fps * min(10, min length / 2, length limit / 2))), track_eval.py:990-1000 */
    int32_t median_kernel;         /* round(fps), made odd: the second medfilt of `moving` (track_eval.py:931-939) */
    int32_t reserved;
} ysmr_evaluate_params;

/* Input: the six columns of the table evaluate_tracks receives (rows ordered by TRACK_ID, POSITION_T; row i has
 * DataFrame index i), device pointers.  Outputs, device, n_rows entries each: WIDTH and HEIGHT in micrometres,
 * angle_diff (int32), moving, turn_points, motility_phenotype (int8), tp_of_tracks (f64, NaN where not moving),
 * travelled_dist -- the columns of <name>_analysed.csv -- and stats_dev f64 [tracks][12], the columns of
 * <name>_statistics.csv in the reference's order (Turn Points (TP/s), Distance, Speed, Time, Displacement, Perc.
 * Motile, Arc-Chord Ratio, Bacteria Length (a float32 value), Displacement divided by length, Motility Phenotype,
 * TRACK_ID, Median Speed); room for n_rows tracks.  *n_tracks_out: the number of tracks.  Synchronous. */
size_t ysmr_evaluate_workspace_bytes(long long n_rows);
int ysmr_evaluate_tracks(void *stream, long long n_rows, const uint32_t *track_id_dev, const uint32_t *t_dev,
                         const double *x_dev, const double *y_dev, const double *w_dev, const double *h_dev,
                         const ysmr_evaluate_params *params, void *workspace_dev, size_t workspace_bytes,
                         double *width_um_dev, double *height_um_dev, int32_t *angle_diff_dev, int8_t *moving_dev,
                         int8_t *turn_points_dev, double *tp_of_tracks_dev, double *travelled_dist_dev,
                         int8_t *motility_phenotype_dev, double *stats_dev, long long *n_tracks_out);

/* HOST function: atan2(y[i], x[i]) as k_ev_heading and the angle histogram take it -- correctly rounded, in double-double
 * (csrc/atan2_cr.h) -- run on the host, for the CPU tests that compare it with the exact model (tests/atan2_exact.py). */
int ysmr_atan2_devicelike(const double *y, const double *x, long long n, double *out);

/* ---- the track figures: large_xy_plot, rose_graph, angle_distribution_plot, ysmr/plot_functions.py:29-257 ---- */

/* These entry points were ADDED under ABI 15 (see above).  Inputs are columns of the (TRACK_ID, POSITION_T)-ordered table
 * in HBM: the rows of a track are one contiguous run of equal ids.  Every output is a caller-made DEVICE buffer; the calls
 * only enqueue work on `stream`.  The image is this project's own rendering; its rules are DESIGN.md, "The figures". */

/* HOST function: matplotlib's viridis_r as 256 x (R, G, B): out[3 k ..] = cm.viridis_r(k, bytes=True)[:3]. */
int ysmr_plot_colormap(uint8_t *out);

/* out_dev[4] = min u, max u, min v, max v over the rows where u and v are both finite (+inf, -inf, +inf, -inf when there is
 * none).  mode 0 (overview): u = x / px, v = y / px.  mode 1 (rose): u = (x - x_first) / px, v = (y - y_first) / px with the
 * first row of the row's track (upstream's x_norm, y_norm).  Exact: min and max do not depend on order. */
int ysmr_plot_extent(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev, const double *y_dev,
                     int mode, double px, double *out_dev);

typedef struct ysmr_plot_view {
    double  px;                  /* pixels per micrometre: u = x / px */
    double  u0, v0;              /* data coordinates of the axes' lower left corner */
    double  units_per_pixel;     /* the same along u and v: equal aspect */
    int32_t mode;                /* 0: overview (with start dots); 1: rose graph (every track from the origin) */
    int32_t width, height;       /* the canvas */
    int32_t ax_x, ax_y, ax_w, ax_h;   /* the axes rectangle (top-left pixel, size), inside the canvas */
    int32_t r2_dot, r2_start;    /* squared radii of a row's dot and of a track's start dot, 0 .. 4096 */
    int32_t n_grid_cols, n_grid_rows;
    int32_t bar_x, bar_y, bar_w, bar_h;   /* the colour bar; bar_w = 0: none */
    int32_t grid_cols[32];       /* canvas columns / rows of the grid lines (drawn inside the axes only) */
    int32_t grid_rows[32];
} ysmr_plot_view;

/* ysmr_plot_tracks paints rgb_dev: u8 [height][width][3] (R, G, B), top-down, no padding.  A row lands on
 * col = ax_x + floor((u - u0) / units_per_pixel), row = ax_y + ax_h - 1 - floor((v - v0) / units_per_pixel) (f64, unfused;
 * rows with a non-finite u or v are skipped) and paints the pixels (col + dx, row + dy), dx^2 + dy^2 <= r2_dot, that lie
 * inside the axes.  dist_dev[t * dist_stride], t < n_tracks: the track's 'Distance (um)' (column 1 of
 * ysmr_evaluate_tracks' statistics, stride 12).  Colour value c_t = (dist_t - dmin) / (dmax - dmin), 0 for every track
 * where that range is 0 or any distance is not finite; colour = viridis_r[min(255, (int)(c_t * 256))].  Where dots meet,
 * the track of the larger rank wins: rank_t = number of tracks u with c_u > c_t, or c_u == c_t and u < t (the shortest
 * path on top).  mode 0 puts a black dot (r2_start) under them at every track's first row.  Background white, grid
 * (176, 176, 176), a one-pixel black frame just outside the axes and the bar; bar row j from the top has LUT index
 * min(255, (bar_h - 1 - j) * 256 / bar_h).  Rows of tracks beyond n_tracks are not drawn.
 * ysmr_plot_workspace_bytes(n_rows, n_tracks, width, height): the scratch of that call;
 * ysmr_plot_workspace_bytes(n_rows, 0, 0, 0): the scratch of ysmr_plot_angle_histogram.  0: sizes out of range. */
size_t ysmr_plot_workspace_bytes(long long n_rows, long long n_tracks, int width, int height);
int ysmr_plot_tracks(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev, const double *y_dev,
                     long long n_tracks, const double *dist_dev, long long dist_stride, const ysmr_plot_view *view,
                     void *workspace_dev, size_t workspace_bytes, uint8_t *rgb_dev);

/* The histogram of angle_distribution_plot.  A track passes iff (rows with moving == 1) / rows > 0.7 (f64 division of the
 * two counts); a row is selected iff its track passes and moving == 1; *n_points_dev = the selected rows.  A selected row
 * i whose row i - lag belongs to the same track has the heading atan2(x_i - x_{i-lag}, y_i - y_{i-lag}) and counts in bin
 * k with edges[k] <= heading < edges[k + 1] (the last bin closed on the right; found by binary search in edges_dev, n_bins
 * + 1 ascending values); other rows land in no bin.  1 <= n_bins <= 1024; counts_dev: n_bins entries. */
int ysmr_plot_angle_histogram(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev,
                              const double *y_dev, const int8_t *moving_dev, int lag, int n_bins, const double *edges_dev,
                              void *workspace_dev, size_t workspace_bytes, long long *counts_dev, long long *n_points_dev);

/* The polar bar chart (north up, clockwise) as a function of the pixel.  dirs_dev: the n_bins + 1 boundary directions as
 * (east, north) pairs, each bar narrower than half a turn (3 <= n_bins <= 1024); the last should repeat the first bit for
 * bit.  p = (col - cx, cy - row) lies in the wedge of the lowest k with d_k x p <= 0 and d_{k+1} x p > 0 (d x p = d_e * p_n -
 * d_n * p_e in f64, unfused) and is filled iff 0 < |p|^2 <= r2_dev[k].  Filled pixels are (143, 187, 218), black where a
 * 4-neighbour is not filled in the same wedge.  Under the bars a grey (176, 176, 176) ring: the pixels with |p|^2 <=
 * ring_r2 that have a 4-neighbour beyond it.  Everything else white.  rgb_dev as above. */
int ysmr_plot_wedges(void *stream, int width, int height, int cx, int cy, int n_bins, const double *dirs_dev,
                     const long long *r2_dev, long long ring_r2, uint8_t *rgb_dev);

/* ---- the violin plots of evaluate_tracks: violin_plot, ysmr/plot_functions.py:260-370, track_eval.py:1151-1303 ---- */

/* ADDED under ABI 15 as well.  A figure shows one value column of the per-track statistics, split by a cut column:
 * violin 0 is 'All', violin k + 1 the half-open interval [lo[k], hi[k]) of the cut column.  A track belongs to violin 0
 * and to at most one other: the LAST k with lo[k] <= c and c < hi[k] in f64 (upstream's loop overwrites); a NaN c
 * belongs to none.  Seaborn's violinplot(cut=0, bw=.2, gridsize=100, scale='count', width=.95) is what is computed. */
#define YSMR_VIOLIN_GRID      100   /* density points per violin */
#define YSMR_VIOLIN_MAX_CUTS  254   /* intervals of one call of the statistics */
#define YSMR_VIOLIN_MAX_SLOTS 64    /* violins of one painted figure */

typedef struct ysmr_violin_summary {
    long long members;           /* tracks in the category */
    long long values;            /* ... whose value is finite: only these count below.  0: every field below is 0 */
    double    vmin, vmax;
    double    q25, q50, q75;     /* NumPy's linear rule: pos = q (n - 1), lo = floor(pos), t = pos - lo, a = x[lo], b = x[lo + 1]:
                                    a + (b - a) t when t < 0.5, else b - (b - a) (1 - t) */
    double    whisker_lo, whisker_hi;   /* the smallest value >= q25 - 1.5 (q75 - q25), the largest <= q75 + 1.5 (q75 - q25) */
    double    mean;              /* sum / n, the sum in a fixed order (lanes striding by 256, then a tree) */
    double    h;                 /* 0.2 * sqrt(sum (x - mean)^2 / (n - 1)); 0 when n < 2 */
} ysmr_violin_summary;

/* The scratch of either call below (0: sizes out of range); ax_h may be 0 for the statistics alone. */
size_t ysmr_violin_workspace_bytes(long long n_tracks, int n_violins, int ax_h);

/* cut_dev[t * cut_stride], value_dev[t * value_stride], t < n_tracks (columns of the [tracks][12] statistics: stride 12);
 * lo_dev, hi_dev: n_cuts doubles.  Writes summaries_dev[n_cuts + 1] and density_dev[n_cuts + 1][YSMR_VIOLIN_GRID]:
 *   d_j = (1 / (n h sqrt(2 pi))) * sum_i exp(-0.5 ((g_j - x_i) / h)^2),  g_j = vmin + j (vmax - vmin) / 99, g_99 = vmax
 * (the difference before the division; one workgroup per (violin, j), the sum in the fixed order of the mean over the
 * SORTED values).  A violin with values < 2 or h == 0 has no density: zeros.  No floating-point atomics: two calls
 * give the same bytes.  0 <= n_tracks <= 2^30, 0 <= n_cuts <= YSMR_VIOLIN_MAX_CUTS. */
int ysmr_violin_stats(void *stream, long long n_tracks, const double *cut_dev, long long cut_stride, const double *value_dev,
                      long long value_stride, int n_cuts, const double *lo_dev, const double *hi_dev, void *workspace_dev,
                      size_t workspace_bytes, ysmr_violin_summary *summaries_dev, double *density_dev);

typedef struct ysmr_violin_view {
    double  y0;                  /* data value at the lower edge of the axes */
    double  units_per_pixel;
    int32_t width, height;       /* the canvas */
    int32_t ax_x, ax_y, ax_w, ax_h;   /* the axes rectangle (top-left pixel, size), inside the canvas */
    int32_t n_violins;           /* 1 .. YSMR_VIOLIN_MAX_SLOTS: entries of the arrays below and of summaries / density */
    int32_t n_grid_rows;
    int32_t line_half;           /* half widths (pixels) of the whisker line and of a degenerate violin's line */
    int32_t box_half;            /* ... of the quartile box */
    int32_t dot_r2;              /* squared radius of the median dot */
    int32_t reserved;
    int32_t grid_rows[32];       /* canvas rows of the grid lines (drawn inside the axes only) */
    int32_t slot_x[64];          /* canvas column of the slot's left edge */
    int32_t slot_w[64];          /* its width; 0: the violin is not drawn.  Slots lie inside the axes and do not overlap */
    int32_t slot_colour[64];     /* position of the violin in the figure: entry (position mod 10) of the fill table */
} ysmr_violin_view;

/* Paints rgb_dev: u8 [height][width][3].  Two steps ("The figures"):
 * profile -- axes row r (0 on top) has the data value y = y0 + ((ax_h - 1 - r) + 0.5) units_per_pixel; inside [vmin, vmax] the
 *   density is interpolated between its grid neighbours, d = d_j + (d_{j+1} - d_j) t (f64, unfused), and
 *   half = floor(d / peak * values / max_values * 0.95 * slot_w / 2), peak = max_j d_j, max_values the largest `values` of the
 *   drawn violins; -1 outside [vmin, vmax].  A value v lies on axes row ax_h - 1 - floor((v - y0) / units_per_pixel);
 * paint -- integers only, every pixel a function of (x, y); layers from the bottom: white, grid rows (176, 176, 176), the
 *   fill |x - cx| <= half (cx = slot_x + slot_w / 2), its outline (fill pixels with a 4-neighbour that is not fill; (76, 76, 76)),
 *   the whisker line, the quartile box (both (76, 76, 76)), the white median dot, and black left and bottom spines just
 *   outside the axes.  A violin with values == 1 or h == 0 is a horizontal line of half length slot_w * 95 / 200 at its value;
 *   one with values == 0 is not drawn.  A violin paints inside its slot and inside the axes only. */
int ysmr_plot_violins(void *stream, int n_violins, const ysmr_violin_summary *summaries_dev, const double *density_dev,
                      const ysmr_violin_view *view, void *workspace_dev, size_t workspace_bytes, uint8_t *rgb_dev);

/* ---- the figures' PNG files: lettering and deflate on the device (csrc/png.hip) ---- */

/* ADDED under ABI 15 as well.  With these a figure leaves the device as a finished zlib stream: the canvas is never
 * downloaded.  Which text goes where stays the host's decision (plot_functions.py). */

typedef struct ysmr_stamp {
    int32_t  x, y;               /* canvas position of the bitmap's top-left pixel; may lie outside the canvas */
    int32_t  w, h;               /* the bitmap's size; a record with w < 1 or h < 1 paints nothing */
    uint32_t bit_offset;         /* of the bitmap's first bit in `bits`: pixel (col, row) is bit bit_offset + row * w + col,
                                    bit k being (bits[k / 8] >> (k % 8)) & 1 */
    uint32_t colour;             /* R | G << 8 | B << 16 */
} ysmr_stamp;

/* Paints the set bits of every record into rgb_dev: u8 [height][width][3]; pixels outside the canvas are dropped (the
 * clipping of stamp_text / stamp_text_vertical).  Where records overlap the LATER record wins, whatever the scheduling: a
 * pixel is stored only by the last record with a set bit on it.  records_dev and bits_dev are device buffers; a record
 * whose bits do not lie inside bits_bytes paints nothing.  0 <= n_records <= 4096, bits_bytes <= 2^28. */
int ysmr_plot_stamp(void *stream, uint8_t *rgb_dev, int width, int height, const ysmr_stamp *records_dev, int n_records,
                    const uint8_t *bits_dev, size_t bits_bytes);

/* The zlib stream of a canvas' PNG scanlines: height rows of S = 1 + 3 width bytes, a filter byte 0 in front of every row.
 * The stream is 78 01, ONE deflate block (BFINAL = 1, BTYPE = 01: the fixed Huffman code of RFC 1951, 3.2.6), the end-of-block
 * code, padding to a byte and the Adler-32 of the scanline bytes, big-endian.  Every row is cut into pieces of 1024 bytes (the
 * last one shorter) and a piece is parsed on its own, greedily: at byte i, with L3 and LS the match lengths at the distances 3
 * and S (LS = 0 when S > 32768), each capped at 258 and at the piece's end -- (L3, 3) if L3 >= LS and L3 >= 3, else (LS, S) if
 * LS >= 4, else the literal.  A match's source may lie anywhere before it.  Integers only and no atomics on a sum: two calls
 * give the same bytes (tests/png_deflate_model.py restates the stream).
 * ysmr_png_stream_bytes_max: ceil((3 + 9 H S + 7) / 8) + 6 -- no code spends more than 9 bits on a byte -- rounded up to a
 * word, plus a word for the packer; out_dev must hold that much and is overwritten up to it.  *out_len_dev: the stream's
 * bytes.  1 <= width, height <= 16384 (the size calls return 0 outside); workspace_dev and out_len_dev 8-byte aligned, out_dev
 * 4-byte aligned.  The calls only enqueue work on `stream`. */
size_t ysmr_png_workspace_bytes(int width, int height);
size_t ysmr_png_stream_bytes_max(int width, int height);
int ysmr_png_deflate(void *stream, const uint8_t *rgb_dev, int width, int height, void *workspace_dev, size_t workspace_bytes,
                     uint8_t *out_dev, size_t out_bytes, unsigned long long *out_len_dev);

/* ADDED under ABI 15 as well: the same scanline bytes as a smaller stream.  78 01, ONE deflate block with BFINAL = 1 and
 * BTYPE = 10 (a dynamic Huffman code, RFC 1951, 3.2.7), the end-of-block code, padding to a byte, Adler-32 big-endian.
 * Parse -- the pieces are ysmr_png_deflate's, and a piece is parsed on its own, greedily, with FOUR distances: 3, S, S - 3 and
 * S + 3 (the pixel before, above, above-right, above-left).  A distance d is eligible at stream position p when d <= 32768 and
 * p >= d; sources are positions of the scanline stream, they cross row ends and include the filter bytes.  At byte i, every
 * length capped at 258 and at the piece's end, the longest eligible match wins; it must have 3 bytes at distance 3 and 4 at
 * the other three; ties go in the order 3, S, S - 3, S + 3; no match: the literal.  With the distances 3 and S alone this is
 * exactly ysmr_png_deflate's rule.
 * Codes -- the histogram of the 286 literal/length symbols (one end of block among them) and of the 30 distance symbols over
 * the whole parse; integer atomics only, so two calls give the same bytes.  While fewer than two distance symbols are used,
 * the lowest unused one counts once (zlib's rule: two distance codes at least).  Code lengths as ysmr_png_code_lengths makes
 * them, at most 15 bits (7 for the code-length alphabet), codes canonical (RFC 1951, 3.2.2).  The header: HLIT, HDIST, HCLEN
 * without trailing zero lengths, then the two length sequences run-length coded as ONE sequence, run by run of equal values:
 * r zeros are 18 (up to 138) while r >= 11, then 17 if r >= 3, then single zeros; r lengths v > 0 are v once, then 16 (up
 * to 6) while r >= 3 remain, then single v's (csrc/png_codes.h; tests/png_dynamic_model.py restates the stream).
 * ysmr_png_dynamic_stream_bytes_max: ceil((4498 + 15 H S + 15) / 8) + 6 -- 4498 bits is the longest header, no code spends
 * more than 15 bits on a byte, the end of block at most 15 -- rounded up to a word, plus a word for the packer; out_dev must
 * hold that much and is zeroed up to it.  Sizes, alignments and status codes as for ysmr_png_deflate; the calls only
 * enqueue work on `stream`. */
size_t ysmr_png_dynamic_workspace_bytes(int width, int height);
size_t ysmr_png_dynamic_stream_bytes_max(int width, int height);
int ysmr_png_deflate_dynamic(void *stream, const uint8_t *rgb_dev, int width, int height, void *workspace_dev, size_t workspace_bytes,
                             uint8_t *out_dev, size_t out_bytes, unsigned long long *out_len_dev);

/* Host only, no GPU touched: the code lengths ysmr_png_deflate_dynamic gives the histogram counts[0 .. n_symbols) under the
 * limit max_bits, from the same text the kernel compiles (csrc/png_codes.h).  The used symbols (count > 0) are sorted by
 * (count, symbol); Huffman's tree is built with two queues, the leaf taken on a tie; leaves deeper than max_bits are counted
 * at max_bits and the Kraft sum is repaired one unit a round (a code of max_bits bits less, one of the longest shorter length
 * i less, two of i + 1 more); the lengths go, shortest first, to the symbols in descending (count, symbol).  Where Huffman's
 * tree fits the limit the total cost is the optimum.  One used symbol has length 1, an unused one 0.
 * 1 <= n_symbols <= 288, 1 <= max_bits <= 15, and no more than 2^max_bits used symbols, else YSMR_ERR_ARG. */
int ysmr_png_code_lengths(const uint32_t *counts, int n_symbols, int max_bits, uint8_t *lengths_out);

#ifdef __cplusplus
}
#endif
#endif /* YSMR_HIP_H */
