/*
 * pcgpu.h — C ABI of the MI355X (gfx950) identity hot path of person_capture.
 *
 * This is the drop-in boundary that replaces the reference's inference runtimes
 * (SURVEY.md §8b). Plain pointers and sizes only; no torch or HIP types appear in
 * the signatures (streams are passed as void*). Every function returns an int
 * status (PC_OK == 0); the message of the last failure on a context is available
 * from pc_last_error(). Device pointers ("d_") are HIP device allocations on the
 * context's device; host pointers ("h_") are ordinary CPU memory.
 *
 * Which reference interface each entry point replaces (file:line in the reference
 * snapshot xmarre/person_capture):
 *
 *   pc_ctx_create / pc_ctx_destroy     ORT InferenceSession(..., providers=[TRT, CUDA, CPU]) setup
 *                                      person_capture/face_embedder.py:557-703, 848-953
 *   pc_net_create                      model load: SCRFD ONNX session (face_embedder.py:1102-1147),
 *                                      ArcFace ONNX session (face_embedder.py:891-953),
 *                                      YOLO(path) (detectors.py:84-269)
 *   pc_net_run                         session.run / run_with_iobinding (face_embedder.py:1331-1343, 1369)
 *   pc_letterbox                       [ext] insightface SCRFD.detect letterbox + cv2.dnn.blobFromImage
 *                                      (called at face_embedder.py:2185)
 *   pc_scrfd_detect                    [ext] SCRFD.detect(img, input_size=(D, D)) -> (det Nx5, kpss Nx5x2)
 *                                      (face_embedder.py:2176-2187)
 *   pc_warp_affine                     cv2.warpAffine(face, M, (112,112), INTER_LINEAR, BORDER_REFLECT)
 *                                      (face_embedder.py:1465-1473)
 *   pc_face_quality                    FaceEmbedder._face_quality (face_embedder.py:1274-1276)
 *   pc_arcface_embed                   FaceEmbedder._arcface_encode (face_embedder.py:1290-1389)
 *   pc_embed_finalize                  flip-sum + L2 (face_embedder.py:1383-1389)
 *   pc_bank_match                      Processor._fd_min (gui_app.py:660-674), batched
 *   pc_rotate_pad                      cv2.rotate + cv2.copyMakeBorder(BORDER_REPLICATE)
 *                                      (face_embedder.py:2165-2169, 2292-2294, 2394)
 *   pc_resize_area                     cv2.resize(..., INTER_AREA) (gui_app.py:1505-1507)
 *   pc_resize_area_batch               the same over a chunk of pre-scan samples (gui_app.py:1505-1507)
 *   pc_resize_linear                   cv2.resize(..., INTER_LINEAR) (face_embedder.py:2264, 2460)
 *   pc_resize_area_fast                cv2.resize(..., INTER_AREA) at integer ratios (face_embedder.py:2460)
 *   pc_face_chips                      the unaligned face chips of the OpenCLIP face mode: cv2.resize(face_bgr,
 *                                      (112,112), INTER_AREA if max(h,w) > 112 else INTER_LINEAR) per kept face
 *                                      (face_embedder.py:2454-2460, 2132-2141), all faces of a batch at once
 *   pc_nv12_to_bgr                     FfmpegPipeReader._nv12_to_bgr (video_io.py:2888-2912), the conversion of
 *                                      the NV12 pipe format (PC_PIPE_PIXFMT=nv12, video_io.py:1225-1228, 1901-1904)
 *   pc_nv12_resize_area_batch /        the same conversion followed by the pre-scan's cv2.resize(..., INTER_AREA)
 *   pc_nv12_resize_area_fast_batch     (gui_app.py:1505-1507) in one pass, no full-size BGR frame in between
 *   pc_hdr_to_bgr                      the float32 HDR pipe format (gbrpf32le, video_io.py:2513-2520): _eotf_pq /
 *                                      _eotf_hlg (video_io.py:3015-3018, 3239-3258) + _python_tonemap_to_bgr8
 *                                      (video_io.py:3183-3192, 3276-3291) with _hable_filmic and _oetf_bt709
 *   pc_yolo_detect                     PersonDetector.detect -> [ext] ultralytics YOLO.predict(conf, iou=0.45,
 *                                      classes=[0], max_det=40, imgsz=640) (detectors.py:271-296)
 *   pc_yolo_pose_detect                FaceEmbedder YOLOv8-face backend (Y8F_DEFAULT, face_embedder.py:33) ->
 *                                      [ext] ultralytics YOLO(pose).predict(conf, iou, max_det, imgsz) with
 *                                      res.boxes + res.keypoints.xy (face_embedder.py:1680-1703, 1391-1429)
 *   pc_clip_prep / pc_clip_embed       ReIDEmbedder.extract: BGR2RGB + open_clip preprocess + encode_image +
 *                                      F.normalize (reid_embedder.py:38-57)
 *   pc_clip_prep_geom / pc_clip_embed_geom   the same for the other towers of ReIDEmbedder(model_name=...)
 *                                      (reid_embedder.py:19-31; the GUI's reid_backbone, gui_app.py:429, 4511):
 *                                      open_clip image_transform(image_size) + the tower's patch size
 *   pc_l2_normalize                    torch.nn.functional.normalize(feats, dim=1) (reid_embedder.py:55)
 *   pc_pil_bicubic_coeffs              Pillow Image.resize(BICUBIC) coefficients inside the open_clip
 *                                      preprocess (reid_embedder.py:49)
 *   pc_crop_metrics                    the cv2 half of phash64, sharpness_norm, exposure_score
 *                                      (dataset_curator.py:55-113) and detect_black_borders
 *                                      (utils.py:152-196), batched; the host finishes them
 *   pc_sim_matrix                      Fs @ Fs.T of Curator.select (dataset_curator.py:961-977)
 *   pc_mmr_order                       mmr_select_with_q (dataset_curator.py:211-238)
 *   pc_frame_gray                      Processor.run's per-frame cv2.cvtColor(frame, BGR2GRAY) (gui_app.py:5754,
 *                                      3425) and the row / column means of detect_black_borders
 *                                      (utils.py:152-196) behind _autocrop_borders (gui_app.py:3360-3384)
 *   pc_gray_region_hist                the strip statistics of _is_real_letterbox_crop (gui_app.py:3429-3447):
 *                                      np.percentile 95 / 99 and np.std, finished on the host from exact counts
 *   pc_gray_motion                     absdiff + threshold(15) + countNonZero of _faceless_validate
 *                                      (gui_app.py:4275-4285), all boxes of a frame at once
 *   pc_gray_resize_area                cv2.resize(gray, (small_w, small_h), INTER_AREA) of _smart_crop_box's
 *                                      gradient saliency (gui_app.py:8295-8301)
 */
#ifndef PCGPU_H
#define PCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_ABI_VERSION 1

#define PC_OK 0
#define PC_ERR_ARG 1
#define PC_ERR_HIP 2
#define PC_ERR_STATE 3
#define PC_ERR_FORMAT 4
#define PC_ERR_CAPACITY 5

/* arithmetic of a network: f16 storage + f32 accumulation (throughput), or
 * exact f32 (parity runs against the CPU oracle). */
#define PC_PREC_F16 0
#define PC_PREC_F32 1
/* pc_arcface_prep / pc_clip_prep only: the centred pixels x - 127.5 in f16 (exact), the input of the
 * f16x3 IResNet program (its stem weights carry the 1/127.5; models.compile_iresnet(split=True)) and
 * of the f16x3 ViT tower (doubled rows, see pc_clip_prep) */
#define PC_PREC_F16X3 2

typedef struct pc_ctx pc_ctx;
typedef struct pc_net pc_net;

/* One letterbox job (SCRFD input): BGR u8 frame on device -> resized into the
 * top-left of a DxD canvas. scale_x/scale_y are 1/(new/old) as cv::resize uses. */
typedef struct pc_letterbox_desc {
  const uint8_t* d_src;
  int32_t H, W, row_stride;
  int32_t new_w, new_h;
  double scale_x, scale_y;
  int32_t simd_end; /* byte index of each row where OpenCV's SIMD vertical pass stops */
  int32_t pad_;
} pc_letterbox_desc;

/* One warpAffine job: crop (top-left pointer + size) -> out_w x out_h x 3 u8.
 * M is the dst->src affine map (cv::warpAffine's internal inverse). */
typedef struct pc_warp_desc {
  const uint8_t* d_src;
  int32_t row_stride;
  int32_t w, h;
  int32_t pad0_;
  double M[6];
  uint8_t* d_dst;
  int32_t out_w, out_h;
  int32_t border; /* 2 = BORDER_REFLECT, 4 = BORDER_REFLECT_101, 0 | (value << 8) = BORDER_CONSTANT */
  int32_t pad1_;
} pc_warp_desc;

/* One u8 -> u8 bilinear resize job (cv2.resize semantics, BGR): INTER_LINEAR, or INTER_AREA
 * when not both axes downscale (area_mode = 1: OpenCV's area-mode linear coefficients). */
typedef struct pc_resize_desc {
  const uint8_t* d_src;
  int32_t H, W, row_stride;
  int32_t new_w, new_h;
  double scale_x, scale_y; /* 1 / inv_scale */
  int32_t simd_end;
  int32_t area_mode;
  uint8_t* d_dst; /* new_h x new_w x 3 contiguous */
  double inv_x, inv_y; /* dsize / ssize, or the fx / fy given */
} pc_resize_desc;

/* One INTER_AREA coefficient: source index, destination index, weight. */
typedef struct pc_area_tab {
  int32_t si;
  int32_t di;
  float alpha;
} pc_area_tab;

/* One YOLOv8 letterbox job ([ext] ultralytics LetterBox(auto=True, stride=32), detectors.py:274):
 * BGR u8 frame -> cv2.resize INTER_LINEAR to new_w x new_h placed at (left, top) of an
 * Hp x Wp canvas filled with 114; identity = 1 when no resize happens (same shape). */
typedef struct pc_yolo_letterbox_desc {
  const uint8_t* d_src;
  int32_t H, W, row_stride;
  int32_t new_w, new_h;
  int32_t top, left;
  double scale_x, scale_y;
  int32_t simd_end;
  int32_t identity;
} pc_yolo_letterbox_desc;

/* [ext] ultralytics ops.scale_boxes per frame: box = clip((box - pad) / gain, [0,W0] x [0,H0]) */
typedef struct pc_yolo_scale {
  float gain, pad_x, pad_y, W0, H0;
} pc_yolo_scale;

/* One BGR u8 image crop on the device (top-left pointer, size, bytes per row). */
typedef struct pc_crop_desc {
  const uint8_t* d_src;
  int32_t H, W, row_stride, pad_;
} pc_crop_desc;

/* One face rectangle of pc_face_chips: BGR u8 on the device (top-left pointer at any byte offset of a
 * frame, size, bytes per row of the frame). */
typedef struct pc_chip_desc {
  const uint8_t* d_src;
  int32_t H, W, row_stride, pad_;
} pc_chip_desc;
/* the cv::resize path of a rectangle (pc_face_chip_plan) */
#define PC_CHIP_COPY 0      /* 112 x 112: copied */
#define PC_CHIP_AREA_FAST 1 /* INTER_AREA at integer ratios (1 on an axis included) */
#define PC_CHIP_AREA 2      /* INTER_AREA, both axes shrink: generic float coefficients */
#define PC_CHIP_LINEAR 3    /* bilinear; area_mode 1 when INTER_AREA was asked but an axis upscales */
#define PC_CHIP_SIDE 112
#define PC_CHIP_MAX_SIDE 16384

/* One NV12 frame of pc_nv12_to_bgr on the device: the Y plane (H rows of W bytes, y_stride apart), the
 * interleaved U, V plane (H / 2 rows of W bytes, uv_stride apart) and the BGR u8 destination (H rows of
 * 3 W bytes, dst_stride apart). H and W even, 2 .. PC_NV12_MAX_SIDE. */
typedef struct pc_nv12_desc {
  const uint8_t* d_y;
  const uint8_t* d_uv;
  int32_t H, W, y_stride, uv_stride;
  uint8_t* d_dst;
  int32_t dst_stride;
  int32_t pad_;
} pc_nv12_desc;
#define PC_NV12_MAX_SIDE 16384

/* One HDR frame of pc_hdr_to_bgr on the device: float32 R, G and B samples of the PQ / HLG signal (or of
 * linear light), sample (y, x) of a channel at its pointer + y * row_stride + x * pix_stride floats, and the
 * BGR u8 destination (H rows of 3 W bytes, dst_stride apart). pix_stride 1: three planes (the pipe's gbrpf32le
 * bytes wrapped as they are: d_g, d_b, d_r in that order in memory); pix_stride 3: an interleaved H x W x 3
 * RGB array (d_g = d_r + 1, d_b = d_r + 2). H and W 1 .. PC_HDR_MAX_SIDE, no parity requirement.
 * target_nits / peak_nits: the arguments of _python_tonemap_to_bgr8. */
typedef struct pc_hdr_desc {
  const float* d_r;
  const float* d_g;
  const float* d_b;
  int32_t H, W, pix_stride, row_stride;
  uint8_t* d_dst;
  int32_t dst_stride;
  int32_t transfer; /* PC_HDR_PQ / PC_HDR_HLG / PC_HDR_LINEAR */
  double target_nits, peak_nits;
} pc_hdr_desc;
#define PC_HDR_MAX_SIDE 16384
#define PC_HDR_PQ 0     /* _eotf_pq (video_io.py:3239-3251) */
#define PC_HDR_HLG 1    /* _eotf_hlg (video_io.py:3254-3258), the reader's _transfer == "arib-std-b67" */
#define PC_HDR_LINEAR 2 /* the samples are linear light already (1.0 = 10 000 nits) */

/* One crop of the dataset curator's metrics batch (pc_crop_metrics): a BGR u8 image on the device and
 * the geometry of its two INTER_AREA targets, [0] the <= 256 plane of sharpness_norm (w2 x h2;
 * the gray plane itself when max(h, w) <= 256) and [1] the 32 x 32 plane of phash64. Per target:
 * kind (PC_CURATE_COPY: the gray plane is the target; PC_CURATE_FAST: integer ratios isx x isy,
 * OpenCV's resizeAreaFast; PC_CURATE_AREA: generic tables), and for PC_CURATE_AREA the positions
 * xs / ys in h_starts of the target's x / y start arrays (ow + 1 / oh + 1 entries, each an index
 * into h_tabs; destination d's coefficients are h_tabs[start[d] .. start[d + 1])). */
#define PC_CURATE_COPY 0
#define PC_CURATE_FAST 1
#define PC_CURATE_AREA 2
typedef struct pc_curate_desc {
  const uint8_t* d_src;
  int32_t row_stride, w, h;
  int32_t w2, h2;
  int32_t kind[2];
  int32_t isx[2], isy[2];
  int32_t xs[2], ys[2];
  int32_t pad_;
} pc_curate_desc;

/* The per-image record pc_crop_metrics writes at the front of d_out (n records, then the row and
 * column sums): everything except coef is an exact integer. */
typedef struct pc_curate_record {
  uint64_t sum_g2;    /* sum of the <= 256 plane */
  int64_t sum_lap;    /* sum of its ksize-1 Laplacian (BORDER_REFLECT_101) */
  uint64_t sum_lap2;  /* sum of the squares */
  int32_t w2, h2;
  uint32_t hist[256]; /* of the full-size gray plane */
  float coef[64];     /* [u][v] 8x8 low-frequency block of the orthonormal DCT-II of the 32 x 32 plane */
} pc_curate_record;

/* One frame of pc_frame_gray: a BGR u8 image on the device (32 <= w, h <= PC_GAUGE_MAX_SIDE, rows row_stride
 * >= 3 w bytes apart) and where its results go: the gray plane (h rows of gray_pitch bytes; pointer and pitch
 * multiples of 16, gray_pitch >= w rounded up to 16: the bytes of a row from w to that multiple are written as
 * 0), row_sum[h] and col_sum[w] (u32, 4-byte aligned). */
typedef struct pc_gray_desc {
  const uint8_t* d_src;
  int32_t row_stride, w, h;
  int32_t gray_pitch;
  uint8_t* d_gray;
  uint32_t* d_row_sum;
  uint32_t* d_col_sum;
} pc_gray_desc;
#define PC_GAUGE_MAX_SIDE 16384

/* One rectangle of pc_gray_region_hist: columns [x, x + w), rows [y, y + h) of a u8 plane whose rows are
 * pitch bytes apart. 1 <= w, h <= PC_GAUGE_MAX_SIDE, 0 <= x, y, x + w <= pitch <= PC_GAUGE_MAX_PITCH,
 * y + h <= PC_GAUGE_MAX_SIDE (the caller answers for the plane having that many rows). */
typedef struct pc_gray_region {
  const uint8_t* d_plane;
  int32_t pitch, x, y, w, h;
  int32_t pad_;
} pc_gray_region;
#define PC_GAUGE_MAX_PITCH (1 << 20)

/* One box of pc_gray_motion: columns [x1, x2), rows [y1, y2) of two u8 planes of the same pitch.
 * 0 <= x1 < x2 <= pitch <= PC_GAUGE_MAX_PITCH, 0 <= y1 < y2 <= PC_GAUGE_MAX_SIDE, x2 - x1 <= PC_GAUGE_MAX_SIDE. */
typedef struct pc_motion_box {
  const uint8_t* d_cur;
  const uint8_t* d_prev;
  int32_t pitch, x1, y1, x2, y2;
  int32_t pad_;
} pc_motion_box;

int pc_abi_version(void);

/* ---- context ---- */
int pc_ctx_create(int device_id, pc_ctx** out);
int pc_ctx_destroy(pc_ctx* ctx);
const char* pc_last_error(const pc_ctx* ctx);
int pc_ctx_set_stream(pc_ctx* ctx, void* hip_stream); /* NULL = context-owned stream */
void* pc_ctx_stream(pc_ctx* ctx);
/* Re-create the context-owned stream at a HIP stream priority (lower = higher priority,
 * clamped to the device's range). No reference counterpart: the face embedder's second
 * (embed) stream is a build-side scheduling choice (two streams). */
int pc_ctx_set_priority(pc_ctx* ctx, int priority);
int pc_ctx_sync(pc_ctx* ctx);
int pc_device_alloc(pc_ctx* ctx, size_t bytes, void** d_out);
int pc_device_free(pc_ctx* ctx, void* d_ptr);
/* stream-ordered wait: work enqueued on ctx after this call waits for fence f (recorded on any
 * context of the same device). */
int pc_ctx_wait_fence(pc_ctx* ctx, void* f);
/* host frame staging (replaces the per-frame pageable upload of the reference's frame feed,
 * video_io.py:1093-1135 -> FaceEmbedder.extract): rows of row_bytes, src_stride apart, packed
 * by up to `threads` host threads into a ring of 4 pinned slots, then one async H2D on the
 * context stream. The host array may be reused when this returns. */
int pc_frame_stage(pc_ctx* ctx, void* d_dst, const void* h_src, size_t row_bytes, size_t rows, size_t src_stride,
                   int threads);
int pc_copy_h2d(pc_ctx* ctx, void* d_dst, const void* h_src, size_t bytes); /* stream-ordered */
int pc_copy_d2h(pc_ctx* ctx, void* h_dst, const void* d_src, size_t bytes); /* stream-ordered */
int pc_copy_d2d(pc_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int pc_memset(pc_ctx* ctx, void* d_dst, int value, size_t bytes);
/* device -> device pitched copy (cv2.resize to the same size copies, resize.cpp) */
int pc_copy_2d(pc_ctx* ctx, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch, size_t width_bytes,
               size_t rows);
/* Pinned host memory (page-locked: D2H copies into it stay asynchronous) and stream
 * fences. A fence is a HIP event recorded on the context stream; pc_fence_wait blocks
 * the host until everything enqueued before the record has finished. Used to overlap
 * the host-side detector policy of one chunk of frames with device work of the next
 * (FaceEmbedder.extract_batch). */
int pc_host_alloc(pc_ctx* ctx, size_t bytes, void** h_out);
int pc_host_free(pc_ctx* ctx, void* h_ptr);
int pc_fence_create(pc_ctx* ctx, void** fence_out);
int pc_fence_record(pc_ctx* ctx, void* fence);
int pc_fence_wait(pc_ctx* ctx, void* fence);
int pc_fence_destroy(pc_ctx* ctx, void* fence);

/* ---- networks (serialized program produced by person_capture_amd.netdef) ---- */
/* pc_net_create and pc_net_plan decode and validate the program first (csrc/pc_program.cpp) and refuse, with
 * PC_ERR_FORMAT and a message that names the op kind and the rule (pc_last_error / pc_net_plan's err), before
 * anything is allocated or launched:
 *   ids       a tensor, buffer or array id outside its table; an unknown op kind; a truncated table
 *   tensors   H, W or C below 1; a channel slice [coff, coff + C) outside the pixel stride cs; H * W * cs
 *             beyond the tensor's buffer; is_f32 unlike its buffer's; split / f16c8 storage rules
 *   element   a max pool, upsample, LayerNorm or attention that reads or writes, or a stem that reads, an
 *   type      is_f32 tensor of an f16 net (those kernels move the net's own type)
 *   max pool  k < 1, stride < 1, pad outside [0, k / 2]; an output that is not (H + 2 pad - k) / stride + 1 in
 *             each direction; channels unlike the input's; C, cs or coff no multiple of 4
 *   upsample  an output that is not exactly twice the input; min(C), cs or coff no whole 16-byte vectors
 *   LayerNorm C outside [1, 2048], wider than its input or output (the halves of split tensors), an output
 *             wider than 2048; pixel counts that differ; gamma or beta shorter than C; a positional table
 *             whose rows are not the pixels of an image or whose array is shorter than rows * C
 *   attention a head dim other than 64 / 80; 3 * heads * d wider than qkv or heads * d wider than the output
 *             (halves); token counts that differ; qkv cs no multiple of 8, output cs no multiple of 4 (f32)
 *             or 8; an offset not aligned to 16 bytes
 *   conv      1 or 2 segments; an output size that does not follow from every segment's window; a same-size
 *             residual of another size, an upsampled one that is not half the output rounded up; weights
 *             shorter than npad * ktot, bias shorter than npad (9 * npad in border mode), slopes than npad
 * A net that is created is runnable: no shape rule is left to fail as a launch error. */
int pc_net_create(pc_ctx* ctx, const void* h_program, size_t program_bytes, int precision, int max_batch,
                  pc_net** out);
int pc_net_destroy(pc_net* net);
/* d_input: NHWC, dims as pc_net_input_dims; activation dtype of the net's precision */
int pc_net_run(pc_net* net, const void* d_input, int batch);
int pc_net_input_dims(pc_net* net, int32_t* h_dims4 /* H, W, C, pixel stride */);
int pc_net_output(pc_net* net, int index, void** d_ptr, int32_t* h_dims5 /* H, W, C, pixel stride, is_f32 */);
int pc_net_num_outputs(pc_net* net);
/* algorithmic FLOPs per image (2*MAC over all conv layers) and kernel launches per run */
int pc_net_stats(pc_net* net, double* h_flops_per_image, int32_t* h_launches);
/* resident block chains of the net (pc_conv_chain: runs of IResNet identity blocks executed
 * one image per workgroup): returns their count; *h_min_batch = the batch from which they
 * are used, *h_images_per_round = images one round of workgroups covers (the CU count).
 * (No reference counterpart: a scheduling hint for FaceEmbedder's ArcFace batch quantum.) */
int pc_net_chain_info(pc_net* net, int32_t* h_min_batch, int32_t* h_images_per_round);
/* the chained conv_hxi launches a plan would make (host logic only, no device): ops = n_ops x 32 program
 * op words, eligible[i] != 0 marks the ops the plan runs on the one-image-per-workgroup f16x3 forms,
 * outs the net's output tensors, cap the layers per launch (<= 0: no cap). Writes up to max_runs
 * (first op, layers) pairs and returns the number of launches. (No reference counterpart.) */
int pc_plan_hxi_runs(const int32_t* h_ops, int n_ops, const int32_t* h_eligible, const int32_t* h_outs, int n_outs,
                     int cap, int32_t* h_runs, int max_runs);
/* The plans pc_net_create would make for a program under the current environment (host logic only, no
 * device): decodes, validates and plans. Writes the small-batch class sizes (ascending, at most max_cls)
 * to h_cls_batch and, per (class c, op i), PC_PLAN_WORDS int32 at h_plans[(c * max_ops + i) * PC_PLAN_WORDS];
 * class 0 is the max-batch plan, class 1 + k the plan for runs of at most h_cls_batch[k] images:
 *   [0] op kind  [1] kernel code and [2] form word, as pc_net_profile_ops reports them in [4] / [5] for a
 *   per-layer launch of the op (-1 for ops that are no convs)  [3] K-row bytes  [4] split-K  [5] igemm tile cfg
 * Returns the number of classes (1 + the small-batch ones), or -PC_ERR_* with the message in err (err_len
 * bytes, may be null). (No reference counterpart.) */
#define PC_PLAN_WORDS 6
int pc_net_plan(const void* h_program, size_t program_bytes, int precision, int max_batch, int32_t* h_cls_batch,
                int max_cls, int32_t* h_plans, int max_ops, char* err, int err_len);
/* the batch from which the chains run (<= 0: never). A chain workgroup needs a whole CU's
 * LDS, so a net that shares the device with another stream's kernels (FaceEmbedder's embed
 * stream beside SCRFD) runs faster per-conv: measured C3 1925 vs 1705 frames/s. */
int pc_net_set_chain_min_batch(pc_net* net, int32_t min_batch);
/* capture pc_net_run(batch) into a HIP graph and replay it on later runs of the same batch */
int pc_net_set_graph(pc_net* net, int enable);
/* with graphs enabled, capture / replay only runs of at most max_batch images (the per-frame
 * extract() path: dozens of small launches per net run); larger runs launch eagerly (and can
 * be profiled). Default: every batch. Replaces nothing in the reference (launch plumbing). */
int pc_net_set_graph_max_batch(pc_net* net, int32_t max_batch);
/* HIP-event timing of every op of every later (non-graph) run; enable resets the counters.
 * read: [0] conv ms, [1] conv launches, [2] conv FLOPs (algorithmic), [3] other ms, [4] other launches */
int pc_net_profile(pc_net* net, int enable);
/* f16c8 nets: run the program once on N images at d_in and set every f16c8 tensor's
 * e4m3 scale exponents from its largest magnitude, 2^headroom_log2 below the format's range. Clears the
 * net's captured graphs. h_absmax (optional, [n_tensor] floats): the measured max |x| per tensor (0 where
 * not measured). Replaces no reference interface (the reference's TensorRT engines carry no such
 * scales: f16c8 is this build's f32-class arithmetic on the f16 / fp8 MFMA path). */
int pc_net_calibrate(pc_net* net, const void* d_in, int N, int headroom_log2, float* h_absmax);
int pc_net_profile_read(pc_net* net, double* h_out5);
/* Per-launch detail of the profiled runs, 6 doubles per record: op index, op kind, ms, FLOPs,
   kernel (100+k: static-schedule tile k, 600+k: its f16c8 form, 200+v: t2d variant v, 300: resident chain, 500: halo-staged f16x3, k >= 0: halo tile k, -1: generic implicit-GEMM), implicit-GEMM tile (static-schedule tiles: their form, bit 0 fused split, bit 1 register weight fragments, bit 2 128-byte K rows). Returns the record count (<0: -status). */
int pc_net_profile_ops(pc_net* net, double* h_out, int max_recs);

/* ---- image kernels ---- */
int pc_letterbox(pc_ctx* ctx, int precision, const pc_letterbox_desc* h_descs, int n, int D, void* d_out);
int pc_warp_affine(pc_ctx* ctx, const pc_warp_desc* h_descs, int n);
int pc_resize_linear(pc_ctx* ctx, const pc_resize_desc* h_descs, int n);
int pc_face_quality(pc_ctx* ctx, const uint8_t* d_chips, int n, int side, double* d_out);
/* precision PC_PREC_F16 / PC_PREC_F32: x/127.5 - 1 in that dtype (face_embedder.py:1281-1288);
 * PC_PREC_F16X3: x - 127.5 in f16 (the f16x3 program's centred input) */
int pc_arcface_prep(pc_ctx* ctx, int precision, const uint8_t* d_chips, int n, int side, int flip, void* d_out);
int pc_rotate_pad(pc_ctx* ctx, const uint8_t* d_src, int H, int W, int row_stride, int deg, int pad, uint8_t* d_dst);
/* cv2.resize INTER_AREA at an exact integer ratio isx x isy (OpenCV resizeAreaFast). */
int pc_resize_area_fast(pc_ctx* ctx, const uint8_t* d_src, int row_stride, int isx, int isy, uint8_t* d_dst, int OH,
                        int OW);
int pc_resize_area(pc_ctx* ctx, const uint8_t* d_src, int row_stride, const pc_area_tab* h_xtab,
                   const int32_t* h_xstart, int n_x, const pc_area_tab* h_ytab, const int32_t* h_ystart, int n_y,
                   uint8_t* d_dst, int OH, int OW);
/* The same cv2.resize INTER_AREA for n equally sized frames at once (the pre-scan's downscale of a
 * speculative chunk of samples, gui_app.py:1505-1507 per sample): h_srcs / h_dsts are host arrays of n
 * device pointers, tables as pc_resize_area. 16-byte aligned sources and row_stride take the row-
 * staged kernel (one launch); others the per-pixel one. Output bytes equal pc_resize_area's. */
int pc_resize_area_batch(pc_ctx* ctx, const uint8_t* const* h_srcs, uint8_t* const* h_dsts, int n, int row_stride,
                         const pc_area_tab* h_xtab, const int32_t* h_xstart, int n_x, const pc_area_tab* h_ytab,
                         const int32_t* h_ystart, int n_y, int OH, int OW);
/* Host only (no context, no device): which path OpenCV 4.9's cv::resize takes for an H x W u8 rectangle
 * resized to 112 x 112 with INTER_AREA if max(H, W) > 112 else INTER_LINEAR, as pc_face_chips decides it
 * (the same decision as imageops.resize_plan). h_out4 = PC_CHIP_* kind, isx, isy (integer ratios, for
 * PC_CHIP_AREA_FAST), area_mode (for PC_CHIP_LINEAR). PC_ERR_ARG unless 1 <= H, W <= PC_CHIP_MAX_SIDE. */
int pc_face_chip_plan(int H, int W, int32_t* h_out4);
/* n face rectangles of any sizes and paths -> d_chips [n][112][112][3] u8, chip i exactly
 * cv2.resize(rectangle i, (112,112), INTER_AREA if max(H,W) > 112 else INTER_LINEAR): the bytes of
 * pc_copy_2d / pc_resize_area_fast / pc_resize_area / pc_resize_linear for that rectangle. One descriptor
 * upload and one launch whatever n and the mix of sizes; the INTER_AREA coefficients are derived on the
 * device. n == 0: PC_OK, nothing enqueued. A null pointer, H or W outside [1, PC_CHIP_MAX_SIDE],
 * row_stride < 3 W or n < 0: PC_ERR_ARG before anything is enqueued. */
int pc_face_chips(pc_ctx* ctx, const pc_chip_desc* h_descs, int n, uint8_t* d_chips);
/* FfmpegPipeReader._nv12_to_bgr (video_io.py:2888-2912) for n NV12 frames of any mix of sizes in one
 * launch: each chroma sample serves its 2 x 2 pixels; in f32 with every operation rounded once (no fused
 * multiply-add), C = y - 16, D = u - 128, E = v - 128, r = k0 C + k1 E, g = (k0 C - k2 D) - k3 E,
 * b = k0 C + k4 D with k = (1.16438356, 1.79274107, 0.21324861, 0.53290933, 2.11240179) rounded to f32,
 * clamped to [0, 255], truncated, stored B, G, R. Frames whose pointers and strides are all multiples of 16
 * move 16 bytes per load and store; others (and the last W % 16 pixels of a row) go byte by byte. Nothing
 * outside [row, row + W) of a source row is read, nothing outside [row, row + 3 W) of a destination row
 * written. n == 0: PC_OK, nothing enqueued. A null pointer, an odd size or one outside [2, PC_NV12_MAX_SIDE],
 * y_stride < W, uv_stride < W, dst_stride < 3 W or n < 0: PC_ERR_ARG before anything is staged or enqueued. */
int pc_nv12_to_bgr(pc_ctx* ctx, const pc_nv12_desc* h_descs, int n);
/* pc_nv12_to_bgr followed by pc_resize_area_batch (the pre-scan's downscale, gui_app.py:1505-1507, of
 * frames the NV12 pipe delivered, video_io.py:2888-2912) for n equally sized H x W NV12 frames, without
 * the full-size BGR frame: every output pixel is the INTER_AREA sum over source pixels converted in
 * registers, so the bytes equal the two calls'. h_ys / h_uvs / h_dsts: host arrays of n device pointers
 * (destination OH x OW x 3 contiguous); tables as pc_resize_area, every source index checked against H, W. */
int pc_nv12_resize_area_batch(pc_ctx* ctx, const uint8_t* const* h_ys, const uint8_t* const* h_uvs,
                              uint8_t* const* h_dsts, int n, int H, int W, int y_stride, int uv_stride,
                              const pc_area_tab* h_xtab, const int32_t* h_xstart, int n_x, const pc_area_tab* h_ytab,
                              const int32_t* h_ystart, int n_y, int OH, int OW);
/* The same at an exact integer ratio isx x isy (pc_resize_area_fast's arithmetic; OW isx <= W, OH isy <= H). */
int pc_nv12_resize_area_fast_batch(pc_ctx* ctx, const uint8_t* const* h_ys, const uint8_t* const* h_uvs,
                                   uint8_t* const* h_dsts, int n, int H, int W, int y_stride, int uv_stride, int isx,
                                   int isy, int OH, int OW);
/* _eotf_pq / _eotf_hlg (video_io.py:3239-3258) followed by _python_tonemap_to_bgr8 (video_io.py:3276-3291)
 * for n HDR frames of any mix of sizes, layouts and transfers in one launch: per pixel the EOTF of each
 * channel, BT.2020 luminance, the Hable curve, the rescale, the BT.709 OETF, trunc(o * 255 + 0.5), stored
 * B, G, R. Every operation in f32 rounded once in the reference's order (no fused multiply-add, IEEE
 * division, subnormals kept); power and exp are the f64 functions rounded to f32 (the operation in full:
 * person_capture_amd/frames_hdr.py). Frames whose sample pointers and row strides are multiples of 16 bytes
 * and whose destination pointer and stride are multiples of 4 move 16 bytes per load and 12 per store;
 * others (and the last W % 4 pixels of a row) go float by float and byte by byte. No float outside the W
 * pixels of a source row is read, nothing outside [row, row + 3 W) of a destination row written; a NaN
 * sample gives some byte. n == 0: PC_OK, nothing enqueued. A null pointer, a sample pointer not 4-byte
 * aligned, H or W outside [1, PC_HDR_MAX_SIDE], pix_stride other than 1 or 3, row_stride < W pix_stride,
 * dst_stride < 3 W, an unknown transfer, target_nits or peak_nits non-finite or <= 0, or n < 0: PC_ERR_ARG
 * before anything is staged or enqueued, whichever frame of the batch is the bad one. */
int pc_hdr_to_bgr(pc_ctx* ctx, const pc_hdr_desc* h_descs, int n);

/* ---- detection ---- */
/* Runs letterbox -> SCRFD net -> decode(score >= det_thresh) -> NMS(nms_thresh) for n frames.
 * Outputs (device): d_dets [n][max_det][5], d_kps [n][max_det][10], d_count [n] (number kept,
 * may exceed max_det: then only the first max_det rows are written; call again with a larger
 * max_det for the full list), d_ncand [n] candidates above threshold. No candidate cap: every
 * anchor of the net has a slot, as the reference keeps every candidate >= det_thresh. */
int pc_scrfd_detect(pc_net* net, const pc_letterbox_desc* h_descs, int n, int D, float det_thresh,
                    float nms_thresh, const float* h_det_scale, int max_det, float* d_dets, float* d_kps,
                    int32_t* d_count, int32_t* d_ncand);

/* ---- embedding / match ---- */
int pc_embed_finalize(pc_ctx* ctx, const float* d_e, int ld, int n, int dim, int flip, float* d_out);
/* chips: [n][side][side][3] BGR u8 (side == net input side). d_feat: [n][dim] unit f32. A net whose
 * program flags a centred input (f16x3 IResNet) gets the PC_PREC_F16X3 preprocessing. */
int pc_arcface_embed(pc_net* net, const uint8_t* d_chips, int n, int flip, float* d_feat);
/* Processor._fd_min for n query rows d_q [n][dim] against d_bank [b][dim] unit rows: each query is divided
 * by max(||q||, 1e-6), d_fd[i] = 1 - max_r dot(bank[r], q_i), d_idx[i] (may be null) the first row that
 * reaches the maximum. An empty bank (b == 0; d_bank is not read) gives d_fd[i] = 9.0 and d_idx[i] = -1.
 * dim % 64 != 0 or dim > 1024: PC_ERR_HIP, nothing enqueued (pc_embed_finalize and pc_l2_normalize too). */
int pc_bank_match(pc_ctx* ctx, const float* d_q, int n, const float* d_bank, int b, int dim, float* d_fd,
                  int32_t* d_idx);

/* ---- person detection (YOLOv8) ---- */
/* letterbox -> YOLOv8 net -> DFL decode (best class 0, score > conf) -> NMS(iou) -> scale_boxes,
 * for n frames sharing one Hp x Wp canvas. d_dets [n][max_det][5] (x1, y1, x2, y2, conf) in frame
 * pixels, d_count [n] kept (<= max_det), d_ncand [n] candidates (capacity 16384 per frame). */
/* letterbox only (the first stage of pc_yolo_detect): d_out [n][Hp][Wp][4] in the precision's dtype */
int pc_yolo_letterbox(pc_ctx* ctx, int precision, const pc_yolo_letterbox_desc* h_descs, int n, int Hp, int Wp,
                      void* d_out);
int pc_yolo_detect(pc_net* net, const pc_yolo_letterbox_desc* h_descs, int n, int Hp, int Wp, float conf, float iou,
                   const pc_yolo_scale* h_scale, int max_det, float* d_dets, int32_t* d_count, int32_t* d_ncand);
/* Pose-head variant (YOLOv8-face, nkpt keypoints x (x, y, visibility)): as pc_yolo_detect (all
 * classes kept, the head's nc = channels - 64 - 3 nkpt), plus d_kpts [n][max_det][nkpt][3] in frame
 * pixels: Pose.kpts_decode, ops.scale_coords with h_kpt_pad [n][2] = the unrounded letterbox pad
 * ((Wp - W gain) / 2, (Hp - H gain) / 2), clip, and x = y = 0 where visibility < 0.5. */
int pc_yolo_pose_detect(pc_net* net, const pc_yolo_letterbox_desc* h_descs, int n, int Hp, int Wp, float conf,
                        float iou, const pc_yolo_scale* h_scale, const float* h_kpt_pad, int max_det, int nkpt,
                        float* d_dets, float* d_kpts, int32_t* d_count, int32_t* d_ncand);

/* ---- ReID body embedding (OpenCLIP ViT-L/14 image tower) ---- */
/* preprocess n crops -> ViT-L/14 patch matrix [n][257][608] (token 0 and K padding zero), normalised, in the
 * precision's dtype. PC_PREC_F16X3: [n][257][1216] f16, each row the centred pixels x - 127.5 (x the
 * Pillow-resampled u8 value; exact in f16) written twice as two 608-wide halves, token 0 and columns
 * 588..607 of each half zero - the input of the f16x3 tower, whose program carries the normalisation
 * (models_clip.compile_clip_vit(split=True)). */
int pc_clip_prep(pc_ctx* ctx, int precision, const pc_crop_desc* h_crops, int n, void* d_out);
/* preprocess + image tower + F.normalize: d_feat [n][dim] unit f32. The net's input selects the
 * preprocessing: 1x257x608 the normalised matrix in the net's dtype; 1x257x1216 flagged centred on an
 * f16 net the PC_PREC_F16X3 form (any other width / flag combination: PC_ERR_FORMAT, nothing launched).
 * The f16x3 tower holds its weights as [W_hi, W_hi, W_lo] f16 (6 bytes per parameter against 4 for
 * f32) and its activations as [hi | lo] pairs (twice the f16 arena). */
int pc_clip_embed(pc_net* net, const pc_crop_desc* h_crops, int n, float* d_feat);
/* pc_clip_prep for any tower of the OpenCLIP ViT family (ReIDEmbedder(model_name=...),
 * reid_embedder.py:19-31: open_clip preprocess at the model's image size): Resize(side) + CenterCrop(side)
 * with side in {224, 336}, patches of `patch` in {14, 16, 32} pixels (side % patch == 0; else PC_ERR_ARG).
 * d_out [n][T][Kp], T = (side / patch)^2 + 1, Kp = 3 patch^2 rounded up to 32 (PC_PREC_F16X3: [n][T][2 Kp]);
 * same arithmetic and modes. pc_clip_prep is this call at (224, 14). */
int pc_clip_prep_geom(pc_ctx* ctx, int precision, int side, int patch, const pc_crop_desc* h_crops, int n, void* d_out);
/* pc_clip_embed for a tower of that geometry (ReIDEmbedder.extract, reid_embedder.py:38-57, with the
 * model_name of reid_embedder.py:19-31). The net's input must be 1 x T x Kp (or 1 x T x 2 Kp flagged centred
 * on an f16 net) for exactly this side and patch: anything else is PC_ERR_FORMAT before any launch - the
 * geometry is never guessed from the padded width. pc_clip_embed is this call at (224, 14). */
int pc_clip_embed_geom(pc_net* net, int side, int patch, const pc_crop_desc* h_crops, int n, float* d_feat);
/* rows of d_e (stride ld floats) / max(||row||, eps) -> d_out [n][dim] */
int pc_l2_normalize(pc_ctx* ctx, const float* d_e, int ld, int n, int dim, float eps, float* d_out);
/* Pillow BICUBIC resample coefficients (precompute_coeffs + normalize_coeffs_8bpc) for output
 * positions [first, first+count) of an in_size -> out_size resize: h_bounds [count][2] (min, n),
 * h_kk [count][ksize] Q22. Returns ksize (< 0: -status). */
int pc_pil_bicubic_coeffs(int in_size, int out_size, int first, int count, int32_t* h_bounds, int32_t* h_kk, int kmax);
/* torchvision Resize(side) + CenterCrop(side) geometry: h_out4 = resized w, h, crop top, left */
int pc_clip_geometry(int h, int w, int side, int32_t* h_out4);

/* ---- dataset curator: crop metrics and MMR ranking ---- */
/* Host only (no context, no device): checks n descriptors (32 <= w, h <= 16384, row_stride >= 3 w,
 * w2 / h2 = the reference's int(round(w s)), int(round(h s)) with s = 256 / max(h, w) and >= 1, 32 x 32
 * for target 1, kinds that fit the sizes; anything else PC_ERR_ARG) and lays out the buffers of
 * pc_crop_metrics. h_off [n][5] byte offsets: [0] gray plane, [1] <= 256 plane, [2] 32 x 32 plane in
 * d_scratch (pitches: width rounded up to 16; a PC_CURATE_COPY target is the gray plane), [3] the
 * image's pc_curate_record, [4] its row_sum[h] then col_sum[w] (u32) in d_out. */
int pc_crop_metrics_layout(const pc_curate_desc* h_imgs, int n, uint64_t* h_off, size_t* h_scratch_bytes,
                           size_t* h_out_bytes);
/* The image half of the curator's per-crop metrics for n crops in four launches, stream-ordered:
 * BGR2GRAY (14-bit coefficients, as pc_face_quality) with histogram, row and column sums (what
 * exposure_score, dataset_curator.py:101-113, and detect_black_borders, utils.py:152-196, read), the
 * INTER_AREA planes of sharpness_norm (dataset_curator.py:81-98) and phash64 (dataset_curator.py:55-71),
 * the Laplacian sums, and the DCT block from the host's cosine table h_dct [8][32] f64
 * (c_u cos(pi (2 x + 1) u / 64)). Buffers are the caller's, sized and laid out by
 * pc_crop_metrics_layout; d_out is zeroed here. The host derives the reference's values from the
 * integers (person_capture_amd/curate.py). */
int pc_crop_metrics(pc_ctx* ctx, const pc_curate_desc* h_imgs, int n, const pc_area_tab* h_tabs, int n_tabs,
                    const int32_t* h_starts, int n_starts, const double* h_dct, void* d_scratch, size_t scratch_bytes,
                    void* d_out, size_t out_bytes);
/* S = F F^T of Curator.select (dataset_curator.py:961-977; Fs @ Fs.T at :972): d_F [n][dim] f32 rows
 * (unit or all zero), d_S [n][n] f32. Every element is one fmaf chain over k ascending, so S is
 * exactly symmetric and two runs give the same bytes. 1 <= n <= 8192. */
int pc_sim_matrix(pc_ctx* ctx, const float* d_F, int n, int dim, float* d_S);
/* mmr_select_with_q (dataset_curator.py:211-238) on the device: d_S [n][n] f32 symmetric, d_q [n] f32,
 * d_order [k] i32; score = alpha q - (1 - alpha) max(0, max over picked S) in f64, greatest first,
 * lowest index on ties. 1 <= k <= n <= 8192. */
int pc_mmr_order(pc_ctx* ctx, const float* d_S, const float* d_q, int n, int k, double alpha, int32_t* d_order);

/* ---- main-pass frame gauges (Processor.run's gray-plane measurements, gui_app.py:5740-8002) ---- */
/* cv2.cvtColor(frame, BGR2GRAY) of every processed frame (gui_app.py:5754; the second one of
 * _is_real_letterbox_crop, gui_app.py:3425, is the same plane) for n frames of any mix of sizes in one
 * launch, with the row and column sums of the plane that detect_black_borders (utils.py:152-196, called at
 * gui_app.py:3370) turns into means. The 14-bit-coefficient arithmetic of pc_face_quality and
 * pc_crop_metrics; none of the latter's resized planes, Laplacian or DCT. The sums are zeroed here. Nothing
 * outside [row, row + 3 w) of a source row is read. n == 0: PC_OK, nothing enqueued. n < 0, a null or
 * misaligned pointer, a side outside [32, PC_GAUGE_MAX_SIDE], row_stride < 3 w, or a gray_pitch that is no
 * multiple of 16 or smaller than w rounded up to 16: PC_ERR_ARG before anything is staged or enqueued,
 * whichever frame of the batch is the bad one. */
int pc_frame_gray(pc_ctx* ctx, const pc_gray_desc* h_descs, int n);
/* Exact 256-bin histograms of n rectangles of gray planes, d_out [n][256] u32 (zeroed here), in one launch:
 * what _is_real_letterbox_crop's _strip_ok (gui_app.py:3429-3447) sorts twice per strip for
 * np.percentile(., 95), np.percentile(., 99) and np.std; the host derives all three from the counts.
 * Rectangles may overlap (the four strips of a frame share its corners); each is counted in full. Row
 * segments move 16 bytes per load where they are aligned, byte by byte in their heads, tails and in strips
 * narrower than that; no byte outside [x, x + w) of a row is read. n == 0: PC_OK, nothing enqueued. n < 0 or
 * > 65535, a null pointer, d_out not 4-byte aligned or a rectangle outside the limits of pc_gray_region:
 * PC_ERR_ARG before anything is staged or enqueued. */
int pc_gray_region_hist(pc_ctx* ctx, const pc_gray_region* h_regions, int n, uint32_t* d_out);
/* cv2.absdiff + cv2.threshold(diff, thresh, 255, THRESH_BINARY) + cv2.countNonZero of _faceless_validate
 * (gui_app.py:4277-4282, thresh 15) for n boxes in one launch: d_counts[i] (u32, zeroed here) = the pixels of
 * box i with |cur - prev| > thresh, strictly. 0 <= thresh <= 255. n == 0: PC_OK, nothing enqueued. n < 0 or
 * > 65535, a null pointer, d_counts not 4-byte aligned, thresh out of range or a box outside the limits of
 * pc_motion_box: PC_ERR_ARG before anything is staged or enqueued. */
int pc_gray_motion(pc_ctx* ctx, const pc_motion_box* h_boxes, int n, int thresh, uint32_t* d_counts);
/* cv2.resize(gray, (ow, oh), INTER_AREA) of one w x h gray plane, the small plane of _smart_crop_box's
 * gradient saliency (gui_app.py:8295-8301): kind PC_CURATE_FAST (integer ratios isx x isy, ow isx <= w,
 * oh isy <= h; tables ignored) or PC_CURATE_AREA (tables as pc_resize_area, every source index checked
 * against w, h), the one-channel arithmetic of pc_crop_metrics' planes. The identity (PC_CURATE_COPY) is
 * the caller's: the plane is its own resize. 1 <= ow <= w, 1 <= oh <= h <= PC_GAUGE_MAX_SIDE, pitch >= w,
 * dst_pitch >= ow; anything else PC_ERR_ARG before anything is staged or enqueued. */
int pc_gray_resize_area(pc_ctx* ctx, const uint8_t* d_gray, int pitch, int w, int h, int kind, int isx, int isy,
                        const pc_area_tab* h_xtab, const int32_t* h_xstart, int n_x, const pc_area_tab* h_ytab,
                        const int32_t* h_ystart, int n_y, uint8_t* d_dst, int dst_pitch, int ow, int oh);

/* ---- host-side align geometry (CPU, batched) ---- */
/* cv::estimateAffinePartial2D(from, to, method=LMEDS) for n point sets of npts points each
 * (h_from [n][npts][2], shared h_to [npts][2]); h_M [n][6] src->dst, h_ok [n] 0/1.
 * Replaces the call at face_embedder.py:1466-1468. */
int pc_estimate_affine_partial(const float* h_from, const float* h_to, int npts, int n, double* h_M, int32_t* h_ok);
/* the inversion cv::warpAffine applies to M (no WARP_INVERSE_MAP) */
int pc_invert_affine(const double* h_M, double* h_iM);

#ifdef __cplusplus
}
#endif
#endif /* PCGPU_H */
