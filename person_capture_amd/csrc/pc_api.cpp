// C-ABI layer (include/pcgpu.h): contexts, host frame staging and the image / detection / embedding
// entry points of the identity hot path. Compiled by hipcc for gfx950. The network executor behind
// pc_net_run is pc_net.cpp; the entry points here that run a net see its internals through pc_net_dev.h.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include <map>
#include <algorithm>
#include <thread>
#include <mutex>
#include <memory>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <system_error>
#include "../../include/pcgpu.h"
#include "pc_net_dev.h"
#include "pc_curate.h"
#include "pc_gauge.h"

namespace pc {
struct LetterboxDesc;
struct WarpDesc;
struct AreaTab;
struct ResizeDesc;
hipError_t resize_linear_launch(const ResizeDesc* d_descs, int N, int max_pixels, hipStream_t s);
hipError_t letterbox_launch(int f32, const LetterboxDesc* d_descs, int N, int D, void* out, hipStream_t s);
hipError_t warp_launch(const WarpDesc* d_descs, int N, int max_pixels, hipStream_t s);
hipError_t quality_launch(const uint8_t* chips, int N, int side, double* out, hipStream_t s);
hipError_t arcprep_launch(int mode, const uint8_t* chips, int N, int side, int flip, void* out, hipStream_t s);
hipError_t rotate_pad_launch(const uint8_t* src, int H, int W, int row_stride, int deg, int pad, uint8_t* dst, int OH,
                             int OW, hipStream_t s);
hipError_t resize_area_fast_launch(const uint8_t* src, int row_stride, int isx, int isy, uint8_t* dst, int OH, int OW,
                                   hipStream_t s);
hipError_t resize_area_launch(const uint8_t* src, int row_stride, const AreaTab* xtab, const int* xstart,
                              const AreaTab* ytab, const int* ystart, uint8_t* dst, int OH, int OW, hipStream_t s);
hipError_t resize_area_rows_launch(const void* jobs, int n, int row_stride, const AreaTab* xtab, const int* xstart,
                                  const AreaTab* ytab, const int* ystart, int OH, int OW, int span_bytes,
                                  hipStream_t s);
hipError_t face_chips_launch(const void* d_jobs, int n, hipStream_t s);
// pc_nv12.hip
hipError_t nv12_to_bgr_launch(const void* d_jobs, int n, long long nwg, hipStream_t s);
hipError_t nv12_resize_area_launch(const void* d_jobs, int n, int y_stride, int uv_stride, const AreaTab* xtab,
                                   const int* xstart, const AreaTab* ytab, const int* ystart, int OH, int OW,
                                   hipStream_t s);
hipError_t nv12_resize_area_fast_launch(const void* d_jobs, int n, int y_stride, int uv_stride, int isx, int isy,
                                        int OH, int OW, hipStream_t s);
// pc_hdr.hip
hipError_t hdr_to_bgr_launch(const void* d_jobs, int n, long long nwg, hipStream_t s);
hipError_t curate_metrics_launch(const void* d_imgs, int n, const void* d_bands, int nbands, const void* d_tabs,
                                 const int* d_starts, const double* d_dct, int max_pixels, hipStream_t s);
hipError_t sim_matrix_launch(const float* F, int n, int dim, float* S, hipStream_t s);
hipError_t mmr_order_launch(const float* S, const float* q, int n, int k, double alpha, int* order, hipStream_t s);
// pc_gauge.hip
hipError_t frame_gray_launch(const void* d_imgs, const void* d_bands, int nbands, int band, hipStream_t s);
hipError_t gauge_region_hist_launch(const void* d_regs, const void* d_jobs, int njobs, hipStream_t s);
hipError_t gauge_motion_launch(const void* d_boxes, const void* d_jobs, int njobs, int thresh, hipStream_t s);
hipError_t gauge_resize_launch(const uint8_t* gray, long long gpitch, int kind, int isx, int isy, const void* xt,
                               const int* xs, const void* yt, const int* ys, uint8_t* dst, long long dpitch, int ow,
                               int oh, hipStream_t s);
hipError_t embed_finalize_launch(const float* e, int ld, int n, int dim, int flip, float* out, hipStream_t s);
hipError_t bank_match_launch(const float* q, int n, const float* bank, int B, int dim, float* fd, int* idx,
                             hipStream_t s);
struct DecodeLevel {
  const float* out;
  int H, W, cs, stride;
  int loc_offset;
  int anchor_offset;
};
struct DecodeParams {
  DecodeLevel lv[3];
  int nlv;
  int total_loc;
  float thresh;
  const float* det_scale;
  float* cand;
  int* count;
  int cap;
};
hipError_t scrfd_decode_launch(const DecodeParams& p, int N, hipStream_t s);
hipError_t scrfd_nms_big_launch(const float* cand, const int* count, int cap, int pcap, unsigned long long* keys,
                                int* slot_of, float* kept, float nms_thresh, int max_det, float* dets, float* kps,
                                int* nkeep, int N, hipStream_t s);
hipError_t scrfd_nms_launch(const float* cand, const int* count, int cap, float nms_thresh, int max_det, float* dets,
                            float* kps, int* nkeep, int N, hipStream_t s);
hipError_t embed_l2_launch(const float* e, int ld, int n, int dim, float eps, float* out, hipStream_t s);
// pc_yolo.hip
struct YoloLetterboxDesc;
hipError_t yolo_letterbox_launch(int f32, const YoloLetterboxDesc* d_descs, int N, int Hp, int Wp, void* out,
                                 hipStream_t s);
struct YoloLevel { const float* out; int H, W, cs, stride; int loc_offset; };
struct YoloDecodeParams { YoloLevel lv[3]; int nlv, total, nc; float conf; float* cand; int* count; int cap; };
struct YoloScale;
hipError_t yolo_decode_launch(const YoloDecodeParams& p, int N, hipStream_t s);
struct YoloKptScale;
hipError_t yolo_nms_big_launch(const float* cand, const int* count, int cap, int pcap, unsigned long long* keys,
                               int* slot_of, float* kept, float iou, int max_det, const YoloScale* sc, float* dets,
                               int* nkeep, int* keep_anchor, int N, hipStream_t s);
hipError_t yolo_kpts_launch(const YoloDecodeParams& p, int nk, int koff, int max_det, const int* nkeep,
                            const int* keep_anchor, const YoloScale* sc, const YoloKptScale* ksc, float* kpts, int N,
                            hipStream_t s);
hipError_t yolo_nms_launch(const float* cand, const int* count, int cap, float iou, int max_det, const YoloScale* sc,
                           float* dets, int* nkeep, int N, hipStream_t s, int* keep_anchor = nullptr);
// pc_clip.hip
struct ClipPrepDesc {
  const uint8_t* src; int H, W, row_stride; int kh, kv;
  const int* hb; const int* hk; const int* vb; const int* vk; int row0, nrows; uint8_t* tmp;
};
hipError_t clip_prep_launch(int mode, const ClipPrepDesc* d_descs, int N, int max_rows, int side, int patch, void* out,
                            hipStream_t s);
}  // namespace pc

using namespace pc;

static_assert(sizeof(pc_letterbox_desc) == 56, "letterbox desc layout");
static_assert(sizeof(pc_warp_desc) == 96, "warp desc layout");
static_assert(sizeof(pc_area_tab) == 12, "area tab layout");
static_assert(sizeof(pc_curate_desc) == 72 && sizeof(pc_curate_record) == 1312, "curate layouts");
static_assert(sizeof(pc_resize_desc) == 80, "resize desc layout");
static_assert(sizeof(pc_chip_desc) == 24, "chip desc layout");
static_assert(sizeof(pc_nv12_desc) == 48, "nv12 desc layout");
static_assert(sizeof(pc_hdr_desc) == 72, "hdr desc layout");
static_assert(sizeof(pc_yolo_letterbox_desc) == 64, "yolo letterbox desc layout");
static_assert(sizeof(pc_yolo_scale) == 20, "yolo scale layout");

// Persistent host workers for pc_frame_stage: a frame is packed into pinned memory in row
// chunks taken in order by the workers, and the caller's thread issues each chunk's H2D as soon
// as it is packed, so the copy engine runs behind the packing instead of after it (r04: the
// 6.2 MB of a 1080p frame cost ~0.3 ms of packing with per-call threads, then the H2D).
// One frame's packing job: chunks are taken from `next`; done[c] and active are guarded by the pool's
// mutex. A job lives until its last holder drops it; the caller waits for active == 0 before its
// frame (which the job's function refers to) goes out of scope.
struct StageJob {
  std::function<void(int)> fn;
  int nchunks = 0;
  std::atomic<int> next{0};
  std::vector<char> done;
  int active = 0;                    // workers inside fn
};

// Persistent packing workers of pc_frame_stage. A worker takes the current job under the lock (a
// snapshot: the job's function, chunk count and counters belong to that frame alone), works it
// without the lock, and never sees another frame's job in between - a late wake-up finds either no
// job or the next frame's, whose state is its own object (the shared job / nchunks
// fields were re-assigned while a late worker still read them).
struct StagePool {
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;        // workers: a new job
  std::condition_variable done_cv;   // caller: a chunk finished / a worker left the job
  std::shared_ptr<StageJob> cur;     // the frame being packed (guarded by mu)
  unsigned gen = 0;                  // bumped per job (guarded by mu)
  bool stop = false;
  void start(int n) {
    for (int i = 0; i < n; ++i) {
      try {
        th.emplace_back([this] { loop(); });
      } catch (const std::system_error&) {
        break;   // fewer workers: the caller packs what nobody takes
      }
    }
  }
  void loop() {
    unsigned seen = 0;
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv.wait(lk, [&] { return stop || (cur && gen != seen); });
      if (stop) return;
      seen = gen;
      std::shared_ptr<StageJob> j = cur;
      ++j->active;
      lk.unlock();
      work(*j);
      lk.lock();
      --j->active;
      done_cv.notify_all();
    }
  }
  // take chunks of job j until none is left (the caller runs this too)
  void work(StageJob& j) {
    for (int c; (c = j.next.fetch_add(1)) < j.nchunks;) {
      j.fn(c);
      std::lock_guard<std::mutex> g(mu);
      j.done[c] = 1;
      done_cv.notify_all();
    }
  }
  ~StagePool() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
};

static int stage_copy(pc_ctx* c, const void* h, size_t nbytes, void** d_out) {
  const size_t bytes = (nbytes + 255) & ~size_t(255);
  if (bytes > c->stage_cap) {
    // grow the ring (rare: thousands of descriptors in one call); everything staged so
    // far must have been consumed before the old buffers go
    HIPCHK(c, hipStreamSynchronize(c->stream));
    size_t cap = c->stage_cap;
    while (cap < bytes) cap *= 2;
    char *h = nullptr, *d = nullptr;
    if (hipHostMalloc((void**)&h, cap, hipHostMallocDefault) != hipSuccess) return fail(c, PC_ERR_HIP, "staging grow");
    if (hipMalloc((void**)&d, cap) != hipSuccess) { hipHostFree(h); return fail(c, PC_ERR_HIP, "staging grow"); }
    hipHostFree(c->stage_h);
    hipFree(c->stage_d);
    c->stage_h = h; c->stage_d = d; c->stage_cap = cap; c->stage_off = 0;
  }
  if (c->stage_off + bytes > c->stage_cap) {
    // wrap: everything previously staged must have been consumed
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_off = 0;
  }
  memcpy(c->stage_h + c->stage_off, h, nbytes);
  HIPCHK(c, hipMemcpyAsync(c->stage_d + c->stage_off, c->stage_h + c->stage_off, nbytes, hipMemcpyHostToDevice,
                           c->stream));
  *d_out = c->stage_d + c->stage_off;
  c->stage_off += bytes;
  return PC_OK;
}

extern "C" int pc_abi_version(void) { return PC_ABI_VERSION; }

extern "C" int pc_ctx_create(int device_id, pc_ctx** out) {
  if (!out) return PC_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PC_ERR_HIP;
  if (device_id < 0 || device_id >= ndev) return PC_ERR_ARG;
  pc_ctx* c = new pc_ctx();
  c->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess) { delete c; return PC_ERR_HIP; }
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return PC_ERR_HIP; }
  c->stream = c->own_stream;
  if (hipMalloc(&c->zero, 4096) != hipSuccess || hipMemset(c->zero, 0, 4096) != hipSuccess) { delete c; return PC_ERR_HIP; }
  c->stage_cap = 8u << 20;
  if (hipHostMalloc((void**)&c->stage_h, c->stage_cap, hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&c->stage_d, c->stage_cap) != hipSuccess) {
    delete c;
    return PC_ERR_HIP;
  }
  // the context's one tuning switch, read here once (A/B: the per-pixel INTER_AREA kernel)
  c->area_direct = getenv("PC_AREA_DIRECT") && atoi(getenv("PC_AREA_DIRECT")) != 0;
  *out = c;
  return PC_OK;
}

extern "C" int pc_ctx_destroy(pc_ctx* c) {
  if (!c) return PC_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->zero) hipFree(c->zero);
  if (c->stage_h) hipHostFree(c->stage_h);
  if (c->stage_d) hipFree(c->stage_d);
  if (c->cand) hipFree(c->cand);
  if (c->cand_count) hipFree(c->cand_count);
  if (c->nms_big) hipFree(c->nms_big);
  if (c->det_scale) hipFree(c->det_scale);
  if (c->ycand) hipFree(c->ycand);
  if (c->ykeep) hipFree(c->ykeep);
  if (c->ybig) hipFree(c->ybig);
  if (c->ycount) hipFree(c->ycount);
  if (c->clip_tmp) hipFree(c->clip_tmp);
  delete c->pool;
  for (auto& fs : c->fslots) {
    if (fs.h) hipHostFree(fs.h);
    if (fs.ev) hipEventDestroy(fs.ev);
  }
  if (c->own_stream) hipStreamDestroy(c->own_stream);
  delete c;
  return PC_OK;
}

extern "C" const char* pc_last_error(const pc_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" int pc_ctx_set_stream(pc_ctx* c, void* s) {
  if (!c) return PC_ERR_ARG;
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return PC_OK;
}
extern "C" void* pc_ctx_stream(pc_ctx* c) { return c ? (void*)c->stream : nullptr; }
// Re-create the context-owned stream at a scheduling priority (HIP convention: lower =
// higher priority; clamped to hipDeviceGetStreamPriorityRange). Work already queued on the
// old stream is drained first.
extern "C" int pc_ctx_set_priority(pc_ctx* c, int priority) {
  if (!c) return PC_ERR_ARG;
  int least = 0, greatest = 0;
  HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
  const int p = priority < greatest ? greatest : (priority > least ? least : priority);
  hipStream_t s = nullptr;
  HIPCHK(c, hipStreamCreateWithPriority(&s, hipStreamNonBlocking, p));
  HIPCHK(c, hipStreamSynchronize(c->own_stream));
  const bool own = c->stream == c->own_stream;
  hipStreamDestroy(c->own_stream);
  c->own_stream = s;
  if (own) c->stream = s;
  return PC_OK;
}
extern "C" int pc_ctx_sync(pc_ctx* c) {
  if (!c) return PC_ERR_ARG;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return PC_OK;
}
extern "C" int pc_device_alloc(pc_ctx* c, size_t bytes, void** d) {
  if (!c || !d) return PC_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(d, bytes ? bytes : 16));
  return PC_OK;
}
extern "C" int pc_device_free(pc_ctx* c, void* d) {
  if (!c) return PC_ERR_ARG;
  if (d) HIPCHK(c, hipFree(d));
  return PC_OK;
}
extern "C" int pc_host_alloc(pc_ctx* c, size_t bytes, void** h) {
  if (!c || !h) return PC_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipHostMalloc(h, bytes ? bytes : 16, hipHostMallocDefault));
  return PC_OK;
}
extern "C" int pc_host_free(pc_ctx* c, void* h) {
  if (!c) return PC_ERR_ARG;
  if (h) HIPCHK(c, hipHostFree(h));
  return PC_OK;
}
extern "C" int pc_fence_create(pc_ctx* c, void** f) {
  if (!c || !f) return PC_ERR_ARG;
  hipEvent_t e = nullptr;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *f = (void*)e;
  return PC_OK;
}
extern "C" int pc_fence_record(pc_ctx* c, void* f) {
  if (!c || !f) return PC_ERR_ARG;
  HIPCHK(c, hipEventRecord((hipEvent_t)f, c->stream));
  return PC_OK;
}
extern "C" int pc_fence_wait(pc_ctx* c, void* f) {
  if (!c || !f) return PC_ERR_ARG;
  HIPCHK(c, hipEventSynchronize((hipEvent_t)f));
  return PC_OK;
}
extern "C" int pc_fence_destroy(pc_ctx* c, void* f) {
  if (!c) return PC_ERR_ARG;
  if (f) HIPCHK(c, hipEventDestroy((hipEvent_t)f));
  return PC_OK;
}
extern "C" int pc_ctx_wait_fence(pc_ctx* c, void* f) {
  if (!c || !f) return PC_ERR_ARG;
  HIPCHK(c, hipStreamWaitEvent(c->stream, (hipEvent_t)f, 0));
  return PC_OK;
}

// Host frame -> device through the context's ring of pinned slots: the rows (row_bytes each,
// src_stride apart: a numpy slice need not be contiguous) are packed into the slot by up to
// `threads` host threads, then one H2D from the slot is enqueued on the context stream. The
// caller's array is free again when this returns; the device copy completes in stream order.
// A pageable hipMemcpyAsync would stage through the runtime's own bounce buffers in
// ~MB-sized pieces with the calling thread blocked for the whole transfer.
extern "C" int pc_frame_stage(pc_ctx* c, void* d_dst, const void* h_src, size_t row_bytes, size_t rows,
                              size_t src_stride, int threads) {
  if (!c || !d_dst || !h_src || src_stride < row_bytes) return PC_ERR_ARG;
  const size_t n = row_bytes * rows;
  if (!n) return PC_OK;
  std::lock_guard<std::mutex> lock(c->fslot_mu);   // the slot ring and its stream order
  auto& fs = c->fslots[c->fslot_next];
  c->fslot_next = (c->fslot_next + 1) % 4;
  if (fs.pending) HIPCHK(c, hipEventSynchronize(fs.ev));
  fs.pending = false;
  if (fs.cap < n) {
    if (fs.h) hipHostFree(fs.h);
    fs.h = nullptr;
    fs.cap = 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipHostMalloc((void**)&fs.h, n, hipHostMallocDefault));
    fs.cap = n;
  }
  if (!fs.ev) HIPCHK(c, hipEventCreateWithFlags(&fs.ev, hipEventDisableTiming));
  const char* src = (const char*)h_src;
  auto pack = [&](size_t r0, size_t r1) {
    if (src_stride == row_bytes) {
      memcpy(fs.h + r0 * row_bytes, src + r0 * row_bytes, (r1 - r0) * row_bytes);
    } else {
      for (size_t r = r0; r < r1; ++r) memcpy(fs.h + r * row_bytes, src + r * src_stride, row_bytes);
    }
  };
  int nt = std::max(1, std::min(threads, 16));
  if (n < (size_t(2) << 20)) nt = 1;   // below ~2 MB the handoff costs more than it saves
  if (nt == 1) {
    pack(0, rows);
    HIPCHK(c, hipMemcpyAsync(d_dst, fs.h, n, hipMemcpyHostToDevice, c->stream));
  } else {
    if (!c->pool) {
      c->pool = new StagePool();
      c->pool->start(nt - 1);
    }
    StagePool& P = *c->pool;
    // ~512 KB chunks: the first H2D starts after one chunk, the last follows the last pack
    const int nch = (int)std::min<size_t>(64, std::max<size_t>(nt, (n + (512u << 10) - 1) / (512u << 10)));
    const size_t per = (rows + nch - 1) / nch;
    auto job = std::make_shared<StageJob>();
    job->fn = [&](int ch) { pack(std::min(rows, ch * per), std::min(rows, (ch + 1) * per)); };
    job->nchunks = nch;
    job->done.assign(nch, 0);
    {
      std::lock_guard<std::mutex> g(P.mu);
      P.cur = job;
      ++P.gen;
    }
    P.cv.notify_all();
    // issue each chunk's copy in order as soon as it is packed; pack the rest here when the
    // workers are behind (the copies of chunk i overlap the packing of chunks > i)
    hipError_t herr = hipSuccess;
    for (int ch = 0; ch < nch; ++ch) {
      for (;;) {
        {
          std::unique_lock<std::mutex> lk(P.mu);
          if (job->done[ch]) break;
          if (job->next.load() >= nch) {   // everything taken: wait for chunk ch
            P.done_cv.wait(lk, [&] { return job->done[ch] != 0; });
            break;
          }
        }
        const int mine = job->next.fetch_add(1);
        if (mine < nch) {
          job->fn(mine);
          std::lock_guard<std::mutex> g(P.mu);
          job->done[mine] = 1;
        }
      }
      const size_t r0 = std::min(rows, ch * per), r1 = std::min(rows, (ch + 1) * per);
      if (r1 > r0 && herr == hipSuccess)
        herr = hipMemcpyAsync((char*)d_dst + r0 * row_bytes, fs.h + r0 * row_bytes, (r1 - r0) * row_bytes,
                              hipMemcpyHostToDevice, c->stream);
    }
    {   // the job's function refers to this frame: no worker may still be inside it, and none may
        // pick it up later (it stops being the current job)
      std::unique_lock<std::mutex> lk(P.mu);
      P.done_cv.wait(lk, [&] { return job->active == 0; });
      P.cur.reset();
    }
    if (herr != hipSuccess) return fail(c, PC_ERR_HIP, std::string("frame_stage H2D: ") + hipGetErrorString(herr));
  }
  HIPCHK(c, hipEventRecord(fs.ev, c->stream));
  fs.pending = true;
  return PC_OK;
}

extern "C" int pc_copy_h2d(pc_ctx* c, void* d, const void* h, size_t n) {
  if (!c) return PC_ERR_ARG;
  if (n) HIPCHK(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  return PC_OK;
}
extern "C" int pc_copy_d2h(pc_ctx* c, void* h, const void* d, size_t n) {
  if (!c) return PC_ERR_ARG;
  if (n) HIPCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream));
  return PC_OK;
}
extern "C" int pc_copy_d2d(pc_ctx* c, void* d, const void* s, size_t n) {
  if (!c) return PC_ERR_ARG;
  if (n) HIPCHK(c, hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, c->stream));
  return PC_OK;
}
extern "C" int pc_copy_2d(pc_ctx* c, void* d_dst, size_t dst_pitch, const void* d_src, size_t src_pitch,
                          size_t width_bytes, size_t rows) {
  if (!c || !d_dst || !d_src || width_bytes > dst_pitch || width_bytes > src_pitch)
    return fail(c, PC_ERR_ARG, "pc_copy_2d: bad arguments");
  if (!width_bytes || !rows) return PC_OK;
  HIPCHK(c, hipMemcpy2DAsync(d_dst, dst_pitch, d_src, src_pitch, width_bytes, rows, hipMemcpyDeviceToDevice,
                             c->stream));
  return PC_OK;
}

extern "C" int pc_memset(pc_ctx* c, void* d, int v, size_t n) {
  if (!c) return PC_ERR_ARG;
  if (n) HIPCHK(c, hipMemsetAsync(d, v, n, c->stream));
  return PC_OK;
}

// ===========================================================================
// image / detection / embedding entry points
// ===========================================================================
extern "C" int pc_letterbox(pc_ctx* c, int prec, const pc_letterbox_desc* h, int n, int D, void* d_out) {
  if (!c || !h || n <= 0 || D <= 0 || !d_out) return fail(c, PC_ERR_ARG, "pc_letterbox: bad arguments");
  void* dd;
  int rc = stage_copy(c, h, sizeof(pc_letterbox_desc) * n, &dd);
  if (rc) return rc;
  HIPCHK(c, letterbox_launch(prec == PC_PREC_F32, (const LetterboxDesc*)dd, n, D, d_out, c->stream));
  return PC_OK;
}

extern "C" int pc_resize_linear(pc_ctx* c, const pc_resize_desc* h, int n) {
  if (!c || !h || n < 0) return fail(c, PC_ERR_ARG, "pc_resize_linear: bad arguments");
  if (n == 0) return PC_OK;
  int maxpix = 0;
  for (int i = 0; i < n; ++i) maxpix = std::max(maxpix, h[i].new_w * h[i].new_h);
  void* dd;
  int rc = stage_copy(c, h, sizeof(pc_resize_desc) * n, &dd);
  if (rc) return rc;
  HIPCHK(c, resize_linear_launch((const ResizeDesc*)dd, n, maxpix, c->stream));
  return PC_OK;
}

extern "C" int pc_warp_affine(pc_ctx* c, const pc_warp_desc* h, int n) {
  if (!c || !h || n < 0) return fail(c, PC_ERR_ARG, "pc_warp_affine: bad arguments");
  if (n == 0) return PC_OK;
  int maxpix = 0;
  for (int i = 0; i < n; ++i) maxpix = std::max(maxpix, h[i].out_w * h[i].out_h);
  void* dd;
  int rc = stage_copy(c, h, sizeof(pc_warp_desc) * n, &dd);
  if (rc) return rc;
  HIPCHK(c, warp_launch((const WarpDesc*)dd, n, maxpix, c->stream));
  return PC_OK;
}

extern "C" int pc_face_quality(pc_ctx* c, const uint8_t* chips, int n, int side, double* out) {
  if (!c || n < 0 || side <= 0 || side > 128) return fail(c, PC_ERR_ARG, "pc_face_quality: bad arguments");
  if (n == 0) return PC_OK;
  HIPCHK(c, quality_launch(chips, n, side, out, c->stream));
  return PC_OK;
}

extern "C" int pc_arcface_prep(pc_ctx* c, int prec, const uint8_t* chips, int n, int side, int flip, void* out) {
  if (!c || n < 0) return fail(c, PC_ERR_ARG, "pc_arcface_prep: bad arguments");
  if (n == 0) return PC_OK;
  if (prec != PC_PREC_F16 && prec != PC_PREC_F32 && prec != PC_PREC_F16X3)
    return fail(c, PC_ERR_ARG, "pc_arcface_prep: bad precision");
  HIPCHK(c, arcprep_launch(prec, chips, n, side, flip, out, c->stream));
  return PC_OK;
}

extern "C" int pc_rotate_pad(pc_ctx* c, const uint8_t* src, int H, int W, int row_stride, int deg, int pad,
                             uint8_t* dst) {
  if (!c || !src || !dst || H <= 0 || W <= 0 || pad < 0 || (deg != 0 && deg != 90 && deg != 180 && deg != 270))
    return fail(c, PC_ERR_ARG, "pc_rotate_pad: bad arguments");
  const int RH = (deg == 90 || deg == 270) ? W : H;
  const int RW = (deg == 90 || deg == 270) ? H : W;
  HIPCHK(c, rotate_pad_launch(src, H, W, row_stride, deg, pad, dst, RH + 2 * pad, RW + 2 * pad, c->stream));
  return PC_OK;
}

extern "C" int pc_resize_area_batch(pc_ctx* c, const uint8_t* const* srcs, uint8_t* const* dsts, int n, int row_stride,
                                    const pc_area_tab* xt, const int32_t* xs, int n_x, const pc_area_tab* yt,
                                    const int32_t* ys, int n_y, int OH, int OW);

extern "C" int pc_resize_area(pc_ctx* c, const uint8_t* src, int row_stride, const pc_area_tab* xt,
                              const int32_t* xs, int n_x, const pc_area_tab* yt, const int32_t* ys, int n_y,
                              uint8_t* dst, int OH, int OW) {
  if (!c || !src || !dst || !xt || !xs || !yt || !ys) return fail(c, PC_ERR_ARG, "pc_resize_area: bad arguments");
  return pc_resize_area_batch(c, &src, &dst, 1, row_stride, xt, xs, n_x, yt, ys, n_y, OH, OW);
}

// LDS span of resize_area_rows_u8: the widest 256-pixel output group's source bytes from a 16-byte
// boundary to one past its last byte rounded up to 16
static int area_span_bytes(const pc_area_tab* xt, const int32_t* xs, int OW) {
  int m = 0;
  for (int x0 = 0; x0 < OW; x0 += 256) {
    const int xl = std::min(x0 + 255, OW - 1);
    const int c0 = xt[xs[x0]].si, c1 = xt[xs[xl + 1] - 1].si;
    m = std::max(m, ((c1 * 3 + 3 + 15) & ~15) - ((c0 * 3) & ~15));
  }
  return m;
}

extern "C" int pc_resize_area_batch(pc_ctx* c, const uint8_t* const* srcs, uint8_t* const* dsts, int n, int row_stride,
                                    const pc_area_tab* xt, const int32_t* xs, int n_x, const pc_area_tab* yt,
                                    const int32_t* ys, int n_y, int OH, int OW) {
  if (!c || !srcs || !dsts || !xt || !xs || !yt || !ys || n < 0 || OH <= 0 || OW <= 0 || n_x <= 0 || n_y <= 0)
    return fail(c, PC_ERR_ARG, "pc_resize_area_batch: bad arguments");
  if (n == 0) return PC_OK;
  bool aligned = row_stride % 16 == 0;
  for (int i = 0; i < n; ++i) {
    if (!srcs[i] || !dsts[i]) return fail(c, PC_ERR_ARG, "pc_resize_area_batch: null frame");
    aligned = aligned && ((uintptr_t)srcs[i] & 15) == 0;
  }
  const int span = area_span_bytes(xt, xs, OW);
  void *dxt, *dxs, *dyt, *dys;
  int rc;
  if ((rc = stage_copy(c, xt, sizeof(pc_area_tab) * n_x, &dxt))) return rc;
  if ((rc = stage_copy(c, xs, sizeof(int32_t) * (OW + 1), &dxs))) return rc;
  if ((rc = stage_copy(c, yt, sizeof(pc_area_tab) * n_y, &dyt))) return rc;
  if ((rc = stage_copy(c, ys, sizeof(int32_t) * (OH + 1), &dys))) return rc;
  if (aligned && span <= 8192 && !c->area_direct) {   // (pc_image.hip AREA_ROWB: 4K -> 416 spans ~7.1 KB)
    std::vector<const void*> jobs(2 * (size_t)n);
    for (int i = 0; i < n; ++i) { jobs[2 * i] = srcs[i]; jobs[2 * i + 1] = dsts[i]; }
    void* dj;
    if ((rc = stage_copy(c, jobs.data(), sizeof(void*) * jobs.size(), &dj))) return rc;
    HIPCHK(c, resize_area_rows_launch(dj, n, row_stride, (const AreaTab*)dxt, (const int*)dxs, (const AreaTab*)dyt,
                                      (const int*)dys, OH, OW, span, c->stream));
    return PC_OK;
  }
  for (int i = 0; i < n; ++i)   // unaligned frames: the per-pixel kernel
    HIPCHK(c, resize_area_launch(srcs[i], row_stride, (const AreaTab*)dxt, (const int*)dxs, (const AreaTab*)dyt,
                                 (const int*)dys, dsts[i], OH, OW, c->stream));
  return PC_OK;
}

extern "C" int pc_resize_area_fast(pc_ctx* c, const uint8_t* src, int row_stride, int isx, int isy, uint8_t* dst,
                                   int OH, int OW) {
  if (!c || !src || !dst || isx < 1 || isy < 1 || OH <= 0 || OW <= 0)
    return fail(c, PC_ERR_ARG, "pc_resize_area_fast: bad arguments");
  HIPCHK(c, resize_area_fast_launch(src, row_stride, isx, isy, dst, OH, OW, c->stream));
  return PC_OK;
}

// ---- face chips of the OpenCLIP face mode ----
// cv::resize's dispatch (OpenCV 4.9 imgproc/src/resize.cpp: cv::resize then hal::resize) for H x W -> 112 x 112,
// INTER_AREA if max(H, W) > 112 else INTER_LINEAR; imageops.resize_plan states the same for any target.
struct ChipPlan { int kind, isx, isy, area_mode; double inv_x, inv_y, scale_x, scale_y; };

static ChipPlan chip_plan(int H, int W) {
  ChipPlan p{};
  p.inv_x = (double)PC_CHIP_SIDE / W;
  p.inv_y = (double)PC_CHIP_SIDE / H;
  p.scale_x = 1.0 / p.inv_x;   // (not W / 112: they can differ in the last bit)
  p.scale_y = 1.0 / p.inv_y;
  p.isx = (int)std::nearbyint(p.scale_x);   // cvRound
  p.isy = (int)std::nearbyint(p.scale_y);
  if (H == PC_CHIP_SIDE && W == PC_CHIP_SIDE) { p.kind = PC_CHIP_COPY; return p; }
  bool area = std::max(H, W) > PC_CHIP_SIDE;
  const double eps = 2.220446049250313e-16;
  const bool fast = std::fabs(p.scale_x - p.isx) < eps && std::fabs(p.scale_y - p.isy) < eps &&
                    W == p.isx * PC_CHIP_SIDE && H == p.isy * PC_CHIP_SIDE;
  if (!area && fast && p.isx == 2 && p.isy == 2) area = true;   // (INTER_LINEAR at exactly 2 x 2 down)
  if (area && p.scale_x >= 1 && p.scale_y >= 1) {
    p.kind = fast ? PC_CHIP_AREA_FAST : PC_CHIP_AREA;
  } else {
    p.kind = PC_CHIP_LINEAR;
    p.area_mode = area ? 1 : 0;
  }
  return p;
}

static bool chip_size_ok(int H, int W) { return H >= 1 && W >= 1 && H <= PC_CHIP_MAX_SIDE && W <= PC_CHIP_MAX_SIDE; }

extern "C" int pc_face_chip_plan(int H, int W, int32_t* out4) {
  if (!out4 || !chip_size_ok(H, W)) return PC_ERR_ARG;
  const ChipPlan p = chip_plan(H, W);
  out4[0] = p.kind; out4[1] = p.isx; out4[2] = p.isy; out4[3] = p.area_mode;
  return PC_OK;
}

// OpenCV's 128-bit VResizeLinearVec_32s8u stops here in a row of 112 x 3 bytes (the 16-byte loop, then 8-byte
// steps while x < width - 8; engines.opencv_vresize_simd_end)
static int chip_simd_end() {
  const int wb = PC_CHIP_SIDE * 3;
  int x = wb / 16 * 16;
  while (x < wb - 8) x += 8;
  return x;
}

extern "C" int pc_face_chips(pc_ctx* c, const pc_chip_desc* h, int n, uint8_t* d_chips) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || (n > 0 && (!h || !d_chips))) return fail(c, PC_ERR_ARG, "pc_face_chips: bad arguments");
  if (n == 0) return PC_OK;
  struct Job { pc_resize_desc r; int32_t kind, isx, isy, pad_; };   // pc_image.hip ChipJob
  static_assert(sizeof(Job) == 96, "chip job layout");
  std::vector<Job> jobs((size_t)n);
  const int simd_end = chip_simd_end();
  for (int i = 0; i < n; ++i) {
    const pc_chip_desc& d = h[i];
    if (!d.d_src || !chip_size_ok(d.H, d.W) || (long long)d.row_stride < 3LL * d.W)
      return fail(c, PC_ERR_ARG, "pc_face_chips: bad rectangle (non-null, 1 <= H, W <= 16384, row_stride >= 3 W)");
    const ChipPlan p = chip_plan(d.H, d.W);
    Job& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.r.d_src = d.d_src; j.r.H = d.H; j.r.W = d.W; j.r.row_stride = d.row_stride;
    j.r.new_w = j.r.new_h = PC_CHIP_SIDE;
    j.r.scale_x = p.scale_x; j.r.scale_y = p.scale_y; j.r.inv_x = p.inv_x; j.r.inv_y = p.inv_y;
    j.r.simd_end = simd_end; j.r.area_mode = p.area_mode;
    j.r.d_dst = d_chips + (size_t)i * PC_CHIP_SIDE * PC_CHIP_SIDE * 3;
    j.kind = p.kind; j.isx = p.isx; j.isy = p.isy;
  }
  void* dj;
  int rc = stage_copy(c, jobs.data(), sizeof(Job) * (size_t)n, &dj);
  if (rc) return rc;
  HIPCHK(c, face_chips_launch(dj, n, c->stream));
  return PC_OK;
}

// ---- NV12 frames (pc_nv12.hip) ----
static bool nv12_size_ok(int H, int W) {
  return H >= 2 && W >= 2 && H <= PC_NV12_MAX_SIDE && W <= PC_NV12_MAX_SIDE && !(H & 1) && !(W & 1);
}

extern "C" int pc_nv12_to_bgr(pc_ctx* c, const pc_nv12_desc* h, int n) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || (n > 0 && !h)) return fail(c, PC_ERR_ARG, "pc_nv12_to_bgr: bad arguments");
  if (n == 0) return PC_OK;
  struct Job {   // pc_nv12.hip Nv12Job
    const uint8_t *y, *uv; uint8_t* dst;
    int32_t H, W, y_stride, uv_stride, dst_stride, aligned, ux, wg0;
  };
  static_assert(sizeof(Job) == 56, "nv12 job layout");
  std::vector<Job> jobs((size_t)n);
  long long nwg = 0;
  for (int i = 0; i < n; ++i) {
    const pc_nv12_desc& d = h[i];
    if (!d.d_y || !d.d_uv || !d.d_dst || !nv12_size_ok(d.H, d.W) || d.y_stride < d.W || d.uv_stride < d.W ||
        (long long)d.dst_stride < 3LL * d.W)
      return fail(c, PC_ERR_ARG, "pc_nv12_to_bgr: bad frame (non-null planes, even 2 <= H, W <= 16384, y_stride >= W, "
                                 "uv_stride >= W, dst_stride >= 3 W)");
    Job& j = jobs[i];
    j.y = d.d_y; j.uv = d.d_uv; j.dst = d.d_dst;
    j.H = d.H; j.W = d.W; j.y_stride = d.y_stride; j.uv_stride = d.uv_stride; j.dst_stride = d.dst_stride;
    j.aligned = (((uintptr_t)d.d_y | (uintptr_t)d.d_uv | (uintptr_t)d.d_dst | (uintptr_t)d.y_stride |
                  (uintptr_t)d.uv_stride | (uintptr_t)d.dst_stride) & 15) == 0;
    j.ux = (d.W + 15) / 16;
    if (nwg >= (1LL << 31)) return fail(c, PC_ERR_ARG, "pc_nv12_to_bgr: too many pixels for one launch");
    j.wg0 = (int32_t)nwg;
    nwg += ((long long)j.ux * (d.H / 2) + 255) / 256;
  }
  if (nwg >= (1LL << 31)) return fail(c, PC_ERR_ARG, "pc_nv12_to_bgr: too many pixels for one launch");
  void* dj;
  int rc = stage_copy(c, jobs.data(), sizeof(Job) * (size_t)n, &dj);
  if (rc) return rc;
  HIPCHK(c, nv12_to_bgr_launch(dj, n, nwg, c->stream));
  return PC_OK;
}

// ---- HDR linear-light frames (pc_hdr.hip) ----
extern "C" int pc_hdr_to_bgr(pc_ctx* c, const pc_hdr_desc* h, int n) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || (n > 0 && !h)) return fail(c, PC_ERR_ARG, "pc_hdr_to_bgr: bad arguments");
  if (n == 0) return PC_OK;
  struct Job {   // pc_hdr.hip HdrJob
    const float *r, *g, *b; uint8_t* dst;
    int32_t H, W, pix_stride, row_stride, dst_stride, transfer;
    float t32, peak;
    int32_t wide, ux, wg0, pad_;
  };
  static_assert(sizeof(Job) == 80, "hdr job layout");
  std::vector<Job> jobs((size_t)n);
  long long nwg = 0;
  for (int i = 0; i < n; ++i) {
    const pc_hdr_desc& d = h[i];
    const uintptr_t src = (uintptr_t)d.d_r | (uintptr_t)d.d_g | (uintptr_t)d.d_b;
    if (!d.d_r || !d.d_g || !d.d_b || !d.d_dst || (src & 3) || d.H < 1 || d.W < 1 || d.H > PC_HDR_MAX_SIDE ||
        d.W > PC_HDR_MAX_SIDE || (d.pix_stride != 1 && d.pix_stride != 3) ||
        (long long)d.row_stride < (long long)d.W * d.pix_stride || (long long)d.dst_stride < 3LL * d.W ||
        d.transfer < PC_HDR_PQ || d.transfer > PC_HDR_LINEAR || !std::isfinite(d.target_nits) ||
        !std::isfinite(d.peak_nits) || d.target_nits <= 0 || d.peak_nits <= 0)
      return fail(c, PC_ERR_ARG, "pc_hdr_to_bgr: bad frame (non-null 4-byte aligned samples, 1 <= H, W <= 16384, "
                                 "pix_stride 1 or 3, row_stride >= W pix_stride, dst_stride >= 3 W, a known "
                                 "transfer, finite target_nits and peak_nits > 0)");
    Job& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.r = d.d_r; j.g = d.d_g; j.b = d.d_b; j.dst = d.d_dst;
    j.H = d.H; j.W = d.W; j.pix_stride = d.pix_stride; j.row_stride = d.row_stride; j.dst_stride = d.dst_stride;
    j.transfer = d.transfer;
    j.t32 = (float)d.target_nits;
    j.peak = (float)std::max(d.peak_nits, 1e-3);
    // 16-byte loads: planes each aligned, or one interleaved R, G, B triple sequence from an aligned d_r
    const bool src16 = d.pix_stride == 1 ? (src & 15) == 0
                                         : (((uintptr_t)d.d_r & 15) == 0 && d.d_g == d.d_r + 1 && d.d_b == d.d_r + 2);
    j.wide = src16 && (((size_t)d.row_stride * 4) & 15) == 0 &&
             (((uintptr_t)d.d_dst | (uintptr_t)d.dst_stride) & 3) == 0;
    j.ux = (d.W + 3) / 4;
    if (nwg >= (1LL << 31)) return fail(c, PC_ERR_ARG, "pc_hdr_to_bgr: too many pixels for one launch");
    j.wg0 = (int32_t)nwg;
    nwg += ((long long)j.ux * d.H + 255) / 256;
  }
  if (nwg >= (1LL << 31)) return fail(c, PC_ERR_ARG, "pc_hdr_to_bgr: too many pixels for one launch");
  void* dj;
  int rc = stage_copy(c, jobs.data(), sizeof(Job) * (size_t)n, &dj);
  if (rc) return rc;
  HIPCHK(c, hdr_to_bgr_launch(dj, n, nwg, c->stream));
  return PC_OK;
}

// the frames of a fused downscale: n triples (Y, UV, destination) staged for the kernels
static int nv12_area_jobs(pc_ctx* c, const char* what, const uint8_t* const* ys, const uint8_t* const* uvs,
                          uint8_t* const* dsts, int n, int H, int W, int y_stride, int uv_stride,
                          std::vector<const void*>& jobs) {
  if (!ys || !uvs || !dsts || n < 0 || n > 65535 || !nv12_size_ok(H, W) || y_stride < W || uv_stride < W)
    return fail(c, PC_ERR_ARG, std::string(what) + ": bad arguments");
  jobs.resize(3 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    if (!ys[i] || !uvs[i] || !dsts[i]) return fail(c, PC_ERR_ARG, std::string(what) + ": null frame");
    jobs[3 * i] = ys[i]; jobs[3 * i + 1] = uvs[i]; jobs[3 * i + 2] = dsts[i];
  }
  return PC_OK;
}

// every coefficient of an INTER_AREA table inside [0, ssize) and every destination's window inside the table
static bool area_table_ok(const pc_area_tab* t, int n_t, const int32_t* start, int dsize, int ssize) {
  for (int i = 0; i < n_t; ++i)
    if (t[i].si < 0 || t[i].si >= ssize) return false;
  if (start[0] < 0 || start[dsize] > n_t) return false;
  for (int d = 0; d < dsize; ++d)
    if (start[d] > start[d + 1]) return false;
  return true;
}

extern "C" int pc_nv12_resize_area_batch(pc_ctx* c, const uint8_t* const* ys, const uint8_t* const* uvs,
                                         uint8_t* const* dsts, int n, int H, int W, int y_stride, int uv_stride,
                                         const pc_area_tab* xt, const int32_t* xs, int n_x, const pc_area_tab* yt,
                                         const int32_t* ysr, int n_y, int OH, int OW) {
  if (!c) return PC_ERR_ARG;
  std::vector<const void*> jobs;
  int rc = nv12_area_jobs(c, "pc_nv12_resize_area_batch", ys, uvs, dsts, n, H, W, y_stride, uv_stride, jobs);
  if (rc) return rc;
  if (!xt || !xs || !yt || !ysr || n_x <= 0 || n_y <= 0 || OH <= 0 || OW <= 0 || OH > H || OW > W ||
      !area_table_ok(xt, n_x, xs, OW, W) || !area_table_ok(yt, n_y, ysr, OH, H))
    return fail(c, PC_ERR_ARG, "pc_nv12_resize_area_batch: bad tables");
  if (n == 0) return PC_OK;
  void *dxt, *dxs, *dyt, *dys, *dj;
  if ((rc = stage_copy(c, xt, sizeof(pc_area_tab) * n_x, &dxt))) return rc;
  if ((rc = stage_copy(c, xs, sizeof(int32_t) * (OW + 1), &dxs))) return rc;
  if ((rc = stage_copy(c, yt, sizeof(pc_area_tab) * n_y, &dyt))) return rc;
  if ((rc = stage_copy(c, ysr, sizeof(int32_t) * (OH + 1), &dys))) return rc;
  if ((rc = stage_copy(c, jobs.data(), sizeof(void*) * jobs.size(), &dj))) return rc;
  HIPCHK(c, nv12_resize_area_launch(dj, n, y_stride, uv_stride, (const AreaTab*)dxt, (const int*)dxs,
                                    (const AreaTab*)dyt, (const int*)dys, OH, OW, c->stream));
  return PC_OK;
}

extern "C" int pc_nv12_resize_area_fast_batch(pc_ctx* c, const uint8_t* const* ys, const uint8_t* const* uvs,
                                              uint8_t* const* dsts, int n, int H, int W, int y_stride, int uv_stride,
                                              int isx, int isy, int OH, int OW) {
  if (!c) return PC_ERR_ARG;
  std::vector<const void*> jobs;
  int rc = nv12_area_jobs(c, "pc_nv12_resize_area_fast_batch", ys, uvs, dsts, n, H, W, y_stride, uv_stride, jobs);
  if (rc) return rc;
  if (isx < 1 || isy < 1 || OH <= 0 || OW <= 0 || (long long)OW * isx > W || (long long)OH * isy > H)
    return fail(c, PC_ERR_ARG, "pc_nv12_resize_area_fast_batch: bad ratios");
  if (n == 0) return PC_OK;
  void* dj;
  if ((rc = stage_copy(c, jobs.data(), sizeof(void*) * jobs.size(), &dj))) return rc;
  HIPCHK(c, nv12_resize_area_fast_launch(dj, n, y_stride, uv_stride, isx, isy, OH, OW, c->stream));
  return PC_OK;
}

extern "C" int pc_embed_finalize(pc_ctx* c, const float* e, int ld, int n, int dim, int flip, float* out) {
  if (!c || n < 0) return fail(c, PC_ERR_ARG, "pc_embed_finalize: bad arguments");
  if (n == 0) return PC_OK;
  HIPCHK(c, embed_finalize_launch(e, ld, n, dim, flip, out, c->stream));
  return PC_OK;
}

extern "C" int pc_bank_match(pc_ctx* c, const float* q, int n, const float* bank, int b, int dim, float* fd,
                             int32_t* idx) {
  if (!c || n < 0 || b < 0 || dim <= 0) return fail(c, PC_ERR_ARG, "pc_bank_match: bad arguments");
  if (n == 0) return PC_OK;
  HIPCHK(c, bank_match_launch(q, n, bank, b, dim, fd, idx, c->stream));
  return PC_OK;
}

extern "C" int pc_arcface_embed(pc_net* net, const uint8_t* chips, int n, int flip, float* feat) {
  if (!net || n < 0) return PC_ERR_ARG;
  pc_ctx* c = net->ctx;
  if (n == 0) return PC_OK;
  const int rows = flip ? 2 * n : n;
  if (rows > net->max_batch) return fail(c, PC_ERR_ARG, "pc_arcface_embed: 2n exceeds the net's max batch");
  const NetTensor& I = net->tens[net->in_tensor];
  if (I.C != 4 || I.H != I.W) return fail(c, PC_ERR_FORMAT, "arcface net input must be square NHWC4");
  const size_t need = (size_t)net->max_batch * I.H * I.W * 4 * (net->f32 ? 4 : 2);
  if (net->prep_bytes < need) {
    if (net->prep) HIPCHK(c, hipFree(net->prep));
    HIPCHK(c, hipMalloc(&net->prep, need));
    net->prep_bytes = need;
  }
  HIPCHK(c, arcprep_launch(net->f32 ? PC_PREC_F32 : (net->in_centered ? PC_PREC_F16X3 : PC_PREC_F16), chips, n, I.H,
                           flip, net->prep, c->stream));
  int rc = pc_net_run(net, net->prep, rows);
  if (rc) return rc;
  const NetTensor& O = net->tens[net->outs[0]];
  const float* e = (const float*)tensor_ptr(net, net->outs[0]);
  HIPCHK(c, embed_finalize_launch(e, O.cs, n, O.C, flip, feat, c->stream));
  return PC_OK;
}

extern "C" int pc_scrfd_detect(pc_net* net, const pc_letterbox_desc* h, int n, int D, float det_thresh,
                               float nms_thresh, const float* h_det_scale, int max_det, float* dets, float* kps,
                               int32_t* count, int32_t* ncand) {
  if (!net || !h || n <= 0 || !h_det_scale || max_det <= 0) return PC_ERR_ARG;
  pc_ctx* c = net->ctx;
  if (n > net->max_batch) return fail(c, PC_ERR_ARG, "pc_scrfd_detect: batch exceeds max batch");
  if ((int)net->outs.size() != 3) return fail(c, PC_ERR_FORMAT, "SCRFD net must have 3 outputs");
  const NetTensor& I = net->tens[net->in_tensor];
  if (I.H != D || I.W != D) return fail(c, PC_ERR_ARG, "pc_scrfd_detect: D does not match the net input size");
  // candidate capacity = every anchor of the net (no cap: the reference keeps all
  // candidates >= det_thresh); images with more than 8192 go through scrfd_nms_big
  int cap = 0;
  for (int l = 0; l < 3; ++l) cap += net->tens[net->outs[l]].H * net->tens[net->outs[l]].W * 2;
  int pcap = 8192;
  while (pcap < cap) pcap <<= 1;
  const size_t cand_need = (size_t)n * cap * 16 * 4;
  // the candidate rows and the per-image counters are sized independently: a later call
  // with more images but a smaller D needs fewer rows and more counters
  if (c->cand_bytes < cand_need) {
    if (c->cand) hipFree(c->cand);
    c->cand = nullptr;
    c->cand_bytes = 0;
    HIPCHK(c, hipMalloc((void**)&c->cand, cand_need));
    c->cand_bytes = cand_need;
  }
  if (c->cand_images < (size_t)n) {
    if (c->cand_count) hipFree(c->cand_count);
    if (c->det_scale) hipFree(c->det_scale);
    c->cand_count = nullptr;
    c->det_scale = nullptr;
    c->cand_images = 0;
    HIPCHK(c, hipMalloc((void**)&c->cand_count, (size_t)n * 4 + 256));
    HIPCHK(c, hipMalloc((void**)&c->det_scale, (size_t)n * 4 + 256));
    c->cand_images = n;
  }
  const size_t keys_b = (size_t)n * pcap * 8, map_b = (size_t)n * cap * 4, kept_b = (size_t)n * cap * 16;
  if (c->nms_big_bytes < keys_b + map_b + kept_b) {
    if (c->nms_big) hipFree(c->nms_big);
    HIPCHK(c, hipMalloc(&c->nms_big, keys_b + map_b + kept_b));
    c->nms_big_bytes = keys_b + map_b + kept_b;
  }
  // letterbox into the net's own input staging area (reuse prep scratch)
  const size_t need = (size_t)net->max_batch * D * D * 4 * (net->f32 ? 4 : 2);
  if (net->prep_bytes < need) {
    if (net->prep) HIPCHK(c, hipFree(net->prep));
    HIPCHK(c, hipMalloc(&net->prep, need));
    net->prep_bytes = need;
  }
  int rc = pc_letterbox(c, net->f32 ? PC_PREC_F32 : PC_PREC_F16, h, n, D, net->prep);
  if (rc) return rc;
  rc = pc_net_run(net, net->prep, n);
  if (rc) return rc;
  DecodeParams p;
  memset(&p, 0, sizeof(p));
  p.nlv = 3;
  const int strides[3] = {8, 16, 32};
  int loc = 0, anc = 0;
  for (int l = 0; l < 3; ++l) {
    const NetTensor& O = net->tens[net->outs[l]];
    if (!(O.is_f32 || net->f32)) return fail(c, PC_ERR_FORMAT, "SCRFD head outputs must be f32");
    p.lv[l].out = (const float*)tensor_ptr(net, net->outs[l]);
    p.lv[l].H = O.H; p.lv[l].W = O.W; p.lv[l].cs = O.cs; p.lv[l].stride = strides[l];
    p.lv[l].loc_offset = loc; p.lv[l].anchor_offset = anc;
    loc += O.H * O.W;
    anc += O.H * O.W * 2;
  }
  p.total_loc = loc;
  p.thresh = det_thresh;
  void* dscale;
  if ((rc = stage_copy(c, h_det_scale, (size_t)n * 4, &dscale))) return rc;
  HIPCHK(c, hipMemsetAsync(c->cand_count, 0, n * 4, c->stream));
  p.det_scale = (const float*)dscale;
  p.cand = c->cand;
  p.count = c->cand_count;
  p.cap = cap;
  HIPCHK(c, scrfd_decode_launch(p, n, c->stream));
  HIPCHK(c, scrfd_nms_launch(c->cand, c->cand_count, cap, nms_thresh, max_det, dets, kps, count, n, c->stream));
  {
    char* big = (char*)c->nms_big;
    HIPCHK(c, scrfd_nms_big_launch(c->cand, c->cand_count, cap, pcap, (unsigned long long*)big, (int*)(big + keys_b),
                                   (float*)(big + keys_b + map_b), nms_thresh, max_det, dets, kps, count, n,
                                   c->stream));
  }
  if (ncand) HIPCHK(c, hipMemcpyAsync(ncand, c->cand_count, n * 4, hipMemcpyDeviceToDevice, c->stream));
  return PC_OK;
}

// ===========================================================================
// YOLOv8 person detection (PersonDetector.detect, detectors.py:271-296)
// ===========================================================================
static int check_yolo_descs(pc_ctx* c, const pc_yolo_letterbox_desc* h, int n, int Hp, int Wp) {
  for (int i = 0; i < n; ++i) {
    const pc_yolo_letterbox_desc& d = h[i];
    if (!d.d_src || d.H <= 0 || d.W <= 0 || d.row_stride < d.W * 3 || d.new_w <= 0 || d.new_h <= 0 || d.top < 0 ||
        d.left < 0 || d.top + d.new_h > Hp || d.left + d.new_w > Wp || (d.identity && (d.new_w != d.W || d.new_h != d.H)))
      return fail(c, PC_ERR_ARG, "yolo letterbox job out of range");
  }
  return PC_OK;
}

extern "C" int pc_yolo_letterbox(pc_ctx* c, int prec, const pc_yolo_letterbox_desc* h, int n, int Hp, int Wp,
                                 void* out) {
  if (!c || !h || n <= 0 || Hp <= 0 || Wp <= 0 || !out) return fail(c, PC_ERR_ARG, "pc_yolo_letterbox: bad arguments");
  int rc = check_yolo_descs(c, h, n, Hp, Wp);
  if (rc) return rc;
  void* dd;
  if ((rc = stage_copy(c, h, sizeof(pc_yolo_letterbox_desc) * n, &dd))) return rc;
  HIPCHK(c, yolo_letterbox_launch(prec == PC_PREC_F32, (const YoloLetterboxDesc*)dd, n, Hp, Wp, out, c->stream));
  return PC_OK;
}

static int yolo_detect_impl(pc_net* net, const pc_yolo_letterbox_desc* h, int n, int Hp, int Wp, float conf, float iou,
                            const pc_yolo_scale* h_scale, int max_det, float* dets, int32_t* count, int32_t* ncand,
                            int nkpt, const float* h_kpt_pad, float* kpts) {
  if (!net || !h || n <= 0 || !h_scale || max_det <= 0 || !dets || !count) return PC_ERR_ARG;
  if (nkpt < 0 || (nkpt > 0 && (!h_kpt_pad || !kpts || max_det > 1024))) return PC_ERR_ARG;
  const int nk = nkpt * 3;
  pc_ctx* c = net->ctx;
  if (n > net->max_batch) return fail(c, PC_ERR_ARG, "pc_yolo_detect: batch exceeds max batch");
  if ((int)net->outs.size() != 3) return fail(c, PC_ERR_FORMAT, "YOLO net must have 3 head outputs");
  const NetTensor& I = net->tens[net->in_tensor];
  if (I.H != Hp || I.W != Wp || I.C != 4) return fail(c, PC_ERR_ARG, "pc_yolo_detect: canvas does not match the net input");
  if (int e = check_yolo_descs(c, h, n, Hp, Wp)) return e;
  const size_t need = (size_t)net->max_batch * Hp * Wp * 4 * (net->f32 ? 4 : 2);
  if (net->prep_bytes < need) {
    if (net->prep) HIPCHK(c, hipFree(net->prep));
    HIPCHK(c, hipMalloc(&net->prep, need));
    net->prep_bytes = need;
  }
  int rc = pc_yolo_letterbox(c, net->f32 ? PC_PREC_F32 : PC_PREC_F16, h, n, Hp, Wp, net->prep);
  if (rc) return rc;
  rc = pc_net_run(net, net->prep, n);
  if (rc) return rc;
  YoloDecodeParams p;
  memset(&p, 0, sizeof(p));
  p.nlv = 3;
  int loc = 0, nc = -1;
  for (int l = 0; l < 3; ++l) {
    const NetTensor& O = net->tens[net->outs[l]];
    if (!(O.is_f32 || net->f32)) return fail(c, PC_ERR_FORMAT, "YOLO head outputs must be f32");
    const int ncl = O.C - 64 - nk;
    if (ncl <= 0 || (nc >= 0 && ncl != nc)) return fail(c, PC_ERR_FORMAT, "YOLO head channel layout");
    nc = ncl;
    p.lv[l].out = (const float*)tensor_ptr(net, net->outs[l]);
    p.lv[l].H = O.H; p.lv[l].W = O.W; p.lv[l].cs = O.cs;
    p.lv[l].stride = Hp / O.H;
    p.lv[l].loc_offset = loc;
    loc += O.H * O.W;
  }
  // candidate slots for every anchor: a low threshold on a big canvas may pass most of them
  // (above 16384 candidates the global-memory NMS runs)
  const int cap = std::max(16384, loc);
  if (c->ycand_images < (size_t)n || c->ycand_cap < cap) {
    if (c->ycand) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(c->ycand); }
    if (c->ycount) hipFree(c->ycount);
    HIPCHK(c, hipMalloc((void**)&c->ycand, (size_t)n * cap * 8 * 4));
    HIPCHK(c, hipMalloc((void**)&c->ycount, (size_t)n * 4));
    c->ycand_images = n;
    c->ycand_cap = cap;
  }
  p.total = loc;
  p.nc = nc;
  p.conf = conf;
  p.cand = c->ycand;
  p.count = c->ycount;
  p.cap = cap;
  void* dsc;
  if ((rc = stage_copy(c, h_scale, sizeof(pc_yolo_scale) * n, &dsc))) return rc;
  HIPCHK(c, hipMemsetAsync(c->ycount, 0, n * 4, c->stream));
  HIPCHK(c, yolo_decode_launch(p, n, c->stream));
  int* keep_anchor = nullptr;
  if (nk) {
    if (c->ykeep_bytes < (size_t)n * max_det * 4) {
      if (c->ykeep) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(c->ykeep)); }
      HIPCHK(c, hipMalloc((void**)&c->ykeep, (size_t)n * max_det * 4));
      c->ykeep_bytes = (size_t)n * max_det * 4;
    }
    keep_anchor = c->ykeep;
  }
  HIPCHK(c, yolo_nms_launch(c->ycand, c->ycount, cap, iou, max_det, (const YoloScale*)dsc, dets, count, n, c->stream,
                            keep_anchor));
  if (loc > 16384) {
    int pcap = 8192;
    while (pcap < cap) pcap <<= 1;
    const size_t kb = (size_t)n * pcap * 8 + (size_t)n * cap * 4 + (size_t)n * max_det * 16;
    if (c->ybig_bytes < kb) {
      if (c->ybig) { HIPCHK(c, hipStreamSynchronize(c->stream)); hipFree(c->ybig); }
      HIPCHK(c, hipMalloc(&c->ybig, kb));
      c->ybig_bytes = kb;
    }
    char* b = (char*)c->ybig;
    HIPCHK(c, yolo_nms_big_launch(c->ycand, c->ycount, cap, pcap, (unsigned long long*)b,
                                  (int*)(b + (size_t)n * pcap * 8), (float*)(b + (size_t)n * pcap * 8 + (size_t)n * cap * 4),
                                  iou, max_det, (const YoloScale*)dsc, dets, count, keep_anchor, n, c->stream));
  }
  if (nk) {
    void* dks;
    if ((rc = stage_copy(c, h_kpt_pad, sizeof(float) * 2 * n, &dks))) return rc;
    HIPCHK(c, yolo_kpts_launch(p, nk, 64 + nc, max_det, count, keep_anchor, (const YoloScale*)dsc,
                               (const YoloKptScale*)dks, kpts, n, c->stream));
  }
  if (ncand) HIPCHK(c, hipMemcpyAsync(ncand, c->ycount, n * 4, hipMemcpyDeviceToDevice, c->stream));
  return PC_OK;
}

extern "C" int pc_yolo_detect(pc_net* net, const pc_yolo_letterbox_desc* h, int n, int Hp, int Wp, float conf,
                              float iou, const pc_yolo_scale* h_scale, int max_det, float* dets, int32_t* count,
                              int32_t* ncand) {
  return yolo_detect_impl(net, h, n, Hp, Wp, conf, iou, h_scale, max_det, dets, count, ncand, 0, nullptr, nullptr);
}

extern "C" int pc_yolo_pose_detect(pc_net* net, const pc_yolo_letterbox_desc* h, int n, int Hp, int Wp, float conf,
                                   float iou, const pc_yolo_scale* h_scale, const float* h_kpt_pad, int max_det,
                                   int nkpt, float* dets, float* kpts, int32_t* count, int32_t* ncand) {
  if (nkpt <= 0) return fail(net ? net->ctx : nullptr, PC_ERR_ARG, "pc_yolo_pose_detect: nkpt must be positive");
  return yolo_detect_impl(net, h, n, Hp, Wp, conf, iou, h_scale, max_det, dets, count, ncand, nkpt, h_kpt_pad, kpts);
}

// ===========================================================================
// ReID: OpenCLIP ViT image tower (ReIDEmbedder.extract, reid_embedder.py:38-57)
// ===========================================================================
static const int kClipKmax = 64;

// the tower geometries pc_clip.hip, the conv K tile and the attention kernels are tested at
static bool clip_geom_ok(int side, int patch) {
  return (side == 224 || side == 336) && (patch == 14 || patch == 16 || patch == 32) && side % patch == 0;
}

extern "C" int pc_clip_prep_geom(pc_ctx* c, int prec, int side, int patch, const pc_crop_desc* h, int n, void* out) {
  if (!c || !h || n <= 0 || !out) return fail(c, PC_ERR_ARG, "pc_clip_prep: bad arguments");
  if (!clip_geom_ok(side, patch)) return fail(c, PC_ERR_ARG, "pc_clip_prep: side in {224, 336}, patch in {14, 16, 32}, side % patch == 0");
  // host: geometry + Pillow coefficient tables for the `side` kept columns / rows of each crop size; crops
  // of one size share one table (the 112 x 112 chips of the OpenCLIP face mode: one table per call)
  struct Tabs { int kh, kv, row0, nrows; std::vector<int32_t> hb, hk, vb, vk; };
  std::vector<Tabs> T;
  std::map<std::pair<int, int>, int> tab_of_size;
  std::vector<int> ti(n);
  size_t tmp_bytes = 0, tab_ints = 0;
  int max_rows = 0;
  for (int i = 0; i < n; ++i) {
    const pc_crop_desc& d = h[i];
    if (!d.d_src || d.H <= 0 || d.W <= 0 || d.row_stride < d.W * 3) return fail(c, PC_ERR_ARG, "pc_clip_prep: bad crop");
    const auto seen = tab_of_size.find({d.H, d.W});
    if (seen != tab_of_size.end()) {
      ti[i] = seen->second;
      tmp_bytes += (size_t)T[ti[i]].nrows * side * 3;
      continue;
    }
    ti[i] = tab_of_size[{d.H, d.W}] = (int)T.size();
    int32_t g[4];
    pc_clip_geometry(d.H, d.W, side, g);
    T.emplace_back();
    Tabs& t = T.back();
    t.hb.resize(2 * side); t.vb.resize(2 * side);
    t.hk.resize((size_t)side * kClipKmax); t.vk.resize((size_t)side * kClipKmax);
    t.kh = pc_pil_bicubic_coeffs(d.W, g[0], g[3], side, t.hb.data(), t.hk.data(), kClipKmax);
    t.kv = pc_pil_bicubic_coeffs(d.H, g[1], g[2], side, t.vb.data(), t.vk.data(), kClipKmax);
    if (t.kh < 0 || t.kv < 0) return fail(c, PC_ERR_CAPACITY, "pc_clip_prep: crop too large for the resample tables");
    t.hk.resize((size_t)side * t.kh); t.vk.resize((size_t)side * t.kv);
    int lo = 1 << 30, hi = 0;
    for (int y = 0; y < side; ++y) { lo = std::min(lo, t.vb[2 * y]); hi = std::max(hi, t.vb[2 * y] + t.vb[2 * y + 1]); }
    t.row0 = lo; t.nrows = std::max(hi - lo, 1);
    for (int y = 0; y < side; ++y) t.vb[2 * y] -= lo;
    max_rows = std::max(max_rows, t.nrows);
    tmp_bytes += (size_t)t.nrows * side * 3;
    tab_ints += t.hb.size() + t.hk.size() + t.vb.size() + t.vk.size();
  }
  if (c->clip_tmp_bytes < tmp_bytes) {
    if (c->clip_tmp) { HIPCHK(c, hipStreamSynchronize(c->stream)); HIPCHK(c, hipFree(c->clip_tmp)); }
    HIPCHK(c, hipMalloc(&c->clip_tmp, tmp_bytes));
    c->clip_tmp_bytes = tmp_bytes;
  }
  std::vector<int32_t> tabs;
  tabs.reserve(tab_ints);
  std::vector<size_t> off(T.size() * 4);
  for (int i = 0; i < (int)T.size(); ++i) {
    off[4 * i + 0] = tabs.size(); tabs.insert(tabs.end(), T[i].hb.begin(), T[i].hb.end());
    off[4 * i + 1] = tabs.size(); tabs.insert(tabs.end(), T[i].hk.begin(), T[i].hk.end());
    off[4 * i + 2] = tabs.size(); tabs.insert(tabs.end(), T[i].vb.begin(), T[i].vb.end());
    off[4 * i + 3] = tabs.size(); tabs.insert(tabs.end(), T[i].vk.begin(), T[i].vk.end());
  }
  void* dtab;
  int rc = stage_copy(c, tabs.data(), tabs.size() * 4, &dtab);
  if (rc) return rc;
  std::vector<ClipPrepDesc> descs(n);
  size_t tmp_off = 0;
  for (int i = 0; i < n; ++i) {
    ClipPrepDesc& d = descs[i];
    const int32_t* tb = (const int32_t*)dtab;
    const int k = ti[i];
    d.src = h[i].d_src; d.H = h[i].H; d.W = h[i].W; d.row_stride = h[i].row_stride;
    d.kh = T[k].kh; d.kv = T[k].kv;
    d.hb = tb + off[4 * k]; d.hk = tb + off[4 * k + 1]; d.vb = tb + off[4 * k + 2]; d.vk = tb + off[4 * k + 3];
    d.row0 = T[k].row0; d.nrows = T[k].nrows;
    d.tmp = (uint8_t*)c->clip_tmp + tmp_off;
    tmp_off += (size_t)T[k].nrows * side * 3;
  }
  void* ddesc;
  if ((rc = stage_copy(c, descs.data(), sizeof(ClipPrepDesc) * n, &ddesc))) return rc;
  HIPCHK(c, clip_prep_launch(prec == PC_PREC_F32 ? 1 : (prec == PC_PREC_F16X3 ? 2 : 0), (const ClipPrepDesc*)ddesc, n,
                             max_rows, side, patch, out, c->stream));
  return PC_OK;
}

extern "C" int pc_clip_prep(pc_ctx* c, int prec, const pc_crop_desc* h, int n, void* out) {
  return pc_clip_prep_geom(c, prec, 224, 14, h, n, out);
}

extern "C" int pc_clip_embed_geom(pc_net* net, int side, int patch, const pc_crop_desc* h, int n, float* feat) {
  if (!net || !h || n < 0 || !feat) return PC_ERR_ARG;
  pc_ctx* c = net->ctx;
  if (!clip_geom_ok(side, patch)) return fail(c, PC_ERR_ARG, "pc_clip_embed: side in {224, 336}, patch in {14, 16, 32}, side % patch == 0");
  if (n == 0) return PC_OK;
  if (n > net->max_batch) return fail(c, PC_ERR_ARG, "pc_clip_embed: batch exceeds max batch");
  const NetTensor& I = net->tens[net->in_tensor];
  // the net's input against the explicit geometry: [1][(side/patch)^2 + 1][cpad(3 patch^2)]
  const int tok = (side / patch) * (side / patch) + 1, kpad = (3 * patch * patch + 31) / 32 * 32;
  // the f16x3 tower (models_clip.compile_clip_vit(split=True)): a centred input of doubled rows on an f16 net
  const bool x3 = I.C == 2 * kpad;
  if (I.H != 1 || I.W != tok || (I.C != kpad && !x3))
    return fail(c, PC_ERR_FORMAT, "CLIP net input must be 1 x tokens x padded patch columns of its geometry (1x257x608 at 224 / 14)");
  if (x3 ? (!net->in_centered || net->f32 || I.split) : net->in_centered)
    return fail(c, PC_ERR_FORMAT, "CLIP net input: doubled rows centred on an f16 net (f16x3 tower, 1x257x1216 at 224 / 14) or normalised rows");
  const size_t need = (size_t)net->max_batch * tok * I.C * (net->f32 ? 4 : 2);
  if (net->prep_bytes < need) {
    if (net->prep) HIPCHK(c, hipFree(net->prep));
    HIPCHK(c, hipMalloc(&net->prep, need));
    net->prep_bytes = need;
  }
  int rc = pc_clip_prep_geom(c, net->f32 ? PC_PREC_F32 : (x3 ? PC_PREC_F16X3 : PC_PREC_F16), side, patch, h, n, net->prep);
  if (rc) return rc;
  rc = pc_net_run(net, net->prep, n);
  if (rc) return rc;
  const NetTensor& O = net->tens[net->outs[0]];
  if (!(O.is_f32 || net->f32) || O.H * O.W != 1) return fail(c, PC_ERR_FORMAT, "CLIP output must be f32 [1][1][dim]");
  HIPCHK(c, embed_l2_launch((const float*)tensor_ptr(net, net->outs[0]), O.cs, n, O.C, 1e-12f, feat, c->stream));
  return PC_OK;
}

extern "C" int pc_clip_embed(pc_net* net, const pc_crop_desc* h, int n, float* feat) {
  return pc_clip_embed_geom(net, 224, 14, h, n, feat);
}

extern "C" int pc_l2_normalize(pc_ctx* c, const float* e, int ld, int n, int dim, float eps, float* out) {
  if (!c || n < 0 || !e || !out) return fail(c, PC_ERR_ARG, "pc_l2_normalize: bad arguments");
  if (n == 0) return PC_OK;
  HIPCHK(c, embed_l2_launch(e, ld, n, dim, eps, out, c->stream));
  return PC_OK;
}

// ---- dataset curator ----
// A target's tables, checked on the host before anything is launched: monotone starts inside the
// coefficient array, every source index inside the gray plane's axis.
static bool curate_tables_ok(const pc_area_tab* tabs, int n_tabs, const int32_t* starts, int n_starts, int at, int dlen,
                             int slen) {
  if (at < 0 || (long long)at + dlen + 1 > n_starts) return false;
  const int32_t* s = starts + at;
  if (s[0] < 0 || s[dlen] > n_tabs) return false;
  for (int d = 0; d < dlen; ++d)
    if (s[d + 1] < s[d]) return false;
  for (int k = s[0]; k < s[dlen]; ++k)
    if (tabs[k].si < 0 || tabs[k].si >= slen) return false;
  return true;
}

extern "C" int pc_crop_metrics(pc_ctx* c, const pc_curate_desc* h, int n, const pc_area_tab* tabs, int n_tabs,
                               const int32_t* starts, int n_starts, const double* h_dct, void* d_scratch,
                               size_t scratch_bytes, void* d_out, size_t out_bytes) {
  // (n <= 16384: the resize launch has two grid rows per image)
  if (!c || n < 0 || n > 16384 || n_tabs < 0 || n_starts < 0) return fail(c, PC_ERR_ARG, "pc_crop_metrics: bad arguments");
  if (n == 0) return PC_OK;
  if (!h || !h_dct || !d_scratch || !d_out || (n_tabs > 0 && !tabs) || (n_starts > 0 && !starts))
    return fail(c, PC_ERR_ARG, "pc_crop_metrics: null argument");
  if (((uintptr_t)d_scratch & 15) || ((uintptr_t)d_out & 15))
    return fail(c, PC_ERR_ARG, "pc_crop_metrics: buffers must be 16-byte aligned");
  std::vector<uint64_t> off((size_t)n * 5);
  size_t need_s = 0, need_o = 0;
  if (pc_crop_metrics_layout(h, n, off.data(), &need_s, &need_o) != PC_OK)
    return fail(c, PC_ERR_ARG, "pc_crop_metrics: bad image descriptor (32 <= w, h <= 16384, row_stride >= 3 w, "
                               "w2 / h2 / kinds as sharpness_norm and phash64 resize)");
  if (scratch_bytes < need_s || out_bytes < need_o)
    return fail(c, PC_ERR_ARG, "pc_crop_metrics: scratch / output buffer smaller than pc_crop_metrics_layout asks");
  std::vector<CurateImg> imgs((size_t)n);
  std::vector<int> bands;
  int max_pixels = 32 * 32;
  for (int i = 0; i < n; ++i) {
    const pc_curate_desc& q = h[i];
    if (!q.d_src) return fail(c, PC_ERR_ARG, "pc_crop_metrics: null image");
    const uint64_t* o = &off[(size_t)i * 5];
    CurateImg& m = imgs[i];
    m.src = q.d_src;
    m.row_stride = q.row_stride; m.w = q.w; m.h = q.h;
    m.gpitch = (q.w + 15) & ~15;
    m.gray = (uint8_t*)d_scratch + o[0];
    for (int t = 0; t < 2; ++t) {
      CurateTarget& T = m.t[t];
      T.ow = t ? 32 : q.w2;
      T.oh = t ? 32 : q.h2;
      T.kind = q.kind[t]; T.isx = q.isx[t]; T.isy = q.isy[t]; T.xs = q.xs[t]; T.ys = q.ys[t];
      T.dst = (uint8_t*)d_scratch + o[1 + t];
      T.pitch = T.kind == PC_CURATE_COPY ? m.gpitch : ((T.ow + 15) & ~15);
      if (T.kind == PC_CURATE_AREA && (!curate_tables_ok(tabs, n_tabs, starts, n_starts, T.xs, T.ow, q.w) ||
                                       !curate_tables_ok(tabs, n_tabs, starts, n_starts, T.ys, T.oh, q.h)))
        return fail(c, PC_ERR_ARG, "pc_crop_metrics: INTER_AREA tables out of range");
      max_pixels = std::max(max_pixels, T.ow * T.oh);
    }
    pc_curate_record* rec = (pc_curate_record*)((char*)d_out + o[3]);
    m.sums = (unsigned long long*)&rec->sum_g2;
    m.wh = &rec->w2;
    m.hist = rec->hist;
    m.coef = rec->coef;
    m.row_sum = (unsigned*)((char*)d_out + o[4]);
    m.col_sum = m.row_sum + q.h;
    for (int y = 0; y < q.h; y += CURATE_BAND) { bands.push_back(i); bands.push_back(y); }
  }
  // one staged blob (a second stage_copy could wrap the ring over the first): descriptors, bands,
  // coefficient table, starts, cosine table, each from a 16-byte boundary
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  const size_t o_img = 0, o_band = up16(o_img + imgs.size() * sizeof(CurateImg));
  const size_t o_tab = up16(o_band + bands.size() * sizeof(int));
  const size_t o_st = up16(o_tab + (size_t)n_tabs * sizeof(pc_area_tab));
  const size_t o_dct = up16(o_st + (size_t)n_starts * sizeof(int32_t));
  const size_t total = o_dct + 256 * sizeof(double);
  std::vector<char> blob(total, 0);
  memcpy(blob.data() + o_img, imgs.data(), imgs.size() * sizeof(CurateImg));
  memcpy(blob.data() + o_band, bands.data(), bands.size() * sizeof(int));
  if (n_tabs) memcpy(blob.data() + o_tab, tabs, (size_t)n_tabs * sizeof(pc_area_tab));
  if (n_starts) memcpy(blob.data() + o_st, starts, (size_t)n_starts * sizeof(int32_t));
  memcpy(blob.data() + o_dct, h_dct, 256 * sizeof(double));
  void* dv = nullptr;
  int rc = stage_copy(c, blob.data(), total, &dv);
  if (rc) return rc;
  char* db = (char*)dv;
  HIPCHK(c, hipMemsetAsync(d_out, 0, need_o, c->stream));
  HIPCHK(c, curate_metrics_launch(db + o_img, n, db + o_band, (int)(bands.size() / 2), db + o_tab,
                                  (const int*)(db + o_st), (const double*)(db + o_dct), max_pixels, c->stream));
  return PC_OK;
}

extern "C" int pc_sim_matrix(pc_ctx* c, const float* F, int n, int dim, float* S) {
  if (!c || n < 0 || n > 8192 || dim <= 0) return fail(c, PC_ERR_ARG, "pc_sim_matrix: 0 <= n <= 8192, dim >= 1");
  if (n == 0) return PC_OK;
  if (!F || !S) return fail(c, PC_ERR_ARG, "pc_sim_matrix: null argument");
  HIPCHK(c, sim_matrix_launch(F, n, dim, S, c->stream));
  return PC_OK;
}

extern "C" int pc_mmr_order(pc_ctx* c, const float* S, const float* q, int n, int k, double alpha, int32_t* order) {
  if (!c || n < 0 || n > 8192 || k < 0 || k > n || !(alpha == alpha))
    return fail(c, PC_ERR_ARG, "pc_mmr_order: 0 <= k <= n <= 8192");
  if (n == 0 || k == 0) return PC_OK;
  if (!S || !q || !order) return fail(c, PC_ERR_ARG, "pc_mmr_order: null argument");
  HIPCHK(c, mmr_order_launch(S, q, n, k, alpha, order, c->stream));
  return PC_OK;
}

// ---- main-pass frame gauges (pc_gauge.hip) ----
static_assert(sizeof(pc_gray_desc) == 48 && sizeof(pc_gray_region) == 32 && sizeof(pc_motion_box) == 40,
              "gauge layouts");

// the rows of `h` rows of U units each, cut into jobs of about GAUGE_JOB_UNITS units
static void gauge_jobs(std::vector<GaugeJob>& jobs, int item, int w, int h) {
  const int U = (w + 15) / 16 + 1;
  const int rows = std::max(1, GAUGE_JOB_UNITS / U);
  for (int y = 0; y < h; y += rows) jobs.push_back(GaugeJob{item, y, std::min(rows, h - y), 0});
}

extern "C" int pc_frame_gray(pc_ctx* c, const pc_gray_desc* h, int n) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || n > 65535 || (n > 0 && !h)) return fail(c, PC_ERR_ARG, "pc_frame_gray: bad arguments");
  if (n == 0) return PC_OK;
  std::vector<GaugeImg> imgs((size_t)n);
  std::vector<int> bands;
  for (int i = 0; i < n; ++i) {
    const pc_gray_desc& q = h[i];
    if (!q.d_src || !q.d_gray || !q.d_row_sum || !q.d_col_sum || q.w < 32 || q.h < 32 || q.w > PC_GAUGE_MAX_SIDE ||
        q.h > PC_GAUGE_MAX_SIDE || (long long)q.row_stride < 3LL * q.w || (q.gray_pitch & 15) ||
        q.gray_pitch < ((q.w + 15) & ~15) || ((uintptr_t)q.d_gray & 15) || ((uintptr_t)q.d_row_sum & 3) ||
        ((uintptr_t)q.d_col_sum & 3))
      return fail(c, PC_ERR_ARG, "pc_frame_gray: bad frame (non-null pointers, 32 <= w, h <= 16384, row_stride >= 3 w, "
                                 "d_gray and gray_pitch multiples of 16, gray_pitch >= w rounded up to 16, "
                                 "4-byte aligned sums)");
    GaugeImg& m = imgs[i];
    memset(&m, 0, sizeof(m));
    m.src = q.d_src; m.row_stride = q.row_stride; m.w = q.w; m.h = q.h; m.gpitch = q.gray_pitch;
    m.gray = q.d_gray; m.row_sum = q.d_row_sum; m.col_sum = q.d_col_sum;
  }
  // Rows per workgroup: the tallest band of 32, 16, 8 that still gives GAUGE_MIN_WG workgroups (four per CU;
  // one 4K frame in bands of 32 would be 68 workgroups on 256 CUs), else 8. A shorter band costs one more
  // column atomic per column and band, so it is not taken where the batch fills the device anyway.
  int band = GAUGE_BAND;
  for (; band > 8; band >>= 1) {
    long long wg = 0;
    for (int i = 0; i < n; ++i) wg += (h[i].h + band - 1) / band;
    if (wg >= GAUGE_MIN_WG) break;
  }
  for (int i = 0; i < n; ++i)
    for (int y = 0; y < h[i].h; y += band) { bands.push_back(i); bands.push_back(y); }
  const size_t o_band = (imgs.size() * sizeof(GaugeImg) + 15) & ~size_t(15);
  const size_t total = o_band + bands.size() * sizeof(int);
  std::vector<char> blob(total, 0);
  memcpy(blob.data(), imgs.data(), imgs.size() * sizeof(GaugeImg));
  memcpy(blob.data() + o_band, bands.data(), bands.size() * sizeof(int));
  void* dv = nullptr;
  int rc = stage_copy(c, blob.data(), total, &dv);
  if (rc) return rc;
  // The column sums are accumulated: zero them. A frame whose row sums end where its column sums begin is
  // zeroed as one span (the row sums are written in full afterwards), and spans that touch share a memset:
  // frames laid out back to back cost one. Nothing between two spans is written.
  auto span = [&](int i, char*& lo, char*& hi) {
    lo = (char*)h[i].d_col_sum;
    hi = lo + (size_t)h[i].w * 4;
    if ((char*)(h[i].d_row_sum + h[i].h) == lo) lo = (char*)h[i].d_row_sum;
  };
  for (int i = 0; i < n;) {
    char *lo, *hi;
    span(i, lo, hi);
    int j = i + 1;
    for (; j < n; ++j) {
      char *a, *b;
      span(j, a, b);
      if (a != hi) break;
      hi = b;
    }
    HIPCHK(c, hipMemsetAsync(lo, 0, (size_t)(hi - lo), c->stream));
    i = j;
  }
  HIPCHK(c, frame_gray_launch(dv, (char*)dv + o_band, (int)(bands.size() / 2), band, c->stream));
  return PC_OK;
}

extern "C" int pc_gray_region_hist(pc_ctx* c, const pc_gray_region* h, int n, uint32_t* d_out) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || n > 65535 || (n > 0 && (!h || !d_out)) || ((uintptr_t)d_out & 3))
    return fail(c, PC_ERR_ARG, "pc_gray_region_hist: bad arguments");
  if (n == 0) return PC_OK;
  std::vector<GaugeRegion> regs((size_t)n);
  std::vector<GaugeJob> jobs;
  for (int i = 0; i < n; ++i) {
    const pc_gray_region& q = h[i];
    if (!q.d_plane || q.w < 1 || q.h < 1 || q.w > PC_GAUGE_MAX_SIDE || q.h > PC_GAUGE_MAX_SIDE || q.x < 0 || q.y < 0 ||
        q.pitch > PC_GAUGE_MAX_PITCH || (long long)q.x + q.w > q.pitch || (long long)q.y + q.h > PC_GAUGE_MAX_SIDE)
      return fail(c, PC_ERR_ARG, "pc_gray_region_hist: bad region (non-null plane, 1 <= w, h <= 16384, 0 <= x, y, "
                                 "x + w <= pitch <= 2^20, y + h <= 16384)");
    GaugeRegion& r = regs[i];
    memset(&r, 0, sizeof(r));
    r.base = q.d_plane + (long long)q.y * q.pitch + q.x;
    r.pitch = q.pitch; r.w = q.w; r.h = q.h;
    r.hist = d_out + (size_t)i * 256;
    gauge_jobs(jobs, i, q.w, q.h);
  }
  const size_t o_job = (regs.size() * sizeof(GaugeRegion) + 15) & ~size_t(15);
  const size_t total = o_job + jobs.size() * sizeof(GaugeJob);
  std::vector<char> blob(total, 0);
  memcpy(blob.data(), regs.data(), regs.size() * sizeof(GaugeRegion));
  memcpy(blob.data() + o_job, jobs.data(), jobs.size() * sizeof(GaugeJob));
  void* dv = nullptr;
  int rc = stage_copy(c, blob.data(), total, &dv);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)n * 256 * sizeof(uint32_t), c->stream));
  HIPCHK(c, gauge_region_hist_launch(dv, (char*)dv + o_job, (int)jobs.size(), c->stream));
  return PC_OK;
}

extern "C" int pc_gray_motion(pc_ctx* c, const pc_motion_box* h, int n, int thresh, uint32_t* d_counts) {
  if (!c) return PC_ERR_ARG;
  if (n < 0 || n > 65535 || (n > 0 && (!h || !d_counts)) || ((uintptr_t)d_counts & 3) || thresh < 0 || thresh > 255)
    return fail(c, PC_ERR_ARG, "pc_gray_motion: bad arguments (0 <= n <= 65535, 0 <= thresh <= 255)");
  if (n == 0) return PC_OK;
  std::vector<GaugeBox> boxes((size_t)n);
  std::vector<GaugeJob> jobs;
  for (int i = 0; i < n; ++i) {
    const pc_motion_box& q = h[i];
    if (!q.d_cur || !q.d_prev || q.x1 < 0 || q.y1 < 0 || q.x2 <= q.x1 || q.y2 <= q.y1 || q.pitch > PC_GAUGE_MAX_PITCH ||
        q.x2 > q.pitch || q.y2 > PC_GAUGE_MAX_SIDE || q.x2 - q.x1 > PC_GAUGE_MAX_SIDE)
      return fail(c, PC_ERR_ARG, "pc_gray_motion: bad box (non-null planes, 0 <= x1 < x2 <= pitch <= 2^20, "
                                 "0 <= y1 < y2 <= 16384, x2 - x1 <= 16384)");
    GaugeBox& b = boxes[i];
    memset(&b, 0, sizeof(b));
    const long long off = (long long)q.y1 * q.pitch + q.x1;
    b.cur = q.d_cur + off; b.prev = q.d_prev + off;
    b.pitch = q.pitch; b.w = q.x2 - q.x1; b.h = q.y2 - q.y1;
    b.count = d_counts + i;
    gauge_jobs(jobs, i, b.w, b.h);
  }
  const size_t o_job = (boxes.size() * sizeof(GaugeBox) + 15) & ~size_t(15);
  const size_t total = o_job + jobs.size() * sizeof(GaugeJob);
  std::vector<char> blob(total, 0);
  memcpy(blob.data(), boxes.data(), boxes.size() * sizeof(GaugeBox));
  memcpy(blob.data() + o_job, jobs.data(), jobs.size() * sizeof(GaugeJob));
  void* dv = nullptr;
  int rc = stage_copy(c, blob.data(), total, &dv);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(uint32_t), c->stream));
  HIPCHK(c, gauge_motion_launch(dv, (char*)dv + o_job, (int)jobs.size(), thresh, c->stream));
  return PC_OK;
}

extern "C" int pc_gray_resize_area(pc_ctx* c, const uint8_t* d_gray, int pitch, int w, int h, int kind, int isx, int isy,
                                   const pc_area_tab* xt, const int32_t* xs, int n_x, const pc_area_tab* yt,
                                   const int32_t* ys, int n_y, uint8_t* d_dst, int dst_pitch, int ow, int oh) {
  if (!c) return PC_ERR_ARG;
  if (!d_gray || !d_dst || w < 1 || h < 1 || w > PC_GAUGE_MAX_SIDE || h > PC_GAUGE_MAX_SIDE || pitch < w || ow < 1 ||
      oh < 1 || ow > w || oh > h || dst_pitch < ow)
    return fail(c, PC_ERR_ARG, "pc_gray_resize_area: bad arguments (1 <= ow <= w <= pitch, 1 <= oh <= h <= 16384, "
                               "dst_pitch >= ow)");
  if (kind == PC_CURATE_FAST) {
    if (isx < 1 || isy < 1 || (long long)ow * isx > w || (long long)oh * isy > h)
      return fail(c, PC_ERR_ARG, "pc_gray_resize_area: integer ratios outside the plane");
    HIPCHK(c, gauge_resize_launch(d_gray, pitch, 1, isx, isy, nullptr, nullptr, nullptr, nullptr, d_dst, dst_pitch, ow, oh,
                                  c->stream));
    return PC_OK;
  }
  if (kind != PC_CURATE_AREA) return fail(c, PC_ERR_ARG, "pc_gray_resize_area: kind is PC_CURATE_FAST or PC_CURATE_AREA");
  if (!xt || !xs || !yt || !ys || n_x <= 0 || n_y <= 0 || !area_table_ok(xt, n_x, xs, ow, w) ||
      !area_table_ok(yt, n_y, ys, oh, h))
    return fail(c, PC_ERR_ARG, "pc_gray_resize_area: INTER_AREA tables out of range");
  auto up16 = [](size_t v) { return (v + 15) & ~size_t(15); };
  const size_t o_xs = up16((size_t)n_x * sizeof(pc_area_tab));
  const size_t o_yt = up16(o_xs + (size_t)(ow + 1) * sizeof(int32_t));
  const size_t o_ys = up16(o_yt + (size_t)n_y * sizeof(pc_area_tab));
  const size_t total = o_ys + (size_t)(oh + 1) * sizeof(int32_t);
  std::vector<char> blob(total, 0);
  memcpy(blob.data(), xt, (size_t)n_x * sizeof(pc_area_tab));
  memcpy(blob.data() + o_xs, xs, (size_t)(ow + 1) * sizeof(int32_t));
  memcpy(blob.data() + o_yt, yt, (size_t)n_y * sizeof(pc_area_tab));
  memcpy(blob.data() + o_ys, ys, (size_t)(oh + 1) * sizeof(int32_t));
  void* dv = nullptr;
  int rc = stage_copy(c, blob.data(), total, &dv);
  if (rc) return rc;
  char* db = (char*)dv;
  HIPCHK(c, gauge_resize_launch(d_gray, pitch, 2, 0, 0, db, (const int*)(db + o_xs), db + o_yt, (const int*)(db + o_ys),
                                d_dst, dst_pitch, ow, oh, c->stream));
  return PC_OK;
}
