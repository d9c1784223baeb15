// lk_engine_images.cpp - the image slots of the engine: upload (or device copy) of a frame, its pyramid levels, pinning,
// the pair and rotate calls, lk_get_pyramid_level.
#include "lk_engine_state.hpp"

// level buffers of one slot for a rows x cols frame (+ two zeroed guard rows per level; the
// pyramid kernels write every target pixel themselves, so the guard rows are only redone when
// the geometry of the level changes)
static int prepare_slot(lk_engine *e, DevImage &im, int rows, int cols, hipStream_t st) {
  int r = rows, c = cols;
  for (int l = 0; l <= e->cfg.py_stop; ++l) {
    size_t need = (size_t)(r + 2) * (size_t)c + 16;
    if (need > im.cap[l]) {
      if (im.lvl[l]) {
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipFree(im.lvl[l]));
        im.lvl[l] = nullptr;
      }
      HIPCHK(hipMalloc((void **)&im.lvl[l], need));
      im.cap[l] = need;
      im.guard_rows[l] = -1;
    }
    if (im.guard_rows[l] != r || im.guard_cols[l] != c) {
      HIPCHK(hipMemsetAsync(im.lvl[l] + (size_t)r * (size_t)c, 0, 2 * (size_t)c + 16, st));
      im.guard_rows[l] = r;
      im.guard_cols[l] = c;
    }
    r /= 2;
    c /= 2;
  }
  return LK_ERROR_NONE;
}

// Is a host pointer pinned (hipHostMalloc / hipHostRegister: lk_pin_host_memory)?  A copy from pinned memory is a DMA the
// stream orders; from pageable memory the runtime stages it, and the caller's buffer is only safe once the stream has
// passed the copy.
bool host_pinned(const void *p) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError(); // (pageable memory: not an error of ours)
    return false;
  }
  return a.type == hipMemoryTypeHost;
}

// upload (or device copy) of one frame into `im` + its pyramid levels, on stream `st`
int fill_image(lk_engine *e, DevImage &im, const void *src, bool src_on_device, int rows, int cols, int step, hipStream_t st,
               bool timed) {
  {
    int rc = prepare_slot(e, im, rows, cols, st);
    if (rc)
      return rc;
  }
  int r = rows, c = cols;
  // two or more pyramid levels on a device-resident frame: upload copy + levels 1, 2 in ONE
  // launch (lk_pyramid2_kernel); host frames are copied first and the kernel runs in place
  const bool fused = e->cfg.py_stop >= 2 && rows >= 4 && cols >= 4;
  if (!fused || !src_on_device)
    HIPCHK(hipMemcpy2DAsync(im.lvl[0], (size_t)cols, src, (size_t)step, (size_t)cols, (size_t)rows,
                            src_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (timed)
    HIPCHK(hipEventRecord(e->ev_p0, st));
  r = rows;
  c = cols;
  int l = 1;
  if (fused) {
    const bool in_place = !src_on_device;
    const uint8_t *srcs[1] = {in_place ? im.lvl[0] : (const uint8_t *)src};
    const int steps[1] = {in_place ? cols : step};
    HIPCHK(lk_launch_pyramid2(1, srcs, steps, rows, cols, &im.lvl[0], &im.lvl[1], &im.lvl[2], st));
    r = rows / 4;
    c = cols / 4;
    l = 3;
  }
  for (; l <= e->cfg.py_stop; ++l) { // (remaining) levels up to stop (pyramid_class.cpp:92)
    HIPCHK(lk_launch_pyramid(im.lvl[l - 1], r, c, im.lvl[l], st));
    r /= 2;
    c /= 2;
  }
  if (timed) {
    HIPCHK(hipEventRecord(e->ev_p1, st));
    e->pyr_timed = true;
  }
  im.rows = rows;
  im.cols = cols;
  im.valid = true;
  return LK_ERROR_NONE;
}

// after / consumed (lk_group: frames that arrive by a collective on another stream): the fill waits for `after` on its
// stream instead of the host waiting for the collective, and `consumed` is recorded behind the last kernel that reads src
static int set_image_common(lk_engine *e, int slot, const void *src, bool src_on_device, int rows,
                            int cols, int step, hipEvent_t after = nullptr, hipEvent_t consumed = nullptr) {
  Range range_("lk:upload+pyramid");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (slot < 0 || slot > 2 || !src || rows < 1 || cols < 1 || step < cols)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_image: bad arguments");
  HIPCHK(hipSetDevice(e->cfg.device));
  // the next-frame slot is filled on its own stream so it can overlap a running solve
  // (manager_class.cpp:1438-1447 / nxtStream in cuda_pyramid.cu:504,557)
  std::unique_lock<std::mutex> lock(e->nxt_mu, std::defer_lock);
  hipStream_t st = e->stream;
  if (slot == LK_IMG_NXT) {
    lock.lock();
    st = e->nxt_stream;
  }
  DevImage &im = e->img[slot];
  if (after)
    HIPCHK(hipStreamWaitEvent(st, after, 0));
  {
    int rc = fill_image(e, im, src, src_on_device, rows, cols, step, st, slot != LK_IMG_NXT && e->timing);
    if (rc)
      return rc;
  }
  if (consumed)
    HIPCHK(hipEventRecord(consumed, st));
  if (slot == LK_IMG_NXT) {
    HIPCHK(hipEventRecord(e->nxt_done, st));
    e->nxt_pending = true;
  } else {
    e->lv_dirty = true;
  }
  if (!src_on_device && !host_pinned(src)) // pageable host memory: the copy must have left it
    HIPCHK(hipStreamSynchronize(st));
  return LK_ERROR_NONE;
}

int lk_pin_host_memory(void *ptr, size_t bytes) {
  if (!ptr || !bytes)
    return LK_ERROR_BAD_DOMAIN;
  return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? LK_ERROR_NONE : LK_ERROR_DEVICE;
}
int lk_unpin_host_memory(void *ptr) {
  if (!ptr)
    return LK_ERROR_BAD_DOMAIN;
  return hipHostUnregister(ptr) == hipSuccess ? LK_ERROR_NONE : LK_ERROR_DEVICE;
}

int lk_set_image(lk_engine *e, int slot, const uint8_t *host_pixels, int rows, int cols, int step) {
  return set_image_common(e, slot, host_pixels, false, rows, cols, step);
}

int lk_set_image_device(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step) {
  return set_image_common(e, slot, device_pixels, true, rows, cols, step);
}

int lk_internal_set_image_device_after(lk_engine *e, int slot, const void *device_pixels, int rows, int cols, int step,
                                       hipEvent_t after, hipEvent_t consumed) {
  return set_image_common(e, slot, device_pixels, true, rows, cols, step, after, consumed);
}

static void swap_images(DevImage &a, DevImage &b) { std::swap(a, b); }

// CudaClass::resetImagePyramids takes the frames of a pair together (cuda_class.cu:475-519);
// for device-resident frames both uploads and both pairs of pyramid levels share ONE launch.
int lk_set_image_pair_device(lk_engine *e, const void *und_pixels, int und_step, const void *def_pixels,
                             int def_step, int rows, int cols) {
  Range range_("lk:upload+pyramid pair");
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!und_pixels || !def_pixels || rows < 1 || cols < 1 || und_step < cols || def_step < cols)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_set_image_pair_device: bad arguments");
  if (e->cfg.py_stop < 2 || rows < 4 || cols < 4) { // nothing to fuse
    int rc = set_image_common(e, LK_IMG_UND, und_pixels, true, rows, cols, und_step);
    return rc ? rc : set_image_common(e, LK_IMG_DEF, def_pixels, true, rows, cols, def_step);
  }
  HIPCHK(hipSetDevice(e->cfg.device));
  hipStream_t st = e->stream;
  DevImage &u = e->img[LK_IMG_UND], &d = e->img[LK_IMG_DEF];
  int rc = prepare_slot(e, u, rows, cols, st);
  if (!rc)
    rc = prepare_slot(e, d, rows, cols, st);
  if (rc)
    return rc;
  if (e->timing)
    HIPCHK(hipEventRecord(e->ev_p0, st));
  const uint8_t *srcs[2] = {(const uint8_t *)und_pixels, (const uint8_t *)def_pixels};
  const int steps[2] = {und_step, def_step};
  uint8_t *l0[2] = {u.lvl[0], d.lvl[0]}, *l1[2] = {u.lvl[1], d.lvl[1]}, *l2[2] = {u.lvl[2], d.lvl[2]};
  HIPCHK(lk_launch_pyramid2(2, srcs, steps, rows, cols, l0, l1, l2, st));
  for (DevImage *im : {&u, &d}) {
    int r = rows / 4, c = cols / 4;
    for (int l = 3; l <= e->cfg.py_stop; ++l) {
      HIPCHK(lk_launch_pyramid(im->lvl[l - 1], r, c, im->lvl[l], st));
      r /= 2;
      c /= 2;
    }
    im->rows = rows;
    im->cols = cols;
    im->valid = true;
  }
  if (e->timing) {
    HIPCHK(hipEventRecord(e->ev_p1, st));
    e->pyr_timed = true;
  }
  e->lv_dirty = true;
  return LK_ERROR_NONE;
}

int lk_rotate_und_from_def(lk_engine *e) { // pyramid_class.cpp:211-226: def is emptied
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (!e->img[LK_IMG_DEF].valid)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_rotate_und_from_def: no deformed image");
  swap_images(e->img[LK_IMG_UND], e->img[LK_IMG_DEF]);
  e->img[LK_IMG_DEF].valid = false; // keeps its allocation for reuse
  e->lv_dirty = true;
  return LK_ERROR_NONE;
}

int lk_rotate_def_from_nxt(lk_engine *e) { // pyramid_class.cpp:228-258
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  std::lock_guard<std::mutex> lock(e->nxt_mu);
  if (!e->img[LK_IMG_NXT].valid)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_rotate_def_from_nxt: no next image");
  HIPCHK(hipSetDevice(e->cfg.device));
  if (e->nxt_pending) { // fence: the solve stream must see the finished next pyramid
    HIPCHK(hipStreamWaitEvent(e->stream, e->nxt_done, 0));
    e->nxt_pending = false;
  }
  swap_images(e->img[LK_IMG_DEF], e->img[LK_IMG_NXT]);
  e->img[LK_IMG_NXT].valid = false;
  e->lv_dirty = true;
  return LK_ERROR_NONE;
}

int lk_get_pyramid_level(lk_engine *e, int slot, int level, uint8_t *host_out, int *rows, int *cols) {
  if (!e)
    return LK_ERROR_BAD_DOMAIN;
  if (slot < 0 || slot > 2 || level < 0 || level > e->cfg.py_stop || !e->img[slot].valid)
    return e->fail(LK_ERROR_BAD_DOMAIN, "lk_get_pyramid_level: bad slot/level");
  const DevImage &im = e->img[slot];
  int r = im.rows >> level, c = im.cols >> level;
  if (rows)
    *rows = r;
  if (cols)
    *cols = c;
  if (host_out) {
    HIPCHK(hipSetDevice(e->cfg.device));
    hipStream_t st = slot == LK_IMG_NXT ? e->nxt_stream : e->stream;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(host_out, im.lvl[level], (size_t)r * (size_t)c, hipMemcpyDeviceToHost));
  }
  return LK_ERROR_NONE;
}
