// skyjo_host.h - what the two host-side units of libskyjo_vec.so share, and nothing else: the environment engine (skyjo_capi.hip) and
// the packed nets + learner (skyjo_learner.hip).  Both sit behind the one extern "C" boundary of include/skyjo_vec.h; everything
// declared here has hidden visibility or is inline, so the library exports what the header declares and no more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/skyjo_vec.h"
#include "skyjo_layout.h"
#include "skyjo_policy.h"

#define SK_HIDDEN __attribute__((visibility("hidden")))

// ---- the error state: ONE thread_local message for the whole library (defined in skyjo_capi.hip, read by skyjo_vec_last_error) ----
SK_HIDDEN int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(SKYJO_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));             \
  } while (0)

// Every entry point that takes a handle runs on the handle's device, whatever the calling thread's current device is
// (a second thread starts on device 0; torch.cuda.set_device may have switched it), and leaves the caller's current
// device as it found it.
struct SK_HIDDEN DevGuard {
  int prev = -1;
  bool switched = false;
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DevGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

struct SK_HIDDEN DevBuf {  // a scratch allocation that frees itself
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// the `layout` argument of every entry point that reads records in either form
static inline int check_layout(int32_t layout) {
  if (layout != SKYJO_REC_ROW_MAJOR && layout != SKYJO_REC_TILE_PLANAR) return fail(SKYJO_E_INVALID, "layout must be SKYJO_REC_ROW_MAJOR or SKYJO_REC_TILE_PLANAR");
  return SKYJO_OK;
}

// ---- a packed net.  The learner unit makes, rewrites and frees it; the engine's skyjo_vec_model_rollout reads net, obs_dim, out_dim
// and device_id.  (k_mlp_update's view of the blob is derived from these when a call needs it: skyjo_learner.hip, mlp_update_args) ----
struct skyjo_vec_mlp {
  SkMlpDev net{};
  void *blob = nullptr;
  int device_id = 0, obs_dim = 0, out_dim = 0;
};

// One launch of the policy net (nets == 2: policy and value branch over the same records, grid.y = 2) in the net's precision
// (the kernels live in skyjo_policy.hip).  `planar`: the records lie tile-planar (SKYJO_REC_TILE_PLANAR).
// e0 / e1: the events that time the kernel (the engine's skyjo_vec_profile, slot 4), or null.
static inline int launch_mlp(const skyjo_vec_mlp *ma, const skyjo_vec_mlp *mb, int nets, const uint8_t *rec, int rec_bytes, int obs_dim, int64_t n, float *out_a,
                             const SkMlpDraw &draw, float *out_b, hipStream_t s, int planar, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  SkMlpRecords r;
  r.base = rec, r.rec_bytes = rec_bytes, r.obs_dim = obs_dim, r.planar = planar, r.n = (long long)n;
  HIPCHK((hipError_t)sk_launch_mlp(ma->net, mb->net, nets, r, out_a, draw, out_b, s, e0, e1));
  return SKYJO_OK;
}

// ---- the engine as the learner unit sees it (struct skyjo_vec itself is private to skyjo_capi.hip, which defines both functions) ----
struct SkEngineView {
  int device_id;
  int32_t B;          // games
  size_t G;           // tiles * 64: the record slots of one step of a tile-planar buffer
  uint64_t game_id0;
  const SkLayout *L;  // the handle's own copy: valid as long as the handle
};
SK_HIDDEN SkEngineView sk_engine_view(const skyjo_vec *h);

// skyjo_vec_rollout_select's scratch: one allocation of the handle that only grows (at least 64 blocks; a call that needs more frees
// and re-allocates, which waits for whatever still reads the old one).  Per block of SK_SEL_ROWS rows its count / exclusive offset
// (8 bytes), then two partial sums (16 bytes): `*cap_out` blocks at `*scratch_out`.  Freed by skyjo_vec_destroy; not part of a snapshot.
SK_HIDDEN int sk_engine_select_scratch(skyjo_vec *h, size_t blocks, void **scratch_out, size_t *cap_out);
