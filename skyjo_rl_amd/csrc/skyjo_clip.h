// skyjo_clip.h - included from skyjo_learner.hip only.  The global L2 norm of a list of float32 tensors and torch's clipping coefficient
// for it, in front of the native Adam: skyjo_vec_grad_norm (k_grad_norm) writes (norm, coef) to two floats on the device, and
// skyjo_vec_mlp_adam_step_clipped (k_mlp_update, skyjo_update.h) reads the coefficient from there.  include/skyjo_vec.h and DESIGN.md 4
// have the definition; tests/grad_clip_ref.py restates it.
//
// (a) k_grad_norm: ONE workgroup of SKC_THREADS threads, one launch.  The job is the twelve gradient tensors of a branch pair, at most
//     about 164 k floats: like k_mlp_update's, its cost is the launch (nobody has timed it).
// (b) The order of the additions is fixed by the segment list alone.  Thread t walks the segments in order; of a segment it takes, in
//     this order, element t of the head (the h < 4 floats in front of the first 16-byte boundary), the 16-byte groups t, t + 1024, ...
//     of the body - the four floats of a group in ascending address - and element t of the tail (the < 4 floats behind the last whole
//     group).  Every square and every addition is double (the unit is compiled with -ffp-contract=off: a product and a sum, two
//     roundings).  Then sk_wave_sum's xor tree per wavefront, and thread 0 adds the sixteen wavefronts in ascending order.  No atomics:
//     the same input gives the same bits on every call.
// (c) The coefficient is torch.nn.utils.clip_grad_norm_'s, operation for operation in float32: torch evaluates its
//     `max_norm / (total_norm + 1e-6)` as `(total_norm + 1e-6).reciprocal() * max_norm` (Tensor.__rtruediv__) - a correctly rounded
//     reciprocal and a product, TWO roundings, which differs from the one division in the last bit for about a quarter of all norms -
//     and clamps it with torch.clamp(max=1), which keeps a NaN.
// (d) The segments are read only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "skyjo_learner_util.h"

#define SKC_THREADS 1024
#define SKC_MAX_SEGMENTS 32

struct SkNormArgs {
  const float *ptr[SKC_MAX_SEGMENTS];  // 4-byte aligned; null only with count 0
  long long count[SKC_MAX_SEGMENTS];   // >= 0
  int n;                               // 1 .. SKC_MAX_SEGMENTS
  float max_norm;                      // > 0; +inf: measure only
  float *out;                          // [2]: norm, coefficient
};

// torch's clip_coef_clamped for a norm (c), in float32
__device__ inline float skc_coef(float norm, float max_norm) {
  if (isinf(max_norm)) return 1.0f;  // measure only, whatever the norm
  const float c = (1.0f / (norm + 1e-6f)) * max_norm;
  return c < 1.0f ? c : (c >= 1.0f ? 1.0f : c);  // (not fminf: a NaN stays a NaN)
}

__global__ __launch_bounds__(SKC_THREADS) void k_grad_norm(SkNormArgs a) {
  __shared__ double wsum[SKC_THREADS / 64];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int k = 0; k < a.n; k++) {
    const float *p = a.ptr[k];
    const long long n = a.count[k];
    if (n <= 0) continue;
    const long long to_boundary = (long long)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
    const long long head = to_boundary < n ? to_boundary : n, groups = (n - head) >> 2, tail = n - head - 4 * groups;
    if (t < head) {
      const double x = (double)p[t];
      s += x * x;
    }
    const float4 *body = (const float4 *)(p + head);
    for (long long i = t; i < groups; i += SKC_THREADS) {
      const float4 q = body[i];
      const double x = (double)q.x, y = (double)q.y, z = (double)q.z, w = (double)q.w;
      s += x * x;
      s += y * y;
      s += z * z;
      s += w * w;
    }
    if (t < tail) {
      const double x = (double)p[head + 4 * groups + t];
      s += x * x;
    }
  }
  s = sk_wave_sum(s);
  if ((t & 63) == 0) wsum[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    double x = wsum[0];
    for (int w = 1; w < SKC_THREADS / 64; w++) x += wsum[w];
    const float norm = (float)sqrt(x);
    a.out[0] = norm;
    a.out[1] = skc_coef(norm, a.max_norm);
  }
}
