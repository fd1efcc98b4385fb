// skyjo_loss.h - learner kernels (included from skyjo_learner.hip after skyjo_batches.h: they reduce with sk_wave_sum).
// The PPO loss head of a learner minibatch: from the policy branch's raw logits, the log-mask and the value output to the loss, its
// statistics and the gradients with respect to the logits and the value - what stands between a model's two outputs and
// optimizer.step().  include/skyjo_vec.h (skyjo_vec_ppo_loss) and DESIGN.md 4 have the definition; tests/ppo_loss_ref.py restates it.
//
// (a) k_ppo_loss: a workgroup owns SK_LOSS_ROWS consecutive rows.  It fetches their logits and log-mask stretches as 16-byte pieces
//     (the run starts on a 16-byte boundary and, SK_LOSS_ROWS being even, is a whole number of pieces but for the last run's tail,
//     which is read dword by dword) and keeps ONE image in LDS: z = logits + log_mask, row i at dword i * SK_LOSS_STRIDE.  The stride
//     is 27, not 26: ds_read_b32 serves 32 lanes per cycle out of 32 banks, and 26 i mod 32 meets every bank twice.  Lane i then
//     does row i in float32 - max-subtracted softmax, ratio, clipped surrogate, entropy, value loss - writes the 26 gradients over
//     its z and the value gradient to its column; the image leaves as 16-byte stores over the run's flat [rows * 26] stretch, the
//     shape of k_gather_rows' float outputs.  A row's loss terms, kl and clip bit are widened to double, a wavefront sums them by
//     sk_wave_sum's xor tree, thread 0 adds the wavefronts in order: partial[6 b .. 6 b + 5].  No atomics, no private segment.
// (b) k_ppo_loss_finish, ONE workgroup: thread t owns a contiguous span of blocks, then the wavefront's tree, then the wavefronts in
//     order (k_select_scan's order), divided by m: stats[0 .. 5] = loss, policy_loss, vf_loss, entropy, kl, clip_fraction.
//     The same input gives the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/skyjo_vec.h"

#define SK_LOSS_ROWS 128     // even: a run's byte length (rows * 104) is a multiple of 16
#define SK_LOSS_THREADS 128  // one lane per row
#define SK_LOSS_WAVES (SK_LOSS_THREADS / 64)
#define SK_LOSS_STRIDE 27    // dwords between the rows of the LDS image (odd: conflict-free for one lane per row)
#define SK_LOSS_STATS 6
#define SK_LOSS_FIN_THREADS 1024

struct SkLossArgs {
  const float *logits, *log_mask;  // [m][26], 16-byte aligned
  const float *value;              // [m]
  const long long *actions;        // [m], each in [0, 26)
  const float *logp_old, *adv, *vt, *v_old;
  float *g_logits;                 // [m][26], 16-byte aligned
  float *g_value;                  // [m]
  double *partial;                 // [blocks][6]
  long long m;
  float lo, hi;                    // 1 - clip, 1 + clip (rounded once from double)
  float vf_coef, ent_coef, vf_clip;  // vf_clip <= 0: no value clipping
  float inv_m;
};

__global__ __launch_bounds__(SK_LOSS_THREADS) void k_ppo_loss(SkLossArgs a) {
  __shared__ float zs[SK_LOSS_ROWS * SK_LOSS_STRIDE];
  __shared__ double wsum[SK_LOSS_WAVES][SK_LOSS_STATS];
  constexpr int K = SKYJO_NUM_ACTIONS;
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * SK_LOSS_ROWS;
  const int rows = a.m - o0 < SK_LOSS_ROWS ? (int)(a.m - o0) : SK_LOSS_ROWS;
  const int total = rows * K;

  {  // z = logits + log_mask into the image
    const float *lg = a.logits + o0 * K, *lm = a.log_mask + o0 * K;
    for (int e = tid * 4; e < total; e += SK_LOSS_THREADS * 4) {
      float x[4], y[4];
      if (e + 4 <= total) {
        const float4 u = *(const float4 *)(lg + e), v = *(const float4 *)(lm + e);
        x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w;
        y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          x[j] = e + j < total ? lg[e + j] : 0.f;
          y[j] = e + j < total ? lm[e + j] : 0.f;
        }
      }
      int i = e / K, k = e - i * K;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (e + j < total) zs[i * SK_LOSS_STRIDE + k] = x[j] + y[j];
        if (++k == K) k = 0, i++;
      }
    }
  }
  __syncthreads();

  double st[SK_LOSS_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (tid < rows) {
    const long long o = o0 + tid;
    float *zr = zs + tid * SK_LOSS_STRIDE;
    const long long act = a.actions[o];
    const int ai = (unsigned long long)act < (unsigned long long)K ? (int)act : 0;  // (the precondition; never out of the image)
    const float lp_old = a.logp_old[o], A = a.adv[o], v = a.value[o], vt = a.vt[o], vo = a.v_old[o];
    float z[K];
#pragma unroll
    for (int k = 0; k < K; k++) z[k] = zr[k];
    float M = z[0];
#pragma unroll
    for (int k = 1; k < K; k++) M = fmaxf(M, z[k]);
    float p[K], S = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) {
      z[k] -= M;
      p[k] = expf(z[k]);
      S += p[k];
    }
    const float logS = logf(S);
    float H = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) {
      p[k] /= S;
      z[k] -= logS;  // logp_k
      if (p[k] > 0.f) H -= p[k] * z[k];
    }
    const float lp = (zr[ai] - M) - logS;
    const float r = expf(lp - lp_old);
    const float pl = -fminf(r * A, fminf(fmaxf(r, a.lo), a.hi) * A);
    const bool clipped = (A > 0.f && r > a.hi) || (A < 0.f && r < a.lo);
    // -g r (delta_ka - p_k) with 1 - p_a taken as the sum of the others: a chosen action whose p rounds to 1 keeps its gradient,
    // and the 26 terms of a row sum to 0 within their roundings
    const float gs = a.inv_m * (clipped ? 0.f : A * r), es = a.inv_m * a.ent_coef;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < K; k++) q += k == ai ? 0.f : p[k];
#pragma unroll
    for (int k = 0; k < K; k++) {
      float g = k == ai ? -(gs * q) : gs * p[k];
      if (p[k] > 0.f) g += es * (p[k] * (z[k] + H));
      else if (k != ai) g = 0.f;
      zr[k] = g;
    }
    const float d1 = v - vt;
    float vl = d1 * d1, d = 2.f * d1;
    if (a.vf_clip > 0.f) {
      const float dv = v - vo;
      const float vc = vo + fminf(fmaxf(dv, -a.vf_clip), a.vf_clip);
      const float d2 = vc - vt, vl2 = d2 * d2;
      if (fabsf(dv) > a.vf_clip && !(vl >= vl2)) d = 0.f;
      vl = fmaxf(vl, vl2);
    }
    a.g_value[o] = a.inv_m * (a.vf_coef * d);
    st[1] = (double)pl, st[2] = (double)vl, st[3] = (double)H;
    st[0] = (st[1] + (double)a.vf_coef * st[2]) - (double)a.ent_coef * st[3];
    st[4] = (double)lp_old - (double)lp;
    st[5] = clipped ? 1.0 : 0.0;
  }
#pragma unroll
  for (int j = 0; j < SK_LOSS_STATS; j++) st[j] = sk_wave_sum(st[j]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < SK_LOSS_STATS; j++) wsum[tid >> 6][j] = st[j];
  }
  __syncthreads();
  if (tid < SK_LOSS_STATS) {
    double s = wsum[0][tid];
    for (int w = 1; w < SK_LOSS_WAVES; w++) s += wsum[w][tid];
    a.partial[(size_t)blockIdx.x * SK_LOSS_STATS + tid] = s;
  }

  {  // the gradients, out of the image
    float *dst = a.g_logits + o0 * K;
    for (int e = tid * 4; e < total; e += SK_LOSS_THREADS * 4) {
      int i = e / K, k = e - i * K;
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        x[j] = e + j < total ? zs[i * SK_LOSS_STRIDE + k] : 0.f;
        if (++k == K) k = 0, i++;
      }
      if (e + 4 <= total) {
        *(float4 *)(dst + e) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (e + j < total) dst[e + j] = x[j];
      }
    }
  }
}

__global__ __launch_bounds__(SK_LOSS_FIN_THREADS) void k_ppo_loss_finish(const double *partial, int nb, double m, double *stats_out) {
  __shared__ double wsum[SK_LOSS_FIN_THREADS / 64][SK_LOSS_STATS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (nb + SK_LOSS_FIN_THREADS - 1) / SK_LOSS_FIN_THREADS;
  const long long lo_ = (long long)t * per;
  const int lo = lo_ < nb ? (int)lo_ : nb, hi = lo + per < nb ? lo + per : nb;
  double s[SK_LOSS_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = lo; i < hi; i++) {
#pragma unroll
    for (int j = 0; j < SK_LOSS_STATS; j++) s[j] += partial[(size_t)i * SK_LOSS_STATS + j];
  }
#pragma unroll
  for (int j = 0; j < SK_LOSS_STATS; j++) s[j] = sk_wave_sum(s[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < SK_LOSS_STATS; j++) wsum[w][j] = s[j];
  }
  __syncthreads();
  if (t < SK_LOSS_STATS) {
    double x = 0.0;
    for (int i = 0; i < SK_LOSS_FIN_THREADS / 64; i++) x += wsum[i][t];
    stats_out[t] = x / m;
  }
}
