// skyjo_loss.h - learner kernels (included from skyjo_learner.hip).
// The PPO loss head of a learner minibatch: from the policy branch's raw logits, the log-mask and the value output to the loss, its
// statistics and the gradients with respect to the logits and the value - what stands between a model's two outputs and
// optimizer.step().  include/skyjo_vec.h (skyjo_vec_ppo_loss) and DESIGN.md 4 have the definition; tests/ppo_loss_ref.py restates it.
//
// (a) k_ppo_loss: a workgroup owns SK_LOSS_ROWS consecutive rows.  It fetches their logits and log-mask stretches as 16-byte pieces
//     (the run starts on a 16-byte boundary and, SK_LOSS_ROWS being even, is a whole number of pieces but for the last run's tail,
//     which is read dword by dword) and keeps ONE image in LDS: z = logits + log_mask, row i at dword i * SK_LOSS_STRIDE.  The stride
//     is 27, not 26: ds_read_b32 serves 32 lanes per cycle out of 32 banks, and 26 i mod 32 meets every bank twice.  Lane i then
//     does row i in DOUBLE from the float32 image - max-subtracted softmax, ratio, clipped surrogate, entropy, value loss; the
//     device's float32 logf has a mean signed error of -7e-08 on 1 <= S <= 26, which does not average out over rows and sat whole in
//     the kl and entropy statistics (EXPERIMENTS); 26 elements a row make the wider arithmetic free - rounds each of the 26 gradients once over
//     its z and the value gradient to its column; the image leaves as 16-byte stores over the run's flat [rows * 26] stretch
//     (sk_store_stretch: the loop of k_gather_rows' float outputs).  A row's loss terms, kl and clip bit are widened to double, a
//     wavefront sums them by sk_wave_sum's xor tree, thread 0 adds the wavefronts in order: partial[6 b .. 6 b + 5].  No atomics, no
//     private segment.
// (b) k_ppo_loss_finish, ONE workgroup: thread t owns a contiguous span of blocks, then the wavefront's tree, then the wavefronts in
//     order (k_select_scan's order), divided by m: stats[0 .. 5] = loss, policy_loss, vf_loss, entropy, kl, clip_fraction.
//     The same input gives the same bits on every call.
// (c) k_ppo_loss<true> (skyjo_vec_ppo_loss_kl) adds the KL penalty against the behaviour distribution.  A SECOND image at the same
//     stride holds zo = old_logits + log_mask (13 824 bytes more, fetched by the same 16-byte walk).  The lane streams its old row
//     out of LDS - once for the maximum, once for the sum, once inside the gradient loop, where po_k and logpo_k are formed, used
//     and dropped - instead of holding a third 26-float array in registers: still no private segment.  A seventh statistic,
//     action_kl, follows the six.  k_ppo_loss<false> is the kernel of (a), statement for statement: every addition sits behind
//     `if constexpr (KL)`, and with kl_coeff == 0 the <true> form adds nothing to a gradient or to the loss - the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/skyjo_vec.h"
#include "skyjo_learner_util.h"

#define SK_LOSS_ROWS 128     // even: a run's byte length (rows * 104) is a multiple of 16
#define SK_LOSS_THREADS 128  // one lane per row
#define SK_LOSS_WAVES (SK_LOSS_THREADS / 64)
#define SK_LOSS_STRIDE 27    // dwords between the rows of the LDS image (odd: conflict-free for one lane per row)
#define SK_LOSS_STATS 6
#define SK_LOSS_KL_STATS 7   // ... and action_kl
#define SK_LOSS_FIN_THREADS 1024

struct SkLossArgs {
  const float *logits, *log_mask;  // [m][26], 16-byte aligned
  const float *old_logits;         // [m][26], 16-byte aligned (k_ppo_loss<true> only)
  const float *value;              // [m]
  const long long *actions;        // [m], each in [0, 26)
  const float *logp_old, *adv, *vt, *v_old;
  float *g_logits;                 // [m][26], 16-byte aligned
  float *g_value;                  // [m]
  double *partial;                 // [blocks][6], <true>: [blocks][7]
  long long m;
  double lo, hi;                   // 1 - clip, 1 + clip, in double from the float32 clip
  float vf_coef, ent_coef, vf_clip;  // vf_clip <= 0: no value clipping
  float kl_coeff;                  // >= 0 (k_ppo_loss<true> only)
};

template <bool KL>
__global__ __launch_bounds__(SK_LOSS_THREADS) void k_ppo_loss(SkLossArgs a) {
  constexpr int NS = KL ? SK_LOSS_KL_STATS : SK_LOSS_STATS;
  __shared__ float zs[SK_LOSS_ROWS * SK_LOSS_STRIDE];
  __shared__ float zos[KL ? SK_LOSS_ROWS * SK_LOSS_STRIDE : 1];  // the old rows' image (unused, and dropped, without KL)
  __shared__ double wsum[SK_LOSS_WAVES][NS];
  constexpr int K = SKYJO_NUM_ACTIONS;
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * SK_LOSS_ROWS;
  const int rows = a.m - o0 < SK_LOSS_ROWS ? (int)(a.m - o0) : SK_LOSS_ROWS;
  const int total = rows * K;

  {  // z = logits + log_mask into the image
    const float *lg = a.logits + o0 * K, *lm = a.log_mask + o0 * K;
    [[maybe_unused]] const float *ol = KL ? a.old_logits + o0 * K : nullptr;
    for (int e = tid * 4; e < total; e += SK_LOSS_THREADS * 4) {
      float x[4], y[4];
      [[maybe_unused]] float xo[4];
      if (e + 4 <= total) {
        const float4 u = *(const float4 *)(lg + e), v = *(const float4 *)(lm + e);
        x[0] = u.x, x[1] = u.y, x[2] = u.z, x[3] = u.w;
        y[0] = v.x, y[1] = v.y, y[2] = v.z, y[3] = v.w;
        if constexpr (KL) {
          const float4 w = *(const float4 *)(ol + e);
          xo[0] = w.x, xo[1] = w.y, xo[2] = w.z, xo[3] = w.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
          x[j] = e + j < total ? lg[e + j] : 0.f;
          y[j] = e + j < total ? lm[e + j] : 0.f;
          if constexpr (KL) xo[j] = e + j < total ? ol[e + j] : 0.f;
        }
      }
      int i = e / K, k = e - i * K;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (e + j < total) {
          zs[i * SK_LOSS_STRIDE + k] = x[j] + y[j];
          if constexpr (KL) zos[i * SK_LOSS_STRIDE + k] = xo[j] + y[j];
        }
        if (++k == K) k = 0, i++;
      }
    }
  }
  __syncthreads();

  double st[NS] = {};
  if (tid < rows) {
    const long long o = o0 + tid;
    float *zr = zs + tid * SK_LOSS_STRIDE;
    const long long act = a.actions[o];
    const int ai = (unsigned long long)act < (unsigned long long)K ? (int)act : 0;  // (the precondition; never out of the image)
    // every float32 input of the row is widened once; the row is evaluated in double and every output rounded once (header)
    const double lp_old = a.logp_old[o], A = a.adv[o], v = a.value[o], vt = a.vt[o], vo = a.v_old[o];
    const double inv_m = 1.0 / (double)a.m, lo = a.lo, hi = a.hi;  // (1 / m is rounded once, in double)
    double z[K];
#pragma unroll
    for (int k = 0; k < K; k++) z[k] = (double)zr[k];
    double M = z[0];
#pragma unroll
    for (int k = 1; k < K; k++) M = fmax(M, z[k]);
    double p[K], S = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) {
      z[k] -= M;
      p[k] = exp(z[k]);
      S += p[k];
    }
    const double logS = log(S);
    double H = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) {
      p[k] /= S;
      z[k] -= logS;  // logp_k
      if (p[k] > 0.0) H -= p[k] * z[k];
    }
    const double lp = ((double)zr[ai] - M) - logS;
    const double r = exp(lp - lp_old);
    const double pl = -fmin(r * A, fmin(fmax(r, lo), hi) * A);
    const bool clipped = (A > 0.0 && r > hi) || (A < 0.0 && r < lo);
    // -g r (delta_ka - p_k) with 1 - p_a taken as the sum of the others: a chosen action whose p rounds to 1 keeps its gradient,
    // and the 26 terms of a row sum to 0 within their roundings
    const double gs = inv_m * (clipped ? 0.0 : A * r), es = inv_m * (double)a.ent_coef;
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < K; k++) q += k == ai ? 0.0 : p[k];
    // the old distribution's maximum, sum and log-sum; its 26 terms are formed again, one at a time, in the gradient loop
    [[maybe_unused]] const float *zor = zos + (KL ? tid * SK_LOSS_STRIDE : 0);
    [[maybe_unused]] double Mo = 0.0, So = 0.0, logSo = 0.0, akl = 0.0;
    [[maybe_unused]] const double ks = inv_m * (double)a.kl_coeff;
    if constexpr (KL) {
      Mo = (double)zor[0];
#pragma unroll
      for (int k = 1; k < K; k++) Mo = fmax(Mo, (double)zor[k]);
#pragma unroll
      for (int k = 0; k < K; k++) So += exp((double)zor[k] - Mo);
      logSo = log(So);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
      double g = k == ai ? -(gs * q) : gs * p[k];
      if (p[k] > 0.0) g += es * (p[k] * (z[k] + H));
      else if (k != ai) g = 0.0;
      if constexpr (KL) {
        // po_k == 0 exactly at a masked k (as p_k): no term there; z[k] = logp_k is finite wherever po_k > 0, also where p_k is 0
        const double zo = (double)zor[k] - Mo, po = exp(zo) / So;
        if (po > 0.0) akl += po * ((zo - logSo) - z[k]);
        if (a.kl_coeff != 0.f) g += ks * (p[k] - po);
      }
      zr[k] = (float)g;
    }
    const double d1 = v - vt;
    double vl = d1 * d1, d = 2.0 * d1;
    if (a.vf_clip > 0.f) {
      const double dv = v - vo, c = (double)a.vf_clip;
      const double vc = vo + fmin(fmax(dv, -c), c);
      const double d2 = vc - vt, vl2 = d2 * d2;
      if (fabs(dv) > c && !(vl >= vl2)) d = 0.0;
      vl = fmax(vl, vl2);
    }
    a.g_value[o] = (float)(inv_m * ((double)a.vf_coef * d));
    st[1] = pl, st[2] = vl, st[3] = H;
    st[0] = (st[1] + (double)a.vf_coef * st[2]) - (double)a.ent_coef * st[3];
    st[4] = lp_old - lp;
    st[5] = clipped ? 1.0 : 0.0;
    if constexpr (KL) {
      st[6] = akl;
      if (a.kl_coeff != 0.f) st[0] += (double)a.kl_coeff * st[6];
    }
  }
#pragma unroll
  for (int j = 0; j < NS; j++) st[j] = sk_wave_sum(st[j]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NS; j++) wsum[tid >> 6][j] = st[j];
  }
  __syncthreads();
  if (tid < NS) {
    double s = wsum[0][tid];
    for (int w = 1; w < SK_LOSS_WAVES; w++) s += wsum[w][tid];
    a.partial[(size_t)blockIdx.x * NS + tid] = s;
  }

  // the gradients, out of the image
  sk_store_stretch<SK_LOSS_THREADS>(a.g_logits + o0 * K, total, K, [&](int i, int k) { return zs[i * SK_LOSS_STRIDE + k]; });
}

template <int NS>  // SK_LOSS_STATS, or SK_LOSS_KL_STATS after k_ppo_loss<true>
__global__ __launch_bounds__(SK_LOSS_FIN_THREADS) void k_ppo_loss_finish(const double *partial, int nb, double m, double *stats_out) {
  __shared__ double wsum[SK_LOSS_FIN_THREADS / 64][NS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (nb + SK_LOSS_FIN_THREADS - 1) / SK_LOSS_FIN_THREADS;
  const long long lo_ = (long long)t * per;
  const int lo = lo_ < nb ? (int)lo_ : nb, hi = lo + per < nb ? lo + per : nb;
  double s[NS] = {};
  for (int i = lo; i < hi; i++) {
#pragma unroll
    for (int j = 0; j < NS; j++) s[j] += partial[(size_t)i * NS + j];
  }
#pragma unroll
  for (int j = 0; j < NS; j++) s[j] = sk_wave_sum(s[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NS; j++) wsum[w][j] = s[j];
  }
  __syncthreads();
  if (t < NS) {
    double x = 0.0;
    for (int i = 0; i < SK_LOSS_FIN_THREADS / 64; i++) x += wsum[i][t];
    stats_out[t] = x / m;
  }
}
