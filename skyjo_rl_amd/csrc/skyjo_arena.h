// skyjo_arena.h - learner-unit kernels (included from skyjo_learner.hip).
// The evaluation path beside the training rollout: every SEAT of a game has a policy of its own - a net that is sampled, a net that
// is played greedily, or the uniform draw over the legal actions - and the episode-end columns of a buffer become per-seat results.
// include/skyjo_vec.h (skyjo_vec_arena_*, skyjo_vec_episode_stats) and DESIGN.md 4 have the definitions; tests/arena_ref.py restates
// the greedy rule and the statistics.
//
// (a) k_arena<false>: one lane per game, 256 games per workgroup (k_sample's shape).  The lane reads its game's agent byte - with a
//     sk_rec_byte call of its own, never through a pointer to a neighbouring byte: for the direct observation with four players the
//     bytes Dp + 26 and Dp + 28 lie in different 16-byte pieces - and the seven mask words, and looks up the seat's kind and net.  The
//     logits of net j lie as [B][26] floats in slice j of the workspace (one full-batch launch of the net per distinct net wrote them).
//     For every net that SOME lane of the workgroup plays (a workgroup-uniform test: a ballot per wavefront, the four answers or-ed
//     through LDS) the workgroup's 256 x 26 contiguous floats are staged in LDS with 16-byte loads, and the lanes of that net copy
//     their row into registers.  Then
//       SKYJO_SEAT_SAMPLE   sk_draw_action on the row                       (the bits of k_sample and of the net's own epilogue)
//       SKYJO_SEAT_RANDOM   sk_draw_action on 26 zeros                      (uniform over the legal actions)
//       SKYJO_SEAT_GREEDY   the smallest k that maximises m[k] = logits[k] + (legal ? 0 : FLOAT_MIN): sk_draw_action's m, no random number
//     26.6 KB of LDS, no atomics, no private segment (the seats' kinds and nets are bit fields, not arrays that a lane would index).
// (b) k_episode_stats / k_episode_stats_finish: over the rows (t, game) of the final_rewards / episode_end columns, the number of rows
//     that ended an episode and per seat the sum of its final reward over them, the sum of the squares and the number of rows in which
//     the seat holds the row's maximum (a tie counts for every tied seat).  A lane owns SK_STAT_ITERS rows; their maxima stay in
//     registers while the seats are walked one after the other.  Every term is a double; a lane adds its rows in order, a wavefront
//     by sk_wave_sum's xor tree, thread 0 the wavefronts in order: partial[b][1 + 3 N].  The finish kernel, ONE workgroup: thread t
//     owns a contiguous span of blocks, then the tree, then the wavefronts in order (k_ppo_loss_finish's order).  No atomics: the same
//     input gives the same bits on every call.  The rewards are read only where episode_end is set.
// (c) k_arena<true>: (a), and what a learner needs of the acting seat - the iteration of skyjo_vec_arena_act / _collect.  One body:
//     every addition sits behind `if constexpr (ACT)`, and the actions are those of <false> for the same (seats, records, seed, ticket).
//     logp[g] = (m[a] - mx) - __logf(sum) of the chosen action a under the seat's masked distribution: a sampled and a random seat (26
//     zero logits: -log(number of legal actions)) take it from sk_draw_action itself, a greedy seat from sk_logp_at at its argmax.
//     values_out[g] = output 0 of the acting seat's VALUE net on this record: the host ran one full-batch forward per distinct value
//     net into slice j of `values` ([n] floats each, rounded up to 16 bytes), the lane reads its seat's slice at g - one coalesced
//     load, nothing is staged - and a seat without a value net writes 0.0f.  actions == null: the values only (the bootstrap row of a
//     buffer); no logits are read then.  The seats' value nets are a bit field like their policy nets: no private segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/skyjo_vec.h"
#include "skyjo_draw.h"
#include "skyjo_layout.h"
#include "skyjo_learner_util.h"

#define SK_ARENA_BLOCK 256  // games per workgroup: 256 x 26 floats of one net are one contiguous, 16-byte aligned stretch
#define SK_ARENA_NO_VNET 15u
static_assert(SKYJO_MAX_PLAYERS <= SK_ARENA_NO_VNET, "a seat's value net is a 4-bit field whose largest value means none");

// a net's slice of the workspace, in floats: [B][26] (a value net's: [B]), rounded up to whole 16-byte pieces so that every slice starts on one
__host__ __device__ static inline long long sk_arena_slice(long long B) { return (B * SKYJO_NUM_ACTIONS + 3) & ~3LL; }
__host__ __device__ static inline long long sk_arena_vslice(long long B) { return (B + 3) & ~3LL; }

struct SkArenaArgs {
  const uint8_t *rec;    // one iteration's records, either layout
  const float *logits;   // [nets] slices of sk_arena_slice(n) floats; null when no seat has a net
  int32_t *actions;      // [n]; k_arena<true>: null for the values only
  long long n;           // games
  uint64_t seed, ticket, game_id0;
  int32_t Dp, rec_bytes, planar, N, nets;
  uint32_t kinds;        // seat s: bits 2 s, 2 s + 1 = SKYJO_SEAT_*
  uint64_t seat_net;     // seat s: bits 4 s .. 4 s + 3 = its net's slice (unused for SKYJO_SEAT_RANDOM)
  // k_arena<true> only
  float *logp;           // [n]; null iff actions is
  float *values_out;     // [n]
  const float *values;   // [value nets] slices of sk_arena_vslice(n) floats; null when no seat has a value net
  uint64_t seat_vnet;    // seat s: bits 4 s .. 4 s + 3 = its value net's slice, SK_ARENA_NO_VNET: none
};

// The log-probability of action `act` under the masked distribution of `row`: sk_draw_action's m, mx and sum - masked logits, the
// exponentials summed in blocks of four, the block totals left to right - and its closing expression, without the draw.  For the action
// sk_draw_action returns on the same row and mask these are the bits it writes to *logp_out.
__device__ __forceinline__ float sk_logp_at(const float *row, const uint32_t *mw, int act) {
  float m[SKYJO_NUM_ACTIONS], mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < SKYJO_NUM_ACTIONS; k++) {
    const bool on = ((mw[k >> 2] >> ((k & 3) * 8)) & 0xffu) != 0;
    m[k] = on ? row[k] : row[k] + SK_DRAW_FLOAT_MIN;
    mx = fmaxf(mx, m[k]);
  }
  constexpr int NB = (SKYJO_NUM_ACTIONS + 3) / 4;
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    float b = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (4 * j + i < SKYJO_NUM_ACTIONS) {
        const float e = __expf(m[4 * j + i] - mx);
        b = i ? b + e : e;
      }
    sum = sum + b;
  }
  float ma = m[0];
#pragma unroll
  for (int k = 1; k < SKYJO_NUM_ACTIONS; k++) ma = act == k ? m[k] : ma;
  return (ma - mx) - __logf(sum);
}

template <bool ACT>
__global__ __launch_bounds__(SK_ARENA_BLOCK) void k_arena(SkArenaArgs a) {
  __shared__ float rows[SK_ARENA_BLOCK * SKYJO_NUM_ACTIONS];
  __shared__ uint32_t wplayed[SK_ARENA_BLOCK / 64];
  constexpr int K = SKYJO_NUM_ACTIONS;
  const int tid = threadIdx.x;
  const long long g0 = (long long)blockIdx.x * SK_ARENA_BLOCK;
  const int nb = (int)(a.n - g0 < SK_ARENA_BLOCK ? a.n - g0 : SK_ARENA_BLOCK);
  const bool live = tid < nb;
  const long long g = g0 + tid;
  const bool acting = !ACT || a.actions != nullptr;  // (a kernel argument: the same answer in every lane)
  uint32_t mw[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};  // 26 mask bytes from offset Dp (4-byte aligned: a word never straddles two 16-byte pieces)
  int kind = SKYJO_SEAT_RANDOM, mine = -1;
  if (live) {
    if (acting) {
#pragma unroll
      for (int k = 0; k < 7; k++) mw[k] = *(const uint32_t *)sk_rec_byte(a.rec, g, a.Dp + 4 * k, a.rec_bytes, a.planar);
    }
    int seat = (int)*sk_rec_byte(a.rec, g, a.Dp + 26, a.rec_bytes, a.planar);
    seat = seat < a.N ? seat : 0;  // (a record the engine wrote never says otherwise)
    if constexpr (ACT) {
      const uint32_t vn = (uint32_t)((a.seat_vnet >> (4 * seat)) & 15u);
      a.values_out[g] = vn == SK_ARENA_NO_VNET ? 0.0f : a.values[(long long)vn * sk_arena_vslice(a.n) + g];
    }
    if (acting) {
      kind = (int)((a.kinds >> (2 * seat)) & 3u);
      mine = kind == SKYJO_SEAT_RANDOM ? -1 : (int)((a.seat_net >> (4 * seat)) & 15u);
    }
  }
  if (!acting) return;  // (workgroup-uniform: no lane is left waiting at a barrier below)
  float row[K];
#pragma unroll
  for (int k = 0; k < K; k++) row[k] = 0.f;
  // which nets the workgroup's lanes play: a wavefront's by ballot, the four wavefronts' through 16 bytes of LDS
  uint32_t played = 0u;
  for (int j = 0; j < a.nets; j++) played |= __ballot(mine == j) != 0ull ? 1u << j : 0u;
  if ((tid & 63) == 0) wplayed[tid >> 6] = played;
  __syncthreads();
  played = (wplayed[0] | wplayed[1]) | (wplayed[2] | wplayed[3]);
  const int words = nb * K;
  for (int j = 0; j < a.nets; j++) {
    if (!((played >> j) & 1u)) continue;  // (the same answer in every lane of the workgroup)
    __syncthreads();                      // (the lanes of the net before have their rows)
    const float *src = a.logits + (long long)j * sk_arena_slice(a.n) + g0 * K;  // (16-byte aligned: the slice is, and 256 * 26 * 4 bytes are)
    for (int w = tid * 4; w < words; w += SK_ARENA_BLOCK * 4) {
      if (w + 4 <= words) {
        const float4 v = *(const float4 *)(src + w);
        rows[w] = v.x, rows[w + 1] = v.y, rows[w + 2] = v.z, rows[w + 3] = v.w;
      } else {
        for (int k = w; k < words; k++) rows[k] = src[k];
      }
    }
    __syncthreads();
    if (mine == j) {
#pragma unroll
      for (int k = 0; k < K; k++) row[k] = rows[tid * K + k];
    }
  }
  if (!live) return;
  int act;
  [[maybe_unused]] float lp;
  if (kind == SKYJO_SEAT_GREEDY) {
    float best = 0.f;
    act = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
      const bool on = ((mw[k >> 2] >> ((k & 3) * 8)) & 0xffu) != 0;
      const float m = on ? row[k] : row[k] + SK_DRAW_FLOAT_MIN;
      if (k == 0 || m > best) best = m, act = k;
    }
    if constexpr (ACT) lp = sk_logp_at(row, mw, act);
  } else {
    act = sk_draw_action(row, mw, 0, a.seed, a.ticket, a.game_id0 + (uint64_t)g, ACT ? &lp : nullptr, nullptr);
  }
  a.actions[g] = act;
  if constexpr (ACT) a.logp[g] = lp;
}

#define SK_STAT_THREADS 256
#define SK_STAT_WAVES (SK_STAT_THREADS / 64)
#define SK_STAT_ITERS 4                              // rows per lane
#define SK_STAT_ROWS (SK_STAT_THREADS * SK_STAT_ITERS)  // a block's: row  b * SK_STAT_ROWS + k * SK_STAT_THREADS + tid
#define SK_STAT_FIN_THREADS 1024

__global__ __launch_bounds__(SK_STAT_THREADS) void k_episode_stats(const double *rew, const uint8_t *end, long long rows, int N, double *partial) {
  __shared__ double wsum[SK_STAT_WAVES][3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const long long r0 = (long long)blockIdx.x * SK_STAT_ROWS + tid;
  const int S = 1 + 3 * N;
  double *out = partial + (size_t)blockIdx.x * S;
  bool on[SK_STAT_ITERS];
  double mx[SK_STAT_ITERS];
  double cnt = 0.0;
#pragma unroll
  for (int k = 0; k < SK_STAT_ITERS; k++) {
    const long long r = r0 + (long long)k * SK_STAT_THREADS;
    on[k] = r < rows && end[r] != 0;
    mx[k] = 0.0;
    if (on[k]) {
      const double *x = rew + r * N;
      mx[k] = x[0];
      for (int s = 1; s < N; s++) mx[k] = x[s] > mx[k] ? x[s] : mx[k];
      cnt += 1.0;
    }
  }
  for (int s = -1; s < N; s++) {  // s = -1: the count
    double v0 = cnt, v1 = 0.0, v2 = 0.0;
    if (s >= 0) {
      v0 = 0.0;
#pragma unroll
      for (int k = 0; k < SK_STAT_ITERS; k++) {
        if (on[k]) {
          const double x = rew[(r0 + (long long)k * SK_STAT_THREADS) * N + s];
          v0 += x;
          v1 += x * x;
          v2 += x == mx[k] ? 1.0 : 0.0;
        }
      }
    }
    v0 = sk_wave_sum(v0), v1 = sk_wave_sum(v1), v2 = sk_wave_sum(v2);
    if (lane == 0) wsum[w][0] = v0, wsum[w][1] = v1, wsum[w][2] = v2;
    __syncthreads();
    if (tid < (s < 0 ? 1 : 3)) {
      double x = wsum[0][tid];
      for (int i = 1; i < SK_STAT_WAVES; i++) x += wsum[i][tid];
      out[s < 0 ? 0 : 1 + 3 * s + tid] = x;
    }
    __syncthreads();
  }
}

// stats_out[0] = the count, then per seat s: [1 + 3 s] the sum, [2 + 3 s] the sum of squares, [3 + 3 s] the wins
__global__ __launch_bounds__(SK_STAT_FIN_THREADS) void k_episode_stats_finish(const double *partial, int nb, int N, double *stats_out) {
  __shared__ double wsum[SK_STAT_FIN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int S = 1 + 3 * N;
  const int per = (nb + SK_STAT_FIN_THREADS - 1) / SK_STAT_FIN_THREADS;
  const long long lo_ = (long long)t * per;
  const int lo = lo_ < nb ? (int)lo_ : nb, hi = lo + per < nb ? lo + per : nb;
  for (int j = 0; j < S; j++) {
    double s = 0.0;
    for (int i = lo; i < hi; i++) s += partial[(size_t)i * S + j];
    s = sk_wave_sum(s);
    if (lane == 0) wsum[w] = s;
    __syncthreads();
    if (t == 0) {
      double x = 0.0;
      for (int i = 0; i < SK_STAT_FIN_THREADS / 64; i++) x += wsum[i];
      stats_out[j] = x;
    }
    __syncthreads();
  }
}
