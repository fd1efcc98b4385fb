// skyjo_epoch.h - included from skyjo_learner.hip only.  What a whole PPO update behind one call (skyjo_vec_ppo_update) needs beside the
// stages' own kernels: an epoch's shuffled order without torch (skyjo_vec_rollout_shuffle: k_epoch_order, k_epoch_faults) and the epoch
// statistics summed on the device (k_update_stats).  include/skyjo_vec.h and DESIGN.md 4 have the definitions; tests/epoch_order_ref.py
// restates the permutation.
//
// (a) k_epoch_order: one lane per position j, order_out[j] = index[perm(j)].  perm is a keyed bijection of [0, count): a balanced
//     Feistel network of six rounds on b bits, b the smallest even number >= 2 with 2^b >= count, walked from j until it lands below
//     count (cycle walking: a bijection of [0, 2^b) restricted to the cycles' visits of [0, count) is one of [0, count)).  The domain is
//     smaller than 4 count, so a walk is short; it is CAPPED at SKE_WALK_CAP applications all the same - a loop in a kernel must end -
//     and a lane that hits the cap writes -1, which the gather reads as a row of zeros.  No sort, no atomics, no cross-lane traffic: a
//     pure function of (count, the six keys, j).  All arithmetic is uint32 with wrap-around; the keys come from the host by value.
// (b) k_epoch_faults: ONE workgroup counts the -1 entries of the order just written (integers: no order of addition to fix) and writes
//     the count - no atomic on a hot word.
// (c) k_update_stats: ONE wavefront, launched once after each step's Adam.  Lane i owns accumulator i: a double product and a double
//     add per step (the unit is compiled with -ffp-contract=off), exactly what examples/ppo.py::_epochs does with torch on the device; after
//     an epoch's last step the lanes write the epoch's row.  The quotients are formed as torch forms `tensor / host scalar` on the GPU:
//     times the reciprocal, which the host computes in double - the launcher passes 1 / max(seen, 1) and 1 / steps by value.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SKE_ROUNDS 6
#define SKE_WALK_CAP 1024
#define SKE_ORDER_THREADS 256
#define SKE_FAULT_THREADS 1024
#define SKE_MAX_COUNT ((long long)1 << 30)
#define SKE_ACC 16  // the accumulators of an epoch: SKYJO_UPDATE_STATS sums (column 9: rows seen) and [10] the steps; the rest unused

__host__ __device__ inline uint32_t ske_fmix32(uint32_t v) {
  v ^= v >> 16;
  v *= 0x85EBCA6Bu;
  v ^= v >> 13;
  v *= 0xC2B2AE35u;
  v ^= v >> 16;
  return v;
}

struct SkOrderArgs {
  const long long *index;
  long long *order;
  uint32_t count;  // 1 .. 2^30
  uint32_t h;      // half the domain's bits: 1 .. 15
  uint32_t key[SKE_ROUNDS];
};

// the keys of (seed, epoch) and the half width of count's domain
static inline void ske_plan(uint64_t seed, uint32_t epoch, long long count, SkOrderArgs &a) {
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  for (uint32_t r = 0; r < SKE_ROUNDS; r++) a.key[r] = ske_fmix32(lo ^ ske_fmix32(hi ^ ske_fmix32(epoch * 0x9E3779B9u + r)));
  uint32_t b = 2;
  while (((long long)1 << b) < count) b += 2;
  a.h = b / 2, a.count = (uint32_t)count;
}

__global__ __launch_bounds__(SKE_ORDER_THREADS) void k_epoch_order(SkOrderArgs a) {
  const uint32_t j = blockIdx.x * SKE_ORDER_THREADS + threadIdx.x;
  if (j >= a.count) return;
  const uint32_t h = a.h, mask = (1u << h) - 1u;
  uint32_t x = j;
  bool found = false;
  for (int w = 0; w < SKE_WALK_CAP && !found; w++) {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < SKE_ROUNDS; r++) {
      const uint32_t t = L ^ (ske_fmix32(R + a.key[r]) & mask);
      L = R, R = t;
    }
    x = (L << h) | R;
    found = x < a.count;
  }
  a.order[j] = found ? a.index[x] : -1ll;
}

__global__ __launch_bounds__(SKE_FAULT_THREADS) void k_epoch_faults(const long long *order, long long count, long long *fault_out) {
  __shared__ long long wsum[SKE_FAULT_THREADS / 64];
  const int t = threadIdx.x;
  long long n = 0;
  for (long long i = t; i < count; i += SKE_FAULT_THREADS) n += order[i] == -1ll ? 1 : 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
  if ((t & 63) == 0) wsum[t >> 6] = n;
  __syncthreads();
  if (t == 0) {
    long long x = 0;
    for (int w = 0; w < SKE_FAULT_THREADS / 64; w++) x += wsum[w];
    *fault_out = x;
  }
}

struct SkStatsArgs {
  const double *stats;           // the loss head's statistics of the step: ns doubles
  const float *pair;             // (norm, coefficient) of the step's skyjo_vec_grad_norm, or null: no clipping
  double *acc;                   // [SKE_ACC]
  double *row;                   // the epoch's row of epoch_stats_out: [SKYJO_UPDATE_STATS]
  const long long *epoch_fault;  // the epoch's shuffle fault count, or null (the caller's orders)
  long long *fault_out;
  double m;                      // the step's rows
  double inv_seen, inv_steps;    // 1 / max(rows of the epoch, 1) and 1 / steps of the epoch, the host's doubles
  int ns;                        // 6, or 7 with the KL term
  int first, last;               // the epoch's first / last step
};

__global__ __launch_bounds__(64) void k_update_stats(SkStatsArgs a) {
  const int i = threadIdx.x;
  if (i > 10) return;
  double x = 0.0, w = 1.0;  // what the lane adds: x * w
  if (i < a.ns) x = a.stats[i], w = a.m;
  else if (i == 7) x = a.pair ? (double)a.pair[0] : 0.0;
  else if (i == 8) x = a.pair ? (double)(a.pair[1] < 1.0f) : 0.0;
  else if (i == 9) x = a.m;
  else if (i == 10) x = 1.0;
  const double before = a.first ? 0.0 : a.acc[i];
  const double now = before + x * w;
  a.acc[i] = now;
  if (!a.last) return;
  if (i < 7) a.row[i] = now * a.inv_seen;
  else if (i < 9) a.row[i] = a.pair ? now * a.inv_steps : 0.0;
  else if (i == 9) a.row[i] = now;
  else if (a.epoch_fault) *a.fault_out += *a.epoch_fault;
}
