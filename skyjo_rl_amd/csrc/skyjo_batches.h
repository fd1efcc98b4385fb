// skyjo_batches.h - learner kernels (included from skyjo_learner.hip; they read records through SkRecords of skyjo_learner_util.h and are no
// part of the environment's sources).  Learner minibatches of a rollout buffer: which rows take part (with the moments of their
// advantages), and the rows of a minibatch as the dense float tensors a learner feeds its model - both on the buffer as it lies,
// in either record layout.
//
// (a) k_select_*: the ascending list of the rows whose flags byte has every bit of `require` - a stable compaction, what
//     torch.nonzero gives - their count, and the sums of a and a * a over their advantages a, each widened to double first.  Three
//     launches, none of which waits for another workgroup: per-block counts and partial sums (ballot + popcount inside a
//     wavefront), an exclusive scan of the block counts in ONE workgroup, the scatter.  The sums have a fixed shape - a lane's
//     SK_SEL_ITERS rows in order, the xor tree of a wavefront, the four wavefronts of a block in order, the blocks in the scan's
//     order - and no atomics: the same input gives the same bits on every call.
// (b) k_gather_rows: a workgroup owns SK_GATHER_ROWS consecutive OUTPUT rows.  It fetches their records as 16-byte pieces into LDS
//     (contiguous in a row-major buffer, 1 024 bytes apart in a tile-planar one: the addresses of sk_rec_byte), and streams the
//     two float outputs as 16-byte stores over the run's flat [rows * D] and [rows * 26] stretches (sk_store_stretch), reading the bytes out of the
//     LDS image - a mask or a meta byte is never reached by pointer arithmetic across a piece (for the direct observation the mask
//     offset is no multiple of 16).  The columns are one lane per row.  A row id outside [0, T * B) reads nothing and gives an
//     all-zero output row.  No private segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>

#include "skyjo_learner_util.h"

#define SK_SEL_THREADS 256
#define SK_SEL_WAVES (SK_SEL_THREADS / 64)
#define SK_SEL_ITERS 16                                 // rows per lane: their loads are in flight together
#define SK_SEL_WAVE_ROWS (64 * SK_SEL_ITERS)            // a wavefront's consecutive rows
#define SK_SEL_ROWS (SK_SEL_WAVES * SK_SEL_WAVE_ROWS)   // a block's: 4 096
#define SK_SCAN_THREADS 1024

// SEATS (skyjo_vec_rollout_select_seats): a row also needs bit agent(row) of seat_mask, the agent byte read in place from the row's
// record (SkRecords::of_row: k_gather_rows' numbers).  Unused otherwise.
struct SkSelectSeats {
  SkRecords rec;
  uint32_t seat_mask;
  int32_t off_agent;
};

// Phase 1 and 3 share the walk: wavefront w of block b owns rows  b * SK_SEL_ROWS + w * SK_SEL_WAVE_ROWS + k * 64 + lane,
// k = 0 .. SK_SEL_ITERS - 1.  SCATTER = false: block_count[b] and (adv given) block_sum[2 b], [2 b + 1].  SCATTER = true:
// block_count holds the exclusive offsets of the scan, and the selected row ids go to index_out.  The seat test is one more term of
// `sel` and nothing else: with every seat in the mask the counts, the offsets and the sums carry the bits of SEATS = false, and
// k_select_scan serves both.
template <bool SCATTER, bool SEATS>
__global__ __launch_bounds__(SK_SEL_THREADS) void k_select_pass(const uint8_t *flags, long long n, uint32_t require, const float *adv,
                                                               long long *block_count, double *block_sum, long long *index_out,
                                                               SkSelectSeats st) {
  __shared__ uint32_t wcnt[SK_SEL_WAVES];
  __shared__ double wsum[SK_SEL_WAVES], wsq[SK_SEL_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * SK_SEL_ROWS + w * SK_SEL_WAVE_ROWS + lane;
  uint32_t f[SK_SEL_ITERS];
  [[maybe_unused]] uint32_t seat[SK_SEL_ITERS];
  float av[SK_SEL_ITERS];
#pragma unroll
  for (int k = 0; k < SK_SEL_ITERS; k++) {
    const long long r = r0 + k * 64;
    f[k] = r < n ? flags[r] : 0u;  // (require is never 0: a row past the end is not selected)
    if constexpr (SEATS) seat[k] = r < n ? *st.rec.byte(st.rec.of_row(r), st.off_agent) : 0u;
    av[k] = 0.f;
    if (!SCATTER && adv && r < n) av[k] = adv[r];
  }
  unsigned long long bal[SK_SEL_ITERS];
  uint32_t cnt = 0;
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int k = 0; k < SK_SEL_ITERS; k++) {
    bool sel = (f[k] & require) == require;
    if constexpr (SEATS) sel = sel && seat[k] < 32u && ((st.seat_mask >> seat[k]) & 1u) != 0u;
    bal[k] = __ballot(sel);
    cnt += (uint32_t)__popcll(bal[k]);
    if (!SCATTER) {
      const double a = sel ? (double)av[k] : 0.0;
      s += a;
      q += a * a;
    }
  }
  if (!SCATTER && adv) s = sk_wave_sum(s), q = sk_wave_sum(q);
  if (lane == 0) wcnt[w] = cnt, wsum[w] = s, wsq[w] = q;
  __syncthreads();
  if constexpr (!SCATTER) {
    if (threadIdx.x == 0) {
      block_count[blockIdx.x] = (long long)((wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]));
      if (adv) {
        block_sum[2 * (size_t)blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        block_sum[2 * (size_t)blockIdx.x + 1] = ((wsq[0] + wsq[1]) + wsq[2]) + wsq[3];
      }
    }
  } else {
    long long off = block_count[blockIdx.x];
    for (int i = 0; i < w; i++) off += wcnt[i];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < SK_SEL_ITERS; k++) {
      if ((bal[k] >> lane) & 1ull) index_out[off + __popcll(bal[k] & below)] = r0 + k * 64;
      off += __popcll(bal[k]);
    }
  }
}

// Phase 2, one workgroup: block_count[0 .. nb) becomes its exclusive scan; the total, and the two sums over the blocks' partials
// (thread t owns a contiguous span of blocks, then the wavefront's tree, then the wavefronts in order), go to count_out /
// moments_out.  nb == 0 writes the zeros.
__global__ __launch_bounds__(SK_SCAN_THREADS) void k_select_scan(long long *block_count, const double *block_sum, int nb, long long *count_out,
                                                                double *moments_out) {
  __shared__ long long wtot[SK_SCAN_THREADS / 64];
  __shared__ double wsum[SK_SCAN_THREADS / 64], wsq[SK_SCAN_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int per = (nb + SK_SCAN_THREADS - 1) / SK_SCAN_THREADS;
  const long long lo_ = (long long)t * per;
  const int lo = lo_ < nb ? (int)lo_ : nb, hi = lo + per < nb ? lo + per : nb;
  long long c = 0;
  double s = 0.0, q = 0.0;
  for (int i = lo; i < hi; i++) {
    c += block_count[i];
    if (moments_out) s += block_sum[2 * (size_t)i], q += block_sum[2 * (size_t)i + 1];
  }
  long long inc = c;  // inclusive scan inside the wavefront
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long y = __shfl_up(inc, d, 64);
    if (lane >= d) inc += y;
  }
  s = sk_wave_sum(s), q = sk_wave_sum(q);
  if (lane == 63) wtot[w] = inc;
  if (lane == 0) wsum[w] = s, wsq[w] = q;
  __syncthreads();
  long long run = inc - c;
  for (int i = 0; i < w; i++) run += wtot[i];
  for (int i = lo; i < hi; i++) {
    const long long x = block_count[i];
    block_count[i] = run;
    run += x;
  }
  if (t == 0) {
    long long total = 0;
    double S = 0.0, Q = 0.0;
    for (int i = 0; i < SK_SCAN_THREADS / 64; i++) total += wtot[i], S += wsum[i], Q += wsq[i];
    *count_out = total;
    if (moments_out) moments_out[0] = S, moments_out[1] = Q;
  }
}

#define SK_GATHER_ROWS 64
#define SK_GATHER_THREADS 256
#define SK_GATHER_MAX_PIECES 13  // rec_bytes / 16 of the largest record: direct observation, 12 players (208 bytes)
#define SK_GATHER_LOADS ((SK_GATHER_ROWS * SK_GATHER_MAX_PIECES + SK_GATHER_THREADS - 1) / SK_GATHER_THREADS)

struct SkGatherArgs {
  SkRecords rec;             // [T (+ 1)] steps
  const long long *index;    // [m] row ids t * B + b, any order, repeats allowed
  const int32_t *actions;    // [T][B]
  const float *logp, *values, *adv, *vt;
  float *obs_out, *lm_out;   // [m][D], [m][26]: 16-byte aligned
  long long *act_out;
  float *logp_out, *adv_out, *vt_out, *val_out;
  uint8_t *seat_out;
  long long m, n_rows;       // n_rows = T * B
  int32_t vstride, D, Dp;
  float mean, std;
};

__global__ __launch_bounds__(SK_GATHER_THREADS) void k_gather_rows(SkGatherArgs a) {
  __shared__ uint4 tile[SK_GATHER_ROWS * SK_GATHER_MAX_PIECES];  // the run's records, row i at byte i * rec_bytes
  __shared__ long long rid[SK_GATHER_ROWS], rrec[SK_GATHER_ROWS];  // row id and record number of row i, -1: id out of range
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * SK_GATHER_ROWS;
  const int rows = a.m - o0 < SK_GATHER_ROWS ? (int)(a.m - o0) : SK_GATHER_ROWS;
  if (tid < SK_GATHER_ROWS) {
    long long r = -1, q = -1;
    if (tid < rows) {
      const long long x = a.index[o0 + tid];
      if (x >= 0 && x < a.n_rows) {
        r = x;
        q = a.rec.of_row(x);
      }
    }
    rid[tid] = r, rrec[tid] = q;
  }
  __syncthreads();

  // the records: piece c of row i.  Row-major: a row's pieces on consecutive lanes; tile-planar: piece c of 64 rows
  const int P = a.rec.rec_bytes >> 4, np = SK_GATHER_ROWS * P;
  uint4 v[SK_GATHER_LOADS];
  int slot[SK_GATHER_LOADS];
#pragma unroll
  for (int k = 0; k < SK_GATHER_LOADS; k++) {
    const int p = tid + k * SK_GATHER_THREADS;
    v[k] = make_uint4(0u, 0u, 0u, 0u);
    slot[k] = -1;
    if (p < np) {
      const int i = a.rec.planar ? (p & (SK_GATHER_ROWS - 1)) : p / P;
      const int c = a.rec.planar ? (p >> 6) : p - i * P;
      if (i < rows) {
        slot[k] = i * P + c;
        const long long q = rrec[i];
        if (q >= 0) v[k] = *(const uint4 *)a.rec.byte(q, c << 4);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < SK_GATHER_LOADS; k++)
    if (slot[k] >= 0) tile[slot[k]] = v[k];

  // the columns: one lane per row, the four wavefronts share them
  {
    const int i = tid & 63, w = tid >> 6;
    if (i < rows && w < 3) {
      const long long r = rid[i], o = o0 + i;
      const bool ok = r >= 0;
      if (w == 0) {
        a.act_out[o] = ok ? (long long)a.actions[r] : 0ll;
        a.logp_out[o] = ok ? a.logp[r] : 0.f;
      } else if (w == 1) {
        a.val_out[o] = ok ? a.values[r * a.vstride] : 0.f;
        a.vt_out[o] = ok ? a.vt[r] : 0.f;
      } else {
        float x = 0.f;
        if (ok) {
          const float d = a.adv[r] - a.mean;  // two float32 operations, each rounded: the definition
          x = d / a.std;
        }
        a.adv_out[o] = x;
      }
    }
  }
  __syncthreads();

  const uint8_t *tb = (const uint8_t *)tile;
  if (tid >= 3 * 64 && tid - 3 * 64 < rows) a.seat_out[o0 + tid - 3 * 64] = tb[(tid - 3 * 64) * a.rec.rec_bytes + a.Dp + 26];  // (zero for a row out of range)
  // observations: (float)(int8) of bytes 0 .. D - 1
  sk_store_stretch<SK_GATHER_THREADS>(a.obs_out + o0 * a.D, rows * a.D, a.D, [&](int i, int k) { return (float)(int8_t)tb[i * a.rec.rec_bytes + k]; });
  // log of the action mask, clamped: 0 where the action is legal, -FLT_MAX where it is not
  sk_store_stretch<SK_GATHER_THREADS>(a.lm_out + o0 * SKYJO_NUM_ACTIONS, rows * SKYJO_NUM_ACTIONS, SKYJO_NUM_ACTIONS, [&](int i, int k) {
    return rid[i] >= 0 && tb[i * a.rec.rec_bytes + a.Dp + k] == 0 ? -FLT_MAX : 0.f;
  });
}

// (c) k_gather_logits (skyjo_vec_rollout_gather_logits): rows of a float [n_rows][26] column - the behaviour logits a learner keeps
//     beside the buffer - by the row ids of k_gather_rows, which knows no such column.  A workgroup owns SK_GATHER_ROWS consecutive
//     OUTPUT rows: their ids go to LDS once, the run's flat [rows * 26] stretch leaves as 16-byte stores (the run starts at byte
//     o0 * 104, o0 a multiple of 64), each element read where its row lies (a row starts on an 8-byte boundary only: dword loads).
//     A row id outside [0, n_rows) reads nothing and gives an all-zero row.
__global__ __launch_bounds__(SK_GATHER_THREADS) void k_gather_logits(const float *column, long long n_rows, const long long *index, long long m,
                                                                    float *out) {
  __shared__ long long rid[SK_GATHER_ROWS];  // -1: id out of range
  const int tid = threadIdx.x;
  const long long o0 = (long long)blockIdx.x * SK_GATHER_ROWS;
  const int rows = m - o0 < SK_GATHER_ROWS ? (int)(m - o0) : SK_GATHER_ROWS;
  if (tid < SK_GATHER_ROWS) {
    long long r = -1;
    if (tid < rows) {
      const long long x = index[o0 + tid];
      if (x >= 0 && x < n_rows) r = x;
    }
    rid[tid] = r;
  }
  __syncthreads();
  sk_store_stretch<SK_GATHER_THREADS>(out + o0 * SKYJO_NUM_ACTIONS, rows * SKYJO_NUM_ACTIONS, SKYJO_NUM_ACTIONS, [&](int i, int k) {
    return rid[i] >= 0 ? column[rid[i] * SKYJO_NUM_ACTIONS + k] : 0.f;
  });
}
