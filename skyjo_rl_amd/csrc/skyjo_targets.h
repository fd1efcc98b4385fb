// skyjo_targets.h - a learner kernel (included from skyjo_learner.hip; it reads records through SkRecords of skyjo_learner_util.h and is no
// part of the environment's sources).  Learner targets of a rollout buffer: per-seat GAE(gamma, lambda), one lane per game.
//
// What RLlib's PPO computes per agent trajectory for the sample batches of the reference's trainer
// (rlskyjo/models/train_model_simple_rllib.py:22-59: `advantages`, `value_targets`) - here over the columns
// skyjo_vec_model_rollout has just written, in place and in either record layout.  SkyJo is turn-based: the seat that acts
// changes from row to row and a seat's "next value" is the value of ITS next row, so a lane walks its game from t = T - 1 down
// to 0 and carries, per seat, the value and the advantage of that seat's next action.  Rewards arrive once, at the episode end,
// for every seat (skyjo_env.py:293-312).
//
// The arithmetic is float32, every operation rounded on its own (-ffp-contract=off) in the order of the chain below:
// that order is the definition, tests/rollout_targets_ref.py restates it in numpy and the GPU test asks for
// the same bits.
//
// Shape: nothing a lane loads depends on its carries, so the inputs of SK_TGT_BLOCK time steps are requested first - the meta bytes,
// the end flags and the values in one round trip, the sparse reward rows of the steps that ended an episode in a second - and the
// dependent chain then runs over registers.  A row of a wavefront's outputs is 64 consecutive floats (bytes for the flags).
// Two to four seats keep their carries in registers, selected by compares; the generic form (one seat, five to twelve) keeps
// them in lane-private LDS columns and reads the rare reward row where the chain meets it.  No instantiation has a private segment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skyjo_learner_util.h"

#define SK_TGT_BLOCK 16  // time steps whose inputs are in flight together
#define SK_TGT_LANES 64  // one wavefront per workgroup: 65 536 games = one wavefront per SIMD

struct SkTargetsArgs {
  const float *values;     // [T + 1][B][vstride]
  const double *rewards;   // [T][B][N]
  const uint8_t *end;      // [T][B]
  float *adv, *vt, *ret;   // [T][B]
  uint8_t *flags;          // [T][B]
  SkRecords rec;           // [T + 1] steps
  int32_t T, N, vstride, off_agent, off_done;
  float gamma, gl;         // gl = float32(gamma) * float32(lambda), rounded once on the host
};

// Per-seat carries.  Two to four seats: registers; the generic form: lane-private LDS columns (seat i of lane l at [i][l]).
// (plain scalars and compare chains, not an array or a struct: nothing here may look like an indexed object to the compiler)
#define SK_TGT_SEL(p, s) sk_tgt_sel<NR>(s, p##0, p##1, p##2, p##3)
#define SK_TGT_PUT(p, s, x)                   \
  do {                                        \
    const float x_ = (x);                     \
    p##0 = (s) == 0 ? x_ : p##0;              \
    if (NR > 1) p##1 = (s) == 1 ? x_ : p##1;  \
    if (NR > 2) p##2 = (s) == 2 ? x_ : p##2;  \
    if (NR > 3) p##3 = (s) == 3 ? x_ : p##3;  \
  } while (0)
template <int NS>
__device__ __forceinline__ float sk_tgt_sel(int s, float v0, float v1, float v2, float v3) {
  float x = v0;
  if (NS > 1) x = s == 1 ? v1 : x;
  if (NS > 2) x = s == 2 ? v2 : x;
  if (NS > 3) x = s == 3 ? v3 : x;
  return x;
}
struct SkSeatLds {
  float *col;  // this lane's column: seat i at col[i * SK_TGT_LANES]
  __device__ __forceinline__ float get(int s) const { return col[s * SK_TGT_LANES]; }
  __device__ __forceinline__ void set(int s, float x) { col[s * SK_TGT_LANES] = x; }
};

template <int NS>
__global__ __launch_bounds__(SK_TGT_LANES) void k_rollout_targets(SkTargetsArgs a) {
  constexpr bool REGS = NS != 0;
  constexpr int NR = REGS ? NS : 1;
  __shared__ float cols[REGS ? 1 : 3 * SKYJO_MAX_PLAYERS * SK_TGT_LANES];
  const int b = blockIdx.x * SK_TGT_LANES + threadIdx.x;
  if (b >= a.rec.B) return;  // (no barrier below: the columns are lane-private)
  const int N = REGS ? NS : a.N;
  const size_t B = (size_t)a.rec.B;

  // seat states as two bit sets: TERMINAL, NEXT, neither = UNKNOWN
  uint32_t term = 0, next = 0;
  const uint32_t all = (1u << N) - 1u;
  bool known = false;
  float rR0 = 0.f, rR1 = 0.f, rR2 = 0.f, rR3 = 0.f, rnv0 = 0.f, rnv1 = 0.f, rnv2 = 0.f, rnv3 = 0.f, rna0 = 0.f, rna1 = 0.f, rna2 = 0.f, rna3 = 0.f;
  SkSeatLds lR{cols + threadIdx.x}, lnv{cols + SKYJO_MAX_PLAYERS * SK_TGT_LANES + threadIdx.x},
      lna{cols + 2 * SKYJO_MAX_PLAYERS * SK_TGT_LANES + threadIdx.x};
  if constexpr (!REGS)
    for (int i = 0; i < N; i++) lR.set(i, 0.f), lnv.set(i, 0.f), lna.set(i, 0.f);
#define SEAT_GET(name, s) (REGS ? SK_TGT_SEL(r##name, s) : l##name.get(s))
#define SEAT_SET(name, s, x)                        \
  do {                                              \
    if constexpr (REGS) SK_TGT_PUT(r##name, s, x);  \
    else l##name.set(s, x);                         \
  } while (0)

  {  // the bootstrap: the seat that would act on records[T] starts NEXT with values[T]
    const long long r = a.rec.at(a.T, b);
    const int s = *a.rec.byte(r, a.off_agent);
    if (*a.rec.byte(r, a.off_done) == 0 && s < N) {
      next = 1u << s;
      SEAT_SET(nv, s, a.values[((size_t)a.T * B + b) * a.vstride]);
      SEAT_SET(na, s, 0.f);
    }
  }

  for (int hi = a.T; hi > 0; hi -= SK_TGT_BLOCK) {
    const int lo = hi > SK_TGT_BLOCK ? hi - SK_TGT_BLOCK : 0;
    // round trip 1: everything the chain reads except the reward rows (k counts down from the block's last step)
    uint32_t seat[SK_TGT_BLOCK], done[SK_TGT_BLOCK], end[SK_TGT_BLOCK];
    float V[SK_TGT_BLOCK];
#pragma unroll
    for (int k = 0; k < SK_TGT_BLOCK; k++) {
      const int t = hi - 1 - k;
      seat[k] = 0, done[k] = 1, end[k] = 0, V[k] = 0.f;
      if (t >= lo) {
        const long long r = a.rec.at(t, b);
        seat[k] = *a.rec.byte(r, a.off_agent);
        done[k] = *a.rec.byte(r, a.off_done);
        end[k] = a.end[(size_t)t * B + b];
        V[k] = a.values[((size_t)t * B + b) * a.vstride];
      }
    }
    // round trip 2 (two to four seats): the reward rows of the steps that ended an episode - about one row in a hundred
    float rw[REGS ? SK_TGT_BLOCK : 1][NR];
    if constexpr (REGS) {
#pragma unroll
      for (int k = 0; k < SK_TGT_BLOCK; k++) {
#pragma unroll
        for (int i = 0; i < NR; i++) rw[k][i] = 0.f;
        if (end[k]) {
          const double *row = a.rewards + ((size_t)(hi - 1 - k) * B + b) * NR;
#pragma unroll
          for (int i = 0; i < NR; i++) rw[k][i] = (float)row[i];
        }
      }
    }
    // the chain
#pragma unroll
    for (int k = 0; k < SK_TGT_BLOCK; k++) {
      const int t = hi - 1 - k;
      if (t < lo) continue;  // (the buffer's first block may be short)
      const size_t o = (size_t)t * B + b;
      if (end[k]) {  // 1. the episode ended in this step: every seat's reward is known
        if constexpr (REGS) {
          rR0 = rw[k][0], rR1 = rw[k][NR > 1 ? 1 : 0], rR2 = rw[k][NR > 2 ? 2 : 0], rR3 = rw[k][NR > 3 ? 3 : 0];
        } else {
          const double *row = a.rewards + o * N;
          for (int i = 0; i < N; i++) lR.set(i, (float)row[i]);
        }
        term = all, next = 0, known = true;
      }
      float A = 0.f, tgt = 0.f, ret = 0.f;
      uint32_t fl = 0;
      if (done[k] != 0) {  // 2. a re-deal or no-op row: no transition, and nothing flows across it
        term = 0, next = 0;
      } else {
        const int s = (int)seat[k] < N ? (int)seat[k] : N - 1;  // (records of the engine never name a seat beyond N - 1)
        const uint32_t bit = 1u << s;
        const float v = V[k], Rs = SEAT_GET(R, s);
        if (term & bit) {  // 3. the seat's last action of the episode
          A = Rs - v;
          fl = SKYJO_TGT_HAS_TARGET;
        } else if (next & bit) {
          const float d = a.gamma * SEAT_GET(nv, s) - v;
          A = d + a.gl * SEAT_GET(na, s);
          fl = SKYJO_TGT_HAS_TARGET;
        }
        if (fl) tgt = A + v;  // 4.
        if (known) ret = Rs, fl |= SKYJO_TGT_EPISODE_KNOWN;  // 5.
        next |= bit, term &= ~bit;  // 6.
        SEAT_SET(nv, s, v);
        SEAT_SET(na, s, A);
      }
      a.adv[o] = A, a.vt[o] = tgt, a.ret[o] = ret, a.flags[o] = (uint8_t)fl;
    }
  }
#undef SEAT_GET
#undef SEAT_SET
}
#undef SK_TGT_SEL
#undef SK_TGT_PUT
