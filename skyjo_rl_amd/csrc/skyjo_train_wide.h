// skyjo_train_wide.h - the learner kernels for a branch whose layer 1 has 32 <= D <= 163 inputs (included from skyjo_learner.hip behind
// skyjo_train.h, whose SkTrainArgs, tiling, macros and helpers it uses).  include/skyjo_vec.h (skyjo_vec_mlp_train_wide_*) and
// DESIGN.md 4 have the definition; tests/mlp_train_wide_ref.py restates the layout.  The bodies are COPIES of skyjo_train.h's with
// layer 1's width a run-time value: sharing them through a function template would have had to leave the narrow kernels' instructions
// as they are (EXPERIMENTS.md), and a copy cannot change them.  k_mlp_train_bwd_rows reads neither x nor W1: the wide backward launches it.
//
// The padded width is K = 8 (D / 8 + 1): a multiple of the k-group of 8 with at least one free column.  x's columns [D, K - 1) are 0,
// column K - 1 is 1 against b1 in W1's column K - 1 - the last term of layer 1's chain.  (D = 31 would give the narrow kernels' 32.)
//
// (a) k_mlp_train_wide_fwd: k_mlp_train_fwd with layer 1 over K / 8 groups, ascending, the order inside a group the documented one.
//     ONE LDS array of 64 x 260 floats (66 560 bytes; the narrow kernel has 75 776): the x tile [64][K + 4] (at K = 168: 44 032 bytes)
//     lies in the h image's place - layer 1 needs x alone, everything behind it the image alone - at the price of one more barrier
//     between a wavefront's last read of x and the first write of h1.  Two workgroups fit a CU's 160 KiB, as with the narrow kernel;
//     a whole x tile beside the image (110 592 bytes) would leave one, and staging x in slabs would add a barrier per slab.
//     W1's rows are D floats long and unaligned: a lane reads its 4 operands element by element, each behind k < D - nothing past a row.
// (b) k_mlp_train_wide_bwd_weights: k_mlp_train_bwd_weights with dW1[j][k] = sum dz1[r][j] xpad[r][k] over all K columns, in
//     CT = ceil(K / 32) column tiles per 32 hidden units.  In workgroup (chunk, y) wavefront w owns the 32 hidden units
//     64 y + 32 (w & 1); wavefronts 0, 1 do their dW3 tile and then the ODD column tiles, wavefronts 2, 3 the EVEN ones (at K = 168:
//     3 and 3; at K = 48: 1 and 1) - one chain per tile over the chunk's rows, ascending, two per step.  A lane whose column is >= K
//     (the last tile's rest) takes zero operands, reads no x and stores nothing.
//     The chunk's partial record, floats: dW2 [256][256], dW1 [256][K] (column K - 1 = db1), dW3 [32][256], db2 [256], db3 [32].
// (c) k_mlp_train_wide_bwd_finish: one thread per element of that record; chunks added in double, chunk 0 first, rounded once.
// Rows, offsets and elements are 64-bit wherever a row count enters (m <= 2^30: row * D passes 2^31 at 13 M rows).
#pragma once
#include "skyjo_train.h"

#define SKTW_MIN_IN 32    // the narrow kernels end at 31
#define SKTW_MAX_IN 163   // SKP_MAX_OBS: 19 + 12 * 12
#define SKTW_PART_FIXED (SKT_H * SKT_H + SKT_OUT * SKT_H + SKT_H + SKT_OUT)  // 74 016: the record without dW1

__host__ __device__ __forceinline__ int sktw_k(int D) { return 8 * (D / 8 + 1); }
__host__ __device__ __forceinline__ int sktw_part(int K) { return SKTW_PART_FIXED + SKT_H * K; }

// the padded x: column k < K of row `row`, which is < m
__device__ __forceinline__ float sktw_x(const SkTrainArgs &a, long long row, int k, int K) {
  return k < a.D ? a.x[row * a.D + k] : (k == K - 1 ? 1.f : 0.f);
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_wide_fwd(SkTrainArgs a) {
  __shared__ __attribute__((aligned(16))) float hs[SKT_TILE_ROWS * SKT_HS];  // first the x tile [64][K + 4], then the activation image
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
  const long long r0 = (long long)blockIdx.x * SKT_TILE_ROWS;
  const int rows = a.m - r0 < SKT_TILE_ROWS ? (int)(a.m - r0) : SKT_TILE_ROWS;
  const int u0 = 64 * w;  // this wavefront's hidden units
  const int K = sktw_k(a.D), XS = K + 4;
  float *const xs = hs;

  for (int i = w; i < SKT_TILE_ROWS; i += 4)  // a row per wavefront and pass: consecutive lanes, consecutive columns
    for (int k = lane; k < K; k += 64) xs[i * XS + k] = i < rows ? sktw_x(a, r0 + i, k, K) : 0.f;
  __syncthreads();

  skt_acc acc[2][2];
  // ---- layer 1: k over the K padded columns, W1 read element by element (its rows are D floats: no alignment) ----
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
  for (int k0 = 0; k0 < K; k0 += 8) {
    float4 av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      av[t] = *(const float4 *)(xs + (32 * t + c) * XS + k0 + 4 * hh);
      const int u = u0 + 32 * t + c;
      float b[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int k = k0 + 4 * hh + q;
        b[q] = k < a.D ? a.w1[u * a.D + k] : (k == K - 1 ? a.b1[u] : 0.f);
      }
      bv[t] = make_float4(b[0], b[1], b[2], b[3]);
    }
    skt_group(acc, av, bv);
  }
  __syncthreads();  // (every wavefront has read the x tile: the image may take its place)
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * i + SKT_ROW(r, hh), u = u0 + 32 * j + c;
        const float h = tanhf(acc[i][j][r]);  // (a row beyond m: tanhf(0) = 0)
        hs[row * SKT_HS + u] = h;
        if (row < rows) a.h1[(size_t)(r0 + row) * SKT_H + u] = h;
      }
  __syncthreads();

  // ---- layer 2 ----
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
#pragma unroll 2
  for (int k0 = 0; k0 < SKT_H; k0 += 8) {
    float4 av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      av[t] = *(const float4 *)(hs + (32 * t + c) * SKT_HS + k0 + 4 * hh);
      bv[t] = *(const float4 *)(a.w2 + (size_t)(u0 + 32 * t + c) * SKT_H + k0 + 4 * hh);
    }
    skt_group(acc, av, bv);
  }
  __syncthreads();  // (every wavefront has read h1's image)
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int u = u0 + 32 * j + c;
    const float bias = a.b2[u];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * i + SKT_ROW(r, hh);
        const float h = row < rows ? tanhf(acc[i][j][r] + bias) : 0.f;
        hs[row * SKT_HS + u] = h;
        if (row < rows) a.h2[(size_t)(r0 + row) * SKT_H + u] = h;
      }
  }
  __syncthreads();

  // ---- layer 3: wavefront w < 2 does rows 32 w .. 32 w + 31, output o = c ----
  if (w < 2) {
    skt_acc o3 = skt_zero();
    const bool live = c < a.O;
    const float *wrow = a.w3 + (size_t)(live ? c : 0) * SKT_H + 4 * hh;
#pragma unroll 4
    for (int k0 = 0; k0 < SKT_H; k0 += 8) {
      const float4 av = *(const float4 *)(hs + (32 * w + c) * SKT_HS + k0 + 4 * hh);
      float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live) bv = *(const float4 *)(wrow + k0);
      o3 = SKT_MFMA(av.x, bv.x, o3);
      o3 = SKT_MFMA(av.y, bv.y, o3);
      o3 = SKT_MFMA(av.z, bv.z, o3);
      o3 = SKT_MFMA(av.w, bv.w, o3);
    }
    if (live) {
      const float bias = a.b3[c];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * w + SKT_ROW(r, hh);
        if (row < rows) a.out[(size_t)(r0 + row) * a.O + c] = o3[r] + bias;
      }
    }
  }
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_wide_bwd_weights(SkTrainArgs a) {
  __shared__ float red[8][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
  const int y = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * SKT_CHUNK_ROWS;
  const int rows = a.m - r0 < SKT_CHUNK_ROWS ? (int)(a.m - r0) : SKT_CHUNK_ROWS;
  const int steps = (rows + 1) >> 1;  // (the steps beyond hold rows >= m only: zero operands, nothing to add)
  const int K = sktw_k(a.D);
  const size_t part_w1 = (size_t)SKT_H * SKT_H, part_w3 = part_w1 + (size_t)SKT_H * K, part_b2 = part_w3 + SKT_OUT * SKT_H,
               part_b3 = part_b2 + SKT_H;
  float *part = a.part + (size_t)blockIdx.x * sktw_part(K);
  const int j0 = 64 * y, i0 = 64 * w;

  {  // ---- dW2[j][i], j in this slice, i in this wavefront's 64 ----
    skt_acc acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
    const float *pa = a.dz2 + (size_t)r0 * SKT_H + j0 + c, *pb = a.h1 + (size_t)r0 * SKT_H + i0 + c;
    for (int s0 = 0; s0 < steps; s0 += 4) {  // (4 steps' loads in flight; a step beyond `steps` adds 0 * 0)
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int r = 2 * (s0 + v) + hh;
        const bool ok = r < rows;
        float av[2], bv[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
          av[t] = ok ? pa[(size_t)r * SKT_H + 32 * t] : 0.f;
          bv[t] = ok ? pb[(size_t)r * SKT_H + 32 * t] : 0.f;
        }
        acc[0][0] = SKT_MFMA(av[0], bv[0], acc[0][0]);
        acc[0][1] = SKT_MFMA(av[0], bv[1], acc[0][1]);
        acc[1][0] = SKT_MFMA(av[1], bv[0], acc[1][0]);
        acc[1][1] = SKT_MFMA(av[1], bv[1], acc[1][1]);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++)
#pragma unroll
        for (int r = 0; r < 16; r++)
          part[SKT_PART_W2 + (j0 + 32 * i + SKT_ROW(r, hh)) * SKT_H + i0 + 32 * j + c] = acc[i][j][r];
  }

  const int u = j0 + 32 * (w & 1);  // the 32 hidden units of this wavefront's dW3 and dW1 tiles
  if (w < 2) {  // ---- wavefronts 0, 1: dW3[o][i] for i = u + c ----
    skt_acc acc = skt_zero();
    for (int s0 = 0; s0 < steps; s0 += 4) {
      float av[4], bv[4];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int r = 2 * (s0 + v) + hh;
        const bool ok = r < rows;
        av[v] = bv[v] = 0.f;
        if (ok && c < a.O) av[v] = a.g[(size_t)(r0 + r) * a.O + c];
        if (ok) bv[v] = a.h2[(size_t)(r0 + r) * SKT_H + u + c];
      }
#pragma unroll
      for (int v = 0; v < 4; v++) acc = SKT_MFMA(av[v], bv[v], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) part[part_w3 + SKT_ROW(r, hh) * SKT_H + u + c] = acc[r];
  }
  // ---- dW1[j][k] for j = u + (row), k = 32 ct + c: wavefronts 0, 1 the odd column tiles ct, wavefronts 2, 3 the even ones ----
  for (int ct = w < 2 ? 1 : 0; 32 * ct < K; ct += 2) {
    skt_acc acc = skt_zero();
    const int k = 32 * ct + c;
    const bool col = k < K;  // (false in the rest of the last tile only: no operand is read, nothing is stored)
    for (int s0 = 0; s0 < steps; s0 += 4) {
      float av[4], bv[4];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int r = 2 * (s0 + v) + hh;
        av[v] = bv[v] = 0.f;
        if (r < rows) {
          av[v] = a.dz1[(size_t)(r0 + r) * SKT_H + u + c];
          if (col) bv[v] = sktw_x(a, r0 + r, k, K);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; v++) acc = SKT_MFMA(av[v], bv[v], acc);
    }
    if (col)
#pragma unroll
      for (int r = 0; r < 16; r++) part[part_w1 + (size_t)(u + SKT_ROW(r, hh)) * K + k] = acc[r];
  }

  {  // ---- db2 for this slice's 64 columns: 4 runs of 64 rows;  db3 (y == 0): 8 runs of 32 rows ----
    const int col = tid & 63, q = tid >> 6;
    float s2 = 0.f;
    for (int r = 64 * q; r < 64 * q + 64 && r < rows; r++) s2 += a.dz2[(size_t)(r0 + r) * SKT_H + j0 + col];
    red[q][col] = s2;
    __syncthreads();
    if (tid < 64) part[part_b2 + j0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
    if (y == 0) {  // (uniform in the workgroup)
      const int o = tid & 31, q3 = tid >> 5;
      float s3 = 0.f;
      if (o < a.O)
        for (int r = 32 * q3; r < 32 * q3 + 32 && r < rows; r++) s3 += a.g[(size_t)(r0 + r) * a.O + o];
      red[q3][o] = s3;
      __syncthreads();
      if (tid < 32) {
        float s = red[0][tid];
#pragma unroll
        for (int k = 1; k < 8; k++) s += red[k][tid];
        part[part_b3 + tid] = s;
      }
    }
  }
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_wide_bwd_finish(SkTrainArgs a) {
  const int K = sktw_k(a.D), total = sktw_part(K);
  const int e = blockIdx.x * SKT_THREADS + threadIdx.x;
  if (e >= total) return;
  const int part_w1 = SKT_H * SKT_H, part_w3 = part_w1 + SKT_H * K, part_b2 = part_w3 + SKT_OUT * SKT_H, part_b3 = part_b2 + SKT_H;
  float *dst = nullptr;
  if (e < part_w1) {
    dst = a.grads[2] + e;
  } else if (e < part_w3) {
    const int j = (e - part_w1) / K, k = (e - part_w1) - j * K;
    if (k < a.D) dst = a.grads[0] + j * a.D + k;
    else if (k == K - 1) dst = a.grads[1] + j;
  } else if (e < part_b2) {
    if (((e - part_w3) >> 8) < a.O) dst = a.grads[4] + (e - part_w3);
  } else if (e < part_b3) {
    dst = a.grads[3] + (e - part_b2);
  } else if (e - part_b3 < a.O) {
    dst = a.grads[5] + (e - part_b3);
  }
  if (!dst) return;
  double s = 0.0;
  for (int ch = 0; ch < a.chunks; ch++) s += (double)a.part[(size_t)ch * total + e];
  *dst = (float)s;
}
