// skyjo_train.h - learner kernels (included from skyjo_learner.hip).
// One branch of ActionMaskModel - Linear(D,256)-tanh-Linear(256,256)-tanh-Linear(256,O), 1 <= D <= 31, 1 <= O <= 32 - trained on
// its float32 master parameters as they lie in torch's nn.Linear layout: the forward that KEEPS its activations and the backward
// that reads them.  include/skyjo_vec.h (skyjo_vec_mlp_train_*) and DESIGN.md 4 have the definition and the workspace;
// tests/mlp_train_ref.py restates it in float64.
//
// Every product runs on the exact float32 matrix instruction v_mfma_f32_32x32x2_f32: float32 in, float32 accumulate, bit for bit an
// fmaf chain in the order the steps are issued - no bf16 split, no scaled operands (those are the rollout nets': skyjo_policy.h).
// Lane l of a wavefront (c = l & 31, hh = l >> 5) gives A[c][k = hh] and B[k = hh][c] of a step and holds
// C[(r & 3) + 8 (r >> 2) + 4 hh][c] in register r of its 16; SKT_ROW(r, hh) is that row.  A workgroup is 4 wavefronts, one per SIMD.
//
// (a) k_mlp_train_fwd: a workgroup owns SKT_TILE_ROWS = 64 consecutive rows; wavefront w owns 64 of the 256 hidden units (2 x 2 tiles of
//     32 x 32, 64 accumulator registers).  x goes to LDS padded to 32 columns - columns [D, 31) are 0, column 31 is 1, and W1's column
//     31 is b1 (the packed layer 1 carries b1 the same way) - rows beyond m are all zero.  h1 = tanhf(.) goes to the workspace and to an
//     LDS image [64][256 + 4]; layer 2 takes its A operand from that image and W2 straight from memory, 8 k at a time: a lane reads
//     16 bytes of its W2 row (k0 + 4 hh .. + 3) and 16 bytes of its h1 row at the same k and issues 4 steps, so the chain of an output
//     runs over k in the order k0, k0 + 4, k0 + 1, k0 + 5, ... within each group of 8, groups ascending; b2 is added after the chain.
//     h2 = tanhf(.) replaces h1 in the image; wavefronts 0 and 1 then do the 32 rows each of layer 3 (W3's rows >= O are zero operands,
//     not read) and write out[row][o] for row < m, o < O.  The saved activation is the value the next layer consumed.
// (b) k_mlp_train_bwd_rows: the same tiling.  dz2 = (g W3) (1 - h2 h2) with g padded to 32 columns of zeros in LDS (k ascending, only
//     the ceil(O / 2) steps that hold a column < O), dz1 = (dz2 W2) (1 - h1 h1) with dz2 from an LDS image and W2's rows read
//     128 bytes per half wavefront (k in the order of (a)); both to the workspace, rows < m only.
// (c) k_mlp_train_bwd_weights: workgroup (c, y) owns the SKT_CHUNK_ROWS = 256 rows of chunk c and the hidden units [64 y, 64 y + 64):
//     the contraction runs over the chunk's rows, ascending, two per step, both operands read from the workspace as they lie (rows
//     beyond m enter as zeros - they are never read).  dW2[j][i] = sum dz2[r][j] h1[r][i] for its 64 j and all i (wavefront w: 64 of the
//     i), then wavefronts 0, 1: dW3[o][i] = sum g[r][o] h2[r][i] for 32 of its 64 i each, wavefronts 2, 3: dW1[j][k] = sum dz1[r][j] x[r][k]
//     over the padded x for 32 of its 64 j each - column 31 of that is db1.  db2 (its 64 columns) and, in y == 0, db3 are column sums
//     in 4 / 8 runs of 64 / 32 rows, the runs added in order.  Everything goes to the chunk's partial record, SKT_PART floats.
// (d) k_mlp_train_bwd_finish: one thread per element of the record adds the chunks' partials in double, chunk 0 first, and rounds once
//     into the gradient tensor.  No chain over rows is longer than 256; no atomics; the same input gives the same bits on every call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SKT_H 256            // hidden units
#define SKT_IN 32            // layer 1's padded input width: column 31 carries the bias
#define SKT_OUT 32           // layer 3's padded output width
#define SKT_TILE_ROWS 64     // rows of a workgroup in (a) and (b)
#define SKT_CHUNK_ROWS 256   // rows of a chunk in (c): the longest chain over rows
#define SKT_THREADS 256
#define SKT_HS (SKT_H + 4)   // dwords between the rows of an activation image in LDS (16-byte aligned rows, not a multiple of 32)
#define SKT_XS (SKT_IN + 4)  // the same for the x / g image
#define SKT_SLICES 4         // (c): hidden-unit slices of 64 per chunk
// a chunk's partial record, floats: dW2 [256][256], dW1 [256][32] (padded: column 31 = db1), dW3 [32][256] (padded rows), db2 [256], db3 [32]
#define SKT_PART_W2 0
#define SKT_PART_W1 (SKT_H * SKT_H)
#define SKT_PART_W3 (SKT_PART_W1 + SKT_H * SKT_IN)
#define SKT_PART_B2 (SKT_PART_W3 + SKT_OUT * SKT_H)
#define SKT_PART_B3 (SKT_PART_B2 + SKT_H)
#define SKT_PART (SKT_PART_B3 + SKT_OUT)
#define SKT_ROW(r, hh) (((r) & 3) + 8 * ((r) >> 2) + 4 * (hh))

typedef float skt_acc __attribute__((ext_vector_type(16)));

struct SkTrainArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3;  // nn.Linear layout; w2 and w3 16-byte aligned
  const float *x;                            // [m][D]
  const float *g;                            // [m][O] (backward)
  float *out;                                // [m][O] (forward)
  float *h1, *h2, *dz2, *dz1;                // [m][256] each, in the workspace
  float *part;                               // [chunks][SKT_PART]
  float *grads[6];
  long long m;
  int D, O, chunks;
};

#define SKT_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ skt_acc skt_zero() {
  skt_acc z;
#pragma unroll
  for (int r = 0; r < 16; r++) z[r] = 0.f;
  return z;
}

// the padded x: column k of row `row`, which is < m
__device__ __forceinline__ float skt_x(const SkTrainArgs &a, long long row, int k) {
  return k < a.D ? a.x[row * a.D + k] : (k == SKT_IN - 1 ? 1.f : 0.f);
}

// One k-group of 8 on a 2 x 2 block of tiles: av[t] / bv[t] hold the lane's 4 operands of row / column tile t at k0 + 4 hh .. + 3
__device__ __forceinline__ void skt_group(skt_acc (&acc)[2][2], const float4 (&av)[2], const float4 (&bv)[2]) {
  const float a0[4] = {av[0].x, av[0].y, av[0].z, av[0].w}, a1[4] = {av[1].x, av[1].y, av[1].z, av[1].w};
  const float b0[4] = {bv[0].x, bv[0].y, bv[0].z, bv[0].w}, b1[4] = {bv[1].x, bv[1].y, bv[1].z, bv[1].w};
#pragma unroll
  for (int t = 0; t < 4; t++) {
    acc[0][0] = SKT_MFMA(a0[t], b0[t], acc[0][0]);
    acc[0][1] = SKT_MFMA(a0[t], b1[t], acc[0][1]);
    acc[1][0] = SKT_MFMA(a1[t], b0[t], acc[1][0]);
    acc[1][1] = SKT_MFMA(a1[t], b1[t], acc[1][1]);
  }
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_fwd(SkTrainArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[SKT_TILE_ROWS * SKT_XS];
  __shared__ __attribute__((aligned(16))) float hs[SKT_TILE_ROWS * SKT_HS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
  const long long r0 = (long long)blockIdx.x * SKT_TILE_ROWS;
  const int rows = a.m - r0 < SKT_TILE_ROWS ? (int)(a.m - r0) : SKT_TILE_ROWS;
  const int u0 = 64 * w;  // this wavefront's hidden units

  for (int e = tid; e < SKT_TILE_ROWS * SKT_IN; e += SKT_THREADS) {
    const int i = e >> 5, k = e & 31;
    xs[i * SKT_XS + k] = i < rows ? skt_x(a, r0 + i, k) : 0.f;
  }
  __syncthreads();

  skt_acc acc[2][2];
  // ---- layer 1: k over the 32 padded columns, W1 read element by element (its rows are D floats: no alignment) ----
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
#pragma unroll
  for (int k0 = 0; k0 < SKT_IN; k0 += 8) {
    float4 av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      av[t] = *(const float4 *)(xs + (32 * t + c) * SKT_XS + k0 + 4 * hh);
      const int u = u0 + 32 * t + c;
      float b[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int k = k0 + 4 * hh + q;
        b[q] = k < a.D ? a.w1[u * a.D + k] : (k == SKT_IN - 1 ? a.b1[u] : 0.f);
      }
      bv[t] = make_float4(b[0], b[1], b[2], b[3]);
    }
    skt_group(acc, av, bv);
  }
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

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_bwd_rows(SkTrainArgs a) {
  __shared__ __attribute__((aligned(16))) float gs[SKT_TILE_ROWS * SKT_XS];
  __shared__ __attribute__((aligned(16))) float ds[SKT_TILE_ROWS * SKT_HS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
  const long long r0 = (long long)blockIdx.x * SKT_TILE_ROWS;
  const int rows = a.m - r0 < SKT_TILE_ROWS ? (int)(a.m - r0) : SKT_TILE_ROWS;
  const int u0 = 64 * w;

  for (int e = tid; e < SKT_TILE_ROWS * SKT_OUT; e += SKT_THREADS) {
    const int i = e >> 5, k = e & 31;
    gs[i * SKT_XS + k] = (i < rows && k < a.O) ? a.g[(size_t)(r0 + i) * a.O + k] : 0.f;
  }
  __syncthreads();

  skt_acc acc[2][2];
  // ---- dz2 = (g W3) (1 - h2 h2): k = the output o, two per step ----
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
  const int steps = (a.O + 1) >> 1;
  for (int s = 0; s < steps; s++) {
    const int k = 2 * s + hh;
    float av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      av[t] = gs[(32 * t + c) * SKT_XS + k];
      bv[t] = k < a.O ? a.w3[(size_t)k * SKT_H + u0 + 32 * t + c] : 0.f;
    }
    acc[0][0] = SKT_MFMA(av[0], bv[0], acc[0][0]);
    acc[0][1] = SKT_MFMA(av[0], bv[1], acc[0][1]);
    acc[1][0] = SKT_MFMA(av[1], bv[0], acc[1][0]);
    acc[1][1] = SKT_MFMA(av[1], bv[1], acc[1][1]);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * i + SKT_ROW(r, hh), u = u0 + 32 * j + c;
        float d = 0.f;
        if (row < rows) {
          const float h = a.h2[(size_t)(r0 + row) * SKT_H + u];
          d = acc[i][j][r] * (1.f - h * h);
          a.dz2[(size_t)(r0 + row) * SKT_H + u] = d;
        }
        ds[row * SKT_HS + u] = d;
      }
  __syncthreads();

  // ---- dz1 = (dz2 W2) (1 - h1 h1): k = layer 2's unit, W2[k][u] ----
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++) acc[i][j] = skt_zero();
#pragma unroll 2
  for (int k0 = 0; k0 < SKT_H; k0 += 8) {
    float4 av[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      av[t] = *(const float4 *)(ds + (32 * t + c) * SKT_HS + k0 + 4 * hh);
      const float *col = a.w2 + (size_t)(k0 + 4 * hh) * SKT_H + u0 + 32 * t + c;
      bv[t] = make_float4(col[0], col[SKT_H], col[2 * SKT_H], col[3 * SKT_H]);
    }
    skt_group(acc, av, bv);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int row = 32 * i + SKT_ROW(r, hh), u = u0 + 32 * j + c;
        if (row < rows) {
          const float h = a.h1[(size_t)(r0 + row) * SKT_H + u];
          a.dz1[(size_t)(r0 + row) * SKT_H + u] = acc[i][j][r] * (1.f - h * h);
        }
      }
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_bwd_weights(SkTrainArgs a) {
  __shared__ float red[8][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, hh = lane >> 5;
  const int y = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * SKT_CHUNK_ROWS;
  const int rows = a.m - r0 < SKT_CHUNK_ROWS ? (int)(a.m - r0) : SKT_CHUNK_ROWS;
  const int steps = (rows + 1) >> 1;  // (the steps beyond hold rows >= m only: zero operands, nothing to add)
  float *part = a.part + (size_t)blockIdx.x * SKT_PART;
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

  {  // ---- wavefronts 0, 1: dW3[o][i] for i = j0 + 32 w + c;  wavefronts 2, 3: dW1[j][k] for j = j0 + 32 (w - 2) + (row), k = c ----
    skt_acc acc = skt_zero();
    const bool third = w < 2;
    const int u = j0 + 32 * (w & 1);
    for (int s0 = 0; s0 < steps; s0 += 4) {
      float av[4], bv[4];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const int r = 2 * (s0 + v) + hh;
        const bool ok = r < rows;
        av[v] = bv[v] = 0.f;
        if (third) {
          if (ok && c < a.O) av[v] = a.g[(size_t)(r0 + r) * a.O + c];
          if (ok) bv[v] = a.h2[(size_t)(r0 + r) * SKT_H + u + c];
        } else if (ok) {
          av[v] = a.dz1[(size_t)(r0 + r) * SKT_H + u + c];
          bv[v] = skt_x(a, r0 + r, c);
        }
      }
#pragma unroll
      for (int v = 0; v < 4; v++) acc = SKT_MFMA(av[v], bv[v], acc);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int row = SKT_ROW(r, hh);
      if (third) part[SKT_PART_W3 + row * SKT_H + u + c] = acc[r];
      else part[SKT_PART_W1 + (u + row) * SKT_IN + c] = acc[r];
    }
  }

  {  // ---- db2 for this slice's 64 columns: 4 runs of 64 rows;  db3 (y == 0): 8 runs of 32 rows ----
    const int col = tid & 63, q = tid >> 6;
    float s2 = 0.f;
    for (int r = 64 * q; r < 64 * q + 64 && r < rows; r++) s2 += a.dz2[(size_t)(r0 + r) * SKT_H + j0 + col];
    red[q][col] = s2;
    __syncthreads();
    if (tid < 64) part[SKT_PART_B2 + j0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
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
        part[SKT_PART_B3 + tid] = s;
      }
    }
  }
}

__global__ __launch_bounds__(SKT_THREADS) void k_mlp_train_bwd_finish(SkTrainArgs a) {
  const int e = blockIdx.x * SKT_THREADS + threadIdx.x;
  if (e >= SKT_PART) return;
  float *dst = nullptr;
  if (e < SKT_PART_W1) {
    dst = a.grads[2] + e;
  } else if (e < SKT_PART_W3) {
    const int j = (e - SKT_PART_W1) >> 5, k = (e - SKT_PART_W1) & 31;
    if (k < a.D) dst = a.grads[0] + j * a.D + k;
    else if (k == SKT_IN - 1) dst = a.grads[1] + j;
  } else if (e < SKT_PART_B2) {
    if (((e - SKT_PART_W3) >> 8) < a.O) dst = a.grads[4] + (e - SKT_PART_W3);
  } else if (e < SKT_PART_B3) {
    dst = a.grads[3] + (e - SKT_PART_B2);
  } else if (e - SKT_PART_B3 < a.O) {
    dst = a.grads[5] + (e - SKT_PART_B3);
  }
  if (!dst) return;
  double s = 0.0;
  for (int ch = 0; ch < a.chunks; ch++) s += (double)a.part[(size_t)ch * SKT_PART + e];
  *dst = (float)s;
}
