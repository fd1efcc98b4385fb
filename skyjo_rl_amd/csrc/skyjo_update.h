// skyjo_update.h - included from skyjo_learner.hip after skyjo_policy.h (it uses SKP_*).  The packed net's layout, stated once, and the
// kernel that writes an existing skyjo_vec_mlp's blob in place from device memory: skyjo_vec_mlp_update (repack) and
// skyjo_vec_mlp_adam_step / _adam_step_clipped (torch.optim.Adam's rule in front of the pack, on g or on g times a coefficient read
// from the device).  include/skyjo_vec.h and DESIGN.md 4 have the definition; tests/mlp_pack_ref.py restates the layout.
//
// (a) There is one packer: k_mlp_update.  skyjo_vec_mlp_create stages its host arrays on the device and runs it too, so the skp_* packing
//     helpers are device code only.  The unit is compiled with -ffp-contract=off, which makes the kernel's arithmetic the reference's
//     (tests/mlp_pack_ref.py): v = SKP_SCALE * w is one rounded float32 multiply, the bf16 rounding works on the bit pattern,
//     lo = bf16(v - float(hi)) is one rounded subtraction (float32 subnormals are kept), - 2 v is exact, and the bf16-mode bias sums add
//     the rounded weights of a row in double in ascending k.
// (b) k_mlp_update<ADAM>: SKU_BLOCKS workgroups of SKU_THREADS threads, ONE launch.  Workgroup u < 8 owns the hidden rows 32 u .. 32 u + 31
//     (the m-tile u of both hidden layers): thread t packs the W2 fragment (u, ks = t / 64, lane = t % 64) - its eight k are two
//     contiguous float4s of the row, acc_k's order - the first 64 KS threads also pack a W1 fragment (natural k order, k = 16 KS - 1 is b1;
//     KS = skp_w1_ksteps(obs_dim) k-steps, at most 11 x 64 = 704 of the 1 024), and
//     after a barrier one lane per row forms b2's entry: in bf16 mode it walks its row's 256 weights, which its own workgroup has just
//     written.  Workgroup 8 owns layer 3 the same way and spreads the 32 row biases over b3's accumulator layout.  A thread that owns
//     an element reads p, g, m, v once, writes p, m, v once and packs the new p from its registers; every store to the blob is a whole
//     16-byte fragment.  The job is about 80 k elements: nine workgroups are one wave of work for nine compute units and the cost is
//     the launch.
// (c) Ordering is the stream's: a net launch queued on the same stream afterwards sees the new weights.  A launch on ANOTHER stream
//     that still reads the blob is the caller's race - nothing here waits for it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#define SKU_THREADS 1024  // one W2 (or W3) fragment per thread of a workgroup: 16 k-steps x 64 lanes
#define SKU_BLOCKS 9      // 8 m-tiles of the hidden layers + layer 3
#define SKU_W1_FRAGS(ks) (8 * (ks) * 64)  // layer 1's piece: ks = skp_w1_ksteps(obs_dim) k-steps of 16 columns
#define SKU_W2_FRAGS (8 * 16 * 64)
#define SKU_W3_FRAGS (16 * 64)
#define SKU_TENSORS 6     // w1, b1, w2, b2, w3, b3

// ---- the layout, as k_mlp_update writes it ----
__device__ inline uint16_t skp_bf16(float f) {  // round to nearest even, on the bit pattern
  uint32_t u;
  memcpy(&u, &f, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ inline float skp_bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// what the high half leaves over, again rounded to bf16: f = hi + lo to 16 significant bits
__device__ inline uint16_t skp_bf16_lo(float f) { return skp_bf16(f - skp_bf16_to_float(skp_bf16(f))); }

// The two hidden layers are stored times 2 / ln 2 (weights AND biases, before the rounding to bf16 / the split into two bf16): their
// accumulators are then the exponent of tanh(x) = 1 - 2 / (2^(x 2 / ln 2) + 1) as they stand - no multiply per activation (skyjo_policy.hip)
__device__ inline float skp_scaled(float w) { return SKP_SCALE * w; }
// the high (or only) half of a weight of layer 2 / 3.  bf16 mode: the layer takes r = (1 - tanh) / 2 of the layer before: - 2 W as
// weights (exact: a power of two), W 1 joins the bias (skp_bias_sum)
__device__ inline uint16_t skp_hi(float v, bool split) { return split ? skp_bf16(v) : skp_bf16(-2.0f * v); }

// element j of the fragment of lane l: which k it holds.  Layer 1 in natural order (the kernel builds that operand from the record
// itself), layers 2 and 3 in the order the accumulators of the layer before come out (hh = l >> 5)
// Layer 1 takes KS = obs_dim / 16 + 1 k-steps (at least the narrow nets' two), K = 16 KS columns: column k < obs_dim is feature k, column K - 1
// carries b1 against a constant 1, the columns between are zero.  obs_dim <= 31: KS = 2 and the bias in column 31; 47: K = 48, the bias in the
// last free column; 48: KS = 4.
__host__ __device__ inline int skp_w1_ksteps(int obs_dim) { return obs_dim < 16 ? 2 : obs_dim / 16 + 1; }
__device__ inline int skp_w1_k(int s, int hh, int j) { return 16 * s + 8 * hh + j; }
__device__ inline int skp_acc_k(int ks, int hh, int j) { return 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * hh + (j & 3); }
__device__ inline int skp_row(int u, int l) { return 32 * u + (l & 31); }
// where a fragment lies, counted in fragments of 8 values
__device__ inline size_t skp_w1_frag(int u, int s, int l, int ks) { return ((size_t)u * ks + s) * 64 + l; }
__device__ inline size_t skp_w2_frag(int u, int ks, int l) { return ((size_t)u * 16 + ks) * 64 + l; }
__device__ inline size_t skp_w3_frag(int ks, int l) { return (size_t)ks * 64 + l; }
// b3 lies in accumulator layout, [64 lanes][16 registers]: the output row of register r of a lane of half hh
__device__ inline int skp_b3_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
// b2's entry (scaled = true) or a row bias of b3: the bias, and in bf16 mode + W 1 with the row's weights as they are stored:
// bf16-rounded, added in double in ascending k
__device__ inline float skp_bias_sum(float bias, const float *row, bool scaled, bool split) {
  double b = (double)(scaled ? skp_scaled(bias) : bias);
  if (!split)
    for (int k = 0; k < SKP_HIDDEN; k++) b += (double)skp_bf16_to_float(skp_bf16(scaled ? skp_scaled(row[k]) : row[k]));
  return (float)b;
}

// The pieces of the blob, in the order skyjo_vec_mlp_export writes them: w1, w2, w3, b2, b3, w1l, w2l, w3l (bytes; the *l pieces are
// empty in bf16 mode; ks: layer 1's k-steps, skp_w1_ksteps).  In a skyjo_vec_mlp's blob each starts at a 256-byte boundary:
// skp_piece_offset, piece 8 being the blob's size.
__host__ __device__ inline size_t skp_piece_bytes(int piece, bool split, int ks) {
  switch (piece) {
    case 0: return (size_t)SKU_W1_FRAGS(ks) * 16;
    case 1: return (size_t)SKU_W2_FRAGS * 16;
    case 2: return (size_t)SKU_W3_FRAGS * 16;
    case 3: return (size_t)SKP_HIDDEN * 4;
    case 4: return (size_t)64 * 16 * 4;
    case 5: return split ? (size_t)SKU_W1_FRAGS(ks) * 16 : 0;
    case 6: return split ? (size_t)SKU_W2_FRAGS * 16 : 0;
    default: return split ? (size_t)SKU_W3_FRAGS * 16 : 0;
  }
}
__host__ __device__ inline size_t skp_piece_offset(int piece, bool split, int ks) {
  size_t o = 0;
  for (int k = 0; k < piece; k++) o += (skp_piece_bytes(k, split, ks) + 255) & ~(size_t)255;
  return o;
}

// ---- the Adam state of one net: exp_avg of the six tensors back to back, padded to SKU_STATE_ALIGN floats, then exp_avg_sq ----
#define SKU_STATE_ALIGN 64
__host__ __device__ inline size_t sku_tensor_elems(int i, int obs_dim, int out_dim) {
  switch (i) {
    case 0: return (size_t)SKP_HIDDEN * obs_dim;
    case 1: return SKP_HIDDEN;
    case 2: return (size_t)SKP_HIDDEN * SKP_HIDDEN;
    case 3: return SKP_HIDDEN;
    case 4: return (size_t)out_dim * SKP_HIDDEN;
    default: return (size_t)out_dim;
  }
}
__host__ __device__ inline size_t sku_tensor_offset(int i, int obs_dim, int out_dim) {  // (every tensor but b3 is a multiple of 256 floats)
  size_t o = 0;
  for (int k = 0; k < i; k++) o += sku_tensor_elems(k, obs_dim, out_dim);
  return o;
}
__host__ __device__ inline size_t sku_state_half(int obs_dim, int out_dim) {
  const size_t n = sku_tensor_offset(SKU_TENSORS, obs_dim, out_dim);
  return (n + SKU_STATE_ALIGN - 1) / SKU_STATE_ALIGN * SKU_STATE_ALIGN;
}

struct SkUpdArgs {
  float *p[SKU_TENSORS];        // w1 [256][obs_dim], b1 [256], w2 [256][256], b2 [256], w3 [out_dim][256], b3 [out_dim]; w2, w3 16-byte aligned
  const float *g[SKU_TENSORS];  // ADAM only: the gradients, same shapes (read only)
  float *m, *v;                 // ADAM only: exp_avg / exp_avg_sq, tensor i at sku_tensor_offset(i)
  size_t off[SKU_TENSORS];
  uint4 *f1, *f2, *f3, *g1, *g2, *g3;  // the blob's fragment pieces (g*: the low halves, split only)
  float *c2, *c3;
  int obs_dim, out_dim, split;
  // torch.optim.Adam's scalars, rounded to float32 once on the host: 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), sqrt(1 - beta2^t), eps
  float w1, beta2, w2, step_size, bc2_sqrt, eps;
  // ADAM only, skyjo_vec_mlp_adam_step_clipped: the clipping coefficient on the device (skyjo_clip.h) - the rule takes g * *coef, one
  // rounded float32 multiply, for g.  Null: g as it is, skyjo_vec_mlp_adam_step bit for bit
  const float *coef;
};

// both views of a blob, from its base: the net kernels' (read only; no low halves in bf16 mode) and k_mlp_update's
inline void skp_blob_views(void *blob, bool split, int obs_dim, SkMlpDev &net, SkUpdArgs &a) {
  uint8_t *b = (uint8_t *)blob;
  const int ks = skp_w1_ksteps(obs_dim);
  net.w1 = a.f1 = (uint4 *)(b + skp_piece_offset(0, split, ks)), net.w2 = a.f2 = (uint4 *)(b + skp_piece_offset(1, split, ks));
  net.w3 = a.f3 = (uint4 *)(b + skp_piece_offset(2, split, ks));
  net.b2 = a.c2 = (float *)(b + skp_piece_offset(3, split, ks)), net.b3 = a.c3 = (float *)(b + skp_piece_offset(4, split, ks));
  net.w1l = a.g1 = split ? (uint4 *)(b + skp_piece_offset(5, split, ks)) : nullptr;
  net.w2l = a.g2 = split ? (uint4 *)(b + skp_piece_offset(6, split, ks)) : nullptr;
  net.w3l = a.g3 = split ? (uint4 *)(b + skp_piece_offset(7, split, ks)) : nullptr;
  net.split = a.split = split ? 1 : 0;
}

// torch.optim.Adam (no amsgrad, no weight decay) on one element, in torch's single-tensor operation order:
//   m <- m + (g - m) (1 - beta1);  v <- v beta2 + ((1 - beta2) g) g;  p <- p + (-step_size m) / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// g == 0 with m == v == 0 leaves p's bits as they are (p + -0).
__device__ inline float sku_adam(const SkUpdArgs &a, float p, float g, float &m, float &v) {
  m = m + (g - m) * a.w1;
  v = v * a.beta2 + (a.w2 * g) * g;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  return p + (-a.step_size * m) / denom;
}

// the gradient the rule takes: g, or with a coefficient g * coef
__device__ inline float sku_grad(const SkUpdArgs &a, float g, float coef) { return a.coef ? g * coef : g; }

// coef: *a.coef, read once per thread (k_mlp_update); counts with a.coef only
template <bool ADAM>
__device__ inline float sku_elem(const SkUpdArgs &a, int tensor, size_t i, float coef) {
  float p = a.p[tensor][i];
  if (ADAM) {
    const size_t s = a.off[tensor] + i;
    float m = a.m[s], v = a.v[s];
    p = sku_adam(a, p, sku_grad(a, a.g[tensor][i], coef), m, v);
    a.p[tensor][i] = p, a.m[s] = m, a.v[s] = v;
  }
  return p;
}

// four consecutive elements of w2 / w3 (i a multiple of 4: 16-byte accesses)
template <bool ADAM>
__device__ inline void sku_elem4(const SkUpdArgs &a, int tensor, size_t i, float *out, float coef) {
  const float4 p = *(const float4 *)(a.p[tensor] + i);
  out[0] = p.x, out[1] = p.y, out[2] = p.z, out[3] = p.w;
  if (ADAM) {
    const size_t s = a.off[tensor] + i;
    const float4 g = *(const float4 *)(a.g[tensor] + i), m4 = *(const float4 *)(a.m + s), v4 = *(const float4 *)(a.v + s);
    float gg[4] = {g.x, g.y, g.z, g.w}, m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = sku_adam(a, out[j], sku_grad(a, gg[j], coef), m[j], v[j]);
    *(float4 *)(a.p[tensor] + i) = make_float4(out[0], out[1], out[2], out[3]);
    *(float4 *)(a.m + s) = make_float4(m[0], m[1], m[2], m[3]);
    *(float4 *)(a.v + s) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

__device__ inline uint4 sku_pack8(const uint16_t *h) {
  return make_uint4((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16),
                    (uint32_t)h[4] | ((uint32_t)h[5] << 16), (uint32_t)h[6] | ((uint32_t)h[7] << 16));
}

// the fragment of eight values x (already scaled where the layer is): high halves to hi[at], low halves to lo[at] in split mode
__device__ inline void sku_store_frag(const float *x, bool split, bool fold, uint4 *hi, uint4 *lo, size_t at) {
  uint16_t h[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    h[j] = fold ? skp_hi(x[j], split) : skp_bf16(x[j]);
    l[j] = skp_bf16_lo(x[j]);
  }
  hi[at] = sku_pack8(h);
  if (split) lo[at] = sku_pack8(l);
}

template <bool ADAM>
__global__ __launch_bounds__(SKU_THREADS) void k_mlp_update(SkUpdArgs a) {
  __shared__ float rowb[32];
  const int t = threadIdx.x, l = t & 63, ks = t >> 6, hh = l >> 5;
  const bool split = a.split != 0;
  const int k0 = skp_acc_k(ks, hh, 0);  // the fragment's k are k0 .. k0 + 3 and k0 + 8 .. k0 + 11
  const float coef = ADAM && a.coef ? *a.coef : 1.f;
  if (blockIdx.x < 8) {
    const int u = blockIdx.x, m = skp_row(u, l);
    float x[8];
    sku_elem4<ADAM>(a, 2, (size_t)m * SKP_HIDDEN + k0, x, coef);
    sku_elem4<ADAM>(a, 2, (size_t)m * SKP_HIDDEN + k0 + 8, x + 4, coef);
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = skp_scaled(x[j]);
    sku_store_frag(x, split, true, a.f2, a.g2, skp_w2_frag(u, ks, l));
    const int ks1 = skp_w1_ksteps(a.obs_dim);
    if (t < 64 * ks1) {  // (ks is the k-step s of layer 1 here)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = skp_w1_k(ks, hh, j);
        x[j] = skp_scaled(k < a.obs_dim ? sku_elem<ADAM>(a, 0, (size_t)m * a.obs_dim + k, coef) : (k == 16 * ks1 - 1 ? sku_elem<ADAM>(a, 1, m, coef) : 0.f));
      }
      sku_store_frag(x, split, false, a.f1, a.g1, skp_w1_frag(u, ks, l, ks1));
    }
    __syncthreads();  // the workgroup's rows of w2 are written: bf16 mode sums them
    if (t < 32) {
      const int row = 32 * u + t;
      a.c2[row] = skp_bias_sum(sku_elem<ADAM>(a, 3, row, coef), a.p[2] + (size_t)row * SKP_HIDDEN, true, split);
    }
  } else {
    const int m = l & 31;
    float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (m < a.out_dim) {
      sku_elem4<ADAM>(a, 4, (size_t)m * SKP_HIDDEN + k0, x, coef);
      sku_elem4<ADAM>(a, 4, (size_t)m * SKP_HIDDEN + k0 + 8, x + 4, coef);
    }
    sku_store_frag(x, split, true, a.f3, a.g3, skp_w3_frag(ks, l));
    __syncthreads();
    if (t < 32) rowb[t] = t < a.out_dim ? skp_bias_sum(sku_elem<ADAM>(a, 5, t, coef), a.p[4] + (size_t)t * SKP_HIDDEN, false, split) : 0.f;
    __syncthreads();
    if (t < 256) {  // lane t / 4, registers 4 q .. 4 q + 3: the rows 8 q + 4 hh + 0 .. 3
      const int lane = t >> 2, q = t & 3, r0 = skp_b3_row(4 * q, lane >> 5);
      *(float4 *)(a.c3 + (size_t)lane * 16 + 4 * q) = make_float4(rowb[r0], rowb[r0 + 1], rowb[r0 + 2], rowb[r0 + 3]);
    }
  }
}
