// skyjo_learner_util.h - what more than one of the learner unit's kernel headers needs, and nothing else: the wavefront sum their
// reductions share, the store loop over a run's flat float stretch, and the records of a rollout buffer.  Each header that uses one of
// the three includes this file itself.  No part of the environment's sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "skyjo_host.h"
#include "skyjo_layout.h"

// the sum of a wavefront, the same bits in every lane: x[l] + x[l ^ 32], then ^ 16, ... ^ 1
__device__ __forceinline__ double sk_wave_sum(double x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// A workgroup of THREADS lanes writes a run's flat [rows * rowlen] float stretch, total = rows * rowlen elements from dst (16-byte
// aligned): four consecutive elements per lane and round, a whole group as one 16-byte store, the last partial group element by element.
// at(i, k) gives element k of row i; it is called for elements below total only, once each.
template <int THREADS, class F>
__device__ __forceinline__ void sk_store_stretch(float *dst, int total, int rowlen, F at) {
  for (int e = threadIdx.x * 4; e < total; e += THREADS * 4) {
    int i = e / rowlen, k = e - i * rowlen;
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      x[j] = e + j < total ? at(i, k) : 0.f;
      if (++k == rowlen) k = 0, i++;
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

// The records of a [T (+ 1)] rollout buffer in either layout.  Step t holds B games; its records start rec_stride records behind those
// of step t - 1 (B row-major, tiles * 64 tile-planar: the padding slots of a partial tile are never rows).
struct SkRecords {
  const uint8_t *rec;
  long long rec_stride;
  int32_t B, rec_bytes, planar;
#ifdef __HIPCC__
  // the record number of game b in step t, and of row id r = t * B + b (row-major that is r itself: no division)
  __device__ __forceinline__ long long at(long long t, long long b) const { return t * rec_stride + b; }
  __device__ __forceinline__ long long of_row(long long r) const {
    if (!planar) return r;
    const long long t = r / B;
    return at(t, r - t * B);
  }
  // byte k of record q (sk_rec_byte: never reached from a neighbouring byte's pointer)
  __device__ __forceinline__ const uint8_t *byte(long long q, int k) const { return sk_rec_byte(rec, q, k, rec_bytes, planar); }
#endif
};

static inline SkRecords sk_records(const SkEngineView &e, const void *records, int32_t layout) {
  SkRecords r{};
  r.rec = (const uint8_t *)records, r.planar = layout == SKYJO_REC_TILE_PLANAR;
  r.rec_stride = r.planar ? (long long)e.G : (long long)e.B;
  r.B = e.B, r.rec_bytes = e.L->rec_bytes;
  return r;
}
