// skyjo_record.h - part of skyjo_device.h (included from there, in its place: the parts build on each other in that order).
// The output record (collect_observation + action mask) and the bank of pre-dealt episodes.
#pragma once
#ifndef SKYJO_DEVICE_PARTS
#error "include skyjo_device.h"
#endif

// ------------------------------------------------------------------------------------------
// collect_observation (skyjo.py:148-199) + action mask (skyjo.py:201-224) -> output record.
// obs[0..16] are a straight copy of state bytes 16..32, obs[17] / obs[18] come from the header
// registers; the card part is the observer's `vis` row (indirect) or all rows in absolute seat
// order (direct, skyjo.py:279-302).
// ------------------------------------------------------------------------------------------
template <bool INDIRECT>
__device__ __forceinline__ void emit_record(const SkParams &P, uint8_t *lp, const HdrRegs &h, const ObsRegs &ob, int action,
                                            uint8_t *out, uint4 *held = nullptr, const uint4 *pre_a = nullptr, uint32_t pre_b = 0) {
  const int phase = h.w0 & 0xff;
  const uint32_t q0 = ob.q0, q1 = ob.q1, q2 = ob.q2;
  const uint32_t act24 = ((uint32_t)action & 0xffu) << 24;  // byte D of the record: the action this step applied (-1: none)
  uint32_t m[8];
  {
    // (computed in both phases and masked: a branch on the phase measured 2 us slower per launch)
    const uint32_t pm = phase ? 0xffffffffu : 0u;
    m[0] = ob.nz0 & pm, m[1] = ob.nz1 & pm, m[2] = ob.nz2 & pm, m[3] = ob.hd0 & pm, m[4] = ob.hd1 & pm, m[5] = ob.hd2 & pm;
    m[6] = (phase ? 0u : 0x0101u) | (((h.w0 >> 8) & 0xffu) << 16) | ((uint32_t)phase << 24);
    m[7] = (((h.w0 >> 16) & F_DONE) ? 1u : 0u) | ((h.w0 >> 24) << 8) | ((h.w2 & 0xffffu) << 16);
  }
  // obs[0..15] are chunk 1 of the record; obs[16] = hist[14], obs[17] = discard top, obs[18] = hand card
  const uint4 a = pre_a ? *pre_a : LQ(1);  // (pre_*: the caller has requested them together with the row)
  const uint32_t s8 = (pre_a ? pre_b : (uint32_t)LB(32)) | ((h.w1 >> 24) << 8) | ((h.w2 >> 24) << 16);
  if (INDIRECT) {
    uint4 *o = (uint4 *)out;
    uint4 b;
    b.x = s8 | (q0 << 24), b.y = (q0 >> 8) | (q1 << 24), b.z = (q1 >> 8) | (q2 << 24), b.w = (q2 >> 8) | act24;
    if (held) {  // the caller stores the record itself
      held[0] = a, held[1] = b, held[2] = make_uint4(m[0], m[1], m[2], m[3]), held[3] = make_uint4(m[4], m[5], m[6], m[7]);
    } else {
      o[0] = a, o[1] = b;
      o[2] = make_uint4(m[0], m[1], m[2], m[3]);
      o[3] = make_uint4(m[4], m[5], m[6], m[7]);
    }
  } else {
    // direct observation (skyjo.py:279-302): every player's visible row in absolute seat order, 12 bytes each, packed
    // behind obs[18]; a row is one chunk read
    uint32_t *o = (uint32_t *)out;
    const int N = P.L.N;
    o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
    uint32_t carry = s8;  // three bytes waiting for the next word's top byte
    for (int p = 0; p < N; p++) {
      const uint4 r = LQ((sk_pb(P.L, p) + PB_VIS) >> 4);
      o[4 + 3 * p] = carry | (r.x << 24);
      o[5 + 3 * p] = (r.x >> 8) | (r.y << 24);
      o[6 + 3 * p] = (r.y >> 8) | (r.z << 24);
      carry = r.z >> 8;
    }
    o[4 + 3 * N] = carry | act24;
    uint32_t *om = o + (P.L.Dp >> 2);
#pragma unroll
    for (int w = 0; w < 8; w++) om[w] = m[w];
  }
}

// ------------------------------------------------------------------------------------------
// Take the pre-dealt next episode (SkyjoGame.reset, skyjo.py:52-74; the dealing itself is k_deal).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t bank_rec16(const SkParams &P, int slot, int g) {  // first 16-byte piece of the bank record (slot, game)
  return ((size_t)slot * P.tiles * SK_TILE + (size_t)g) * P.L.chunks;
}
__device__ __forceinline__ void load_spare(const SkParams &P, uint8_t *lp, int slot, int tile, int lane) {
  const uint4 *s = P.spare + bank_rec16(P, slot, tile * SK_TILE + lane);
  const int n = P.L.chunks;
  for (int c = 0; c < n; c += 6) {  // (groups of six as in tile_load: one memory round trip per group)
    uint4 v[6];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (c + k < n) v[k] = s[c + k];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (c + k < n) LQ(c + k) = v[k];
  }
}
__device__ __forceinline__ void store_spare(const SkParams &P, uint8_t *lp, int slot, int g) {  // the lane's record in LDS -> its bank slot
  uint4 *d = P.spare + bank_rec16(P, slot, g);
  const int n = P.L.chunks;
  for (int c = 0; c < n; c += 6) {
    uint4 v[6];
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (c + k < n) v[k] = LQ(c + k);
#pragma unroll
    for (int k = 0; k < 6; k++)
      if (c + k < n) d[c + k] = v[k];
  }
}

__device__ __forceinline__ void bank_advance(const SkParams &P, uint8_t *lp, int g, int head, uint32_t dc) {
  const uint8_t nh = (uint8_t)((head + 1) % SK_BANK);
  P.bank_head[g] = nh;
  LB(H_BANK) = nh;
  P.deals_consumed[g] = dc + 1;
  P.done[g] = 0;
}

// k_reset / generic form: plain loads, the record passes through registers.  Returns false (slot untouched) when the
// bank is empty.
__device__ __forceinline__ bool consume_spare(const SkParams &P, uint8_t *lp, int tile, int lane, int g, int head) {
  const size_t G = (size_t)P.tiles * SK_TILE;
  const uint8_t ready = P.spare_ready[(size_t)head * G + g];
  const uint32_t dc = P.deals_consumed[g];
  if (!ready) return false;
  load_spare(P, lp, head, tile, lane);
  P.spare_ready[(size_t)head * G + g] = 0;  // k_scan finds the banks that are not full
  bank_advance(P, lp, g, head, dc);
  return true;
}

// The step kernel's form, in two halves: a request, and a commit that waits for everything this wavefront has in flight and
// finishes the hand-over.  Between the two the wavefront steps its live games, which hides the memory round trip of the few
// lanes that are resetting (about every second iteration has one).  If the bank turns out to be empty the slot holds a stale
// record: the caller deals in place, which rewrites every word of it.
// Two forms of the pair.  `spare_issue` / `spare_commit` (steps with caller actions, two players and the generic player counts, and the games
// beyond the cooperative group below): the resetting lane asks for its whole record by LDS-DMA straight into its own (dead: its
// game is over) slot of the tile - no registers, no LDS writes, but one instruction per 16-byte piece that occupies all 64 lanes
// for one or two games.  `spare_issue_coop` / `spare_commit_coop` (the fused rollouts at three and four players): the wavefront
// fetches the record together, one load and one LDS write (further down).
// (Measured and dropped in round 3, EXPERIMENTS.md: the bookkeeping words kept in registers for the whole launch - same time; the
// record requested a whole iteration earlier, when the game ends - slower.  Round 5 #5: a cooperative fetch through loads the
// COMPILER tracked - slower, for the waits and copies it placed; the cooperative form below keeps its load out of its sight.)
struct SpareRegs {
  uint32_t dc;
  int head;
  uint8_t ready;
};
__device__ __forceinline__ void spare_issue(const SkParams &P, uint8_t *lp, uint32_t lds_tile, int tile, int lane, int g, SpareRegs &r) {
  const size_t G = (size_t)P.tiles * SK_TILE;
  r.head = LB(H_BANK) % SK_BANK;  // (read before the record is overwritten)
  r.ready = P.spare_ready[(size_t)r.head * G + g];
  r.dc = P.deals_consumed[g];
  const uint32_t voff = (uint32_t)(bank_rec16(P, r.head, g) * 16);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every LDS read of the old record has returned
  dma_bank_record<false>((const uint8_t *)P.spare, voff, lds_tile, P.L.chunks);
}
__device__ __forceinline__ bool spare_commit(const SkParams &P, uint8_t *lp, int g, const SpareRegs &r) {
  sk_vm_drain();
  if (!r.ready) return false;
  P.spare_ready[(size_t)r.head * (size_t)P.tiles * SK_TILE + g] = 0;  // the dealing run finds the banks that are not full
  bank_advance(P, lp, g, r.head, r.dc);
  return true;
}

// The fused rollouts' form at three and four players (step_body with the on-device policy), cooperative: the record of
// (slot, game) is CH = `chunks` consecutive 16-byte pieces of the game-major bank, and a resetting game is one lane in about a
// hundred - so the WAVEFRONT fetches it, GP = 64 / CH = 3 games at a time: lane CH * k + j takes piece j of the k-th resetting
// game with ONE global_load_dwordx4, and writes it at commit time with ONE ds_write_b128 into that game's column of the tile
// (lds_tile + j * 1024 + lane_k * 16).  Both functions are entered like the two above - by the resetting lanes only, at the same
// places - and switch the other lanes on for the few instructions that need them (lanes without a game included: they are fetch
// lanes, never a source of `head` / `g`).  With fewer than GP resetting games the idle groups fetch and write the FIRST game's
// pieces once more (same bytes to the same address).  The request leaves the piece and its LDS address in five registers; the
// commit is the wait, one LDS write and nothing else.  (Measured, EXPERIMENTS.md: switching the idle groups off - a mask
// computed from the number of games - was 0.7 % slower.)  Resetting games beyond the first GP of an iteration (0.95 % of the
// lanes reset per iteration: rare) take the LDS-DMA of spare_issue.
// The load is asm volatile: the compiler neither counts it nor waits for it, and the
// one wait is the hand-placed vmcnt(0) of the commit - the same wait as spare_commit's (loads and stores share vmcnt and retire
// in order on this ISA family: nothing weaker is to be had once record stores may be in flight).
// What it costs: the LDS write of the commit is on the wavefront's path (a game's pieces lie 1 KiB apart, i.e. on the same four
// banks), where the LDS-DMA landed beside the stepping lanes.  It pays where the step wavefront shares its SIMD's issue slots
// with a dealing wavefront (65 536 x 3: faster, EXPERIMENTS.md) and loses where it has the SIMD to itself (4 096 x 2, one workgroup of two
// wavefronts per CU: - 3.6 %, EXPERIMENTS.md) - the two-player kernels, whose BASELINE configuration is that small batch, keep
// the LDS-DMA.
// The registers the two statements write with lanes switched on that the surrounding code has switched off.  The compiler's
// register liveness assumes that a write inside a divergent region touches the region's lanes only, so a temporary DEFINED in
// there could be given a register that still holds state of the stepping lanes.  Hence sk_coop_reserve(): step_body defines all
// six under full EXEC at the top of the iteration, in front of `if (valid)`, and the statements take them as read-write ("+v")
// operands; sk_coop_release() reads d and a under full EXEC again at the end of the iteration.  The registers are then live for ALL
// lanes in between - also through the stepping lanes' branch, whose lanes hold the pieces while they step (a value that only the
// commit's branch reads is free for the stepping branch to overwrite: that is how a build without the release lost its pieces).
// What the compiler still may do is copy such a value under a divergent EXEC (a live-range split, an uncoalesced phi), which would
// move the owning lanes' part only: tools/check_coop_regs.py compiles the unit and verifies for every instantiation that reserve,
// request, commit and release name the same registers and that nothing else writes them in between (tests/test_coop_regs.py).
typedef uint32_t sk_u32x4 __attribute__((ext_vector_type(4)));
struct CoopRegs {
  sk_u32x4 d;     // the piece this lane fetches for a resetting game, from the request to the commit
  uint32_t a, t;  // a: its LDS address (lds_tile + j * 1024 + lane_k * 16); t: the request's scratch
};
__device__ __forceinline__ void sk_coop_reserve(CoopRegs &c) { asm volatile("; coop reserve %0 %1 %2" : "=v"(c.d), "=v"(c.a), "=v"(c.t)); }
__device__ __forceinline__ void sk_coop_release(const CoopRegs &c) { asm volatile("; coop release %0 %1" ::"v"(c.d), "v"(c.a)); }
// lanes [a, b) as an EXEC mask, its two halves (long long: the immediates print as 32-bit values)
__device__ __forceinline__ constexpr long long sk_lanes_lo(int a, int b) {
  return (long long)(((b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull)) & 0xffffffffull);
}
__device__ __forceinline__ constexpr long long sk_lanes_hi(int a, int b) {
  return (long long)(((b >= 64 ? ~0ull : (1ull << b) - 1ull) & ~((1ull << a) - 1ull)) >> 32);
}
#define SK_COOP_E0 "s_mov_b32 exec_lo, %[e0l]\n\ts_mov_b32 exec_hi, %[e0h]\n\t"  // lanes [0, 3 CH): all three groups
#define SK_COOP_E1 "s_mov_b32 exec_lo, %[e1l]\n\ts_mov_b32 exec_hi, %[e1h]\n\t"  // lanes [CH, 3 CH): the second and third
#define SK_COOP_E2 "s_mov_b32 exec_lo, %[e2l]\n\ts_mov_b32 exec_hi, %[e2h]\n\t"  // lanes [2 CH, 3 CH): the third
#define SK_COOP_MASKS(CH)                                                                                                   \
  [ch] "n"(CH), [e0l] "n"(sk_lanes_lo(0, 3 * CH)), [e0h] "n"(sk_lanes_hi(0, 3 * CH)), [e1l] "n"(sk_lanes_lo(CH, 3 * CH)),   \
      [e1h] "n"(sk_lanes_hi(CH, 3 * CH)), [e2l] "n"(sk_lanes_lo(2 * CH, 3 * CH)), [e2h] "n"(sk_lanes_hi(2 * CH, 3 * CH))
template <int CH>
__device__ __forceinline__ void spare_issue_coop(const SkParams &P, uint8_t *lp, uint32_t lds_tile, int lane, int g, SpareRegs &r, CoopRegs &c) {
  static_assert(64 / CH == 3, "three or four players: three games per group");
  const size_t G = (size_t)P.tiles * SK_TILE;
  r.head = LB(H_BANK) % SK_BANK;  // (read before the record is overwritten)
  r.ready = P.spare_ready[(size_t)r.head * G + g];
  r.dc = P.deals_consumed[g];
  const uint32_t voff = (uint32_t)(bank_rec16(P, r.head, g) * 16);
  // the first three resetting lanes (this code runs under their mask); absent ones = the first: its pieces are fetched and written again
  unsigned long long m = __builtin_amdgcn_ballot_w64(true);
  const int l0 = __ffsll((long long)m) - 1;
  m &= m - 1;
  const int l1 = m ? __ffsll((long long)m) - 1 : l0;
  m &= m - 1;
  const int l2 = m ? __ffsll((long long)m) - 1 : l0;
  m &= m - 1;
  const uint32_t s0 = __builtin_amdgcn_readlane(voff, l0), s1 = __builtin_amdgcn_readlane(voff, l1), s2 = __builtin_amdgcn_readlane(voff, l2);
  // LDS side: group k writes to column l_k - a0 for all, then the steps from one group's column to the next
  const uint32_t a0 = lds_tile + 16u * (uint32_t)l0, a1 = 16u * (uint32_t)(l1 - l0), a2 = 16u * (uint32_t)(l2 - l1);
  unsigned long long sv;
  // t = the lane's piece j = lane - CH * k, a = the k-th game's bank offset + 16 j -> the load; then a = a0 (+ a1 (+ a2)) + 1024 j
  // (the load stays BEHIND the dozen instructions in front of it: the compiler re-materialises P.spare's SGPR pair with v_readlane_b32, a
  // vector-memory instruction that reads an SGPR a VALU instruction wrote needs five wait states, and nobody inserts them inside a statement)
  asm volatile("; coop request %[d] %[a] %[t]\n\ts_mov_b64 %[sv], exec\n\t" SK_COOP_E0
               "v_mbcnt_lo_u32_b32 %[t], -1, 0\n\tv_mbcnt_hi_u32_b32 %[t], -1, %[t]\n\tv_mov_b32 %[a], %[s0]\n\t"
               SK_COOP_E1 "v_mov_b32 %[a], %[s1]\n\tv_subrev_u32 %[t], %[ch], %[t]\n\t"
               SK_COOP_E2 "v_mov_b32 %[a], %[s2]\n\tv_subrev_u32 %[t], %[ch], %[t]\n\t"
               SK_COOP_E0 "v_lshl_add_u32 %[a], %[t], 4, %[a]\n\tglobal_load_dwordx4 %[d], %[a], %[base]\n\t"
               "s_nop 0\n\tv_lshl_add_u32 %[a], %[t], 10, %[a0]\n\t"
               SK_COOP_E1 "v_add_u32 %[a], %[a1], %[a]\n\t"
               SK_COOP_E2 "v_add_u32 %[a], %[a2], %[a]\n\t"
               "s_mov_b64 exec, %[sv]"
               : [d] "+v"(c.d), [t] "+v"(c.t), [a] "+v"(c.a), [sv] "=&s"(sv)
               : [base] "s"(P.spare), [s0] "s"(s0), [s1] "s"(s1), [s2] "s"(s2), [a0] "s"(a0), [a1] "s"(a1), [a2] "s"(a2), SK_COOP_MASKS(CH)
               : "memory");
  if (SK_RARE(m != 0)) {  // (wavefront-uniform) more resetting games than one group serves
    if ((m >> lane) & 1) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every LDS read of the old record has returned
      dma_bank_record<false>((const uint8_t *)P.spare, voff, lds_tile, CH);
    }
#ifdef SK_DIAG
    // resets served by the LDS-DMA: word 7 of the tile's section sums, which only -DSK_STAMPS builds use otherwise (skyjo_vec_debug_stamps()[7])
    if (lane == l0) P.stamps[(size_t)(g / SK_TILE) * 8 + 7] += (unsigned long long)__popcll(m);
#endif
  }
}
template <int CH>
__device__ __forceinline__ bool spare_commit_coop(const SkParams &P, uint8_t *lp, int g, const SpareRegs &r, const CoopRegs &c) {
  unsigned long long sv;
  // everything this wavefront has in flight (the pieces, the LDS-DMA of the games beyond the group), then the pieces into the tile
  asm volatile("; coop commit %[d] %[a]\n\ts_waitcnt vmcnt(0)\n\ts_mov_b64 %[sv], exec\n\t" SK_COOP_E0 "ds_write_b128 %[a], %[d]\n\ts_waitcnt lgkmcnt(0)\n\ts_mov_b64 exec, %[sv]"
               : [sv] "=&s"(sv)
               : [a] "v"(c.a), [d] "v"(c.d), SK_COOP_MASKS(CH)
               : "memory");
  if (!r.ready) return false;
  P.spare_ready[(size_t)r.head * (size_t)P.tiles * SK_TILE + g] = 0;  // the dealing run finds the banks that are not full
  bank_advance(P, lp, g, r.head, r.dc);
  return true;
}

// LDS stride of one staged record: the record's own size, plus 16 bytes when that is a multiple of 32 dwords / 4 - the
// lane-per-record dword writes then spread over 8 banks groups instead of 4.
__device__ __forceinline__ constexpr int sk_stage_stride(int rec_bytes) { return ((rec_bytes >> 2) & 7) == 0 ? rec_bytes + 16 : rec_bytes; }

// Fallback when the pre-dealt episode is not available inside a launch (a mid-game reshuffle just
// invalidated it, or the game already took one in this launch): deal right here, on this lane, from
// the game's current stream position.  Rare and slow (one lane active), never changes results.
// When the game's stream cannot be had (wait_deal_done timed out: sticky device error) stream and bank stay untouched and
// the slot is left as a finished game: it asks again in the next iteration.
// Returns false in that case: the caller must not present the slot as a freshly re-dealt game (status stays ERROR, no reset counted).
__device__ __forceinline__ bool deal_inline(const SkParams &P, uint8_t *lp, uint8_t *fp, int g, int tile, int lane, int head);
