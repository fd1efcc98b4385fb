/*
 * skyjo_vec.h - C ABI of the MI355X-native vectorised SkyJo environment (libskyjo_vec.so).
 *
 * This is the drop-in boundary for ONE hot path of michaelfeil/skyjo_rl: the SkyJo state transition
 * plus observation / action-mask build.  The reference has no FFI: the path sits behind two Python
 * classes, so every entry point below cites the Python interface it replaces
 * (paths relative to the reference checkout):
 *
 *   SkyjoGame.__init__ / reset / set_seed      rlskyjo/game/skyjo.py:20-49, 52-74, 84-94
 *   SkyjoGame.collect_observation              rlskyjo/game/skyjo.py:148-199 (+ helpers :201-302)
 *   SkyjoGame.act                              rlskyjo/game/skyjo.py:308-335 (+ :337-498)
 *   SkyjoGame.get_game_metrics/expected_action rlskyjo/game/skyjo.py:500-504
 *   SimpleSkyjoEnv.step / reset / seed         rlskyjo/environment/skyjo_env.py:216-252, 254-267, 280-290
 *   SimpleSkyjoEnv._calc_final_rewards         rlskyjo/environment/skyjo_env.py:293-312
 *   TerminateIllegalWrapper(illegal_reward=-1) rlskyjo/environment/skyjo_env.py:23
 *
 * All games of a handle share one configuration and live on ONE GPU in an LDS-friendly tiled
 * structure-of-arrays layout.  Unless a parameter is named *_host, data pointers are
 * DEVICE pointers (e.g. torch tensor .data_ptr()); buffers are caller-owned, the handle owns its
 * state.  `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls on one
 * handle must be serialised by the caller; every call is asynchronous on `stream` unless it has a
 * host output.  Return value: 0 = ok, negative = SKYJO_E_*; skyjo_vec_last_error() describes the
 * last failure on the calling thread.  Game-level illegal actions are data (status byte), never
 * errors.  There is NO CPU fallback: without a gfx950 device skyjo_vec_create fails.
 */
#ifndef SKYJO_VEC_H
#define SKYJO_VEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKYJO_ABI_VERSION 4
#define SKYJO_MAX_PLAYERS 12 /* skyjo.py:24-26 */
#define SKYJO_NUM_ACTIONS 26 /* skyjo.py:46 */
#define SKYJO_NUM_CARDS 150  /* skyjo.py:80 */
#define SKYJO_HAND_NONE 15   /* skyjo.py:33 */
#define SKYJO_REFUNDED (-14) /* skyjo.py:34 */

/* error codes */
#define SKYJO_OK 0
#define SKYJO_E_INVALID (-1) /* bad argument / handle */
#define SKYJO_E_DEVICE (-2)  /* HIP runtime error (text in last_error) */
#define SKYJO_E_NOGPU (-3)   /* no usable gfx950 device */
#define SKYJO_E_STATE (-4)   /* call not valid in the current state (e.g. step before seed) */

/* per-game status byte of the last step */
#define SKYJO_ST_OK 0        /* action applied */
#define SKYJO_ST_ILLEGAL 1   /* action masked out or out of range: TerminateIllegalWrapper semantics */
#define SKYJO_ST_NOOP_DONE 2 /* game already over and auto_reset off (skyjo.py:316-321) */
#define SKYJO_ST_RESET 3     /* game was over: a new episode was dealt, the action was ignored */
#define SKYJO_ST_ERROR 4     /* the engine raised a device error (skyjo_vec_check_error): this episode was cut off / could not be dealt */

/* skyjo_vec_step: a game whose action is SKYJO_ACTION_SKIP is left exactly as it is (no step, no reset; its record is
 * still written) - the single-game views use it to step ONE game of a shared engine (SkyjoGame(engine=, index=)). */
#define SKYJO_ACTION_SKIP (-1000)

/* RNG modes */
#define SKYJO_RNG_MT19937 0 /* numpy legacy stream, bit-identical deals to the reference */
#define SKYJO_RNG_PHILOX 1  /* counter-based Philox4x32-10 sessions, same shuffle algorithm */

typedef struct skyjo_vec skyjo_vec; /* opaque */

typedef struct skyjo_vec_config {
  int32_t abi_version;      /* SKYJO_ABI_VERSION */
  int32_t num_envs;         /* parallel games on this device */
  int32_t num_players;      /* 1..12                       (skyjo.py:21) */
  int32_t observe_indirect; /* observe_other_player_indirect (skyjo.py:42-45) */
  double score_penalty;     /* skyjo.py:21,496-497 */
  double mean_reward;       /* skyjo_env.py:43,308 */
  double reward_refunded;   /* skyjo_env.py:44,310-311 */
  double illegal_reward;    /* skyjo_env.py:23 (-1) */
  int32_t device_id;        /* HIP device ordinal */
  int32_t rng_mode;         /* SKYJO_RNG_* */
  int32_t auto_reset;       /* 1: a finished game is re-dealt by the next step */
  int32_t reserved;
  uint64_t game_id0;        /* global id of local game 0 (multi-GPU shards; seeds and policy keys use it) */
} skyjo_vec_config;

/* Output record: one per game per step, `record_bytes` long (64 for the indirect observation):
 *   [0, D)            int8 observations            (skyjo.py:180-190)
 *   [D]               int8 the action the step that wrote this record applied to the game (-1: none - the game was
 *                     reset / already over / skipped, or the record comes from reset / observe; -2: the caller's action
 *                     was outside 0 .. 25 and refused as illegal); D is odd, so the byte is the padding between the
 *                     observation and the mask
 *   [Dp, Dp+26)       int8 action_mask, Dp = (D+3)&~3 (skyjo.py:201-224)
 *   [Dp+26]           expected player (agent id)   (skyjo.py:503)
 *   [Dp+27]           phase 0 = draw, 1 = place
 *   [Dp+28]           done                         (skyjo_env.py:247)
 *   [Dp+29]           status SKYJO_ST_*
 *   [Dp+30, Dp+32)    uint16 steps in this episode */
typedef struct skyjo_vec_info {
  int32_t num_envs, num_players, obs_dim, record_bytes;
  int32_t mask_offset, meta_offset, state_bytes, tile_games;
} skyjo_vec_info;

typedef struct skyjo_vec_counters {
  uint64_t steps;    /* applied actions incl. the consumed terminal draw */
  uint64_t episodes; /* games that reached their natural end */
  uint64_t illegal;  /* games ended by an illegal action */
  uint64_t resets;   /* deals consumed */
  uint64_t sum_len;  /* sum of episode lengths of finished episodes */
  uint64_t reshuffles;
  uint64_t iters;    /* lockstep iterations executed */
  uint64_t waits;    /* deals made on the in-kernel slow path (pre-dealt episode not available) */
  double sum_score[SKYJO_MAX_PLAYERS];     /* per seat, finished episodes (skyjo.py:59) */
  double sum_reward[SKYJO_MAX_PLAYERS];    /* per seat, finished + illegal episodes (skyjo_env.py:293-312) */
  double sum_reward_sq[SKYJO_MAX_PLAYERS]; /* per seat, squares of the same rewards */
  double sum_refunded[SKYJO_MAX_PLAYERS];  /* per seat, num_refunded of finished episodes (skyjo.py:57) */
} skyjo_vec_counters;

/* Canonical per-game state (debug, fixtures, snapshot/restore).  Field names follow skyjo.py. */
typedef struct skyjo_game_state {
  int8_t players_cards[SKYJO_MAX_PLAYERS][12];  /* skyjo.py:63 */
  int8_t players_masked[SKYJO_MAX_PLAYERS][12]; /* skyjo.py:72, 0 refunded / 1 open / 2 hidden */
  int8_t drawpile[SKYJO_NUM_CARDS];             /* pop from the end, skyjo.py:366 */
  int8_t discard_pile[SKYJO_NUM_CARDS];         /* push/pop at the end, skyjo.py:370,393 */
  int16_t n_draw, n_disc;
  int8_t hand_card;        /* 15 = none */
  uint8_t expected_player; /* skyjo.py:144 */
  uint8_t expected_phase;  /* 0 draw / 1 place */
  uint8_t is_terminated;   /* skyjo.py:54 */
  uint8_t done;            /* env-level: terminated or ended by illegal action */
  uint8_t status;
  uint16_t episode_steps;
  uint32_t episode;        /* deals since seeding, 0 = the deal made by seed() */
  uint32_t reshuffles;
  int32_t num_refunded[SKYJO_MAX_PLAYERS]; /* skyjo.py:57 */
  int32_t num_placed[SKYJO_MAX_PLAYERS];   /* skyjo.py:58 */
  double final_score[SKYJO_MAX_PLAYERS];   /* skyjo.py:59, valid when is_terminated */
  double rewards[SKYJO_MAX_PLAYERS];       /* skyjo_env.py:244, valid when done */
} skyjo_game_state;

const char *skyjo_vec_last_error(void);
int skyjo_vec_abi_version(void);

/* SkyjoGame.__init__ + SimpleSkyjoEnv.__init__ (skyjo.py:20-49, skyjo_env.py:38-153) for num_envs games.
 * Unlike the reference no cards are dealt until skyjo_vec_seed. */
int skyjo_vec_create(const skyjo_vec_config *cfg, skyjo_vec **out);
int skyjo_vec_destroy(skyjo_vec *h);
int skyjo_vec_get_info(const skyjo_vec *h, skyjo_vec_info *out);

/* SkyjoGame.set_seed (skyjo.py:84-88) per game: game i is seeded with seeds_host[i], or with
 * base_seed + game_id0 + i when seeds_host is NULL; the legacy stream is seeded with value+1 and
 * the first deal is made immediately, exactly like set_seed.  Must precede every other call. */
int skyjo_vec_seed(skyjo_vec *h, const uint64_t *seeds_host, uint64_t base_seed, void *stream);
/* SkyjoGame.set_seed (skyjo.py:84-88) for ONE game of the batch: its stream is re-seeded with value + 1, its bank of
 * pre-dealt episodes is dealt again and the first deal becomes the live game.  The other games are untouched. */
int skyjo_vec_seed_one(skyjo_vec *h, int32_t game, uint64_t value, void *stream);

/* SkyjoGame.reset / SimpleSkyjoEnv.reset (skyjo.py:52-74, skyjo_env.py:254-267) for the games whose
 * mask byte is non-zero (all when mask is NULL).  records_out (may be NULL): [num_envs][record_bytes]. */
int skyjo_vec_reset(skyjo_vec *h, const uint8_t *mask, void *records_out, void *stream);

/* SimpleSkyjoEnv.step (skyjo_env.py:216-252) = SkyjoGame.act (skyjo.py:308-335) for the expected player
 * of every game, then the observation of the next expected player.  actions: int32[num_envs]. */
int skyjo_vec_step(skyjo_vec *h, const int32_t *actions, void *records_out, void *stream);

/* `iters` lockstep iterations with the uniform random admissible policy (rlskyjo/models/random_admissible_policy.py:6-28)
 * evaluated on device.  The call is cut into launches at the dealing cadence (SKYJO_OPT_DEAL_INTERVAL); in the one-kernel
 * form (SKYJO_OPT_OVERLAP 3) up to 16 whole dealing cycles share ONE launch when the call asks for that many iterations at
 * once - the games' tiles then stay in LDS across the cycle ends (65 536 x 3: 37 -> 44 x 10^9 env-steps/s from 64 to 512+
 * iterations per call).  Results do not depend on how a caller slices its iterations into calls.
 * records_out: NULL, or [iters][num_envs][record_bytes] (record AFTER each iteration);
 * actions_out: NULL, or int32[iters][num_envs] (-1 where no action was applied) - the same value is byte D of every
 * record, so a caller that keeps the records does not need this array. */
int skyjo_vec_rollout(skyjo_vec *h, int32_t iters, uint64_t policy_seed, void *records_out, int32_t *actions_out,
                      void *stream);

/* SimpleSkyjoEnv.observe (skyjo_env.py:199-214) = collect_observation(player) (skyjo.py:148-199) without
 * changing state.  players: int32[num_envs] or NULL for the expected player of each game. */
int skyjo_vec_observe(skyjo_vec *h, const int32_t *players, void *records_out, void *stream);

/* Split records into the reference's dense arrays: obs int8[n][D], mask int8[n][26]; any output may be NULL. */
int skyjo_vec_unpack(skyjo_vec *h, const void *records, int64_t n_records, int8_t *obs, int8_t *mask,
                     uint8_t *agent, uint8_t *phase, uint8_t *done, uint8_t *status, void *stream);
/* The same for records in the tile-planar layout (SKYJO_OPT_RECORD_LAYOUT = SKYJO_REC_TILE_PLANAR): `n_tiles` blocks of 64 records
 * (64 * record_bytes bytes each) in, dense rows of 64 n_tiles records out - [iters * tiles] blocks of a rollout give rows ordered
 * (iteration, tile, lane), i.e. (iteration, game) with the games of a partial last tile padded to 64. */
int skyjo_vec_unpack_tiles(skyjo_vec *h, const void *records, int64_t n_tiles, int8_t *obs, int8_t *mask,
                           uint8_t *agent, uint8_t *phase, uint8_t *done, uint8_t *status, void *stream);

/* rewards double[num_envs][num_players] (skyjo_env.py:293-312; valid where done), device pointers owned by h */
const double *skyjo_vec_rewards_ptr(const skyjo_vec *h);
const double *skyjo_vec_scores_ptr(const skyjo_vec *h);
const uint8_t *skyjo_vec_done_ptr(const skyjo_vec *h);

/* Sticky device error of the handle: 0, or SKYJO_E_DEVICE with the reason in skyjo_vec_last_error() - today the one case
 * is a step kernel that gave up waiting for the dealing kernel that should run beside it (SKYJO_OPT_OVERLAP); the games
 * concerned show SKYJO_ST_ERROR once (the stream the dealing kernel may still hold is left alone), results since then
 * are void, skyjo_vec_seed clears it (and skyjo_vec_snapshot_restore: a snapshot is only ever taken of a clean run).  A game
 * whose in-place deal or reset timed out shows done / SKYJO_ST_ERROR (not RESET; no reset is counted), its rewards are zero.
 * Synchronises `stream`.
 * Every synchronising call below (and the *_host conveniences, snapshot_create) makes the same check by itself. */
int skyjo_vec_check_error(skyjo_vec *h, void *stream);

/* synchronising host-side accessors */
int skyjo_vec_get_counters(skyjo_vec *h, skyjo_vec_counters *out_host, void *stream);
int skyjo_vec_reset_counters(skyjo_vec *h, void *stream);
int skyjo_vec_get_state(skyjo_vec *h, int32_t game, skyjo_game_state *out_host, void *stream);
int skyjo_vec_set_state(skyjo_vec *h, int32_t game, const skyjo_game_state *in_host, void *stream);
/* np.random.seed(value) on one game's legacy stream without dealing (fixture injection) */
int skyjo_vec_seed_raw(skyjo_vec *h, int32_t game, uint32_t value, void *stream);

/* The reference draws its deals and mid-game reshuffles from numpy's process-global legacy stream (skyjo.py:81,94,101,135),
 * the same one policy_ra(obs, mask) without a generator draws from (random_admissible_policy.py:22-23).  For a handle in
 * MT19937 mode with SKYJO_OPT_NO_BANK these two calls move that stream in and out of one game in numpy's own terms -
 * np.random.get_state(): key uint32[624], pos 0..624 - so a single-game view can hand the caller's stream to the device
 * before a deal or a reshuffle and hand it back afterwards (skyjo_rl_amd/game.py: SkyjoGame(global_rng=True)).
 * get_state returns the block completed the way numpy keeps it (the engine regenerates the state lazily).  Both synchronise.
 * (This is the reference's behaviour with numba's JIT DISABLED - the mode its seeded test pins.  Jitted, the reference's
 * np.random calls use numba's private generator and never touch the caller's global stream; a view in this mode re-seeds
 * and advances the caller's stream instead: skyjo_rl_amd/game.py, module docstring.) */
int skyjo_vec_rng_set_state(skyjo_vec *h, int32_t game, const uint32_t *key_host, int32_t pos, void *stream);
int skyjo_vec_rng_get_state(skyjo_vec *h, int32_t game, uint32_t *key_out_host, int32_t *pos_out_host, void *stream);

/* Kernel timing with HIP events on the launch stream: while enabled, every kernel of the path is launched with a
 * (start, stop) event pair that receives the kernel's own begin and end timestamps.  Returns and clears what was
 * collected since the last call - sum of milliseconds and launch count per kernel: [0] k_step, [1] k_scan, [2] k_deal,
 * [3] k_publish, [4] the policy / value net launches of skyjo_vec_model_rollout - then switches collection on (1) or off (0).
 * Synchronises the device. */
#define SKYJO_PROF_KERNELS 5
int skyjo_vec_profile(skyjo_vec *h, int enable, double ms_out[SKYJO_PROF_KERNELS], int64_t launches_out[SKYJO_PROF_KERNELS]);

/* Snapshot / restore of the WHOLE engine (the reference has no such feature): every live game, every bank
 * of pre-dealt episodes, every RNG stream with its position, statistics and the policy counter.  A snapshot lives in
 * device memory owned by the library; restoring it into the handle it was taken from makes every later call produce
 * exactly what it produced after the snapshot was taken.  Both calls drain the dealing pipeline and synchronise. */
typedef struct skyjo_vec_snapshot skyjo_vec_snapshot; /* opaque */
int skyjo_vec_snapshot_create(skyjo_vec *h, skyjo_vec_snapshot **out, void *stream);
int skyjo_vec_snapshot_restore(skyjo_vec *h, const skyjo_vec_snapshot *snap, void *stream);
int skyjo_vec_snapshot_bytes(const skyjo_vec_snapshot *snap, size_t *bytes_out);
int skyjo_vec_snapshot_destroy(skyjo_vec_snapshot *snap);

/* Diagnostic builds only (-DSK_STAMPS): per-section shader-cycle sums, 8 for the step kernel followed by 8 for
 * the dealing kernel, summed over wavefronts, cleared on read.  The shipped build returns zeros. */
int skyjo_vec_debug_stamps(skyjo_vec *h, uint64_t *out16_host);
/* Diagnostic builds (-DSK_TRACE) only: placement and time span of every wavefront of the last two step / dealing launches,
 * uint64 [4][tiles][8] (tools/dev/placement.py).  Zeros in the shipped build. */
int skyjo_vec_debug_trace(skyjo_vec *h, uint64_t *out_host);

/* Tunables.  SKYJO_OPT_DEAL_INTERVAL: lockstep iterations (steps or rollout iterations) between two runs of the
 * dealing kernel (1..1024).  Unless it is set, the engine starts at 88 (three
 * and more players) or 64 - 80 or 56 with the dealing kernel beside the step kernel - and adapts: every dealing run reports how many banks it found empty, any empty bank shortens
 * the interval, a long calm stretch lengthens it again - so it settles below the episode length of the policy in use.  Every game owns a bank of three
 * pre-dealt episodes and a dealing run adds at most one per game; a finished game whose bank is empty deals in
 * place (slow path, same result, counted in skyjo_vec_counters.waits). */
#define SKYJO_OPT_DEAL_INTERVAL 1
/* SKYJO_OPT_OVERLAP - where the dealing runs (results do not depend on it):
 *   0  in line on the caller's stream, after the step launch that makes it due;
 *   2  the two-stream form: the dealing kernel on a stream of its own beside the step kernels that follow (its episodes are
 *      published one dealing cycle later; the step kernel plans and publishes the runs itself, nothing on the caller's
 *      stream waits for the dealing stream).  Default, for batches that leave SIMDs idle (at most 768 tiles of 64 games), of
 *      the engines form 3 does not cover;
 *   3  the one-kernel form (k_cycle): every workgroup is one CU's worth of wavefronts, one step and one dealing wavefront per
 *      SIMD, the dealing wavefronts work for the games of their own workgroup - the hand-over never leaves the CU, so it needs
 *      no L2 write-back / invalidation.  Two to four players, either observation; S = 1 .. 4 step and as many dealing wavefronts
 *      per workgroup, whichever spreads the batch over the CUs and fits their LDS regions into 160 KB.  A launch may span up to
 *      16 dealing cycles.  The default wherever it exists, except where the LDS forces S below the batch's share of tiles per CU
 *      (a full chip of four-player games: form 0 there); the fused rollout only - other calls deal
 *      as in form 0;
 *   1  "beside the step kernel" in whichever of the two forms the engine prefers.
 * skyjo_vec_get_option returns 0, 2 or 3. */
#define SKYJO_OPT_OVERLAP 2
/* Fault injection for the tests (never needed in production): SKYJO_OPT_DEBUG_SPIN_LOG2 - a step kernel that has to wait
 * for an overlapped dealing kernel gives up after 2^value polls (default 22) and raises the sticky device error that
 * skyjo_vec_get_counters reports; SKYJO_OPT_DEBUG_DEAL_DELAY - every dealing wavefront sleeps value x 8128 cycles first. */
#define SKYJO_OPT_DEBUG_SPIN_LOG2 3
#define SKYJO_OPT_DEBUG_DEAL_DELAY 4
/* SKYJO_OPT_NO_BANK (set before skyjo_vec_seed): 1 = no episodes are dealt ahead - every reset deals in place from the
 * stream's current position, exactly when the reference would (skyjo.py:52-74).  Slow for batches; it is what lets ONE
 * game share the process-global numpy stream with its caller (skyjo_vec_rng_set_state / _get_state below). */
#define SKYJO_OPT_NO_BANK 5
/* SKYJO_OPT_RECORD_LAYOUT - how skyjo_vec_rollout lays out records_out (every other call writes row-major records unless ..._ALL below is chosen):
 *   SKYJO_REC_ROW_MAJOR    [iters][num_envs][record_bytes] - the default;
 *   SKYJO_REC_TILE_PLANAR  [iters][tiles][P][64][16], tiles = ceil(num_envs / 64), P = record_bytes / 16 (4 for the indirect
 *                          observation; 5 / 6 / 7 for the direct one with 2 / 3 / 4 players): the record of game 64 t + l is cut into
 *                          16-byte pieces, piece p at byte ((it * tiles + t) * P + p) * 1024 + l * 16.  A tile's records of one
 *                          iteration are still one contiguous block (P KiB), but every store instruction of the step wavefront now
 *                          writes 1 KiB of it straight from the registers the record was assembled in - no staging through LDS.
 *                          The buffer holds tiles * 64 records per iteration (the slots of a partial last tile beyond num_envs are
 *                          not written).  The one-kernel form (SKYJO_OPT_OVERLAP 3) only; skyjo_vec_unpack_tiles turns such blocks
 *                          into the reference's dense arrays. */
#define SKYJO_OPT_RECORD_LAYOUT 6
#define SKYJO_REC_ROW_MAJOR 0
#define SKYJO_REC_TILE_PLANAR 1
/* SKYJO_REC_TILE_PLANAR_ALL (round 6; indirect observation, two to four players): as SKYJO_REC_TILE_PLANAR, and every other device-style call
 * that writes records - skyjo_vec_reset, _observe, _step, _step_collect, _model_rollout (its records buffer is then
 * [T + 1][tiles][P][64][16]) - writes them tile-planar too, so that a rollout with the policy net never holds a row-major record
 * (the net, the masked draw and the episode-end columns read the blocks in place: skyjo_vec_*_layout).  The *_host calls stay row-major. */
#define SKYJO_REC_TILE_PLANAR_ALL 2
/* The older forms of a dealing run, kept for the engines the one-kernel form does not cover and selectable so that the parity tests
 * can hold them against the oracle (results never depend on them):
 *   SKYJO_OPT_INLINE_WORK_LIST 1: an in-line run uses the k_scan + work-list form (default 0: the dealing kernel scans the banks itself);
 *   SKYJO_OPT_UNPIPELINED      1: a run beside the step kernel uses the k_scan / k_publish form, whose caller's stream waits for every
 *                                 run (default 0: the step kernel plans and publishes the runs itself).
 * SKYJO_OPT_CYCLE_S (before skyjo_vec_seed): step - and dealing - wavefronts per workgroup of the one-kernel form, 1 .. 4; 0 = the
 * batch's share of tiles per compute unit (the default).  SKYJO_OPT_MAX_CYCLES_PER_LAUNCH: dealing cycles ONE launch of
 * skyjo_vec_rollout may span, 1 .. 16 (default 16).  The shipped library reads no environment variable; the measurement switches of
 * tools/dev/README.md exist in -DSK_DIAG builds only. */
#define SKYJO_OPT_INLINE_WORK_LIST 7
#define SKYJO_OPT_UNPIPELINED 8
#define SKYJO_OPT_CYCLE_S 9
#define SKYJO_OPT_MAX_CYCLES_PER_LAUNCH 10
int skyjo_vec_set_option(skyjo_vec *h, int option, int64_t value);
int skyjo_vec_get_option(const skyjo_vec *h, int option, int64_t *value_out);

/* Caller piece of config 5: the masking and sampling step of the action-mask policy model,
 * rlskyjo/models/action_mask_model.py:58-74 -  masked = logits + clamp(log(action_mask), min=FLOAT_MIN)  - followed
 * by RLlib's categorical draw from softmax(masked), fused into one pass over the records the engine has just
 * written (the mask bytes are read in place, offset mask_offset of each record).
 *   logits     float32 [n][26]  the policy net's outputs (device)
 *   records    [n][record_bytes] as written by step / reset / observe / rollout (device)
 *   seed, ticket   the uniform of game i is word 0 of Philox4x32-10(counter = (ticket, game_id0 + i, 0x53414D50),
 *              key = seed): the same (seed, ticket) reproduces the same draws; advance ticket once per step.
 *              Word by word, with gid = game_id0 + i as a 64-bit sum (it wraps) and M = 0xffffffff:
 *                counter = (ticket & M, ticket >> 32, gid & M, 0x53414D50 ^ (gid >> 32)),  key = (seed & M, seed >> 32);
 *              uniform = (float)(word 0 >> 8) * 2^-24, 24 bits in [0, 1).  tests/net_ref.py restates it, tests/test_net_ref.py
 *              holds the restatement to Random123's published vectors and tests/test_gpu_net_synthetic.py the kernel to it.
 *   no_masking != 0: the mask is ignored (action_mask_model.py:53-56,66-67)
 *   actions_out int32 [n]; logp_out float32 [n] (log-probability of the drawn action) or NULL;
 *   uniform_out float32 [n] (the uniforms in [0, 1), for tests) or NULL.
 * Arithmetic is float32: probabilities agree with torch.softmax to 1e-6 (tests/test_gpu_sampler.py).  The order of the sums is part
 * of the definition (csrc/skyjo_draw.h: exponentials in blocks of four actions, block totals left to right, the CDF of a block
 * starting from the total before it; the action is the smallest k of non-zero probability whose CDF value exceeds uniform * sum), so that the draw made in
 * the net's own launch (skyjo_vec_mlp_act_value: two lanes per game) and this one (one lane per game) give the same bits. */
int skyjo_vec_sample_actions(skyjo_vec *h, const void *records, const float *logits, int64_t n, uint64_t seed,
                             uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                             float *uniform_out, void *stream);

/* The policy net of config 5 on the matrix cores: RLlib's default fully connected net as the reference's
 * TorchActionMaskModel builds it (rlskyjo/models/action_mask_model.py:41-52: obs -> 256 tanh -> 256 tanh -> outputs),
 * evaluated for n records in one kernel that reads the int8 observation out of each record: 1 <= obs_dim <= 163, either
 * observation (31 features indirect, 19 + 12 N direct: 43 at two players, 67 at four, 163 at twelve).  Up to 31 inputs run in
 * k_net_bf16 / k_net_split, more in their wide forms (k_net_bf16_wide / k_net_split_wide: layer 1's weights read from memory, everything
 * behind it the same code), which read the first 16 * (obs_dim / 16 + 1) bytes of every record: record_bytes must hold them, as an
 * engine's records of that obs_dim do (SKYJO_E_INVALID otherwise, nothing launched).  Weights are given once in torch.nn.Linear layout (row-major [out][in], float32, HOST pointers) and
 * kept on the device as bf16 MFMA fragments (one per weight, or a high and a low one: see SKYJO_MLP_*); accumulation is
 * float32.  out: float32 [n][out_dim] (device), out_dim <= 32 (26 logits for the policy branch, 1 for the value branch).
 * tests/test_gpu_policy_net.py states the tolerance of either precision against the float32 torch module. */
typedef struct skyjo_vec_mlp skyjo_vec_mlp; /* opaque */
/* precision of a packed net.  SKYJO_MLP_FP32 is the drop-in for the reference's float32 TorchFC
 * (action_mask_model.py:43-49): every operand is the sum of two bf16 values and every product three MFMAs into a float32
 * accumulator, logits / values within 1e-4 of the float32 module (tests/test_gpu_policy_net.py).  SKYJO_MLP_BF16 keeps
 * weights and activations as single bf16 values: a third of the matrix work, logits within 8e-2. */
#define SKYJO_MLP_BF16 0
#define SKYJO_MLP_FP32 1
int skyjo_vec_mlp_create(int32_t device_id, int32_t obs_dim, int32_t out_dim, int32_t precision, const float *w1, const float *b1,
                         const float *w2, const float *b2, const float *w3, const float *b3, skyjo_vec_mlp **out);
int skyjo_vec_mlp_destroy(skyjo_vec_mlp *m);
int skyjo_vec_mlp_forward(const skyjo_vec_mlp *m, const void *records, int32_t record_bytes, int64_t n, float *out,
                          void *stream);
/* Policy branch (out_dim == 26) and the draw of skyjo_vec_sample_actions in ONE launch: the logits never leave the
 * registers (logits_out, float32 [n][26], may be NULL).  Same (seed, ticket) -> the same actions as
 * skyjo_vec_mlp_forward followed by skyjo_vec_sample_actions, bit for bit. */
int skyjo_vec_mlp_act(skyjo_vec *h, const skyjo_vec_mlp *m, const void *records, int64_t n, uint64_t seed, uint64_t ticket,
                      int32_t no_masking, int32_t *actions_out, float *logp_out, float *logits_out, void *stream);

/* Policy AND value branch of the action-mask model (two nets of skyjo_vec_mlp_create over the same records) in ONE
 * launch: the draw of skyjo_vec_mlp_act for the policy net, values_out float32 [n][value out_dim] for the other. */
int skyjo_vec_mlp_act_value(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, const void *records, int64_t n,
                            uint64_t seed, uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                            float *logits_out, float *values_out, void *stream);
/* Rollout collection: for the records a step has just written (device, [num_envs][record_bytes]) mark the games whose
 * episode ended in that step - episode_end_out uint8 [num_envs] - and copy their final rewards (skyjo_env.py:293-312)
 * into final_rewards_out double [num_envs][num_players], zeros elsewhere.  One small kernel, no host traffic. */
int skyjo_vec_episode_ends(skyjo_vec *h, const void *records, double *final_rewards_out, uint8_t *episode_end_out, void *stream);

/* The same consumers for records in an explicit layout (SKYJO_REC_ROW_MAJOR, or SKYJO_REC_TILE_PLANAR: what skyjo_vec_rollout writes with
 * SKYJO_OPT_RECORD_LAYOUT = tile-planar - piece p of game 64 t + l at block t * 64 * record_bytes + p * 1024 + l * 16 - is read in place,
 * no skyjo_vec_unpack_tiles pass; n counts games, the last tile's block is complete in memory whatever n).  Same results, bit for
 * bit, as the row-major calls on the same records (tests/test_gpu_record_layout.py).  value / values_out of ..._act_value_layout
 * may be NULL (then it is skyjo_vec_mlp_act). */
int skyjo_vec_mlp_forward_layout(const skyjo_vec_mlp *m, const void *records, int32_t record_bytes, int32_t layout, int64_t n, float *out,
                                 void *stream);
int skyjo_vec_mlp_act_value_layout(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, const void *records, int32_t layout,
                                   int64_t n, uint64_t seed, uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                                   float *logits_out, float *values_out, void *stream);
int skyjo_vec_sample_actions_layout(skyjo_vec *h, const void *records, int32_t layout, const float *logits, int64_t n, uint64_t seed,
                                    uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                                    float *uniform_out, void *stream);
int skyjo_vec_episode_ends_layout(skyjo_vec *h, const void *records, int32_t layout, double *final_rewards_out, uint8_t *episode_end_out,
                                  void *stream);

/* The learner's way back to the matrix cores, in place: an existing net's packed weights rewritten from DEVICE memory by one kernel
 * launch on `stream` - no allocation, no host copy, no synchronisation; the handle keeps its identity.
 *
 * The packed layout (one kernel writes it, for skyjo_vec_mlp_create - from its host arrays, staged on the device - and for the calls
 * below; fragment = 8 bf16 values = 16 bytes, value j of lane l, hh = l >> 5; S = 2 / ln 2
 * rounded to float32, bf16(x) = round to nearest even on the bit pattern, every product and difference one rounded float32 operation):
 *   w1  [8 u][KS s][64 l] fragments  bf16(S * W1[32 u + (l & 31)][k]), k = 16 s + 8 hh + j, over KS = max(2, obs_dim / 16 + 1) k-steps (integer
 *                                    division) = K = 16 KS columns: k in [obs_dim, K - 1) holds 0, k = K - 1 holds b1.  obs_dim <= 31: KS = 2, b1 in
 *                                    column 31; 47: K = 48, b1 in the last free column; 48: KS = 4; 163: KS = 11
 *   w2  [8 u][16 ks][64 l]           hi(S * W2[32 u + (l & 31)][acc_k]), acc_k = 32 (ks >> 1) + 16 (ks & 1) + 8 (j >> 2) + 4 hh + (j & 3)
 *   w3  [16 ks][64 l]                hi(W3[l & 31][acc_k]); the rows >= out_dim hold hi(0)
 *   b2  float32 [256]                S * b2[u];  bf16 mode: + sum over k = 0 .. 255, ascending, in double, of bf16(S * W2[u][k])
 *   b3  float32 [64 l][16 r]         b3[row], row = (r & 3) + 8 (r >> 2) + 4 hh; bf16 mode: + the same sum of bf16(W3[row][k]); rows >= out_dim 0
 *   w1l, w2l, w3l                    SKYJO_MLP_FP32 only, the layouts of w1, w2, w3: lo(v) = bf16(v - float(bf16(v))) of the same v
 * with hi(v) = bf16(v) for SKYJO_MLP_FP32 and bf16(-2 v) for SKYJO_MLP_BF16.  Only w1 / w1l depend on obs_dim; in a handle's blob every piece
 * starts on a 256-byte boundary, in this order.
 *
 * skyjo_vec_mlp_update: the six arrays are device float32 arrays in torch.nn.Linear layout - [256][obs_dim], [256], [256][256], [256],
 * [out_dim][256], [out_dim] - with obs_dim, out_dim and the precision the handle was created with; w2 and w3 16-byte aligned.
 * Afterwards the packed weights are the layout above of these values, for every finite input: what skyjo_vec_mlp_create gives for them.
 *
 * skyjo_vec_mlp_adam_step: the same kernel with torch.optim.Adam's rule (no amsgrad, no weight decay) in front of the pack.  Per
 * element, in float32:  m <- beta1 m + (1 - beta1) g;  v <- beta2 v + (1 - beta2) g^2;
 *                       p <- p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps),  t = step (counts from 1).
 * params[i] / grads[i]: w1, b1, w2, b2, w3, b3 as above (params are rewritten, grads are read only; w2, w3 and their gradients 16-byte
 * aligned).  The bias corrections are computed on the host, in double, from `step` and the float32 values of beta1 / beta2 as they
 * are passed; nothing is counted on the device and nothing is read back.  state: caller-owned, 16-byte aligned, at least
 * skyjo_vec_mlp_adam_state_bytes(m) bytes, zero-filled by the caller before step 1: float32 exp_avg of the six tensors back to
 * back in that order, padded with zeros to a multiple of 64 floats, then exp_avg_sq the same way.  An element with g == 0 and zero
 * state keeps its bits.  In bf16 mode the row sums of b2 / b3 are taken from the updated rows in the same launch.
 * SKYJO_E_INVALID (nothing is launched, the net is unchanged): a null pointer, a misaligned array, state_bytes too small, step < 1,
 * lr not finite, beta1 or beta2 outside [0, 1), eps negative or not finite.
 *
 * skyjo_vec_grad_norm: the global L2 norm of n device float32 arrays and the coefficient torch.nn.utils.clip_grad_norm_ scales by -
 * what RLlib's PPO clips a policy's gradients with (grad_clip) - in ONE launch of one workgroup of 1024 threads on `stream`, on the
 * current device; the job is a branch pair's twelve gradient tensors, at most about 164 k floats, and its cost is the launch (not
 * timed).  tensors[i] / counts[i], i < n, 1 <= n <= 32: read only, any 4-byte boundary, any count >= 0 (a pointer may be NULL where
 * its count is 0).  The sum of the squares of every element is taken in DOUBLE, each square and each addition, in an order that the
 * segment list alone fixes: thread t walks the segments in order and takes of each the element t of the head (the floats in front of
 * the first 16-byte boundary), the 16-byte groups t, t + 1024, ... in ascending address and the element t of the tail; a wavefront
 * adds its lanes x[l] + x[l ^ 32], then ^ 16 .. ^ 1, and the sixteen wavefronts are added in ascending order.  No atomics: the same
 * input gives the same bits on every call.  out2 (device, two floats):
 *   out2[0] = (float)sqrt(sum)
 *   out2[1] = the coefficient as torch forms it, in float32: c = (1 / (out2[0] + 1e-6f)) * max_norm - torch evaluates its
 *             `max_norm / (total_norm + 1e-6)` as reciprocal() * max_norm, two roundings - then c where c < 1, 1 where c >= 1 and c
 *             itself where it is NaN (torch.clamp(max=1) keeps a NaN).  max_norm = +INFINITY measures only: out2[1] = 1 whatever
 *             the norm.  A NaN element gives (NaN, NaN), an infinite one (+inf, 0).
 * SKYJO_E_INVALID (nothing is launched, out2 is untouched): a null argument, n outside 1 .. 32, a negative count, a NULL tensor with
 * a count > 0, a tensor or out2 that is not 4-byte aligned, max_norm NaN or <= 0.
 *
 * skyjo_vec_mlp_adam_step_clipped: skyjo_vec_mlp_adam_step - the same kernel, the same arguments and checks - with one change: every
 * thread reads *coef_device (device, one float32: out2 + 1 of a skyjo_vec_grad_norm queued before it on the same stream) and the rule
 * takes g * *coef_device, ONE rounded float32 multiply, wherever it reads g.  The gradients themselves are not rewritten.  With a
 * coefficient of exactly 1 the result carries the bits of skyjo_vec_mlp_adam_step; a NaN coefficient reaches every parameter, as
 * torch's does (no step is skipped: the host owns the step count).  SKYJO_E_INVALID besides the unclipped step's: coef_device NULL or
 * not 4-byte aligned.
 *
 * Ordering is the stream's: a net launch or rollout queued on the same stream afterwards sees the new weights.  A launch on ANOTHER
 * stream that still reads the net is the caller's race.
 *
 * skyjo_vec_mlp_export (for tests): the pieces copied back to back to dst_device (device, at least skyjo_vec_mlp_packed_bytes(m)
 * bytes), on `stream`, in the order w1, w2, w3, b2, b3, w1l, w2l, w3l (the *l pieces absent in bf16 mode) - without the padding that
 * separates them inside the handle, which is uninitialised. */
int skyjo_vec_mlp_update(skyjo_vec_mlp *m, const float *w1, const float *b1, const float *w2, const float *b2, const float *w3,
                         const float *b3, void *stream);
int64_t skyjo_vec_mlp_adam_state_bytes(const skyjo_vec_mlp *m); /* 0 for NULL */
int skyjo_vec_mlp_adam_step(skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                            float lr, float beta1, float beta2, float eps, int64_t step, void *stream);
int skyjo_vec_grad_norm(const float *const tensors[], const int64_t counts[], int32_t n, float max_norm, float *out2, void *stream);
int skyjo_vec_mlp_adam_step_clipped(skyjo_vec_mlp *m, float *const params[6], const float *const grads[6], void *state, int64_t state_bytes,
                                    float lr, float beta1, float beta2, float eps, int64_t step, const float *coef_device, void *stream);
int64_t skyjo_vec_mlp_packed_bytes(const skyjo_vec_mlp *m); /* 0 for NULL */
int skyjo_vec_mlp_export(const skyjo_vec_mlp *m, void *dst_device, int64_t bytes, void *stream);

/* skyjo_vec_step that also does what skyjo_vec_episode_ends does, inside the step kernel (no extra launch): the lane that
 * ends an episode writes episode_end_out[game] = 1 and the game's final rewards, every other game 0 / zeros. */
int skyjo_vec_step_collect(skyjo_vec *h, const int32_t *actions, void *records_out, double *final_rewards_out,
                           uint8_t *episode_end_out, void *stream);

/* Config 5's collection loop in ONE call (what rlskyjo/models/train_model_simple_rllib.py:22-59 has RLlib's
 * rollout workers do, per step: forward of the action-mask model, masked draw, env step, bookkeeping of episode ends): T
 * lockstep iterations of  [policy (+ value) net with the draw in its epilogue] -> [step kernel with the episode-end
 * columns] - two launches per iteration, nothing on the host in between.  All buffers are device memory of the caller:
 *   records        [T+1][num_envs][record_bytes]  IN: records[0] = what the first actor sees (skyjo_vec_observe / the last
 *                                                  records of the previous call); OUT: records[t+1] = after step t
 *   actions        int32 [T][num_envs]            the drawn actions
 *   logp           float32 [T][num_envs] or NULL  their log-probabilities
 *   values         float32 [T+1][num_envs][value out_dim]  (required iff `value` is given; [T] = bootstrap value)
 *   final_rewards  double [T][num_envs][num_players] and episode_end uint8 [T][num_envs]: both or neither
 * The draw of iteration t uses (seed, first_ticket + t) as in skyjo_vec_mlp_act: the same call sequence made one launch at a
 * time from the host gives the same bits.
 * Either observation: the policy net (26 outputs) must live on the engine's device and have the engine's obs_dim, the value net the
 * policy net's obs_dim, precision and device (SKYJO_E_INVALID otherwise).  The learner's native branches serve either observation as well:
 * skyjo_vec_mlp_train_* at 1 <= obs_dim <= 31, skyjo_vec_mlp_train_wide_* at 32 <= obs_dim <= 163, and skyjo_vec_ppo_update picks the
 * pair that fits the engine's observation. */
typedef struct skyjo_vec_rollout_buffers {
  void *records;
  int32_t *actions;
  float *logp;
  float *values;
  double *final_rewards;
  uint8_t *episode_end;
} skyjo_vec_rollout_buffers;
int skyjo_vec_model_rollout(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, int32_t T, uint64_t seed,
                            uint64_t first_ticket, int32_t no_masking, const skyjo_vec_rollout_buffers *buffers, void *stream);

/* Learner targets of a rollout buffer, on device: what RLlib's PPO attaches to the sample batches of the reference's trainer
 * (rlskyjo/models/train_model_simple_rllib.py:22-59) - `advantages` and `value_targets` by GAE(gamma, lambda) per agent trajectory -
 * computed for every row (t, game) of the columns skyjo_vec_model_rollout has written, one kernel, one lane per game walking
 * t = T - 1 .. 0 with per-seat carries (the seat that acts changes from row to row; DESIGN.md 4 has the recursion and its
 * operation order, which is part of the definition: float32, no fused multiply-add).
 *   records        [T+1] records in `layout` (SKYJO_REC_ROW_MAJOR: [T+1][num_envs][record_bytes]; SKYJO_REC_TILE_PLANAR:
 *                  [T+1][tiles][P][64][16], read in place); only the agent and done bytes are read
 *   values         float32 [T+1][num_envs][value_stride], component 0 is used; [T] bootstraps the seat records[T] expects
 *   final_rewards  double [T][num_envs][num_players], read only where episode_end uint8 [T][num_envs] is set
 *   gamma, lambda  in [0, 1]
 *   advantages_out, value_targets_out, returns_out  float32 [T][num_envs];  flags_out uint8 [T][num_envs], SKYJO_TGT_* bits
 * returns_out is the final reward of the acting seat's episode where that episode ended inside the buffer (0 elsewhere).  A row whose
 * record shows done (a re-deal / no-op, not a transition) gets zeros and no flag.  A seat's last action inside the buffer in an episode
 * that did not end there serves as the bootstrap of the seat's earlier actions and has no target itself - except for the seat
 * records[T] expects, whose bootstrap is values[T]. */
#define SKYJO_TGT_HAS_TARGET 1    /* advantages_out / value_targets_out are defined for the row */
#define SKYJO_TGT_EPISODE_KNOWN 2 /* the row is a transition of an episode that ended inside the buffer: returns_out is its seat's final reward */
int skyjo_vec_rollout_targets(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const float *values, int32_t value_stride,
                              const double *final_rewards, const uint8_t *episode_end, float gamma, float lambda,
                              float *advantages_out, float *value_targets_out, float *returns_out, uint8_t *flags_out, void *stream);

/* Learner minibatches of a rollout buffer, on device: which rows take part, and the rows of one minibatch as the dense tensors a
 * learner feeds its model - both read the buffer as it lies (DESIGN.md 4 has the definitions).
 *
 * skyjo_vec_rollout_select: the rows r of a flags column (in practice flags_out of skyjo_vec_rollout_targets seen as [T * num_envs]) with
 * (flags[r] & require_bits) == require_bits, in ascending order - a stable compaction, what torch.nonzero gives - and the moments of
 * their advantages.  Three launches (per-block counts, a scan of the block counts in one workgroup, the scatter), none waits for
 * another workgroup; the sums have a fixed reduction shape and use no atomics: the same input gives the same bits on every call.
 *   flags         uint8 [n_rows];  require_bits in 1 .. 255
 *   advantages    float32 [n_rows] or NULL
 *   index_out     int64 [n_rows]: the first *count_out entries are written
 *   count_out     int64 [1] (device): the number of selected rows; 0 is a valid result
 *   moments_out   double [2] (device; NULL iff advantages is NULL): the sum of a and the sum of a * a over the selected rows, every a
 *                 widened to double first; both 0.0 when no row is selected
 * n_rows == 0 writes count 0 and zero moments.  The block scratch belongs to the handle (allocated on first use, grown when needed). */
int skyjo_vec_rollout_select(skyjo_vec *h, const uint8_t *flags, int64_t n_rows, int32_t require_bits,
                             const float *advantages /* may be NULL */, int64_t *index_out /* [n_rows] */,
                             int64_t *count_out /* device, 1 */, double *moments_out /* device, 2; NULL iff advantages is NULL */,
                             void *stream);
/* skyjo_vec_rollout_select_seats: skyjo_vec_rollout_select over the n_rows = T * num_envs rows of a buffer, restricted to the rows in which
 * one of a set of seats acted - a row needs  (flags[r] & require_bits) == require_bits  AND bit agent(r) of seat_mask, agent(r) the agent
 * byte of the row's record, read in place from records[0 .. T) in `layout` (row r is game r % num_envs of step r / num_envs; the
 * padding slots of a tile-planar buffer are no rows).  The per-seat minibatches of a buffer in which every seat trains a policy of its
 * own (skyjo_vec_arena_collect): the moments are those of the chosen seats' rows alone.  The same three launches, the same reduction
 * shape, no atomics, the handle's scratch: the same input gives the same bits on every call, and with every seat in seat_mask index,
 * count and moments carry the bits of skyjo_vec_rollout_select.
 *   records    as for skyjo_vec_rollout_targets; only the agent byte is read;  T >= 1
 *   seat_mask  bit s = seat s takes part; non-zero, no bit at or above num_players
 *   flags, require_bits, advantages, index_out, count_out, moments_out: as for skyjo_vec_rollout_select
 * SKYJO_E_INVALID (nothing is launched): a null pointer, T < 1, require_bits outside 1 .. 255, a seat_mask of 0 or with a bit at or above
 * num_players, advantages without moments_out or the reverse, a layout that is neither SKYJO_REC_ROW_MAJOR nor SKYJO_REC_TILE_PLANAR. */
int skyjo_vec_rollout_select_seats(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const uint8_t *flags,
                                   int32_t require_bits, uint32_t seat_mask, const float *advantages /* may be NULL */,
                                   int64_t *index_out /* [T * num_envs] */, int64_t *count_out /* device, 1 */,
                                   double *moments_out /* device, 2; NULL iff advantages is NULL */, void *stream);
/* skyjo_vec_rollout_gather: the rows index[0 .. m) of the buffer - row ids r = t * num_envs + b, 0 <= r < T * num_envs, in any order,
 * repeats allowed (a learner passes a shuffled slice of the selection) - as dense [m]-major outputs, one kernel:
 *   records        the buffer's records in `layout` (as for skyjo_vec_rollout_targets; row r is record b of step t), 16-byte aligned
 *   actions int32, logp / advantages / value_targets float32 [T][num_envs];  values float32 [T (+ 1)][num_envs][value_stride]
 *   obs_out            float32 [m][obs_dim]  (float)(int8) of the record's observation bytes; 16-byte aligned
 *   logmask_out        float32 [m][26]       0.0f where the action-mask byte is non-zero, -FLT_MAX elsewhere: what
 *                                            clamp(log(action_mask), min=FLOAT_MIN) of action_mask_model.py:70 yields; 16-byte aligned
 *   actions_out        int64 [m];  logp_out, values_out (component 0), value_targets_out float32 [m]: the columns' rows
 *   advantages_out     float32 [m]           (advantages[r] - adv_mean) / adv_std: two float32 operations, each rounded, IEEE
 *                                            division; (0, 1) returns the column unchanged
 *   seats_out          uint8 [m]             the seat that acted (the record's agent byte)
 * A row id outside [0, T * num_envs) reads nothing and gives an all-zero output row.  adv_mean must be finite, adv_std finite and
 * greater than 0.  m == 0 is no work. */
int skyjo_vec_rollout_gather(skyjo_vec *h, const void *records, int32_t layout, int32_t T, const int64_t *index, int64_t m,
                             const int32_t *actions, const float *logp, const float *values, int32_t value_stride,
                             const float *advantages, const float *value_targets, float adv_mean, float adv_std,
                             float *obs_out, float *logmask_out, int64_t *actions_out, float *logp_out, float *advantages_out,
                             float *value_targets_out, float *values_out, uint8_t *seats_out, void *stream);
/* skyjo_vec_rollout_gather_logits: the rows index[0 .. m) of a float32 [n_rows][26] column that lies beside the buffer - the behaviour
 * policy's logits, one row per row id r = t * num_envs + b (skyjo_vec_rollout_buffers has no such column, and skyjo_vec_rollout_gather no
 * such output) - as out float32 [m][26], 16-byte aligned, one kernel.  The contract of skyjo_vec_rollout_gather: any order, repeats
 * allowed, m == 0 is no work, a row id outside [0, n_rows) reads nothing and gives an all-zero row.  Needs no handle: it runs on the
 * current device, on `stream`.  SKYJO_E_INVALID (nothing is launched): a null pointer, a negative m or n_rows, an out that is not 16-byte
 * aligned, a column or an index that is not aligned to its element size. */
int skyjo_vec_rollout_gather_logits(const float *column /* [n_rows][26] */, int64_t n_rows, const int64_t *index, int64_t m,
                                    float *out /* [m][26], 16-byte aligned */, void *stream);

/* The PPO loss head of a learner minibatch, on device: everything between a model's two outputs and optimizer.step() - the masked
 * softmax of action_mask_model.py:58-74, the clipped surrogate, the value loss and the entropy of the PPO the reference trains with
 * (rlskyjo/models/train_model_simple_rllib.py:54-57; without the KL penalty of RLlib's default loss: skyjo_vec_ppo_loss_kl below) - in one kernel that reads every input once and writes the gradients with
 * respect to the logits and the value, plus a single-workgroup launch that finishes the statistics.  Needs no engine handle: it runs
 * on the current device, on `stream`.  All arrays are dense device arrays of m >= 1 rows:
 *   logits         float32 [m][26]  the policy branch's raw output; 16-byte aligned
 *   log_mask       float32 [m][26]  logmask_out of skyjo_vec_rollout_gather (0 or -FLT_MAX); 16-byte aligned
 *   value          float32 [m];  actions int64 [m], each in [0, 26) - a precondition: an action outside is read as action 0
 *   logp_old, advantages, value_targets, values_old  float32 [m]
 *   clip > 0 (finite);  vf_coef;  ent_coef;  vf_clip: <= 0, +inf or NaN mean "no value clipping"
 * Per row, in double from the float32 inputs (every output is rounded once; the device's float32 logf carries a mean signed error of
 * -7e-08 on 1 <= S <= 26 that does not average out over the rows' kl and entropy):  z = logits + log_mask;  M = max z;  e = exp(z - M);  S = sum e;  logp = z - M - log S;  p = e / S (a masked
 * action has p == 0 exactly);  lp = logp[action];  r = exp(lp - logp_old);  A = advantage;
 *   pl = -min(r A, clamp(r, 1 - clip, 1 + clip) A);   H = -sum over p > 0 of p logp;   kl = logp_old - lp;
 *   vl = (v - vt)^2, and with value clipping vl = max(vl, (vc - vt)^2), vc = v_old + clamp(v - v_old, -vf_clip, vf_clip);
 *   clipped = (A > 0 and r > 1 + clip) or (A < 0 and r < 1 - clip).
 * L = 1/m sum (pl + vf_coef vl - ent_coef H).  The outputs:
 *   grad_logits_out float32 [m][26] dL/dlogits = 1/m [ -g r (delta_ka - p_k) + ent_coef p_k (logp_k + H) ], g = 0 if clipped else A; the
 *                                   entropy term is exactly 0 where p_k == 0, so a masked k != action gets exactly 0.0; 16-byte aligned
 *   grad_value_out  float32 [m]     1/m vf_coef d, d = 2 (v - vt) - but 0 where the value clamp saturates and (vc - vt)^2 > (v - vt)^2
 *   stats_out       double [6]      loss, policy_loss, vf_loss, entropy, kl, clip_fraction: means over the m rows; every row's terms are
 *                                   doubles and summed in a fixed order without atomics - the same input gives the
 *                                   same bits on every call
 *   scratch         caller-owned, 8-byte aligned, at least skyjo_vec_ppo_loss_scratch_bytes(m) bytes (the per-workgroup partial sums)
 * These are the gradients torch's autograd gives for the same expression.  SKYJO_E_INVALID on a null pointer, m < 1, a clip that is
 * not finite and positive, a misaligned array or a scratch that is too small. */
int64_t skyjo_vec_ppo_loss_scratch_bytes(int64_t m); /* 0 for m < 1 */
int skyjo_vec_ppo_loss(const float *logits, const float *log_mask, const float *value, const int64_t *actions, const float *logp_old,
                       const float *advantages, const float *value_targets, const float *values_old, int64_t m, float clip,
                       float vf_coef, float ent_coef, float vf_clip, float *grad_logits_out, float *grad_value_out,
                       double *stats_out /* device, 6 */, void *scratch, int64_t scratch_bytes, void *stream);
/* skyjo_vec_ppo_loss_kl: the same head with the KL penalty of RLlib's default PPO loss, which the reference's script leaves switched on
 * (ppo.DEFAULT_CONFIG untouched: kl_coeff 0.2, kl_target 0.01) - the divergence of the new masked distribution from the BEHAVIOUR
 * policy's whole masked distribution, not the sampled estimate `kl` above.  ray is not installed where this library is developed: the
 * form of the term is restated from memory of RLlib 1.9's torch policy, not checked against it.  The arguments, the definitions and the
 * promises of skyjo_vec_ppo_loss, and:
 *   old_logits     float32 [m][26]  the behaviour policy's raw logits of the rows (skyjo_vec_rollout_gather_logits); 16-byte aligned
 *   kl_coeff       finite, >= 0
 * Per row, in double, beside the above:  zo = old_logits + log_mask;  Mo = max zo;  So = sum exp(zo - Mo);  logpo = zo - Mo - log So;
 * po = exp(zo - Mo) / So;
 *   akl = sum over k with po_k > 0 of po_k (logpo_k - logp_k)      KL(pi_old || pi_new); logp_k is finite wherever the action is legal,
 *                                                                  also where p_k underflowed to 0 (in double: a gap of 745)
 * L = 1/m sum (pl + vf_coef vl - ent_coef H + kl_coeff akl).  The outputs:
 *   grad_logits_out   as above, plus 1/m kl_coeff (p_k - po_k) - 0 at a masked k, where p_k == po_k == 0: the masked k != action still gets
 *                     exactly 0.0.  With kl_coeff == 0 nothing is added: the bits of skyjo_vec_ppo_loss
 *   grad_value_out    as above
 *   stats_out         double [7]: the six above - the loss with the new term; with kl_coeff == 0 the bits of skyjo_vec_ppo_loss - and
 *                     action_kl, the mean of akl, computed whatever kl_coeff is (a coefficient can adapt from 0)
 *   scratch           at least skyjo_vec_ppo_loss_kl_scratch_bytes(m) bytes
 * A row with one legal action has p = po = 1: akl == 0.0 and a KL gradient term of 0.0, both exactly.  The same input gives the same
 * bits on every call.  SKYJO_E_INVALID as for skyjo_vec_ppo_loss, and on a null or misaligned old_logits and a kl_coeff that is
 * negative or not finite. */
int64_t skyjo_vec_ppo_loss_kl_scratch_bytes(int64_t m); /* 0 for m < 1 */
int skyjo_vec_ppo_loss_kl(const float *logits, const float *log_mask, const float *old_logits, const float *value, const int64_t *actions,
                          const float *logp_old, const float *advantages, const float *value_targets, const float *values_old, int64_t m,
                          float clip, float vf_coef, float ent_coef, float vf_clip, float kl_coeff, float *grad_logits_out,
                          float *grad_value_out, double *stats_out /* device, 7 */, void *scratch, int64_t scratch_bytes, void *stream);

/* One branch of the model - Linear(obs_dim, 256) - tanh - Linear(256, 256) - tanh - Linear(256, out_dim), 1 <= obs_dim <= 31,
 * 1 <= out_dim <= 32 (a wider layer 1: skyjo_vec_mlp_train_wide_* below) - trained on its float32 master parameters, on device: the forward that keeps its
 * activations and the backward that reads them, what torch's autograd otherwise does between a minibatch and the loss head and between
 * the loss head and the optimizer.  Needs no handle: the calls run on the current device, on `stream`.  Every product runs on the exact
 * float32 matrix instruction (float32 in, float32 accumulate: an fmaf chain), not on the packed nets' bf16 pairs; tanh is tanhf.
 *   params[i] / grads[i]  w1, b1, w2, b2, w3, b3 in torch.nn.Linear layout - [256][obs_dim], [256], [256][256], [256], [out_dim][256],
 *                         [out_dim] - the order of skyjo_vec_mlp_adam_step; w2 and w3 16-byte aligned.  grads are OVERWRITTEN
 *   x                     float32 [m][obs_dim], dense (obs_out of skyjo_vec_rollout_gather);  m >= 1
 *   out / grad_out        float32 [m][out_dim]: the branch's output, and the gradient of the loss with respect to it
 *   workspace             caller-owned, 16-byte aligned, at least skyjo_vec_mlp_train_workspace_bytes(obs_dim, out_dim, m) bytes.  Floats:
 *                         h1 [m][256], h2 [m][256], dz2 [m][256], dz1 [m][256], then one record of 82 208 per chunk of 256 rows
 *                         (ceil(m / 256) chunks): dW2 [256][256], dW1 [256][32] (column k >= obs_dim unused but 31, which is db1),
 *                         dW3 [32][256] (rows >= out_dim unused), db2 [256], db3 [32]
 * skyjo_vec_mlp_train_forward:  h1 = tanh(x W1^T + b1), h2 = tanh(h1 W2^T + b2), out = h2 W3^T + b3, one kernel, 64 rows per workgroup;
 * h1 and h2 - the values the next layer consumed - stay in the workspace.  A sum over k runs in one float32 chain: layer 1 over
 * x padded to 32 columns with a 1 in column 31 against b1 (so b1 is the chain's term k = 31), layers 2 and 3 from 0 with the bias added
 * to the finished sum; within every group of 8 consecutive k the order is k0, k0 + 4, k0 + 1, k0 + 5, k0 + 2, k0 + 6, k0 + 3, k0 + 7.
 * skyjo_vec_mlp_train_backward: reads the activations which the FORWARD OF THE SAME (params, x, m) LEFT IN THE SAME WORKSPACE - nothing
 * is recomputed and nothing checks it - and runs three kernels.  Rows: dz2 = (g W3) (1 - h2 h2), dz1 = (dz2 W2) (1 - h1 h1), chains
 * over k as above (over out_dim: ascending).  Weights: dW3 = g^T h2, dW2 = dz2^T h1, dW1 = dz1^T x and the column sums db3, db2, db1 of
 * g, dz2, dz1, per chunk of 256 rows: one chain over the chunk's rows, ascending, for a weight (db1 as the column of ones in the padded
 * x), runs of 64 (db2) or 32 (db3) rows added in order for the other biases.  Finish: an element's chunk partials are added in double,
 * chunk 0 first, and rounded to float32 once.  No chain over rows is longer than 256, no atomics: the same input gives the same bits
 * on every call.  Rows beyond m of the last tile and chunk enter as zeros and are never read or written.
 * SKYJO_E_INVALID (nothing is launched): a null pointer (an element of params or grads included), m < 1, obs_dim or out_dim out of
 * range, a workspace that is too small, w2 / w3 / workspace not 16-byte aligned. */
int64_t skyjo_vec_mlp_train_workspace_bytes(int32_t obs_dim, int32_t out_dim, int64_t m); /* 0 for invalid arguments */
int skyjo_vec_mlp_train_forward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m,
                                float *out /* [m][out_dim] */, void *workspace, int64_t workspace_bytes, void *stream);
int skyjo_vec_mlp_train_backward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x,
                                 const float *grad_out /* [m][out_dim] */, int64_t m, float *const grads[6] /* overwritten */,
                                 void *workspace, int64_t workspace_bytes, void *stream);

/* The same pair for a branch whose layer 1 is wider: 32 <= obs_dim <= 163 (the direct observation's 19 + 12 num_players features),
 * 1 <= out_dim <= 32, 1 <= m <= 2^30.  Every width has exactly one implementation: these entries refuse obs_dim <= 31 and >= 164 with
 * SKYJO_E_INVALID (skyjo_vec_mlp_train_wide_workspace_bytes returns 0), as the pair above refuses obs_dim >= 32.  Parameters,
 * arguments, validation and everything that is not layer 1 - layers 2 and 3, the row pass of the backward, dW2, dW3, db2, db3, the
 * finish - are as above, word for word.  What depends on obs_dim:
 *   the padded width   K = 8 (obs_dim / 8 + 1), integer division: a multiple of the k-group of 8 with at least one free column
 *                      (32 -> 40, 39 -> 40, 40 -> 48, 43 -> 48, 67 -> 72, 163 -> 168; obs_dim = 31 would give the 32 above).  x is
 *                      padded with zeros in columns [obs_dim, K - 1) and a 1 in column K - 1, against b1 in W1's column K - 1
 *   layer 1            one float32 chain over the K padded columns, groups of 8 ascending, within a group k0, k0 + 4, k0 + 1, k0 + 5,
 *                      k0 + 2, k0 + 6, k0 + 3, k0 + 7: b1 is the chain's LAST term, k = K - 1
 *   dW1, db1           dW1[j][k] = sum over the rows of dz1[r][j] xpad[r][k] for all K columns, one chain per chunk of 256 rows,
 *                      rows ascending; column K - 1 of that is db1
 *   workspace          h1, h2, dz2, dz1 [m][256] each, then one record of 74 016 + 256 K floats per chunk of 256 rows: dW2 [256][256],
 *                      dW1 [256][K] (columns [obs_dim, K - 1) unused), dW3 [32][256] (rows >= out_dim unused), db2 [256], db3 [32] -
 *                      4 (4 m 256 + ceil(m / 256) (74 016 + 256 K)) bytes.  At K = 32 the record would be the 82 208 above
 * The error texts carry these functions' names. */
int64_t skyjo_vec_mlp_train_wide_workspace_bytes(int32_t obs_dim, int32_t out_dim, int64_t m); /* 0 for invalid arguments */
int skyjo_vec_mlp_train_wide_forward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x, int64_t m,
                                     float *out /* [m][out_dim] */, void *workspace, int64_t workspace_bytes, void *stream);
int skyjo_vec_mlp_train_wide_backward(int32_t obs_dim, int32_t out_dim, const float *const params[6], const float *x,
                                      const float *grad_out /* [m][out_dim] */, int64_t m, float *const grads[6] /* overwritten */,
                                      void *workspace, int64_t workspace_bytes, void *stream);

/* An epoch's shuffled order of a selection, on device, without a sort: order_out[j] = index[perm(j)], 0 <= j < count, perm a keyed
 * bijection of [0, count) that is a pure function of (count, seed, epoch, j) - one lane per j, no atomics, no cross-lane traffic.  Needs
 * no handle: it runs on the current device, on `stream`.  1 <= count <= 2^30; count == 0 is no work (fault_out is still written);
 * order_out must not alias index.  index holds row ids, which are not negative.  All arithmetic is uint32 with wrap-around:
 *   fmix32(v):  v ^= v >> 16;  v *= 0x85EBCA6B;  v ^= v >> 13;  v *= 0xC2B2AE35;  v ^= v >> 16
 *   key[r] = fmix32(seed_lo ^ fmix32(seed_hi ^ fmix32(epoch * 0x9E3779B9 + r))), r = 0 .. 5 (the halves of seed; computed on the host
 *            and passed to the kernel by value)
 *   b = the smallest even number >= 2 with 2^b >= count;  h = b / 2;  mask = 2^h - 1
 *   E(x):  L = x >> h, R = x & mask;  six times, r = 0 .. 5:  (L, R) = (R, L ^ (fmix32(R + key[r]) & mask));  the result is (L << h) | R
 *   perm(j) = the first of E(j), E(E(j)), ... that is below count (cycle walking; the domain 2^b is smaller than 4 count)
 * The walk is capped at 1 024 applications of E.  A lane that hits the cap writes -1 to its order_out[j] - skyjo_vec_rollout_gather gives
 * such a row zeros - and fault_out (device, one int64, written by EVERY call) receives the number of such lanes from a single-workgroup
 * pass over order_out: 0 on success.  The longest walk tests/epoch_order_ref.py meets is 48: a non-zero count is a bug, not bad luck.
 * SKYJO_E_INVALID (nothing is launched): a null pointer, count < 0 or > 2^30, a pointer that is not 8-byte aligned, order_out
 * overlapping index. */
int skyjo_vec_rollout_shuffle(const int64_t *index, int64_t count, uint64_t seed, uint32_t epoch, int64_t *order_out /* [count] */,
                              int64_t *fault_out /* device, 1 */, void *stream);

/* A whole PPO update behind one call: `epochs` passes over the selected rows of a rollout buffer in shuffled slices of `minibatch` rows
 * (the last slice of an epoch may be short), every slice one learner step - exactly the launches the calls above make when a host loop
 * issues them one by one, in the same order, with the same arguments, on the one stream:
 *   1. skyjo_vec_rollout_gather of the slice (and skyjo_vec_rollout_gather_logits of `behaviour` with the KL term)
 *   2. skyjo_vec_mlp_train_forward of the policy branch, then of the value branch (here and in 4: skyjo_vec_mlp_train_wide_* on an
 *      engine whose observation has 32 .. 163 features)
 *   3. skyjo_vec_ppo_loss (skyjo_vec_ppo_loss_kl with the KL term)
 *   4. skyjo_vec_mlp_train_backward of the policy branch, then of the value branch
 *   5. skyjo_vec_grad_norm over the twelve gradients - the policy branch's six, then the value branch's - if clipping
 *   6. skyjo_vec_mlp_adam_step (_clipped if clipping) of the policy net, then of the value net, with step first_step + k, k counting
 *      the call's steps from 0 across the epochs
 *   7. one wavefront that adds the step to the epoch's statistics
 * so the parameters, the Adam states and both packed nets end with the bits of that host loop.  Epoch e takes orders[e] where orders is
 * given, and otherwise shuffles index with skyjo_vec_rollout_shuffle(seed, e) into the workspace.  The call allocates nothing, copies
 * nothing to the host, does not synchronise and has no host control flow that depends on device data; EVERY check of every stage runs
 * before the first launch - an update runs whole or not at all.  count == 0 launches the zeroing of epoch_stats_out and fault_out alone.
 *
 * skyjo_vec_ppo_update_args (the caller fills every field; pointers are device memory unless noted):
 *   records, layout, T, actions, logp, values, value_stride, advantages, value_targets   the buffer, as for skyjo_vec_rollout_gather
 *   behaviour      float32 [T * num_envs][26] or NULL: NULL - no KL term; otherwise skyjo_vec_ppo_loss_kl with kl_coeff
 *   index, count   the selection (skyjo_vec_rollout_select): count <= T * num_envs, count <= 2^30; index may be NULL with orders
 *   adv_mean, adv_std   host scalars, as skyjo_vec_rollout_gather takes them: finite, adv_std > 0
 *   epochs >= 1, minibatch >= 1, seed;  orders: NULL or int64 [epochs][count], used instead of the shuffle
 *   clip, vf_coef, ent_coef, vf_clip, kl_coeff   the head's, with the ranges of skyjo_vec_ppo_loss / _kl
 *   policy_net, value_net   the packed nets (26 outputs and 1, the engine's observation, the engine's device);  policy_params /
 *                  value_params: their six float32 master tensors, host arrays of device pointers as for skyjo_vec_mlp_adam_step;
 *                  policy_state / value_state with their byte counts: the Adam states
 *   lr, beta1, beta2, eps   as for skyjo_vec_mlp_adam_step;  first_step >= 1: the step number of the call's first step
 *   max_grad_norm  <= 0 or NaN: no clipping (stage 5 is not launched);  +inf: measure only;  otherwise as for skyjo_vec_grad_norm
 * workspace: caller-owned, 16-byte aligned, at least skyjo_vec_ppo_update_workspace_bytes(h, count, minibatch, with_kl) bytes (a size that
 * grows with count: one allocation for the largest count serves every smaller one).  It holds the minibatch columns, both branches'
 * training workspaces and outputs, the head's gradients, statistics and scratch, the twelve gradients (each 16-byte aligned), the
 * (norm, coefficient) pair, the order, the accumulators and the shuffle's fault word; nothing in it is an input.
 * epoch_stats_out: double [epochs][SKYJO_UPDATE_STATS], one row per epoch, written after the epoch's last step:
 *   [0 .. 5]  loss, policy_loss, vf_loss, entropy, kl, clip_fraction: sum over the steps of (the head's statistic * m) / max(seen, 1),
 *             m the step's rows and seen their sum - a double product and a double add per step
 *   [6]       action_kl, likewise; 0.0 without the KL term
 *   [7]       the mean over the epoch's steps of the norm before clipping, (double)norm added per step; 0.0 without clipping
 *   [8]       the share of steps whose coefficient was below 1, (double)(coef < 1.0f) added per step; 0.0 without clipping
 *   [9]       seen
 * Both quotients are formed as x * (1.0 / n), the reciprocal a host double - as torch divides a device tensor by a host scalar.
 * fault_out (device, one int64): the sum of the epochs' skyjo_vec_rollout_shuffle fault counts; 0 with orders.
 * SKYJO_E_INVALID (nothing is launched): what any stage refuses for these arguments - null pointers, alignments, state and workspace
 * sizes, the hyper-parameter ranges - and epochs, minibatch or first_step < 1, count outside 0 .. min(2^30, T * num_envs), a net on
 * another device, with another observation size or the wrong number of outputs. */
#define SKYJO_UPDATE_STATS 10
typedef struct skyjo_vec_ppo_update_args {
  const void *records;
  const int32_t *actions;
  const float *logp;
  const float *values;
  const float *advantages;
  const float *value_targets;
  const float *behaviour; /* may be NULL */
  const int64_t *index;
  const int64_t *orders; /* may be NULL */
  skyjo_vec_mlp *policy_net;
  skyjo_vec_mlp *value_net;
  float *policy_params[6];
  float *value_params[6];
  void *policy_state;
  void *value_state;
  int64_t policy_state_bytes;
  int64_t value_state_bytes;
  int64_t count;
  int64_t minibatch;
  int64_t first_step;
  uint64_t seed;
  int32_t layout;
  int32_t T;
  int32_t value_stride;
  int32_t epochs;
  float adv_mean, adv_std;
  float clip, vf_coef, ent_coef, vf_clip, kl_coeff;
  float lr, beta1, beta2, eps, max_grad_norm;
} skyjo_vec_ppo_update_args;
int64_t skyjo_vec_ppo_update_workspace_bytes(const skyjo_vec *h, int64_t count, int64_t minibatch, int32_t with_kl); /* 0 for invalid arguments */
int skyjo_vec_ppo_update(skyjo_vec *h, const skyjo_vec_ppo_update_args *a, void *workspace, int64_t workspace_bytes,
                         double *epoch_stats_out /* device, [epochs][SKYJO_UPDATE_STATS] */, int64_t *fault_out /* device, 1 */, void *stream);

/* Arena rollouts: the evaluation path beside skyjo_vec_model_rollout.  Every SEAT has a policy of its own - what the reference's script
 * does when it trains one policy per seat (rlskyjo/models/train_model_simple_rllib.py:43-49) and afterwards plays them with
 * logits.argmax() (:123-130) - and a seat may play policy_ra instead (rlskyjo/models/random_admissible_policy.py:26-28).  In self-play
 * with one shared policy the seats' final rewards are relative to the table's mean (skyjo_env.py:293-312) and average to mean_reward
 * whatever the policy learns; a trained seat against random seats is what shows progress.
 *
 * seats: num_players entries, seat s = the policy of the player the record's agent byte calls s.  Seats that share a `net` pointer share
 * one forward.  skyjo_vec_arena_select, one lockstep iteration's actions: every distinct net gets ONE launch of the net kernel (no draw)
 * over all num_envs records into its slice of the workspace - as many full-batch net launches as there are distinct nets; games are not
 * compacted by seat - and ONE more kernel, one lane per game, takes the game's agent byte and mask out of the record (either layout),
 * the seat's kind and the seat's net's row, and writes actions_out[g]:
 *   SKYJO_SEAT_SAMPLE  the draw of skyjo_vec_sample_actions with (seed, ticket, game_id0 + g) on the seat's net's logits: the bits of
 *                      skyjo_vec_mlp_forward_layout + skyjo_vec_sample_actions_layout, hence of skyjo_vec_mlp_act
 *   SKYJO_SEAT_GREEDY  the smallest k that maximises m[k], m[k] = logits[k] + (legal ? 0 : FLOAT_MIN) in float32 - the m the draw forms;
 *                      no random number is used
 *   SKYJO_SEAT_RANDOM  SKYJO_SEAT_SAMPLE on 26 zero logits: uniform over the legal actions; `net` must be NULL
 * The action is defined for every game; a game whose record already shows `done` has it ignored by the step, as in the training rollout.
 *   workspace  device memory of the caller, 16-byte aligned, at least skyjo_vec_arena_workspace_bytes(h, number of distinct nets) bytes:
 *              per distinct net float32 [num_envs][26], rounded up to a multiple of 16 bytes.  With no net at all (every seat
 *              SKYJO_SEAT_RANDOM) it may be NULL / 0.
 * skyjo_vec_arena_rollout: T lockstep iterations of  [the net forwards] -> [the select kernel] -> [skyjo_vec_step_collect]  on one
 * stream, nothing on the host in between, nothing read back.  buffers as for skyjo_vec_model_rollout - records[0] in, records[1 .. T],
 * actions, final_rewards and episode_end out, in the layout the engine's step writes (SKYJO_OPT_RECORD_LAYOUT) - but logp and values
 * must be NULL, and final_rewards / episode_end are required.  Iteration t draws with ticket first_ticket + t: with every seat
 * SKYJO_SEAT_SAMPLE on one net these are the bits of skyjo_vec_model_rollout.
 * (An engine that was never seeded is refused by the first skyjo_vec_step_collect with SKYJO_E_STATE; that iteration's actions are
 * computed by then, the engine is untouched.)
 * SKYJO_E_INVALID (nothing is launched): a null pointer, T < 1, an unknown kind, a net with SKYJO_SEAT_RANDOM or none without it, a net
 * whose out_dim is not 26, whose obs_dim is not the engine's or that lives on another device, a workspace that is too small or not
 * 16-byte aligned, logp or values set, a layout that is neither SKYJO_REC_ROW_MAJOR nor SKYJO_REC_TILE_PLANAR. */
#define SKYJO_SEAT_SAMPLE 0
#define SKYJO_SEAT_GREEDY 1
#define SKYJO_SEAT_RANDOM 2
typedef struct skyjo_vec_seat_policy {
  const skyjo_vec_mlp *net; /* NULL iff kind == SKYJO_SEAT_RANDOM */
  int32_t kind;             /* SKYJO_SEAT_* */
  int32_t reserved;
} skyjo_vec_seat_policy;
int64_t skyjo_vec_arena_workspace_bytes(const skyjo_vec *h, int32_t distinct_nets); /* 0 for NULL or distinct_nets outside 0 .. 12 */
int skyjo_vec_arena_select(skyjo_vec *h, const skyjo_vec_seat_policy *seats /* [num_players] */, const void *records, int32_t layout,
                           uint64_t seed, uint64_t ticket, int32_t *actions_out /* [num_envs] */, void *workspace,
                           int64_t workspace_bytes, void *stream);
int skyjo_vec_arena_rollout(skyjo_vec *h, const skyjo_vec_seat_policy *seats /* [num_players] */, int32_t T, uint64_t seed,
                            uint64_t first_ticket, const skyjo_vec_rollout_buffers *buffers /* logp and values must be NULL */,
                            void *workspace, int64_t workspace_bytes, void *stream);

/* Arena rollouts a learner can train on: one policy PER SEAT, as the reference's script trains them (train_model_simple_rllib.py:43-49:
 * a PPO policy per agent, policy_mapping_fn = agent id).  The iteration of skyjo_vec_arena_select, which also records, per game, the
 * log-probability of the chosen action and the value estimate of the ACTING seat's own value net - the two columns
 * skyjo_vec_rollout_targets, _select_seats, _gather and skyjo_vec_ppo_loss need to train seat s on the rows in which seat s acted.
 *   seats       as for skyjo_vec_arena_select
 *   value_nets  num_players entries, value_nets[s] = the value net of seat s or NULL; a net needs out_dim 1, the engine's observation
 *               and the engine's device.  Seats that share a pointer share one forward.
 * skyjo_vec_arena_act, one lockstep iteration: one full-batch launch of the net kernel per distinct policy net and one per distinct value
 * net into their slices of the workspace, then ONE kernel, one lane per game:
 *   actions_out[g]  exactly skyjo_vec_arena_select's action for the same (seats, records, seed, ticket)
 *   logp_out[g]     (m[a] - mx) - log(sum): a = the action, m = the masked logits, mx their maximum, sum the float32 sum of
 *                   exp(m - mx) in the draw's order (blocks of four actions, block totals left to right).  SKYJO_SEAT_SAMPLE: the bits
 *                   skyjo_vec_sample_actions and skyjo_vec_mlp_act write;  SKYJO_SEAT_GREEDY: the same expression at the argmax;
 *                   SKYJO_SEAT_RANDOM: the same expression on 26 zero logits, - log(number of legal actions)
 *   values_out[g]   output 0 of value_nets[seat] on record g - the bits skyjo_vec_mlp_forward_layout gives - or 0.0f where it is NULL
 * actions_out and logp_out are both set or both NULL.  Both NULL: values_out only, no policy net is launched - the bootstrap row of a
 * buffer, selected by the seat the record expects.  Launches per iteration: distinct policy nets + distinct value nets + 1 (+ the step).
 *   workspace   device memory of the caller, 16-byte aligned, at least skyjo_vec_arena_act_workspace_bytes(h, distinct policy nets,
 *               distinct value nets) bytes: the policy slices of skyjo_vec_arena_select first, then per distinct value net float32
 *               [num_envs], rounded up to a multiple of 16 bytes.  With no net at all it may be NULL / 0.
 * skyjo_vec_arena_collect: T iterations of  [the forwards] -> [that kernel] -> [skyjo_vec_step_collect], then the values-only pass on
 * records[T], on one stream, nothing read back.  buffers as for skyjo_vec_model_rollout, in the layout the engine's step writes
 * (SKYJO_OPT_RECORD_LAYOUT), EVERY column required; values is float32 [T+1][num_envs][1].  Iteration t draws with ticket
 * first_ticket + t: with every seat SKYJO_SEAT_SAMPLE on one policy net and every seat on one value net, all six columns carry the bits of
 * skyjo_vec_model_rollout.
 * SKYJO_E_INVALID (nothing is launched): what skyjo_vec_arena_select / _rollout refuse, and a null value_nets, values_out or column, only
 * one of actions_out / logp_out, a value net whose out_dim is not 1, whose obs_dim is not the engine's or that lives on another device. */
int64_t skyjo_vec_arena_act_workspace_bytes(const skyjo_vec *h, int32_t distinct_policy_nets,
                                            int32_t distinct_value_nets); /* 0 for NULL or a count outside 0 .. 12 */
int skyjo_vec_arena_act(skyjo_vec *h, const skyjo_vec_seat_policy *seats /* [num_players] */,
                        const skyjo_vec_mlp *const *value_nets /* [num_players], entries may be NULL */, const void *records, int32_t layout,
                        uint64_t seed, uint64_t ticket, int32_t *actions_out /* [num_envs] or NULL */, float *logp_out /* NULL iff actions_out is */,
                        float *values_out /* [num_envs] */, void *workspace, int64_t workspace_bytes, void *stream);
int skyjo_vec_arena_collect(skyjo_vec *h, const skyjo_vec_seat_policy *seats /* [num_players] */,
                            const skyjo_vec_mlp *const *value_nets /* [num_players], entries may be NULL */, int32_t T, uint64_t seed,
                            uint64_t first_ticket, const skyjo_vec_rollout_buffers *buffers /* every column required */, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* Per-seat results of the episodes that ended inside a buffer: over the rows = T * num_envs rows of its final_rewards (double
 * [rows][num_players]) and episode_end (uint8 [rows]) columns, one kernel plus a single-workgroup reduction, all in double, in a fixed
 * order, without atomics - the same input gives the same bits on every call.  Needs no handle: it runs on the current device, on `stream`.
 *   stats_out  double [1 + 3 num_players] (device): [0] the number of rows with episode_end != 0; then per seat s
 *              [1 + 3 s] the sum of the seat's final reward over those rows, [2 + 3 s] the sum of its squares (each square rounded
 *              once), [3 + 3 s] the number of those rows in which the seat's reward equals the row's maximum over the seats (a tie counts
 *              for every tied seat).  All 0 when no row ended an episode.  final_rewards is read only where episode_end is set.
 *   scratch    caller-owned, 8-byte aligned, at least skyjo_vec_episode_stats_scratch_bytes(rows, num_players) bytes
 * SKYJO_E_INVALID (nothing is launched): a null pointer, rows < 1, num_players outside 1 .. 12, a misaligned array, a scratch that is
 * too small. */
int64_t skyjo_vec_episode_stats_scratch_bytes(int64_t rows, int32_t num_players); /* 0 for invalid arguments */
int skyjo_vec_episode_stats(const double *final_rewards, const uint8_t *episode_end, int64_t rows, int32_t num_players,
                            double *stats_out /* device, 1 + 3 num_players */, void *scratch, int64_t scratch_bytes, void *stream);

/* host-pointer conveniences for small batches (single-game AEC view): synchronous.  Up to 4096 games they go through
 * host-mapped memory (one launch + one synchronisation per call, no copies), and step_host / reset_host bring every game's
 * state and rewards back with the records: skyjo_vec_get_state and skyjo_vec_get_rewards_host right after them cost no
 * device traffic. */
int skyjo_vec_step_host(skyjo_vec *h, const int32_t *actions_host, void *records_out_host);
int skyjo_vec_observe_host(skyjo_vec *h, const int32_t *players_host, void *records_out_host);
int skyjo_vec_reset_host(skyjo_vec *h, const uint8_t *mask_host, void *records_out_host);
int skyjo_vec_get_rewards_host(skyjo_vec *h, double *rewards_out_host, double *scores_out_host,
                               uint8_t *done_out_host);

/* The reference's two scoring helpers for CALLER-SUPPLIED hands (its notebook calls them directly; inside a game the step
 * kernel computes the same).  Host pointers, computed on device `device_id`, synchronous; float64 in numpy's operation order.
 *   skyjo_vec_evaluate_game       SkyjoGame._evaluate_game(players_cards, player_won_id, score_penalty)  (skyjo.py:477-498):
 *                             players_cards int8[n][num_players][12], player_won_id int32[n] -> scores double[n][num_players]
 *   skyjo_vec_calc_final_rewards  SimpleSkyjoEnv._calc_final_rewards(final_score, num_refunded)          (skyjo_env.py:293-312):
 *                             final_score double[n][num_players], num_refunded int32[n][num_players] -> rewards double[n][num_players] */
int skyjo_vec_evaluate_game(int32_t device_id, int32_t n, int32_t num_players, const int8_t *players_cards_host,
                        const int32_t *player_won_id_host, double score_penalty, double *scores_out_host);
int skyjo_vec_calc_final_rewards(int32_t device_id, int32_t n, int32_t num_players, const double *final_score_host,
                             const int32_t *num_refunded_host, double mean_reward, double reward_refunded,
                             double *rewards_out_host);

/* plain device-memory helpers so that a caller without torch can own buffers */
int skyjo_dev_malloc(int device_id, size_t bytes, void **out);
int skyjo_dev_free(void *p);
int skyjo_dev_copy(void *dst, const void *src, size_t bytes, int kind /*1 h2d, 2 d2h, 3 d2d*/, void *stream);
int skyjo_dev_sync(void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SKYJO_VEC_H */
