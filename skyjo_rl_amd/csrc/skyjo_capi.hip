// skyjo_capi.hip - host side of libskyjo_vec.so: the extern "C" boundary declared in
// include/skyjo_vec.h, handle / memory management and kernel launches.  gfx950 only, no CPU path.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "skyjo_device.h"
#include "skyjo_host.h"
#include "skyjo_deal_schedule.h"

// Measurement switches (environment variables: tools/dev/README.md) exist in -DSK_DIAG builds only; the shipped library reads no
// environment variable at all - what a caller or a test may choose is an option of skyjo_vec_set_option.
#ifdef SK_DIAG
static const char *sk_diag_env(const char *name) { return getenv(name); }
#else
static inline const char *sk_diag_env(const char *) { return nullptr; }
#endif

namespace {
thread_local std::string g_err;  // the library's one error message: the learner unit fails through fail() too (skyjo_host.h)
}
int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

namespace {

std::atomic<uint64_t> g_generation{0};

#define GUARD(h) DevGuard guard_((h)->cfg.device_id)

constexpr int kMaxCyclesPerLaunch = 16;  // k_cycle: whole dealing cycles per launch (each of deal_every_iters iterations)
constexpr size_t kCuLds = 160 * 1024;    // a compute unit's LDS: what a k_cycle workgroup may fill

// How the dealing runs of the fused rollout are made (SKYJO_OPT_OVERLAP reports 0 for the first two, 2 for the next two, 3 for the
// last).  resolve_form() chooses; results never depend on it.
enum class DealForm {
  InlineScan,             // k_deal on the caller's stream, lane = game, looks at the banks itself
  InlineWorkList,         // k_scan + k_deal on the caller's stream (SKYJO_OPT_INLINE_WORK_LIST)
  TwoStreamsPipelined,    // k_deal on deal_stream; the step kernel plans and publishes the runs (sk_plan_deals / sk_publish_deals)
  TwoStreamsScanPublish,  // k_deal on deal_stream between k_scan and k_publish on the caller's stream (SKYJO_OPT_UNPIPELINED)
  OneKernel               // k_cycle: step and dealing wavefronts in every workgroup, the pipelined protocol without a second stream
};
constexpr bool uses_deal_stream(DealForm f) { return f == DealForm::TwoStreamsPipelined || f == DealForm::TwoStreamsScanPublish; }

// What the caller asked for, as it asked (skyjo_vec_set_option); resolve_form() turns it into a DealForm.
struct DealRequests {
  int overlap = -1;  // SKYJO_OPT_OVERLAP 0 .. 3, -1: never set (the engine's own choice)
  bool unpipelined = false, inline_work_list = false;
  bool no_bank = false;  // SKYJO_OPT_NO_BANK: no pre-dealt episodes, every deal is made in place from the stream's position
  int cycle_s = 0;   // SKYJO_OPT_CYCLE_S (0: the batch's share)
};

// k_deal's third argument: where the run's games come from and who publishes its episodes
enum class DealRun : int {
  ListBeside = 0,  // the work list; k_publish follows
  ListInline = 1,  // the work list; k_deal publishes
  ScanInline = 2,  // lane = game, own scan; k_deal publishes
  Planned = 3      // lane = game, planned by the step kernel, which also publishes
};

// Default number of lockstep iterations between two dealing runs.  A run adds one episode to every bank that is not
// full, so the interval has to stay below the mean episode length of the policy in use (random admissible policy:
// 76 / 105 / 134 steps for 2 / 3 / 4 players) or the banks of SK_BANK episodes drain and finished games deal in
// place (deal_inline: slow, same result).  Measured at 65 536 three-player games (round 2 kernels): 80 -> 23.8, 88 -> 24.5,
// 92 -> 24.9, 96 -> 25.0 x 10^9 steps/s; over 2 x 10^8 episodes 88 and 92 never emptied a bank, 96 did 35 times in
// 1.2 x 10^8 episodes: 88 it is (0.84 of the mean episode length, like 64 for two players).
// With the dealing kernel on its own stream a run's episodes arrive one interval later, so the interval is a step
// shorter there (the runs are hidden behind the step kernel anyway): 64 / 48 with the k_scan + k_publish form, whose
// caller's stream waits for every run; 80 / 56 in the pipelined form (the default), where a step launch should outlast
// the dealing kernel beside it (32 768 x 3 players: 64 -> 17.5, 72 -> 19.0, 80 -> 19.4, 88 -> 19.9 x 10^9 steps/s with one
// bank run dry; 4 096 x 2 players: 48 -> 2.3, 56 -> 2.7, 64 -> 2.9 x 10^9 with twelve).
// The one-kernel form (k_cycle, cycle_s = its S): on a full chip (S = 4, a step and a dealing wavefront on every SIMD) a launch
// should last about as long as its dealing wavefronts - 65 536 x 3 players: 48 -> 32.7, 56 -> 36.0, 60 -> 37.1, 64 -> 37.3, 68 ->
// 36.8, 72 -> 36.5, 80 -> 35.7 x 10^9 steps/s; two players: 40 -> 28.3, 48 -> 30.3, 56 -> 31.3 (64 empties banks).  With S < 4 every
// wavefront has a SIMD to itself, the dealing is hidden anyway and longer launches win (32 768 x 3: 56 -> 22.4, 72 -> 23.2, 80 -> 23.4;
// 32 768 x 4: 64 -> 22.6, 80 -> 23.1, 96 -> 23.7, 112 -> 24.0; 4 096 x 2: 40 -> 2.44, 48 -> 2.88, 56 -> 2.98).
constexpr int deal_interval_default(int num_players, DealForm form, int cycle_s) {
  switch (form) {
    case DealForm::OneKernel:
      if (cycle_s >= 4) return num_players >= 3 ? 64 : 56;
      return num_players >= 4 ? 104 : (num_players == 3 ? 80 : 56);
    case DealForm::TwoStreamsPipelined: return num_players >= 3 ? 80 : 56;
    case DealForm::TwoStreamsScanPublish: return num_players >= 3 ? 64 : 48;
    default: return num_players >= 3 ? 88 : 64;
  }
}

}  // namespace

struct skyjo_vec {
  // ---- identity and what persists of the kernels' arguments (a launch sets its per-launch words on a copy of P) ----
  uint64_t generation = 0;  // unique per created handle in this process (snapshots remember it)
  skyjo_vec_config cfg{};
  SkParams P{};
  size_t G = 0;           // tiles * 64
  bool seeded = false;
  uint64_t iter = 0;        // rollout iterations (the policy's Philox counter)
  uint64_t iters_total = 0; // lockstep iterations of any kind since the counters were reset
  uint32_t *health_host = nullptr;  // host side of P.health_host
  int ncu = 256;            // compute units of the device (k_cycle's workgroup sizing)
  size_t lds_bytes = 0, lds_tile = 0;
  size_t lds_rollout = 0, lds_step = 0;  // the step kernels of 2 / 3 / 4 players keep their statistics in registers: smaller footprints (fused rollout / caller actions)
  // ---- the dealing form: requests -> resolve_form() -> form and, for k_cycle, its workgroup shape ----
  DealRequests req;
  DealForm form = DealForm::InlineScan;
  bool one_kernel_capable = false;  // two to four players and k_cycle may use a whole CU's LDS
  int cycle_s = SK_CYCLE_MAX_S;     // step (= dealing) wavefronts per workgroup of k_cycle
  size_t lds_cycle = 0, lds_cycle_step = 0;  // k_cycle's dynamic LDS and one step wavefront's region in it, for the record layout in force
  uint32_t cycle_deal_arg = 0;      // k_cycle's lds_deal_bytes argument: a dealing wavefront's region | the flag bits (skyjo_cycle.h)
  int max_cycles = 0;       // SKYJO_OPT_MAX_CYCLES_PER_LAUNCH (0: the ABI's maximum, kMaxCyclesPerLaunch)
  hipStream_t deal_stream = nullptr;  // k_deal's stream in the two-stream forms
  hipEvent_t ev_scan = nullptr, ev_dealt = nullptr;
  DealSchedule deal;  // the dealing schedule
  bool rec_planar_all = false;  // ... = SKYJO_REC_TILE_PLANAR_ALL: reset / observe / step / step_collect / model_rollout write their records tile-planar as well
  bool rec_planar = false;  // SKYJO_OPT_RECORD_LAYOUT: skyjo_vec_rollout writes its records tile-planar (one-kernel form, either observation)
  // ---- the host channel of the *_host conveniences (host_bufs) ----
  // Small batches (single-game views) go through host-mapped memory - the kernel reads the actions from it and writes the records
  // AND every game's packed state, rewards and scores to it (sk_export_raw), so a call is one launch + one stream synchronisation,
  // and skyjo_vec_get_state / get_rewards_host afterwards are served from `hm_raw` (raw_valid) without touching the device.
  bool fast_host = false, raw_valid = false;
  bool host_spin = true;    // single-tile engines: spin on the kernel's sign-off word (SKYJO_NO_SPIN=1 at create time: synchronise the stream)
  bool raw_export = false;  // the kernel also writes every game's packed state to host-mapped memory (few tiles only, see skyjo_vec_create)
  uint8_t *hm_block = nullptr;  // one hipHostMalloc: actions | mask | records | raw
  int32_t *hm_actions = nullptr;
  uint8_t *hm_mask = nullptr, *hm_records = nullptr, *hm_raw = nullptr;
  int32_t *hm_actions_d = nullptr;
  uint8_t *hm_mask_d = nullptr, *hm_records_d = nullptr, *hm_raw_d = nullptr;
  int raw_stride = 0;
  uint32_t host_seq = 0;  // sequence number of the last host-style step of a single-tile engine (see skyjo_vec_step_host)
  // larger batches are staged through device scratch, allocated when the first such call needs it
  int32_t *d_actions = nullptr;
  uint8_t *d_records = nullptr;
  uint8_t *d_mask = nullptr;
  // ---- skyjo_vec_rollout_select's scratch (sk_engine_select_scratch: allocated on first use, grown when a call needs more).  Not
  // part of a snapshot. ----
  void *sel_scratch = nullptr;
  size_t sel_blocks = 0;
  // ---- the arena allocator (dalloc) ----
  std::vector<std::pair<void *, size_t>> allocs;  // every device array of the handle with its size (snapshots copy them all)
  // The arrays made at create time are carved out of ONE allocation, the large ones at 2 MB boundaries: how the generator
  // states, the banks and the live tiles lie relative to each other in the memory channels is then the same in every
  // process.  (With one hipMalloc per array it was not: about one process in twenty - one in three when processes of
  // different shapes alternate - ran the dealing kernel at 90 instead of 70 us for its whole life.)
  std::vector<void *> owned;  // what hipFree gets
  uint8_t *arena = nullptr;
  size_t arena_off = 0;
  int arena_mode = 0;  // 1: adding up, 2: carving
  // ---- optional per-launch timing with HIP events on the launch stream (bench.py roofline leg) ----
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[SKYJO_PROF_KERNELS];  // k_step, k_scan, k_deal, k_publish, k_net_*
};

struct skyjo_vec_snapshot {
  const skyjo_vec *owner = nullptr;
  uint64_t owner_generation = 0;     // the handle's id (an address can be reused by a later handle)
  std::vector<size_t> array_bytes;   // size of every array in the blob, in the order of the handle's table
  int device_id = 0;
  void *blob = nullptr;
  size_t bytes = 0;
  // host side of the engine's state
  DealState deal;
  uint32_t health[2] = {0, 0};
  uint64_t iter = 0, iters_total = 0;
};

namespace {

// The sticky device error (skyjo_device.h: SK_ERR_*) as the host-style kernels (step with caller actions, reset, observe)
// left it in the host-mapped word: valid after any synchronisation with the stream they ran on.  The fused rollout kernel does
// not write that word: dev_error_fetch() reads the device's own copy first (get_counters, check_error, snapshot_create).
int dev_error_check(const skyjo_vec *h) {
  if (h->health_host && (h->health_host[2] & SK_ERR_DEAL_TIMEOUT))
    return fail(SKYJO_E_DEVICE, "a step kernel gave up waiting for the dealing kernel that should run beside it (SKYJO_OPT_OVERLAP): "
                                "results since then are void; switch the option off or re-seed");
  return SKYJO_OK;
}

int dev_error_fetch(skyjo_vec *h, hipStream_t s) {
  uint32_t err = 0;
  HIPCHK(hipMemcpyAsync(&err, h->P.dev_error, sizeof(err), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  h->health_host[2] |= err;
  return dev_error_check(h);
}

template <class T>
int dalloc(skyjo_vec *h, T **out, size_t count, bool zero = true) {
  const size_t bytes = count * sizeof(T);
  void *p = nullptr;
  if (h->arena_mode) {
    const size_t al = bytes >= ((size_t)1 << 20) ? ((size_t)2 << 20) : 256;
    const size_t off = (h->arena_off + al - 1) & ~(al - 1);
    h->arena_off = off + bytes;
    if (h->arena_mode == 1) {
      *out = nullptr;
      return SKYJO_OK;
    }
    p = h->arena + off;
  } else {
    HIPCHK(hipMalloc(&p, bytes));
    h->owned.push_back(p);
  }
  if (zero) HIPCHK(hipMemset(p, 0, bytes));
  h->allocs.emplace_back(p, bytes);
  *out = (T *)p;
  return SKYJO_OK;
}

// Profiling: the kernel's own begin / end timestamps (the dispatch packet's completion signal, the same
// source rocprofv3's kernel trace reads) are attached to a pair of events by hipExtLaunchKernelGGL.
int prof_events(skyjo_vec *h, int kernel, hipEvent_t *a, hipEvent_t *b) {
  *a = *b = nullptr;
  if (!h->profile) return SKYJO_OK;
  HIPCHK(hipEventCreate(a));
  HIPCHK(hipEventCreate(b));
  h->ev[kernel].emplace_back(*a, *b);
  return SKYJO_OK;
}

// ---- one table per kernel family: the instantiations that exist, and the only places that name them (the order of the rows is the
// order of the kernels in the code object, nothing else) ----
constexpr uint32_t kDealLds = SK_TILE * (SK_DECK_STRIDE + SK_STG_STRIDE);  // a dealing wavefront of two to four players: byte decks + MtChunkStream's staging rows
constexpr int fixed_players(int n) { return n >= 2 && n <= 4 ? n : 0; }    // the player counts with kernels of their own; 0: the generic ones

template <class Fn>
struct KernelRow {
  int key;  // kernel_key() of the template arguments
  Fn fn;
};
constexpr int kernel_key(int players, bool indirect = false, bool planar = false, bool policy = false) {
  return players | indirect << 4 | planar << 5 | policy << 6;
}
template <class Fn, size_t K>
Fn find_kernel(const KernelRow<Fn> (&table)[K], int key) {
  for (const KernelRow<Fn> &r : table)
    if (r.key == key) return r.fn;
  return nullptr;
}

constexpr KernelRow<decltype(&k_deal<2>)> kDealKernels[] = {{2, k_deal<2>}, {3, k_deal<3>}, {4, k_deal<4>}, {0, k_deal<0>}};

// PL: the records leave tile-planar (SKYJO_OPT_RECORD_LAYOUT)
#define SK_ROW(I, NP, PL) {kernel_key(NP, I, PL), k_cycle<I, NP, PL>}
#define SK_ROWS(I, PL) SK_ROW(I, 2, PL), SK_ROW(I, 3, PL), SK_ROW(I, 4, PL)
constexpr KernelRow<decltype(&k_cycle<true, 2, false>)> kCycleKernels[] = {SK_ROWS(true, false), SK_ROWS(true, true), SK_ROWS(false, true), SK_ROWS(false, false)};
#undef SK_ROWS
#undef SK_ROW

// PL: caller actions, indirect observation, two to four players only (SKYJO_REC_TILE_PLANAR_ALL checks that when it is set)
#define SK_ROW(I, Pol, NP, PL) {kernel_key(NP, I, PL, Pol), k_step<I, Pol, NP, PL>}
#define SK_ROWS(I, Pol) SK_ROW(I, Pol, 2, false), SK_ROW(I, Pol, 3, false), SK_ROW(I, Pol, 4, false), SK_ROW(I, Pol, 0, false)
constexpr KernelRow<decltype(&k_step<true, true, 2>)> kStepKernels[] = {SK_ROW(true, false, 2, true), SK_ROW(true, false, 3, true), SK_ROW(true, false, 4, true),
                                                                        SK_ROWS(true, true), SK_ROWS(true, false), SK_ROWS(false, true), SK_ROWS(false, false)};
#undef SK_ROWS
#undef SK_ROW

// ---- the dealing schedule: the only code that reads or writes h->deal and the kernels' per-launch dealing words.  What the entry
// points use: deals_drain, deals_refill, deals_plan_launch / deals_enter_launch (through launch_step) / deals_finish_launch, and
// the interval's accessors ----

// `tag`: the run's id; `be_read`: the bank_empty word the run reports (a run of the latest id: the word of its own parity, as the step
// kernel that planned it counted)
int launch_deal_kernel(skyjo_vec *h, hipStream_t ds, DealRun run, uint32_t tag, uint32_t be_read) {
  hipEvent_t e0, e1;
  int rc;
  SkParams P = h->P;
  P.deal_tag = tag, P.be_read = be_read;
  if ((rc = prof_events(h, 2, &e0, &e1))) return rc;
  const int np = fixed_players(P.L.N);
  // fixed player counts deal from a byte deck per lane; the generic kernel needs the tile + ring
  hipExtLaunchKernelGGL(find_kernel(kDealKernels, kernel_key(np)), dim3(P.tiles), dim3(SK_TILE), np ? kDealLds : (uint32_t)(h->lds_tile + 16384), ds, e0, e1, 0, P,
                        h->deal.st.list_sel, (int)run);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

// Planned -> Dealing without the k_cycle launch that should have carried the run (the caller went on with another kind of call):
// the dealing kernel alone, on the caller's stream.
int flush_planned(skyjo_vec *h, hipStream_t s) {
  DealSchedule &d = h->deal;
  if (d.inflight != InFlight::Planned) return SKYJO_OK;
  d.inflight = InFlight::Dealing;
  return launch_deal_kernel(h, s, DealRun::Planned, d.inflight_tag, (d.cycle_seq - 1u) & 1u);  // (the word the k_cycle launch that planned it counted into)
}

// Any state -> None: the episodes of the run in flight become available on stream `s`.
int deals_drain(skyjo_vec *h, hipStream_t s) {
  DealSchedule &d = h->deal;
  int rc = flush_planned(h, s);
  if (rc) return rc;
  if (d.inflight == InFlight::None) return SKYJO_OK;
  if (uses_deal_stream(h->form)) HIPCHK(hipStreamWaitEvent(s, h->ev_dealt, 0));
  hipEvent_t e0, e1;
  if ((rc = prof_events(h, 3, &e0, &e1))) return rc;
  if (d.inflight == InFlight::ListRun) {
    hipExtLaunchKernelGGL(k_publish, dim3(64), dim3(256), 0, s, e0, e1, 0, h->P, d.st.list_sel);
  } else {
    const int G = h->P.tiles * SK_TILE;
    hipExtLaunchKernelGGL(k_publish_all, dim3((G + 255) / 256), dim3(256), 0, s, e0, e1, 0, h->P);
  }
  HIPCHK(hipGetLastError());
  d.inflight = InFlight::None;
  return SKYJO_OK;
}

static void adapt_interval(skyjo_vec *h) {
  DealState &st = h->deal.st;
  const volatile uint32_t *hh = h->health_host;
  const uint32_t tag = hh[1], empty = hh[0];
  if (!st.auto_interval || tag == st.health_seen) return;
  st.health_seen = tag;  // the report of a run that has finished since the last look (one or two runs old)
  // An empty bank at scan time is a warning (one more game end before the next run deals in place), not yet a
  // stall: a handful of them is tolerated, one game in a thousand is not.
  const uint32_t many = (uint32_t)(h->P.B / 1024 > 1 ? h->P.B / 1024 : 1);
  if (empty >= many) {
    const int cut = st.deal_every_iters / 8 > 4 ? st.deal_every_iters / 8 : 4;
    st.deal_every_iters = st.deal_every_iters - cut > 8 ? st.deal_every_iters - cut : 8;
    st.calm_runs = 0;
  } else if (empty) {
    st.calm_runs = 0;
  } else if (++st.calm_runs >= 8 && st.deal_every_iters < h->deal.interval_default) {
    st.deal_every_iters += 2;
    st.calm_runs = 0;
  }
}
// the next run's id: it becomes the latest one, for the host and (P.deal_tag, which persists) for the kernels
static uint32_t next_deal_tag(skyjo_vec *h, bool flip_list) {
  DealState &st = h->deal.st;
  if (flip_list) st.list_sel ^= 1;  // (the work lists alternate: k_publish of one run clears the other's counter)
  st.deal_tag = (st.deal_tag + 1) & 0x7fffffffu;
  if (st.deal_tag == 0) st.deal_tag = 1;
  return h->P.deal_tag = st.deal_tag;
}

// One dealing run that the step kernel did not plan: publish the previous one, then deal one episode for every bank that is not
// full.  In line (-> None) k_deal publishes its own episodes; in the two-stream forms (-> ListRun) it runs on deal_stream beside the
// step launches that follow, and its episodes are published at the start of the next run, long before a bank of SK_BANK runs dry.
// The forms that do not plan make every run this way; seeding and resets fill the banks this way in every form (deals_refill).
int start_deals(skyjo_vec *h, hipStream_t s) {
  DealSchedule &d = h->deal;
  int rc;
  if (h->req.no_bank) {  // nothing is ever dealt ahead: a reset deals in place (deal_inline)
    d.st.pending_iters = 0;
    return SKYJO_OK;
  }
  if ((rc = deals_drain(h, s))) return rc;
  adapt_interval(h);
  next_deal_tag(h, true);
  // In line, the dealing kernel looks at the banks itself (lane = game) unless the work list was asked for: no k_scan launch.  Beside
  // the step kernel the list is made here, on the caller's stream, where it is ordered with the step launches around it (its counter
  // was cleared by the previous run's publish step).
  const bool beside = uses_deal_stream(h->form);
  const DealRun run = beside ? DealRun::ListBeside : h->req.inline_work_list ? DealRun::ListInline : DealRun::ScanInline;
  if (run != DealRun::ScanInline) {
    hipEvent_t e0, e1;
    if ((rc = prof_events(h, 1, &e0, &e1))) return rc;
    hipExtLaunchKernelGGL(k_scan, dim3((h->P.B + SK_SCAN_BLOCK - 1) / SK_SCAN_BLOCK), dim3(SK_SCAN_BLOCK), 0, s, e0, e1, 0, h->P,
                          d.st.list_sel);
    HIPCHK(hipGetLastError());
  }
  if (beside) {
    HIPCHK(hipEventRecord(h->ev_scan, s));
    HIPCHK(hipStreamWaitEvent(h->deal_stream, h->ev_scan, 0));
  }
  if ((rc = launch_deal_kernel(h, beside ? h->deal_stream : s, run, d.st.deal_tag, d.st.deal_tag & 1u))) return rc;
  if (beside) {
    HIPCHK(hipEventRecord(h->ev_dealt, h->deal_stream));
    d.inflight = InFlight::ListRun;
  }
  d.st.pending_iters = 0;
  return SKYJO_OK;
}
// One run that nobody planned, then published: what was taken from the banks (a reset, a new seed) is there again on stream `s`.
int deals_refill(skyjo_vec *h, hipStream_t s) {
  const int rc = start_deals(h, s);
  return rc ? rc : deals_drain(h, s);
}

// The pipelined protocol (skyjo_device.h, sk_plan_deals) of TwoStreamsPipelined and OneKernel: the step launch after which the run
// is due plans it on its way out (deals_plan_launch gives the run its id), start_deals_planned() follows the launch.  Nothing on the
// caller's stream waits.
bool plans_ahead(const skyjo_vec *h) {
  return (h->form == DealForm::TwoStreamsPipelined || h->form == DealForm::OneKernel) && !h->req.no_bank;
}
int start_deals_planned(skyjo_vec *h, hipStream_t s) {
  DealSchedule &d = h->deal;
  int rc;
  if (h->form == DealForm::OneKernel) {  // -> Planned: the next k_cycle launch carries the run; nothing is launched here
    if ((rc = flush_planned(h, s))) return rc;  // (an older run that no launch has carried yet: deal it now)
    d.inflight = InFlight::Planned, d.inflight_tag = d.st.deal_tag;
  } else {  // -> Dealing: the dealing kernel goes to its own stream behind an event for the launch that planned the run
    HIPCHK(hipEventRecord(h->ev_scan, s));
    HIPCHK(hipStreamWaitEvent(h->deal_stream, h->ev_scan, 0));
    if ((rc = launch_deal_kernel(h, h->deal_stream, DealRun::Planned, d.st.deal_tag, d.st.deal_tag & 1u))) return rc;
    HIPCHK(hipEventRecord(h->ev_dealt, h->deal_stream));
    d.inflight = InFlight::Dealing;
  }
  d.st.pending_iters = 0;
  adapt_interval(h);  // (for the cycles to come)
  return SKYJO_OK;
}

// Plan a launch: how many of the `wanted` iterations the next step launch takes (plan_launch) and, where the form plans
// ahead and a run is due after it, that run's id.  `fused`: a launch of the fused rollout - in the one-kernel form it keeps its
// tiles in LDS over several dealing cycles when the caller asks for that many iterations at once: up to kMaxCyclesPerLaunch whole
// cycles in ONE launch (the cycle ends inside it are handled by the kernel: step_body, k_cycle).
// (Only where the kernel's cycle ends have a run to hand over: an engine that never deals ahead - SKYJO_OPT_NO_BANK - plans nothing,
// and a cycle end inside its launch would publish and plan with a stale id: ADVICE r4)
StepLaunch deals_plan_launch(skyjo_vec *h, int wanted, bool fused) {
  const DealState &st = h->deal.st;
  const bool planned = plans_ahead(h);
  const int cap = h->max_cycles > 0 ? h->max_cycles : kMaxCyclesPerLaunch;
  StepLaunch L{plan_launch(wanted, st.pending_iters, st.deal_every_iters, fused && planned && h->form == DealForm::OneKernel, cap), 0};
  if (L.due && planned) {
    L.plan_tag = next_deal_tag(h, false);  // the id of the first run planned by this launch; the kernel counts on from it
    for (int c = 1; c < L.cycles; c++) next_deal_tag(h, false);
  }
  return L;
}
// The schedule's part in a step launch: the dealing words of `P`, the launch's copy of h->P.  A k_cycle launch (`cycle_kernel`)
// carries the planned run, *carried = its id (0: none), Planned -> Dealing; in front of any other step kernel that run is dealt
// now - it does not wait for a k_cycle launch.
int deals_enter_launch(skyjo_vec *h, hipStream_t s, const StepLaunch &L, bool cycle_kernel, SkParams &P, uint32_t *carried) {
  DealSchedule &d = h->deal;
  if (d.inflight == InFlight::Planned || d.inflight == InFlight::Dealing) P.ov_flags |= 1u;  // publish what has been dealt since (sk_publish_deals)
  if (L.plan_tag) P.ov_flags |= 2u, P.plan_new_tag = L.plan_tag, P.be_add = L.plan_tag & 1u;
  *carried = 0;
  if (!cycle_kernel) return flush_planned(h, s);
  if (d.inflight == InFlight::Planned) *carried = d.inflight_tag, d.inflight = InFlight::Dealing;
  P.be_add = d.cycle_seq & 1u, P.be_read = (d.cycle_seq & 1u) ^ 1u;  // (the launch's parity, not the run's)
  d.cycle_seq++;
  return SKYJO_OK;
}
// Finish a launch: its iterations count, and the run that fell due is started in the engine's form.
int deals_finish_launch(skyjo_vec *h, hipStream_t s, const StepLaunch &L) {
  h->deal.st.pending_iters += L.iters;
  if (!L.due) return SKYJO_OK;
  return plans_ahead(h) ? start_deals_planned(h, s) : start_deals(h, s);
}

// the interval: resolve_form's default for the form, an explicit value (SKYJO_OPT_DEAL_INTERVAL), the one in force
void deals_set_interval_default(skyjo_vec *h, int iters) {
  h->deal.interval_default = iters;
  if (h->deal.st.auto_interval) h->deal.st.deal_every_iters = iters;
}
void deals_set_interval(skyjo_vec *h, int iters) { h->deal.st.deal_every_iters = iters, h->deal.st.auto_interval = false; }
int deals_interval(const skyjo_vec *h) { return h->deal.st.deal_every_iters; }
// ---- end of the dealing schedule ----

// One step launch as deals_plan_launch sized it; deals_finish_launch follows it.  `host_seq`: see skyjo_vec_step_host.
int launch_step(skyjo_vec *h, hipStream_t s, const StepLaunch &L, bool policy, const int32_t *actions, uint8_t *rec, int32_t *act_out,
                uint64_t policy_seed, double *end_rew = nullptr, uint8_t *end_flag = nullptr, uint8_t *raw_out = nullptr,
                bool planar_out = false, uint32_t host_seq = 0) {
  h->raw_valid = false;  // (the host's copy of the games is stale from here on; step_host sets it again)
  SkParams P = h->P;     // the launch's own copy: the per-launch words are set here and nowhere put back
  P.host_seq = host_seq;
  const bool ind = P.L.indirect != 0;
  // one kernel for the whole dealing cycle: S step + S dealing wavefronts per workgroup (= per CU)
  const bool cycle_kernel = h->form == DealForm::OneKernel && policy && !end_rew && !raw_out;
  int rc;
  hipEvent_t e0, e1;
  uint32_t tag;
  if ((rc = prof_events(h, 0, &e0, &e1)) || (rc = deals_enter_launch(h, s, L, cycle_kernel, P, &tag))) return rc;
  if (cycle_kernel) {
    const int S = h->cycle_s;
    hipExtLaunchKernelGGL(find_kernel(kCycleKernels, kernel_key(P.L.N, ind, h->rec_planar)), dim3((P.tiles + S - 1) / S), dim3(2 * S * SK_TILE), (uint32_t)h->lds_cycle, s,
                          e0, e1, 0, P, rec, act_out, L.iters, policy_seed, h->iter, tag, (uint32_t)h->lds_cycle_step, h->cycle_deal_arg, L.cycles > 1 ? L.iters / L.cycles : 0);
  } else {
    hipExtLaunchKernelGGL(find_kernel(kStepKernels, kernel_key(fixed_players(P.L.N), ind, ind && !policy && planar_out, policy)), dim3(P.tiles), dim3(SK_TILE), (uint32_t)(policy ? h->lds_rollout : h->lds_step), s, e0, e1, 0, P, actions, rec, act_out,
                          L.iters, policy_seed, h->iter, end_rew, end_flag, raw_out, h->raw_stride);
  }
  HIPCHK(hipGetLastError());
  h->iters_total += (uint64_t)L.iters;
  if (policy) h->iter += (uint64_t)L.iters;  // the policy's Philox counter counts rollout iterations only
  return SKYJO_OK;
}

int fetch_record(skyjo_vec *h, const uint4 *base, int game, std::vector<uint8_t> &raw, hipStream_t s) {
  const SkLayout &L = h->P.L;
  raw.assign((size_t)L.state_bytes, 0);
  const uint8_t *src = (const uint8_t *)(base + ((size_t)(game / SK_TILE) * L.chunks) * SK_TILE + game % SK_TILE);
  HIPCHK(hipMemcpy2DAsync(raw.data(), 16, src, SK_TILE * 16, 16, L.chunks, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return SKYJO_OK;
}

// The only place that knows which engine runs which dealing form: requests (h->req), what the engine can do (two to four players,
// a CU's LDS, the batch's share of the chip) and the SK_DIAG switches -> h->form, k_cycle's workgroup shape and LDS, the default
// interval.  Called by skyjo_vec_create and, through change_form(), by every option that changes a request; SKYJO_OPT_RECORD_LAYOUT
// re-runs it for the LDS sizes alone.
void resolve_form(skyjo_vec *h) {
  const SkParams &P = h->P;
  const int N = P.L.N;
  const bool fixed_n = N >= 2 && N <= 4;
  // k_cycle: S step + S dealing wavefronts per workgroup, S = what spreads the batch over the CUs (1 .. 4) or SKYJO_OPT_CYCLE_S; their
  // LDS regions and the claim words must fit one CU (S = 1 always does: at most 32 + 15 KiB)
  int S = h->req.cycle_s ? h->req.cycle_s : (P.tiles + h->ncu - 1) / h->ncu;
  S = S < 1 ? 1 : (S > SK_CYCLE_MAX_S ? SK_CYCLE_MAX_S : S);
  const int natural_s = S;
  size_t region = h->lds_rollout;
  bool no_defer = false;
  if ((size_t)S * (h->lds_rollout + kDealLds) + 32 > kCuLds && (size_t)S * (h->lds_step + kDealLds) + 32 <= kCuLds && N <= 3 &&
      !sk_diag_env("SKYJO_CYCLE_DEFER_ONLY")) {
    // the direct observation of three players on a full chip: the CU's share of tiles fits without the card chunks of the deferred
    // scoring (the games are then scored in the iteration they end: a slower step, but one round of workgroups - 31.0 against 23.5
    // x 10^9 in line; four players, where scoring on the spot costs more: 22.5 against 30.1 - they stay in line)
    region = h->lds_step, no_defer = true;
  }
  while (S > 1 && (size_t)S * (region + kDealLds) + 32 > kCuLds) S--;  // (fewer wavefronts per workgroup, more workgroups)
  h->cycle_s = S;
  if (h->rec_planar && !P.L.indirect) {
    // the direct observation's wide records leave from registers in this layout: the staging area shrinks to the rare paths' 4 KiB of
    // scratch, and where the card chunks of the deferred scoring did not fit beside it (three players on a full chip) they do now
    const size_t base = h->lds_tile + 4096, with_defer = base + (size_t)N * 1024;
    no_defer = (size_t)S * (with_defer + kDealLds) + 32 > kCuLds;
    region = no_defer ? base : with_defer;
  }
  h->lds_cycle_step = region, h->lds_cycle = (size_t)S * (region + kDealLds) + 32;
  h->cycle_deal_arg = kDealLds | (no_defer ? 1u << 29 : 0u);
  if (const char *e = sk_diag_env("SKYJO_CYCLE_SPLIT")) h->cycle_deal_arg |= (uint32_t)(atoi(e) & 3) << 30;  // diagnostic: 1 = roles by SIMD parity, 2 = by SIMD pair
  h->one_kernel_capable = fixed_n && h->lds_cycle <= kCuLds && !sk_diag_env("SKYJO_LDS_PAD");
  // (the attribute belongs to the function, not to the handle: always the whole CU, so that engines of different batch sizes -
  // different S - can live side by side in one process)
  for (int planar = 0; planar < 2 && h->one_kernel_capable; planar++)
    if (hipFuncSetAttribute((const void *)find_kernel(kCycleKernels, kernel_key(N, P.L.indirect != 0, planar != 0)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCuLds) != hipSuccess) {
      (void)hipGetLastError();
      h->one_kernel_capable = false;
    }
  // The engine's own choice: the one-kernel form wherever it fits (measured at 4 096 .. 65 536 games and two to four players: + 9 .. 32 %
  // over the two-stream form, + 18 .. 57 % over dealing in line, EXPERIMENTS.md round 4).
  // (Batches beyond four tiles per CU run in two or more rounds of workgroups - a workgroup's LDS fills its CU: 98 304 x 3 29.1
  // against 23.8 in line, 131 072 x 3 34.0 against 21.0; counter-based deals 37.5 / 49.4 against 39.6 / 32.5: the one-kernel
  // form still wins everywhere but at one and a half rounds of counter-based deals.  Not so where the LDS - not the batch - makes
  // the workgroups smaller than a CU's share of the tiles, i.e. a full chip of four-player games or of the direct observation: S = 3,
  // 342 workgroups in one and a third rounds, 25.5 against 30.0 and 17.5 against 23.6 in line.)
  bool prefer_one = S == natural_s;
  if (const char *e = sk_diag_env("SKYJO_MERGED")) prefer_one = atoi(e) != 0;
  prefer_one = prefer_one && h->one_kernel_capable;
  // Otherwise the dealing kernel runs beside the step kernel (own stream) when the batch leaves SIMDs free: up to 768 tiles of
  // the 1024 one-wavefront-per-SIMD slots (three-player games, beside / in line, x 10^9 steps/s: 32 768: 17.1 / 15.5,
  // 49 152: 23.1 / 22.6, 57 344: 25.2 / 26.1, 65 536: 20.3 / 29.0 - on a full chip the two kernels compete for the same
  // vector ALUs), in line above that.
  bool one = false, beside = false;
  switch (h->req.overlap) {
    case 0: break;
    case 1: one = prefer_one, beside = !one; break;
    case 2: beside = true; break;
    case 3: one = h->one_kernel_capable; break;  // (the option refuses it where it is not)
    default: {
      const char *e = sk_diag_env("SKYJO_OVERLAP");
      one = prefer_one && !e;
      beside = !one && (e ? atoi(e) != 0 : P.tiles <= 768);
    }
  }
  h->form = one      ? DealForm::OneKernel
            : beside ? (h->req.unpipelined ? DealForm::TwoStreamsScanPublish : DealForm::TwoStreamsPipelined)
                     : (h->req.inline_work_list ? DealForm::InlineWorkList : DealForm::InlineScan);
  deals_set_interval_default(h, deal_interval_default(N, h->form, h->cycle_s));
}

// Every option that changes a request goes through here: nothing runs and nothing is in flight in the old form when the new one
// takes over (the caller's stream may be a non-blocking one, so the device is synchronised before the null stream publishes).
int change_form(skyjo_vec *h, const DealRequests &req) {
  HIPCHK(hipDeviceSynchronize());
  int rc = deals_drain(h, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  h->req = req;
  resolve_form(h);
  return SKYJO_OK;
}

}  // namespace

// ---- the engine as the learner unit sees it (skyjo_host.h) ----
SkEngineView sk_engine_view(const skyjo_vec *h) { return {h->cfg.device_id, h->P.B, h->G, h->P.game_id0, &h->P.L}; }

int sk_engine_select_scratch(skyjo_vec *h, size_t blocks, void **scratch_out, size_t *cap_out) {
  if (!h->sel_scratch || blocks > h->sel_blocks) {
    const size_t cap = blocks > 64 ? blocks : 64;
    if (h->sel_scratch) HIPCHK(hipFree(h->sel_scratch));  // (waits for whatever still reads it)
    h->sel_scratch = nullptr, h->sel_blocks = 0;
    HIPCHK(hipMalloc(&h->sel_scratch, cap * (sizeof(long long) + 2 * sizeof(double))));
    h->sel_blocks = cap;
  }
  *scratch_out = h->sel_scratch, *cap_out = h->sel_blocks;
  return SKYJO_OK;
}

extern "C" {

const char *skyjo_vec_last_error(void) { return g_err.c_str(); }
int skyjo_vec_abi_version(void) { return SKYJO_ABI_VERSION; }

int skyjo_vec_create(const skyjo_vec_config *cfg, skyjo_vec **out) {
  if (!cfg || !out) return fail(SKYJO_E_INVALID, "null argument");
  *out = nullptr;
  if (cfg->abi_version != SKYJO_ABI_VERSION) return fail(SKYJO_E_INVALID, "abi_version mismatch");
  if (cfg->num_envs <= 0) return fail(SKYJO_E_INVALID, "num_envs must be > 0");
  if (cfg->num_players <= 0 || cfg->num_players > SKYJO_MAX_PLAYERS)  // skyjo.py:24-26
    return fail(SKYJO_E_INVALID, "Skyjo can be played from 1 up to 8 (recommended) / 12 (theoretical) players");
  if (cfg->rng_mode != SKYJO_RNG_MT19937 && cfg->rng_mode != SKYJO_RNG_PHILOX)
    return fail(SKYJO_E_INVALID, "unknown rng_mode");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SKYJO_E_NOGPU, "no HIP device visible: this library has no CPU fallback");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(SKYJO_E_INVALID, "device_id out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, cfg->device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !sk_diag_env("SKYJO_ALLOW_ANY_GPU"))
    return fail(SKYJO_E_NOGPU, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950");
  DevGuard guard_(cfg->device_id);  // (the caller's current device is restored on return)

  skyjo_vec *h = new (std::nothrow) skyjo_vec();
  if (!h) return fail(SKYJO_E_INVALID, "out of host memory");
  h->cfg = *cfg;
  h->generation = ++g_generation;
  SkParams &P = h->P;
  P.L = sk_make_layout(cfg->num_players, cfg->observe_indirect);
  P.B = cfg->num_envs;
  P.tiles = (cfg->num_envs + SK_TILE - 1) / SK_TILE;
  P.rng_mode = cfg->rng_mode;
  P.auto_reset = cfg->auto_reset ? 1 : 0;
  P.score_penalty = cfg->score_penalty, P.mean_reward = cfg->mean_reward;
  P.reward_refunded = cfg->reward_refunded, P.illegal_reward = cfg->illegal_reward;
  P.game_id0 = cfg->game_id0;
  P.spin_log2 = 22, P.debug_deal_delay = 0;
  h->G = (size_t)P.tiles * SK_TILE;
  h->lds_tile = (size_t)P.L.chunks * 1024;
  // tile + one iteration's records (64 B each, or rec_bytes + 16 for the direct observation; the rare paths' RNG scratch
  // aliases this area) + per-lane per-seat float64 statistics
  h->lds_bytes = h->lds_tile + (size_t)SK_TILE * (P.L.indirect ? 64 : P.L.rec_bytes + 16) + (size_t)SK_ACC_KINDS * cfg->num_players * 512 +
                 (cfg->num_players < 8 ? (size_t)cfg->num_players * 1024 : 0);  // + the card chunks of games waiting to be scored
  const bool fixed_n = cfg->num_players >= 2 && cfg->num_players <= 4;
  h->lds_step = fixed_n ? h->lds_tile + (size_t)SK_TILE * (P.L.indirect ? 64 : P.L.rec_bytes + 16) : h->lds_bytes;
  h->lds_rollout = fixed_n ? h->lds_step + (size_t)cfg->num_players * 1024 : h->lds_bytes;
  if (const char *e = sk_diag_env("SKYJO_LDS_PAD"))  // diagnostic: caps the wavefronts per CU
    h->lds_bytes += (size_t)atoi(e), h->lds_rollout += (size_t)atoi(e), h->lds_step += (size_t)atoi(e);
  const size_t rec16 = (size_t)P.tiles * P.L.chunks * SK_TILE;
  if ((uint64_t)SK_BANK * rec16 * 16 >= (1ull << 32)) {  // (LDS-DMA addresses the bank with 32-bit offsets)
    delete h;
    return fail(SKYJO_E_INVALID, "num_envs too large for one handle");
  }
  int rc = SKYJO_OK;
  const size_t N = (size_t)cfg->num_players;
  auto carve = [&]() -> int {
    int rc = SKYJO_OK;
    // (the largest array first: 164 MB at the headline size, walked in 64-byte pieces by the dealing kernel - it gets the
    // most contiguous backing a freshly started process can have)
    if (cfg->rng_mode == SKYJO_RNG_MT19937 && (rc = dalloc(h, &P.mt, h->G * 624 + 16, false)  /* + 16: MtChunkStream::issue reads one word beyond a state */)) {
      return rc;
    }
    if ((rc = dalloc(h, &P.state, rec16)) || (rc = dalloc(h, &P.spare, SK_BANK * rec16)) ||
        (rc = dalloc(h, &P.spare_ready, SK_BANK * h->G)) || (rc = dalloc(h, &P.bank_head, h->G)) ||
        (rc = dalloc(h, &P.busy, h->G)) || (rc = dalloc(h, &P.cancel, h->G)) || (rc = dalloc(h, &P.done_flag, h->G)) || (rc = dalloc(h, &P.plan_tag, h->G)) || (rc = dalloc(h, &P.plan_ep, h->G)) ||
        (rc = dalloc(h, &P.deal_list, 2 * h->G)) || (rc = dalloc(h, &P.deal_ep, 2 * h->G)) ||
        (rc = dalloc(h, &P.deal_count, 2)) || (rc = dalloc(h, &P.bank_empty, 2)) ||
        (rc = dalloc(h, &P.mt_idx, (1 + SK_BANK) * h->G)) || (rc = dalloc(h, &P.seeds, h->G)) ||
        (rc = dalloc(h, &P.deals_consumed, h->G)) || (rc = dalloc(h, &P.rewards, h->G * N)) ||
        (rc = dalloc(h, &P.scores, h->G * N)) || (rc = dalloc(h, &P.done, h->G)) ||
        (rc = dalloc(h, &P.acc_tile, (size_t)P.tiles * SK_ACC_KINDS * SKYJO_MAX_PLAYERS)) || (rc = dalloc(h, &P.dev_error, 1)) ||
        (rc = dalloc(h, &P.counters, 1)) || (rc = dalloc(h, &P.tile_counters, (size_t)P.tiles * 8)) || (rc = dalloc(h, &P.stamps, (size_t)P.tiles * 32))) {
      return rc;
    }
    return SKYJO_OK;
  };
  h->arena_mode = 1, h->arena_off = 0;
  (void)carve();
  {
    const size_t two_mb = (size_t)2 << 20, total = h->arena_off + two_mb;
    void *raw = nullptr;
    if (hipMalloc(&raw, total) != hipSuccess) {
      skyjo_vec_destroy(h);
      return fail(SKYJO_E_DEVICE, "hipMalloc failed for the engine's arrays");
    }
    h->owned.push_back(raw);
    h->arena = (uint8_t *)(((uintptr_t)raw + two_mb - 1) & ~(uintptr_t)(two_mb - 1));
  }
  h->arena_mode = 2, h->arena_off = 0;
  rc = carve();
  h->arena_mode = 0;
  if (rc) {
    skyjo_vec_destroy(h);
    return rc;
  }
  int prio_least = 0, prio_greatest = 0;  // the dealing kernel fills what the step kernel leaves idle: lowest priority
  (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (hipStreamCreateWithPriority(&h->deal_stream, hipStreamNonBlocking, prio_least) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_scan, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_dealt, hipEventDisableTiming) != hipSuccess) {
    skyjo_vec_destroy(h);
    return fail(SKYJO_E_DEVICE, "cannot create the dealing stream / events");
  }
  {
    void *dp = nullptr;
    if (hipHostMalloc((void **)&h->health_host, 4 * sizeof(uint32_t), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer(&dp, h->health_host, 0) != hipSuccess) {
      skyjo_vec_destroy(h);
      return fail(SKYJO_E_DEVICE, "cannot map the bank-health word");
    }
    h->health_host[0] = h->health_host[1] = h->health_host[2] = h->health_host[3] = 0;
    P.health_host = (volatile uint32_t *)dp;
  }
  h->raw_stride = (int)((P.L.state_bytes + 16 * cfg->num_players + 8 + 15) & ~15);
  if (h->G <= 4096) {  // small batches: the *_host calls go through host-mapped memory (see the handle's fields)
    const size_t a = (h->G * 4 + 255) & ~(size_t)255, m = (h->G + 255) & ~(size_t)255, r = (h->G * (size_t)P.L.rec_bytes + 255) & ~(size_t)255,
                 w = h->G * (size_t)h->raw_stride;
    void *dp = nullptr;
    if (hipHostMalloc((void **)&h->hm_block, a + m + r + w, hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer(&dp, h->hm_block, 0) == hipSuccess) {
      memset(h->hm_block, 0, a + m + r + w);
      uint8_t *d = (uint8_t *)dp;
      h->hm_actions = (int32_t *)h->hm_block, h->hm_mask = h->hm_block + a, h->hm_records = h->hm_block + a + m, h->hm_raw = h->hm_block + a + m + r;
      h->hm_actions_d = (int32_t *)d, h->hm_mask_d = d + a, h->hm_records_d = d + a + m, h->hm_raw_d = d + a + m + r;
      h->fast_host = !sk_diag_env("SKYJO_NO_FAST_HOST");
      h->host_spin = !sk_diag_env("SKYJO_NO_SPIN");
      // Whole games come back with the records only for a few tiles (the single-game views: get_state / rewards after a step
      // without device traffic).  At raw_stride ~ 400 B per game the export is per-lane 16-byte stores at that stride over
      // PCIe - for a mid-size batch whose caller may never ask for a state that is dead weight.
      h->raw_export = h->fast_host && P.tiles <= 4 && !sk_diag_env("SKYJO_NO_RAW_EXPORT");
    }
  }
  h->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  if (const char *e = sk_diag_env("SKYJO_FUSED_SCAN")) h->req.inline_work_list = atoi(e) == 0;  // (diagnostic builds: the options' initial values)
  if (const char *e = sk_diag_env("SKYJO_PIPELINED")) h->req.unpipelined = atoi(e) == 0;
  resolve_form(h);
  if (const char *e = sk_diag_env("SKYJO_DEAL_INTERVAL")) {
    const int v = atoi(e);
    if (v >= 1 && v <= 1024) deals_set_interval(h, v);
  }
  *out = h;
  return SKYJO_OK;
}

int skyjo_vec_destroy(skyjo_vec *h) {
  if (!h) return SKYJO_OK;
  GUARD(h);
  (void)hipDeviceSynchronize();
  if (h->deal_stream) (void)hipStreamDestroy(h->deal_stream);
  if (h->ev_scan) (void)hipEventDestroy(h->ev_scan);
  if (h->ev_dealt) (void)hipEventDestroy(h->ev_dealt);
  for (void *p : h->owned) (void)hipFree(p);
  if (h->sel_scratch) (void)hipFree(h->sel_scratch);
  for (auto &v : h->ev)
    for (auto &e : v) (void)hipEventDestroy(e.first), (void)hipEventDestroy(e.second);
  if (h->health_host) (void)hipHostFree(h->health_host);
  if (h->hm_block) (void)hipHostFree(h->hm_block);
  delete h;
  return SKYJO_OK;
}

int skyjo_vec_get_info(const skyjo_vec *h, skyjo_vec_info *out) {
  if (!h || !out) return fail(SKYJO_E_INVALID, "null argument");
  const SkLayout &L = h->P.L;
  out->num_envs = h->P.B, out->num_players = L.N, out->obs_dim = L.D, out->record_bytes = L.rec_bytes;
  out->mask_offset = L.Dp, out->meta_offset = L.Dp + 26, out->state_bytes = L.state_bytes, out->tile_games = SK_TILE;
  return SKYJO_OK;
}

int skyjo_vec_seed(skyjo_vec *h, const uint64_t *seeds_host, uint64_t base_seed, void *stream) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  hipStream_t s = (hipStream_t)stream;
  GUARD(h);
  h->raw_valid = false;
  uint64_t *d_seeds = nullptr;
  if (seeds_host) {
    HIPCHK(hipMalloc((void **)&d_seeds, sizeof(uint64_t) * (size_t)h->P.B));
    HIPCHK(hipMemcpyAsync(d_seeds, seeds_host, sizeof(uint64_t) * (size_t)h->P.B, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipDeviceSynchronize());  // (nothing of the old life of the handle is still running)
  HIPCHK(hipMemsetAsync(h->P.done, 0, h->G, s));
  HIPCHK(hipMemsetAsync(h->P.dev_error, 0, sizeof(uint32_t), s));  // a new seeding starts from a clean slate
  h->health_host[2] = 0;
  int rc;
  if ((rc = deals_drain(h, s))) return rc;  // drain the dealing pipeline of the previous seeding, if any
  hipLaunchKernelGGL(k_seed, dim3((h->P.B + 255) / 256), dim3(256), 0, s, h->P, (const uint64_t *)d_seeds, base_seed, 0,
                     h->P.B);
  HIPCHK(hipGetLastError());
  // set_seed deals immediately (skyjo.py:88): deal #0 becomes the live game, the following ones fill the bank
  if ((rc = deals_refill(h, s))) return rc;
  h->seeded = true;
  if ((rc = skyjo_vec_reset(h, nullptr, nullptr, stream))) return rc;
  for (int k = 1; k < SK_BANK; k++)
    if ((rc = deals_refill(h, s))) return rc;
  if (d_seeds) {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipFree(d_seeds));
  }
  h->iter = 0;
  return skyjo_vec_reset_counters(h, stream);
}

static int ensure_scratch(skyjo_vec *h);

int skyjo_vec_seed_one(skyjo_vec *h, int32_t game, uint64_t value, void *stream) {
  if (!h || game < 0 || game >= h->P.B) return fail(SKYJO_E_INVALID, "bad argument");
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  GUARD(h);
  h->raw_valid = false;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = ensure_scratch(h)) || (rc = deals_drain(h, s))) return rc;  // nobody else may be using the stream that is re-seeded
  uint64_t *d_seed = (uint64_t *)h->d_actions;                               // (8 bytes of the host-style scratch)
  HIPCHK(hipMemcpyAsync(d_seed, &value, sizeof(value), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // (`value` lives on this stack frame)
  hipLaunchKernelGGL(k_seed, dim3(1), dim3(64), 0, s, h->P, (const uint64_t *)d_seed, (uint64_t)0, (int)game, 1);
  HIPCHK(hipGetLastError());
  if ((rc = deals_refill(h, s))) return rc;  // deal #0 of the new stream ...
  HIPCHK(hipMemsetAsync(h->d_mask, 0, h->G, s));
  const uint8_t one = 1;
  HIPCHK(hipMemcpyAsync(h->d_mask + game, &one, 1, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  if ((rc = skyjo_vec_reset(h, h->d_mask, nullptr, stream))) return rc;    // ... becomes the live game
  for (int k = 1; k < SK_BANK; k++)
    if ((rc = deals_refill(h, s))) return rc;
  return SKYJO_OK;
}

int skyjo_vec_snapshot_create(skyjo_vec *h, skyjo_vec_snapshot **out, void *stream) {
  if (!h || !out) return fail(SKYJO_E_INVALID, "null argument");
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  GUARD(h);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = deals_drain(h, s))) return rc;  // no deal in flight: the arrays below are the whole truth
  HIPCHK(hipDeviceSynchronize());
  if ((rc = dev_error_fetch(h, s))) return rc;   // (a voided run is not worth keeping)
  skyjo_vec_snapshot *sn = new (std::nothrow) skyjo_vec_snapshot();
  if (!sn) return fail(SKYJO_E_INVALID, "out of host memory");
  sn->owner = h, sn->owner_generation = h->generation, sn->device_id = h->cfg.device_id;
  for (auto &a : h->allocs) sn->bytes += (a.second + 255) & ~(size_t)255, sn->array_bytes.push_back(a.second);
  if (hipMalloc(&sn->blob, sn->bytes) != hipSuccess) {
    delete sn;
    return fail(SKYJO_E_DEVICE, "hipMalloc failed for the snapshot");
  }
  size_t off = 0;
  for (auto &a : h->allocs) {
    hipError_t e = hipMemcpyAsync((uint8_t *)sn->blob + off, a.first, a.second, hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) {
      (void)hipFree(sn->blob);
      delete sn;
      return fail(SKYJO_E_DEVICE, std::string("snapshot copy: ") + hipGetErrorString(e));
    }
    off += (a.second + 255) & ~(size_t)255;
  }
  if (hipError_t e = hipStreamSynchronize(s); e != hipSuccess) {
    (void)hipFree(sn->blob);
    delete sn;
    return fail(SKYJO_E_DEVICE, std::string("snapshot copy: ") + hipGetErrorString(e));
  }
  sn->deal = h->deal.st;  // (nothing in flight: the state is the whole schedule)
  sn->iter = h->iter, sn->iters_total = h->iters_total;
  sn->health[0] = h->health_host[0], sn->health[1] = h->health_host[1];
  *out = sn;
  return SKYJO_OK;
}

int skyjo_vec_snapshot_restore(skyjo_vec *h, const skyjo_vec_snapshot *sn, void *stream) {
  if (!h || !sn) return fail(SKYJO_E_INVALID, "null argument");
  if (sn->owner != h || sn->owner_generation != h->generation)  // (a destroyed handle's address may have been reused)
    return fail(SKYJO_E_INVALID, "the snapshot was taken from another handle");
  // the blob is the handle's arrays in table order: the same count (or fewer: the host-style scratch may have been
  // allocated since) of the same sizes
  if (sn->array_bytes.size() > h->allocs.size()) return fail(SKYJO_E_INVALID, "the snapshot does not fit the handle's arrays");
  for (size_t k = 0; k < sn->array_bytes.size(); k++)
    if (sn->array_bytes[k] != h->allocs[k].second) return fail(SKYJO_E_INVALID, "the snapshot does not fit the handle's arrays");
  GUARD(h);
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = deals_drain(h, s))) return rc;
  HIPCHK(hipDeviceSynchronize());
  size_t off = 0;
  for (size_t k = 0; k < sn->array_bytes.size(); k++) {  // (arrays allocated after the snapshot are not part of it)
    const auto &a = h->allocs[k];
    HIPCHK(hipMemcpyAsync(a.first, (const uint8_t *)sn->blob + off, a.second, hipMemcpyDeviceToDevice, s));
    off += (a.second + 255) & ~(size_t)255;
  }
  HIPCHK(hipStreamSynchronize(s));
  h->deal.st = sn->deal, h->P.deal_tag = sn->deal.deal_tag;  // (the drain above left nothing in flight; form and options stay today's)
  h->iter = sn->iter, h->iters_total = sn->iters_total;
  h->health_host[0] = sn->health[0], h->health_host[1] = sn->health[1];
  h->health_host[2] = 0;  // the restored device word is clean (snapshot_create refuses a voided run): so is the host's copy
  h->raw_valid = false;
  return SKYJO_OK;
}

int skyjo_vec_snapshot_bytes(const skyjo_vec_snapshot *sn, size_t *bytes_out) {
  if (!sn || !bytes_out) return fail(SKYJO_E_INVALID, "null argument");
  *bytes_out = sn->bytes;
  return SKYJO_OK;
}

int skyjo_vec_snapshot_destroy(skyjo_vec_snapshot *sn) {
  if (!sn) return SKYJO_OK;
  DevGuard guard_(sn->device_id);
  (void)hipFree(sn->blob);
  delete sn;
  return SKYJO_OK;
}

static int reset_impl(skyjo_vec *h, const uint8_t *mask, void *records_out, hipStream_t s, uint8_t *raw_out, int planar = 0) {
  int rc;
  h->raw_valid = false;
  if ((rc = deals_drain(h, s))) return rc;  // make every dealt episode available
  dim3 grid(h->P.tiles), block(SK_TILE);
  if (h->P.L.indirect)
    hipLaunchKernelGGL((k_reset<true>), grid, block, h->lds_bytes, s, h->P, mask, (uint8_t *)records_out, raw_out, h->raw_stride, planar);
  else
    hipLaunchKernelGGL((k_reset<false>), grid, block, h->lds_bytes, s, h->P, mask, (uint8_t *)records_out, raw_out, h->raw_stride, 0);
  HIPCHK(hipGetLastError());
  return deals_refill(h, s);  // what was taken (one episode per game and cycle)
}

int skyjo_vec_reset(skyjo_vec *h, const uint8_t *mask, void *records_out, void *stream) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  return reset_impl(h, mask, records_out, (hipStream_t)stream, nullptr, h->rec_planar_all ? 1 : 0);
}

static int step_once(skyjo_vec *h, const int32_t *actions, void *records_out, double *end_rew, uint8_t *end_flag, hipStream_t s,
                     uint8_t *raw_out = nullptr, bool planar_out = false, uint32_t host_seq = 0) {
  const StepLaunch L = deals_plan_launch(h, 1, false);
  const int rc = launch_step(h, s, L, false, actions, (uint8_t *)records_out, nullptr, 0, end_rew, end_flag, raw_out, planar_out && records_out, host_seq);
  return rc ? rc : deals_finish_launch(h, s, L);
}

int skyjo_vec_step(skyjo_vec *h, const int32_t *actions, void *records_out, void *stream) {
  if (!h || !actions) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  return step_once(h, actions, records_out, nullptr, nullptr, (hipStream_t)stream, nullptr, h->rec_planar_all);
}

int skyjo_vec_step_collect(skyjo_vec *h, const int32_t *actions, void *records_out, double *final_rewards_out,
                           uint8_t *episode_end_out, void *stream) {
  if (!h || !actions || !final_rewards_out || !episode_end_out) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  return step_once(h, actions, records_out, final_rewards_out, episode_end_out, (hipStream_t)stream, nullptr, h->rec_planar_all);
}

// ---- config 5's collection loop (include/skyjo_vec.h: skyjo_vec_model_rollout) ----
static int model_check(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, int32_t T, const skyjo_vec_rollout_buffers *b) {
  if (!h || !policy || !b || T < 0 || !b->records || !b->actions) return fail(SKYJO_E_INVALID, "skyjo_vec_model_rollout: bad argument");
  if (value && !b->values) return fail(SKYJO_E_INVALID, "skyjo_vec_model_rollout: a value net needs a values buffer");
  if ((b->final_rewards == nullptr) != (b->episode_end == nullptr))
    return fail(SKYJO_E_INVALID, "skyjo_vec_model_rollout: final_rewards and episode_end go together");
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  if (policy->net.out_dim != SKYJO_NUM_ACTIONS) return fail(SKYJO_E_INVALID, "the policy net needs 26 outputs");
  if (policy->device_id != h->cfg.device_id || policy->obs_dim != h->P.L.D)
    return fail(SKYJO_E_INVALID, "the policy net must live on the engine's device and take the engine's observation (obs_dim)");
  if (value && (policy->obs_dim != value->obs_dim || policy->device_id != value->device_id || policy->net.split != value->net.split))
    return fail(SKYJO_E_INVALID, "policy and value net must share the observation size, the precision and the device");
  return SKYJO_OK;
}
// iteration t: [policy (+ value) net with the draw in its epilogue] -> [step kernel with the episode-end columns]
static int model_iter(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, int t, uint64_t seed, uint64_t first_ticket,
                      int32_t no_masking, const skyjo_vec_rollout_buffers *b, hipStream_t s) {
  const size_t B = (size_t)h->P.B, rb = (size_t)h->P.L.rec_bytes, N = (size_t)h->P.L.N, vd = value ? (size_t)value->net.out_dim : 0;
  const bool planar = h->rec_planar_all;        // (SKYJO_REC_TILE_PLANAR_ALL: an iteration's records are tiles * 64 slots, piece-planar)
  const size_t per_it = (planar ? h->G : B) * rb;
  uint8_t *rec = (uint8_t *)b->records;
  SkMlpDraw d{};
  d.enable = 1, d.mask_offset = h->P.L.Dp, d.no_masking = no_masking, d.seed = seed, d.ticket = first_ticket + (uint64_t)t;
  d.game_id0 = h->P.game_id0, d.actions = b->actions + (size_t)t * B, d.logp = b->logp ? b->logp + (size_t)t * B : nullptr;
  hipEvent_t e0, e1;  // skyjo_vec_profile's slot 4
  int rc = prof_events(h, 4, &e0, &e1);
  if (rc) return rc;
  rc = launch_mlp(policy, value ? value : policy, value ? 2 : 1, rec + (size_t)t * per_it, (int)rb, policy->obs_dim, (int64_t)B, nullptr, d,
                  value ? b->values + (size_t)t * B * vd : nullptr, s, planar ? 1 : 0, e0, e1);
  if (rc) return rc;
  return step_once(h, b->actions + (size_t)t * B, rec + (size_t)(t + 1) * per_it, b->final_rewards ? b->final_rewards + (size_t)t * B * N : nullptr,
                   b->episode_end ? b->episode_end + (size_t)t * B : nullptr, s, nullptr, planar);
}
// the bootstrap value of the records a rollout ends on
static int model_tail(skyjo_vec *h, const skyjo_vec_mlp *value, int T, const skyjo_vec_rollout_buffers *b, hipStream_t s) {
  if (!value) return SKYJO_OK;
  const size_t B = (size_t)h->P.B, rb = (size_t)h->P.L.rec_bytes, vd = (size_t)value->net.out_dim;
  SkMlpDraw nodraw{};
  return launch_mlp(value, value, 1, (const uint8_t *)b->records + (size_t)T * (h->rec_planar_all ? h->G : B) * rb, (int)rb, value->obs_dim, (int64_t)B,
                    b->values + (size_t)T * B * vd, nodraw, nullptr, s, h->rec_planar_all ? 1 : 0);
}

int skyjo_vec_model_rollout(skyjo_vec *h, const skyjo_vec_mlp *policy, const skyjo_vec_mlp *value, int32_t T, uint64_t seed,
                            uint64_t first_ticket, int32_t no_masking, const skyjo_vec_rollout_buffers *b, void *stream) {
  int rc = model_check(h, policy, value, T, b);
  if (rc) return rc;
  GUARD(h);
  for (int t = 0; t < T; t++)
    if ((rc = model_iter(h, policy, value, t, seed, first_ticket, no_masking, b, (hipStream_t)stream))) return rc;
  return model_tail(h, value, T, b, (hipStream_t)stream);
}

int skyjo_vec_rollout(skyjo_vec *h, int32_t iters, uint64_t policy_seed, void *records_out, int32_t *actions_out,
                      void *stream) {
  if (!h || iters < 0) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  hipStream_t s = (hipStream_t)stream;
  uint8_t *rec = (uint8_t *)records_out;
  const bool planar = h->rec_planar;
  if (planar && rec && h->form != DealForm::OneKernel)
    return fail(SKYJO_E_STATE, "SKYJO_OPT_RECORD_LAYOUT = tile-planar needs the one-kernel dealing form (SKYJO_OPT_OVERLAP 3)");
  for (int done = 0; done < iters;) {
    const StepLaunch L = deals_plan_launch(h, iters - done, true);
    int rc;
    if ((rc = launch_step(h, s, L, true, nullptr, rec, actions_out, policy_seed)) || (rc = deals_finish_launch(h, s, L))) return rc;
    done += L.iters;
    if (rec) rec += (size_t)L.iters * (planar ? h->G : (size_t)h->P.B) * h->P.L.rec_bytes;
    if (actions_out) actions_out += (size_t)L.iters * h->P.B;
  }
  return SKYJO_OK;
}

static int observe_impl(skyjo_vec *h, const int32_t *players, void *records_out, void *stream, int planar) {
  if (!h || !records_out) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  dim3 grid(h->P.tiles), block(SK_TILE);
  hipStream_t s = (hipStream_t)stream;
  if (h->P.L.indirect)
    hipLaunchKernelGGL((k_observe<true>), grid, block, h->lds_bytes, s, h->P, players, (uint8_t *)records_out, planar);
  else
    hipLaunchKernelGGL((k_observe<false>), grid, block, h->lds_bytes, s, h->P, players, (uint8_t *)records_out, 0);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
int skyjo_vec_observe(skyjo_vec *h, const int32_t *players, void *records_out, void *stream) {
  return observe_impl(h, players, records_out, stream, h && h->rec_planar_all ? 1 : 0);
}

static int unpack_impl(skyjo_vec *h, const void *records, int64_t n, int8_t *obs, int8_t *mask, uint8_t *agent, uint8_t *phase, uint8_t *done,
                       uint8_t *status, void *stream, int planar) {
  if (!h || !records || n < 0) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (n == 0) return SKYJO_OK;
  long long total = n * (long long)(h->P.L.D + 26);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_unpack, dim3(blocks), dim3(256), 0, (hipStream_t)stream, h->P.L, (const uint8_t *)records,
                     (long long)n, obs, mask, agent, phase, done, status, planar);
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}

int skyjo_vec_unpack(skyjo_vec *h, const void *records, int64_t n, int8_t *obs, int8_t *mask, uint8_t *agent,
                     uint8_t *phase, uint8_t *done, uint8_t *status, void *stream) {
  return unpack_impl(h, records, n, obs, mask, agent, phase, done, status, stream, 0);
}

int skyjo_vec_unpack_tiles(skyjo_vec *h, const void *records, int64_t n_tiles, int8_t *obs, int8_t *mask, uint8_t *agent,
                           uint8_t *phase, uint8_t *done, uint8_t *status, void *stream) {
  return unpack_impl(h, records, n_tiles * SK_TILE, obs, mask, agent, phase, done, status, stream, 1);
}

const double *skyjo_vec_rewards_ptr(const skyjo_vec *h) { return h ? h->P.rewards : nullptr; }
const double *skyjo_vec_scores_ptr(const skyjo_vec *h) { return h ? h->P.scores : nullptr; }
const uint8_t *skyjo_vec_done_ptr(const skyjo_vec *h) { return h ? h->P.done : nullptr; }

int skyjo_vec_sample_actions_layout(skyjo_vec *h, const void *records, int32_t layout, const float *logits, int64_t n, uint64_t seed,
                                    uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                                    float *uniform_out, void *stream) {
  if (!h || !records || !logits || !actions_out || n < 0) return fail(SKYJO_E_INVALID, "null argument");
  if (int rc = check_layout(layout)) return rc;
  GUARD(h);
  if (n == 0) return SKYJO_OK;
  const int64_t blocks = (n + SK_SAMPLE_BLOCK - 1) / SK_SAMPLE_BLOCK;
  hipLaunchKernelGGL(k_sample, dim3((unsigned)blocks), dim3(SK_SAMPLE_BLOCK), 0, (hipStream_t)stream, h->P.L,
                     (const uint8_t *)records, logits, (long long)n, seed, ticket, h->P.game_id0, (int)no_masking,
                     actions_out, logp_out, uniform_out, (int)(layout == SKYJO_REC_TILE_PLANAR));
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
int skyjo_vec_sample_actions(skyjo_vec *h, const void *records, const float *logits, int64_t n, uint64_t seed,
                             uint64_t ticket, int32_t no_masking, int32_t *actions_out, float *logp_out,
                             float *uniform_out, void *stream) {
  return skyjo_vec_sample_actions_layout(h, records, SKYJO_REC_ROW_MAJOR, logits, n, seed, ticket, no_masking, actions_out, logp_out, uniform_out,
                                         stream);
}

int skyjo_vec_episode_ends_layout(skyjo_vec *h, const void *records, int32_t layout, double *final_rewards_out, uint8_t *episode_end_out,
                                  void *stream) {
  if (!h || !records || !final_rewards_out || !episode_end_out) return fail(SKYJO_E_INVALID, "null argument");
  if (int rc = check_layout(layout)) return rc;
  GUARD(h);
  hipLaunchKernelGGL(k_episode_ends, dim3((h->P.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, h->P, (const uint8_t *)records,
                     final_rewards_out, episode_end_out, (int)(layout == SKYJO_REC_TILE_PLANAR));
  HIPCHK(hipGetLastError());
  return SKYJO_OK;
}
int skyjo_vec_episode_ends(skyjo_vec *h, const void *records, double *final_rewards_out, uint8_t *episode_end_out, void *stream) {
  return skyjo_vec_episode_ends_layout(h, records, SKYJO_REC_ROW_MAJOR, final_rewards_out, episode_end_out, stream);
}

int skyjo_vec_get_counters(skyjo_vec *h, skyjo_vec_counters *out, void *stream) {
  if (!h || !out) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  static_assert(sizeof(SkCounters) == sizeof(skyjo_vec_counters), "counter structs must match");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(h->P.counters, 0, sizeof(SkCounters), s));
  hipLaunchKernelGGL(k_reduce_stats, dim3(64), dim3(256), 0, s, h->P);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, h->P.counters, sizeof(SkCounters), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  out->iters = h->iters_total;
  return dev_error_fetch(h, s);
}

int skyjo_vec_check_error(skyjo_vec *h, void *stream) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  return dev_error_fetch(h, (hipStream_t)stream);
}

int skyjo_vec_reset_counters(skyjo_vec *h, void *stream) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  const size_t n = (size_t)h->P.tiles * SK_ACC_KINDS * SKYJO_MAX_PLAYERS * sizeof(double);
  h->iters_total = 0;
  HIPCHK(hipMemsetAsync(h->P.counters, 0, sizeof(SkCounters), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(h->P.tile_counters, 0, (size_t)h->P.tiles * 8 * sizeof(unsigned long long), (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(h->P.acc_tile, 0, n, (hipStream_t)stream));
  return SKYJO_OK;
}

// raw packed record (skyjo_layout.h) -> the canonical form of include/skyjo_vec.h (rewards / final_score are filled by the caller)
static void decode_state(const SkLayout &L, const uint8_t *r, skyjo_game_state *o) {
  memset(o, 0, sizeof(*o));
  for (int p = 0; p < L.N; p++)
    for (int k = 0; k < 12; k++) {
      int8_t c = (int8_t)r[sk_pb(L, p) + PB_CARDS + k], v = (int8_t)r[sk_pb(L, p) + PB_VIS + k];
      o->players_cards[p][k] = c;
      o->players_masked[p][k] = v == SKYJO_HAND_NONE ? 2 : (v == SKYJO_REFUNDED ? 0 : 1);
    }
  const int role = r[H_ROLE];
  o->n_draw = r[H_NDRAW], o->n_disc = r[H_NDISC];
  for (int k = 0; k < o->n_draw; k++) o->drawpile[k] = (int8_t)r[L.off_pile + (role ? SK_NCARDS - 1 - k : k)];
  for (int k = 0; k < o->n_disc; k++) o->discard_pile[k] = (int8_t)r[L.off_pile + (role ? k : SK_NCARDS - 1 - k)];
  o->hand_card = (int8_t)r[H_HAND];
  o->expected_player = r[H_PLAYER], o->expected_phase = r[H_PHASE];
  o->is_terminated = (r[H_FLAGS] & F_TERMINATED) ? 1 : 0;
  o->done = (r[H_FLAGS] & F_DONE) ? 1 : 0;
  o->status = r[H_STATUS];
  memcpy(&o->episode_steps, &r[H_EPLEN], 2);
  memcpy(&o->episode, &r[H_EPISODE], 4);
  o->reshuffles = r[H_RESH];
  for (int p = 0; p < L.N; p++) {
    o->num_refunded[p] = r[sk_pb(L, p) + PB_REFUNDED];
    uint16_t pl;
    memcpy(&pl, &r[sk_pb(L, p) + PB_PLACED], 2);
    o->num_placed[p] = pl;
  }
}

int skyjo_vec_get_state(skyjo_vec *h, int32_t game, skyjo_game_state *o, void *stream) {
  if (!h || !o || game < 0 || game >= h->P.B) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  hipStream_t s = (hipStream_t)stream;
  const SkLayout &L = h->P.L;
  if (h->raw_valid) {  // the last *_host call brought every game back with its records: no device traffic
    const uint8_t *raw = h->hm_raw + (size_t)game * h->raw_stride;
    decode_state(L, raw, o);
    const double *d = (const double *)(raw + L.state_bytes);
    if (o->done) {
      memcpy(o->rewards, d, sizeof(double) * L.N);
      if (o->is_terminated) memcpy(o->final_score, d + L.N, sizeof(double) * L.N);
    }
    return dev_error_check(h);
  }
  std::vector<uint8_t> r;
  int rc = fetch_record(h, h->P.state, game, r, s);
  if (rc) return rc;
  decode_state(L, r.data(), o);
  if (o->done) {
    HIPCHK(hipMemcpyAsync(o->rewards, h->P.rewards + (size_t)game * L.N, sizeof(double) * L.N, hipMemcpyDeviceToHost, s));
    if (o->is_terminated)
      HIPCHK(hipMemcpyAsync(o->final_score, h->P.scores + (size_t)game * L.N, sizeof(double) * L.N,
                            hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return dev_error_check(h);
}

int skyjo_vec_set_state(skyjo_vec *h, int32_t game, const skyjo_game_state *in, void *stream) {
  if (!h || !in || game < 0 || game >= h->P.B) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  h->raw_valid = false;
  const SkLayout &L = h->P.L;
  if (in->n_draw < 0 || in->n_disc < 0 || in->n_draw + in->n_disc > SK_NCARDS)
    return fail(SKYJO_E_INVALID, "pile sizes out of range");
  if (in->expected_player >= L.N || in->expected_phase > 1) return fail(SKYJO_E_INVALID, "bad expected action");
  hipStream_t s = (hipStream_t)stream;
  std::vector<uint8_t> r((size_t)L.state_bytes, 0);
  int ms = 1 << 30, mh = 1 << 30;
  for (int p = 0; p < L.N; p++) {
    int sum = 0, hid = 0;
    for (int k = 0; k < 12; k++) {
      int8_t c = in->players_cards[p][k];
      int m = in->players_masked[p][k];
      if (c < -2 && !(m == 0 && c == SKYJO_REFUNDED)) return fail(SKYJO_E_INVALID, "card value out of range");
      if (c > 12) return fail(SKYJO_E_INVALID, "card value out of range");
      int8_t v = m == 2 ? (int8_t)SKYJO_HAND_NONE : (m == 0 ? (int8_t)SKYJO_REFUNDED : c);
      r[sk_pb(L, p) + PB_CARDS + k] = (uint8_t)(m == 0 ? (int8_t)SKYJO_REFUNDED : c);
      r[sk_pb(L, p) + PB_VIS + k] = (uint8_t)v;
      if (m == 1) {
        sum += c;
        if (!L.indirect) r[H_HIST + 2 + c]++;
      }
      if (m == 2) hid++;
    }
    int16_t s16 = (int16_t)sum;
    memcpy(&r[sk_pb(L, p) + PB_SUM], &s16, 2);
    r[sk_pb(L, p) + PB_HIDDEN] = (uint8_t)hid;
    r[sk_pb(L, p) + PB_REFUNDED] = (uint8_t)in->num_refunded[p];
    uint16_t pl = (uint16_t)in->num_placed[p];
    memcpy(&r[sk_pb(L, p) + PB_PLACED], &pl, 2);
    ms = sum < ms ? sum : ms, mh = hid < mh ? hid : mh;
  }
  for (int k = 0; k < in->n_draw; k++) r[L.off_pile + k] = (uint8_t)in->drawpile[k];
  for (int k = 0; k < in->n_disc; k++) {
    int8_t c = in->discard_pile[k];
    if (c < -2 || c > 12) return fail(SKYJO_E_INVALID, "discard value out of range");
    r[L.off_pile + SK_NCARDS - 1 - k] = (uint8_t)c;
    r[H_HIST + 2 + c]++;
  }
  r[H_PHASE] = in->expected_phase, r[H_PLAYER] = in->expected_player;
  r[H_FLAGS] = F_VALID | (in->is_terminated ? (F_TERMINATED | F_DONE) : 0) | (in->done ? F_DONE : 0);
  r[H_STATUS] = in->status;
  r[H_NDRAW] = (uint8_t)in->n_draw, r[H_NDISC] = (uint8_t)in->n_disc, r[H_ROLE] = 0;
  memcpy(&r[H_EPLEN], &in->episode_steps, 2);
  r[H_RESH] = (uint8_t)(in->reshuffles > 255 ? 255 : in->reshuffles);
  memcpy(&r[H_EPISODE], &in->episode, 4);
  r[H_MINSUM] = (uint8_t)(int8_t)(ms < 127 ? ms : 127);
  r[H_MINHID] = (uint8_t)mh;
  r[H_TOP] = in->n_disc ? (uint8_t)in->discard_pile[in->n_disc - 1] : (uint8_t)(int8_t)-3;
  r[H_HAND] = (uint8_t)in->hand_card;
  HIPCHK(hipMemcpyAsync(&r[H_BANK], h->P.bank_head + game, 1, hipMemcpyDeviceToHost, s));  // keep the bank pointer
  HIPCHK(hipStreamSynchronize(s));
  uint8_t *dst = (uint8_t *)(h->P.state + ((size_t)(game / SK_TILE) * L.chunks) * SK_TILE + game % SK_TILE);
  HIPCHK(hipMemcpy2DAsync(dst, SK_TILE * 16, r.data(), 16, 16, L.chunks, hipMemcpyHostToDevice, s));
  uint8_t dn = (r[H_FLAGS] & F_DONE) ? 1 : 0;
  HIPCHK(hipMemcpyAsync(h->P.done + game, &dn, 1, hipMemcpyHostToDevice, s));
  if (dn) {
    HIPCHK(hipMemcpyAsync(h->P.rewards + (size_t)game * L.N, in->rewards, sizeof(double) * L.N, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->P.scores + (size_t)game * L.N, in->final_score, sizeof(double) * L.N,
                          hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return SKYJO_OK;
}

int skyjo_vec_seed_raw(skyjo_vec *h, int32_t game, uint32_t value, void *stream) {
  if (!h || game < 0 || game >= h->P.B) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  if (h->P.rng_mode != SKYJO_RNG_MT19937) return fail(SKYJO_E_STATE, "seed_raw needs the MT19937 mode");
  h->raw_valid = false;
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = deals_drain(h, s))) return rc;  // nobody else may be using the stream that is re-seeded
  hipLaunchKernelGGL(k_seed_raw, dim3(1), dim3(64), 0, s, h->P, game, value);
  HIPCHK(hipGetLastError());
  return deals_refill(h, s);
}

int skyjo_vec_rng_set_state(skyjo_vec *h, int32_t game, const uint32_t *key_host, int32_t pos, void *stream) {
  if (!h || !key_host || game < 0 || game >= h->P.B || pos < 0 || pos > 624) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  if (h->P.rng_mode != SKYJO_RNG_MT19937 || !h->req.no_bank)
    return fail(SKYJO_E_STATE, "skyjo_vec_rng_set_state needs the MT19937 mode and SKYJO_OPT_NO_BANK (episodes dealt ahead would belong to the old stream)");
  hipStream_t s = (hipStream_t)stream;
  // numpy's (key, pos): the words from pos on are regenerated and unconsumed, everything is of one generation - in the
  // engine's terms position pos with 624 - pos words regenerated ahead (MtStream: idx | ahead << 16); pos == 624 is a fresh block
  const int32_t packed = pos >= 624 ? 0 : (pos | ((624 - pos) << 16));
  HIPCHK(hipMemcpyAsync(h->P.mt + (size_t)game * 624, key_host, 624 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->P.mt_idx + game, &packed, sizeof(packed), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));  // (`packed` lives on this stack frame, `key_host` belongs to the caller)
  return SKYJO_OK;
}

int skyjo_vec_rng_get_state(skyjo_vec *h, int32_t game, uint32_t *key_out_host, int32_t *pos_out_host, void *stream) {
  if (!h || !key_out_host || !pos_out_host || game < 0 || game >= h->P.B) return fail(SKYJO_E_INVALID, "bad argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  if (h->P.rng_mode != SKYJO_RNG_MT19937 || !h->req.no_bank)
    return fail(SKYJO_E_STATE, "skyjo_vec_rng_get_state needs the MT19937 mode and SKYJO_OPT_NO_BANK");
  hipStream_t s = (hipStream_t)stream;
  int32_t packed = 0;
  HIPCHK(hipMemcpyAsync(key_out_host, h->P.mt + (size_t)game * 624, 624 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&packed, h->P.mt_idx + game, sizeof(packed), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int idx = packed & 0xffff, ahead = packed >> 16;
  if (idx >= 624) idx = 0;
  if (idx + ahead > 624) return fail(SKYJO_E_STATE, "the stream's regenerated window wraps: not a numpy state (cannot happen without a bank)");
  if (idx == 0 && ahead == 0) {  // everything consumed, nothing of the next block made yet: numpy's pos == 624
    *pos_out_host = 624;
    return SKYJO_OK;
  }
  // The engine regenerates lazily, 16 words at a time; numpy makes the whole block at once.  Finish the block: words
  // idx + ahead .. 623 from the old word, its successor and the (already new, for i >= 227) word 397 further on.
  uint32_t *mt = key_out_host;
  for (int i = idx + ahead; i < 624; i++) {
    const uint32_t y = (mt[i] & 0x80000000u) | (mt[i + 1 == 624 ? 0 : i + 1] & 0x7fffffffu);
    mt[i] = mt[i + 397 >= 624 ? i + 397 - 624 : i + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }
  *pos_out_host = idx;
  return SKYJO_OK;
}

int skyjo_vec_profile(skyjo_vec *h, int enable, double ms_out[SKYJO_PROF_KERNELS], int64_t launches_out[SKYJO_PROF_KERNELS]) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  HIPCHK(hipDeviceSynchronize());
  for (int k = 0; k < SKYJO_PROF_KERNELS; k++) {
    double tot = 0;
    int64_t cnt = 0;
    for (auto &p : h->ev[k]) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) tot += ms, cnt++;
      (void)hipEventDestroy(p.first);
      (void)hipEventDestroy(p.second);
    }
    h->ev[k].clear();
    if (ms_out) ms_out[k] = tot;
    if (launches_out) launches_out[k] = cnt;
  }
  h->profile = enable != 0;
  return SKYJO_OK;
}

int skyjo_vec_debug_stamps(skyjo_vec *h, uint64_t *out16_host) {
  if (!h || !out16_host) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  const size_t half = (size_t)h->P.tiles * 8;
  std::vector<unsigned long long> t(2 * half);
  HIPCHK(hipMemcpy(t.data(), h->P.stamps, t.size() * 8, hipMemcpyDeviceToHost));
  for (int k = 0; k < 16; k++) out16_host[k] = 0;
  for (size_t i = 0; i < 2 * half; i++) out16_host[(i & 7) + (i >= half ? 8 : 0)] += t[i];  // [0,8) step, [8,16) deal
  HIPCHK(hipMemset(h->P.stamps, 0, t.size() * 8));
  return SKYJO_OK;
}

int skyjo_vec_debug_trace(skyjo_vec *h, uint64_t *out_host) {  // [4][tiles][8]: see TRACE_STORE (skyjo_device.h); zeros unless built with -DSK_TRACE
  if (!h || !out_host) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, h->P.stamps, (size_t)h->P.tiles * 32 * 8, hipMemcpyDeviceToHost));
  return SKYJO_OK;
}

int skyjo_vec_get_option(const skyjo_vec *h, int option, int64_t *value_out) {
  if (!h || !value_out) return fail(SKYJO_E_INVALID, "null argument");
  switch (option) {
    case SKYJO_OPT_DEAL_INTERVAL: *value_out = deals_interval(h); return SKYJO_OK;
    case SKYJO_OPT_OVERLAP: *value_out = h->form == DealForm::OneKernel ? 3 : uses_deal_stream(h->form) ? 2 : 0; return SKYJO_OK;
    case SKYJO_OPT_NO_BANK: *value_out = h->req.no_bank ? 1 : 0; return SKYJO_OK;
    case SKYJO_OPT_RECORD_LAYOUT: *value_out = h->rec_planar_all ? SKYJO_REC_TILE_PLANAR_ALL : h->rec_planar ? SKYJO_REC_TILE_PLANAR : SKYJO_REC_ROW_MAJOR; return SKYJO_OK;
    case SKYJO_OPT_INLINE_WORK_LIST: *value_out = h->req.inline_work_list ? 1 : 0; return SKYJO_OK;
    case SKYJO_OPT_UNPIPELINED: *value_out = h->req.unpipelined ? 1 : 0; return SKYJO_OK;
    case SKYJO_OPT_CYCLE_S: *value_out = h->cycle_s; return SKYJO_OK;
    case SKYJO_OPT_MAX_CYCLES_PER_LAUNCH: *value_out = h->max_cycles > 0 ? h->max_cycles : kMaxCyclesPerLaunch; return SKYJO_OK;
    default: return fail(SKYJO_E_INVALID, "unknown option");
  }
}

int skyjo_vec_set_option(skyjo_vec *h, int option, int64_t value) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  DealRequests req = h->req;
  switch (option) {
    case SKYJO_OPT_DEAL_INTERVAL:
      if (value < 1 || value > 1024) return fail(SKYJO_E_INVALID, "deal interval must be in 1..1024");
      deals_set_interval(h, (int)value);
      return SKYJO_OK;
    case SKYJO_OPT_OVERLAP:
      // 0: in line; 1: beside the step kernel, in the form this engine prefers; 2: the two-stream form; 3: the one-kernel form (k_cycle)
      if (value < 0 || value > 3) return fail(SKYJO_E_INVALID, "SKYJO_OPT_OVERLAP takes 0 .. 3");
      if (value == 3 && !h->one_kernel_capable) return fail(SKYJO_E_INVALID, "the one-kernel form needs two to four players");
      req.overlap = (int)value;
      return change_form(h, req);
    case SKYJO_OPT_NO_BANK:
      if (h->seeded) return fail(SKYJO_E_STATE, "SKYJO_OPT_NO_BANK must be set before skyjo_vec_seed");
      h->req.no_bank = value != 0;
      return SKYJO_OK;
    case SKYJO_OPT_RECORD_LAYOUT:
      if (value != SKYJO_REC_ROW_MAJOR && value != SKYJO_REC_TILE_PLANAR && value != SKYJO_REC_TILE_PLANAR_ALL)
        return fail(SKYJO_E_INVALID, "SKYJO_OPT_RECORD_LAYOUT takes SKYJO_REC_ROW_MAJOR, SKYJO_REC_TILE_PLANAR or SKYJO_REC_TILE_PLANAR_ALL");
      if (value != SKYJO_REC_ROW_MAJOR && !h->one_kernel_capable)
        return fail(SKYJO_E_INVALID, "the tile-planar record layout exists for the one-kernel form of the fused rollout (two to four players)");
      if (value == SKYJO_REC_TILE_PLANAR_ALL && !h->P.L.indirect)
        return fail(SKYJO_E_INVALID, "SKYJO_REC_TILE_PLANAR_ALL: reset / observe / step write tile-planar records of the indirect observation only");
      h->rec_planar = value != SKYJO_REC_ROW_MAJOR;
      h->rec_planar_all = value == SKYJO_REC_TILE_PLANAR_ALL;
      resolve_form(h);  // (k_cycle's LDS regions depend on the layout)
      return SKYJO_OK;
    case SKYJO_OPT_INLINE_WORK_LIST:
      req.inline_work_list = value != 0;
      return change_form(h, req);
    case SKYJO_OPT_UNPIPELINED:
      req.unpipelined = value != 0;
      return change_form(h, req);
    case SKYJO_OPT_CYCLE_S:
      if (h->seeded) return fail(SKYJO_E_STATE, "SKYJO_OPT_CYCLE_S must be set before skyjo_vec_seed");
      if (value < 0 || value > SK_CYCLE_MAX_S) return fail(SKYJO_E_INVALID, "SKYJO_OPT_CYCLE_S takes 0 (the batch's share) .. 4");
      req.cycle_s = (int)value;  // (a value whose regions do not fit a CU's LDS is lowered until they do: resolve_form)
      return change_form(h, req);
    case SKYJO_OPT_MAX_CYCLES_PER_LAUNCH:
      if (value < 1 || value > kMaxCyclesPerLaunch) return fail(SKYJO_E_INVALID, "SKYJO_OPT_MAX_CYCLES_PER_LAUNCH takes 1 .. 16");
      h->max_cycles = (int)value;
      return SKYJO_OK;
    case SKYJO_OPT_DEBUG_SPIN_LOG2:
      if (value < 1 || value > 30) return fail(SKYJO_E_INVALID, "spin limit must be 2^1 .. 2^30");
      h->P.spin_log2 = (uint32_t)value;
      return SKYJO_OK;
    case SKYJO_OPT_DEBUG_DEAL_DELAY:
      if (value < 0 || value > (1 << 24)) return fail(SKYJO_E_INVALID, "deal delay out of range");
      h->P.debug_deal_delay = (uint32_t)value;
      return SKYJO_OK;
    default:
      return fail(SKYJO_E_INVALID, "unknown option");
  }
}

// ---- host-pointer conveniences ------------------------------------------------------------
static int ensure_scratch(skyjo_vec *h) {
  int rc;
  if (!h->d_actions && (rc = dalloc(h, &h->d_actions, h->G))) return rc;
  if (!h->d_records && (rc = dalloc(h, &h->d_records, h->G * (size_t)h->P.L.rec_bytes))) return rc;
  if (!h->d_mask && (rc = dalloc(h, &h->d_mask, h->G))) return rc;
  return SKYJO_OK;
}

// The buffers a *_host call works through, chosen once per call: where the host puts the actions (or players) and the mask and gets
// the records, and what the kernels are given for them.  Mapped: both are the host-mapped block, a put / get is a memcpy and the
// kernel also exports whole games where the engine does that (raw_d).  Staged: both are the device scratch, made when the first
// such call needs it, and a put / get is a hipMemcpy on the null stream.
struct HostBufs {
  bool mapped;
  int32_t *actions, *actions_d;
  uint8_t *mask, *mask_d, *records, *records_d;
  uint8_t *raw_d;  // the raw export's target, or null
};
static int host_bufs(skyjo_vec *h, HostBufs *b) {
  if (h->fast_host) {
    *b = {true, h->hm_actions, h->hm_actions_d, h->hm_mask, h->hm_mask_d, h->hm_records, h->hm_records_d, h->raw_export ? h->hm_raw_d : nullptr};
    return SKYJO_OK;
  }
  if (int rc = ensure_scratch(h)) return rc;
  *b = {false, h->d_actions, h->d_actions, h->d_mask, h->d_mask, h->d_records, h->d_records, nullptr};
  return SKYJO_OK;
}
static int host_copy(const HostBufs &b, void *dst, const void *src, size_t bytes, hipMemcpyKind staged_kind) {  // a put or a get
  if (b.mapped) memcpy(dst, src, bytes);
  else HIPCHK(hipMemcpy(dst, src, bytes, staged_kind));
  return SKYJO_OK;
}
static int host_put(const HostBufs &b, void *dst, const void *src_host, size_t bytes) { return host_copy(b, dst, src_host, bytes, hipMemcpyHostToDevice); }
static int host_get(const HostBufs &b, void *dst_host, const void *src, size_t bytes) { return host_copy(b, dst_host, src, bytes, hipMemcpyDeviceToHost); }
// The launches are through before the host reads on: the null stream is synchronised unless the kernel's sign-off word `arrived`
// or a staged get follows, which synchronises itself.
static int host_wait(const HostBufs &b, bool arrived, bool get_follows) {
  if (!arrived && (b.mapped || !get_follows)) HIPCHK(hipStreamSynchronize(nullptr));
  return SKYJO_OK;
}

// (host-style records are row-major whatever the layout option)
int skyjo_vec_step_host(skyjo_vec *h, const int32_t *actions_host, void *records_out_host) {
  if (!h || !actions_host) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  HostBufs b;
  int rc;
  if ((rc = host_bufs(h, &b)) || (rc = host_put(b, b.actions, actions_host, sizeof(int32_t) * (size_t)h->P.B))) return rc;
  // Mapped: actions read from / records and whole games written to host-mapped memory - one launch, one synchronisation.
  // A single tile is a single wavefront: it signs off with a sequence number in host-mapped memory as its very last
  // store, and the host spins on that word - a stream synchronisation costs ~10 us more than the kernel takes.  (The
  // stream stays ordered: whatever is launched next runs behind this kernel as usual.)
  const bool spin = b.mapped && h->P.tiles == 1 && h->host_spin;
  if (spin) h->host_seq = h->host_seq + 1 ? h->host_seq + 1 : 1;
  if ((rc = step_once(h, b.actions_d, b.records_d, nullptr, nullptr, nullptr, b.raw_d, false, spin ? h->host_seq : 0))) return rc;
  bool arrived = false;
  if (spin) {
    const volatile uint32_t *flag = h->health_host + 3;
    for (long k = 0; k < 4000000 && !(arrived = __atomic_load_n(flag, __ATOMIC_ACQUIRE) == h->host_seq); k++) __builtin_ia32_pause();
  }
  if ((rc = host_wait(b, arrived, records_out_host != nullptr))) return rc;  // (also the fallback when the word does not come: ~0.1 s of spinning)
  h->raw_valid = b.raw_d != nullptr;
  if (records_out_host && (rc = host_get(b, records_out_host, b.records, (size_t)h->P.B * h->P.L.rec_bytes))) return rc;
  return dev_error_check(h);
}

int skyjo_vec_observe_host(skyjo_vec *h, const int32_t *players_host, void *records_out_host) {
  if (!h || !records_out_host) return fail(SKYJO_E_INVALID, "null argument");
  GUARD(h);
  HostBufs b;  // (the games do not change: a valid host copy of them stays valid)
  int rc;
  if ((rc = host_bufs(h, &b)) || (players_host && (rc = host_put(b, b.actions, players_host, sizeof(int32_t) * (size_t)h->P.B)))) return rc;
  if ((rc = observe_impl(h, players_host ? b.actions_d : nullptr, b.records_d, nullptr, 0)) || (rc = host_wait(b, false, true))) return rc;
  if ((rc = host_get(b, records_out_host, b.records, (size_t)h->P.B * h->P.L.rec_bytes))) return rc;
  return dev_error_check(h);
}

int skyjo_vec_reset_host(skyjo_vec *h, const uint8_t *mask_host, void *records_out_host) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  if (!h->seeded) return fail(SKYJO_E_STATE, "skyjo_vec_seed must be called first");
  HostBufs b;
  int rc;
  if ((rc = host_bufs(h, &b)) || (mask_host && (rc = host_put(b, b.mask, mask_host, (size_t)h->P.B)))) return rc;
  if ((rc = reset_impl(h, mask_host ? b.mask_d : nullptr, b.records_d, nullptr, b.raw_d)) || (rc = host_wait(b, false, records_out_host != nullptr))) return rc;
  h->raw_valid = b.raw_d != nullptr;
  if (records_out_host && (rc = host_get(b, records_out_host, b.records, (size_t)h->P.B * h->P.L.rec_bytes))) return rc;
  return dev_error_check(h);
}

int skyjo_vec_get_rewards_host(skyjo_vec *h, double *rewards_out, double *scores_out, uint8_t *done_out) {
  if (!h) return fail(SKYJO_E_INVALID, "null handle");
  GUARD(h);
  const size_t n = (size_t)h->P.B * h->P.L.N;
  if (h->raw_valid) {  // served from what the last *_host call brought back
    const size_t N = (size_t)h->P.L.N;
    for (int g = 0; g < h->P.B; g++) {
      const uint8_t *raw = h->hm_raw + (size_t)g * h->raw_stride + h->P.L.state_bytes;
      if (rewards_out) memcpy(rewards_out + g * N, raw, 8 * N);
      if (scores_out) memcpy(scores_out + g * N, raw + 8 * N, 8 * N);
      if (done_out) done_out[g] = raw[16 * N + 4];
    }
    return dev_error_check(h);
  }
  if (rewards_out) HIPCHK(hipMemcpy(rewards_out, h->P.rewards, n * sizeof(double), hipMemcpyDeviceToHost));
  if (scores_out) HIPCHK(hipMemcpy(scores_out, h->P.scores, n * sizeof(double), hipMemcpyDeviceToHost));
  if (done_out) HIPCHK(hipMemcpy(done_out, h->P.done, (size_t)h->P.B, hipMemcpyDeviceToHost));
  return dev_error_check(h);
}

int skyjo_dev_malloc(int device_id, size_t bytes, void **out) {
  if (!out) return fail(SKYJO_E_INVALID, "null argument");
  DevGuard guard_(device_id);
  HIPCHK(hipMalloc(out, bytes ? bytes : 1));
  return SKYJO_OK;
}
int skyjo_dev_free(void *p) {
  if (p) HIPCHK(hipFree(p));
  return SKYJO_OK;
}
// ---- the reference's scoring helpers for caller-supplied hands (host pointers; computed on the device) ----
namespace {
int score_device(int32_t device_id, int *ndev_out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SKYJO_E_NOGPU, "no HIP device visible: this library has no CPU fallback");
  if (device_id < 0 || device_id >= ndev) return fail(SKYJO_E_INVALID, "device_id out of range");
  *ndev_out = ndev;
  return SKYJO_OK;
}
}  // namespace

int skyjo_vec_evaluate_game(int32_t device_id, int32_t n, int32_t num_players, const int8_t *players_cards_host, const int32_t *player_won_id_host,
                        double score_penalty, double *scores_out_host) {
  if (!players_cards_host || !player_won_id_host || !scores_out_host || n < 0) return fail(SKYJO_E_INVALID, "skyjo_vec_evaluate_game: bad argument");
  if (num_players <= 0 || num_players > SKYJO_MAX_PLAYERS) return fail(SKYJO_E_INVALID, "skyjo_vec_evaluate_game: num_players must be 1..12");
  for (int32_t i = 0; i < n; i++)
    if (player_won_id_host[i] < 0 || player_won_id_host[i] >= num_players) return fail(SKYJO_E_INVALID, "skyjo_vec_evaluate_game: player_won_id out of range");
  int ndev, rc;
  if ((rc = score_device(device_id, &ndev))) return rc;
  if (n == 0) return SKYJO_OK;
  DevGuard guard_(device_id);
  const size_t cb = (size_t)n * num_players * 12, wb = (size_t)n * 4, sb = (size_t)n * num_players * 8;
  const size_t o_w = (cb + 255) & ~(size_t)255, o_s = o_w + ((wb + 255) & ~(size_t)255);
  DevBuf d;
  HIPCHK(hipMalloc(&d.p, o_s + sb));
  uint8_t *b = (uint8_t *)d.p;
  HIPCHK(hipMemcpy(b, players_cards_host, cb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b + o_w, player_won_id_host, wb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_evaluate_game, dim3((n + 63) / 64), dim3(64), 0, nullptr, (int)n, (int)num_players, (const int8_t *)b, (const int32_t *)(b + o_w),
                     score_penalty, (double *)(b + o_s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(scores_out_host, b + o_s, sb, hipMemcpyDeviceToHost));
  return SKYJO_OK;
}

int skyjo_vec_calc_final_rewards(int32_t device_id, int32_t n, int32_t num_players, const double *final_score_host, const int32_t *num_refunded_host,
                             double mean_reward, double reward_refunded, double *rewards_out_host) {
  if (!final_score_host || !num_refunded_host || !rewards_out_host || n < 0) return fail(SKYJO_E_INVALID, "skyjo_vec_calc_final_rewards: bad argument");
  if (num_players <= 0 || num_players > SKYJO_MAX_PLAYERS) return fail(SKYJO_E_INVALID, "skyjo_vec_calc_final_rewards: num_players must be 1..12");
  int ndev, rc;
  if ((rc = score_device(device_id, &ndev))) return rc;
  if (n == 0) return SKYJO_OK;
  DevGuard guard_(device_id);
  const size_t sb = (size_t)n * num_players * 8, fb = (size_t)n * num_players * 4;
  const size_t o_f = (sb + 255) & ~(size_t)255, o_r = o_f + ((fb + 255) & ~(size_t)255);
  DevBuf d;
  HIPCHK(hipMalloc(&d.p, o_r + sb));
  uint8_t *b = (uint8_t *)d.p;
  HIPCHK(hipMemcpy(b, final_score_host, sb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b + o_f, num_refunded_host, fb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_final_rewards, dim3((n + 63) / 64), dim3(64), 0, nullptr, (int)n, (int)num_players, (const double *)b, (const int32_t *)(b + o_f),
                     mean_reward, reward_refunded, (double *)(b + o_r));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(rewards_out_host, b + o_r, sb, hipMemcpyDeviceToHost));
  return SKYJO_OK;
}

int skyjo_dev_copy(void *dst, const void *src, size_t bytes, int kind, void *stream) {
  hipMemcpyKind k = kind == 1 ? hipMemcpyHostToDevice : kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
  if (kind == 2) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SKYJO_OK;
}
int skyjo_dev_sync(void *stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return SKYJO_OK;
}

}  // extern "C"
