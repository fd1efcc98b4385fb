// skyjo_deal_schedule.h - the dealing schedule of the engine's host side (skyjo_capi.hip, "the dealing schedule") in plain C++: its
// state and the arithmetic that sizes a step launch.  No HIP, no handle: tests/launch_plan_check.cpp includes this file alone.
#pragma once
#include <stdint.h>

// The dealing run that has been started and not yet published.
enum class InFlight {
  None,
  ListRun,  // a work-list run on deal_stream: k_publish makes its episodes available
  Planned,  // a run the step kernel planned, waiting for the k_cycle launch that carries it (inflight_tag: its id)
  Dealing   // a planned run that is being dealt or has been: the next step kernel publishes it, or k_publish_all
};

// The schedule's host state.  A new field goes into DealState when an engine that is snapshotted, run on and restored must meet it
// again as it was: a snapshot holds the struct as one value, so it is then saved and restored without another line.  It goes into
// DealSchedule itself when it follows from the engine's form and options, which a restore keeps as they are (interval_default), or
// describes a run in flight or a launch count, which the drain in front of every snapshot and restore settles (inflight,
// inflight_tag, cycle_seq).
struct DealState {
  int pending_iters = 0;      // lockstep iterations since the dealing kernel last ran
  int deal_every_iters = 64;  // ... between two runs (the form's default, SKYJO_OPT_DEAL_INTERVAL, adapt_interval)
  // The interval adapts itself unless it was set explicitly: every dealing run reports how many banks it found empty
  // (host-mapped word, no synchronisation); any empty bank shortens the interval, a long calm stretch lengthens it
  // back towards the default.  Results never depend on the cadence (tests/test_gpu_parity.py), only the speed does.
  bool auto_interval = true;
  int calm_runs = 0;
  uint32_t health_seen = 0;
  int list_sel = 0;       // the work list of the latest run (the two alternate)
  uint32_t deal_tag = 0;  // id of the latest dealing run (SkParams.deal_tag is its copy for the kernels)
};
struct DealSchedule {
  DealState st;
  int interval_default = 64;
  InFlight inflight = InFlight::None;
  uint32_t inflight_tag = 0;
  uint32_t cycle_seq = 0;  // k_cycle launches so far: launch L counts empty banks into bank_empty[L & 1] and reports the other word
};

constexpr int kMaxRolloutChunk = 128;  // lockstep iterations per k_step launch (the tile stays in LDS for a whole launch)

struct LaunchPlan {
  int iters;   // lockstep iterations of the launch: 1 .. wanted
  int cycles;  // whole dealing cycles in it (> 1: a k_cycle launch whose cycle ends are handled by the kernel)
  bool due;    // a dealing run is due when the launch is through
};
// One step launch as the schedule planned it: its size and, where the form plans ahead and a run is due after it, the id of the run
// the launch plans on its way out (of the first one, when the launch spans several cycles).
struct StepLaunch : LaunchPlan {
  uint32_t plan_tag;  // 0: the launch plans nothing
};

// `wanted`: iterations the caller still asks for (>= 1); `pending`: iterations since the last run; `every`: the dealing interval;
// `multi_cycle`: the launch may span several cycles (the one-kernel form of the fused rollout, planning ahead); `cycle_cap`: at most
// that many.  A launch ends where the next run is due, so the cadence does not depend on how the caller slices its calls; an
// interval that was shortened below `pending` makes the run due after one more iteration.
constexpr LaunchPlan plan_launch(int wanted, int pending, int every, bool multi_cycle, int cycle_cap) {
  int n = wanted < kMaxRolloutChunk ? wanted : kMaxRolloutChunk;
  const int left = every - pending;
  if (n > left) n = left > 0 ? left : 1;
  const bool due = pending + n >= every;
  int cycles = 1;
  // several cycles only from a cycle's start, and only where the launch ends on a run that is due
  if (multi_cycle && due && pending == 0) {
    cycles = wanted / every;
    cycles = cycles < 1 ? 1 : (cycles > cycle_cap ? cycle_cap : cycles);
    n = cycles * every;
  }
  return {n, cycles, due};
}
