// launch_plan_check.cpp - the launch planning of the engine's host side (skyjo_deal_schedule.h, which this program includes alone) over
// every interval, cycle cap, starting point and slicing of tests/test_launch_plan.py's docstring.  Built with
// -fsanitize=address,undefined and run by that test; prints "LAUNCH-PLAN-OK <launches>" or the first violation.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../skyjo_rl_amd/csrc/skyjo_deal_schedule.h"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;  // fixed seed: the slicings are the same in every run
static int draw(int lo, int hi) {               // xorshift64*, lo .. hi inclusive
  g_rng ^= g_rng >> 12, g_rng ^= g_rng << 25, g_rng ^= g_rng >> 27;
  return lo + (int)(((g_rng * 0x2545f4914f6cdd1dull) >> 33) % (uint64_t)(hi - lo + 1));
}

#define CHECK(cond)                                                                                                                      \
  do {                                                                                                                                   \
    if (!(cond)) {                                                                                                                       \
      printf("FAILED %s: every=%d cap=%d multi=%d pending0=%d cut=%d at=%d wanted=%d pending=%d -> iters=%d cycles=%d due=%d\n", #cond, \
             every, cap, (int)multi, pending0, cut, at, wanted, pending, L.iters, L.cycles, (int)L.due);                                \
      return 1;                                                                                                                          \
    }                                                                                                                                    \
  } while (0)

int main() {
  const int kTotal = 5000, kCuts = 30;
  const int everys[] = {1, 8, 40, 64, 128, 129, 1000}, caps[] = {1, 4, 16};
  long launches = 0;
  for (int every : everys)
    for (int cap : caps)
      for (int m = 0; m < 2; m++) {
        const bool multi = m != 0;
        const int starts[] = {0, 5, every - 1, every + 3};  // (the last: an interval that was shortened below what is pending)
        for (int pending0 : starts) {
          // the global iterations after which a run falls due, whatever the slicing
          std::vector<int> expect;
          for (int t = std::max(every - pending0, 1); t <= kTotal; t += every) expect.push_back(t);
          for (int cut = 0; cut < kCuts; cut++) {
            std::vector<int> got;
            int at = 0, pending = pending0;
            while (at < kTotal) {
              const int call = std::min(draw(1, 300), kTotal - at);
              for (int done = 0; done < call;) {
                const int wanted = call - done;
                const LaunchPlan L = plan_launch(wanted, pending, every, multi, cap);
                launches++;
                CHECK(L.iters >= 1 && L.iters <= wanted);
                CHECK(L.cycles >= 1);
                CHECK(L.iters <= 128 || L.cycles > 1);
                if (L.cycles > 1) {
                  CHECK(multi && pending == 0 && L.iters == L.cycles * every && L.cycles <= cap && L.due);
                  for (int c = 1; c < L.cycles; c++) got.push_back(at + c * every);  // (the cycle ends inside the launch)
                } else {
                  CHECK(pending + L.iters <= std::max(every, pending + 1));  // never past a due point
                }
                CHECK(L.due == (pending + L.iters >= every || L.cycles > 1));
                at += L.iters, done += L.iters;
                pending = L.due ? 0 : pending + L.iters;
                if (L.due) got.push_back(at);
              }
            }
            const LaunchPlan L{0, 0, false};  // (no launch at hand: CHECK prints one)
            const int wanted = 0;
            CHECK(at == kTotal);
            CHECK(got == expect);
          }
        }
      }
  printf("LAUNCH-PLAN-OK %ld\n", launches);
  return 0;
}
