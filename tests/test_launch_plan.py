"""The launch planning of the engine's host side (skyjo_rl_amd/csrc/skyjo_deal_schedule.h: how many lockstep iterations and dealing
cycles the next step launch takes, and whether a dealing run is due after it) as a pure function, on the CPU.

tests/launch_plan_check.cpp includes that header alone and is built with AddressSanitizer + UBSan, as `make -C oracle check-asan`
builds the oracle.  It runs 5 000 iterations, cut into calls of 1 .. 300 iterations by a fixed-seed generator (30 cuts per case), over
every = 1, 8, 40, 64, 128, 129, 1000; cycle cap = 1, 4, 16; multi-cycle launches on and off; starting pending = 0, 5, every - 1 and
every + 3 (an interval that was shortened below what is pending), and checks for every launch

* 1 <= iters <= what the call still wants, and iters <= 128 unless cycles > 1;
* cycles > 1 only with multi-cycle on, from pending == 0, with iters == cycles * every and cycles <= cap;
* a single-cycle launch never passes a due point: pending + iters <= max(every, pending + 1);

and for every cut that the global iteration numbers at which runs fall due are max(every - pending0, 1) and then every `every`
iterations: the cadence does not depend on how the caller slices its calls."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_under_address_and_ub_sanitizer(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "the check is built with g++ (the oracle's compiler family)"
    exe = str(tmp_path / "launch_plan_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "launch_plan_check.cpp")], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("LAUNCH-PLAN-OK "), (out.stdout[-2000:], out.stderr[-3000:])
    assert "AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
    assert int(out.stdout.split()[1]) > 100000  # (every case ran: 7 x 3 x 2 x 4 x 30 cuts of 5 000 iterations)
