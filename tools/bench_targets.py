"""Learner targets on device against the Python loop they replace, at config 5's shape (65 536 x 4 players, T = 320), both record
layouts: ``rollout.compute_targets`` (skyjo_vec_rollout_targets, one kernel: advantages, value targets, returns, flags by per-seat
GAE) and ``examples.ppo.compute_returns`` (a torch loop over T: Monte-Carlo returns and a mask only - strictly less work) on the
same buffer.  Both are timed with HIP events around CALLS calls after a warm-up.  The roof fraction is the kernel's ALGORITHMIC bytes
- T B (2 meta + 1 end flag + 4 value read, 13 written) plus the reward rows of the episode ends - over the call time and the
HBM peak of 8 TB/s: a report, not a gate.
    python tools/bench_targets.py [B] [T] [calls] [json out]        (one JSON line; needs the GPU)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from examples.ppo import compute_returns  # noqa: E402
from skyjo_rl_amd import SkyjoVecEnv  # noqa: E402
from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet  # noqa: E402
from skyjo_rl_amd.rollout import RolloutBuffer, collect, compute_targets  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 320
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    N = 4
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_targets.py measures on the GPU: none found")
    out = {"config": f"{B} x {N} players, T = {T}", "calls": calls, "layouts": {}}
    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=31).cuda()
    for layout in ("row-major", "tile-planar-all"):
        env = SkyjoVecEnv(B, num_players=N)
        env.set_record_layout(layout)
        env.seed(None, 5)
        env.reset()
        pol, val = FusedNet(model.policy), FusedNet(model.value)
        buf = RolloutBuffer(env, T)
        collect(env, pol, val, buf, seed=1, first_ticket=0)
        ends = int(buf.episode_end.sum())
        alg = T * B * (2 + 1 + 4 + 13) + ends * N * 8
        # alternate the two sides (twice each) so that whatever else the host does meets both
        dev, loop = [], []
        for _ in range(2):
            dev.append(timed(lambda: compute_targets(buf, gamma=0.99, lam=0.95), calls, 3))
            loop.append(timed(lambda: compute_returns(buf), max(calls // 2, 10), 1))
        returns, mask = compute_returns(buf)
        same = bool(torch.equal((buf.target_flags & 2) != 0, mask)) and bool(torch.equal(buf.returns[mask], returns[mask]))
        d, p = min(dev), min(loop)
        out["layouts"][layout] = {
            "compute_targets_ms": dev, "compute_returns_loop_ms": loop, "speedup": p / d, "episode_ends": ends,
            "algorithmic_bytes": alg, "algorithmic_GBps": alg / (d * 1e-3) / 1e9, "hbm_roof_fraction": alg / (d * 1e-3) / HBM_PEAK,
            "returns_and_mask_agree": same}
        pol.close(), val.close(), env.close()
        del buf
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")
    ok = all(v["speedup"] > 1 and v["returns_and_mask_agree"] for v in out["layouts"].values())
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
