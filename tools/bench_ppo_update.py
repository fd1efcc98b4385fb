"""One PPO update through the host loop against the same update behind one native call, on the example's model (31-256-256-26 policy and
31-256-256-1 value branch, float32-grade nets) and a 65 536 games x 4 players, T = 64 buffer of its own self-play:
  python  ``examples.ppo.ppo_update(native_batches=True, native_loss=True, native_nets=True, shuffle="torch")`` - the parent's path: per
          step about thirteen ctypes calls, per epoch a ``torch.randperm``, a fancy-index allocation and one read
  native  the same call with ``shuffle="native", native_update=True``: ``learner.NativeUpdate`` / ``skyjo_vec_ppo_update``, one read at the end
at minibatch 128 (RLlib's ``sgd_minibatch_size`` default), 1 024 and 32 768, ``EPOCHS`` epochs each, ``ent_coef`` 0.01, ``vf_clip`` 0.2 and
``grad_clip`` 0.5.  Each timed call starts from identical state - a deep copy of the model, fresh nets and a fresh ``NativeAdam``, made
outside the window - and is timed by a host clock around work that starts and ends in a device synchronise (targets, selection and the
reads are part of what either path costs).  The sides alternate, ROUNDS rounds after one warm-up call each per size; min / median / max
over the rounds.  Both sides use different shuffles, so their results differ; that the one call carries the host loop's bits from the
same shuffle is what tests/test_gpu_ppo_update_native.py holds, and is checked here once more at the largest minibatch.  The ratio is a
report, whichever way it comes out.
    python tools/bench_ppo_update.py [rounds] [epochs] [json out]        (one JSON line; needs the GPU)"""
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from examples.ppo import ppo_update  # noqa: E402
from skyjo_rl_amd import SkyjoVecEnv  # noqa: E402
from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet  # noqa: E402
from skyjo_rl_amd.learner import NativeAdam  # noqa: E402
from skyjo_rl_amd.rollout import RolloutBuffer, collect  # noqa: E402

GAMES, PLAYERS, T, LR = 65536, 4, 64, 3e-4
MINIBATCHES = (128, 1024, 32768)
COMMON = dict(gae=(0.99, 0.95), native_batches=True, native_loss=True, native_nets=True, seed=11, clip=0.3, vf_coef=1.0, ent_coef=0.01, vf_clip=0.2,
              grad_clip=0.5)
SIDES = {"python": dict(shuffle="torch"), "native": dict(shuffle="native", native_update=True)}


class Learner:
    def __init__(self, model):
        self.model = copy.deepcopy(model)
        self.pol, self.val = FusedNet(self.model.policy), FusedNet(self.model.value)
        self.opt = NativeAdam(self.model, self.pol, self.val, lr=LR)

    def close(self):
        self.pol.close(), self.val.close()


def timed(model, buf, minibatch, epochs, side):
    ln = Learner(model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ppo_update(ln.model, buf, ln.opt, epochs=epochs, minibatch=minibatch, **COMMON, **side)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    steps = ln.opt.steps
    ln.close()
    return ms, steps, out["transitions"]


def same_bits(model, buf, minibatch, epochs):
    """The host loop and the one call from the SAME (native) shuffle: do the parameters end with the same bytes?"""
    ends = []
    for native in (False, True):
        ln = Learner(model)
        ppo_update(ln.model, buf, ln.opt, epochs=epochs, minibatch=minibatch, shuffle="native", native_update=native, **COMMON)
        ends.append([p.detach().clone() for p in ln.model.parameters()])
        ln.close()
    return all(torch.equal(p, q) for p, q in zip(*ends))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ppo_update.py measures on the GPU: none found")
    torch.manual_seed(0)
    env = SkyjoVecEnv(GAMES, num_players=PLAYERS)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    pol.close(), val.close()
    result = {"games": GAMES, "players": PLAYERS, "T": T, "epochs": epochs, "rounds": rounds,
              "timing": "host clock around one ppo_update between two device synchronises, fresh learner per call; sides alternate per round; "
                        "min / median / max over rounds",
              "one_call_carries_the_loops_bits_at_32768": same_bits(model, buf, MINIBATCHES[-1], epochs), "minibatch": {}}
    for mb in MINIBATCHES:
        ms = {k: [] for k in SIDES}
        for k, side in SIDES.items():  # warm-up: every shape of the timed window
            timed(model, buf, mb, epochs, side)
        for _ in range(rounds):
            for k, side in SIDES.items():
                t, steps, rows = timed(model, buf, mb, epochs, side)
                ms[k].append(t)
                print("minibatch %d %s: %.1f ms, %d steps, %d rows" % (mb, k, t, steps, rows), file=sys.stderr, flush=True)
        entry = {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_max": max(v)} for k, v in ms.items()}
        entry.update(steps=steps, rows=rows, us_per_step={k: statistics.median(v) * 1e3 / steps for k, v in ms.items()},
                     native_over_python=statistics.median(ms["native"]) / statistics.median(ms["python"]))
        result["minibatch"][str(mb)] = entry
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
