"""The PPO loss head on device against the torch expressions it replaces, at the example's minibatch (m = 32 768 rows, 26 actions):
``learner.ppo_loss`` (skyjo_vec_ppo_loss: one fused kernel and a single-workgroup reduction - loss, statistics and both gradients)
and the lines of ``examples/ppo.py::_torch_loss`` (mask, log_softmax, gather, exp, clamp, min, means, autograd backwards, and
the three ``float(...)`` statistics reads per minibatch), on the same seeded inputs in the same run.  Two measurements, each side
alternating with the other, ROUNDS rounds of CALLS calls after a warm-up, timed by a host clock around work that ends in a device
synchronise (the torch side reads statistics back: that stall is part of what it costs):
  head   one forward and backward of the head alone, ``logits`` and ``value`` fixed leaves
  step   one whole minibatch step: the model's two branches forwards, the head, backwards through the branches, Adam
The native time over the torch time is the reported ratio (< 1: the kernel is faster) - a report, whichever way it comes out.  The
outputs of both heads are compared first.
    python tools/bench_loss.py [m] [calls] [rounds] [json out]        (one JSON line; needs the GPU)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from skyjo_rl_amd.action_mask_model import FLOAT_MIN, ActionMaskModel  # noqa: E402
from skyjo_rl_amd.learner import PPOLossBuffers, ppo_loss  # noqa: E402
from skyjo_rl_amd.rollout import Minibatch  # noqa: E402

CLIP, VF_COEF, OBS_DIM = 0.3, 1.0, 31


def inputs(m, dev, seed=0):
    """A seeded minibatch the shape ``rollout.minibatches`` delivers: two fifths of the actions legal, the chosen one among them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(s, device=dev, generator=g)
    n = lambda *s: torch.randn(s, device=dev, generator=g)
    obs = torch.floor(r(m, OBS_DIM) * 15 - 2)
    legal = r(m, 26) < 0.4
    actions = torch.where(legal, r(m, 26), r(m, 26) - 2).argmax(1)
    legal[torch.arange(m, device=dev), actions] = True
    log_mask = torch.where(legal, 0.0, FLOAT_MIN).to(torch.float32)
    logits = 2 * n(m, 26)
    lp = torch.log_softmax(logits + log_mask, -1).gather(1, actions.unsqueeze(1)).squeeze(1)
    values = n(m)
    mb = Minibatch(obs, log_mask, actions, lp - (r(m) - 0.5), n(m), values + 1.5 * n(m), values, None)
    return logits, values + 0.3 * n(m), mb


def torch_head(logits_raw, value, mb):
    """``examples/ppo.py::_torch_loss``'s lines between the model's outputs and ``loss.backward()``: (loss, pl, vl, logp)."""
    logits = logits_raw + mb.log_mask
    logp = torch.log_softmax(logits, -1).gather(1, mb.actions.unsqueeze(1)).squeeze(1)
    ratio = torch.exp(logp - mb.logp)
    pl = -torch.min(ratio * mb.advantages, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * mb.advantages).mean()
    vl = ((value - mb.value_targets) ** 2).mean()
    return pl + VF_COEF * vl, pl, vl, logp


def torch_reads(mb, pl, vl, logp, n):
    """... and its three statistics reads."""
    return float(pl.detach()) * n, float(vl.detach()) * n, float((mb.logp - logp).mean().detach()) * n


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def alternate(sides, calls, rounds, warmup=10):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, calls))
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_max": max(v)} for k, v in ms.items()}


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_loss.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    logits0, value0, mb = inputs(m, dev)
    out = PPOLossBuffers(m, dev)

    # both heads compute the same thing on these inputs
    lg, v = logits0.clone().requires_grad_(), value0.clone().requires_grad_()
    loss, pl, vl, logp = torch_head(lg, v, mb)
    loss.backward()
    res = ppo_loss(logits0, value0, mb, clip=CLIP, vf_coef=VF_COEF, out=out)
    agree = {"loss": abs(float(res.stats[0]) - float(loss.detach())), "grad_logits_times_m": float((res.grad_logits - lg.grad).abs().max()) * m,
             "grad_value_times_m": float((res.grad_value - v.grad).abs().max()) * m}

    def head_torch(reads=True):
        lg.grad = v.grad = None
        loss, pl, vl, logp = torch_head(lg, v, mb)
        loss.backward()
        if reads:
            torch_reads(mb, pl, vl, logp, m)

    head = alternate({"torch": head_torch, "torch_without_reads": lambda: head_torch(False),
                      "native": lambda: ppo_loss(logits0, value0, mb, clip=CLIP, vf_coef=VF_COEF, out=out)}, calls, rounds)

    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=OBS_DIM).to(dev)
    state = {k: t.clone() for k, t in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    tot = torch.zeros((6,), dtype=torch.float64, device=dev)

    def step_torch():
        loss, pl, vl, logp = torch_head(model.policy(mb.observations), model.value(mb.observations).squeeze(-1), mb)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        torch_reads(mb, pl, vl, logp, m)

    def step_native():
        logits, value = model.policy(mb.observations), model.value(mb.observations)
        r = ppo_loss(logits, value, mb, clip=CLIP, vf_coef=VF_COEF, out=out)
        opt.zero_grad(set_to_none=True)
        torch.autograd.backward([logits, value], [r.grad_logits, r.grad_value])
        opt.step()
        tot.add_(r.stats * m)

    step = alternate({"torch": step_torch, "native": step_native}, max(calls // 2, 20), rounds)
    model.load_state_dict(state)

    ratio = lambda d, a, b: d[a]["ms_median"] / d[b]["ms_median"]
    result = {"m": m, "calls": calls, "rounds": rounds, "clip": CLIP, "vf_coef": VF_COEF, "model": f"{OBS_DIM}-256-256-26 + {OBS_DIM}-256-256-1, Adam",
              "timing": "host clock around `calls` calls ending in a device synchronise; sides alternate per round; min / median / max over rounds",
              "agreement_abs": agree, "head": head, "step": step,
              "head_native_over_torch": ratio(head, "native", "torch"),
              "head_native_over_torch_without_reads": ratio(head, "native", "torch_without_reads"),
              "step_native_over_torch": ratio(step, "native", "torch")}
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
