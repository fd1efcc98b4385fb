"""The branches' training forward and backward on device against the torch autograd they replace, at the example's minibatch
(m = 32 768 rows) and the default model (31-256-256-26 policy, 31-256-256-1 value): ``learner.NativeBranch``
(skyjo_vec_mlp_train_forward / _backward: float32 matrix-instruction kernels on the master parameters) and ``model.policy(x)`` /
``model.value(x)`` with ``torch.autograd.backward``, on the same seeded inputs in the same run.  Two measurements, the two sides
alternating block by block, ROUNDS blocks of CALLS calls each after a warm-up, every block timed by a pair of device events:
  pair   forward and backward of both branches, ``grad_out`` fixed
  step   one whole minibatch step: the branches, ``ppo_loss``, ``NativeAdam.step()`` - ``ppo_update(native_nets=True)``'s loop body
         against ``ppo_update(native_loss=True)``'s (learning rate 0: the parameters stay where they are)
The native time over the torch time is the reported ratio (< 1: the kernels are faster) - a report, whichever way it comes out.  The
gradients of both sides are compared first.  ``--obs-dim D`` (default 31: everything as above) measures a model of D inputs instead,
up to the direct observation's 163, on integer-valued x of that width: ``learner.native_branch`` picks ``NativeBranch`` or, from 32
inputs, ``NativeWideBranch`` (skyjo_vec_mlp_train_wide_*).
    python tools/bench_train.py [--obs-dim D] [m] [calls] [rounds] [json out]   (one JSON line; needs the GPU; default out: profiles/train_bench.json)"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet  # noqa: E402
from skyjo_rl_amd.learner import NativeAdam, PPOLossBuffers, native_branch, ppo_loss  # noqa: E402
from tools.bench_loss import CLIP, OBS_DIM, VF_COEF, inputs  # noqa: E402


def timed(fn, calls):
    """Milliseconds per call of `calls` calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def alternate(sides, calls, rounds, warmup=10):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timed(fn, calls))
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_max": max(v)} for k, v in ms.items()}


def main():
    argv, obs_dim = list(sys.argv), OBS_DIM
    if "--obs-dim" in argv:
        at = argv.index("--obs-dim")
        obs_dim = int(argv[at + 1])
        del argv[at:at + 2]
    m = int(argv[1]) if len(argv) > 1 else 32768
    calls = int(argv[2]) if len(argv) > 2 else 50
    rounds = int(argv[3]) if len(argv) > 3 else 9
    out_path = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "train_bench.json")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_train.py measures on the GPU: none found")
    dev = torch.device("cuda", 0)
    _, _, mb = inputs(m, dev)
    if obs_dim != OBS_DIM:  # the same kind of observation - the values of its bytes, -2 .. 12 - at the other width
        wide = torch.floor(torch.rand((m, obs_dim), device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 15 - 2)
        mb = mb._replace(observations=wide)
    x = mb.observations
    gen = torch.Generator(device=dev).manual_seed(1)
    g_logits = torch.randn((m, 26), device=dev, generator=gen) / m
    g_value = torch.randn((m, 1), device=dev, generator=gen) / m

    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=obs_dim).to(dev)
    params = list(model.policy.parameters()) + list(model.value.parameters())
    bp, bv = native_branch(model.policy, m), native_branch(model.value, m)

    def pair_torch():
        for p in params:
            p.grad = None
        torch.autograd.backward([model.policy(x), model.value(x)], [g_logits, g_value])

    def pair_native():
        bp.forward(x), bv.forward(x)
        bp.backward(g_logits), bv.backward(g_value)

    # both sides compute the same thing on these inputs
    pair_torch()
    want = [p.grad.clone() for p in params]
    pair_native()
    agree = max(float((p.grad - w).abs().max() / w.abs().max()) for p, w in zip(params, want))

    pair = alternate({"torch": pair_torch, "native": pair_native}, calls, rounds)

    pol, val = FusedNet(model.policy), FusedNet(model.value)
    opt = NativeAdam(model, pol, val, lr=0.0)
    out = PPOLossBuffers(m, dev)
    tot = torch.zeros((6,), dtype=torch.float64, device=dev)

    def step_native_loss():
        logits, value = model.policy(x), model.value(x)
        r = ppo_loss(logits, value, mb, clip=CLIP, vf_coef=VF_COEF, out=out)
        opt.zero_grad(set_to_none=True)
        torch.autograd.backward([logits, value], [r.grad_logits, r.grad_value])
        opt.step()
        tot.add_(r.stats * m)

    def step_native_nets():
        logits, value = bp.forward(x), bv.forward(x)
        r = ppo_loss(logits, value, mb, clip=CLIP, vf_coef=VF_COEF, out=out)
        bp.backward(r.grad_logits), bv.backward(r.grad_value)
        opt.step()
        tot.add_(r.stats * m)

    step = alternate({"native_loss": step_native_loss, "native_nets": step_native_nets}, calls, rounds)
    pol.close(), val.close()

    # what the native pair moves through memory per row and branch, counted: h1, h2, dz2, dz1 written once (4 x 1 KB); h1 and h2 read
    # by the row pass and again by the weight pass, dz2 and dz1 read by the weight pass (6 x 1 KB; the weight pass's four slices of a
    # chunk share h1 through the cache); x read by the forward and the weight pass, out written, grad_out read by both backward passes
    bytes_per_row = lambda D, O: 4 * (10 * 256 + 2 * D + 3 * O)
    result = {"m": m, "calls": calls, "rounds": rounds, "model": f"{obs_dim}-256-256-26 + {obs_dim}-256-256-1",
              "timing": "a pair of device events around `calls` calls; sides alternate per block; min / median / max over `rounds` blocks",
              "agreement_max_normalised": agree, "pair": pair, "step": step,
              "counted_bytes_per_row": {"policy": bytes_per_row(obs_dim, 26), "value": bytes_per_row(obs_dim, 1)},
              "counted_mb_per_pair": (bytes_per_row(obs_dim, 26) + bytes_per_row(obs_dim, 1)) * m / 1e6,
              "pair_native_over_torch": pair["native"]["ms_median"] / pair["torch"]["ms_median"],
              "step_native_nets_over_native_loss": step["native_nets"]["ms_median"] / step["native_loss"]["ms_median"]}
    line = json.dumps(result)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
