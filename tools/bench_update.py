"""The learner step's way back to the matrix cores, in place against the path it replaces, on the example's model (31-256-256-26 policy and
31-256-256-1 value branch, float32-grade nets).  Per learner step, with gradients already in ``.grad``:
  parent  ``torch.optim.Adam.step()``, then ``close()`` of both nets and ``examples.ppo.repack(model)``: new nets through the host
  native  ``learner.NativeAdam.step()``: Adam and the re-pack of both branches in two launches (skyjo_vec_mlp_adam_step)
and the re-pack alone:
  create  ``FusedNet(seq)`` + ``close()``            update  ``FusedNet.update(seq)``
Each side alternates with the other, ROUNDS rounds of CALLS calls after a warm-up, timed by a host clock around work that starts and ends
in a device synchronise (the parent path has host time: the blocking reads are part of what it costs).  ``native`` and ``update`` are
also timed by device events around the same calls: what the GPU spends between the first launch and the last.  The ratios are a report,
whichever way they come out.  Both paths are first run from the same start and their nets compared.
    python tools/bench_update.py [calls] [rounds] [json out]        (one JSON line; needs the GPU)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from examples.ppo import repack  # noqa: E402
from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet  # noqa: E402
from skyjo_rl_amd.learner import NativeAdam  # noqa: E402

OBS_DIM, LR = 31, 3e-4


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def timed_events(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(sides, calls, rounds, clock=timed, warmup=10):
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(clock(fn, calls))
    return {k: {"ms_min": min(v), "ms_median": statistics.median(v), "ms_max": max(v)} for k, v in ms.items()}


def set_grads(model, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 1e-2


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_update.py measures on the GPU: none found")

    def fresh():
        torch.manual_seed(0)
        model = ActionMaskModel(obs_dim=OBS_DIM).cuda()
        set_grads(model, 1)
        return model

    # both paths end in the same nets: three steps each from the same start (float32 Adam in two operation orders: the parameters
    # agree to rounding, and each path's nets are the pack of its own parameters)
    ma, mb = fresh(), fresh()
    opt_a = torch.optim.Adam(ma.parameters(), lr=LR)
    nets_b = repack(mb)
    opt_b = NativeAdam(mb, nets_b[0], nets_b[1], lr=LR)
    for _ in range(3):
        opt_a.step()
        opt_b.step()
    nets_a, nets_b2 = repack(ma), repack(mb)
    agree = {"max_abs_parameter_difference": max(float((p - q).abs().max()) for p, q in zip(ma.parameters(), mb.parameters())),
             "native_nets_equal_repack_of_their_parameters": all(torch.equal(x.export(), y.export()) for x, y in zip(nets_b, nets_b2))}
    for n in (*nets_a, *nets_b2):
        n.close()

    state = {"nets": repack(ma)}

    def step_parent():
        opt_a.step()
        for n in state["nets"]:
            n.close()
        state["nets"] = repack(ma)

    step = alternate({"parent": step_parent, "native": opt_b.step}, calls, rounds)
    step_events = alternate({"native": opt_b.step}, calls, rounds, clock=timed_events)

    box = {"net": FusedNet(ma.policy)}

    def create():
        box["net"].close()
        box["net"] = FusedNet(ma.policy)

    pack = alternate({"create": create, "update": lambda: nets_b[0].update(mb.policy)}, calls, rounds)
    pack_events = alternate({"update": lambda: nets_b[0].update(mb.policy)}, calls, rounds, clock=timed_events)

    ratio = lambda d, a, b: d[a]["ms_median"] / d[b]["ms_median"]
    result = {"calls": calls, "rounds": rounds, "model": f"{OBS_DIM}-256-256-26 + {OBS_DIM}-256-256-1, float32-grade nets, Adam lr {LR}",
              "timing": "host clock around `calls` calls between two device synchronises; sides alternate per round; min / median / max over rounds; "
                        "*_events: device events around the same calls",
              "agreement": agree, "step": step, "step_native_events": step_events["native"], "pack": pack, "pack_update_events": pack_events["update"],
              "step_native_over_parent": ratio(step, "native", "parent"), "pack_update_over_create": ratio(pack, "update", "create")}
    line = json.dumps(result)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
