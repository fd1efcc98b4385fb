"""Config 5 on the reference's own default, the direct observation (19 + 12 N features: 67 at four players), next to the two things it can
be compared with, in one process on one GPU:
  wide    - rollout.collect with packed nets of env.obs_dim inputs (k_net_bf16_wide / k_net_split_wide): policy + value branch and the masked
            draw in one launch, two launches per lockstep iteration;
  torch   - the same engine driven step by step by the torch module and sample_actions_fused (the policy's three GEMMs in torch, the draw
            in one HIP pass, env.step): all a direct-observation user had before the packed nets took more than 31 inputs.  float32 only
            (no value branch, no rollout columns: it does LESS than the other two);
  narrow  - config 5 as bench.py measures it, on the indirect observation (31 features).
The median of ``rounds`` rounds of T lockstep iterations each, after two warm-up rounds; the wall clock around a synchronised round.
    python tools/bench_wide.py [B] [T] [rounds] [players]        (one JSON line)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench

B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
T = int(sys.argv[2]) if len(sys.argv) > 2 else 64
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 8
N = int(sys.argv[4]) if len(sys.argv) > 4 else 4


def wide_collect(precision):
    import torch
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(0)
    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=False, **bench.ENV_CFG)
    env.seed(None, 3)
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = FusedNet(model.policy, precision=precision), FusedNet(model.value, precision=precision)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=9, first_ticket=0)
    collect(env, pol, val, buf, seed=9, first_ticket=T, first_records=buf.records[T].clone())
    rounds = []
    for r in range(ROUNDS):
        first = buf.records[T].clone()
        torch.cuda.synchronize()
        env.reset_counters()
        t0 = time.perf_counter()
        collect(env, pol, val, buf, seed=9, first_ticket=(2 + r) * T, first_records=first)
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0, env.counters()))
    rounds.sort(key=lambda x: x[0])
    dt, c = rounds[len(rounds) // 2]
    env.profile(1)
    collect(env, pol, val, buf, seed=9, first_ticket=(2 + ROUNDS) * T, first_records=buf.records[T].clone())
    prof = env.profile(0)
    out = {"obs_dim": env.obs_dim, "record_bytes": env.record_bytes, "value": c["steps"] / dt, "unit": "env-steps/s", "ms_per_iteration": 1e3 * dt / T,
           "net_kernel_ms": prof["k_mlp_ms"] / max(prof["k_mlp_launches"], 1), "step_kernel_ms": prof["step_ms"] / max(prof["step_launches"], 1),
           "illegal": int(c["illegal"]), "round_ms": [1e3 * x[0] for x in rounds]}
    pol.close(), val.close(), env.close()
    return out


def torch_stepwise():
    import torch
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, sample_actions_fused

    torch.manual_seed(0)
    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=False, **bench.ENV_CFG)
    env.seed(None, 3)
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    rec = env.observe()
    ticket = 0

    def one_round():
        nonlocal rec, ticket
        with torch.no_grad():
            for _ in range(T):
                rec = env.step(sample_actions_fused(model, env, rec, seed=9, ticket=ticket), out=rec)
                ticket += 1

    one_round(), one_round()
    rounds = []
    for r in range(ROUNDS):
        torch.cuda.synchronize()
        env.reset_counters()
        t0 = time.perf_counter()
        one_round()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0, env.counters()))
    rounds.sort(key=lambda x: x[0])
    dt, c = rounds[len(rounds) // 2]
    out = {"obs_dim": env.obs_dim, "value": c["steps"] / dt, "unit": "env-steps/s", "ms_per_iteration": 1e3 * dt / T, "illegal": int(c["illegal"]),
           "round_ms": [1e3 * x[0] for x in rounds]}
    env.close()
    return out


out = {"config": f"{B} x {N} players, direct observation, action-mask model in the loop", "T": T, "rounds": ROUNDS}
for prec in ("fp32", "bf16"):
    out["wide_" + prec] = wide_collect(prec)
out["torch_fp32"] = torch_stepwise()
for prec in ("fp32", "bf16"):
    narrow = bench.side_model_config(prec, B, N, T, ROUNDS, 0)
    out["narrow_" + prec] = {k: narrow[k] for k in ("value", "unit", "ms_per_iteration", "dominant_kernel_ms", "step_kernel_ms", "round_ms")}
print(json.dumps(out))
