"""Learner minibatches on device against the torch expressions they replace (``examples/ppo.py::ppo_update``, default path), at config
5's shape (65 536 x 4 players, T = 320), both record layouts.  Three timings per layout, each with HIP events around CALLS calls after
a warm-up, the two sides alternated twice, the faster round of each side counted:
  select   ``rollout.select_rows``  against  ``mask.reshape(-1).nonzero()`` + ``adv[idx].mean()`` + ``adv[idx].std()`` (with the read-back
           of the moments that normalising by them as Python floats needs; the torch side's nonzero synchronises by itself)
  gather   ``rollout.gather_rows`` of one 32 768-row minibatch into a reused ``Minibatch``  against  the torch expressions of the
           update loop for the same rows and the same eight outputs, on views made beforehand
  epoch    one epoch of ``rollout.minibatches``  against  the torch path: views, selection, moments, permutation and the gathers; for a
           tile-planar buffer the views are the row-major copy of the whole record block (``buf.views()``), made once per update
The roof fraction is the gather's ALGORITHMIC bytes per row - rec_bytes + 8 + 20 read, 4 D + 104 + 8 + 17 written - over its time and
the HBM peak of 8 TB/s: a report, not a gate.  Exit status 0: the native side is no slower in all six timings and the outputs agree.
    python tools/bench_batches.py [B] [T] [calls] [json out]        (one JSON line; needs the GPU)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from skyjo_rl_amd import SkyjoVecEnv  # noqa: E402
from skyjo_rl_amd._lib import TGT_HAS_TARGET  # noqa: E402
from skyjo_rl_amd.action_mask_model import FLOAT_MIN, ActionMaskModel, FusedNet  # noqa: E402
from skyjo_rl_amd.rollout import (RolloutBuffer, collect, compute_targets, gather_rows, minibatches, new_minibatch,  # noqa: E402
                                  select_rows)

HBM_PEAK = 8.0e12  # bytes / s (MI355X data sheet)
MINIBATCH = 1 << 15


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


def torch_select(buf):
    mask = (buf.target_flags & TGT_HAS_TARGET) != 0
    idx = mask.reshape(-1).nonzero().squeeze(1)
    adv_all = buf.advantages.reshape(-1)
    mean, std = adv_all[idx].mean(), adv_all[idx].std().clamp_min(1e-6)
    return idx, float(mean), float(std)


def torch_columns(buf):
    """The flat views the update loop indexes (for a tile-planar buffer this makes the row-major copy)."""
    v, T = buf.views(), buf.T
    return (v.observations[:T].reshape(-1, v.observations.shape[-1]), v.action_mask[:T].reshape(-1, 26), buf.actions.reshape(-1).long(),
            buf.logp.reshape(-1), buf.values[:T].reshape(-1), buf.value_targets.reshape(-1), buf.advantages.reshape(-1),
            v.agent[:T].reshape(-1))


def torch_gather(cols, j, mean, std):
    obs, am, act, logp_old, val_old, ret, adv_all, agent = cols
    return (obs[j].to(torch.float32), torch.clamp(torch.log(am[j].to(torch.float32)), min=FLOAT_MIN), act[j], logp_old[j],
            (adv_all[j] - mean) / std, ret[j], val_old[j], agent[j])


def torch_epoch(buf, gen):
    cols = torch_columns(buf)
    idx, mean, std = torch_select(buf)
    perm = idx[torch.randperm(idx.numel(), device=idx.device, generator=gen)]
    for k in range(0, perm.numel(), MINIBATCH):
        torch_gather(cols, perm[k:k + MINIBATCH], mean, std)


def native_epoch(buf, gen):
    for _ in minibatches(buf, MINIBATCH, generator=gen, normalize=True):
        pass


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 320
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    N = 4
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_batches.py measures on the GPU: none found")
    out = {"config": f"{B} x {N} players, T = {T}, minibatch {MINIBATCH}", "calls": calls, "layouts": {}}
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
        compute_targets(buf, gamma=0.99, lam=0.95)
        gen = torch.Generator(device=buf.actions.device).manual_seed(0)

        sel = select_rows(buf)
        idx, mean, std = torch_select(buf)
        same = bool(torch.equal(sel.index, idx)) and abs(sel.mean - mean) <= 1e-5 * abs(mean) and abs(sel.std - std) <= 1e-5 * abs(std)
        rows = sel.index[torch.randperm(sel.count, device=idx.device, generator=gen)[:MINIBATCH]].contiguous()
        mb = new_minibatch(buf, rows.numel())
        cols = torch_columns(buf)
        norm = (sel.mean, max(sel.std, 1e-6))
        got, want = gather_rows(buf, rows, normalize=norm, out=mb), torch_gather(cols, rows, norm[0], norm[1])
        same = same and all(bool(torch.equal(a, b)) for a, b in zip(got[:4] + got[5:], want[:4] + want[5:]))
        same = same and bool(torch.allclose(got.advantages, want[4], rtol=1e-6, atol=1e-7))  # (torch divides by a double scalar)

        t = {k: {"native_ms": [], "torch_ms": []} for k in ("select", "gather", "epoch")}
        for _ in range(2):  # alternate the two sides so that whatever else the host does meets both
            t["select"]["native_ms"].append(timed(lambda: select_rows(buf), calls, 2))
            t["select"]["torch_ms"].append(timed(lambda: torch_select(buf), calls, 2))
            t["gather"]["native_ms"].append(timed(lambda: gather_rows(buf, rows, normalize=norm, out=mb), calls * 10, 5))
            t["gather"]["torch_ms"].append(timed(lambda: torch_gather(cols, rows, norm[0], norm[1]), calls * 10, 5))
            del cols  # (the epoch's torch side makes its own views: for a tile-planar buffer the copy is part of what it costs)
            t["epoch"]["native_ms"].append(timed(lambda: native_epoch(buf, gen), max(calls // 5, 2), 1))
            t["epoch"]["torch_ms"].append(timed(lambda: torch_epoch(buf, gen), max(calls // 5, 2), 1))
            cols = torch_columns(buf)
        for v in t.values():
            v["speedup"] = min(v["torch_ms"]) / min(v["native_ms"])
        rb, D = env.record_bytes, env.obs_dim
        per_row = (rb + 8 + 20) + (4 * D + 104 + 8 + 17)
        g = min(t["gather"]["native_ms"]) * 1e-3
        out["layouts"][layout] = dict(t, selected_rows=sel.count, rows=T * B, gather_rows=int(rows.numel()), algorithmic_bytes_per_row=per_row,
                                      gather_algorithmic_GBps=per_row * rows.numel() / g / 1e9,
                                      gather_hbm_roof_fraction=per_row * rows.numel() / g / HBM_PEAK, outputs_agree=same)
        pol.close(), val.close(), env.close()
        del buf, cols, mb
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 4:
        with open(sys.argv[4], "w") as f:
            f.write(line + "\n")
    ok = all(v["outputs_agree"] and all(v[k]["speedup"] >= 1 for k in ("select", "gather", "epoch")) for v in out["layouts"].values())
    raise SystemExit(0 if ok else 1)


if __name__ == "__main__":
    main()
