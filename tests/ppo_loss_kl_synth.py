"""Seeded inputs for the PPO loss head with the KL penalty (``skyjo_vec_ppo_loss_kl``): the minibatches of tests/ppo_loss_synth.py
plus ``old_logits`` - the behaviour policy's logits - related to the row's ``logits`` in the ways an update meets and in the ways only
a synthetic row reaches.  Not collected: a helper of tests/test_ppo_loss_kl_ref.py and tests/test_gpu_ppo_loss_kl.py.

The old row of row i by ``OLD_KINDS[i % 8]`` (the row's own kind is ``ppo_loss_synth.KINDS[i % 8]``, so the pairs are fixed):
``identical`` - bit for bit the new logits (the first minibatch of an update: one-legal rows at i % 8 == 0, multi-legal at 5);
``near`` / ``far`` - the new logits plus N(0, 0.05) / N(0, 0.5); ``redraw`` - independent logits of the row's kind; ``extreme`` - the
rows with logits in +-80, by (i // 8) % 3: an independent redraw; an old distribution DOMINANT on the legal action the new one
likes least (where the gap is wide enough, new p < 1e-30 there, and 0 in float32 from a gap of 104); the new logits with the new
favourite 400 lower (po underflows to 0 where new p is the largest).  The last two need two legal actions, or stay identical."""
from collections import namedtuple

import numpy as np

from tests import ppo_loss_kl_ref as klref
from tests import ppo_loss_synth as synth

K = synth.K
ROW_COUNTS, COEFFS = synth.ROW_COUNTS, synth.COEFFS
KL_COEFFS = (0.0, 0.2, 1.0)
OLD_KINDS = ("identical", "near", "far", "extreme", "redraw", "identical", "near", "far")

KLBatch = namedtuple("KLBatch", synth.Batch._fields + ("old_logits",))


def make(m):
    """``ppo_loss_synth.make(m)`` - the same bits - and ``old_logits`` float32 [m, 26]."""
    b = synth.make(m)
    rng = np.random.default_rng(77000 + m)
    old = b.logits.copy()
    legal = b.log_mask == 0
    for i in range(m):
        kind = OLD_KINDS[i % 8]
        if kind == "near":
            old[i] = (b.logits[i].astype(np.float64) + rng.normal(0.0, 0.05, K)).astype(np.float32)
        elif kind == "far":
            old[i] = (b.logits[i].astype(np.float64) + rng.normal(0.0, 0.5, K)).astype(np.float32)
        elif kind == "redraw":
            old[i] = rng.normal(0.0, 2.0, K).astype(np.float32)
        elif kind == "extreme":
            sub = (i // 8) % 3
            z = np.where(legal[i], b.logits[i].astype(np.float64), np.nan)
            if sub == 0:
                old[i] = rng.uniform(-80.0, 80.0, K).astype(np.float32)
            elif legal[i].sum() >= 2 and sub == 1:
                row = rng.normal(0.0, 1.0, K)
                row[int(np.nanargmin(z))] += 30.0
                old[i] = row.astype(np.float32)
            elif legal[i].sum() >= 2:
                old[i, int(np.nanargmax(z))] -= np.float32(400.0)
    return KLBatch(*b, old)


def reference(b, ent_coef, vf_clip, kl_coeff, clip=synth.CLIP, vf_coef=1.0):
    return klref.ppo_loss_kl(b.logits, b.log_mask, b.old_logits, b.value, b.actions, b.logp, b.advantages, b.value_targets, b.values,
                             kl_coeff=kl_coeff, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip)


def branches(b):
    """Which of the listed situations the batch contains: a dict of booleans."""
    m = len(b.actions)
    out = reference(b, 0.0, None, 0.2)
    legal = b.log_mask == 0
    n_legal = legal.sum(axis=1)
    multi = n_legal > 1
    same = (b.old_logits == b.logits).all(axis=1)
    delta = np.abs(b.old_logits.astype(np.float64) - b.logits.astype(np.float64)).max(axis=1)
    kind = np.array(OLD_KINDS)[np.arange(m) % 8]
    p, po = out["p"], out["po"]
    z = b.logits.astype(np.float64) + b.log_mask.astype(np.float64)
    gap = z - z.max(axis=1, keepdims=True)                       # new p is 0 in float32 below about -104
    zo = b.old_logits.astype(np.float64) + b.log_mask.astype(np.float64)
    gapo = zo - zo.max(axis=1, keepdims=True)
    return {"one_legal": bool((n_legal == 1).any()), "large_logits": bool((np.abs(b.logits).max(axis=1) > 70).any()),
            "identical_one_legal": bool((same & ~multi).any()), "identical_multi_legal": bool((same & multi).any()),
            "near": bool(((kind == "near") & (delta > 0) & (delta < 0.3)).any()), "far": bool(((kind == "far") & (delta > 0.3)).any()),
            "redraw": bool(((kind == "redraw") & (delta > 1.0)).any()), "redraw_large": bool(((kind == "extreme") & (np.abs(b.old_logits).max(axis=1) > 70) & ~same).any()),
            "new_tiny_where_old_dominant": bool((multi[:, None] & legal & (p < 1e-30) & (po > 0.5)).any()),
            "new_zero_in_float32_where_old_positive": bool((legal & (gap < -110.0) & (po > 1e-30)).any()),
            "old_zero_in_float32_where_new_positive": bool((legal & (gapo < -110.0) & (p > 0.5)).any()),
            "action_kl_zero": bool((out["akl"] == 0.0).any()), "action_kl_above_10": bool((out["akl"] > 10.0).any())}


def torch_head_kl(logits, log_mask, old_logits, value, actions, logp_old, adv, vt, v_old, kl_coeff, clip=synth.CLIP, vf_coef=1.0, ent_coef=0.0,
                  vf_clip=None):
    """``ppo_loss_synth.torch_head`` plus ``kl_coeff * KL(pi_old || pi_new)`` over the masked distributions, as torch expressions in the
    dtype of the arguments.  Returns (loss, stats): the seven statistics as detached scalars."""
    import torch

    loss, stats = synth.torch_head(logits, log_mask, value, actions, logp_old, adv, vt, v_old, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef,
                                   vf_clip=vf_clip)
    logp_all = torch.log_softmax(logits + log_mask, -1)
    logpo = torch.log_softmax(old_logits + log_mask, -1)
    po = torch.softmax(old_logits + log_mask, -1)
    akl = torch.where(po > 0, po * (logpo - logp_all), torch.zeros_like(po)).sum(-1).mean()
    loss = loss + kl_coeff * akl
    return loss, [loss.detach()] + stats[1:] + [akl.detach()]


def torch_head_on(b, dtype, ent_coef, vf_clip, kl_coeff, device="cpu"):
    """``torch_head_kl`` on a ``KLBatch`` with ``logits`` and ``value`` as leaves: (stats as floats, grad_logits, grad_value) as numpy."""
    import torch

    t = lambda x: torch.from_numpy(x).to(device=device, dtype=dtype)
    logits, value = t(b.logits).requires_grad_(), t(b.value).requires_grad_()
    loss, stats = torch_head_kl(logits, t(b.log_mask), t(b.old_logits), value, torch.from_numpy(b.actions).to(device), t(b.logp),
                                t(b.advantages), t(b.value_targets), t(b.values), kl_coeff, ent_coef=ent_coef, vf_clip=vf_clip)
    loss.backward()
    return [float(s) for s in stats], logits.grad.double().cpu().numpy(), value.grad.double().cpu().numpy()


TOL_KEYS = synth.TOL_KEYS + ("action_kl",)


def float32_deviation():
    """``ppo_loss_synth.float32_deviation`` for this head: the largest absolute deviation of ``torch_head_kl`` in float32 on the CPU
    from the float64 restatement, per output - ``action_kl`` among them, the gradient including the penalty's - over every
    (row count, coefficients, kl_coeff) case of the GPU test."""
    import torch

    dev = dict.fromkeys(TOL_KEYS, 0.0)
    for m in ROW_COUNTS:
        b = make(m)
        for ent_coef, vf_clip in COEFFS:
            for kl_coeff in KL_COEFFS:
                want = reference(b, ent_coef, vf_clip, kl_coeff)
                stats, gl, gv = torch_head_on(b, torch.float32, ent_coef, vf_clip, kl_coeff)
                dl, dv = float(np.abs(gl - want["grad_logits"]).max()), float(np.abs(gv - want["grad_value"]).max())
                for k, x in (("grad_logits", dl), ("grad_logits_times_m", dl * m), ("grad_value", dv), ("grad_value_times_m", dv * m)):
                    dev[k] = max(dev[k], x)
                for k, s, w in zip(klref.STATS, stats, want["stats"]):
                    dev[k] = max(dev[k], abs(s - float(w)))
    return dev
