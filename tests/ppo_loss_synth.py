"""Seeded inputs for the PPO loss head (``skyjo_vec_ppo_loss``): minibatches whose rows reach every branch of the definition, drawn so
that a float32 and a float64 evaluation cannot disagree about a branch - a row that comes too close to one is drawn again.  Not
collected: a helper of tests/test_ppo_loss_ref.py and tests/test_gpu_ppo_loss.py."""
from collections import namedtuple

import numpy as np

from tests import ppo_loss_ref as ref

FLT_MAX = np.float32(np.finfo(np.float32).max)
K = 26
CLIP, VF_CLIP = 0.3, 0.2                      # the bounds the rows are placed around
COEFFS = [(0.0, None), (0.0, VF_CLIP), (0.01, None), (0.01, VF_CLIP)]   # (ent_coef, vf_clip) of every test
ROW_COUNTS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097]  # 127 .. 129: the kernel's rows per workgroup -1, +0, +1
KINDS = ("one_legal", "all_legal", "dominant", "large", "random", "random", "random", "random")  # the kind of row i is KINDS[i % 8]
MARGIN = 1e-3

Batch = namedtuple("Batch", ["logits", "log_mask", "value", "actions", "logp", "advantages", "value_targets", "values", "draws", "dropped"])


def seed_of(m):
    return 1000 + m


def _policy_rows(rng, idx):
    """logits, log_mask, actions of the rows ``idx`` (their kinds by idx % 8)."""
    n = idx.size
    kind = np.array(KINDS)[idx % len(KINDS)]
    logits = rng.normal(0.0, 2.0, (n, K))
    legal = rng.random((n, K)) < 0.4
    big = kind == "large"
    logits[big] = rng.uniform(-80.0, 80.0, (int(big.sum()), K))   # an un-subtracted softmax would overflow
    legal[kind == "all_legal"] = True
    first = rng.integers(0, K, n)
    legal[np.arange(n), first] = True                                # at least one legal action
    only = kind == "one_legal"
    legal[only] = False
    legal[only, first[only]] = True
    # the action: a legal one, uniformly
    score = np.where(legal, rng.random((n, K)), -1.0)
    actions = score.argmax(axis=1)
    dom = kind == "dominant"
    logits[dom] = rng.normal(0.0, 1.0, (int(dom.sum()), K))
    logits[dom, actions[dom]] += 30.0                                # every other action has p < 1e-10
    log_mask = np.where(legal, np.float32(0.0), -FLT_MAX).astype(np.float32)
    return logits.astype(np.float32), log_mask, actions.astype(np.int64)


def make(m, seed=None, clip=CLIP, vf_clip=VF_CLIP):
    """A ``Batch`` of m rows as float32 / int64 numpy arrays (the columns of ``rollout.Minibatch`` plus ``logits`` and ``value``);
    ``draws`` / ``dropped``: how many rows were drawn and how many of those draws were thrown away."""
    rng = np.random.default_rng(seed_of(m) if seed is None else seed)
    logits, log_mask, actions = _policy_rows(rng, np.arange(m))
    z = logits.astype(np.float64) + log_mask.astype(np.float64)
    zz = z - z.max(axis=1, keepdims=True)
    lp = (zz - np.log(np.exp(zz).sum(axis=1, keepdims=True)))[np.arange(m), actions]
    logp_old, adv, value, v_old, vt = (np.zeros(m, dtype=np.float32) for _ in range(5))
    todo = np.arange(m)
    draws = dropped = 0
    while todo.size:
        n = todo.size
        draws += n
        logp_old[todo] = (lp[todo] - rng.uniform(-0.7, 0.7, n)).astype(np.float32)   # r in [0.5, 2.0]: both sides of both bounds
        a = rng.normal(0.0, 1.0, n)
        a[todo % 5 == 0] = 0.0                                                          # an advantage of exactly 0
        adv[todo] = a.astype(np.float32)
        v_old[todo] = rng.normal(0.0, 1.0, n).astype(np.float32)
        # v - v_old on both sides of +-vf_clip, and not at it
        mag = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.75 * vf_clip, n), rng.uniform(1.25 * vf_clip, 2.5 * vf_clip, n))
        value[todo] = (v_old[todo].astype(np.float64) + mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        vt[todo] = rng.normal(0.0, 1.5, n).astype(np.float32)
        # the conditions, in float64 on the float32 values the kernel will see
        d = lambda x: x[todo].astype(np.float64)
        r = np.exp(lp[todo] - d(logp_old))
        dv = d(value) - d(v_old)
        vc = d(v_old) + np.clip(dv, -vf_clip, vf_clip)
        vl1, vl2 = (d(value) - d(vt)) ** 2, (vc - d(vt)) ** 2
        bad = np.abs(lp[todo] - d(logp_old)) > 10.0
        bad |= (np.abs(r - (1.0 - clip)) < MARGIN) | (np.abs(r - (1.0 + clip)) < MARGIN)
        bad |= (np.abs(dv) > vf_clip) & (np.abs(vl1 - vl2) < MARGIN * np.maximum(1.0, vl1))
        bad |= np.abs(np.abs(dv) - vf_clip) < MARGIN
        dropped += int(bad.sum())
        todo = todo[bad]
    return Batch(logits, log_mask, value, actions, logp_old, adv, vt, v_old, draws, dropped)


def reference(b, ent_coef, vf_clip, clip=CLIP, vf_coef=1.0):
    return ref.ppo_loss(b.logits, b.log_mask, b.value, b.actions, b.logp, b.advantages, b.value_targets, b.values, clip=clip,
                        vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip)


def branches(b, clip=CLIP, vf_clip=VF_CLIP):
    """Which of the listed situations the batch contains: a dict of booleans."""
    out = reference(b, 0.0, vf_clip, clip)
    legal = (b.log_mask == 0).sum(axis=1)
    p_a = out["p"][np.arange(len(b.actions)), b.actions]
    r, A, dv = out["ratio"], b.advantages, b.value.astype(np.float64) - b.values.astype(np.float64)
    return {"one_legal": bool((legal == 1).any()), "all_legal": bool((legal == K).any()),
            "dominant": bool(((legal > 1) & (1.0 - p_a < 1e-9)).any()), "large_logits": bool((np.abs(b.logits).max(axis=1) > 70).any()),
            "adv_pos": bool((A > 0).any()), "adv_neg": bool((A < 0).any()), "adv_zero": bool((A == 0).any()),
            "r_below": bool((r < 1 - clip).any()), "r_inside": bool(((r > 1 - clip) & (r < 1 + clip)).any()), "r_above": bool((r > 1 + clip).any()),
            "clipped_pos": bool(((A > 0) & (r > 1 + clip)).any()), "clipped_neg": bool(((A < 0) & (r < 1 - clip)).any()),
            "dv_below": bool((dv < -vf_clip).any()), "dv_inside": bool((np.abs(dv) < vf_clip).any()), "dv_above": bool((dv > vf_clip).any())}


def torch_head(logits, log_mask, value, actions, logp_old, adv, vt, v_old, clip=CLIP, vf_coef=1.0, ent_coef=0.0, vf_clip=None):
    """The loss head as torch expressions, in the dtype and on the device of its arguments: literally the lines of
    ``examples/ppo.py::_torch_loss`` - extended by ``- ent_coef * entropy`` and the value-clip ``max``.  Returns
    (loss, stats): stats = [loss, policy_loss, vf_loss, entropy, kl, clip_fraction] as detached scalars."""
    import torch

    z = logits + log_mask  # action_mask_model.py:70-71
    logp_all = torch.log_softmax(z, -1)
    logp = logp_all.gather(1, actions.unsqueeze(1)).squeeze(1)
    ratio = torch.exp(logp - logp_old)
    pl = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    vl_rows = (value - vt) ** 2
    if vf_clip is not None:
        vc = v_old + torch.clamp(value - v_old, -vf_clip, vf_clip)
        vl_rows = torch.max(vl_rows, (vc - vt) ** 2)
    vl = vl_rows.mean()
    p = torch.softmax(z, -1)
    entropy = -torch.where(p > 0, p * logp_all, torch.zeros_like(p)).sum(-1).mean()
    loss = pl + vf_coef * vl
    if ent_coef != 0.0:
        loss = loss - ent_coef * entropy
    with torch.no_grad():
        kl = (logp_old - logp).mean()
        cf = (((adv > 0) & (ratio > 1 + clip)) | ((adv < 0) & (ratio < 1 - clip))).to(logits.dtype).mean()
    return loss, [x.detach() for x in (loss, pl, vl, entropy, kl, cf)]


def torch_head_on(b, dtype, ent_coef, vf_clip, device="cpu"):
    """``torch_head`` on a ``Batch`` with ``logits`` and ``value`` as leaves: (stats list of floats, grad_logits, grad_value) as numpy."""
    import torch

    t = lambda x: torch.from_numpy(x).to(device=device, dtype=dtype)
    logits, value = t(b.logits).requires_grad_(), t(b.value).requires_grad_()
    loss, stats = torch_head(logits, t(b.log_mask), value, torch.from_numpy(b.actions).to(device), t(b.logp), t(b.advantages),
                             t(b.value_targets), t(b.values), ent_coef=ent_coef, vf_clip=vf_clip)
    loss.backward()
    return [float(s) for s in stats], logits.grad.double().cpu().numpy(), value.grad.double().cpu().numpy()


TOL_KEYS = ("grad_logits", "grad_logits_times_m", "grad_value", "grad_value_times_m") + ref.STATS


def float32_deviation():
    """The largest absolute deviation of ``torch_head`` in float32 on the CPU from the float64 restatement, per output, over every
    (row count, coefficients) case of the GPU test: what a correct float32 evaluation of the definition may be off by.  The gradients
    carry the factor 1 / m, so they are recorded twice: as they are, and times m (a bound that m = 1 does not dominate)."""
    import torch

    dev = dict.fromkeys(TOL_KEYS, 0.0)
    for m in ROW_COUNTS:
        b = make(m)
        for ent_coef, vf_clip in COEFFS:
            want = reference(b, ent_coef, vf_clip)
            stats, gl, gv = torch_head_on(b, torch.float32, ent_coef, vf_clip)
            dl, dv = float(np.abs(gl - want["grad_logits"]).max()), float(np.abs(gv - want["grad_value"]).max())
            for k, x in (("grad_logits", dl), ("grad_logits_times_m", dl * m), ("grad_value", dv), ("grad_value_times_m", dv * m)):
                dev[k] = max(dev[k], x)
            for k, s, w in zip(ref.STATS, stats, want["stats"]):
                dev[k] = max(dev[k], abs(s - float(w)))
    return dev
