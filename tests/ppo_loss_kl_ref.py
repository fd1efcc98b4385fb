"""``skyjo_vec_ppo_loss_kl`` (include/skyjo_vec.h) restated in numpy float64 for the tests - shares no code with the
kernel: the head of tests/ppo_loss_ref.py plus the KL penalty against the behaviour distribution, its statistic ``action_kl`` and its
hand-derived gradient ``kl_coeff (p - po) / m`` (tests/test_ppo_loss_kl_ref.py checks it against torch's autograd).  Not collected:
a helper."""
import numpy as np

from tests import ppo_loss_ref as ref

STATS = ref.STATS + ("action_kl",)


def old_distribution(old_logits, log_mask):
    """(po, logpo) of the masked behaviour distribution, float64 [m, 26]."""
    zo = np.asarray(old_logits, dtype=np.float64) + np.asarray(log_mask, dtype=np.float64)
    zo = zo - zo.max(axis=1, keepdims=True)
    eo = np.exp(zo)
    So = eo.sum(axis=1, keepdims=True)
    return eo / So, zo - np.log(So)


def ppo_loss_kl(logits, log_mask, old_logits, value, actions, logp_old, adv, vt, v_old, kl_coeff=0.2, clip=0.3, vf_coef=1.0, ent_coef=0.0,
                vf_clip=None):
    """The dict of ``ppo_loss_ref.ppo_loss`` with ``stats`` float64 [7] in the order of ``STATS`` (the loss includes the penalty),
    ``grad_logits`` including its gradient, and per row ``akl``, ``po``, ``logpo``; ``grad_logits_base`` / ``kl_grad``: the two parts."""
    out = ref.ppo_loss(logits, log_mask, value, actions, logp_old, adv, vt, v_old, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip)
    m = out["p"].shape[0]
    po, logpo = old_distribution(old_logits, log_mask)
    pos = po > 0
    akl = np.where(pos, po * (np.where(pos, logpo, 0.0) - np.where(pos, out["logp"], 0.0)), 0.0).sum(axis=1)
    kl_grad = kl_coeff * (out["p"] - po) / m
    stats = np.concatenate([out["stats"], [akl.mean()]])
    stats[0] += kl_coeff * akl.mean()
    out.update(stats=stats, grad_logits_base=out["grad_logits"], kl_grad=kl_grad, grad_logits=out["grad_logits"] + kl_grad, akl=akl, po=po,
               logpo=logpo)
    return out
