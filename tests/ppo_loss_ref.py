"""``skyjo_vec_ppo_loss`` (include/skyjo_vec.h) restated in numpy float64 for the tests - shares no code with the kernel:
the loss, its six statistics and both gradients, the latter derived by hand (tests/test_ppo_loss_ref.py checks them against torch's
autograd on the expression of ``examples/ppo.py``).  Not collected: a helper."""
import numpy as np

STATS = ("loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_fraction")


def ppo_loss(logits, log_mask, value, actions, logp_old, adv, vt, v_old, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None):
    """All inputs as numpy arrays ([m, 26] / [m]); every value is widened to float64 first.  Returns a dict: ``stats`` float64 [6] in
    the order of ``STATS``, ``grad_logits`` [m, 26], ``grad_value`` [m], and per row ``clipped`` (bool), ``p``, ``logp``, ``ratio``,
    ``saturated`` (the value clamp is active), ``clipped_count`` (int)."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    logits, log_mask, v, logp_old, A, vt, v_old = (f(x) for x in (logits, log_mask, value, logp_old, adv, vt, v_old))
    v = v.reshape(-1)
    m = logits.shape[0]
    rows = np.arange(m)
    a = np.asarray(actions, dtype=np.int64)
    z = logits + log_mask
    M = z.max(axis=1, keepdims=True)
    e = np.exp(z - M)
    S = e.sum(axis=1, keepdims=True)
    logp = z - M - np.log(S)
    p = e / S
    lp = logp[rows, a]
    r = np.exp(lp - logp_old)
    lo, hi = 1.0 - clip, 1.0 + clip
    pl = -np.minimum(r * A, np.clip(r, lo, hi) * A)
    plogp = np.where(p > 0, p * np.where(p > 0, logp, 0.0), 0.0)
    H = -plogp.sum(axis=1)
    vl1 = (v - vt) ** 2
    d = 2.0 * (v - vt)
    saturated = np.zeros(m, dtype=bool)
    if vf_clip is not None and np.isfinite(vf_clip) and vf_clip > 0:
        vc = v_old + np.clip(v - v_old, -vf_clip, vf_clip)
        vl2 = (vc - vt) ** 2
        saturated = np.abs(v - v_old) > vf_clip
        d = np.where(saturated & ~(vl1 >= vl2), 0.0, d)
        vl = np.maximum(vl1, vl2)
    else:
        vl = vl1
    kl = logp_old - lp
    clipped = ((A > 0) & (r > hi)) | ((A < 0) & (r < lo))
    g = np.where(clipped, 0.0, A)
    delta = np.zeros_like(p)
    delta[rows, a] = 1.0
    ent_term = np.where(p > 0, p * (np.where(p > 0, logp, 0.0) + H[:, None]), 0.0)
    grad_logits = (-(g * r)[:, None] * (delta - p) + ent_coef * ent_term) / m
    grad_value = vf_coef * d / m
    row_loss = pl + vf_coef * vl - ent_coef * H
    stats = np.array([row_loss.mean(), pl.mean(), vl.mean(), H.mean(), kl.mean(), clipped.sum() / m], dtype=np.float64)
    return {"stats": stats, "grad_logits": grad_logits, "grad_value": grad_value, "clipped": clipped, "clipped_count": int(clipped.sum()),
            "p": p, "logp": logp, "ratio": r, "saturated": saturated}
