"""The learner's loss head on the GPU: ``ppo_loss`` takes the two outputs of ``ActionMaskModel``'s branches on a ``rollout.Minibatch``
and returns the PPO loss, its statistics and the gradients with respect to both outputs - ONE fused kernel plus a single-workgroup
reduction (``skyjo_vec_ppo_loss``, csrc/skyjo_loss.h) instead of the chain of small torch expressions and their autograd twins that
otherwise stands between the model and ``optimizer.step()``.  ``PPOLoss`` wraps it as a ``torch.autograd.Function``.

The definition (include/skyjo_vec.h has it in full): the masked softmax of ``action_mask_model.py:58-74`` - logits plus
the log-mask - the clipped surrogate, the squared value error and the entropy of the PPO the reference trains with
(``rlskyjo/models/train_model_simple_rllib.py:54-57``: RLlib's PPO, ``clip_param`` 0.3, ``vf_loss_coeff`` 1.0)::

    L = mean( -min(r A, clamp(r, 1 - clip, 1 + clip) A) + vf_coef vl - ent_coef H )

with ``r = exp(logp[action] - logp_old)``, ``vl = (v - vt)^2`` and ``H`` the entropy of the masked distribution.  ``vf_clip`` is
RLlib's ``vf_clip_param`` form: ``vl = max(vl, (vc - vt)^2)`` with ``vc = v_old + clamp(v - v_old, -vf_clip, vf_clip)``.  ray is not
installed where this package is developed: that form is restated from memory of RLlib's torch policy, not checked against it (as
``action_mask_model.py`` says of ``TorchFC``).  The gradients are the ones torch's autograd gives for the same expression; the
statistics are means over the rows, accumulated in double in a fixed order - the same input gives the same bits on every call.
"""
import math
from collections import namedtuple

import torch

from . import _lib

PPOLossResult = namedtuple("PPOLossResult", ["stats", "grad_logits", "grad_value"])
STATS = ("loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_fraction")  # the order of ``PPOLossResult.stats``
NUM_ACTIONS = 26


class PPOLossBuffers:
    """The outputs and the scratch of ``ppo_loss`` for up to ``rows`` rows, to pass as ``out=`` minibatch after minibatch."""

    def __init__(self, rows, device):
        if rows < 1:
            raise ValueError("rows must be at least 1")
        L = _lib.load()
        self.rows = int(rows)
        self.stats = torch.empty((6,), dtype=torch.float64, device=device)
        self.grad_logits = torch.empty((rows, NUM_ACTIONS), dtype=torch.float32, device=device)
        self.grad_value = torch.empty((rows,), dtype=torch.float32, device=device)
        self.scratch = torch.empty((int(L.skyjo_vec_ppo_loss_scratch_bytes(self.rows)) // 8,), dtype=torch.float64, device=device)


def _column(name, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {list(shape)} on {device}")
    return t


@torch.no_grad()
def ppo_loss(logits, value, mb, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None, out=None):
    """The loss head on the minibatch ``mb`` (a ``rollout.Minibatch``, or anything with its ``log_mask``, ``actions``, ``logp``,
    ``advantages``, ``value_targets`` and ``values``): ``logits`` float32 [m, 26] - the policy branch's raw output, the mask NOT yet
    added - and ``value`` float32 [m] or [m, 1], all contiguous on one GPU.  Returns ``PPOLossResult(stats, grad_logits, grad_value)``:
    ``stats`` float64 [6] on the device in the order of ``STATS`` (means over the m rows), ``grad_logits`` float32 [m, 26] and
    ``grad_value`` float32 of ``value``'s shape - the gradients of ``stats[0]``.  Nothing is read back: no host synchronisation.
    ``vf_clip``: None, <= 0 or inf - no value clipping.  ``out``: a ``PPOLossBuffers`` of at least m rows whose tensors (and scratch)
    are reused; the results are views of it, valid until the next call with the same ``out``.  ``mb.actions`` must lie in [0, 26) - a
    precondition, not checked (the kernel reads an action outside as 0)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != NUM_ACTIONS or logits.shape[0] < 1:
        raise ValueError("logits must be a float32 tensor of shape [m, 26], m >= 1")
    dev, m, f = logits.device, logits.shape[0], torch.float32
    if dev.type != "cuda":
        raise ValueError("ppo_loss runs on the GPU: logits is on " + str(dev))
    _column("logits", logits, f, (m, NUM_ACTIONS), dev)
    if not isinstance(value, torch.Tensor) or tuple(value.shape) not in ((m,), (m, 1)):
        raise ValueError(f"value must have shape [{m}] or [{m}, 1]")
    _column("value", value, f, tuple(value.shape), dev)
    _column("mb.log_mask", mb.log_mask, f, (m, NUM_ACTIONS), dev)
    _column("mb.actions", mb.actions, torch.int64, (m,), dev)
    for name in ("logp", "advantages", "value_targets", "values"):
        _column("mb." + name, getattr(mb, name), f, (m,), dev)
    clip = float(clip)
    if not (math.isfinite(clip) and clip > 0.0):
        raise ValueError("clip must be finite and greater than 0")
    vf_clip = 0.0 if vf_clip is None or not math.isfinite(float(vf_clip)) or float(vf_clip) <= 0.0 else float(vf_clip)
    if out is None:
        out = PPOLossBuffers(m, dev)
    elif not isinstance(out, PPOLossBuffers) or out.rows < m or out.stats.device != dev:
        raise ValueError("out must be a PPOLossBuffers of at least m rows on the inputs' device")
    grad_logits, grad_value = out.grad_logits[:m], out.grad_value[:m]
    if any(t.data_ptr() % 16 for t in (logits, mb.log_mask)):
        raise ValueError("logits and mb.log_mask must start on a 16-byte boundary (a slice that starts at an odd row does not)")
    L = _lib.load()
    vp = lambda t: t.data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(L.skyjo_vec_ppo_loss(vp(logits), vp(mb.log_mask), vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages),
                                        vp(mb.value_targets), vp(mb.values), m, clip, float(vf_coef), float(ent_coef), vf_clip,
                                        vp(grad_logits), vp(grad_value), vp(out.stats), vp(out.scratch), out.scratch.numel() * 8, stream))
    return PPOLossResult(out.stats, grad_logits, grad_value.view(value.shape))


class PPOLoss(torch.autograd.Function):
    """``loss, stats = PPOLoss.apply(logits, value, mb, clip, vf_coef, ent_coef, vf_clip)``: ``ppo_loss`` inside autograd.  ``loss``
    is ``stats[0]`` as a float32 scalar; ``stats`` (float64 [6]) is not differentiable.  Backward hands the gradients the kernel
    already computed, times the incoming gradient, to ``logits`` and ``value``."""

    @staticmethod
    def forward(ctx, logits, value, mb, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None):
        res = ppo_loss(logits.detach(), value.detach(), mb, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip)
        ctx.save_for_backward(res.grad_logits, res.grad_value)
        ctx.mark_non_differentiable(res.stats)
        return res.stats[0].to(torch.float32), res.stats

    @staticmethod
    def backward(ctx, grad_loss, _grad_stats):
        grad_logits, grad_value = ctx.saved_tensors
        return grad_logits * grad_loss, grad_value * grad_loss, None, None, None, None, None
