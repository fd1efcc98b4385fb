"""The learner's loss head on the GPU: ``ppo_loss`` takes the two outputs of ``ActionMaskModel``'s branches on a ``rollout.Minibatch``
and returns the PPO loss, its statistics and the gradients with respect to both outputs - ONE fused kernel plus a single-workgroup
reduction (``skyjo_vec_ppo_loss``, csrc/skyjo_loss.h) instead of the chain of small torch expressions and their autograd twins that
otherwise stands between the model and ``optimizer.step()``.  ``PPOLoss`` wraps it as a ``torch.autograd.Function``.  ``NativeAdam`` is the
step itself: Adam fused with the re-pack of the updated weights into the ``FusedNet``s' MFMA fragments, in place (``skyjo_vec_mlp_adam_step``,
csrc/skyjo_update.h) - the rollout that follows needs no new nets.

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
import ctypes as C
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


class NativeAdam:
    """``torch.optim.Adam`` (no amsgrad, no weight decay) for ``model``'s two branches, fused with the re-pack of their ``FusedNet``s:
    ``step()`` is one ``skyjo_vec_mlp_adam_step`` per branch - two kernel launches on torch's current stream, nothing else.  Each
    element's thread reads p, g, exp_avg, exp_avg_sq, applies the rule, writes the three back and packs the new p into the net's MFMA
    fragments in place: when ``step()`` returns, ``policy_net`` and ``value_net`` are queued to hold the updated weights - no
    ``repack``, no new handles, no host copy, no allocation, no synchronisation.  A rollout on the same stream sees them.

    Duck-typed to what ``examples/ppo.py:ppo_update`` calls on its ``optimizer`` (``zero_grad``, ``step``); not a
    ``torch.optim.Optimizer``.  ``lr`` is a plain attribute and may be set between steps.  ``lr``, ``betas`` and ``eps`` reach the
    kernel as float32 (the ABI's type): the bias corrections are computed from the float32 values of the betas.  ``state`` maps a
    parameter to its ``exp_avg`` / ``exp_avg_sq`` views, as ``torch.optim.Adam.state`` does."""

    def __init__(self, model, policy_net, value_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self._L = _lib.load()
        self.lr, self.betas, self.eps = lr, (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0
        self.state = {}
        self._branches = []
        for seq, net in ((model.policy, policy_net), (model.value, value_net)):
            params = net.branch_parameters(seq)
            dev = params[0].device
            n = int(self._L.skyjo_vec_mlp_adam_state_bytes(net._h)) // 4
            buf = torch.zeros((n,), dtype=torch.float32, device=dev)
            at = 0
            for p in params:
                self.state[p] = {"exp_avg": buf[at:at + p.numel()].view(p.shape), "exp_avg_sq": buf[n // 2 + at:n // 2 + at + p.numel()].view(p.shape)}
                at += p.numel()
            pp = (C.c_void_p * 6)(*[p.data_ptr() for p in params])
            self._branches.append((net, params, buf, pp))

    def zero_grad(self, set_to_none=True):
        for _, params, _, _ in self._branches:
            for p in params:
                if p.grad is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    @torch.no_grad()
    def step(self):
        calls = []
        for net, params, buf, pp in self._branches:  # every check before the first launch: both branches step, or neither
            if not net._h:
                raise ValueError("a FusedNet of this optimizer is closed")
            for p in params:
                if p.grad is None:
                    raise ValueError("a parameter has no gradient (.grad is None): NativeAdam steps every parameter of both branches")
                _column("a parameter's .grad", p.grad, torch.float32, tuple(p.shape), p.device)
            calls.append((net, buf, pp, (C.c_void_p * 6)(*[p.grad.data_ptr() for p in params])))
        for net, buf, pp, gg in calls:
            with torch.cuda.device(buf.device):
                _lib.check(self._L.skyjo_vec_mlp_adam_step(net._h, pp, gg, buf.data_ptr(), buf.numel() * 4, float(self.lr), self.betas[0],
                                                           self.betas[1], self.eps, self.steps + 1, torch.cuda.current_stream().cuda_stream))
        self.steps += 1
