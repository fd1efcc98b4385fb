"""The learner's loss head on the GPU: ``ppo_loss`` takes the two outputs of ``ActionMaskModel``'s branches on a ``rollout.Minibatch``
and returns the PPO loss, its statistics and the gradients with respect to both outputs - ONE fused kernel plus a single-workgroup
reduction (``skyjo_vec_ppo_loss``, csrc/skyjo_loss.h) instead of the chain of small torch expressions and their autograd twins that
otherwise stands between the model and ``optimizer.step()``.  ``PPOLoss`` wraps it as a ``torch.autograd.Function``.  ``NativeAdam`` is the
step itself: Adam fused with the re-pack of the updated weights into the ``FusedNet``s' MFMA fragments, in place (``skyjo_vec_mlp_adam_step``,
csrc/skyjo_update.h) - the rollout that follows needs no new nets - and with ``max_grad_norm`` RLlib's ``grad_clip`` in front of it: ``grad_norm``
(``skyjo_vec_grad_norm``, csrc/skyjo_clip.h) takes the global norm of both branches' gradients and the step reads the coefficient from the
device.  ``NativeBranch`` is what remains in between: one branch's forward, which keeps its activations, and its backward on the float32 master parameters (``skyjo_vec_mlp_train_forward`` / ``_backward``,
csrc/skyjo_train.h: the exact float32 matrix instruction, no autograd graph, no allocation per step); ``NativeWideBranch`` is the same for the
direct observation's 32 to 163 inputs (``skyjo_vec_mlp_train_wide_*``, csrc/skyjo_train_wide.h), and ``native_branch`` picks between them.  ``NativeUpdate`` queues all of it - every epoch and every
minibatch step of an update, the shuffles and the epoch statistics included - behind ONE native call (``skyjo_vec_ppo_update``, csrc/skyjo_epoch.h).

The definition (include/skyjo_vec.h has it in full): the masked softmax of ``action_mask_model.py:58-74`` - logits plus
the log-mask - the clipped surrogate, the squared value error and the entropy of the PPO the reference trains with
(``rlskyjo/models/train_model_simple_rllib.py:54-57``: RLlib's PPO, ``clip_param`` 0.3, ``vf_loss_coeff`` 1.0)::

    L = mean( -min(r A, clamp(r, 1 - clip, 1 + clip) A) + vf_coef vl - ent_coef H )

with ``r = exp(logp[action] - logp_old)``, ``vl = (v - vt)^2`` and ``H`` the entropy of the masked distribution.  ``vf_clip`` is
RLlib's ``vf_clip_param`` form: ``vl = max(vl, (vc - vt)^2)`` with ``vc = v_old + clamp(v - v_old, -vf_clip, vf_clip)``.  ray is not
installed where this package is developed: that form is restated from memory of RLlib's torch policy, not checked against it (as
``action_mask_model.py`` says of ``TorchFC``).  The gradients are the ones torch's autograd gives for the same expression; a row is
evaluated in double from its float32 inputs and every output rounded once (the device's float32 ``logf`` is biased by -7e-08 on a
softmax's sum, which no mean over rows removes); the statistics are means over the rows, accumulated in double in a fixed order - the
same input gives the same bits on every call.

``ppo_loss_kl`` (``skyjo_vec_ppo_loss_kl``) is the same head with the term RLlib's DEFAULT PPO loss carries besides - the reference leaves
``ppo.DEFAULT_CONFIG`` as it is, ``kl_coeff`` 0.2 and ``kl_target`` 0.01 with it::

    L = mean( surrogate + kl_coeff KL(pi_old(.|s) || pi_new(.|s)) + vf_coef vl - ent_coef H )

over the WHOLE masked distributions - which needs the behaviour policy's logits per row (``rollout.behaviour_logits``, gathered by
``rollout.minibatches(behaviour=True)``), not the ``logp`` of the chosen action the ``kl`` statistic above is estimated from.  Its seventh
statistic ``action_kl`` is the mean of that divergence; ``KLCoeff`` adapts the coefficient from it after an update: times 1.5 above
``2 kl_target``, times 0.5 below ``0.5 kl_target``.  The term and the rule are, like ``vf_clip``, restated from memory of RLlib 1.9.
"""
import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib

PPOLossResult = namedtuple("PPOLossResult", ["stats", "grad_logits", "grad_value"])
STATS = ("loss", "policy_loss", "vf_loss", "entropy", "kl", "clip_fraction")  # the order of ``PPOLossResult.stats``
STATS_KL = STATS + ("action_kl",)  # ... of ``ppo_loss_kl``'s
NUM_ACTIONS = 26
HIDDEN = 256
TRAIN_TILE_ROWS = 64     # SKT_TILE_ROWS of csrc/skyjo_train.h: the rows of a workgroup in the forward and the backward's row pass
TRAIN_CHUNK_ROWS = 256   # SKT_CHUNK_ROWS: the rows of one partial of the weight gradients - the longest chain over rows


class PPOLossBuffers:
    """The outputs and the scratch of ``ppo_loss`` for up to ``rows`` rows, to pass as ``out=`` minibatch after minibatch."""

    _num_stats, _scratch_bytes = 6, "skyjo_vec_ppo_loss_scratch_bytes"

    def __init__(self, rows, device):
        if rows < 1:
            raise ValueError("rows must be at least 1")
        L = _lib.load()
        self.rows = int(rows)
        self.stats = torch.empty((self._num_stats,), dtype=torch.float64, device=device)
        self.grad_logits = torch.empty((rows, NUM_ACTIONS), dtype=torch.float32, device=device)
        self.grad_value = torch.empty((rows,), dtype=torch.float32, device=device)
        self.scratch = torch.empty((int(getattr(L, self._scratch_bytes)(self.rows)) // 8,), dtype=torch.float64, device=device)


class PPOLossKLBuffers(PPOLossBuffers):
    """``PPOLossBuffers`` for ``ppo_loss_kl``: seven statistics, and the scratch of ``skyjo_vec_ppo_loss_kl_scratch_bytes``."""

    _num_stats, _scratch_bytes = 7, "skyjo_vec_ppo_loss_kl_scratch_bytes"


def _column(name, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {list(shape)} on {device}")
    return t


def _ppo_loss(who, cls, logits, value, mb, old_logits, kl_coeff, clip, vf_coef, ent_coef, vf_clip, out):
    """``ppo_loss`` (``cls`` is ``PPOLossBuffers``) and ``ppo_loss_kl`` (``PPOLossKLBuffers``: ``old_logits`` and ``kl_coeff`` count) under
    the name ``who``: the checks, the buffers and the native call."""
    kl = cls is PPOLossKLBuffers
    if not isinstance(logits, torch.Tensor) or logits.dim() != 2 or logits.shape[1] != NUM_ACTIONS or logits.shape[0] < 1:
        raise ValueError("logits must be a float32 tensor of shape [m, 26], m >= 1")
    dev, m, f = logits.device, logits.shape[0], torch.float32
    if dev.type != "cuda":
        raise ValueError(who + " runs on the GPU: logits is on " + str(dev))
    _column("logits", logits, f, (m, NUM_ACTIONS), dev)
    if not isinstance(value, torch.Tensor) or tuple(value.shape) not in ((m,), (m, 1)):
        raise ValueError(f"value must have shape [{m}] or [{m}, 1]")
    _column("value", value, f, tuple(value.shape), dev)
    if kl:
        _column("old_logits", old_logits, f, (m, NUM_ACTIONS), dev)
    _column("mb.log_mask", mb.log_mask, f, (m, NUM_ACTIONS), dev)
    _column("mb.actions", mb.actions, torch.int64, (m,), dev)
    for name in ("logp", "advantages", "value_targets", "values"):
        _column("mb." + name, getattr(mb, name), f, (m,), dev)
    clip, kl_coeff = float(clip), float(kl_coeff) if kl else None
    if not (math.isfinite(clip) and clip > 0.0):
        raise ValueError("clip must be finite and greater than 0")
    if kl and not (math.isfinite(kl_coeff) and kl_coeff >= 0.0):
        raise ValueError("kl_coeff must be finite and not negative")
    vf_clip = 0.0 if vf_clip is None or not math.isfinite(float(vf_clip)) or float(vf_clip) <= 0.0 else float(vf_clip)
    if out is None:
        out = cls(m, dev)
    elif not isinstance(out, cls) or out.rows < m or out.stats.device != dev:
        raise ValueError(f"out must be a {cls.__name__} of at least m rows on the inputs' device")
    grad_logits, grad_value = out.grad_logits[:m], out.grad_value[:m]
    if any(t.data_ptr() % 16 for t in ((logits, mb.log_mask, old_logits) if kl else (logits, mb.log_mask))):
        raise ValueError(("logits, mb.log_mask and old_logits" if kl else "logits and mb.log_mask")
                         + " must start on a 16-byte boundary (a slice that starts at an odd row does not)")
    L = _lib.load()
    vp = lambda t: t.data_ptr()
    rows = (vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages), vp(mb.value_targets), vp(mb.values), m, clip, float(vf_coef),
            float(ent_coef), vf_clip)
    with torch.cuda.device(dev):
        outs = (vp(grad_logits), vp(grad_value), vp(out.stats), vp(out.scratch), out.scratch.numel() * 8, torch.cuda.current_stream(dev).cuda_stream)
        if kl:
            _lib.check(L.skyjo_vec_ppo_loss_kl(vp(logits), vp(mb.log_mask), vp(old_logits), *rows, kl_coeff, *outs))
        else:
            _lib.check(L.skyjo_vec_ppo_loss(vp(logits), vp(mb.log_mask), *rows, *outs))
    return PPOLossResult(out.stats, grad_logits, grad_value.view(value.shape))


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
    return _ppo_loss("ppo_loss", PPOLossBuffers, logits, value, mb, None, None, clip, vf_coef, ent_coef, vf_clip, out)


@torch.no_grad()
def ppo_loss_kl(logits, value, mb, old_logits, kl_coeff=0.2, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None, out=None):
    """``ppo_loss`` with the KL penalty against the behaviour distribution (``skyjo_vec_ppo_loss_kl``): ``old_logits`` float32 [m, 26],
    contiguous on the inputs' GPU and starting on a 16-byte boundary - the raw logits of the policy that played, for the rows of ``mb``
    (the second element of what ``rollout.minibatches(behaviour=True)`` yields) - and ``kl_coeff``, finite and >= 0 (RLlib's default
    0.2; ``float(KLCoeff)`` works).  Returns ``PPOLossResult`` with ``stats`` float64 [7] in the order of ``STATS_KL``: the loss includes
    ``kl_coeff * action_kl``, the gradient ``kl_coeff (p - p_old) / m``; ``action_kl`` is computed also when ``kl_coeff`` is 0, where
    everything else carries the bits of ``ppo_loss``.  ``out``: a ``PPOLossKLBuffers``.  Everything else as for ``ppo_loss``."""
    return _ppo_loss("ppo_loss_kl", PPOLossKLBuffers, logits, value, mb, old_logits, kl_coeff, clip, vf_coef, ent_coef, vf_clip, out)


class KLCoeff:
    """RLlib's adaptive KL coefficient as a host float: ``update(mean_action_kl)`` - once per training iteration, with the mean
    ``action_kl`` of the update's minibatches - multiplies ``coeff`` by 1.5 where the mean exceeds ``2 * target`` and by 0.5 where it
    is below ``0.5 * target``; both inequalities are strict, a value on an edge leaves it alone.  Defaults: RLlib's ``kl_coeff`` 0.2
    and ``kl_target`` 0.01.  The rule is restated from memory of RLlib 1.9's ``KLCoeffMixin.update_kl``, not checked against it.
    ``float(k)`` is the coefficient.  A coefficient of 0 stays 0: start above it to have a penalty at all."""

    def __init__(self, coeff=0.2, target=0.01):
        coeff, target = float(coeff), float(target)
        if not (math.isfinite(coeff) and coeff >= 0.0):
            raise ValueError("coeff must be finite and not negative")
        if not (math.isfinite(target) and target > 0.0):
            raise ValueError("target must be finite and greater than 0")
        self.coeff, self.target = coeff, target

    def __float__(self):
        return self.coeff

    def update(self, mean_action_kl):
        """Apply the rule; returns the coefficient."""
        x = float(mean_action_kl)
        if x > 2.0 * self.target:
            self.coeff *= 1.5
        elif x < 0.5 * self.target:
            self.coeff *= 0.5
        return self.coeff


def _head_forward(ctx, res):
    """What ``PPOLoss.forward`` and ``PPOLossKL.forward`` do with their head's result."""
    ctx.save_for_backward(res.grad_logits, res.grad_value)
    ctx.mark_non_differentiable(res.stats)
    return res.stats[0].to(torch.float32), res.stats


def _head_backward(ctx, grad_loss, _grad_stats):
    """... and their ``backward``: ``logits`` and ``value`` get a gradient, every other input of ``apply`` None."""
    grad_logits, grad_value = ctx.saved_tensors
    return (grad_logits * grad_loss, grad_value * grad_loss) + (None,) * (len(ctx.needs_input_grad) - 2)


class PPOLoss(torch.autograd.Function):
    """``loss, stats = PPOLoss.apply(logits, value, mb, clip, vf_coef, ent_coef, vf_clip)``: ``ppo_loss`` inside autograd.  ``loss``
    is ``stats[0]`` as a float32 scalar; ``stats`` (float64 [6]) is not differentiable.  Backward hands the gradients the kernel
    already computed, times the incoming gradient, to ``logits`` and ``value``."""

    @staticmethod
    def forward(ctx, logits, value, mb, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None):
        return _head_forward(ctx, ppo_loss(logits.detach(), value.detach(), mb, clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip))

    backward = staticmethod(_head_backward)


class PPOLossKL(torch.autograd.Function):
    """``loss, stats = PPOLossKL.apply(logits, value, mb, old_logits, kl_coeff, clip, vf_coef, ent_coef, vf_clip)``: ``ppo_loss_kl``
    inside autograd, as ``PPOLoss`` is ``ppo_loss``: ``stats`` float64 [7], not differentiable; ``old_logits`` gets no gradient."""

    @staticmethod
    def forward(ctx, logits, value, mb, old_logits, kl_coeff=0.2, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None):
        return _head_forward(ctx, ppo_loss_kl(logits.detach(), value.detach(), mb, old_logits.detach(), kl_coeff=kl_coeff, clip=clip,
                                              vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip))

    backward = staticmethod(_head_backward)


MAX_NORM_SEGMENTS = 32  # SKC_MAX_SEGMENTS of csrc/skyjo_clip.h: the tensors of one ``grad_norm``


def _max_norm(name, max_norm):
    """``max_norm`` as the float the ABI takes: None - +inf, measure only; otherwise its float32 value must be greater than 0."""
    if max_norm is None:
        return math.inf
    if isinstance(max_norm, bool) or not isinstance(max_norm, (int, float)):
        raise ValueError(name + " must be None or a number")
    x = float(max_norm)
    if not C.c_float(x).value > 0.0:  # (NaN, <= 0, or so small that it is 0 as a float32)
        raise ValueError(name + " must be greater than 0 as a float32, and not NaN")
    return x


@torch.no_grad()
def grad_norm(tensors, max_norm=None, out=None):
    """The global L2 norm of ``tensors`` - a list of 1 to 32 contiguous float32 tensors on one GPU, of any shapes - and the coefficient
    ``torch.nn.utils.clip_grad_norm_(.., max_norm)`` would scale them by, in ONE native launch on torch's current stream
    (``skyjo_vec_grad_norm``, csrc/skyjo_clip.h; not timed: a single workgroup, its cost is the launch).  Returns a float32 ``[2]``
    tensor on that GPU, ``(norm, coef)``: the sum of squares is accumulated in double in a fixed order - the same input gives the same
    bits on every call - and rounded once after the root; ``coef`` is torch's float32 ``clamp(max_norm / (norm + 1e-6), max=1)`` bit for
    bit (torch evaluates the quotient as ``reciprocal() * max_norm``), NaN where the norm is.  ``max_norm`` None (or inf): measure
    only, ``coef`` is 1.  Nothing is read back: no host synchronisation.  The tensors are not changed.  ``out``: a contiguous float32
    ``[2]`` tensor on the same GPU to write instead of a new one."""
    if not isinstance(tensors, (list, tuple)) or not 1 <= len(tensors) <= MAX_NORM_SEGMENTS:
        raise ValueError(f"tensors must be a list of 1 to {MAX_NORM_SEGMENTS} tensors")
    if not isinstance(tensors[0], torch.Tensor) or tensors[0].device.type != "cuda":
        raise ValueError("grad_norm runs on the GPU: tensors[0] is not a tensor there")
    dev = tensors[0].device
    for i, t in enumerate(tensors):
        _column(f"tensors[{i}]", t, torch.float32, tuple(t.shape) if isinstance(t, torch.Tensor) else (), dev)
    x = _max_norm("max_norm", max_norm)
    if out is None:
        out = torch.empty((2,), dtype=torch.float32, device=dev)
    else:
        _column("out", out, torch.float32, (2,), dev)
    n = len(tensors)
    pp, cc = (C.c_void_p * n)(*[t.data_ptr() for t in tensors]), (C.c_int64 * n)(*[t.numel() for t in tensors])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().skyjo_vec_grad_norm(pp, cc, n, x, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out


class NativeAdam:
    """``torch.optim.Adam`` (no amsgrad, no weight decay) for ``model``'s two branches, fused with the re-pack of their ``FusedNet``s:
    ``step()`` is one ``skyjo_vec_mlp_adam_step`` per branch - two kernel launches on torch's current stream, nothing else.  Each
    element's thread reads p, g, exp_avg, exp_avg_sq, applies the rule, writes the three back and packs the new p into the net's MFMA
    fragments in place: when ``step()`` returns, ``policy_net`` and ``value_net`` are queued to hold the updated weights - no
    ``repack``, no new handles, no host copy, no allocation, no synchronisation.  A rollout on the same stream sees them.

    Duck-typed to what ``examples/ppo.py:ppo_update`` calls on its ``optimizer`` (``zero_grad``, ``step``); not a
    ``torch.optim.Optimizer``.  ``lr`` is a plain attribute and may be set between steps.  ``lr``, ``betas`` and ``eps`` reach the
    kernel as float32 (the ABI's type): the bias corrections are computed from the float32 values of the betas.  ``state`` maps a
    parameter to its ``exp_avg`` / ``exp_avg_sq`` views, as ``torch.optim.Adam.state`` does.

    ``max_grad_norm``: None - exactly the above, and ``grad_stats`` is None.  A number - the gradients are clipped by their global L2
    norm as ``torch.nn.utils.clip_grad_norm_`` over all TWELVE tensors of the two branches clips them (RLlib's ``grad_clip``: one norm
    per policy, not one per branch), without leaving the native path: ``step()`` is then three launches - ``grad_norm`` over the twelve
    ``.grad``s into ``grad_stats``, a float32 ``[2]`` device tensor ``(norm before clipping, coefficient)`` allocated here, once, and one
    ``skyjo_vec_mlp_adam_step_clipped`` per branch, which reads the coefficient from there and takes ``g * coef`` for ``g``; the
    ``.grad``s themselves are not rewritten.  Still no allocation and no synchronisation; ``grad_stats`` holds the last step's pair
    (read it when you read your other statistics).  inf: measure only, the coefficient is 1 and the step carries the bits of the
    unclipped one.  A non-finite norm is not caught: the NaN reaches the parameters, as it does with torch.  Like ``lr`` a plain
    attribute that may be set between steps; it is checked in ``step()`` before the first launch.  The three launches were not timed."""

    def __init__(self, model, policy_net, value_net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
        self._L = _lib.load()
        self.lr, self.betas, self.eps = lr, (float(betas[0]), float(betas[1])), float(eps)
        _max_norm("max_grad_norm", max_grad_norm)
        self.max_grad_norm = max_grad_norm
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
        self._stats = torch.zeros((2,), dtype=torch.float32, device=self._branches[0][2].device)
        self._counts = (C.c_int64 * 12)(*[p.numel() for _, params, _, _ in self._branches for p in params])

    @property
    def grad_stats(self):
        """float32 ``[2]`` on the device, ``(norm, coefficient)`` of the last ``step()``; None while ``max_grad_norm`` is None."""
        return None if self.max_grad_norm is None else self._stats

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
        clip = self.max_grad_norm is not None
        max_norm = _max_norm("max_grad_norm", self.max_grad_norm)
        if clip and any(buf.device != self._stats.device for _, _, buf, _ in self._branches):
            raise ValueError("max_grad_norm needs both branches on one GPU: the norm is one launch over their twelve gradients")
        for net, params, buf, pp in self._branches:  # every check before the first launch: both branches step, or neither
            if not net._h:
                raise ValueError("a FusedNet of this optimizer is closed")
            for p in params:
                if p.grad is None:
                    raise ValueError("a parameter has no gradient (.grad is None): NativeAdam steps every parameter of both branches")
                _column("a parameter's .grad", p.grad, torch.float32, tuple(p.shape), p.device)
            calls.append((net, buf, pp, (C.c_void_p * 6)(*[p.grad.data_ptr() for p in params])))
        if clip:
            twelve = (C.c_void_p * 12)(*[g for _, _, _, gg in calls for g in gg])
            with torch.cuda.device(self._stats.device):
                _lib.check(self._L.skyjo_vec_grad_norm(twelve, self._counts, 12, max_norm, self._stats.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream))
        for net, buf, pp, gg in calls:
            hyper = (buf.data_ptr(), buf.numel() * 4, float(self.lr), self.betas[0], self.betas[1], self.eps, self.steps + 1)
            with torch.cuda.device(buf.device):
                stream = torch.cuda.current_stream().cuda_stream
                if clip:
                    _lib.check(self._L.skyjo_vec_mlp_adam_step_clipped(net._h, pp, gg, *hyper, self._stats.data_ptr() + 4, stream))
                else:
                    _lib.check(self._L.skyjo_vec_mlp_adam_step(net._h, pp, gg, *hyper, stream))
        self.steps += 1


UPDATE_STATS = STATS_KL + ("grad_norm", "grad_clipped", "rows")  # the columns of a row of ``NativeUpdate.run``'s statistics


class NativeUpdate:
    """A whole PPO update behind ONE native call (``skyjo_vec_ppo_update``): ``epochs`` passes over a selection in shuffled slices of
    ``minibatch`` rows, every slice the step ``examples/ppo.py::ppo_update(native_batches=True, native_loss=True, native_nets="auto")``
    makes with a ``NativeAdam`` - gather, both branches' forward, the loss head, both backwards, the global-norm clip, Adam with the
    re-pack - queued launch by launch in the same order with the same arguments, so the parameters, the Adam state and both
    ``FusedNet``s end with the same bits; what the host loop does besides (a dozen ctypes calls per step, ``torch.randperm`` and the
    sums of the statistics per epoch) happens once, or on the device.

    ``env``: the engine whose buffers are updated from; ``model`` with its packed ``policy_net`` / ``value_net`` and ``optimizer``, a
    ``NativeAdam`` made on exactly these; ``max_count``: the largest selection a ``run`` may get; ``minibatch`` and ``epochs``: the
    schedule; ``kl``: the runs carry the KL term (``buf.behaviour`` and ``kl_coeff``).  The workspace (``workspace``, uint8, of
    ``workspace_bytes``: minibatch columns, activations, the twelve gradients, the order ...), the statistics and the fault word are
    allocated here, once; ``run`` allocates nothing.  The gradients live in the workspace: the parameters' ``.grad`` are NOT touched -
    neither read nor written nor set.  Either observation: there is no width rule here - ``FusedNet.branch_parameters`` accepts 1 to 163
    inputs and the C side launches the branch kernels that fit the engine's observation (``NativeBranch``'s up to 31 inputs,
    ``NativeWideBranch``'s from 32)."""

    def __init__(self, env, model, policy_net, value_net, optimizer, max_count, minibatch, epochs, kl=False):
        self._L = _lib.load()
        if not isinstance(optimizer, NativeAdam) or [b[0] for b in optimizer._branches] != [policy_net, value_net]:
            raise ValueError("optimizer must be a NativeAdam made on policy_net and value_net")
        for name, x in (("max_count", max_count), ("minibatch", minibatch), ("epochs", epochs)):
            if isinstance(x, bool) or int(x) != x or x < (0 if name == "max_count" else 1):
                raise ValueError(f"{name} must be an integer, at least {0 if name == 'max_count' else 1}")
        self.env, self.model, self.policy_net, self.value_net, self.optimizer = env, model, policy_net, value_net, optimizer
        self.max_count, self.minibatch, self.epochs, self.kl = int(max_count), int(minibatch), int(epochs), bool(kl)
        self._parameters()
        dev = torch.device("cuda", env.device_index)
        self.workspace_bytes = int(self._L.skyjo_vec_ppo_update_workspace_bytes(env._h, self.max_count, self.minibatch, int(self.kl)))
        if self.workspace_bytes <= 0:
            raise ValueError("max_count or minibatch is out of range")
        self.workspace = torch.empty((self.workspace_bytes,), dtype=torch.uint8, device=dev)
        self.stats = torch.zeros((self.epochs, _lib.UPDATE_STATS), dtype=torch.float64, device=dev)
        self.fault = torch.zeros((1,), dtype=torch.int64, device=dev)

    def _parameters(self):
        """Both branches' six parameters as they are now, checked as ``FusedNet.branch_parameters`` and ``NativeBranch`` check them."""
        if not self.policy_net._h or not self.value_net._h:
            raise ValueError("a FusedNet of this update is closed")
        dev = torch.device("cuda", self.env.device_index)
        out = []
        for seq, net, (_, mine, _, _) in zip((self.model.policy, self.model.value), (self.policy_net, self.value_net), self.optimizer._branches):
            params = net.branch_parameters(seq)
            if net.device != self.env.device_index or any(p.device != dev for p in params):
                raise ValueError("the nets and the parameters must live on the engine's GPU")
            if any(p is not q for p, q in zip(params, mine)):
                raise ValueError("a parameter was replaced since the optimizer was made: its Adam state belongs to the old tensor")
            if params[2].data_ptr() % 16 or params[4].data_ptr() % 16:
                raise ValueError("linear 1.weight and 2.weight must start on a 16-byte boundary")
            out.append(params)
        return out

    @torch.no_grad()
    def run(self, buf, sel, *, seed, clip, vf_coef, ent_coef, vf_clip, kl_coeff=None, grad_clip=None, orders=None):
        """One update on the rows ``sel`` (``rollout.select_rows(buf, ...)``) of ``buf`` (``rollout.compute_targets`` must have run; with
        ``kl`` also ``rollout.behaviour_logits``): the one native call.  Returns ``(stats, fault)`` WITHOUT reading them - ``stats``
        float64 [epochs, 10] on the device, a row per epoch in the order of ``UPDATE_STATS``: the head's six statistics and ``action_kl``
        (0.0 without ``kl``) as row-weighted means, ``grad_norm`` and ``grad_clipped`` as means over the epoch's steps (0.0 without
        ``grad_clip``) and the rows seen; ``fault`` int64 [1]: the shuffles' capped walks, 0 unless a kernel has a bug.  Both are this
        object's tensors, refilled by the next ``run``.  The advantages are normalised with ``(sel.mean, max(sel.std, 1e-6))``.  Epoch e
        is shuffled with ``rollout.epoch_order(sel, seed, e)``'s permutation, or is ``orders[e]`` where ``orders`` (int64
        [epochs, count] on the device) is given.  ``lr`` / ``betas`` / ``eps`` are read from the optimizer now; its ``steps`` advance by
        the steps queued, epochs x ceil(count / minibatch).  ``grad_clip``: None - no clipping; a number > 0 - RLlib's ``grad_clip``, as
        ``NativeAdam.max_grad_norm``; inf - measure only.  The parameters' ``.grad`` are not touched.  ``ValueError``, before any
        launch, for whatever the C side would refuse and for a closed net, a replaced parameter, ``sel.count > max_count`` or a buffer of
        another engine."""
        from . import rollout

        if getattr(buf, "_env", None) is not self.env:
            raise ValueError("buf belongs to another engine")
        if getattr(buf, "advantages", None) is None:
            raise ValueError("run needs the columns of compute_targets(buf)")
        rollout._check_records(buf)
        dev = buf.actions.device
        count = int(sel.count)
        if count > self.max_count:
            raise ValueError(f"sel.count = {count} exceeds max_count = {self.max_count}")
        rollout._check_index(buf, sel.index, tensor=True)
        if sel.index.numel() != count or not sel.index.is_contiguous():
            raise ValueError("sel.index must be contiguous and hold sel.count entries")
        if self.kl != (kl_coeff is not None):
            raise ValueError("kl_coeff belongs to kl=True, and kl=True needs it")
        behaviour = None
        if self.kl:
            behaviour = getattr(buf, "behaviour", None)
            if behaviour is None:
                raise ValueError("kl=True needs the column of behaviour_logits(buf, policy_net)")
            _column("buf.behaviour", behaviour, torch.float32, (buf.T, buf.B, NUM_ACTIONS), dev)
            if not (math.isfinite(float(kl_coeff)) and float(kl_coeff) >= 0.0):
                raise ValueError("kl_coeff must be finite and not negative")
        if not (math.isfinite(float(clip)) and float(clip) > 0.0):
            raise ValueError("clip must be finite and greater than 0")
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
        max_norm = 0.0 if grad_clip is None else _max_norm("grad_clip", grad_clip)
        if orders is not None:
            _column("orders", orders, torch.int64, (self.epochs, count), dev)
        policy, value = self._parameters()
        opt = self.optimizer
        a = _lib.PPOUpdateArgs()
        vp = lambda t: t.data_ptr()
        a.records, a.actions, a.logp, a.values = vp(buf.records), vp(buf.actions), vp(buf.logp), vp(buf.values)
        a.advantages, a.value_targets = vp(buf.advantages), vp(buf.value_targets)
        a.behaviour = None if behaviour is None else vp(behaviour)
        a.index = vp(sel.index) if count else vp(self.workspace)  # (an empty index has no address to pass; nothing reads it)
        a.orders = None if orders is None or count == 0 else vp(orders)
        a.policy_net, a.value_net = self.policy_net._h, self.value_net._h
        a.policy_params, a.value_params = (C.c_void_p * 6)(*map(vp, policy)), (C.c_void_p * 6)(*map(vp, value))
        (_, _, pstate, _), (_, _, vstate, _) = opt._branches
        a.policy_state, a.value_state, a.policy_state_bytes, a.value_state_bytes = vp(pstate), vp(vstate), pstate.numel() * 4, vstate.numel() * 4
        a.count, a.minibatch, a.first_step, a.seed = count, self.minibatch, opt.steps + 1, int(seed)
        a.layout, a.T, a.value_stride, a.epochs = rollout._layout(buf), buf.T, buf.values.shape[-1], self.epochs
        a.adv_mean, a.adv_std = float(sel.mean), float(max(sel.std, 1e-6))
        a.clip, a.vf_coef, a.ent_coef = float(clip), float(vf_coef), float(ent_coef)
        a.vf_clip = 0.0 if vf_clip is None or not math.isfinite(float(vf_clip)) or float(vf_clip) <= 0.0 else float(vf_clip)
        a.kl_coeff = float(kl_coeff) if self.kl else 0.0
        a.lr, a.beta1, a.beta2, a.eps, a.max_grad_norm = float(opt.lr), opt.betas[0], opt.betas[1], opt.eps, max_norm
        with torch.cuda.device(dev):
            rc = self._L.skyjo_vec_ppo_update(self.env._h, C.byref(a), vp(self.workspace), self.workspace_bytes, vp(self.stats), vp(self.fault),
                                              torch.cuda.current_stream(dev).cuda_stream)
        if rc == _lib.E_INVALID:  # (the C side checks everything before its first launch)
            raise ValueError(self._L.skyjo_vec_last_error().decode())
        _lib.check(rc)
        opt.steps += self.epochs * -(-count // self.minibatch)
        return self.stats, self.fault


class _BranchFunction(torch.autograd.Function):
    """``NativeBranch.apply``: the branch's two native calls as one autograd node over (x, w1, b1, w2, b2, w3, b3)."""

    @staticmethod
    def forward(ctx, branch, x, *params):
        out = branch.forward(x.detach())
        ctx.branch, ctx.call = branch, branch._call  # (the workspace's identity: nothing else is saved)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        branch = ctx.branch
        if branch._call != ctx.call:
            raise RuntimeError("this NativeBranch ran another forward since: its workspace holds that call's activations")
        branch._backward(grad_out.contiguous())
        return (None, None) + tuple(g.clone() if need else None for g, need in zip(branch.grads, ctx.needs_input_grad[2:]))


class NativeBranch:
    """One branch of the model (``model.policy`` or ``model.value``: Linear-Tanh-Linear-Tanh-Linear, 256 hidden units) trained by
    native calls on its float32 parameters as they lie: ``forward(x)`` is ONE kernel that leaves h1 and h2 in this object's workspace,
    ``backward(grad_out)`` three more - the row pass, the weight pass over chunks of ``TRAIN_CHUNK_ROWS`` rows and the fixed-order sum
    of the chunks' partials (include/skyjo_vec.h: ``skyjo_vec_mlp_train_*``).  The workspace, the output buffer and the six gradient
    tensors (``grads``: w1, b1, w2, b2, w3, b3) are allocated here, once, for up to ``max_rows`` rows; a step allocates nothing, builds no
    autograd graph and does not synchronise.  The same input gives the same bits on every call.

    ``seq`` is checked with ``FusedNet.branch_parameters``' rules - three ``nn.Linear`` of shapes [256, D], [256, 256], [O, 256] with
    1 <= D <= 31 and 1 <= O <= 32, contiguous float32 on one GPU - at construction and again at every call (a parameter that was
    replaced by one of another shape or device is a ``ValueError``, not a launch).  A wider layer 1 is ``NativeWideBranch``'s;
    ``native_branch(seq, max_rows)`` returns the class that fits."""

    OBS_RANGE = (1, 31)  # the layer-1 widths of this class's entry points
    _ENTRIES = ("skyjo_vec_mlp_train_workspace_bytes", "skyjo_vec_mlp_train_forward", "skyjo_vec_mlp_train_backward")

    def __init__(self, seq, max_rows):
        self._L = _lib.load()
        self._lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
        if len(self._lins) != 3:
            raise ValueError("seq must hold three nn.Linear")
        w1, w3 = self._lins[0].weight, self._lins[2].weight
        if not isinstance(w1, torch.Tensor) or w1.dim() != 2 or not isinstance(w3, torch.Tensor) or w3.dim() != 2:
            raise ValueError("seq's linears must have two-dimensional weights")
        self.obs_dim, self.out_dim, self.device = int(w1.shape[1]), int(w3.shape[0]), w1.device
        if self.device.type != "cuda":
            raise ValueError(type(self).__name__ + " runs on the GPU: the parameters are on " + str(self.device))
        lo, hi = self.OBS_RANGE
        if not (lo <= self.obs_dim <= hi and 1 <= self.out_dim <= 32):
            raise ValueError(f"the branch must have {lo}..{hi} inputs and 1..32 outputs")
        if max_rows < 1:
            raise ValueError("max_rows must be at least 1")
        self.max_rows = int(max_rows)
        params = self.parameters()
        self._workspace_bytes, self._forward, self._backward_entry = (getattr(self._L, n) for n in self._ENTRIES)
        nbytes = int(self._workspace_bytes(self.obs_dim, self.out_dim, self.max_rows))
        if nbytes <= 0:
            raise ValueError("max_rows is out of range")
        self.workspace = torch.empty((nbytes // 4,), dtype=torch.float32, device=self.device)
        self.out = torch.empty((self.max_rows, self.out_dim), dtype=torch.float32, device=self.device)
        self.grads = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in params]
        self._gg = (C.c_void_p * 6)(*[g.data_ptr() for g in self.grads])
        self._x, self._call = None, 0

    def parameters(self):
        """w1, b1, w2, b2, w3, b3 of ``seq`` as they are now, checked."""
        shapes = ((HIDDEN, self.obs_dim), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (self.out_dim, HIDDEN), (self.out_dim,))
        names = ("0.weight", "0.bias", "1.weight", "1.bias", "2.weight", "2.bias")
        params = [t for lin in self._lins for t in (lin.weight, lin.bias)]
        for name, t, shape in zip(names, params, shapes):
            _column("linear " + name, t, torch.float32, shape, self.device)
        if params[2].data_ptr() % 16 or params[4].data_ptr() % 16:
            raise ValueError("linear 1.weight and 2.weight must start on a 16-byte boundary")
        return params

    @torch.no_grad()
    def forward(self, x):
        """``x`` float32 [m, D], contiguous on the branch's GPU, 1 <= m <= ``max_rows``.  Returns the branch's output float32 [m, O]: a
        view of ``out``, valid until the next ``forward``.  ``x`` is kept (not copied) for ``backward``."""
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or not 1 <= x.shape[0] <= self.max_rows:
            raise ValueError(f"x must be a float32 tensor of shape [m, {self.obs_dim}], 1 <= m <= {self.max_rows}")
        m = int(x.shape[0])
        _column("x", x, torch.float32, (m, self.obs_dim), self.device)
        pp = (C.c_void_p * 6)(*[p.data_ptr() for p in self.parameters()])
        with torch.cuda.device(self.device):
            _lib.check(self._forward(self.obs_dim, self.out_dim, pp, x.data_ptr(), m, self.out.data_ptr(), self.workspace.data_ptr(),
                                     self.workspace.numel() * 4, torch.cuda.current_stream().cuda_stream))
        self._x, self._call = x, self._call + 1
        return self.out[:m]

    def _backward(self, grad_out):
        if self._x is None:
            raise ValueError("backward needs a forward first: the workspace holds no activations")
        m = int(self._x.shape[0])
        if not isinstance(grad_out, torch.Tensor) or grad_out.dim() != 2 or grad_out.shape[0] != m:
            raise ValueError(f"grad_out must have the {m} rows of the last forward")
        _column("grad_out", grad_out, torch.float32, (m, self.out_dim), self.device)
        params = self.parameters()
        pp = (C.c_void_p * 6)(*[p.data_ptr() for p in params])
        with torch.cuda.device(self.device):
            _lib.check(self._backward_entry(self.obs_dim, self.out_dim, pp, self._x.data_ptr(), grad_out.data_ptr(), m, self._gg,
                                            self.workspace.data_ptr(), self.workspace.numel() * 4, torch.cuda.current_stream().cuda_stream))
        return params

    @torch.no_grad()
    def backward(self, grad_out):
        """``grad_out`` float32 [m, O] - the gradient with respect to what the last ``forward`` returned, m its row count (anything
        else is a ``ValueError``, as is a call before the first ``forward``).  Overwrites ``grads`` with the gradients of the six
        parameters and makes them the parameters' ``.grad`` - whatever ``zero_grad(set_to_none=True)`` did before; ``NativeAdam.step()``
        or a torch optimizer's reads them there.  Reads the parameters and the ``x`` of that ``forward``: both must be unchanged."""
        for p, g in zip(self._backward(grad_out), self.grads):
            p.grad = g

    def apply(self, x):
        """The same pair inside autograd, ``torch.autograd.Function`` over (x, the six parameters): returns ``forward(x)`` with a
        graph node whose backward runs ``backward``'s kernels and hands CLONES of ``grads`` to autograd - which accumulates them into
        ``.grad`` as it does for any function, so a torch-side loss composes with it.  ``x`` gets no gradient.  Backward after another
        ``forward`` of this object raises ``RuntimeError``: the activations are gone."""
        return _BranchFunction.apply(self, x, *self.parameters())


class NativeWideBranch(NativeBranch):
    """``NativeBranch`` for a branch with 32 to 163 inputs - the direct observation's 19 + 12 N features - on the wide entry points
    (``skyjo_vec_mlp_train_wide_forward`` / ``_backward``, csrc/skyjo_train_wide.h): the same interface, the same guarantees, the same
    ``ValueError``s before any launch; a branch with fewer than 32 inputs is ``NativeBranch``'s and refused here.  Layer 1 runs over
    x padded to K = 8 (D // 8 + 1) columns with b1 as the last term of its chain (include/skyjo_vec.h); everything behind layer 1 is
    ``NativeBranch``'s arithmetic."""

    OBS_RANGE = (32, 163)
    _ENTRIES = ("skyjo_vec_mlp_train_wide_workspace_bytes", "skyjo_vec_mlp_train_wide_forward", "skyjo_vec_mlp_train_wide_backward")


def native_branch(seq, max_rows):
    """``NativeBranch(seq, max_rows)`` or ``NativeWideBranch(seq, max_rows)``: the class whose entry points serve the width of ``seq``'s
    first ``nn.Linear`` (up to 31 inputs, and 32 to 163).  Anything else - no such layer, a width of 0 or beyond 163 - goes to
    ``NativeBranch``, whose checks name what is wrong."""
    first = next((m for m in seq if isinstance(m, torch.nn.Linear)), None) if hasattr(seq, "__iter__") else None
    w = getattr(first, "weight", None)
    wide = isinstance(w, torch.Tensor) and w.dim() == 2 and NativeWideBranch.OBS_RANGE[0] <= w.shape[1] <= NativeWideBranch.OBS_RANGE[1]
    return (NativeWideBranch if wide else NativeBranch)(seq, max_rows)
