"""EXAMPLE, not part of the package (SURVEY C5 - RLlib training - is out of scope).  Learner side of the rollout hand-off: a minimal clipped-PPO update that consumes the columns of
``rollout.RolloutBuffer`` - what ``rlskyjo/models/train_model_simple_rllib.py:22-59`` has RLlib's PPO trainer do with the
sample batches of its rollout workers.  The trainer itself (Ray, tune, checkpoints) stays out of scope; this file shows
that the buffer is sufficient for a learner and closes the loop  collect (HIP kernels) -> update (torch autograd on
``ActionMaskModel``) -> re-pack the weights for the matrix cores -> collect.

Rewards in SkyJo arrive once, at the end of an episode, for every seat (skyjo_env.py:293-312); with RLlib's multi-agent
set-up every seat is its own agent, so the return of a step is the final reward of the seat that acted (gamma = 1 inside
an episode).  Steps of episodes that did not finish inside the buffer carry no return and are masked out.
"""
import math

import torch

from skyjo_rl_amd._lib import TGT_HAS_TARGET
from skyjo_rl_amd.action_mask_model import FLOAT_MIN, FusedNet
from skyjo_rl_amd.learner import (STATS, STATS_KL, UPDATE_STATS, KLCoeff, NativeAdam, NativeBranch, NativeUpdate, PPOLossBuffers, PPOLossKLBuffers, native_branch,
                                  ppo_loss, ppo_loss_kl)
from skyjo_rl_amd.rollout import Minibatch, behaviour_logits, compute_targets, epoch_order, minibatches, select_rows


@torch.no_grad()
def compute_returns(buf):
    """returns float32 [T, B]: final reward (skyjo_env.py:293-312) of the acting seat's episode, and mask bool [T, B]:
    the row is a transition (``buf.valid``) whose episode ended inside the buffer."""
    v = buf.views()
    T, B, N = buf.T, buf.B, buf.N
    agent = v.agent[:T].long()                       # the seat that acted at step t
    carry = torch.zeros((B, N), dtype=torch.float64, device=buf.actions.device)
    known = torch.zeros((B,), dtype=torch.bool, device=buf.actions.device)
    returns = torch.zeros((T, B), dtype=torch.float32, device=buf.actions.device)
    mask = torch.zeros((T, B), dtype=torch.bool, device=buf.actions.device)
    valid = buf.valid
    for t in range(T - 1, -1, -1):
        end = buf.episode_end[t].bool()
        carry = torch.where(end.unsqueeze(-1), buf.final_rewards[t], carry)
        known = known | end
        returns[t] = carry.gather(1, agent[t].unsqueeze(1)).squeeze(1).to(torch.float32)
        mask[t] = known & valid[t]
    return returns, mask


_TORCH_STATS = ("policy_loss", "vf_loss", "kl")  # what the torch loss reports, in the order of ``_torch_read``
_REPORTED = _TORCH_STATS + ("entropy", "clip_fraction", "action_kl")  # an epoch's statistics: those of these the loss has
_CLIP_STATS = ("grad_norm", "grad_clipped")  # ... and with ``grad_clip`` these two, means over the epoch's steps


def _clipped_step(model, optimizer, grad_clip):
    """``optimizer.step()`` behind the clipping of the gradients by their global norm; returns ``_CLIP_STATS`` of the step as a float64
    [2] tensor on the parameters' device - the norm before clipping, and 1 where the coefficient was below 1 - without reading it.  A
    ``NativeAdam`` (its ``max_grad_norm`` is ``grad_clip`` for the step, whatever it was) clips inside its step; for a torch optimizer
    it is ``torch.nn.utils.clip_grad_norm_`` over the parameters of both branches, whose coefficient is formed here once more."""
    if isinstance(optimizer, NativeAdam):
        earlier, optimizer.max_grad_norm = optimizer.max_grad_norm, grad_clip
        try:
            optimizer.step()
            norm, below = optimizer.grad_stats[0], optimizer.grad_stats[1] < 1.0
        finally:
            optimizer.max_grad_norm = earlier
    else:
        norm = torch.nn.utils.clip_grad_norm_(list(model.policy.parameters()) + list(model.value.parameters()), grad_clip)
        below = grad_clip / (norm + 1e-6) < 1.0
        optimizer.step()
    return torch.stack([norm.to(torch.float64), below.to(torch.float64)])


def _torch_batches(buf, minibatch, seed, gae):
    """The torch batch source: the columns of ``buf.views()``, the ``nonzero`` index of the rows with a target and per epoch a
    ``randperm`` of it, every slice as a ``rollout.Minibatch`` (``values`` and ``seats`` None: the torch loss reads neither).  Returns
    ``(epoch, transitions)``; ``epoch()`` yields one epoch's minibatches."""
    v = buf.views()
    T = buf.T
    if gae is None:
        returns, mask = compute_returns(buf)
    else:
        compute_targets(buf, gamma=gae[0], lam=gae[1])
        returns, mask = buf.value_targets, (buf.target_flags & TGT_HAS_TARGET) != 0
    idx = mask.reshape(-1).nonzero().squeeze(1)
    obs = v.observations[:T].reshape(-1, v.observations.shape[-1])
    am = v.action_mask[:T].reshape(-1, 26)
    act = buf.actions.reshape(-1).long()
    logp_old = buf.logp.reshape(-1)
    val_old = buf.values[:T].reshape(-1)
    ret = returns.reshape(-1)
    adv_all = ret - val_old if gae is None else buf.advantages.reshape(-1)
    mean, std = adv_all[idx].mean(), adv_all[idx].std().clamp_min(1e-6)
    gen = torch.Generator(device=idx.device).manual_seed(seed)

    def epoch():
        perm = idx[torch.randperm(idx.numel(), device=idx.device, generator=gen)]
        for k in range(0, perm.numel(), minibatch):
            j = perm[k:k + minibatch]
            # log(1) = 0 and log(0) = -inf clamped to FLOAT_MIN: the two values ``gather_rows`` writes
            yield Minibatch(obs[j].to(torch.float32), torch.clamp(torch.log(am[j].to(torch.float32)), min=FLOAT_MIN), act[j], logp_old[j],
                            (adv_all[j] - mean) / std, ret[j], None, None)

    return epoch, int(idx.numel())


def _native_batches(buf, minibatch, seed, gae, seats, behaviour, shuffle):
    """The native batch source: ``rollout.minibatches`` on the buffer as it lies - with ``behaviour``, ``(minibatch, old_logits)``.
    ``shuffle``: "torch" - a ``randperm`` per epoch from one generator seeded with ``seed``; "native" - ``rollout.epoch_order(sel, seed,
    ep)``, ``ep`` counting the epochs of the call from 0, into one index tensor that every epoch refills (its fault word stays unread: this
    loop reads once per epoch, and that read is the statistics').  Returns ``(epoch, transitions)`` as ``_torch_batches`` does."""
    compute_targets(buf, gamma=gae[0], lam=gae[1])
    sel = select_rows(buf, TGT_HAS_TARGET, seats=seats)
    norm = (sel.mean, max(sel.std, 1e-6))
    kw = {"behaviour": True} if behaviour else {}
    if shuffle == "native":
        order, ep = torch.empty((sel.count,), dtype=torch.int64, device=buf.actions.device), [0]

        def epoch():
            ep[0] += 1
            return minibatches(buf, minibatch, normalize=norm, selection=sel, order=epoch_order(sel, seed, ep[0] - 1, out=order)[0], **kw)

        return epoch, sel.count
    gen = torch.Generator(device=buf.actions.device).manual_seed(seed)
    return (lambda: minibatches(buf, minibatch, generator=gen, normalize=norm, selection=sel, **kw)), sel.count


def _native_update(model, buf, optimizer, epochs, minibatch, seed, gae, seats, kl, coeff, grad_clip, head):
    """``ppo_update(native_update=True)``: the selection, ``learner.NativeUpdate`` on the optimizer's nets and ONE read - the epochs'
    statistics with the fault word - turned into the result ``_epochs`` returns, by its host arithmetic."""
    compute_targets(buf, gamma=gae[0], lam=gae[1])
    sel = select_rows(buf, TGT_HAS_TARGET, seats=seats)
    (policy_net, _, _, _), (value_net, _, _, _) = optimizer._branches
    update = NativeUpdate(buf._env, model, policy_net, value_net, optimizer, sel.count, minibatch, epochs, kl=kl is not None)
    # (without grad_clip the optimizer's own max_grad_norm holds, as in its step(); the statistics report the clipping grad_clip asks for)
    stats, fault = update.run(buf, sel, seed=seed, kl_coeff=None if kl is None else coeff,
                              grad_clip=optimizer.max_grad_norm if grad_clip is None else grad_clip, **head)
    host = torch.cat([stats.reshape(-1), fault.to(torch.float64)]).tolist()  # the call's one read
    names = STATS if kl is None else STATS_KL
    per_epoch = []
    total_kl, total_rows = 0.0, 0
    for ep in range(epochs):
        row = dict(zip(UPDATE_STATS, host[ep * len(UPDATE_STATS):(ep + 1) * len(UPDATE_STATS)]))
        per_epoch.append({k: row[k] for k in _REPORTED if k in names})
        if grad_clip is not None and sel.count:
            per_epoch[-1].update((k, row[k]) for k in _CLIP_STATS)
        if kl is not None:
            total_kl += row["action_kl"] * sel.count
            total_rows += sel.count
    result = {"first": per_epoch[0], "last": per_epoch[-1], "transitions": sel.count}
    if kl is not None:
        mean_kl = total_kl / max(total_rows, 1)
        result.update(mean_action_kl=mean_kl, kl_coeff=kl.update(mean_kl) if isinstance(kl, KLCoeff) and total_rows else float(kl))
    if host[-1] != 0.0:
        raise RuntimeError("skyjo_vec_ppo_update: %d positions of the epochs' orders hit the walk cap (their rows entered as zeros)" % int(host[-1]))
    return result


def _torch_loss(model, mb, clip, vf_coef):
    """The torch loss on a ``Minibatch`` of either source: (loss, policy loss, value loss, logp of the actions taken)."""
    logits = model.policy(mb.observations) + mb.log_mask  # action_mask_model.py:70-71
    logp = torch.log_softmax(logits, -1).gather(1, mb.actions.unsqueeze(1)).squeeze(1)
    value = model.value(mb.observations).squeeze(-1)
    ratio = torch.exp(logp - mb.logp)
    pl = -torch.min(ratio * mb.advantages, torch.clamp(ratio, 1 - clip, 1 + clip) * mb.advantages).mean()
    vl = ((value - mb.value_targets) ** 2).mean()
    return pl + vf_coef * vl, pl, vl, logp


def _torch_read(out, mb):
    """``_TORCH_STATS`` of a ``_torch_loss``: three reads as Python floats, as a host tensor for the epoch's sum (double products and
    sums, as Python's own)."""
    _, pl, vl, logp = out
    return torch.tensor([float(pl.detach()), float(vl.detach()), float((mb.logp - logp).mean().detach())], dtype=torch.float64)


def _epochs(epochs, batches, names, evaluate, read, step, device, transitions, kl):
    """THE loop of ``ppo_update``.  ``batches()`` yields an epoch's minibatches (with ``kl``, paired with the old logits),
    ``evaluate(mb, old_logits)`` runs the model and the loss and leaves the gradients with the parameters, ``read(out, mb)`` is what
    it returned as a float64 vector of the statistics ``names`` on ``device``: summed there times the rows and read once per epoch.
    ``step()`` is the optimizer's step; what it returns (None, or ``_clipped_step``'s pair) is summed per step and read with them.
    A ``KLCoeff`` is updated once, after the last epoch, from the row-weighted mean ``action_kl`` over every minibatch of the call (as
    RLlib averages its learner statistics over the SGD phase before ``update_kl`` - from memory)."""
    stats = []
    total_kl, total_rows = 0.0, 0  # host floats, from the epochs' reads: no synchronisation of their own
    for ep in range(epochs):
        tot = torch.zeros((len(names),), dtype=torch.float64, device=device)
        seen, steps, clip_tot = 0, 0, None
        for item in batches():
            mb, old_logits = (item, None) if kl is None else item
            out = evaluate(mb, old_logits)
            clipped = step()
            n = mb.actions.numel()
            tot += read(out, mb) * n
            seen += n
            if clipped is not None:
                clip_tot = clipped if clip_tot is None else clip_tot.add_(clipped)
                steps += 1
        mean = tot / max(seen, 1)
        if clip_tot is not None:
            mean = torch.cat([mean, clip_tot.to(mean.device) / steps])
        host = mean.tolist()  # the epoch's one read
        stats.append({k: host[names.index(k)] for k in _REPORTED if k in names})
        if clip_tot is not None:
            stats[-1].update(zip(_CLIP_STATS, host[len(names):]))
        if kl is not None:
            total_kl += stats[-1]["action_kl"] * seen
            total_rows += seen
    result = {"first": stats[0], "last": stats[-1], "transitions": transitions}
    if kl is not None:
        mean_kl = total_kl / max(total_rows, 1)
        result.update(mean_action_kl=mean_kl, kl_coeff=kl.update(mean_kl) if isinstance(kl, KLCoeff) and total_rows else float(kl))
    return result


def ppo_update(model, buf, optimizer, epochs=2, minibatch=1 << 15, clip=0.3, vf_coef=1.0, seed=0, gae=None, native_batches=False,
               native_loss=False, ent_coef=0.0, vf_clip=None, native_nets=False, seats=None, kl=None, behaviour_net=None, grad_clip=None,
               shuffle="torch", native_update=False):
    """Clipped-surrogate PPO epochs over the buffer (RLlib defaults: clip_param 0.3, vf_loss_coeff 1.0).  Returns the mean
    losses of the first and the last epoch.  ``gae``: None - Monte-Carlo returns of the episodes that ended inside the buffer
    (``compute_returns``); (gamma, lambda) - advantages, value targets and the row mask of ``rollout.compute_targets`` (one
    native call; rows of unfinished episodes take part, bootstrapped from the value estimates).  ``native_batches`` (needs
    ``gae``): the minibatches come from ``rollout.minibatches`` - row selection, advantage moments and the gather in native calls
    on the buffer as it lies, no ``buf.views()`` - instead of the torch expressions below.  ``native_loss`` (needs
    ``native_batches``): the loss head is ``learner.ppo_loss`` - one kernel between the model's outputs and ``optimizer.step()``; only
    this path knows ``ent_coef`` (an entropy bonus) and ``vf_clip`` (RLlib's ``vf_clip_param``), and its statistics gain ``entropy``
    and ``clip_fraction``.  ``native_nets`` (needs ``native_loss``): the two branches' forwards and backwards are
    ``learner.NativeBranch``'s kernels on the float32 parameters - a minibatch step is then a fixed sequence of native launches.
    ``native_nets="auto"`` builds the branches with ``learner.native_branch``: ``NativeBranch`` up to 31 inputs, ``NativeWideBranch`` for
    the direct observation's 32 to 163.  ``True`` keeps constructing ``NativeBranch`` and so keeps raising its ``ValueError`` on a
    wider model before anything changes: the value had that meaning before the wide kernels existed, and callers (and tests) rely on
    the refusal; with ``native_update=True`` both values are the same, since the C side picks the kernels by the engine's observation.
    ``seats`` (needs ``native_batches``): an iterable of seat numbers - the update runs on the rows in which these seats acted, their
    advantages normalised with their own moments (``rollout.select_rows(buf, seats=...)``): ``model`` is the policy of those seats
    in a buffer that ``arena.collect`` filled.  None: every row, as before.  ``kl`` (needs ``native_loss`` and ``behaviour_net``): a
    float or a ``learner.KLCoeff`` - the loss gains RLlib's KL penalty against the behaviour distribution (``learner.ppo_loss_kl``;
    RLlib's default coefficient is 0.2, adapted towards ``kl_target`` 0.01 - restated from memory, ray is not installed here), with
    ``behaviour_net`` the policy ``FusedNet`` that filled the buffer (of the seats being updated, for an arena buffer).  The epoch
    statistics gain ``action_kl`` and the result ``mean_action_kl`` - the row-weighted mean over every minibatch of the call - and
    ``kl_coeff``: the coefficient AFTER the call, a ``KLCoeff`` having been updated once with that mean.  None: no such term, the
    paths above.  ``grad_clip`` (any path): RLlib's ``grad_clip`` - every step's gradients are scaled by
    ``min(1, grad_clip / (norm + 1e-6))``, ``norm`` the global L2 norm over the parameters of both branches.  A ``learner.NativeAdam``
    does it inside its step (its ``max_grad_norm`` is set for the call's steps: one more native launch, no allocation, no synchronisation), a
    torch optimizer through ``torch.nn.utils.clip_grad_norm_`` between the backward and its step.  The epoch statistics gain
    ``grad_norm`` - the mean over the epoch's steps of the norm before clipping - and ``grad_clipped``, the share of steps whose
    coefficient was below 1; both are summed on the device and come with the epoch's read.  None: no clipping, every path and every
    result as without the keyword.  ``shuffle`` ("native" needs ``native_batches``): "torch" - an epoch's order is a ``torch.randperm``
    from a generator seeded with ``seed``; "native" - ``rollout.epoch_order(sel, seed, ep)``, ``ep`` counted from 0 inside the call: one
    native launch pair per epoch, no generator, no fancy-index allocation.  ``native_update`` (needs ``native_nets`` True or "auto", ``shuffle="native"``
    and a ``learner.NativeAdam``): the whole update is ONE native call (``learner.NativeUpdate``, ``skyjo_vec_ppo_update``) that queues the
    launches the loop below would make, in its order - parameters, Adam state, nets and every number of the result carry the bits of
    ``native_update=False`` - and the statistics of all epochs are read once, at the end; a non-zero fault word of the shuffles raises
    ``RuntimeError`` after that read.  The parameters' ``.grad`` are not touched on this path."""
    if shuffle not in ("torch", "native"):
        raise ValueError('shuffle must be "torch" or "native"')
    if shuffle == "native" and not native_batches:
        raise ValueError('shuffle="native" needs native_batches=True')
    if native_nets not in (False, True, "auto"):
        raise ValueError('native_nets must be False, True or "auto"')
    if native_update and not (native_nets and shuffle == "native" and isinstance(optimizer, NativeAdam)):
        raise ValueError('native_update=True needs native_nets=True or "auto", shuffle="native" and a learner.NativeAdam as optimizer')
    if grad_clip is not None:
        if isinstance(grad_clip, bool) or not isinstance(grad_clip, (int, float)) or not (math.isfinite(grad_clip) and grad_clip > 0):
            raise ValueError("grad_clip must be None or a finite number greater than 0")
        grad_clip = float(grad_clip)
    if kl is not None:
        if isinstance(kl, bool) or not isinstance(kl, (int, float, KLCoeff)):
            raise ValueError("kl must be None, a float or a learner.KLCoeff")
        if not native_loss or not native_batches or gae is None:
            raise ValueError("kl needs native_batches=True, native_loss=True and gae=(gamma, lambda)")
        if not isinstance(behaviour_net, FusedNet):
            raise ValueError("kl needs behaviour_net: the policy FusedNet that filled the buffer")
    else:
        if behaviour_net is not None:
            raise ValueError("behaviour_net belongs to kl")
        if seats is not None and not native_batches:
            raise ValueError("seats belongs to native_batches=True")
        if native_nets and not native_loss:
            raise ValueError('native_nets=True (or "auto") needs native_loss=True')
        if native_loss and not native_batches:
            raise ValueError("native_loss=True needs native_batches=True")
        if not native_loss and (ent_coef != 0.0 or vf_clip is not None):
            raise ValueError("ent_coef and vf_clip belong to native_loss=True")
        if native_batches and gae is None:
            raise ValueError("native_batches=True needs gae=(gamma, lambda)")
    if kl is not None:
        coeff = float(kl)  # constant during the call
        behaviour_logits(buf, behaviour_net)  # before the first step changes (and a NativeAdam re-packs) the net that played
    # the optimizer's step, behind the clipping where there is one
    step = optimizer.step if grad_clip is None else lambda: _clipped_step(model, optimizer, grad_clip)
    # where a minibatch comes from
    if native_batches:
        if native_update:
            return _native_update(model, buf, optimizer, epochs, minibatch, seed, gae, seats, kl, coeff if kl is not None else None, grad_clip,
                                  dict(clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip))
        batches, transitions = _native_batches(buf, minibatch, seed, gae, seats, kl is not None, shuffle)
    else:
        batches, transitions = _torch_batches(buf, minibatch, seed, gae)
    # which loss is evaluated: the torch expressions, whose gradients reach the parameters through their own graph ...
    if not native_loss:
        def evaluate(mb, old_logits):
            out = _torch_loss(model, mb, clip, vf_coef)
            optimizer.zero_grad(set_to_none=True)
            out[0].backward()
            return out

        return _epochs(epochs, batches, _TORCH_STATS, evaluate, _torch_read, step, "cpu", transitions, None)
    # ... or the native head (the kernel adds the mask: action_mask_model.py:70-71): no allocation inside the loop, one read per epoch
    dev, rows = buf.actions.device, max(min(minibatch, transitions), 1)
    out = (PPOLossBuffers if kl is None else PPOLossKLBuffers)(rows, dev)
    head = dict(clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, vf_clip=vf_clip, out=out)
    if kl is None:
        loss = lambda logits, value, mb, old_logits: ppo_loss(logits, value, mb, **head)
    else:
        loss = lambda logits, value, mb, old_logits: ppo_loss_kl(logits, value, mb, old_logits, kl_coeff=coeff, **head)
    # how its gradients reach the parameters
    if native_nets:
        # the branches' own kernels: every call of a step native, no autograd graph, no ``zero_grad`` (``backward`` overwrites the gradients)
        make = native_branch if native_nets == "auto" else NativeBranch  # (True: the class of up to 31 inputs, whatever the model's width)
        policy, value_branch = make(model.policy, rows), make(model.value, rows)
        forward = lambda obs: (policy.forward(obs), value_branch.forward(obs))

        def backward(logits, value, res):
            policy.backward(res.grad_logits)
            value_branch.backward(res.grad_value)
    else:
        forward = lambda obs: (model.policy(obs), model.value(obs))  # autograd runs through the two branches only

        def backward(logits, value, res):
            optimizer.zero_grad(set_to_none=True)
            torch.autograd.backward([logits, value], [res.grad_logits, res.grad_value])

    def evaluate(mb, old_logits):
        logits, value = forward(mb.observations)
        res = loss(logits, value, mb, old_logits)
        backward(logits, value, res)
        return res

    return _epochs(epochs, batches, STATS if kl is None else STATS_KL, evaluate, lambda res, mb: res.stats, step, dev, transitions, kl)


def ppo_update_per_seat(models, buf, optimizers, gae=(0.99, 1.0), native_loss=True, native_nets=False, kls=None, behaviour_nets=None, **kw):
    """One PPO update per seat that has a model, on a buffer ``arena.collect`` filled with every seat playing its own policy - the
    reference's set-up, ``policies = {name: ... for name in env.agents}`` with ``policy_mapping_fn = lambda agent_id: agent_id``
    (``rlskyjo/models/train_model_simple_rllib.py:43-49``).  ``models`` / ``optimizers``: ``buf.N`` entries each, seat s's
    ``ActionMaskModel`` and its optimizer (a ``learner.NativeAdam`` re-packs the seat's ``FusedNet``s in its ``step``), or None for a
    seat that does not learn (a frozen or a random opponent).  Seat s runs ``ppo_update(models[s], buf, optimizers[s], seats=(s,),
    native_batches=True, ...)``: its own rows, normalised with its own moments, as RLlib normalises per policy batch.  Seats that
    share a model must be updated together: call ``ppo_update(..., seats=(s0, s1))`` yourself.  Returns the list of ``ppo_update``'s
    results, None for a seat without a model.  ``kls`` / ``behaviour_nets``: ``buf.N`` entries each - seat s's ``kl`` (a float or its own
    ``learner.KLCoeff``) and the policy ``FusedNet`` that played it -, None where the seat does not learn or learns without the
    penalty; both None: no seat has one.  ``kw``: ``ppo_update``'s other keywords."""
    models, optimizers = list(models), list(optimizers)
    if len(models) != buf.N or len(optimizers) != buf.N:
        raise ValueError(f"models and optimizers need {buf.N} entries each (None for a seat that does not learn)")
    if any((m is None) != (o is None) for m, o in zip(models, optimizers)):
        raise ValueError("a seat has a model and an optimizer, or neither")
    learners = [m for m in models if m is not None]
    if len({id(m) for m in learners}) != len(learners):
        raise ValueError("two seats share a model: update them in one ppo_update(..., seats=(...)) call")
    kls = [None] * buf.N if kls is None else list(kls)
    behaviour_nets = [None] * buf.N if behaviour_nets is None else list(behaviour_nets)
    if len(kls) != buf.N or len(behaviour_nets) != buf.N:
        raise ValueError(f"kls and behaviour_nets need {buf.N} entries each (None for a seat without the KL penalty)")
    if any(m is None and (k is not None or b is not None) for m, k, b in zip(models, kls, behaviour_nets)):
        raise ValueError("a seat without a model takes neither a kl nor a behaviour_net")
    return [None if m is None else ppo_update(m, buf, o, gae=gae, native_batches=True, native_loss=native_loss, native_nets=native_nets,
                                              seats=(s,), kl=kls[s], behaviour_net=behaviour_nets[s], **kw)
            for s, (m, o) in enumerate(zip(models, optimizers))]


def repack(model, device=0):
    """The updated weights as MFMA fragments for the next rollout: (policy FusedNet, value FusedNet) - NEW nets from host copies of the
    parameters (twelve blocking reads, two allocations and a synchronise each, and the old nets to ``close()``).  The in-place way: ``FusedNet.update(seq)`` re-packs an
    existing net from the parameters on the GPU in one launch, and ``learner.NativeAdam(model, pol, val, lr=...)`` passed to
    ``ppo_update`` as its ``optimizer`` does that inside every ``step()`` - the nets a rollout holds then never change identity."""
    return FusedNet(model.policy, device=device), FusedNet(model.value, device=device)


def evaluate_vs_random(env, policy_net, T, seat=0, seed=0, first_ticket=0):
    """Did training help?  ``policy_net`` (the ``FusedNet`` of the trained policy branch) plays GREEDY - ``logits.argmax()`` over the
    legal actions, what ``rlskyjo/models/train_model_simple_rllib.py:123-130`` does with its trained policies - in seat ``seat``, and
    ``policy_ra`` (uniform over the legal actions) plays every other seat, for ``T`` lockstep iterations of ``env`` in one native call
    (``skyjo_rl_amd.arena``).  Returns ``arena.EpisodeStats``: episodes, and per seat the mean / standard deviation of the final reward
    and the win rate; ``stats.mean_reward[seat]`` and ``stats.win_rate[seat]`` are the trained seat's.

    The rewards of the training rollout cannot answer the question.  A seat's final reward is ``-score + mean(scores) + mean_reward``
    (plus the refund bonus; skyjo_env.py:293-312): relative to the table's mean.  In self-play with one shared policy the seats'
    rewards therefore average to ``mean_reward`` per episode whatever the policy has learned - a better policy lowers every seat's
    score and the mean with it.  Against seats that stay random, the trained seat's reward and win rate move with its skill."""
    from skyjo_rl_amd import arena

    seats = ["random"] * env.num_players
    seats[seat] = ("greedy", policy_net)
    return arena.evaluate(env, seats, T, seed=seed, first_ticket=first_ticket)
