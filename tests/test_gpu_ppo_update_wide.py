"""The learner's native path on the direct observation (43 inputs at two players, 67 at four): the hand-off ``NativeWideBranch.forward ->
ppo_loss -> backward`` against torch autograd in float64, ``ppo_update(native_nets="auto")`` step by step, and the one-call update
(``skyjo_vec_ppo_update`` on a wide engine) BYTE FOR BYTE against that loop from identical state - the contract
tests/test_gpu_ppo_update_native.py holds for the narrow nets.  Row-major records, 256 games, T = 8."""
import copy

import numpy as np
import pytest

from tests import mlp_train_ref, mlp_train_wide_ref as ref
from tests.ppo_update_state import Learner as _Learner, flat as _flat, same as _same

pytestmark = pytest.mark.gpu

B, T, EPOCHS, SEED = 256, 8, 2, 11
GAE = (0.99, 0.95)
HEAD = dict(clip=0.3, vf_coef=1.0, ent_coef=0.01, vf_clip=0.2)
MARGIN = 4.0                     # the project's factor (tests/test_gpu_mlp_train.py) on ref.F32_DEVIATION_WIDE
PLAYERS = (2, 4)
_SETUPS = {}


def _setup(N):
    """(env, buf, model, selection) of a direct-observation engine's filled buffer, made once per player count."""
    if N in _SETUPS:
        return _SETUPS[N]
    import torch

    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer, collect, compute_targets, select_rows

    torch.manual_seed(N)
    env = SkyjoVecEnv(B, num_players=N, observe_other_player_indirect=False)
    assert env.obs_dim == 19 + 12 * N and ref.MIN_OBS <= env.obs_dim <= ref.MAX_OBS
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    compute_targets(buf, gamma=GAE[0], lam=GAE[1])
    sel = select_rows(buf)
    pol.close(), val.close()
    assert not buf.planar and 1024 < sel.count <= B * T
    _SETUPS[N] = (env, buf, model, sel)
    return _SETUPS[N]


def _minibatch(count):
    """At least three slices per epoch, the last one short and no multiple of 64 rows."""
    for size in range(600, 664):
        if -(-count // size) >= 3 and (count % size) % 64 != 0:
            return size
    raise AssertionError("no minibatch size for %d rows" % count)


@pytest.mark.parametrize("N", PLAYERS)
def test_hand_off_against_autograd_in_float64(N):
    """The bound is the kernels' own (MARGIN x F32_DEVIATION_WIDE), though the gradients here also carry the loss head's float32 rounding of
    ``grad_logits`` / ``grad_value``.  The value branch's ``b3`` is the plain sum of ``grad_value`` over the rows, whose terms cancel: its
    normalised deviation is the largest of the 24 by far (four players, this seed: 6.87e-06 of 7.2e-06; every policy gradient is below a
    quarter of its bound) and depends on the rollout - on the engine's seed and the rows selected - not on layer 1.  A change to the rollout
    that trips ``value b3`` alone is that cancellation, not the wide kernels."""
    import torch

    from skyjo_rl_amd.learner import NativeWideBranch, native_branch, ppo_loss
    from skyjo_rl_amd.rollout import minibatches
    from tests import ppo_loss_synth as synth

    env, buf, model, sel = _setup(N)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mb = next(iter(minibatches(buf, 1 << 15, generator=gen, normalize=(sel.mean, max(sel.std, 1e-6)), selection=sel)))
    mb = type(mb)(*(c.clone() for c in mb))
    m = mb.actions.numel()
    assert m == sel.count and tuple(mb.observations.shape) == (m, env.obs_dim)

    m64 = copy.deepcopy(model).double()
    c = lambda t: t.double()
    loss, _ = synth.torch_head(m64.policy(c(mb.observations)), c(mb.log_mask), m64.value(c(mb.observations)).squeeze(-1), mb.actions,
                               c(mb.logp), c(mb.advantages), c(mb.value_targets), c(mb.values), clip=0.3)
    want = [torch.autograd.grad(loss, list(seq.parameters()), retain_graph=True) for seq in (m64.policy, m64.value)]

    mine = copy.deepcopy(model)
    bp, bv = native_branch(mine.policy, m), native_branch(mine.value, m)
    assert type(bp) is NativeWideBranch and type(bv) is NativeWideBranch
    logits, value = bp.forward(mb.observations), bv.forward(mb.observations)
    res = ppo_loss(logits, value, mb, clip=0.3)
    bp.backward(res.grad_logits), bv.backward(res.grad_value)
    for name, seq, w in (("policy", mine.policy, want[0]), ("value", mine.value, want[1])):
        for k, p, g64 in zip(ref.PARAMS, seq.parameters(), w):
            d = mlp_train_ref.normalised_deviation(p.grad.cpu().numpy(), g64.cpu().numpy())
            print(f"N={N} {name} {k}: {d:.3e} (bound {MARGIN * ref.F32_DEVIATION_WIDE['A'][k]:.3e})")
            assert d <= MARGIN * ref.F32_DEVIATION_WIDE["A"][k], (name, k, d)


@pytest.mark.parametrize("N", PLAYERS)
def test_step_by_step_update_moves_parameters_and_blobs(N):
    import torch

    from examples.ppo import ppo_update
    from skyjo_rl_amd.action_mask_model import FusedNet

    env, buf, model, sel = _setup(N)
    ln = _Learner(model)
    before = [p.detach().clone() for p in ln.params]
    with pytest.raises(ValueError, match="1..31 inputs"):     # True keeps meaning NativeBranch: refused before anything changes
        ppo_update(ln.model, buf, ln.opt, epochs=1, minibatch=1024, gae=GAE, native_batches=True, native_loss=True, native_nets=True)
    assert all(torch.equal(p.detach(), q) for p, q in zip(ln.params, before)) and ln.opt.steps == 0
    out = ppo_update(ln.model, buf, ln.opt, epochs=EPOCHS, minibatch=1024, gae=GAE, native_batches=True, native_loss=True, native_nets="auto")
    keys = ("policy_loss", "vf_loss", "kl", "entropy", "clip_fraction")
    assert all(set(out[k]) == set(keys) for k in ("first", "last")) and out["transitions"] == sel.count
    assert all(np.isfinite([out[k][j] for k in ("first", "last") for j in keys]))
    assert all(float((p.detach() - q).abs().max()) > 0 for p, q in zip(ln.params, before))
    for net, seq in ((ln.pol, ln.model.policy), (ln.val, ln.model.value)):
        fresh = FusedNet(seq)
        assert torch.equal(net.export(), fresh.export())
        fresh.close()
    ln.close()


def _both(N, kw, kl=False):
    """The step-by-step loop and the one call from identical state: (python result, native result), states and results compared."""
    from examples.ppo import ppo_update
    from skyjo_rl_amd.learner import KLCoeff

    env, buf, model, sel = _setup(N)
    results, states = [], []
    for native in (False, True):
        ln = _Learner(model)
        extra = dict(kl=KLCoeff(), behaviour_net=ln.pol) if kl else {}
        results.append(ppo_update(ln.model, buf, ln.opt, shuffle="native", native_update=native, gae=GAE, native_batches=True,
                                  native_loss=True, native_nets="auto", epochs=EPOCHS, seed=SEED, **HEAD, **extra, **kw))
        if kl:
            results[-1]["coefficient object"] = float(extra["kl"])
        states.append(ln.state())
        assert ln.opt.steps == EPOCHS * -(-sel.count // kw["minibatch"])
        ln.close()
    _same(states[0], states[1], "learner state")
    _same(_flat(results[0]), _flat(results[1]), "result")     # (a non-zero fault word would have raised in the one call)
    return results


@pytest.mark.parametrize("N", PLAYERS)
def test_one_call_equals_the_steps(N):
    _, _, _, sel = _setup(N)
    size = _minibatch(sel.count)
    py, nat = _both(N, dict(minibatch=size))
    print("N=%d: %d rows, minibatch %d (last slice %d), policy loss %.6f -> %.6f" % (N, sel.count, size, sel.count % size,
                                                                                     py["first"]["policy_loss"], py["last"]["policy_loss"]))
    assert py["transitions"] == sel.count and "grad_norm" not in nat["first"] and "kl_coeff" not in nat


@pytest.mark.parametrize("N", PLAYERS)
def test_one_call_equals_the_steps_with_grad_clip(N):
    _, _, _, sel = _setup(N)
    py, nat = _both(N, dict(minibatch=_minibatch(sel.count), grad_clip=0.05))
    print("N=%d clipped: first %r" % (N, py["first"]))
    assert py["first"]["grad_norm"] > 0.0 and 0.0 <= py["first"]["grad_clipped"] <= 1.0


def test_one_call_equals_the_steps_with_the_kl_term():
    _, _, _, sel = _setup(4)
    py, nat = _both(4, dict(minibatch=_minibatch(sel.count), grad_clip=0.05), kl=True)
    assert py["first"]["action_kl"] >= 0.0 and "mean_action_kl" in nat


def test_update_workspace_grows_with_the_wide_branches():
    """``skyjo_vec_ppo_update_workspace_bytes`` on a wide engine is not 0 and holds the wide branches' workspaces."""
    from skyjo_rl_amd import _lib

    env, buf, model, sel = _setup(2)
    L = _lib.load()
    D = env.obs_dim
    small, big = (int(L.skyjo_vec_ppo_update_workspace_bytes(env._h, sel.count, mb, 0)) for mb in (256, 512))
    grow = sum(ref.workspace_bytes(D, O, 512) - ref.workspace_bytes(D, O, 256) for O in (26, 1))
    assert small > 0 and big - small >= grow                  # (every piece is rounded up to 256 bytes: at least the branches' growth)
