"""The learner's way back to the matrix cores in place (skyjo_vec_mlp_update / skyjo_vec_mlp_adam_step, csrc/skyjo_update.h):
``FusedNet.update`` writes the bytes ``FusedNet(seq)`` would and tests/mlp_pack_ref.py says, ``learner.NativeAdam`` is
``torch.optim.Adam``'s rule with the same re-pack behind it, and collect -> learn -> collect closes on the same two handles."""
import copy
import ctypes as C

import numpy as np
import pytest

from . import mlp_pack_ref as ref
from .test_mlp_pack_ref import adam_reference

pytestmark = pytest.mark.gpu

CASES = [(p, o, d) for p in ("fp32", "bf16") for (o, d) in ref.SHAPES]
case = pytest.mark.parametrize("precision,obs_dim,out_dim", CASES)


def _seq(weights, obs_dim, out_dim):
    """A policy-shaped branch on the GPU holding ``weights`` (w1, b1, w2, b2, w3, b3 as numpy)."""
    import torch
    from skyjo_rl_amd.action_mask_model import ActionMaskModel

    seq = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).policy
    with torch.no_grad():
        for p, w in zip(seq.parameters(), weights):
            p.copy_(torch.from_numpy(np.ascontiguousarray(w)))
    return seq.cuda()


def _default_init(obs_dim, out_dim, seed):
    import torch
    from skyjo_rl_amd.action_mask_model import ActionMaskModel

    torch.manual_seed(seed)
    return [p.detach().numpy().copy() for p in ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).policy.parameters()]


def _same(a, b):
    import torch

    return a.shape == b.shape and torch.equal(a, b)


@case
def test_repack_equals_create_equals_ref(precision, obs_dim, out_dim):
    import torch
    from skyjo_rl_amd.action_mask_model import FusedNet

    A, B = _default_init(obs_dim, out_dim, 0), ref.weights_b(obs_dim, out_dim)
    seq_a, seq_b = _seq(A, obs_dim, out_dim), _seq(B, obs_dim, out_dim)
    net = FusedNet(seq_a, precision=precision)
    want = {"A": torch.from_numpy(ref.pack(*A, precision=precision)).cuda(), "B": torch.from_numpy(ref.pack(*B, precision=precision)).cuda()}
    assert _same(net.export(), want["A"])                      # create is what the reference says
    for name, seq in (("B", seq_b), ("A", seq_a), ("B", seq_b)):  # (back and forth on ONE handle: a stale piece would show)
        net.update(seq)
        fresh = FusedNet(seq, precision=precision)
        got = net.export()
        assert _same(got, fresh.export()), name
        assert _same(got, want[name]), name
        fresh.close()
    net.close()


def test_two_creates_back_to_back_keep_their_own_bytes():
    """Nothing of one create (its staging area, its launch) outlives the call: the first net is read after the second exists."""
    import torch
    from skyjo_rl_amd.action_mask_model import FusedNet

    cases = (("fp32", 31, 26, 0), ("bf16", 1, 32, 1))
    weights = [_default_init(o, d, seed) for _, o, d, seed in cases]
    nets = [FusedNet(_seq(w, o, d), precision=p) for w, (p, o, d, _) in zip(weights, cases)]
    for net, w, (p, _, _, _) in zip(nets, weights, cases):
        assert _same(net.export(), torch.from_numpy(ref.pack(*w, precision=p)).cuda()), p
        net.close()


@case
def test_outputs_after_update_are_a_fresh_nets(precision, obs_dim, out_dim):
    import torch
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import FusedNet

    env = SkyjoVecEnv(128, num_players=4)
    env.seed(None, 3)
    rec = env.reset()
    seq_a, seq_c = _seq(_default_init(obs_dim, out_dim, 0), obs_dim, out_dim), _seq(_default_init(obs_dim, out_dim, 1), obs_dim, out_dim)
    net, fresh = FusedNet(seq_a, precision=precision), FusedNet(seq_c, precision=precision)
    before = net(rec)
    net.update(seq_c)
    after = net(rec)  # (queued behind the update on the same stream: no synchronisation between the two)
    want = fresh(rec)
    assert torch.equal(after, want) and not torch.equal(before, want)
    if (precision, obs_dim, out_dim) == ("fp32", 31, 26):  # the tile-planar read of the same records
        rb = rec.shape[-1]
        planar = rec.view(2, 64, rb // 16, 16).permute(0, 2, 1, 3).contiguous()
        assert torch.equal(net(planar, planar=True), want)
    net.close(), fresh.close(), env.close()


_RUNS = {}


def _adam_run(precision, obs_dim, out_dim):
    """ADAM_STEPS steps of NativeAdam on hand-made gradients; what the two Adam tests look at, computed once per case."""
    key = (precision, obs_dim, out_dim)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam

    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).cuda()
    nets = [FusedNet(model.policy, precision=precision), FusedNet(model.value, precision=precision)]
    opt = NativeAdam(model, nets[0], nets[1], **ref.ADAM_HYPER)
    branches = [list(model.policy.parameters()), list(model.value.parameters())]
    zero_p = branches[0][ref.ADAM_ZERO_TENSOR].detach().clone()
    frag, packed = [], []
    for t in range(1, ref.ADAM_STEPS + 1):
        for b, params in enumerate(branches):
            for p, g in zip(params, ref.adam_grads([tuple(p.shape) for p in params], t, seed=77 + b)):
                p.grad = torch.from_numpy(g).cuda()
        opt.step()
        for b, seq in enumerate((model.policy, model.value)):
            fresh = FusedNet(seq, precision=precision)  # (created from the parameters as they now are, read back)
            frag.append((t, b, _same(nets[b].export(), fresh.export())))
            fresh.close()
            want = ref.pack(*[p.detach().cpu().numpy() for p in branches[b]], precision=precision)  # (the layout's own statement)
            packed.append((t, b, _same(nets[b].export(), torch.from_numpy(want).cuda())))
    pol = branches[0]
    _RUNS[key] = {"frag": frag, "packed": packed, "steps": opt.steps,
                  "p": [p.detach().cpu().numpy() for p in pol],
                  "exp_avg": [opt.state[p]["exp_avg"].cpu().numpy() for p in pol],
                  "exp_avg_sq": [opt.state[p]["exp_avg_sq"].cpu().numpy() for p in pol],
                  "zero_unchanged": bool((pol[ref.ADAM_ZERO_TENSOR].detach().view(torch.int32) == zero_p.view(torch.int32)).all())}
    for n in nets:
        n.close()
    return _RUNS[key]


@case
def test_adam_fragments_are_a_fresh_nets_after_every_step(precision, obs_dim, out_dim):
    run = _adam_run(precision, obs_dim, out_dim)
    assert run["steps"] == ref.ADAM_STEPS and len(run["frag"]) == 2 * ref.ADAM_STEPS
    assert all(ok for _, _, ok in run["frag"]), run["frag"]
    assert len(run["packed"]) == 2 * ref.ADAM_STEPS and all(ok for _, _, ok in run["packed"]), run["packed"]


@case
def test_adam_values_against_float64_and_torch(precision, obs_dim, out_dim):
    """d_ours <= 4 d_torch per tensor, for p, exp_avg and exp_avg_sq after step 3 (distances to the float64 rule); where torch's is 0
    ours is 0.  The margin covers equally valid orders of the same few float32 operations; a wrong rule is off by orders of magnitude."""
    run, want = _adam_run(precision, obs_dim, out_dim), adam_reference(obs_dim, out_dim)
    assert run["zero_unchanged"]  # zero gradient, zero state: not a bit moves
    for what, exact in (("p", want["p64"]), ("exp_avg", want["m64"]), ("exp_avg_sq", want["v64"])):
        for i in range(6):
            d_ours, d_torch = float(np.abs(run[what][i].astype(np.float64) - exact[i]).max()), want["d_torch"][what][i]
            print("ADAM_RATIO %s %d %d %s tensor %d: d_ours %.3e d_torch %.3e ratio %s" % (
                precision, obs_dim, out_dim, what, i, d_ours, d_torch, "%.3f" % (d_ours / d_torch) if d_torch else "-"))
            assert d_ours <= 4.0 * d_torch, (what, i, d_ours, d_torch)


def test_loop_closes_in_place():
    import torch
    from examples.ppo import ppo_update, repack
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel
    from skyjo_rl_amd.learner import NativeAdam
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(0)
    B, N, T = 256, 3, 96
    env = SkyjoVecEnv(B, num_players=N)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = repack(model)
    handles = (pol._h.value, val._h.value)
    buf, buf_y = RolloutBuffer(env, T), RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    snap = env.snapshot()
    before = [p.detach().clone() for p in model.parameters()]
    out = ppo_update(model, buf, NativeAdam(model, pol, val, lr=3e-4), epochs=1, minibatch=4096, gae=(0.99, 0.95), native_batches=True,
                     native_loss=True)
    assert out["transitions"] > 4096  # (more than one step)
    collect(env, pol, val, buf, seed=1, first_ticket=T)  # X: the same two objects, nothing between the last step() and here
    assert (pol._h.value, val._h.value) == handles
    assert all(float((p.detach() - q).abs().max()) > 0 for p, q in zip(model.parameters(), before))
    env.restore(snap)
    pol2, val2 = repack(model)
    collect(env, pol2, val2, buf_y, seed=1, first_ticket=T)  # Y: new nets from the host, the parent commit's way
    for name in ("actions", "logp", "values"):
        assert torch.equal(getattr(buf, name), getattr(buf_y, name)), name
    assert torch.equal(buf.records, buf_y.records)
    for n in (pol, val, pol2, val2):
        n.close()
    snap.close(), env.close()


@case
def test_validation_leaves_the_net_unchanged(precision, obs_dim, out_dim):
    import torch
    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam

    torch.manual_seed(0)
    model = ActionMaskModel(obs_dim=obs_dim, num_outputs=out_dim).cuda()
    seq = model.policy
    net, vnet = FusedNet(seq, precision=precision), FusedNet(model.value, precision=precision)
    before = net.export()
    f64 = copy.deepcopy(seq).double()
    transposed = copy.deepcopy(seq)
    transposed[2].weight.data = transposed[2].weight.data.t()
    assert not transposed[2].weight.is_contiguous()
    other = ActionMaskModel(obs_dim=obs_dim % 31 + 1, num_outputs=out_dim).policy.cuda()
    for bad in (f64, transposed, copy.deepcopy(seq).cpu(), other):
        with pytest.raises(ValueError):
            net.update(bad)
    closed = FusedNet(seq, precision=precision)
    closed.close()
    with pytest.raises(ValueError):
        closed.update(seq)
    with pytest.raises(ValueError):
        NativeAdam(model, closed, vnet)

    L = _lib.load()
    params = list(seq.parameters())
    p0 = [p.detach().clone() for p in params]
    grads = [torch.ones_like(p) for p in params]
    nbytes = int(L.skyjo_vec_mlp_adam_state_bytes(net._h))
    assert nbytes >= 8 * sum(p.numel() for p in params) and nbytes % 16 == 0
    state = torch.zeros((nbytes // 4,), dtype=torch.float32, device="cuda")
    pp, gg = (C.c_void_p * 6)(*[p.data_ptr() for p in params]), (C.c_void_p * 6)(*[g.data_ptr() for g in grads])
    ok = dict(state_bytes=nbytes, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1)
    for change in (dict(state_bytes=nbytes - 4), dict(step=0), dict(step=-3), dict(lr=float("inf")), dict(lr=float("nan")), dict(beta1=1.0),
                   dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(beta2=-1e-3)):
        a = dict(ok, **change)
        rc = L.skyjo_vec_mlp_adam_step(net._h, pp, gg, state.data_ptr(), a["state_bytes"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["step"],
                                       torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and len(L.skyjo_vec_last_error()) > 10, change
    # the same through the class: a gradient that is missing, a learning rate that is not a number
    opt = NativeAdam(model, net, vnet, lr=1e-3)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.lr = float("inf")
    with pytest.raises(_lib.SkyjoNativeError):
        opt.step()
    opt.lr = 1e-3
    params[3].grad = None
    with pytest.raises(ValueError):
        opt.step()
    assert opt.steps == 0
    assert _same(net.export(), before) and not bool(state.any())
    assert all(torch.equal(p.detach(), q) for p, q in zip(params, p0))
    opt.zero_grad()
    assert all(p.grad is None for p in model.parameters())
    net.close(), vnet.close()
