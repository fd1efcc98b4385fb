"""The native PPO update, step by step: ``examples/ppo.py::ppo_update(native_batches=True, native_loss=True, native_nets=True)`` with a
``learner.NativeAdam`` (A), its ``kl=`` form on a tile-planar buffer (B) and ``ppo_update_per_seat`` on an ``arena.collect`` buffer (C) are
RECORDED - the minibatches as they are yielded, the loss head's inputs and outputs, and around every ``NativeAdam.step()`` the parameters,
their gradients, the Adam state, the step count and both nets' fragments - and every step of the record is compared with the
teacher-forced float64 restatement of tests/ppo_step_ref.py (``check_run``; the bounds are stated there: 4 x torch's own float32
evaluation of the same step, bit for bit where nothing is computed).  ``examples/ppo.py`` is not changed: the record is taken by
wrapping the names it calls.  The shuffle is reproduced here - ``torch.Generator(device).manual_seed(seed)``, one ``torch.randperm`` per
epoch over the ascending selection - from the buffer's flags, not read from the code under test.

Shape: 256 games (four record tiles), three players, T = 64, two epochs, a minibatch size chosen from the selection's count such that an
epoch has at least four minibatches and a short last one whose row count is no multiple of 64 (the training kernels' tile), and
``ent_coef`` = 0.01, ``vf_clip`` = 0.2: both optional terms of the head are live.

One synthetic case beside them: ``skyjo_vec_mlp_adam_step`` through the C ABI on hand-made non-zero state at step 1, 7, 1000, 10^6 and
2^31 + 5 - the bias corrections far beyond the three steps of tests/test_gpu_mlp_update.py."""
import ctypes as C

import numpy as np
import pytest

from tests import mlp_pack_ref
from tests import ppo_step_ref as ref

pytestmark = pytest.mark.gpu

B, N, T, EPOCHS, SEED = 256, 3, 64, 2, 11
GAE = (0.99, 0.95)
HEAD = dict(clip=0.3, vf_coef=1.0, ent_coef=0.01, vf_clip=0.2)
LR = 3e-4


def _np(t):
    return t.detach().cpu().numpy().copy()


def _minibatch_size(counts, lo=1000):
    """The first size from ``lo`` up for which every selection has at least four minibatches per epoch and a short last one whose row
    count is no multiple of 64."""
    for size in range(lo, lo + 64):
        if all(-(-c // size) >= 4 and (c % size) % 64 != 0 for c in counts):
            return size
    raise AssertionError("no minibatch size for %r" % (counts,))


class _Learner:
    """One model with its nets and its NativeAdam, and what the record needs of it."""

    def __init__(self, key, model, pol, val, opt, seat=None):
        self.key, self.model, self.pol, self.val, self.opt, self.seat = key, model, pol, val, opt, seat
        self.branches = {"policy": list(model.policy.parameters()), "value": list(model.value.parameters())}
        self.nets = {"policy": pol, "value": val}

    def snapshot(self, grads=False, export=False):
        s = {"params": {b: [_np(p) for p in ps] for b, ps in self.branches.items()},
             "exp_avg": {b: [_np(self.opt.state[p]["exp_avg"]) for p in ps] for b, ps in self.branches.items()},
             "exp_avg_sq": {b: [_np(self.opt.state[p]["exp_avg_sq"]) for p in ps] for b, ps in self.branches.items()}}
        if grads:
            s["grads"] = {b: [_np(p.grad) for p in ps] for b, ps in self.branches.items()}
        if export:
            s["export"] = {b: _np(net.export()) for b, net in self.nets.items()}
        return s

    def everything(self):
        """name -> array of all that another learner's step must not touch."""
        s = self.snapshot(export=True)
        out = {"learner %s %s %s %s" % (self.key, what, b, k): a for what in ("params", "exp_avg", "exp_avg_sq") for b in ref.BRANCHES
               for k, a in zip(ref.PARAMS, s[what][b])}
        out.update({"learner %s fragments %s" % (self.key, b): s["export"][b] for b in ref.BRANCHES})
        return out


class _Recorder:
    """Wraps ``examples.ppo``'s ``minibatches``, ``ppo_loss`` / ``ppo_loss_kl`` and every learner's ``opt.step``; ``steps`` is the record."""

    def __init__(self, monkeypatch, learners):
        from examples import ppo

        self.learners, self.steps, self.pending, self.yielded = learners, [], None, None
        real_mb, real_loss, real_kl = ppo.minibatches, ppo.ppo_loss, ppo.ppo_loss_kl

        def minibatches(buf, size, **kw):
            for item in real_mb(buf, size, **kw):
                mb, old = item if kw.get("behaviour") else (item, None)
                self.yielded = (mb, old)
                self.pending = {"mb": {name: _np(col) for name, col in zip(ref.COLUMNS, mb)}, "old_logits": None if old is None else _np(old)}
                yield item                                     # (what the update gets is the object itself, not the clone)

        def loss(real):
            def wrapped(logits, value, mb, *args, **kw):
                res = real(logits, value, mb, *args, **kw)
                self.pending.update(logits=_np(logits), value=_np(value), stats=_np(res.stats), grad_logits=_np(res.grad_logits), grad_value=_np(res.grad_value))
                return res
            return wrapped

        monkeypatch.setattr(ppo, "minibatches", minibatches)
        monkeypatch.setattr(ppo, "ppo_loss", loss(real_loss))
        monkeypatch.setattr(ppo, "ppo_loss_kl", loss(real_kl))
        for ln in learners:
            ln.opt.step = self._step(ln, ln.opt.step)

    def _held(self):
        """The Minibatch (and old_logits) as the update holds them now."""
        mb, old = self.yielded
        out = {"minibatch " + name: _np(col) for name, col in zip(ref.COLUMNS, mb)}
        if old is not None:
            out["minibatch old_logits"] = _np(old)
        return out

    def _step(self, ln, real):
        def step():
            rec, self.pending = self.pending, None
            assert rec is not None and "logits" in rec, "a step without a minibatch and a loss of its own"
            others = [o for o in self.learners if o is not ln]
            before = ln.snapshot(grads=True)
            rec["bystanders_before"] = {"minibatch " + k: v for k, v in rec["mb"].items()}
            if rec["old_logits"] is not None:
                rec["bystanders_before"]["minibatch old_logits"] = rec["old_logits"]
            for o in others:
                rec["bystanders_before"].update(o.everything())
            t = ln.opt.steps + 1
            real()
            after = ln.snapshot(export=True)
            rec["bystanders_after"] = self._held()
            for o in others:
                rec["bystanders_after"].update(o.everything())
            assert ln.opt.steps == t
            rec.update(learner=ln.key, t=t, grads=before.pop("grads"), before=before, export=after.pop("export"), after=after)
            self.steps.append(rec)
        return step


def _buffer_dict(buf):
    e = buf._env
    beh = getattr(buf, "behaviour", None)
    return dict(records=_np(buf.records), planar=buf.planar, rec_bytes=e.record_bytes, D=e.obs_dim, B=buf.B, T=buf.T, stride=e.tiles * 64 if buf.planar else buf.B,
                actions=_np(buf.actions), logp=_np(buf.logp), values=_np(buf.values[..., 0]), advantages=_np(buf.advantages), value_targets=_np(buf.value_targets),
                behaviour=None if beh is None else _np(beh))


def _columns(buf):
    return [(name, _np(getattr(buf, name))) for name in ("records", "actions", "logp", "values", "advantages", "value_targets", "target_flags", "final_rewards", "episode_end")]


def _selections(buf, learners):
    """Per learner (selection, mean, std), restated from the buffer's flags, agent bytes and advantages."""
    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.rollout import compute_targets

    compute_targets(buf, gamma=GAE[0], lam=GAE[1])
    flags, adv = _np(buf.target_flags), _np(buf.advantages)
    agent = _np(buf.views().agent[: buf.T])
    out = {}
    for ln in learners:
        sel = ref.select(flags, _lib.TGT_HAS_TARGET, agent, None if ln.seat is None else (ln.seat,))
        out[ln.key] = (sel,) + ref.selection_moments(adv, sel)
    return out


def _expected_indices(sel, size, device):
    """The row ids of every minibatch of the update, epoch by epoch: [[index]]."""
    import torch

    gen = torch.Generator(device=device).manual_seed(SEED)
    out = []
    for _ in range(EPOCHS):
        perm = sel[torch.randperm(sel.size, device=device, generator=gen).cpu().numpy()]
        out.append([perm[k:k + size] for k in range(0, sel.size, size)])
    return out


def _run(buf, learners, rec, sels, size, hp, results, before, kls=None, first_params=None):
    """The ``check_run`` dict of a finished, recorded update."""
    run = dict(hyper=hp, precision=learners[0].pol.precision, buffer=_buffer_dict(buf), learners={}, steps=rec.steps,
               untouched=[(name, a, b) for (name, a), (_, b) in zip(before, _columns(buf))])
    for ln in learners:
        sel, mean, std = sels[ln.key]
        mine = [i for i, s in enumerate(rec.steps) if s["learner"] == ln.key]
        want = _expected_indices(sel, size, buf.actions.device)
        per_epoch = len(want[0])
        assert len(mine) == EPOCHS * per_epoch, (ln.key, len(mine), per_epoch)
        assert per_epoch >= 4 and want[0][-1].size == sel.size % size and want[0][-1].size % 64 != 0 and 0 < want[0][-1].size < size
        epochs = [mine[e * per_epoch:(e + 1) * per_epoch] for e in range(EPOCHS)]
        for ep, idx in zip(epochs, want):
            for i, index in zip(ep, idx):
                rec.steps[i]["index"] = index
        run["learners"][ln.key] = dict(selection=sel, mean=mean, std=std, seat=ln.seat, epochs=epochs, out=results[ln.key],
                                       behaviour_params=None if first_params is None else first_params[ln.key], kl=None if kls is None else kls[ln.key])
    assert [s["t"] for s in rec.steps if s["learner"] == learners[0].key] == list(range(1, EPOCHS * len(run["learners"][learners[0].key]["epochs"][0]) + 1))
    return run


def _shared_model_setup(layout):
    import torch

    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(0)
    env = SkyjoVecEnv(B, num_players=N)
    env.set_record_layout(layout)
    env.seed(None, 9)
    env.reset()
    assert env.tiles == 4
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    ln = _Learner(0, model, pol, val, NativeAdam(model, pol, val, lr=LR))
    return env, buf, ln


def _case_a(monkeypatch):
    from examples.ppo import ppo_update

    env, buf, ln = _shared_model_setup("row-major")
    assert not buf.planar
    sels = _selections(buf, [ln])
    size = _minibatch_size([sels[0][0].size])
    before = _columns(buf)
    rec = _Recorder(monkeypatch, [ln])
    out = ppo_update(ln.model, buf, ln.opt, epochs=EPOCHS, minibatch=size, seed=SEED, gae=GAE, native_batches=True, native_loss=True, native_nets=True, **HEAD)
    assert "kl_coeff" not in out and out["transitions"] == sels[0][0].size
    run = _run(buf, [ln], rec, sels, size, ref.hyper(lr=LR, **HEAD), {0: out}, before)
    print("case A: %d rows, minibatch %d, %d steps" % (sels[0][0].size, size, len(rec.steps)))
    ln.pol.close(), ln.val.close(), env.close()
    return run


def _case_b(monkeypatch):
    from examples.ppo import ppo_update
    from skyjo_rl_amd.learner import KLCoeff

    env, buf, ln = _shared_model_setup("tile-planar-all")
    assert buf.planar
    sels = _selections(buf, [ln])
    size = _minibatch_size([sels[0][0].size])
    before = _columns(buf)
    first = {0: [_np(p) for p in ln.branches["policy"]]}         # the parameters of the net that played, before the first step
    rec = _Recorder(monkeypatch, [ln])
    coeff = KLCoeff()
    start = (coeff.coeff, coeff.target)
    out = ppo_update(ln.model, buf, ln.opt, epochs=EPOCHS, minibatch=size, seed=SEED, gae=GAE, native_batches=True, native_loss=True, native_nets=True,
                     kl=coeff, behaviour_net=ln.pol, **HEAD)
    assert out["kl_coeff"] == float(coeff) and out["transitions"] == sels[0][0].size
    run = _run(buf, [ln], rec, sels, size, ref.hyper(lr=LR, kl_coeff=start[0], **HEAD), {0: out}, before, kls={0: start}, first_params=first)
    assert all(s["old_logits"] is not None and s["stats"].shape == (7,) for s in rec.steps)
    print("case B: %d rows, minibatch %d, %d steps, mean_action_kl %.3e, kl_coeff %r" % (sels[0][0].size, size, len(rec.steps), out["mean_action_kl"], out["kl_coeff"]))
    ln.pol.close(), ln.val.close(), env.close()
    return run


def _case_c(monkeypatch):
    import torch

    from examples.ppo import ppo_update_per_seat
    from skyjo_rl_amd import arena
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.learner import NativeAdam
    from skyjo_rl_amd.rollout import RolloutBuffer
    from tests.test_gpu_arena import _engine

    env = _engine(N, B)
    learners = []
    for s in (0, 2):
        torch.manual_seed(20 + s)
        m = ActionMaskModel(obs_dim=31).cuda()
        pol, val = FusedNet(m.policy), FusedNet(m.value)
        learners.append(_Learner(s, m, pol, val, NativeAdam(m, pol, val, lr=LR), seat=s))
    buf = RolloutBuffer(env, T)
    arena.collect(env, [("sample", learners[0].pol), "random", ("sample", learners[1].pol)], [learners[0].val, None, learners[1].val], buf, seed=8, first_ticket=1000)
    sels = _selections(buf, learners)
    size = _minibatch_size([sels[k][0].size for k in (0, 2)])
    before = _columns(buf)
    rec = _Recorder(monkeypatch, learners)
    res = ppo_update_per_seat([learners[0].model, None, learners[1].model], buf, [learners[0].opt, None, learners[1].opt], gae=GAE, native_nets=True, epochs=EPOCHS,
                              minibatch=size, seed=SEED, **HEAD)
    assert res[1] is None and [res[s]["transitions"] for s in (0, 2)] == [sels[s][0].size for s in (0, 2)]
    run = _run(buf, learners, rec, sels, size, ref.hyper(lr=LR, **HEAD), {0: res[0], 2: res[2]}, before)
    # seat 0's steps all come before seat 2's, every row of a step is its seat's, and the other seat is among each step's bystanders
    order = [s["learner"] for s in rec.steps]
    assert order == sorted(order) and set(order) == {0, 2}
    assert all(bool((s["mb"]["seats"] == s["learner"]).all()) for s in rec.steps)
    assert all(any(k.startswith("learner %d fragments" % (2 - s["learner"])) for k in s["bystanders_before"]) for s in rec.steps)
    print("case C: rows %r, minibatch %d, %d steps" % ([sels[k][0].size for k in (0, 2)], size, len(rec.steps)))
    for ln in learners:
        ln.pol.close(), ln.val.close()
    env.close()
    return run


CASES = {"A": _case_a, "B": _case_b, "C": _case_c}
_FAILURES = {}


@pytest.fixture(params=sorted(CASES))
def failures(request):
    """The case's update recorded and compared, once per case: ``check_run``'s failures, every ratio printed."""
    name = request.param
    if name not in _FAILURES:
        with pytest.MonkeyPatch.context() as mp:
            run = CASES[name](mp)
        _FAILURES[name] = ref.check_run(run, log=lambda line: print("case", name, line))
        for f in _FAILURES[name]:
            print("PPO_STEP_FAILURE case", name, f)
    return _FAILURES[name]


def test_every_step_is_the_restatements_bits_gradients_and_adam(failures):
    """Everything but the float outputs' comparison with the yardstick: minibatches, ``old_logits``, fragments, bystanders and the
    buffer bit for bit, every epoch a permutation of the selection, the twelve gradients of every step, Adam over the run, the
    behaviour column against the parameters before the first step, the row count and the coefficient's rule."""
    bad = [f for f in failures if f[0] not in ref.FLOAT_KINDS]
    assert bad == [], "%d failures, the first: %r" % (len(bad), bad[0])


def test_float_outputs_are_within_four_times_torchs_float32_deviation(failures):
    """logits, value, the statistics, grad_logits and grad_value of every step, and the reported means: d_ours <= 4 d_torch.

    The case that made ``k_ppo_loss`` evaluate its rows in double.  With the head in float32 this test failed in all three cases
    (EXPERIMENTS.md): the device's float32 ``logf`` has a mean SIGNED error of -7.0e-08 on the sums of a masked softmax, which does not
    average out over rows - the epoch mean of ``kl`` was 4.4e-08 ... 4.8e-08 off where the yardstick is off by 1.9e-09 ... 3.9e-09
    (ratios 12 ... 23), and the same error stood in the per-step statistics (ratios up to 20.3) - and grad_logits exceeded 4 on 5 of 88
    steps (up to 8.36).  Measured since: grad_logits 2.61, the statistics 0.61, the epoch means 1.45, ``mean_action_kl`` 0.001."""
    bad = [f for f in failures if f[0] in ref.FLOAT_KINDS]
    assert bad == [], "%d failures, the first: %r" % (len(bad), bad[0])


def test_adam_step_far_beyond_three_steps():
    """``skyjo_vec_mlp_adam_step`` through the C ABI on hand-made non-zero state, one step each at ``ADAM_FAR_STEPS`` from the same start:
    p, exp_avg and exp_avg_sq against ``adam_ref`` with d_ours <= 4 d_torch per tensor, both the largest over the steps; where torch's is 0
    (the tensor whose gradient and state are zero) ours is 0.  The fragments are ``pack`` of the parameters read back."""
    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet

    L = _lib.load()
    hp = ref.ADAM_FAR_HYPER
    p0, g0, m0, v0 = ref.adam_inputs()
    seq = ActionMaskModel(obs_dim=p0[0].shape[1], num_outputs=p0[4].shape[0]).policy.cuda()
    params = list(seq.parameters())
    net = FusedNet(seq)
    n = int(L.skyjo_vec_mlp_adam_state_bytes(net._h)) // 4
    total = sum(p.size for p in p0)
    assert n % 2 == 0 and n // 2 >= total
    flat = lambda arrays: np.concatenate([a.reshape(-1) for a in arrays] + [np.zeros(n // 2 - total, dtype=np.float32)])
    state0 = torch.from_numpy(np.concatenate([flat(m0), flat(v0)])).cuda()
    grads = [torch.from_numpy(g).cuda() for g in g0]
    pp, gg = (C.c_void_p * 6)(*[p.data_ptr() for p in params]), (C.c_void_p * 6)(*[g.data_ptr() for g in grads])
    worst = {}
    for t in ref.ADAM_FAR_STEPS:
        state = state0.clone()
        with torch.no_grad():
            for p, w in zip(params, p0):
                p.copy_(torch.from_numpy(w))
        _lib.check(L.skyjo_vec_mlp_adam_step(net._h, pp, gg, state.data_ptr(), n * 4, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], t,
                                             torch.cuda.current_stream().cuda_stream))
        host = state.cpu().numpy()
        got_p = [_np(p) for p in params]
        got = {"p": got_p, "exp_avg": [], "exp_avg_sq": []}
        at = 0
        for w in p0:
            got["exp_avg"].append(host[at:at + w.size].reshape(w.shape)), got["exp_avg_sq"].append(host[n // 2 + at:n // 2 + at + w.size].reshape(w.shape))
            at += w.size
        assert not host[total:n // 2].any() and not host[n // 2 + total:].any()       # the padding stays zero
        assert ref.same_bits(_np(net.export()), mlp_pack_ref.pack(*got_p, precision=net.precision)), t
        want, yard = ref.adam(p0, g0, m0, v0, hp, t), ref.torch_adam(p0, g0, m0, v0, hp, t)
        for what, w3, y3 in zip(ref.ADAM_OUTPUTS, want, yard):
            for k, a, w, y in zip(ref.PARAMS, got[what], w3, y3):
                mx = worst.setdefault((what, k), [0.0, 0.0])
                d_ours, d_torch = ref.deviation(a.astype(np.float64), w), ref.deviation(y, w)
                print("ADAM_FAR step %d %s %s: d_ours %.3e d_torch %.3e" % (t, what, k, d_ours, d_torch))
                mx[0], mx[1] = max(mx[0], d_ours), max(mx[1], d_torch)
    for (what, k), (d_ours, d_torch) in worst.items():
        print("ADAM_FAR_RATIO %s %s: d_ours %.3e d_torch %.3e ratio %s" % (what, k, d_ours, d_torch, "%.3f" % (d_ours / d_torch) if d_torch else "-"))
        assert d_ours <= ref.MARGIN * d_torch, (what, k, d_ours, d_torch)
    net.close()
