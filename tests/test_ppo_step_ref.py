"""tests/ppo_step_ref.py without a GPU: the float64 step against torch's float64 autograd and ``torch.optim.Adam``, and the checker
``check_run`` against simulated updates - a correct float32 evaluation that is not its yardstick (numpy float32 matmuls, split sums),
which it must accept, and six wrong updates, each differing from the correct one in exactly one thing, which it must reject."""
import ast
import functools
import os

import numpy as np
import pytest

from tests import mlp_pack_ref, mlp_train_ref
from tests import ppo_loss_kl_synth as kl_synth
from tests import ppo_loss_synth as synth
from tests import ppo_step_ref as ref

F32 = np.float32
POLICY, VALUE = (31, 26), (31, 1)
BOUND = 1e-12


def _start():
    return {"policy": [np.array(p) for p in mlp_train_ref.weights(POLICY, "A")], "value": [np.array(p) for p in mlp_train_ref.weights(VALUE, "A")]}


def _zeros(params, dtype):
    return {b: [np.zeros(p.shape, dtype=dtype) for p in params[b]] for b in ref.BRANCHES}


def _forward64(p, x):
    return mlp_train_ref.forward_backward(p, x, np.zeros((x.shape[0], p[4].shape[0])))["out"]


# ---------------------------------------------------------------- 1. the helper stands alone
def test_the_helper_imports_nothing_from_the_package():
    tree = ast.parse(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ppo_step_ref.py")).read())
    names = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names += [a.name for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            names += [(node.module or "") + "." + a.name for a in node.names]
    assert names and not [n for n in names if n.split(".")[0] in ("skyjo_rl_amd", "examples")], names
    assert all(n.split(".")[0] in ("numpy", "torch", "tests") for n in names), names


# ---------------------------------------------------------------- 2. the restatement against float64 autograd
def _synthetic_minibatch(m, start):
    """``ppo_loss_synth.make(m)`` on the features of ``mlp_train_ref.inputs``: the batch's rows keep their places relative to the bounds
    (the ratio around 1 +- clip, v - v_old around +- vf_clip, the old logits' relation to the new) with the NET's outputs on x in the
    place of the batch's own ``logits`` and ``value``.  Returns (minibatch dict, old_logits)."""
    b = kl_synth.make(m)
    x = np.array(mlp_train_ref.inputs(POLICY, m)[0])
    logits = _forward64(start["policy"], x).astype(F32)
    value = _forward64(start["value"], x).reshape(m).astype(F32)
    lp = lambda lg: ref.ppo_loss_ref.ppo_loss(lg, b.log_mask, b.value, b.actions, b.logp, b.advantages, b.value_targets, b.values)["logp"][np.arange(m), b.actions]
    logp = (lp(logits) - (lp(b.logits) - b.logp.astype(np.float64))).astype(F32)
    values = (value.astype(np.float64) - (b.value.astype(np.float64) - b.values.astype(np.float64))).astype(F32)
    old = (logits.astype(np.float64) + (b.old_logits.astype(np.float64) - b.logits.astype(np.float64))).astype(F32)
    mb = dict(observations=x, log_mask=b.log_mask, actions=b.actions, logp=logp, advantages=b.advantages, value_targets=b.value_targets, values=values,
              seats=np.zeros(m, dtype=np.uint8))
    return mb, old


@pytest.mark.parametrize("kl", [False, True], ids=["plain", "kl"])
def test_five_consecutive_steps_equal_float64_autograd_and_torch_adam(kl):
    import torch

    hp = ref.hyper(ent_coef=0.01, vf_clip=0.2, kl_coeff=0.2 if kl else None)
    start = _start()
    state = {"params": start, "exp_avg": _zeros(start, np.float64), "exp_avg_sq": _zeros(start, np.float64), "t": 1}
    leaves = {b: [torch.from_numpy(p.astype(np.float64)).requires_grad_() for p in start[b]] for b in ref.BRANCHES}
    opt = torch.optim.Adam([p for b in ref.BRANCHES for p in leaves[b]], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], foreach=False)
    worst = {}
    for m in (65, 127, 256, 257, 63):
        mb, old = _synthetic_minibatch(m, start)
        got = ref.step(state, mb, hp, old if kl else None)
        now = {b: [p.detach().numpy() for p in leaves[b]] for b in ref.BRANCHES}
        want = ref.torch_step(now, mb, hp, old if kl else None, dtype=torch.float64)
        assert got["stats"].shape == (7 if kl else 6,) and got["logits"].shape == (m, 26) and got["value"].shape == (m,)
        pairs = [(k, got[k], want[k]) for k in ("logits", "value", "stats", "grad_logits", "grad_value")]
        pairs += [("grad %s %s" % (b, k), g, w) for b in ref.BRANCHES for k, g, w in zip(ref.PARAMS, got["grads"][b], want["grads"][b])]
        for b in ref.BRANCHES:
            for p, g in zip(leaves[b], want["grads"][b]):
                p.grad = torch.from_numpy(g.copy())
        opt.step()
        for b in ref.BRANCHES:
            for k, p, i in zip(ref.PARAMS, leaves[b], range(6)):
                pairs += [("p %s %s" % (b, k), got["next"]["params"][b][i], p.detach().numpy()),
                          ("exp_avg %s %s" % (b, k), got["next"]["exp_avg"][b][i], opt.state[p]["exp_avg"].numpy()),
                          ("exp_avg_sq %s %s" % (b, k), got["next"]["exp_avg_sq"][b][i], opt.state[p]["exp_avg_sq"].numpy())]
        for name, g, w in pairs:
            d = ref.deviation(g, w)
            worst[name.split()[0]] = max(worst.get(name.split()[0], 0.0), d)
            assert d <= BOUND, (m, state["t"], name, d)
        assert got["next"]["t"] == state["t"] + 1
        state = got["next"]
    print("largest normalised deviation from float64 torch:", {k: "%.2e" % v for k, v in worst.items()})
    assert state["t"] == 6
    assert all(float(np.abs(p - q).max()) > 0 for b in ref.BRANCHES for p, q in zip(state["params"][b], start[b]))  # (every tensor moved)


def test_the_yardstick_is_the_float32_action_mask_model():
    """``torch_step`` spells the branches with ``nn.functional``: the same bits as ``ActionMaskModel``'s own modules and autograd."""
    import torch

    from skyjo_rl_amd.action_mask_model import ActionMaskModel

    hp = ref.hyper(ent_coef=0.01, vf_clip=0.2)
    start = _start()
    mb, _ = _synthetic_minibatch(257, start)
    got = ref.torch_step(start, mb, hp)
    model = ActionMaskModel(obs_dim=31)
    with torch.no_grad():
        for seq, b in ((model.policy, "policy"), (model.value, "value")):
            for p, w in zip(seq.parameters(), start[b]):
                p.copy_(torch.from_numpy(w))
    t = lambda a: torch.from_numpy(np.array(a))
    x = t(mb["observations"])
    logits = model.policy(x)
    loss, stats = synth.torch_head(logits, t(mb["log_mask"]), model.value(x).squeeze(-1), t(mb["actions"]), t(mb["logp"]), t(mb["advantages"]),
                                   t(mb["value_targets"]), t(mb["values"]), clip=hp["clip"], vf_coef=hp["vf_coef"], ent_coef=hp["ent_coef"], vf_clip=hp["vf_clip"])
    loss.backward()
    assert np.array_equal(got["logits"], logits.detach().double().numpy()) and got["stats"][0] == float(stats[0])
    for seq, b in ((model.policy, "policy"), (model.value, "value")):
        for k, p, g in zip(ref.PARAMS, seq.parameters(), got["grads"][b]):
            assert np.array_equal(g, p.grad.double().numpy()), (b, k)


def test_adam_far_steps_equal_torch_in_float64():
    """The synthetic Adam case's reference at steps far beyond three: ``adam`` against ``torch.optim.Adam`` in float64."""
    import torch

    p, g, m, v = ref.adam_inputs()
    for t in ref.ADAM_FAR_STEPS:
        want = ref.adam(p, g, m, v, ref.ADAM_FAR_HYPER, t)
        got = ref.torch_adam(p, g, m, v, ref.ADAM_FAR_HYPER, t, dtype=torch.float64)
        for what, w3, g3 in zip(ref.ADAM_OUTPUTS, want, got):
            for k, a, b in zip(ref.PARAMS, g3, w3):
                assert ref.deviation(a, b) <= BOUND, (t, what, k)
    # the steps tell each other apart: the bias corrections at 1, 7 and 1000 are not those of a step far away
    ps = [np.concatenate([x.reshape(-1) for x in ref.adam(p, g, m, v, ref.ADAM_FAR_HYPER, t)[0]]) for t in ref.ADAM_FAR_STEPS]
    assert all(float(np.abs(ps[i] - ps[j]).max()) > 1e-5 for i in range(3) for j in range(i + 1, 4))


# ---------------------------------------------------------------- 3. a simulated update: float32 numpy, another summation order
T, B, REC_BYTES, MINIBATCH, EPOCHS = 6, 130, 64, 200, 2


def _mm(a, b):
    """a @ b in float32 with the sum over k split in two halves: another order than one matmul's."""
    h = a.shape[1] // 2
    return (a[:, :h] @ b[:h] + a[:, h:] @ b[h:]).astype(F32) if h else (a @ b).astype(F32)


def _rows(fn, n, chunk=64):
    """sum over row chunks of fn(lo, hi), float32 partials added in order."""
    out = None
    for lo in range(0, n, chunk):
        part = fn(lo, min(lo + chunk, n)).astype(F32)
        out = part if out is None else (out + part).astype(F32)
    return out


def _forward32(p, x):
    w1, b1, w2, b2, w3, b3 = p
    h1 = np.tanh((_mm(x, w1.T.copy()) + b1).astype(F32))
    h2 = np.tanh((_mm(h1, w2.T.copy()) + b2).astype(F32))
    return (_mm(h2, w3.T.copy()) + b3).astype(F32), h1, h2


def _backward32(p, x, h1, h2, g):
    w1, b1, w2, b2, w3, b3 = p
    n = x.shape[0]
    one = F32(1.0)
    dz2 = (_mm(g, w3) * (one - h2 * h2)).astype(F32)
    dz1 = (_mm(dz2, w2) * (one - h1 * h1)).astype(F32)
    tw = lambda a, b: _rows(lambda lo, hi: a[lo:hi].T @ b[lo:hi], n)
    sm = lambda a: _rows(lambda lo, hi: a[lo:hi].sum(axis=0), n)
    return [tw(dz1, x), sm(dz1), tw(dz2, h1), sm(dz2), tw(g, h2), sm(g)]


def _adam32(p, g, m, v, hp, t):
    """The documented rule in float32 operations, textbook order (not torch's)."""
    b1, b2 = hp["betas"]
    m = (F32(b1) * m + F32(1.0 - b1) * g).astype(F32)
    v = (F32(b2) * v + F32(1.0 - b2) * (g * g)).astype(F32)
    denom = (np.sqrt(v) / F32(np.sqrt(1.0 - b2 ** t)) + F32(hp["eps"])).astype(F32)
    return (p - F32(hp["lr"] / (1.0 - b1 ** t)) * (m / denom)).astype(F32), m, v


@functools.lru_cache(maxsize=None)
def _buffer():
    """A row-major buffer of T x B hand-made records (31 observation bytes, 26 mask bytes at 32, the seat at 58) with learner columns
    that fit the starting net: logp near its log-probabilities, values near its value estimates."""
    rng = np.random.default_rng(2024)
    start = _start()
    rec = np.zeros((T, B, REC_BYTES), dtype=np.uint8)
    rec[..., :31] = rng.integers(-2, 13, (T, B, 31)).astype(np.int8).view(np.uint8)
    legal = rng.random((T, B, 26)) < 0.4
    first = rng.integers(0, 26, (T, B))
    np.put_along_axis(legal, first[..., None], True, axis=2)
    rec[..., 32:58] = legal
    rec[..., 58] = np.arange(B) % 3
    actions = np.where(legal, rng.random((T, B, 26)), -1.0).argmax(axis=2).astype(np.int32)
    x = rec[..., :31].view(np.int8).astype(F32).reshape(-1, 31)
    z = _forward64(start["policy"], x) + np.where(legal.reshape(-1, 26), 0.0, float(np.finfo(F32).min))
    z = z - z.max(axis=1, keepdims=True)
    lp = (z - np.log(np.exp(z).sum(axis=1, keepdims=True)))[np.arange(T * B), actions.reshape(-1)]
    v = _forward64(start["value"], x).reshape(-1)
    flags = (rng.random((T, B)) < 0.9).astype(np.uint8) | np.uint8(2)
    buf = dict(records=rec, planar=False, rec_bytes=REC_BYTES, D=31, B=B, T=T, stride=B, actions=actions,
               logp=(lp + rng.uniform(-0.4, 0.4, T * B)).astype(F32).reshape(T, B), values=(v + rng.normal(0.0, 0.3, T * B)).astype(F32).reshape(T, B),
               advantages=rng.normal(0.5, 2.0, (T, B)).astype(F32), value_targets=(v + rng.normal(0.0, 1.0, T * B)).astype(F32).reshape(T, B),
               behaviour=None)
    return buf, flags


def _simulate(variant=None, kl=False, behaviour=None):
    """A recorded update as tests/test_gpu_ppo_step.py records one, computed here in numpy float32.  ``variant``: None - correct; "a" .. "f"
    - the wrong updates of the tests below."""
    buf, flags = _buffer()
    buf = dict(buf)
    hp = ref.hyper(ent_coef=0.01, vf_clip=0.2, kl_coeff=0.2 if kl else None)
    params = _start()
    m_, v_ = _zeros(params, F32), _zeros(params, F32)
    x_all = ref.gather_expected(buf, np.arange(T * B))["observations"]
    if kl:
        buf["behaviour"] = (_forward32(params["policy"], x_all)[0] if behaviour is None else behaviour).reshape(T, B, 26)
    sel = ref.select(flags, 1)
    mean, std = ref.selection_moments(buf["advantages"], sel)
    assert -(-sel.size // MINIBATCH) >= 4 and (sel.size % MINIBATCH) % 64 != 0
    rng = np.random.default_rng(5)
    learner = dict(selection=sel, mean=mean, std=std, seat=None, behaviour_params=[p.copy() for p in params["policy"]], epochs=[], kl=(0.2, 0.01) if kl else None)
    steps, t, prev_x = [], 0, None
    per_epoch = []
    for ep in range(EPOCHS):
        perm = sel[rng.permutation(sel.size)]
        learner["epochs"].append([])
        tot, seen = 0.0, 0
        for k in range(0, sel.size, MINIBATCH):
            index = perm[k:k + MINIBATCH]
            g = ref.gather_expected(buf, index, mean, std)
            old = g.pop("old_logits", None)
            x, n = g["observations"], index.size
            before = {"params": {b: [p.copy() for p in params[b]] for b in ref.BRANCHES}, "exp_avg": {b: [a.copy() for a in m_[b]] for b in ref.BRANCHES},
                      "exp_avg_sq": {b: [a.copy() for a in v_[b]] for b in ref.BRANCHES}}
            logits, ph1, ph2 = _forward32(params["policy"], x)
            value, vh1, vh2 = _forward32(params["value"], x)
            h = ref.head(logits, value, g, hp, old)
            gl, gv = h["grad_logits"].astype(F32), h["grad_value"].astype(F32)
            if variant == "c" and n < MINIBATCH:
                gl, gv = (gl * F32(n / MINIBATCH)).astype(F32), (gv * F32(n / MINIBATCH)).astype(F32)
            xb = prev_x if variant == "d" and prev_x is not None and prev_x.shape == x.shape else x
            grads = {"policy": _backward32(params["policy"], xb, ph1, ph2, gl), "value": _backward32(params["value"], xb, vh1, vh2, gv.reshape(n, 1))}
            t += 1
            for b in ref.BRANCHES:
                for i in range(6):
                    gi = grads["value"][2] if variant == "b" and (b, i) == ("policy", 2) else grads[b][i]
                    params[b][i], m_[b][i], v_[b][i] = _adam32(params[b][i], gi, m_[b][i], v_[b][i], hp, 1 if variant == "a" else t)
            after = {"params": {b: [p.copy() for p in params[b]] for b in ref.BRANCHES}, "exp_avg": {b: [a.copy() for a in m_[b]] for b in ref.BRANCHES},
                     "exp_avg_sq": {b: [a.copy() for a in v_[b]] for b in ref.BRANCHES}}
            packed = before if variant == "f" else after
            learner["epochs"][-1].append(len(steps))
            steps.append(dict(learner=0, index=index, mb=g, old_logits=old, t=t, before=before, after=after, grads=grads,
                              export={b: mlp_pack_ref.pack(*packed["params"][b]) for b in ref.BRANCHES}, logits=logits, value=value, stats=h["stats"],
                              grad_logits=gl, grad_value=gv))
            tot, seen, prev_x = tot + h["stats"] * n, seen + n, x
        per_epoch.append((tot / seen, seen))
    names = ref.ppo_loss_kl_ref.STATS if kl else ref.ppo_loss_ref.STATS
    as_out = lambda s: {k: float(s[names.index(k)]) for k in names if k != "loss"}
    out = {"first": as_out(per_epoch[0][0]), "last": as_out(per_epoch[-1][0]), "transitions": int(sel.size)}
    if kl:
        out["mean_action_kl"] = float(sum(s[6] * n for s, n in per_epoch) / sum(n for _, n in per_epoch))
        out["kl_coeff"] = ref.kl_rule(0.2, 0.01, out["mean_action_kl"])
    learner["out"] = out
    return dict(hyper=hp, precision="fp32", buffer=buf, learners={0: learner}, steps=steps, untouched=[("records", buf["records"], buf["records"].copy())])


@functools.lru_cache(maxsize=None)
def _failures(variant, kl=False):
    quiet = lambda line: None
    if variant == "e":
        first = _simulate(None, kl=True)["steps"][0]["after"]["params"]["policy"]   # the net after the first step has re-packed it
        x_all = ref.gather_expected(_buffer()[0], np.arange(T * B))["observations"]
        return ref.check_run(_simulate(None, kl=True, behaviour=_forward32(first, x_all)[0]), log=quiet)
    return ref.check_run(_simulate(variant, kl=kl), log=quiet)


@pytest.mark.parametrize("kl", [False, True], ids=["plain", "kl"])
def test_the_checker_accepts_a_correct_float32_update_that_is_not_its_yardstick(kl, capsys):
    ratios = {}
    run = _simulate(None, kl=kl)
    assert len(run["steps"]) == EPOCHS * 4 and run["steps"][3]["index"].size % 64 != 0
    assert ref.check_run(run, ratios=ratios) == []
    text = capsys.readouterr().out
    assert text.count("PPO_STEP_RATIO") > 100 and "PPO_STEP_MAX adam p" in text   # every ratio is printed
    assert {"logits", "grad", "adam p", "adam exp_avg", "adam exp_avg_sq", "epoch_stats"} <= set(ratios) and all(r <= ref.MARGIN for r in ratios.values())
    assert not np.array_equal(run["steps"][0]["logits"].astype(np.float64), ref.torch_step(run["steps"][0]["before"]["params"], run["steps"][0]["mb"], run["hyper"],
                                                                                             run["steps"][0]["old_logits"])["logits"])


def _kinds(failures):
    return {f[0] for f in failures}


def test_rejects_a_step_number_stuck_at_one():
    f = _failures("a")
    assert f and _kinds(f) == {"adam"}
    assert any("policy w2 p" in d for _, _, d in f) and any("value w2 p" in d for _, _, d in f)


def test_rejects_the_value_branchs_w2_gradient_stepped_into_the_policy_branch():
    f = _failures("b")
    assert f and _kinds(f) == {"adam"} and all(d.startswith("policy w2 ") for _, _, d in f)
    assert {d.split(":")[0] for _, _, d in f} == {"policy w2 p", "policy w2 exp_avg", "policy w2 exp_avg_sq"}


def test_rejects_a_short_minibatch_scaled_by_the_buffers_row_count():
    f = _failures("c")
    kinds = _kinds(f)
    assert "grad" in kinds and kinds == {"grad_logits", "grad_value", "grad"}          # the gradient checks, and nothing else: Adam is fed the native gradient
    short = [w for k, w, _ in f if k == "grad"]
    assert short and all("rows)" in w and "%d rows)" % MINIBATCH not in w for w in short)  # only the short steps
    assert {d.split(":")[0] for k, _, d in f if k == "grad"} == {"%s %s" % (b, k) for b in ref.BRANCHES for k in ref.PARAMS}


def test_rejects_a_backward_on_the_previous_minibatchs_x():
    f = _failures("d")
    assert f and _kinds(f) == {"grad"} and {d.split(":")[0] for _, _, d in f} == {"policy w1", "value w1"}


def test_rejects_old_logits_taken_after_the_first_step():
    f = _failures("e")
    assert f and _kinds(f) == {"behaviour"}
    assert _failures(None, kl=True) == []


def test_rejects_fragments_one_step_old():
    f = _failures("f")
    assert f and _kinds(f) == {"export"} and len(f) == 2 * EPOCHS * 4
