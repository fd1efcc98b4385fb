"""One minibatch step of the native PPO update (``examples/ppo.py::ppo_update(native_batches=True, native_loss=True, native_nets=True)`` with
a ``learner.NativeAdam``, its ``kl=`` form, ``ppo_update_per_seat``) in numpy float64, TEACHER-FORCED, and the comparison of a recorded
update with it.  It composes the restatements that exist and rewrites none: ``mlp_train_ref.forward_backward`` (the two branches),
``ppo_loss_ref.ppo_loss`` / ``ppo_loss_kl_ref.ppo_loss_kl`` (the head), ``mlp_pack_ref.adam_ref`` / ``pack`` (the optimizer and the
fragments), ``rollout_batches_ref.gather`` (the minibatch).  numpy and the other helpers only, nothing from the package.  Not collected.

Teacher-forced: every boundary is compared from the NATIVE values that enter it.  ``step`` takes the float32 parameters as they were
before the step and gives logits, value, the head's statistics and gradients and the twelve parameter gradients; ``adam`` takes the
parameters, the state and the float32 gradient the optimizer was handed and gives the new p, exp_avg, exp_avg_sq.  No drift accumulates
over the steps, and no tolerance has to cover Adam's sign sensitivity to a gradient that is all but zero.

The yardstick of every float comparison is torch's own float32 evaluation of the same step from the same inputs on the CPU -
``torch_step``: ``ppo_loss_synth.torch_head`` (``torch_head_kl``) through Linear-Tanh-Linear-Tanh-Linear and autograd;
``torch_adam``: ``torch.optim.Adam(foreach=False)`` on float32 copies with its ``step`` set - never the code under test.  With d the
``mlp_train_ref.normalised_deviation`` from the float64 restatement and MARGIN = 4 (the project's margin for another equally valid
float32 summation order):

    logits, value, grad_logits, grad_value     per step:           d_ours <= 4 d_torch
    the statistics                             per step, the vector as one tensor: d_ours <= 4 d_torch
    the twelve parameter gradients             per step:           d_ours <= 4 max(d_torch, mlp_train_ref.F32_DEVIATION["A"][k])
    Adam's p, exp_avg, exp_avg_sq              per learner and tensor, both the largest over the run's steps: d_ours <= 4 d_torch
    the epoch means of ``out``                 |ours - f64 mean| <= 4 x the row-weighted mean of the yardstick's |deviation| per minibatch

(The yardstick's deviation on a mean is taken as the row-weighted mean of its per-minibatch |deviations|, not as |its mean - the float64
mean|: the latter is one scalar in which errors of both signs cancel by luck - on the simulated update of tests/test_ppo_step_ref.py
torch's was 2.1e-10 on one epoch's vf_loss where every correct float32 evaluation, numpy's included, is off by some 5e-9, a ratio of
23.8 - the same reason for which Adam's one-element b3 is judged over the whole run.)

and bit for bit: the minibatch against ``gather`` of the expected row ids, ``old_logits`` against the rows of the behaviour column, both
nets' fragments against ``pack`` of the parameters read back, and everything a step must not touch.

``check_run(run)`` is that comparison: it takes what a run recorded and returns the failures, a list of ``(kind, where, detail)``.

A run is a dict:
    hyper        ``hyper(...)``
    precision    the nets' ("fp32" / "bf16")
    buffer       dict for ``gather_expected`` (records, planar, rec_bytes, D, B, T, stride, actions, logp, values, advantages, value_targets)
                 and ``behaviour`` float32 [T, B, 26] or None
    learners     {key: dict(selection int64 ascending, mean, std, seat (or None), behaviour_params (policy parameters before the first
                 step, KL form) , epochs [[step numbers]], out (ppo_update's result), kl (None, or (coeff before, target) of a KLCoeff))}
    steps        [dict(learner, index, mb {column: array}, old_logits, t, before / after {"params", "exp_avg", "exp_avg_sq"} each
                 {"policy": [6], "value": [6]}, grads {"policy": [6], "value": [6]}, export {"policy": uint8, "value": uint8}, logits, value,
                 stats, grad_logits, grad_value, bystanders_before / bystanders_after {name: array})]
    untouched    [(name, before, after)]: compared bit for bit
"""
import numpy as np

from tests import mlp_pack_ref, mlp_train_ref, ppo_loss_kl_ref, ppo_loss_kl_synth, ppo_loss_ref, ppo_loss_synth, rollout_batches_ref

MARGIN = 4.0
BRANCHES = ("policy", "value")
PARAMS = mlp_train_ref.PARAMS
COLUMNS = ("observations", "log_mask", "actions", "logp", "advantages", "value_targets", "values", "seats")
ADAM_OUTPUTS = ("p", "exp_avg", "exp_avg_sq")
BEHAVIOUR_MAX = 1e-4  # tests/test_gpu_policy_net.py: max |packed fp32 net - float32 module| of the logits
STD_FLOOR = 1e-6      # examples/ppo.py: norm = (sel.mean, max(sel.std, 1e-6))
deviation = mlp_train_ref.normalised_deviation
FLOAT_KINDS = frozenset(("logits", "value", "stats", "grad_logits", "grad_value", "epoch_stats", "mean_action_kl"))


def hyper(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None, kl_coeff=None):
    """The hyper-parameters as the float32 values the ABI takes (Python floats holding them): the restatement, like the kernels' host
    side, forms everything else - 1 - beta, the bias corrections - from these."""
    f = lambda x: float(np.float32(x))
    return dict(lr=f(lr), betas=(f(betas[0]), f(betas[1])), eps=f(eps), clip=f(clip), vf_coef=f(vf_coef), ent_coef=f(ent_coef),
                vf_clip=None if vf_clip is None else f(vf_clip), kl_coeff=None if kl_coeff is None else f(kl_coeff))


def head(logits, value, mb, hp, old_logits=None):
    """The loss head's restatement on a minibatch (a dict of the ``rollout.Minibatch`` columns): ``ppo_loss_ref.ppo_loss``, or with
    ``hp["kl_coeff"]`` ``ppo_loss_kl_ref.ppo_loss_kl``."""
    cols = (mb["actions"], mb["logp"], mb["advantages"], mb["value_targets"], mb["values"])
    kw = dict(clip=hp["clip"], vf_coef=hp["vf_coef"], ent_coef=hp["ent_coef"], vf_clip=hp["vf_clip"])
    if hp["kl_coeff"] is None:
        return ppo_loss_ref.ppo_loss(logits, mb["log_mask"], value, *cols, **kw)
    return ppo_loss_kl_ref.ppo_loss_kl(logits, mb["log_mask"], old_logits, value, *cols, kl_coeff=hp["kl_coeff"], **kw)


def adam(params, grads, exp_avg, exp_avg_sq, hp, t):
    """Adam on one branch: the six tensors before the step, the gradient the optimizer was handed, step number t (from 1) -> three
    lists of float64 arrays: the new p, exp_avg, exp_avg_sq."""
    out = [mlp_pack_ref.adam_ref(p, g, m, v, hp["lr"], hp["betas"], hp["eps"], t) for p, g, m, v in zip(params, grads, exp_avg, exp_avg_sq)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def step(state, mb, hp, old_logits=None):
    """One minibatch step of one branch pair in float64.  ``state``: {"params", "exp_avg", "exp_avg_sq": {"policy": [6], "value": [6]}, "t"}
    - the parameters and both Adam states before the step, ``t`` the number of this step.  Returns {"logits" [m, 26], "value" [m], "stats",
    "grad_logits", "grad_value", "action_kl" (KL form: per row), "grads": {"policy": [6], "value": [6]}, "next": the state after the step
    taken with these float64 gradients (a teacher-forced comparison does not use it)}."""
    x = mb["observations"]
    m = np.shape(x)[0]
    P, V = state["params"]["policy"], state["params"]["value"]
    logits = mlp_train_ref.forward_backward(P, x, np.zeros((m, np.shape(P[4])[0])))["out"]
    value = mlp_train_ref.forward_backward(V, x, np.zeros((m, 1)))["out"]
    h = head(logits, value, mb, hp, old_logits)
    gp = mlp_train_ref.forward_backward(P, x, h["grad_logits"])
    gv = mlp_train_ref.forward_backward(V, x, h["grad_value"].reshape(m, 1))
    grads = {"policy": [gp[k] for k in PARAMS], "value": [gv[k] for k in PARAMS]}
    nxt = {"params": {}, "exp_avg": {}, "exp_avg_sq": {}, "t": state["t"] + 1}
    for b in BRANCHES:
        nxt["params"][b], nxt["exp_avg"][b], nxt["exp_avg_sq"][b] = adam(state["params"][b], grads[b], state["exp_avg"][b], state["exp_avg_sq"][b],
                                                                         hp, state["t"])
    return {"logits": logits, "value": value.reshape(m), "stats": h["stats"], "grad_logits": h["grad_logits"], "grad_value": h["grad_value"],
            "action_kl": h.get("akl"), "grads": grads, "next": nxt}


def torch_step(params, mb, hp, old_logits=None, dtype=None):
    """The yardstick: the same step's forward, head and autograd in torch on the CPU in ``dtype`` (float32) - Linear-Tanh-Linear-Tanh-
    Linear as ``ActionMaskModel``'s branches are, ``ppo_loss_synth.torch_head`` (``ppo_loss_kl_synth.torch_head_kl``).  ``params``:
    {"policy": [6], "value": [6]}.  Returns ``step``'s dict (float64 numpy) without "next" and "action_kl"."""
    import torch

    dtype = dtype or torch.float32
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    leaves = {b: [t(p).requires_grad_() for p in params[b]] for b in BRANCHES}
    x = t(mb["observations"])

    def branch(p):
        h1 = torch.tanh(torch.nn.functional.linear(x, p[0], p[1]))
        return torch.nn.functional.linear(torch.tanh(torch.nn.functional.linear(h1, p[2], p[3])), p[4], p[5])

    logits, value = branch(leaves["policy"]), branch(leaves["value"])
    logits.retain_grad(), value.retain_grad()
    cols = (torch.from_numpy(np.array(mb["actions"])), t(mb["logp"]), t(mb["advantages"]), t(mb["value_targets"]), t(mb["values"]))
    kw = dict(clip=hp["clip"], vf_coef=hp["vf_coef"], ent_coef=hp["ent_coef"], vf_clip=hp["vf_clip"])
    if hp["kl_coeff"] is None:
        loss, stats = ppo_loss_synth.torch_head(logits, t(mb["log_mask"]), value.squeeze(-1), *cols, **kw)
    else:
        loss, stats = ppo_loss_kl_synth.torch_head_kl(logits, t(mb["log_mask"]), t(old_logits), value.squeeze(-1), *cols, hp["kl_coeff"], **kw)
    loss.backward()
    n = lambda a: a.detach().double().numpy()
    return {"logits": n(logits), "value": n(value).reshape(-1), "stats": np.array([float(s) for s in stats]), "grad_logits": n(logits.grad),
            "grad_value": n(value.grad).reshape(-1), "grads": {b: [n(p.grad) for p in leaves[b]] for b in BRANCHES}}


def torch_adam(params, grads, exp_avg, exp_avg_sq, hp, t, dtype=None):
    """The yardstick of ``adam``: ``torch.optim.Adam(foreach=False)`` on ``dtype`` (float32) copies, its state set to exp_avg /
    exp_avg_sq and its ``step`` to t - 1, one ``step()``.  Three lists of float64 arrays."""
    import torch

    dtype = dtype or torch.float32
    c = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    ps = [c(p).requires_grad_() for p in params]
    opt = torch.optim.Adam(ps, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], foreach=False)
    for p, g, m, v in zip(ps, grads, exp_avg, exp_avg_sq):
        p.grad = c(g)
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": c(m), "exp_avg_sq": c(v)}
    opt.step()
    n = lambda a: a.detach().double().numpy()
    return [n(p) for p in ps], [n(opt.state[p]["exp_avg"]) for p in ps], [n(opt.state[p]["exp_avg_sq"]) for p in ps]


ADAM_FAR_STEPS = (1, 7, 1000, 10 ** 6, 2 ** 31 + 5)  # the bias corrections at work, almost 1, and 1 - a step number beyond int32
ADAM_FAR_HYPER = hyper(**mlp_pack_ref.ADAM_HYPER)


def adam_inputs(shape=mlp_pack_ref.SHAPES[0]):
    """The synthetic Adam case: (p, g, exp_avg, exp_avg_sq) of one branch of ``shape``, float32 lists - default-initialised parameters,
    ``mlp_pack_ref.adam_grads`` as the gradient, and a hand-made NON-ZERO state from two more draws of it (exp_avg a tenth of one,
    exp_avg_sq the square of the other); tensor ``ADAM_ZERO_TENSOR`` is zero in all three."""
    p = [np.array(w) for w in mlp_train_ref.weights(shape, "A")]
    shapes = [w.shape for w in p]
    g = mlp_pack_ref.adam_grads(shapes, 1, seed=77)
    m = [(np.float32(0.1) * a).astype(np.float32) for a in mlp_pack_ref.adam_grads(shapes, 2, seed=78)]
    v = [(a * a).astype(np.float32) for a in mlp_pack_ref.adam_grads(shapes, 3, seed=79)]
    return p, g, m, v


def kl_rule(coeff, target, mean_action_kl):
    """``learner.KLCoeff.update`` as its docstring states it: times 1.5 above 2 target, times 0.5 below 0.5 target, both strict."""
    return coeff * 1.5 if mean_action_kl > 2.0 * target else coeff * 0.5 if mean_action_kl < 0.5 * target else coeff


def select(flags, require, agent=None, seats=None):
    """Ascending ids of the rows with every bit of ``require`` (in which one of ``seats`` acted: ``arena_collect_ref.select_by_seat``)."""
    if seats is None:
        return rollout_batches_ref.select(flags, require)
    from tests import arena_collect_ref

    return arena_collect_ref.select_by_seat(flags, require, agent, seats)[0]


def selection_moments(advantages, index):
    """(mean, std) of the selected rows' advantages as ``examples/ppo.py`` normalises with them: ``rollout.select_rows``' moments, the
    standard deviation at least 1e-6."""
    s, q = rollout_batches_ref.moments(advantages, index)
    mean, std = rollout_batches_ref.mean_std(s, q, int(np.size(index)))
    return mean, max(std, STD_FLOOR)


def gather_expected(buffer, index, mean=0.0, std=1.0):
    """``rollout_batches_ref.gather`` of the rows ``index`` of a recorded buffer, plus "old_logits": the same rows of its behaviour
    column where it has one."""
    b = buffer
    out = rollout_batches_ref.gather(b["records"], b["planar"], b["rec_bytes"], b["D"], b["B"], b["T"], b["stride"], index, b["actions"], b["logp"],
                                     b["values"], b["advantages"], b["value_targets"], mean, std)
    if b.get("behaviour") is not None:
        out["old_logits"] = np.asarray(b["behaviour"], dtype=np.float32).reshape(-1, 26)[np.asarray(index, dtype=np.int64)]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def weighted_means(stats, rows):
    """The row-weighted mean of per-minibatch statistics [k, s] with ``rows`` [k]: what ``ppo_update`` reports per epoch."""
    stats, rows = np.asarray(stats, dtype=np.float64), np.asarray(rows, dtype=np.float64)
    return (stats * rows[:, None]).sum(axis=0) / rows.sum()


def yardstick_mean_deviation(torch_stats, ref_stats, rows):
    """The yardstick's deviation on a row-weighted mean: the row-weighted mean of its per-minibatch |deviations| - what its error on the
    mean can be, without the credit of errors of both signs cancelling in one particular sum (see the module docstring)."""
    return weighted_means(np.abs(np.asarray(torch_stats, dtype=np.float64) - np.asarray(ref_stats, dtype=np.float64)), rows)


def _ratio(d_ours, d_torch):
    return "%.3f" % (d_ours / d_torch) if d_torch > 0.0 else ("0" if d_ours == 0.0 else "inf")


class _Ledger:
    """Collects the failures, prints every comparison and keeps the largest d_ours / bound-deviation ratio per quantity."""

    def __init__(self, log, ratios):
        self.failures, self.log, self.ratios = [], log, {} if ratios is None else ratios

    def fail(self, kind, where, detail):
        self.failures.append((kind, where, detail))

    def compare(self, kind, where, name, d_ours, d_ref, quantity=None):
        """d_ours <= MARGIN d_ref, printed and recorded."""
        self.log("PPO_STEP_RATIO %s %s %s: d_ours %.3e d_torch %.3e ratio %s" % (where, kind, name, d_ours, d_ref, _ratio(d_ours, d_ref)))
        q = quantity or kind
        r = d_ours / d_ref if d_ref > 0.0 else (0.0 if d_ours == 0.0 else float("inf"))
        self.ratios[q] = max(self.ratios.get(q, 0.0), r)
        if not d_ours <= MARGIN * d_ref:
            self.fail(kind, where, "%s: d_ours %.3e > %g x %.3e" % (name, d_ours, MARGIN, d_ref))


def check_run(run, log=print, ratios=None):
    """Compare a recorded update with the restatement (module docstring).  Returns the list of failures ``(kind, where, detail)``; kinds:
    "minibatch", "old_logits", "seats", "epoch", "logits", "value", "stats", "grad_logits", "grad_value", "grad", "adam", "export", "bystander",
    "untouched", "behaviour", "epoch_stats", "transitions", "mean_action_kl", "kl_coeff" - ``FLOAT_KINDS`` are the comparisons of a float output with
    the yardstick, the others are exact or carry the parameter gradients' floor.  ``ratios``: a dict that receives the largest ratio per quantity."""
    led = _Ledger(log, ratios)
    hp, buffer = run["hyper"], run["buffer"]
    kl_form = hp["kl_coeff"] is not None
    stat_names = ppo_loss_kl_ref.STATS if kl_form else ppo_loss_ref.STATS
    adam_max = {}   # (learner, branch, tensor, output) -> [d_ours, d_torch], the largest over the run
    per_step = []   # (rows, restated statistics, yardstick statistics) of every step
    for i, s in enumerate(run["steps"]):
        L = run["learners"][s["learner"]]
        where = "learner %s step %d (t = %d, %d rows)" % (s["learner"], i, s["t"], np.size(s["index"]))
        # ---- the minibatch, bit for bit
        want = gather_expected(buffer, s["index"], L["mean"], L["std"])
        for name in COLUMNS:
            if not same_bits(s["mb"][name], want[name]):
                led.fail("minibatch", where, name + " is not the gather of the expected rows")
        if kl_form and not same_bits(s["old_logits"], want["old_logits"]):
            led.fail("old_logits", where, "old_logits is not the expected rows of the behaviour column")
        if L.get("seat") is not None and not bool((np.asarray(s["mb"]["seats"]) == L["seat"]).all()):
            led.fail("seats", where, "a row of another seat")
        # ---- forward, head, backward: from the native parameters and the minibatch as it was yielded
        state = {"params": s["before"]["params"], "exp_avg": s["before"]["exp_avg"], "exp_avg_sq": s["before"]["exp_avg_sq"], "t": s["t"]}
        old = s["old_logits"] if kl_form else None
        ref = step(state, s["mb"], hp, old)
        tor = torch_step(s["before"]["params"], s["mb"], hp, old)
        per_step.append((int(np.size(s["index"])), ref["stats"], tor["stats"]))
        for name in ("logits", "value", "grad_logits", "grad_value"):
            got = np.asarray(s[name], dtype=np.float64).reshape(ref[name].shape)
            led.compare(name, where, name, deviation(got, ref[name]), deviation(tor[name], ref[name]))
        got_stats = np.asarray(s["stats"], dtype=np.float64)
        led.compare("stats", where, "all", deviation(got_stats, ref["stats"]), deviation(tor["stats"], ref["stats"]))
        for b in BRANCHES:
            for k, g, w, y in zip(PARAMS, s["grads"][b], ref["grads"][b], tor["grads"][b]):
                floor = max(deviation(y, w), mlp_train_ref.F32_DEVIATION["A"][k])
                led.compare("grad", where, "%s %s" % (b, k), deviation(np.asarray(g, dtype=np.float64).reshape(w.shape), w), floor)
        # ---- Adam: from the native parameters, state and gradient; the fragments: pack() of the parameters as read back
        for b in BRANCHES:
            args = (s["before"]["params"][b], s["grads"][b], s["before"]["exp_avg"][b], s["before"]["exp_avg_sq"][b], hp, s["t"])
            w3, y3 = adam(*args), torch_adam(*args)
            for what, key, w, y in zip(ADAM_OUTPUTS, ("params", "exp_avg", "exp_avg_sq"), w3, y3):
                for k, got, wk, yk in zip(PARAMS, s["after"][key][b], w, y):
                    mx = adam_max.setdefault((s["learner"], b, k, what), [0.0, 0.0])
                    mx[0] = max(mx[0], deviation(np.asarray(got, dtype=np.float64).reshape(wk.shape), wk))
                    mx[1] = max(mx[1], deviation(yk, wk))
            blob = mlp_pack_ref.pack(*[np.asarray(p, dtype=np.float32) for p in s["after"]["params"][b]], precision=run["precision"])
            if not same_bits(np.asarray(s["export"][b], dtype=np.uint8).reshape(-1), blob):
                led.fail("export", where, "the %s net's fragments are not pack() of the parameters read back" % b)
        # ---- what the step must not touch
        for name, a in s.get("bystanders_before", {}).items():
            if not same_bits(a, s["bystanders_after"][name]):
                led.fail("bystander", where, name + " changed")
    for (learner, b, k, what), (d_ours, d_torch) in adam_max.items():
        led.compare("adam", "learner %s, largest over the run" % (learner,), "%s %s %s" % (b, k, what), d_ours, d_torch, quantity="adam " + what)
    for name, a, b in run.get("untouched", ()):
        if not same_bits(a, b):
            led.fail("untouched", "run", name + " changed")
    # ---- per learner: the epochs, the behaviour column, the reported means
    for key, L in run["learners"].items():
        where = "learner %s" % (key,)
        mine = [i for i, s in enumerate(run["steps"]) if s["learner"] == key]
        if sorted(i for ep in L["epochs"] for i in ep) != mine:
            led.fail("epoch", where, "the epochs do not partition the learner's steps")
        for e, ep in enumerate(L["epochs"]):
            rows = np.concatenate([np.asarray(run["steps"][i]["index"], dtype=np.int64) for i in ep]) if ep else np.zeros(0, dtype=np.int64)
            if not np.array_equal(np.sort(rows), np.asarray(L["selection"], dtype=np.int64)):
                led.fail("epoch", where, "epoch %d does not visit every selected row exactly once" % e)
        if kl_form:
            x = gather_expected(buffer, np.arange(buffer["T"] * buffer["B"]))["observations"]
            P = L["behaviour_params"]
            want = mlp_train_ref.forward_backward(P, x, np.zeros((x.shape[0], 26)))["out"]
            rows = np.asarray(L["selection"], dtype=np.int64)  # (an arena buffer: the other seats' rows are another net's to explain)
            d = float(np.abs(np.asarray(buffer["behaviour"], dtype=np.float64).reshape(-1, 26)[rows] - want[rows]).max())
            log("PPO_STEP_BEHAVIOUR %s: max |behaviour - float64 forward of the parameters before the first step| %.3e (bound %.0e)" % (where, d, BEHAVIOUR_MAX))
            if not d <= BEHAVIOUR_MAX:
                led.fail("behaviour", where, "max |behaviour - float64 forward before the first step| = %.3e > %.0e" % (d, BEHAVIOUR_MAX))
        out = L.get("out")
        if out is None:
            continue
        if out["transitions"] != np.size(L["selection"]):
            led.fail("transitions", where, "%r rows reported, %d selected" % (out["transitions"], np.size(L["selection"])))
        report = [n for n in stat_names if n != "loss"]
        for name, ep in (("first", L["epochs"][0]), ("last", L["epochs"][-1])):
            n = [per_step[i][0] for i in ep]
            w, y = weighted_means([per_step[i][1] for i in ep], n), yardstick_mean_deviation([per_step[i][2] for i in ep], [per_step[i][1] for i in ep], n)
            if set(out[name]) != set(report):
                led.fail("epoch_stats", where, "out[%r] has the keys %s" % (name, sorted(out[name])))
                continue
            for stat in report:
                k = stat_names.index(stat)
                led.compare("epoch_stats", where, "%s %s" % (name, stat), abs(float(out[name][stat]) - w[k]), y[k])
        if kl_form:
            n = [per_step[i][0] for i in mine]
            w = weighted_means([per_step[i][1] for i in mine], n)[6]
            y = yardstick_mean_deviation([per_step[i][2] for i in mine], [per_step[i][1] for i in mine], n)[6]
            led.compare("mean_action_kl", where, "mean_action_kl", abs(float(out["mean_action_kl"]) - w), y)
            if L.get("kl") is not None:
                want = kl_rule(L["kl"][0], L["kl"][1], float(out["mean_action_kl"]))
                if out["kl_coeff"] != want:
                    led.fail("kl_coeff", where, "kl_coeff %r is not the rule applied once (%r)" % (out["kl_coeff"], want))
    for q in sorted(led.ratios):
        log("PPO_STEP_MAX %s: largest ratio %.3f" % (q, led.ratios[q]))
    return led.failures
