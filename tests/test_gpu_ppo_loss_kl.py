"""The KL penalty of the PPO loss head on the GPU, layer by layer: ``skyjo_vec_ppo_loss_kl`` against the float64 restatement of
tests/ppo_loss_kl_ref.py on the rows of tests/ppo_loss_kl_synth.py (within the recorded float32 deviation; exact zeros, counts and
guard tails; at ``kl_coeff`` 0 the bits of ``skyjo_vec_ppo_loss``), ``skyjo_vec_rollout_gather_logits`` against ``torch.index_select``,
``rollout.behaviour_logits`` against the net's own forward and the rollout's ``logp``, and ``examples.ppo.ppo_update(kl=...)`` end
to end on both learner paths."""
import numpy as np
import pytest

from tests import ppo_loss_kl_synth as ks
from tests import ppo_loss_synth as synth

pytestmark = pytest.mark.gpu

ROWS_PER_WORKGROUP = 128   # SK_LOSS_ROWS of csrc/skyjo_loss.h: ks.ROW_COUNTS holds it and its two neighbours
# The largest absolute deviation, per output, of the SAME expression evaluated by torch in float32 on the CPU from the float64
# restatement, over every (row count, coefficients, kl_coeff in {0, 0.2, 1}) case below (tests/ppo_loss_kl_synth.py::float32_deviation;
# measured values rounded up to two digits; tests/test_ppo_loss_kl_ref.py asserts that a fresh measurement does not exceed them).  The
# kernel is allowed 4 times these, the margin and the reason of tests/test_gpu_ppo_loss.py: room for another, equally valid float32
# operation order and for device exp / log within a couple of ulp.  The gradients carry the factor 1 / m: both their plain bound and
# the bound on m * gradient hold.  (loss and action_kl are larger than the six of the head without the penalty: a row whose old
# distribution sits on an action the new one has all but dropped has a divergence above 100, and float32 keeps 7 digits of it.)
F32_DEVIATION = {
    "grad_logits": 1.6e-07, "grad_logits_times_m": 2.2e-05, "grad_value": 1.3e-08, "grad_value_times_m": 1.3e-06,
    "loss": 2.1e-06, "policy_loss": 1.7e-07, "vf_loss": 3.6e-07, "entropy": 8.2e-08, "kl": 1.4e-07, "clip_fraction": 1.5e-08,
    "action_kl": 1.6e-06,
}
MARGIN = 4.0
SENTINEL = 0x7FC0DEAD      # a NaN with a payload: the guard tails' pattern, as float32 bits
GUARD = 64                 # elements before and after every output


def _mb(b, dev):
    import torch

    from skyjo_rl_amd.rollout import Minibatch

    t = lambda x: torch.from_numpy(x).to(dev)
    return (t(b.logits), t(b.value), t(b.old_logits),
            Minibatch(None, t(b.log_mask), t(b.actions), t(b.logp), t(b.advantages), t(b.value_targets), t(b.values), None))


@pytest.fixture(scope="module")
def cases():
    """Every row count once: the batch on the device and, per (coefficients, kl_coeff), the restatement - shared and left unchanged."""
    import torch

    dev = torch.device("cuda", 0)
    out = {}
    for m in ks.ROW_COUNTS:
        b = ks.make(m)
        out[m] = (b, _mb(b, dev), {(c, k): ks.reference(b, *c, k) for c in ks.COEFFS for k in ks.KL_COEFFS})
    return out


def _guarded(n, dtype, dev):
    """A tensor of n elements inside a larger one filled with the sentinel: (whole, view).  The view starts 16-byte aligned."""
    import torch

    whole = torch.empty((GUARD + n + GUARD,), dtype=dtype, device=dev)
    whole.view(torch.int32).fill_(SENTINEL)
    return whole, whole[GUARD:GUARD + n]


def _tails_intact(bufs):
    import torch

    for whole, view in bufs:
        w = whole.view(torch.int32).cpu().numpy()
        inner = view.numel() * view.element_size() // 4
        pad = (w.size - inner) // 2
        assert (w[:pad] == SENTINEL).all() and (w[pad + inner:] == SENTINEL).all(), "an output's guard tail was written"


def _call_guarded(logits, value, old, mb, ent_coef, vf_clip, kl_coeff):
    """The C entry on guarded outputs: stats float64 [7] and the two gradients as float32 numpy, after checking the tails."""
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev, m = logits.device, logits.shape[0]
    nbytes = int(L.skyjo_vec_ppo_loss_kl_scratch_bytes(m))
    bufs = [_guarded(m * 26, torch.float32, dev), _guarded(m, torch.float32, dev), _guarded(7, torch.float64, dev),
            _guarded(nbytes // 8, torch.float64, dev)]
    (_, gl), (_, gv), (_, st), (_, sc) = bufs
    vp = lambda t: t.data_ptr()
    rc = L.skyjo_vec_ppo_loss_kl(vp(logits), vp(mb.log_mask), vp(old), vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages),
                                 vp(mb.value_targets), vp(mb.values), m, synth.CLIP, 1.0, ent_coef, 0.0 if vf_clip is None else vf_clip, kl_coeff,
                                 vp(gl), vp(gv), vp(st), vp(sc), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.skyjo_vec_last_error()
    _tails_intact(bufs)
    assert not (gl.view(torch.int32).cpu().numpy() == SENTINEL).any(), "grad_logits has elements the kernel did not write"
    assert not (gv.view(torch.int32).cpu().numpy() == SENTINEL).any()
    return st.cpu().numpy(), gl.view(m, 26).cpu().numpy(), gv.cpu().numpy()


@pytest.mark.parametrize("kl_coeff", ks.KL_COEFFS)
@pytest.mark.parametrize("ent_coef,vf_clip", ks.COEFFS)
@pytest.mark.parametrize("m", ks.ROW_COUNTS)
def test_kernel_against_restatement(cases, m, ent_coef, vf_clip, kl_coeff):
    b, (logits, value, old, mb), wants = cases[m]
    want = wants[((ent_coef, vf_clip), kl_coeff)]
    stats, gl32, gv32 = _call_guarded(logits, value, old, mb, ent_coef, vf_clip, kl_coeff)
    dl = np.abs(gl32.astype(np.float64) - want["grad_logits"]).max()
    dv = np.abs(gv32.astype(np.float64) - want["grad_value"]).max()
    ds = np.abs(stats - want["stats"])
    print(f"m={m} ent={ent_coef} vf_clip={vf_clip} kl_coeff={kl_coeff}: grad_logits {dl:.3e} (x m {dl * m:.3e}) grad_value {dv:.3e} "
          f"(x m {dv * m:.3e}) stats", " ".join("%.3e" % x for x in ds))
    T = F32_DEVIATION
    assert dl <= MARGIN * min(T["grad_logits"], T["grad_logits_times_m"] / m)
    assert dv <= MARGIN * min(T["grad_value"], T["grad_value_times_m"] / m)
    for k, name in enumerate(ks.klref.STATS):
        assert ds[k] <= MARGIN * T[name], (name, ds[k])
    assert stats[5] * m == want["clipped_count"] and stats[5] == want["clipped_count"] / m
    masked = b.log_mask != 0
    masked[np.arange(m), b.actions] = False
    assert (gl32[masked] == 0.0).all()                                   # exactly 0.0 at every masked k != a


def test_one_legal_rows_have_no_divergence_and_no_kl_gradient(cases):
    """A minibatch of one-legal rows only, the old logits ANOTHER draw: p = po = 1, so action_kl is 0.0 and the gradient that of the
    head without the penalty, both exactly."""
    import torch

    from skyjo_rl_amd.learner import ppo_loss, ppo_loss_kl

    b, (logits, value, old, mb), _ = cases[4097]
    rows = torch.arange(0, 4097, 8, device=logits.device)                # the one-legal rows: ppo_loss_synth.KINDS[0]
    assert ((b.log_mask[::8] == 0).sum(axis=1) == 1).all() and rows.numel() == 513
    sub = type(mb)(*(None if c is None else c[rows].contiguous() for c in mb))
    lg, v = logits[rows].contiguous(), value[rows].contiguous()
    gen = torch.Generator(device=logits.device).manual_seed(5)
    other = torch.randn(lg.shape, device=lg.device, generator=gen) * 3.0
    assert not torch.equal(other, lg)
    plain = [t.clone() for t in ppo_loss(lg, v, sub, ent_coef=0.01, vf_clip=synth.VF_CLIP)]
    for kl_coeff in (0.2, 1.0):
        got = ppo_loss_kl(lg, v, sub, other, kl_coeff=kl_coeff, ent_coef=0.01, vf_clip=synth.VF_CLIP)
        assert float(got.stats[6]) == 0.0
        assert torch.equal(got.grad_logits, plain[1]) and torch.equal(got.grad_value, plain[2]) and torch.equal(got.stats[:6], plain[0])


@pytest.mark.parametrize("m", [1, 129, 4097])
def test_kl_coeff_zero_gives_the_bits_of_the_head_without_the_penalty(cases, m):
    import torch

    from skyjo_rl_amd.learner import ppo_loss, ppo_loss_kl

    _, (logits, value, old, mb), wants = cases[m]
    for ent_coef, vf_clip in ks.COEFFS:
        plain = [t.clone() for t in ppo_loss(logits, value, mb, ent_coef=ent_coef, vf_clip=vf_clip)]
        got = ppo_loss_kl(logits, value, mb, old, kl_coeff=0.0, ent_coef=ent_coef, vf_clip=vf_clip)
        assert got.stats.shape == (7,) and torch.equal(got.stats[:6], plain[0])
        assert torch.equal(got.grad_logits, plain[1]) and torch.equal(got.grad_value, plain[2])
        assert abs(float(got.stats[6]) - wants[((ent_coef, vf_clip), 0.0)]["stats"][6]) <= MARGIN * F32_DEVIATION["action_kl"]   # ... and is computed


def test_deterministic_and_out_reuse(cases):
    import torch

    from skyjo_rl_amd.learner import PPOLossBuffers, PPOLossKLBuffers, ppo_loss_kl

    _, (logits, value, old, mb), _ = cases[4097]
    _, (l2, v2, o2, mb2), _ = cases[257]
    kw = dict(kl_coeff=0.2, ent_coef=0.01, vf_clip=synth.VF_CLIP)
    first = [t.clone() for t in ppo_loss_kl(logits, value, mb, old, **kw)]
    again = ppo_loss_kl(logits, value, mb, old, **kw)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, again))
    out = PPOLossKLBuffers(4097, logits.device)
    small = [t.clone() for t in ppo_loss_kl(l2, v2, mb2, o2, **kw)]
    reused = ppo_loss_kl(l2, v2, mb2, o2, out=out, **kw)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(small, reused))
    c = ppo_loss_kl(logits, value, mb, old, out=out, **kw)
    assert c.grad_logits.data_ptr() == out.grad_logits.data_ptr() and c.stats.data_ptr() == out.stats.data_ptr() and c.stats.shape == (7,)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, c))
    d = ppo_loss_kl(logits, value.unsqueeze(1), mb, old, **kw)
    assert d.grad_value.shape == (4097, 1) and torch.equal(d.grad_value.squeeze(1), first[2]) and torch.equal(d.stats, first[0])
    with pytest.raises(ValueError):
        ppo_loss_kl(logits, value, mb, old, out=PPOLossBuffers(4097, logits.device), **kw)      # six statistics: not this head's buffers
    with pytest.raises(ValueError):
        ppo_loss_kl(logits, value, mb, old, out=PPOLossKLBuffers(4096, logits.device), **kw)


def test_non_default_stream(cases):
    import torch

    from skyjo_rl_amd.learner import ppo_loss_kl

    _, (logits, value, old, mb), _ = cases[1000]
    want = [t.clone() for t in ppo_loss_kl(logits, value, mb, old, vf_clip=synth.VF_CLIP)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.zeros((1 << 20,), device=logits.device)
        for _ in range(8):
            x = x * 1.0001 + 1.0                       # work queued on the stream ahead of the call
        moved = old + x[:1]                            # ... which the call's input depends on: a constant added to a row's old logits
        got = ppo_loss_kl(logits, value, mb, moved - x[:1], vf_clip=synth.VF_CLIP)
        same_input = torch.equal(moved - x[:1], old)
        y = x.sum()
        got2 = [t.clone() for t in ppo_loss_kl(logits, value, mb, old, vf_clip=synth.VF_CLIP)]
    s.synchronize()
    if same_input:
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got))
    assert bool(torch.isfinite(y)) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, got2))


def test_autograd_function(cases):
    import torch

    from skyjo_rl_amd.learner import PPOLossKL, ppo_loss_kl

    _, (logits, value, old, mb), _ = cases[257]
    want = [t.clone() for t in ppo_loss_kl(logits, value, mb, old, kl_coeff=0.5, ent_coef=0.01, vf_clip=synth.VF_CLIP)]
    for scale in (1.0, 0.5):
        lg, v = logits.clone().requires_grad_(), value.clone().requires_grad_()
        loss, stats = PPOLossKL.apply(lg, v, mb, old, 0.5, 0.3, 1.0, 0.01, synth.VF_CLIP)
        assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad and not stats.requires_grad
        assert torch.equal(stats, want[0]) and float(loss.detach()) == float(want[0][0].float())
        (loss * scale).backward()
        assert torch.equal(lg.grad, want[1] * scale) and torch.equal(v.grad, want[2] * scale)    # a power of two: bitwise


def test_validation_launches_nothing(cases):
    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import PPOLossKLBuffers, ppo_loss_kl

    L = _lib.load()
    _, (logits, value, old, mb), _ = cases[64]
    dev = logits.device
    out = PPOLossKLBuffers(64, dev)
    outs = (out.stats, out.grad_logits, out.grad_value)
    for t in outs:
        t.view(torch.int32).fill_(SENTINEL)
    bad = [
        (logits, value, mb, old.double()), (logits, value, mb, old.cpu()), (logits, value, mb, old.t().contiguous().t()),
        (logits, value, mb, old[:, :25]), (logits, value, mb, old[:63]), (logits, value, mb, None),
        (logits.double(), value, mb, old), (logits, value.cpu(), mb, old), (logits, value, mb._replace(values=mb.values[:10]), old),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            ppo_loss_kl(*args, out=out)
    for kl_coeff in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ppo_loss_kl(logits, value, mb, old, kl_coeff=kl_coeff, out=out)
    shifted = torch.empty((65, 26), dtype=torch.float32, device=dev)[1:]      # starts 104 bytes in: not on a 16-byte boundary
    shifted.copy_(old)
    with pytest.raises(ValueError, match="16-byte"):
        ppo_loss_kl(logits, value, mb, shifted, out=out)
    # the C entry: SKYJO_E_INVALID (-1) with a message
    vp = lambda t: t.data_ptr()
    nbytes = int(L.skyjo_vec_ppo_loss_kl_scratch_bytes(64))
    good = [vp(logits), vp(mb.log_mask), vp(old), vp(value), vp(mb.actions), vp(mb.logp), vp(mb.advantages), vp(mb.value_targets), vp(mb.values),
            64, 0.3, 1.0, 0.0, 0.0, 0.2, vp(out.grad_logits), vp(out.grad_value), vp(out.stats), vp(out.scratch), nbytes, None]
    ch = lambda k, v: good[:k] + [v] + good[k + 1:]
    cases_c = [ch(k, None) for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 17, 18)]                   # each null pointer
    cases_c += [ch(2, good[2] + 8), ch(2, good[2] + 4)]                                              # misaligned old_logits
    cases_c += [ch(14, -0.5), ch(14, float("nan")), ch(14, float("inf")), ch(14, float("-inf"))]    # kl_coeff
    cases_c += [ch(19, nbytes - 1), ch(19, 0), ch(19, int(L.skyjo_vec_ppo_loss_scratch_bytes(64)))]  # short scratch (six statistics' is short)
    cases_c += [ch(9, 0), ch(9, -5), ch(10, 0.0), ch(0, good[0] + 8), ch(15, good[15] + 8)]
    for args in cases_c:
        assert L.skyjo_vec_ppo_loss_kl(*args) == -1, args
        assert b"skyjo_vec_ppo_loss_kl" in L.skyjo_vec_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.int32) == SENTINEL).all()), "a refused call wrote an output"
    assert L.skyjo_vec_ppo_loss_kl(*good) == 0 and L.skyjo_vec_ppo_loss_kl(*ch(14, 0.0)) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- skyjo_vec_rollout_gather_logits
@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 1000])
def test_gather_logits_equals_index_select(m):
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev = torch.device("cuda", 0)
    n_rows = 300
    gen = torch.Generator(device=dev).manual_seed(300 + m)
    column = torch.randn((n_rows, 26), device=dev, generator=gen)
    store = torch.randint(0, n_rows, (max(m, 1),), device=dev, generator=gen)       # 1 000 ids over 300 rows: repeats
    index = store[:m]                                                               # (m = 0: an empty tensor has no address; store's is passed)
    if m >= 63:
        index[5], index[m - 1], index[17] = -1, n_rows, index[16]
    whole, out = _guarded(max(m, 1) * 26, torch.float32, dev)
    rc = L.skyjo_vec_rollout_gather_logits(column.data_ptr(), n_rows, store.data_ptr(), m, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.skyjo_vec_last_error()
    want = torch.zeros((m, 26), device=dev)
    ok = (index >= 0) & (index < n_rows)
    want[ok] = column.index_select(0, index[ok])
    got = out[:m * 26].view(m, 26)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    if m >= 63:
        assert not ok[5] and not ok[m - 1] and bool((got[5] == 0).all()) and bool((got[m - 1] == 0).all())
    _tails_intact([(whole, out[:m * 26])] if m else [(whole, out[:0])])
    if m == 0:
        assert bool((whole.view(torch.int32) == SENTINEL).all())           # no work


def test_gather_logits_validation_and_python_side():
    import torch

    from skyjo_rl_amd import _lib

    L = _lib.load()
    dev = torch.device("cuda", 0)
    column = torch.zeros((300, 26), device=dev)
    index = torch.arange(64, device=dev)
    out = torch.empty((64, 26), device=dev)
    out.view(torch.int32).fill_(SENTINEL)
    good = [column.data_ptr(), 300, index.data_ptr(), 64, out.data_ptr(), None]
    ch = lambda k, v: good[:k] + [v] + good[k + 1:]
    for args in (ch(0, None), ch(2, None), ch(4, None), ch(3, -1), ch(1, -1), ch(4, good[4] + 8), ch(0, good[0] + 2), ch(2, good[2] + 4)):
        assert L.skyjo_vec_rollout_gather_logits(*args) == -1, args
        assert b"skyjo_vec_rollout_gather_logits" in L.skyjo_vec_last_error()
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == SENTINEL).all()), "a refused call wrote"
    assert L.skyjo_vec_rollout_gather_logits(*good) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ---------------------------------------------------------------- rollout.behaviour_logits
def _collected(layout, arena_seats=None):
    import torch

    from skyjo_rl_amd import arena
    from skyjo_rl_amd.rollout import RolloutBuffer, collect
    from tests.test_gpu_arena import _engine, _nets

    B, N, T = 100, 3, 8                                 # a partial tile: 100 of 128 slots
    env = _engine(N, B, layout)
    env.reset()
    nets = _nets()
    buf = RolloutBuffer(env, T)
    if arena_seats is None:
        collect(env, nets["A"], nets["V"], buf, seed=3, first_ticket=0)
    else:
        arena.collect(env, [("sample", nets[s]) for s in arena_seats], [nets["V"]] * N, buf, seed=3, first_ticket=0)
    torch.cuda.synchronize()
    return env, buf, nets


def _own_logp(buf, behaviour):
    """log_softmax(behaviour + log_mask)[action] in float32 [T, B], as tests/test_gpu_policy_net.py forms it, and the valid rows."""
    import torch

    from skyjo_rl_amd.action_mask_model import FLOAT_MIN

    v = buf.views()
    lm = torch.clamp(torch.log(v.action_mask[: buf.T].to(torch.float32)), min=FLOAT_MIN)
    own = torch.log_softmax(behaviour + lm, -1).gather(2, buf.actions.long().unsqueeze(-1)).squeeze(-1)
    return own, v.done[: buf.T] == 0, v.agent[: buf.T]


@pytest.mark.parametrize("layout", ["row-major", "tile-planar-all"])
def test_behaviour_logits_are_the_nets_own_and_give_the_rollouts_logp(layout):
    import torch

    from skyjo_rl_amd.rollout import behaviour_logits, compute_targets, gather_behaviour, minibatches

    env, buf, nets = _collected(layout)
    assert buf.planar == (layout != "row-major") and getattr(buf, "behaviour", None) is None
    assert behaviour_logits(buf, nets["A"]) is buf
    assert buf.behaviour.shape == (8, 100, 26) and buf.behaviour.dtype == torch.float32
    rows = env.rows_from_planar(buf.records) if buf.planar else buf.records
    for t in range(buf.T):
        assert torch.equal(buf.behaviour[t], nets["A"](rows[t].contiguous())), t
    own, valid, _ = _own_logp(buf, buf.behaviour)
    assert int(valid.sum()) > 700
    assert float((own - buf.logp)[valid].abs().max()) < 1e-5        # the bound of tests/test_gpu_policy_net.py for the same quantity
    # refilled in place; the minibatches hand out its rows beside the Minibatch
    where = buf.behaviour.data_ptr()
    first = buf.behaviour.clone()
    buf.behaviour.zero_()
    behaviour_logits(buf, nets["A"])
    assert buf.behaviour.data_ptr() == where and torch.equal(buf.behaviour, first)
    compute_targets(buf)
    gen = torch.Generator(device="cuda").manual_seed(1)
    seen = 0
    for mb, old in minibatches(buf, 256, generator=gen, behaviour=True):
        assert old.shape == (mb.actions.numel(), 26) and old.data_ptr() % 16 == 0
        lp = torch.log_softmax(old + mb.log_mask, -1).gather(1, mb.actions.unsqueeze(1)).squeeze(1)
        assert float((lp - mb.logp).abs().max()) < 1e-5
        seen += mb.actions.numel()
    assert seen == int(((buf.target_flags & 1) != 0).sum()) and seen > 256
    idx = torch.tensor([0, 799, 5, 5, 800, -1], device="cuda")
    got = gather_behaviour(buf, idx)
    flat = buf.behaviour.view(-1, 26)
    assert torch.equal(got[:4], flat[idx[:4]]) and bool((got[4:] == 0).all())
    with pytest.raises(ValueError):
        behaviour_logits(buf, nets["V"])                              # a value branch: one output
    env.close()


def test_behaviour_logits_of_an_arena_buffer_are_one_seats():
    """Every seat its own policy: the column filled with seat s's net agrees with ``logp`` in the rows where seat s acted - the rows
    ``minibatches(seats=(s,))`` selects - and is that net's forward everywhere."""
    import torch

    from skyjo_rl_amd.rollout import behaviour_logits

    env, buf, nets = _collected("row-major", arena_seats=("A", "B", "A"))
    for name, seats in (("A", (0, 2)), ("B", (1,))):
        behaviour_logits(buf, nets[name])
        own, valid, agent = _own_logp(buf, buf.behaviour)
        mine = valid & torch.isin(agent, torch.tensor(seats, device=agent.device, dtype=agent.dtype))
        assert int(mine.sum()) > 100
        assert float((own - buf.logp)[mine].abs().max()) < 1e-5
        assert torch.equal(buf.behaviour[3], nets[name](buf.records[3]))
    other = valid & (agent == 0)                                      # seat 0 played A: B's logits do not give its logp
    assert float((own - buf.logp)[other].abs().max()) > 1e-3
    env.close()


# ---------------------------------------------------------------- examples.ppo.ppo_update(kl=...)
def _setup(T=64):
    import torch

    from examples.ppo import repack
    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(0)
    B, N = 256, 3
    env = SkyjoVecEnv(B, num_players=N)
    env.seed(None, 9)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = repack(model)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    return env, model, pol, val, buf


@pytest.mark.parametrize("native_nets", [False, True])
def test_ppo_update_with_kl_end_to_end(native_nets):
    import torch

    from examples.ppo import ppo_update
    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import KLCoeff, NativeAdam, ppo_loss_kl
    from skyjo_rl_amd.rollout import behaviour_logits, compute_targets, minibatches, select_rows
    from tests.test_gpu_policy_net import TOL

    env, model, pol, val, buf = _setup()
    # the first minibatch, before any step: old and new policy are the same weights - the packed net against the float32 module
    behaviour_logits(buf, pol)
    compute_targets(buf, gamma=0.99, lam=1.0)
    sel = select_rows(buf, _lib.TGT_HAS_TARGET)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mb, old = next(iter(minibatches(buf, 2048, generator=gen, normalize=(sel.mean, max(sel.std, 1e-6)), selection=sel, behaviour=True)))
    with torch.no_grad():
        res = ppo_loss_kl(model.policy(mb.observations), model.value(mb.observations), mb, old, kl_coeff=0.2)
    first_kl = float(res.stats[6])
    print("action_kl of the first minibatch:", first_kl, "kl:", float(res.stats[4]))
    assert -1e-6 <= first_kl < TOL[pol.precision]["kl"]

    opt = NativeAdam(model, pol, val, lr=3e-4) if native_nets else torch.optim.Adam(model.parameters(), lr=3e-4)
    before = [p.detach().clone() for p in model.policy.parameters()]
    coeff = KLCoeff()
    out = ppo_update(model, buf, opt, epochs=3, minibatch=2048, gae=(0.99, 1.0), native_batches=True, native_loss=True, native_nets=native_nets,
                     kl=coeff, behaviour_net=pol)
    print(out)
    keys = ("policy_loss", "vf_loss", "kl", "entropy", "clip_fraction", "action_kl")
    assert all(set(out[k]) == set(keys) for k in ("first", "last"))
    assert all(np.isfinite([out[k][j] for k in ("first", "last") for j in keys])) and np.isfinite(out["mean_action_kl"])
    assert out["first"]["action_kl"] >= -1e-6 and out["last"]["action_kl"] >= -1e-6 and out["mean_action_kl"] >= -1e-6
    assert out["transitions"] == sel.count
    assert any(float((p.detach() - q).abs().max()) > 0 for p, q in zip(model.policy.parameters(), before))
    assert out["kl_coeff"] == KLCoeff().update(out["mean_action_kl"]) == float(coeff)
    # a float stays what it is (the buffer is stale by now, and a NativeAdam has re-packed the net: only the coefficient is looked at)
    out2 = ppo_update(model, buf, opt, epochs=1, minibatch=2048, gae=(0.99, 1.0), native_batches=True, native_loss=True, native_nets=native_nets,
                      kl=0.5, behaviour_net=pol)
    assert out2["kl_coeff"] == 0.5
    pol.close(), val.close(), env.close()


def test_ppo_update_without_kl_is_the_path_it_was():
    """``kl=None`` against the all-native path written out here from the package's public pieces, on a fresh, identically seeded
    set-up: the same statistics and the same parameters (every kernel of that path promises the same bits on every call)."""
    import torch

    from examples import ppo
    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import STATS, NativeAdam, NativeBranch, PPOLossBuffers, ppo_loss
    from skyjo_rl_amd.rollout import compute_targets, minibatches, select_rows

    def written_out(model, buf, opt, epochs=2, minibatch=2048):
        compute_targets(buf, gamma=0.99, lam=1.0)
        sel = select_rows(buf, _lib.TGT_HAS_TARGET)
        norm = (sel.mean, max(sel.std, 1e-6))
        gen = torch.Generator(device=buf.actions.device).manual_seed(0)
        rows = max(min(minibatch, sel.count), 1)
        bufs = PPOLossBuffers(rows, buf.actions.device)
        policy, value = NativeBranch(model.policy, rows), NativeBranch(model.value, rows)
        stats = []
        for ep in range(epochs):
            tot = torch.zeros((6,), dtype=torch.float64, device=buf.actions.device)
            seen = 0
            for mb in minibatches(buf, minibatch, generator=gen, normalize=norm, selection=sel):
                logits = policy.forward(mb.observations)
                v = value.forward(mb.observations)
                res = ppo_loss(logits, v, mb, clip=0.3, vf_coef=1.0, ent_coef=0.0, vf_clip=None, out=bufs)
                policy.backward(res.grad_logits)
                value.backward(res.grad_value)
                opt.step()
                n = mb.actions.numel()
                tot += res.stats * n
                seen += n
            host = (tot / max(seen, 1)).tolist()
            stats.append({k: host[STATS.index(k)] for k in ("policy_loss", "vf_loss", "kl", "entropy", "clip_fraction")})
        return {"first": stats[0], "last": stats[-1], "transitions": sel.count}

    results, params = [], []
    for direct in (False, True):
        env, model, pol, val, buf = _setup(T=32)
        opt = NativeAdam(model, pol, val, lr=3e-4)
        if direct:
            out = written_out(model, buf, opt)
        else:
            out = ppo.ppo_update(model, buf, opt, epochs=2, minibatch=2048, gae=(0.99, 1.0), native_batches=True, native_loss=True,
                                 native_nets=True, kl=None)
        assert "kl_coeff" not in out and "action_kl" not in out["first"] and getattr(buf, "behaviour", None) is None
        results.append(out)
        params.append([p.detach().clone() for p in model.parameters()])
        pol.close(), val.close(), env.close()
    assert results[0] == results[1]
    assert all(torch.equal(a, b) for a, b in zip(*params))


def test_parameter_gradients_through_the_kl_head():
    """Parameter gradients through ``ppo_loss_kl`` + autograd against the float64 torch expression, within 4 x the float32 torch
    expression's own deviation from it (measured here, as tests/test_gpu_ppo_loss.py does for the head without the penalty).  The old
    logits are the behaviour column moved by N(0, 0.3): a penalty gradient that is not all but zero."""
    import copy

    import torch

    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.learner import ppo_loss_kl
    from skyjo_rl_amd.rollout import behaviour_logits, compute_targets, minibatches, select_rows

    env, model, pol, val, buf = _setup(T=32)
    behaviour_logits(buf, pol)
    compute_targets(buf, gamma=0.99, lam=1.0)
    sel = select_rows(buf, _lib.TGT_HAS_TARGET)
    gen = torch.Generator(device="cuda").manual_seed(0)
    mb, old = next(iter(minibatches(buf, 2048, generator=gen, normalize=(sel.mean, max(sel.std, 1e-6)), selection=sel, behaviour=True)))
    mb = type(mb)(*(c.clone() for c in mb))
    old = old + 0.3 * torch.randn(old.shape, device=old.device, generator=gen)
    params = list(model.parameters())

    def torch_grads(mdl, dtype):
        c = lambda x: x.to(dtype)
        loss, _ = ks.torch_head_kl(mdl.policy(c(mb.observations)), c(mb.log_mask), c(old), mdl.value(c(mb.observations)).squeeze(-1), mb.actions,
                                   c(mb.logp), c(mb.advantages), c(mb.value_targets), c(mb.values), 0.2, clip=0.3)
        return [g.double() for g in torch.autograd.grad(loss, list(mdl.parameters()))]

    g32 = torch_grads(model, torch.float32)
    g64 = torch_grads(copy.deepcopy(model).double(), torch.float64)
    logits, value = model.policy(mb.observations), model.value(mb.observations)
    res = ppo_loss_kl(logits, value, mb, old, kl_coeff=0.2, clip=0.3)
    assert float(res.stats[6]) > 1e-3
    gk = [g.double() for g in torch.autograd.grad([logits, value], params, [res.grad_logits, res.grad_value])]
    for p, a, b, k in zip(params, g32, g64, gk):
        dev32 = float((a - b).abs().max())
        got = float((k - b).abs().max())
        print(f"param {tuple(p.shape)}: torch f32 vs f64 {dev32:.3e}, kernel vs f64 {got:.3e}, scale {float(b.abs().max()):.3e}")
        assert got <= MARGIN * dev32, (tuple(p.shape), got, dev32)
    pol.close(), val.close(), env.close()
