"""``rollout.compute_targets`` (``skyjo_vec_rollout_targets``: per-seat GAE over a rollout buffer, one kernel) on real ``collect``
buffers: bit for bit the float32 recursion of tests/rollout_targets_ref.py in either record layout, within the derived bound of the
float64 textbook GAE (the derivation: tests/test_rollout_targets_ref.py), ``compute_returns``' columns where the episode is known,
the counting identity, the argument errors, and a PPO update that learns from the targets."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = [(1.0, 1.0), (0.99, 1.0), (0.99, 0.95), (0.5, 0.5), (0.0, 0.0)]


def _rollout(B, N, T, layout="row-major", seed=9, model_seed=0):
    import torch

    from skyjo_rl_amd import SkyjoVecEnv
    from skyjo_rl_amd.action_mask_model import ActionMaskModel, FusedNet
    from skyjo_rl_amd.rollout import RolloutBuffer, collect

    torch.manual_seed(model_seed)
    env = SkyjoVecEnv(B, num_players=N)
    env.set_record_layout(layout)
    env.seed(None, seed)
    env.reset()
    model = ActionMaskModel(obs_dim=env.obs_dim).cuda()
    pol, val = FusedNet(model.policy), FusedNet(model.value)
    buf = RolloutBuffer(env, T)
    collect(env, pol, val, buf, seed=1, first_ticket=0)
    return env, model, (pol, val), buf


def _close(env, nets):
    for n in nets:
        n.close()
    env.close()


def _columns(buf):
    return [buf.advantages, buf.value_targets, buf.returns, buf.target_flags]


def _assert_equals_recursion(buf, cols, gamma, lam):
    import torch

    from skyjo_rl_amd.rollout import compute_targets
    from tests import rollout_targets_ref as ref

    assert compute_targets(buf, gamma=gamma, lam=lam) is buf
    want = ref.targets_f32(gamma=gamma, lam=lam, **cols)
    for name, got, w in zip(("advantages", "value_targets", "returns", "flags"), _columns(buf), want):
        assert got.dtype == (torch.uint8 if name == "flags" else torch.float32) and tuple(got.shape) == (buf.T, buf.B)
        assert torch.equal(got.cpu(), torch.from_numpy(w)), (name, gamma, lam)


def test_handoff_shape_bitwise_rules_and_textbook():
    """B = 4096, N = 3, T = 320 (the shape of the hand-off test): all five (gamma, lambda) against the recursion, then the rules."""
    import torch

    from examples.ppo import compute_returns
    from skyjo_rl_amd.rollout import compute_targets
    from tests import rollout_targets_ref as ref

    env, _, nets, buf = _rollout(4096, 3, 320)
    cols = ref.columns_from_buffer(buf)
    for gamma, lam in PARAMS:
        _assert_equals_recursion(buf, cols, gamma, lam)

    compute_targets(buf, gamma=0.99, lam=0.95)
    flags = buf.target_flags
    # bit 1 is compute_returns' mask everywhere, and `returns` its returns where the bit is set
    returns, mask = compute_returns(buf)
    known = (flags & 2) != 0
    assert torch.equal(known, mask) and torch.equal(buf.returns[mask], returns[mask])
    # bit 0 never exceeds buf.valid; the counting identity, its right side from the textbook's episode cut (all games)
    has = (flags & 1) != 0
    valid = buf.valid
    assert bool((has <= valid).all())
    lost = 0
    for b in range(buf.B):
        ep = ref.cut_episodes(cols["done"], cols["episode_end"], b)
        if ep and ep[-1][1] == "T":
            seats = set(int(cols["agent"][t, b]) for t in ep[-1][0])
            if cols["done"][buf.T, b] == 0:
                seats.discard(int(cols["agent"][buf.T, b]))
            lost += len(seats)
    assert int(has.sum()) == int(valid.sum()) - lost and int(has.sum()) >= int(valid.sum()) - buf.N * buf.B
    # 64 games against the float64 textbook, within 4 L 2^-24 M
    sub = {k: np.ascontiguousarray(v[:, :64]) for k, v in cols.items()}
    adv64, tgt64, has64, info = ref.targets_f64(gamma=0.99, lam=0.95, **sub)
    M = max(float(np.abs(sub["values"]).max()), float(np.abs(sub["final_rewards"]).max()))
    bound = 4 * info["longest"] * 2.0 ** -24 * M
    adv, tgt = buf.advantages[:, :64].cpu().numpy(), buf.value_targets[:, :64].cpu().numpy()
    err = max(float(np.abs(adv - adv64).max()), float(np.abs(tgt - tgt64).max()))
    print(f"textbook: L={info['longest']} M={M:.4f} bound={bound:.3e} max error={err:.3e}")
    assert np.array_equal(has[:, :64].cpu().numpy(), has64) and err <= bound
    _close(env, nets)


@pytest.mark.parametrize("N", [1, 2, 4, 5, 8, 12])
def test_player_counts_bitwise(N):
    """The register forms (2, 4) and the generic form (1, 5, 8, 12) at B = 512, T = 256."""
    from tests import rollout_targets_ref as ref

    env, _, nets, buf = _rollout(512, N, 256, seed=20 + N)
    cols = ref.columns_from_buffer(buf)
    assert cols["episode_end"].sum() > 0
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
        _assert_equals_recursion(buf, cols, gamma, lam)
    _close(env, nets)


def test_tile_planar_equals_row_major():
    """The same rollout in 'tile-planar-all' (read in place, never unpacked) gives the same four columns, bit for bit."""
    import torch

    from skyjo_rl_amd.rollout import compute_targets

    out = []
    for layout in ("row-major", "tile-planar-all"):
        env, _, nets, buf = _rollout(4096 + 40, 3, 160, layout=layout)   # (a partial last tile)
        assert buf.planar == (layout != "row-major")
        compute_targets(buf, gamma=0.99, lam=0.95)
        out.append([c.clone() for c in _columns(buf)] + [buf.episode_end.clone()])
        _close(env, nets)
    assert int(out[0][4].sum()) > 0 and int((out[0][3] & 1).sum()) > 0
    for a, b in zip(*out):
        assert torch.equal(a, b)


def test_headline_shape_bitwise():
    """Once at 65 536 x 4 (one wavefront per SIMD), T = 64."""
    from tests import rollout_targets_ref as ref

    env, _, nets, buf = _rollout(65536, 4, 64)
    _assert_equals_recursion(buf, ref.columns_from_buffer(buf), 0.99, 0.95)
    _close(env, nets)


def test_argument_errors():
    from skyjo_rl_amd import _lib
    from skyjo_rl_amd.rollout import compute_targets

    env, _, nets, buf = _rollout(256, 3, 8)
    compute_targets(buf)
    L = _lib.load()
    p = lambda t: t.data_ptr()
    good = [env._h, p(buf.records), _lib.REC_ROW_MAJOR, buf.T, p(buf.values), 1, p(buf.final_rewards), p(buf.episode_end), 0.99, 0.95,
            p(buf.advantages), p(buf.value_targets), p(buf.returns), p(buf.target_flags), env._stream()]
    assert L.skyjo_vec_rollout_targets(*good) == 0
    bad = []
    for k in (0, 1, 4, 6, 7, 10, 11, 12, 13):          # every pointer
        bad.append(good[:k] + [None] + good[k + 1:])
    bad.append(good[:3] + [0] + good[4:])                # T < 1
    for k, x in ((8, -0.01), (8, 1.5), (9, -1.0), (9, 1.0001), (8, float("nan"))):
        bad.append(good[:k] + [x] + good[k + 1:])
    bad.append(good[:2] + [7] + good[3:])                # unknown layout
    for args in bad:
        assert L.skyjo_vec_rollout_targets(*args) == -1, args   # SKYJO_E_INVALID
    with pytest.raises(_lib.SkyjoNativeError):
        compute_targets(buf, gamma=1.01)
    _close(env, nets)


def test_ppo_update_with_gae():
    """``ppo_update(..., gae=(0.99, 0.95))`` learns from the device targets: finite losses, the value loss falls over 3 epochs."""
    import torch

    from examples.ppo import ppo_update

    env, model, nets, buf = _rollout(4096, 3, 320)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4)
    out = ppo_update(model, buf, opt, epochs=3, gae=(0.99, 0.95))
    assert out["transitions"] == int((buf.target_flags & 1).sum()) > int(0.9 * buf.valid.sum())
    assert all(torch.isfinite(torch.tensor([out[k][j] for k in ("first", "last") for j in ("policy_loss", "vf_loss", "kl")])))
    assert out["last"]["vf_loss"] < out["first"]["vf_loss"]
    _close(env, nets)
