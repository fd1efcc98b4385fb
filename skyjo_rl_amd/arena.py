"""Arena rollouts: every SEAT plays a policy of its own, and the episodes that end become per-seat results.

The training rollout (``rollout.collect``) drives all seats with one net, sampled.  That cannot say whether training helped: a seat's
final reward is relative to the table's mean (skyjo_env.py:293-312), so with one shared policy the seats' rewards average to
``mean_reward`` whatever the policy has learned.  The reference's own script trains one policy per seat
(``rlskyjo/models/train_model_simple_rllib.py:43-49``) and afterwards plays the trained policies with ``logits.argmax()``
(``:123-130``).  This module is that evaluation path, beside the training rollout and not inside it: per lockstep iteration ONE
full-batch launch of the net kernel per DISTINCT net, one small kernel that gives every game the action of the seat whose turn it is,
and the engine's ``skyjo_vec_step_collect`` - ``skyjo_vec_arena_rollout`` runs T such iterations in one native call.

A seat is ``("sample", net)`` - the masked categorical draw of the training rollout -, ``("greedy", net)`` - the argmax of the masked
logits, the smallest index on a tie - or ``"random"`` - ``policy_ra``, uniform over the legal actions.  ``net`` is a ``FusedNet`` of a
model's policy branch; seats that hold the same ``FusedNet`` share its forward.  ``episode_stats`` turns the ``final_rewards`` /
``episode_end`` columns of a played buffer into episodes, mean and standard deviation of the final reward and win rate per seat
(``skyjo_vec_episode_stats``).

``collect`` (``act`` for one iteration) is the arena rollout a learner can train on - the reference's own set-up, one PPO policy per
seat: it also records ``logp`` and the ACTING seat's own value estimate (``skyjo_vec_arena_collect``: per iteration one launch per
distinct policy net, one per distinct value net, one kernel, the step), so that ``rollout.compute_targets`` and the per-seat
``rollout.select_rows(buf, seats=...)`` / ``minibatches(..., seats=...)`` apply to the buffer.
"""
import ctypes as C
import math
from collections import namedtuple

from . import _lib

KINDS = {"sample": _lib.SEAT_SAMPLE, "greedy": _lib.SEAT_GREEDY, "random": _lib.SEAT_RANDOM}

EpisodeStats = namedtuple("EpisodeStats", ["episodes", "mean_reward", "std_reward", "win_rate"])


def seat_policies(env, seats):
    """The ctypes array ``skyjo_vec_seat_policy[num_players]`` for ``seats``: a list of ``env.num_players`` entries, each
    ``("sample", FusedNet)``, ``("greedy", FusedNet)`` or ``"random"``.  The array keeps its nets alive (``.nets``: the distinct ones,
    in the order of their first seat).  ``ValueError`` for a wrong length, an unknown kind, a closed net, a missing net or a net
    combined with ``"random"``."""
    seats = list(seats)
    if len(seats) != env.num_players:
        raise ValueError(f"seats has {len(seats)} entries, the engine has {env.num_players} players")
    arr = (_lib.SeatPolicy * len(seats))()
    nets = []
    for s, entry in enumerate(seats):
        kind, net = None, None
        if isinstance(entry, str):
            kind = entry
        elif isinstance(entry, (tuple, list)) and len(entry) in (1, 2) and isinstance(entry[0], str):
            kind, net = entry[0], entry[1] if len(entry) == 2 else None
        if kind not in KINDS:
            raise ValueError(f"seat {s}: {entry!r} is not ('sample', net), ('greedy', net) or 'random'")
        if kind == "random":
            if net is not None:
                raise ValueError(f"seat {s}: 'random' takes no net")
        else:
            handle = getattr(net, "_h", None)
            if net is None or not hasattr(net, "_h"):
                raise ValueError(f"seat {s}: '{kind}' needs a FusedNet")
            if not handle:
                raise ValueError(f"seat {s}: this FusedNet is closed")
            if not any(n is net for n in nets):
                nets.append(net)
            arr[s].net = handle.value if isinstance(handle, C.c_void_p) else handle
        arr[s].kind = KINDS[kind]
    arr.nets = nets
    return arr


def _seats(env, seats):
    return seats if isinstance(seats, C.Array) and getattr(seats, "_type_", None) is _lib.SeatPolicy else seat_policies(env, seats)


def _workspace(env, holder, sp, vn=()):
    """(pointer, bytes) of a workspace for the distinct policy nets of ``sp`` and the distinct value nets of ``vn``, cached on ``holder``
    (one attribute for ``play`` and ``collect``: the larger of the two serves both); (None, 0) when no seat has a net of either kind."""
    need = int(_lib.load().skyjo_vec_arena_act_workspace_bytes(env._h, len({s.net for s in sp if s.net}), len({v for v in vn if v})))
    if need == 0:
        return None, 0
    ws = getattr(holder, "_arena_workspace", None)
    if ws is None or ws.numel() < need:
        torch = env._torch()
        ws = torch.empty((need,), dtype=torch.uint8, device=env._dev())
        holder._arena_workspace = ws
    return C.c_void_p(ws.data_ptr()), ws.numel()


def _check_iteration(env, records, planar):
    """``records`` is one iteration's records of ``env`` in the layout ``planar`` names, or ``ValueError``."""
    want = (env.tiles * 64 if planar else env.num_envs) * env.record_bytes
    if not records.is_contiguous() or records.numel() != want or records.dtype != env._torch().uint8:
        raise ValueError(f"records must be one iteration's contiguous uint8 records ({want} bytes with planar={planar})")


def _check_buffer(env, buf):
    """``buf`` is a ``rollout.RolloutBuffer`` of ``env``'s shape in the layout the engine writes, or ``ValueError``."""
    from . import rollout

    rollout._check_records(buf)
    rollout._check_layout(env, buf)
    if buf.B != env.num_envs or buf.N != env.num_players:
        raise ValueError("buf was made for another engine shape")


def select(env, seats, records, seed=0, ticket=0, actions=None, planar=False, workspace=None):
    """One lockstep iteration's actions (``skyjo_vec_arena_select``): int32 [num_envs] for ``env.step``, the action of the seat each
    game's record expects.  ``records``: one iteration's records of ``env`` - [num_envs, record_bytes], or with ``planar`` one
    tile-planar block [tiles, P, 64, 16], read in place.  ``seats``: as for ``seat_policies`` (or its result).  ``workspace``: an
    object to cache the logits' workspace on (default: the seat array)."""
    from .rollout import _layout

    torch = env._torch()
    sp = _seats(env, seats)
    _check_iteration(env, records, planar)
    if actions is None:
        actions = torch.empty((env.num_envs,), dtype=torch.int32, device=env._dev())
    elif actions.dtype != torch.int32 or actions.numel() != env.num_envs or not actions.is_contiguous():
        raise ValueError("actions must be a contiguous int32 tensor of num_envs elements")
    ws, nbytes = _workspace(env, sp if workspace is None else workspace, sp)
    _lib.check(_lib.load().skyjo_vec_arena_select(env._h, sp, C.c_void_p(records.data_ptr()), _layout(planar),
                                                  int(seed), int(ticket), C.c_void_p(actions.data_ptr()), ws, nbytes, env._stream()))
    return actions


def play(env, seats, buf, seed=0, first_ticket=0, first_records=None):
    """Fill ``buf`` (a ``rollout.RolloutBuffer`` of ``env``) with T lockstep iterations of the seats' policies in one native call
    (``skyjo_vec_arena_rollout``): ``records``, ``actions``, ``final_rewards`` and ``episode_end`` as ``rollout.collect`` lays them
    out; ``buf.logp`` and ``buf.values`` are left as they are.  Either record layout: ``buf.planar`` must be what the engine writes.
    Iteration t draws with ticket ``first_ticket + t``; ``first_records``: the records to start from (default: ``env.observe()``).
    The logits' workspace is cached on the buffer."""
    from . import rollout

    _check_buffer(env, buf)
    sp = _seats(env, seats)
    ws, nbytes = _workspace(env, buf, sp)
    rollout._first(env, buf, first_records)
    vp = lambda t: t.data_ptr()
    b = _lib.RolloutBuffers(vp(buf.records), vp(buf.actions), None, None, vp(buf.final_rewards), vp(buf.episode_end))
    _lib.check(_lib.load().skyjo_vec_arena_rollout(env._h, sp, buf.T, int(seed), int(first_ticket), C.byref(b), ws, nbytes, env._stream()))
    return buf


def value_nets(env, values):
    """The ctypes array ``const skyjo_vec_mlp *[num_players]`` for ``values``: a list of ``env.num_players`` entries, each the
    ``FusedNet`` of a model's value branch or None.  The array keeps its nets alive (``.nets``).  ``ValueError`` for a wrong length, an
    entry that is neither, or a closed net."""
    values = list(values)
    if len(values) != env.num_players:
        raise ValueError(f"values has {len(values)} entries, the engine has {env.num_players} players")
    arr = (C.c_void_p * len(values))()
    nets = []
    for s, net in enumerate(values):
        if net is None:
            continue
        if not hasattr(net, "_h"):
            raise ValueError(f"seat {s}: a value net is a FusedNet or None, not {net!r}")
        handle = net._h
        if not handle:
            raise ValueError(f"seat {s}: this FusedNet is closed")
        if not any(n is net for n in nets):
            nets.append(net)
        arr[s] = handle.value if isinstance(handle, C.c_void_p) else handle
    arr.nets = nets
    return arr


def _values(env, values):
    return values if isinstance(values, C.Array) and getattr(values, "_type_", None) is C.c_void_p else value_nets(env, values)


def act(env, seats, values, records, seed=0, ticket=0, actions=None, logp=None, values_out=None, planar=False, workspace=None,
        values_only=False):
    """One lockstep iteration with the learner's columns (``skyjo_vec_arena_act``): ``(actions, logp, values_out)`` - ``select``'s
    actions (the same bits), float32 [num_envs] the log-probability of each under the acting seat's masked distribution, and float32
    [num_envs] the acting seat's own value estimate (0.0 for a seat without a value net).  ``seats`` / ``records`` / ``planar`` /
    ``workspace``: as for ``select``; ``values``: ``num_players`` entries, each a ``FusedNet`` of a value branch or None (or the
    result of ``value_nets``).  ``values_only``: no action is chosen and no policy net runs - ``(None, None, values_out)``, the
    bootstrap values of the records a rollout ends on."""
    from .rollout import _layout

    torch = env._torch()
    sp, vn = _seats(env, seats), _values(env, values)
    _check_iteration(env, records, planar)

    def column(name, t, dtype):
        if t is None:
            return torch.empty((env.num_envs,), dtype=dtype, device=env._dev())
        if t.dtype != dtype or t.numel() != env.num_envs or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of num_envs elements")
        return t

    if values_only:
        if actions is not None or logp is not None:
            raise ValueError("values_only=True takes neither actions nor logp")
    else:
        actions, logp = column("actions", actions, torch.int32), column("logp", logp, torch.float32)
    values_out = column("values_out", values_out, torch.float32)
    ws, nbytes = _workspace(env, sp if workspace is None else workspace, sp, vn)
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(_lib.load().skyjo_vec_arena_act(env._h, sp, vn, vp(records), _layout(planar), int(seed),
                                               int(ticket), vp(actions), vp(logp), vp(values_out), ws, nbytes, env._stream()))
    return actions, logp, values_out


def collect(env, seats, values, buf, seed=0, first_ticket=0, first_records=None):
    """Fill ALL SIX columns of ``buf`` (a ``rollout.RolloutBuffer`` of ``env``) with T lockstep iterations of the seats' policies in one
    native call (``skyjo_vec_arena_collect``): what ``play`` writes, and ``logp`` - the log-probability of the chosen action under the
    acting seat's masked distribution, for a sampled, a greedy and a random seat alike - and ``values`` [T + 1, B, 1] - the value net of
    the seat that acts in the row, ``values[T]`` that of the seat ``records[T]`` expects, 0.0 for a seat without one.  The buffer then
    goes through ``rollout.compute_targets`` unchanged, and ``rollout.select_rows(buf, seats=(s,))`` / ``minibatches(..., seats=(s,))``
    give seat s its own rows: one learner per seat at one table, a seat against frozen versions of itself, a seat against ``"random"``
    seats.  ``seats``: as for ``play``; ``values``: ``num_players`` entries, each a ``FusedNet`` of a value branch or None.  With every
    seat ``("sample", P)`` and every value ``V`` these are the bits of ``rollout.collect(env, P, V, buf)``.  The workspace is cached on
    the buffer."""
    from . import rollout

    _check_buffer(env, buf)
    if tuple(buf.values.shape) != (buf.T + 1, buf.B, 1):
        raise ValueError(f"buf.values must be [T + 1, B, 1], not {tuple(buf.values.shape)}")
    sp, vn = _seats(env, seats), _values(env, values)
    ws, nbytes = _workspace(env, buf, sp, vn)
    rollout._first(env, buf, first_records)
    vp = lambda t: t.data_ptr()
    b = _lib.RolloutBuffers(vp(buf.records), vp(buf.actions), vp(buf.logp), vp(buf.values), vp(buf.final_rewards), vp(buf.episode_end))
    _lib.check(_lib.load().skyjo_vec_arena_collect(env._h, sp, vn, buf.T, int(seed), int(first_ticket), C.byref(b), ws, nbytes, env._stream()))
    return buf


def stats_from_sums(sums, num_players):
    """``EpisodeStats`` from the ``1 + 3 N`` doubles of ``skyjo_vec_episode_stats`` (the count, then per seat sum, sum of squares,
    wins), the moments taken in double: ``std`` is the unbiased estimate and 0.0 for fewer than two episodes."""
    n = int(sums[0])
    mean, std, win = [], [], []
    for s in range(num_players):
        x, q, w = (float(v) for v in sums[1 + 3 * s: 4 + 3 * s])
        mean.append(x / n if n else 0.0)
        std.append(math.sqrt(max(q - x * x / n, 0.0) / (n - 1)) if n > 1 else 0.0)
        win.append(w / n if n else 0.0)
    return EpisodeStats(n, tuple(mean), tuple(std), tuple(win))


def episode_stats(buf):
    """Per-seat results of the episodes that ended inside a filled buffer: ``EpisodeStats(episodes, mean_reward, std_reward,
    win_rate)`` - the number of rows with ``episode_end``, and per seat (tuples of ``num_players`` floats) the mean and the unbiased
    standard deviation of its final reward over them and the fraction in which it holds the table's highest reward (a tie counts for
    every tied seat).  One native call on the buffer's columns (``skyjo_vec_episode_stats``: sums in double, fixed order); the copy
    of its ``1 + 3 N`` doubles to the host is the only synchronisation."""
    import torch

    L = _lib.load()
    fr, ee = buf.final_rewards, buf.episode_end
    N = fr.shape[-1]
    rows = ee.numel()
    if fr.dtype != torch.float64 or ee.dtype != torch.uint8 or fr.numel() != rows * N or not fr.is_contiguous() or not ee.is_contiguous():
        raise ValueError("final_rewards must be contiguous float64 [..., N] and episode_end contiguous uint8 with the same leading shape")
    need = int(L.skyjo_vec_episode_stats_scratch_bytes(rows, N))
    out = getattr(buf, "_stats_out", None)
    if out is None or out.numel() < 1 + 3 * N + need // 8:
        out = torch.empty((1 + 3 * N + need // 8,), dtype=torch.float64, device=fr.device)  # the sums, then the scratch
        try:
            buf._stats_out = out
        except AttributeError:
            pass
    with torch.cuda.device(fr.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(L.skyjo_vec_episode_stats(C.c_void_p(fr.data_ptr()), C.c_void_p(ee.data_ptr()), rows, N, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(out[1 + 3 * N:].data_ptr()), need, stream))
        host = out[: 1 + 3 * N].cpu()
    return stats_from_sums(host.tolist(), N)


def evaluate(env, seats, T, seed=0, first_ticket=0, first_records=None):
    """``play`` for T iterations on a buffer of its own, then ``episode_stats``."""
    from . import rollout

    buf = rollout.RolloutBuffer(env, T)
    play(env, seats, buf, seed=seed, first_ticket=first_ticket, first_records=first_records)
    return episode_stats(buf)
