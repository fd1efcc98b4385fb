"""PPO-style rollout collection for config 5, all on the GPU and all behind ONE call of the C ABI
(``skyjo_vec_model_rollout``): per lockstep iteration one launch evaluates the policy branch with its masked categorical draw
and the value branch on the matrix cores, and the step kernel writes the next records straight into the buffer and - the lane
that ends an episode - the episode-end flag and the final rewards: two launches per iteration, no torch kernel, no host code
between them.  ``collect_stepwise`` is the same loop made one launch at a time from Python (``FusedNet.act(value_net=...)``,
``skyjo_vec_step_collect``): same bits, used by the tests.  What a learner needs per step of the acting seat
(``rlskyjo/models/train_model_simple_rllib.py:22-59`` has RLlib collect the same columns): observation / action mask (inside the
records), action, log-probability, value estimate, the acting agent, done flags and - at episode ends - the final rewards of
skyjo_env.py:293-312 for every seat.  ``RolloutBuffer.valid`` tells a learner which rows are transitions at all.  ``compute_targets`` adds what RLlib's PPO attaches to those
batches - ``advantages`` and ``value_targets`` by GAE per agent trajectory - in one more native call on the buffer as it lies
(``skyjo_vec_rollout_targets``).  ``select_rows`` / ``gather_rows`` / ``minibatches`` hand the buffer to a learner: the rows that
carry a target, the moments of their advantages, and shuffled minibatches as dense float tensors - again on the buffer as it lies
(``skyjo_vec_rollout_select`` / ``_gather``): no row-major copy of a tile-planar buffer, no knowledge of the record layout.
``learner.ppo_loss`` takes a ``Minibatch`` and the model's two outputs from there: the PPO loss head and its gradients in one kernel.
Where every seat trains a policy of its own (``arena.collect`` fills the same buffer with per-seat ``logp`` and ``values``),
``select_rows`` / ``minibatches`` take ``seats``: the rows in which those seats acted, with the moments of their advantages alone
(``skyjo_vec_rollout_select_seats``).  ``behaviour_logits`` adds the one column the KL penalty of RLlib's PPO loss needs and the
rollout does not record - the behaviour policy's logits per row -, ``gather_behaviour`` / ``minibatches(behaviour=True)`` hand its rows
to ``learner.ppo_loss_kl`` (``skyjo_vec_rollout_gather_logits``).  ``epoch_order`` is an epoch's shuffle without torch: a keyed bijection evaluated on
the device (``skyjo_vec_rollout_shuffle``), which ``minibatches(order=...)`` takes in place of its ``randperm``.
"""
import ctypes as C
import math
from collections import namedtuple

import torch

from . import _lib


class RolloutBuffer:
    """Columns of T lockstep iterations x B games, preallocated once and refilled by ``collect``."""

    def __init__(self, env, T):
        dev = torch.device("cuda", env.device_index)
        B, N = env.num_envs, env.num_players
        self.T, self.B, self.N = T, B, N
        self._env = env
        # records[t] = what the actor of step t saw; [T] = bootstrap.  With the engine's layout 'tile-planar-all' the buffer is tile-planar
        # ([T + 1, tiles, P, 64, 16]: the step kernel writes it from registers, the nets read it in place) and ``views`` copies
        self.planar = env.record_layout == "tile-planar-all"
        self.records = env.new_planar_records(T + 1) if self.planar else env.new_records(T + 1)
        self.actions = torch.empty((T, B), dtype=torch.int32, device=dev)
        self.logp = torch.empty((T, B), dtype=torch.float32, device=dev)
        self.values = torch.empty((T + 1, B, 1), dtype=torch.float32, device=dev)
        self.final_rewards = torch.zeros((T, B, N), dtype=torch.float64, device=dev)  # non-zero rows where episode_end[t]
        self.episode_end = torch.zeros((T, B), dtype=torch.uint8, device=dev)          # 1 where the step ended the episode

    def views(self, env=None):
        """Zero-copy column views of the stored records: observations int8 [T+1, B, D], action_mask int8 [T+1, B, 26],
        agent / phase / done / status uint8 [T+1, B]."""
        e = env or self._env
        return e.split(e.rows_from_planar(self.records) if self.planar else self.records)

    @property
    def valid(self):
        """bool [T, B]: row t of game b is a transition.  Where ``records[t]`` already shows ``done`` the step only re-deals
        the game (auto-reset: the action, log-probability and value stored for it were ignored) - mask those rows out."""
        return self.views().done[: self.T] == 0


def _layout(planar):
    """The C ABI's record layout constant for ``planar``: the flag, or a buffer that has it."""
    return _lib.REC_TILE_PLANAR if getattr(planar, "planar", planar) else _lib.REC_ROW_MAJOR


def _check_layout(env, buf):
    """``buf.planar`` is what the engine writes, or ``ValueError``."""
    if buf.planar != (env.record_layout == "tile-planar-all"):
        raise ValueError(f"buf.planar={buf.planar}, but the engine's record layout is {env.record_layout!r}")


def _check_handoff(env, buf):
    """``buf.planar`` is captured when the buffer is made, the engine reads its layout when it is called, and the native calls take no
    size: a buffer of the other layout would be overrun (num_envs % 64 != 0) or silently filled in the other layout."""
    _check_layout(env, buf)
    want = (buf.T + 1) * (env.tiles * 64 if buf.planar else env.num_envs) * env.record_bytes
    r = buf.records
    if r.dtype != torch.uint8 or not r.is_contiguous() or r.numel() != want:
        raise ValueError(f"buf.records must be contiguous uint8 of {want} bytes (T + 1 = {buf.T + 1} iterations, planar={buf.planar}), "
                         f"not {r.numel()} of shape {tuple(r.shape)}")


def _first(env, buf, first_records):
    _check_handoff(env, buf)
    if first_records is None:
        env.observe(out=buf.records[0])
    else:
        buf.records[0].copy_(first_records)


@torch.no_grad()
def collect(env, policy, value, buf, seed=0, first_ticket=0, first_records=None, no_masking=False):
    """Fill ``buf`` with T steps of the current policy in one native call.  ``policy`` / ``value``: ``FusedNet`` of the
    model's two branches.  ``first_records``: the records the rollout starts from (default: ``env.observe()``)."""
    L = _lib.load()
    vp = lambda t: t.data_ptr()
    _first(env, buf, first_records)
    b = _lib.RolloutBuffers(vp(buf.records), vp(buf.actions), vp(buf.logp), vp(buf.values), vp(buf.final_rewards), vp(buf.episode_end))
    _lib.check(L.skyjo_vec_model_rollout(env._h, policy._h, value._h, buf.T, int(seed), int(first_ticket), 1 if no_masking else 0,
                                         C.byref(b), env._stream()))
    return buf


@torch.no_grad()
def collect_stepwise(env, policy, value, buf, seed=0, first_ticket=0, first_records=None):
    """The same rollout, one launch at a time from Python (the net, then ``skyjo_vec_step_collect``): bit-identical columns."""
    L = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    _first(env, buf, first_records)
    for t in range(buf.T):
        policy.act(env, buf.records[t], seed=seed, ticket=first_ticket + t, actions=buf.actions[t], logp=buf.logp[t],
                   value_net=value, values=buf.values[t], planar=buf.planar)
        # a game that ends in this step has its flag and its final rewards written by the step kernel itself
        _lib.check(L.skyjo_vec_step_collect(env._h, vp(buf.actions[t]), vp(buf.records[t + 1]), vp(buf.final_rewards[t]),
                                            vp(buf.episode_end[t]), env._stream()))
    value(buf.records[buf.T], out=buf.values[buf.T], planar=buf.planar)
    return buf


@torch.no_grad()
def compute_targets(buf, gamma=0.99, lam=1.0):
    """Learner targets of a filled buffer in one native call (``skyjo_vec_rollout_targets``; RLlib's PPO defaults, which the
    reference's script leaves as they are: gamma 0.99, lambda 1.0): per-seat GAE over the T x B rows, read in the buffer's own
    layout - a tile-planar buffer is not unpacked.  Adds to ``buf`` (allocated on first use, refilled afterwards):
    ``advantages`` / ``value_targets`` / ``returns`` float32 [T, B] and ``target_flags`` uint8 [T, B] (bit ``_lib.TGT_HAS_TARGET``:
    the row has an advantage and a value target; bit ``_lib.TGT_EPISODE_KNOWN``: the row is a transition whose episode ended
    inside the buffer and ``returns`` is its seat's final reward).  Returns ``buf``."""
    L = _lib.load()
    if getattr(buf, "advantages", None) is None:
        dev = buf.actions.device
        buf.advantages = torch.empty((buf.T, buf.B), dtype=torch.float32, device=dev)
        buf.value_targets = torch.empty((buf.T, buf.B), dtype=torch.float32, device=dev)
        buf.returns = torch.empty((buf.T, buf.B), dtype=torch.float32, device=dev)
        buf.target_flags = torch.empty((buf.T, buf.B), dtype=torch.uint8, device=dev)
    vp = lambda t: t.data_ptr()
    _lib.check(L.skyjo_vec_rollout_targets(buf._env._h, vp(buf.records), _layout(buf), buf.T,
                                           vp(buf.values), buf.values.shape[-1], vp(buf.final_rewards), vp(buf.episode_end),
                                           float(gamma), float(lam), vp(buf.advantages), vp(buf.value_targets), vp(buf.returns),
                                           vp(buf.target_flags), buf._env._stream()))
    return buf


@torch.no_grad()
def behaviour_logits(buf, policy_net):
    """Fill ``buf.behaviour``, float32 [T, B, 26]: the raw (unmasked) logits of ``policy_net`` - the packed ``FusedNet`` that PLAYED the
    rollout - on ``buf.records[:T]``, read in the buffer's own layout by the net's forward kernel (``FusedNet.__call__``,
    ``skyjo_vec_mlp_forward_layout``): what ``learner.ppo_loss_kl`` takes the behaviour distribution from.  The rollout kernels keep
    only ``logp`` of the chosen action; this is the same net on the same records once more, so
    ``log_softmax(behaviour + log_mask)[action]`` is ``buf.logp`` within the two kernels' rounding.  The column is allocated on first
    use and refilled afterwards; it costs T * B * 104 bytes.  A row-major buffer, and a tile-planar one of whole tiles, is ONE launch;
    a tile-planar buffer with B % 64 != 0 goes one iteration at a time (T launches), each into the first B rows of its blocks - the
    padding slots of the last tile are never rows.

    Call it BEFORE the first optimiser step of the update: ``learner.NativeAdam`` re-packs the net in place, and after a step the net
    is no longer the policy that played.  For an ``arena.collect`` buffer pass the net of the seat(s) about to be updated: the rows
    in which another seat acted then hold that net's logits on a position it did not play - values nobody reads, since
    ``minibatches(seats=...)`` selects the seat's own rows.  Returns ``buf``."""
    _check_records(buf)
    if policy_net.out_dim != 26 or policy_net.obs_dim != buf._env.obs_dim:
        raise ValueError(f"policy_net must be a policy branch of this engine ({buf._env.obs_dim} inputs, 26 outputs), not "
                         f"{policy_net.obs_dim} -> {policy_net.out_dim}")
    if getattr(buf, "behaviour", None) is None:
        buf.behaviour = torch.empty((buf.T, buf.B, 26), dtype=torch.float32, device=buf.actions.device)
    T = buf.T
    if not buf.planar or buf.B % 64 == 0:
        policy_net(buf.records[:T], out=buf.behaviour, planar=buf.planar)
    else:
        for t in range(T):
            policy_net(buf.records[t], out=buf.behaviour[t], planar=True)
    return buf


Selection = namedtuple("Selection", ["index", "count", "mean", "std"])
Minibatch = namedtuple("Minibatch", ["observations", "log_mask", "actions", "logp", "advantages", "value_targets", "values", "seats"])


def _check_records(buf):
    """``buf.planar`` must describe ``buf.records``: [T + 1, tiles, P, 64, 16] tile-planar, [T + 1, B, record_bytes] row-major."""
    e, r = buf._env, buf.records
    want = (buf.T + 1, e.tiles, e.record_bytes // 16, 64, 16) if buf.planar else (buf.T + 1, buf.B, e.record_bytes)
    if tuple(r.shape) != want or not r.is_contiguous():
        raise ValueError(f"buf.records has shape {tuple(r.shape)}, but planar={buf.planar} means {want}")


def _check_index(buf, index, tensor=False):
    """``index`` holds row ids for a gather from ``buf``, or ``ValueError``; ``tensor``: for anything that is no tensor as well."""
    if (tensor and not isinstance(index, torch.Tensor)) or index.dtype != torch.int64 or index.dim() != 1 or index.device != buf.actions.device:
        raise ValueError("index must be a one-dimensional int64 tensor on the buffer's device")


def _seat_mask(buf, seats):
    """The bit mask of ``seats`` (an iterable of seat numbers below ``buf.N``, at least one), or ``ValueError``."""
    mask = 0
    for s in seats:
        if isinstance(s, bool) or int(s) != s or not 0 <= int(s) < buf.N:
            raise ValueError(f"seats holds {s!r}: seat numbers are integers in 0 .. {buf.N - 1}")
        mask |= 1 << int(s)
    if not mask:
        raise ValueError("seats is empty: name at least one seat, or pass None for every seat")
    return mask


@torch.no_grad()
def select_rows(buf, require=_lib.TGT_HAS_TARGET, seats=None):
    """The rows of a buffer whose ``target_flags`` have every bit of ``require`` (``compute_targets`` must have run), in one native
    call (``skyjo_vec_rollout_select``): ``Selection(index, count, mean, std)`` - ``index`` int64 [count], ascending row ids
    ``t * B + b`` (what ``torch.nonzero`` gives; a view of ``buf.row_index``, int64 [T * B], allocated once and refilled by every
    call), ``mean`` / ``std`` Python floats: the moments of the selected rows' ``advantages``, computed in double from the two sums
    the kernel returns, ``std`` unbiased like ``torch.std`` (0.0 for fewer than two rows).  Reading back the count (with the sums,
    one copy) is the only synchronisation.  ``seats``: an iterable of seat numbers - only the rows in which one of these seats acted
    (``skyjo_vec_rollout_select_seats``: the record's agent byte, read in place), with the moments of those rows alone: a seat that
    trains a policy of its own on an ``arena.collect`` buffer; None: every seat."""
    if getattr(buf, "target_flags", None) is None:
        raise ValueError("select_rows needs the columns of compute_targets(buf)")
    _check_records(buf)
    mask = None if seats is None else _seat_mask(buf, seats)
    L = _lib.load()
    n = buf.T * buf.B
    if getattr(buf, "row_index", None) is None:
        dev = buf.actions.device
        buf.row_index = torch.empty((n,), dtype=torch.int64, device=dev)
        buf._select_out = torch.empty((3,), dtype=torch.int64, device=dev)  # the count, then the two sums (as doubles)
    out = buf._select_out
    if mask is None:
        _lib.check(L.skyjo_vec_rollout_select(buf._env._h, buf.target_flags.data_ptr(), n, int(require), buf.advantages.data_ptr(),
                                              buf.row_index.data_ptr(), out.data_ptr(), out[1:].data_ptr(), buf._env._stream()))
    else:
        _lib.check(L.skyjo_vec_rollout_select_seats(buf._env._h, buf.records.data_ptr(), _layout(buf),
                                                    buf.T, buf.target_flags.data_ptr(), int(require), mask, buf.advantages.data_ptr(),
                                                    buf.row_index.data_ptr(), out.data_ptr(), out[1:].data_ptr(), buf._env._stream()))
    host = out.cpu()
    count = int(host[0])
    s, q = (float(x) for x in host[1:].view(torch.float64))
    mean = s / count if count else 0.0
    std = math.sqrt(max(q - s * s / count, 0.0) / (count - 1)) if count > 1 else 0.0
    return Selection(buf.row_index[:count], count, mean, std)


def new_minibatch(buf, size):
    """An empty ``Minibatch`` of ``size`` rows for ``gather_rows(..., out=)``."""
    dev, f = buf.actions.device, torch.float32
    e = lambda *shape, dtype=f: torch.empty(shape, dtype=dtype, device=dev)
    return Minibatch(e(size, buf._env.obs_dim), e(size, 26), e(size, dtype=torch.int64), e(size), e(size), e(size), e(size),
                     e(size, dtype=torch.uint8))


@torch.no_grad()
def gather_rows(buf, index, normalize=None, out=None):
    """The rows ``index`` (int64 row ids ``t * B + b`` on the buffer's device, any order, repeats allowed) as a ``Minibatch`` of
    dense tensors, one native call (``skyjo_vec_rollout_gather``) on the buffer as it lies: ``observations`` float32 [m, D],
    ``log_mask`` float32 [m, 26] (0 where the action is legal, ``FLOAT_MIN`` where not: add it to the logits), ``actions`` int64,
    ``logp`` / ``advantages`` / ``value_targets`` / ``values`` float32 and ``seats`` uint8 [m].  ``normalize``: ``(mean, std)`` -
    advantages come as ``(a - mean) / std`` in float32 - or None, which leaves them as they are.  ``out``: a ``Minibatch`` of at
    least m rows to refill (``new_minibatch``); its first m rows are returned.  A row id outside [0, T * B) gives a row of zeros."""
    if getattr(buf, "advantages", None) is None:
        raise ValueError("gather_rows needs the columns of compute_targets(buf)")
    _check_records(buf)
    _check_index(buf, index)
    index = index.contiguous()
    m = index.numel()
    mean, std = (0.0, 1.0) if normalize is None else normalize
    if out is None:
        out = new_minibatch(buf, m)
    elif any(c.shape[0] < m or not c.is_contiguous() for c in out):
        raise ValueError("out holds fewer rows than index")
    L = _lib.load()
    vp = lambda t: t.data_ptr()
    _lib.check(L.skyjo_vec_rollout_gather(buf._env._h, vp(buf.records), _layout(buf), buf.T,
                                          vp(index), m, vp(buf.actions), vp(buf.logp), vp(buf.values), buf.values.shape[-1],
                                          vp(buf.advantages), vp(buf.value_targets), float(mean), float(std), vp(out.observations),
                                          vp(out.log_mask), vp(out.actions), vp(out.logp), vp(out.advantages), vp(out.value_targets),
                                          vp(out.values), vp(out.seats), buf._env._stream()))
    return out if out.actions.shape[0] == m else Minibatch(*(c[:m] for c in out))


@torch.no_grad()
def gather_behaviour(buf, index, out=None):
    """The rows ``index`` of ``buf.behaviour`` (``behaviour_logits`` must have run) as float32 [m, 26], one native call
    (``skyjo_vec_rollout_gather_logits``): ``index`` as for ``gather_rows`` - any order, repeats allowed, a row id outside [0, T * B)
    gives a row of zeros.  ``out``: a contiguous float32 [>= m, 26] tensor on the buffer's device to refill; its first m rows are
    returned."""
    col = getattr(buf, "behaviour", None)
    if col is None:
        raise ValueError("gather_behaviour needs the column of behaviour_logits(buf, policy_net)")
    dev = buf.actions.device
    _check_index(buf, index, tensor=True)
    if col.dtype != torch.float32 or tuple(col.shape) != (buf.T, buf.B, 26) or col.device != dev or not col.is_contiguous():
        raise ValueError(f"buf.behaviour must be a contiguous float32 tensor of shape [{buf.T}, {buf.B}, 26] on {dev}")
    index = index.contiguous()
    m = index.numel()
    if out is None:
        out = torch.empty((m, 26), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 26 or out.shape[0] < m
          or out.device != dev or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous float32 tensor of shape [>= m, 26] on the buffer's device, starting on a 16-byte boundary")
    if m == 0:  # (an empty index has no address to pass)
        return out[:0]
    with torch.cuda.device(dev):
        _lib.check(_lib.load().skyjo_vec_rollout_gather_logits(col.data_ptr(), buf.T * buf.B, index.data_ptr(), m, out.data_ptr(),
                                                               buf._env._stream()))
    return out[:m]


@torch.no_grad()
def epoch_order(sel, seed, epoch, out=None):
    """The selection ``sel`` (a ``Selection``) in the shuffled order of ``(seed, epoch)``, one native call that needs no torch generator
    (``skyjo_vec_rollout_shuffle``, csrc/skyjo_epoch.h): returns ``(order, fault)`` - ``order`` int64 [count] with
    ``order[j] = sel.index[perm(j)]``, ``perm`` a keyed bijection of [0, count) that is a pure function of ``(count, seed, epoch, j)``
    (include/skyjo_vec.h has it; tests/epoch_order_ref.py restates it), and ``fault`` int64 [1] ON THE DEVICE: the number of positions
    whose walk hit its cap and hold -1 (a row of zeros to ``gather_rows``) - 0 unless the kernel has a bug; read it when you read your
    other statistics.  Nothing is read back here: no synchronisation.  ``seed``: 0 .. 2^64 - 1, ``epoch``: 0 .. 2^32 - 1.  ``out``: a
    contiguous int64 tensor of at least count entries on the index's device, not overlapping it, to refill; its first count entries
    are returned.  What ``minibatches(order=...)`` takes, and what ``skyjo_vec_ppo_update`` does per epoch by itself."""
    index, count = sel.index, int(sel.count)
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1 or index.device.type != "cuda" or not index.is_contiguous():
        raise ValueError("sel.index must be a contiguous one-dimensional int64 tensor on a GPU")
    if index.numel() != count:
        raise ValueError("sel.index does not hold sel.count entries")
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 1 << 64:
        raise ValueError("seed must be an integer in 0 .. 2^64 - 1")
    if isinstance(epoch, bool) or int(epoch) != epoch or not 0 <= int(epoch) < 1 << 32:
        raise ValueError("epoch must be an integer in 0 .. 2^32 - 1")
    dev = index.device
    if out is None:
        out = torch.empty((count,), dtype=torch.int64, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or out.dim() != 1 or out.numel() < count or out.device != dev
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous one-dimensional int64 tensor of at least count entries on the index's device")
    fault = torch.zeros((1,), dtype=torch.int64, device=dev)
    if count == 0:  # (an empty index has no address to pass)
        return out[:0], fault
    with torch.cuda.device(dev):
        rc = _lib.load().skyjo_vec_rollout_shuffle(index.data_ptr(), count, int(seed), int(epoch), out.data_ptr(), fault.data_ptr(),
                                                   torch.cuda.current_stream(dev).cuda_stream)
    if rc == _lib.E_INVALID:
        raise ValueError(_lib.load().skyjo_vec_last_error().decode())
    _lib.check(rc)
    return out[:count], fault


def minibatches(buf, size, generator=None, normalize=True, require=_lib.TGT_HAS_TARGET, selection=None, seats=None, order=None, behaviour=False):
    """One epoch over the selected rows in shuffled minibatches: ``select_rows`` (or a ``selection`` made earlier), a
    ``torch.randperm`` of it (``generator``: a generator on the buffer's device), and ``gather_rows`` per slice of ``size`` rows into
    ONE ``Minibatch`` that every step refills - use a batch before asking for the next.  The last slice may be short.
    ``order``: the epoch's shuffled index itself, int64 [count] on the buffer's device (``epoch_order(selection, seed, epoch)``), taken
    instead of the ``randperm`` draw - the generator is not touched; None: everything as described.
    ``normalize``: True - the selection's (mean, std), a std of 0 counting as 1; ``(mean, std)``; or None / False.  ``seats``: as for
    ``select_rows`` - the rows of these seats only, normalised with their own moments (``ValueError`` next to a ``selection``, which
    has chosen its rows already).  ``behaviour``: True - every step yields ``(minibatch, old_logits)``, ``old_logits`` float32 [m, 26] the
    same rows of ``buf.behaviour`` (``gather_behaviour``; ``behaviour_logits`` must have run), refilled in place like the minibatch."""
    if behaviour and getattr(buf, "behaviour", None) is None:
        raise ValueError("behaviour=True needs the column of behaviour_logits(buf, policy_net)")
    if seats is not None and selection is not None:
        raise ValueError("seats belongs to the selection: pass select_rows(buf, require, seats=...) as selection, or seats alone")
    sel = (select_rows(buf, require) if seats is None else select_rows(buf, require, seats=seats)) if selection is None else selection
    if normalize is True:
        normalize = (sel.mean, sel.std if sel.std > 0.0 else 1.0)
    elif normalize is False:
        normalize = None
    if order is None:
        perm = sel.index[torch.randperm(sel.count, device=sel.index.device, generator=generator)]
    else:
        _check_index(buf, order, tensor=True)
        if order.numel() != sel.count:
            raise ValueError(f"order holds {order.numel()} entries, the selection {sel.count}")
        perm = order
    out = new_minibatch(buf, min(size, sel.count))
    old = torch.empty((out.actions.shape[0], 26), dtype=torch.float32, device=sel.index.device) if behaviour else None
    for k in range(0, sel.count, size):
        mb = gather_rows(buf, perm[k:k + size], normalize=normalize, out=out)
        yield (mb, gather_behaviour(buf, perm[k:k + size], out=old)) if behaviour else mb
