"""numpy restatement of the global-norm gradient clipping in front of the native Adam (include/skyjo_vec.h: skyjo_vec_grad_norm,
skyjo_vec_mlp_adam_step_clipped) and the synthetic segment lists of tests/test_gpu_grad_clip.py.  Written from the
header and from torch.nn.utils.clip_grad_norm_; it shares no code with the library.  Not collected: a helper.

    norm   = sqrt(sum over every element of every tensor of x^2)                                  in float64
    coef   = clamp(max_norm / (norm + 1e-6), max=1)                                               as torch forms it in float32:
             (1 / (norm32 + 1e-6f)) * max_norm32 - ``max_norm / tensor`` is ``tensor.reciprocal() * max_norm``, two roundings -
             and the clamp keeps a NaN; max_norm = +inf measures only: 1
"""
import numpy as np

from tests import mlp_pack_ref

F32 = np.float32
H = mlp_pack_ref.H


def norm(tensors):
    """The global L2 norm of a list of arrays, float64 (squares and sum in float64; inf and NaN propagate)."""
    with np.errstate(all="ignore"):
        return float(np.sqrt(sum(float(np.sum(np.square(np.asarray(t, dtype=np.float64)))) for t in tensors)))


def coef32(norm32, max_norm):
    """The coefficient for a float32 norm, numpy float32, bit for bit what torch's clip_grad_norm_ multiplies the gradients by."""
    n, mx = F32(norm32), F32(max_norm)
    if np.isposinf(mx):
        return F32(1.0)
    with np.errstate(all="ignore"):
        c = F32(F32(F32(1.0) / F32(n + F32(1e-6))) * mx)
    return c if np.isnan(c) or c < F32(1.0) else F32(1.0)


def coef64(norm64, max_norm):
    """The same rule in float64, for the float64 step of the comparison with torch."""
    return min(1.0, float(max_norm) / (float(norm64) + 1e-6))


def ulps(a, b):
    """The distance of two finite float32 of one sign in units of the last place."""
    return abs(int(F32(a).view(np.int32)) - int(F32(b).view(np.int32)))


def bits(x):
    return int(F32(x).view(np.uint32))


def branch_shapes(obs_dim, out_dim):
    return ((H, obs_dim), (H,), (H, H), (H,), (out_dim, H), (out_dim,))


def pair_grads(obs_dim, step=1):
    """The twelve gradient tensors of a policy (obs_dim, 26) beside a value branch (obs_dim, 1): ``mlp_pack_ref.adam_grads``, the
    seeds tests/test_gpu_mlp_update.py gives the two branches."""
    return (mlp_pack_ref.adam_grads(branch_shapes(obs_dim, 26), step, seed=77) + mlp_pack_ref.adam_grads(branch_shapes(obs_dim, 1), step, seed=78))


def _laid_out(arrays, offsets=None, fill=np.nan):
    """One flat float32 buffer holding ``arrays`` in order, array i starting at a position that is ``offsets[i]`` modulo 4 (None: back
    to back), and the views [(start, count)].  The floats between and around the views hold ``fill`` - NaN: a read outside a view
    shows in the norm."""
    flat, views, at = [], [], 0
    for i, a in enumerate(arrays):
        a = np.ascontiguousarray(a, dtype=F32).reshape(-1)
        gap = 0 if offsets is None else 4 + (offsets[i] - at) % 4  # (at least 4 floats of filler in front of every view)
        flat.append(np.full(gap, fill, dtype=F32)), flat.append(a)
        views.append((at + gap, a.size))
        at += gap + a.size
    flat.append(np.full(8, fill, dtype=F32))
    return np.concatenate(flat), views


UNALIGNED_COUNTS = (1, 2, 3, 5, 26, 255, 0)


def cases():
    """name -> dict(flat float32 buffer, views [(start, count)] into it, max_norm): the segment lists (a) .. (i) of
    tests/test_gpu_grad_clip.py.  The buffer goes to the device as one allocation, so a view's alignment there is its start modulo 4."""
    rng = np.random.default_rng(2024)
    normal = lambda n, scale=1.0: (rng.normal(0.0, 1.0, n) * scale).astype(F32)
    out = {}

    def add(name, arrays, max_norm, offsets=None):
        flat, views = _laid_out(arrays, offsets)
        out[name] = dict(flat=flat, views=views, max_norm=float(max_norm))

    pair = pair_grads(17)
    # (a) back to back: the policy's 77 082 floats put the value branch's tensors at 2 modulo 4
    add("a_pair_17", pair, 0.5 * norm(pair))
    # (b) every count at every odd alignment
    counts = [c for c in UNALIGNED_COUNTS for _ in (1, 2, 3)]
    add("b_unaligned", [normal(c) for c in counts], 1.0, offsets=[o for _ in UNALIGNED_COUNTS for o in (1, 2, 3)])
    add("c_one_element", [np.array([-3.25], dtype=F32)], 1.0, offsets=[3])
    # (d) 32 segments: every alignment, empty ones, one longer than a round of the workgroup (1024 groups of 4)
    counts = [0, 1, 4, 7, 64, 300, 5001, 33] * 4
    add("d_32_segments", [normal(c) for c in counts], 7.0, offsets=[i % 4 for i in range(32)])
    add("e_zeros", [np.zeros(c, dtype=F32) for c in (5, 1024, 0, 77)], 1.0, offsets=[1, 0, 2, 3])
    add("f_huge", [normal(c, 1e25) for c in (300, 2, 4100)], 1.0, offsets=[2, 0, 1])      # squares around 1e50: above float32's range
    add("f_tiny", [normal(c, 1e-30) for c in (300, 2, 4100)], 1.0, offsets=[2, 0, 1])     # ... around 1e-60: below it
    with_nan, with_inf = [normal(c) for c in (300, 4100)], [normal(c) for c in (300, 4100)]
    with_nan[1][4099] = np.nan
    with_inf[0][1] = np.inf
    add("g_nan", with_nan, 1.0, offsets=[1, 0])
    add("h_inf", with_inf, 1.0, offsets=[1, 0])
    add("i_measure_only", [normal(c, 10.0) for c in (300, 4100)], np.inf, offsets=[3, 0])
    return out
