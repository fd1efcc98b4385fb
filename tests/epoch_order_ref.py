"""numpy restatement of ``skyjo_vec_rollout_shuffle``'s permutation, written from the text of include/skyjo_vec.h (not from the kernel):
a six-round balanced Feistel network on the smallest even number of bits that holds ``count``, walked from j until it lands below
``count``, the walk capped at ``WALK_CAP`` applications.  All arithmetic is uint32 with wrap-around."""
import numpy as np

ROUNDS, WALK_CAP = 6, 1024
_M32 = 0xFFFFFFFF


def fmix32(v):
    """The finaliser on a Python int or a uint32 array."""
    if isinstance(v, np.ndarray):
        v = v.astype(np.uint32)
        v = v ^ (v >> np.uint32(16))
        v = v * np.uint32(0x85EBCA6B)
        v = v ^ (v >> np.uint32(13))
        v = v * np.uint32(0xC2B2AE35)
        return v ^ (v >> np.uint32(16))
    v &= _M32
    v ^= v >> 16
    v = (v * 0x85EBCA6B) & _M32
    v ^= v >> 13
    v = (v * 0xC2B2AE35) & _M32
    return v ^ (v >> 16)


def keys(seed, epoch):
    """The six round keys of (seed, epoch) as Python ints."""
    lo, hi = seed & _M32, (seed >> 32) & _M32
    return [fmix32(lo ^ fmix32(hi ^ fmix32((epoch * 0x9E3779B9 + r) & _M32))) for r in range(ROUNDS)]


def half_bits(count):
    b = 2
    while (1 << b) < count:
        b += 2
    return b // 2


def encrypt(x, key, h):
    """E on a uint32 array."""
    mask = np.uint32((1 << h) - 1)
    L, R = x >> np.uint32(h), x & mask
    for r in range(ROUNDS):
        L, R = R, L ^ (fmix32(R + np.uint32(key[r])) & mask)
    return (L << np.uint32(h)) | R


def perm(count, seed, epoch, walks=False):
    """perm(0 .. count - 1) as an int64 array, -1 where a walk hit the cap; ``walks``: also each position's number of applications."""
    with np.errstate(over="ignore"):
        key, h = keys(seed, epoch), half_bits(count)
        x = np.arange(count, dtype=np.uint32)
        out = np.full(count, -1, dtype=np.int64)
        steps = np.zeros(count, dtype=np.int64)
        walking = np.arange(count)
        for w in range(1, WALK_CAP + 1):
            if walking.size == 0:
                break
            y = encrypt(x[walking], key, h)
            x[walking] = y
            done = y < count
            out[walking[done]] = y[done]
            steps[walking[done]] = w
            walking = walking[~done]
        steps[walking] = WALK_CAP
    return (out, steps) if walks else out


def order(index, seed, epoch):
    """``order_out`` for ``index`` (int64 array): index[perm(j)], -1 at a capped walk."""
    index = np.asarray(index, dtype=np.int64)
    p = perm(index.size, seed, epoch)
    return np.where(p >= 0, index[np.maximum(p, 0)], -1)
