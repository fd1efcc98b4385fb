"""What a byte-for-byte comparison of two PPO updates needs (tests/test_gpu_ppo_update_wide.py): a learner made from identical state, its
state as bytes, and a result's numbers as bytes.  Not collected: a helper; it needs the GPU only when ``Learner`` is made."""
import copy

import numpy as np

LR = 3e-4


def raw(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


class Learner:
    """A deep copy of ``model`` with fresh nets and a fresh NativeAdam: identical state every time."""

    def __init__(self, model, **adam):
        from skyjo_rl_amd.action_mask_model import FusedNet
        from skyjo_rl_amd.learner import NativeAdam

        self.model = copy.deepcopy(model)
        self.pol, self.val = FusedNet(self.model.policy), FusedNet(self.model.value)
        self.opt = NativeAdam(self.model, self.pol, self.val, lr=LR, **adam)
        self.params = list(self.model.policy.parameters()) + list(self.model.value.parameters())

    def state(self):
        """name -> bytes: the twelve parameters, the 24 Adam tensors, both nets' fragments and the step count."""
        out = {"steps": self.opt.steps}
        for i, p in enumerate(self.params):
            out["param %d" % i] = raw(p)
            out["exp_avg %d" % i], out["exp_avg_sq %d" % i] = raw(self.opt.state[p]["exp_avg"]), raw(self.opt.state[p]["exp_avg_sq"])
        out["fragments policy"], out["fragments value"] = raw(self.pol.export()), raw(self.val.export())
        return out

    def close(self):
        self.pol.close(), self.val.close()


def same(a, b, what):
    assert a.keys() == b.keys(), what
    bad = [k for k in a if a[k] != b[k]]
    assert bad == [], "%s: %d of %d differ, the first: %s" % (what, len(bad), len(a), bad[0])


def flat(result):
    """Every number of a ``ppo_update`` result as name -> bytes of the double (NaN-proof, sign-of-zero-proof)."""
    out = {}
    for k, v in result.items():
        for kk, x in (v.items() if isinstance(v, dict) else [("", v)]):
            out[k + "." + kk] = np.float64(x).tobytes()
    return out
