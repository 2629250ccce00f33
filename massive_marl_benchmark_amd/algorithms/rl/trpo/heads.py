"""The head of TRPO's policy step (agents/algorithms/rl/trpo/trpo.py:287-298, 417-435, 464-478 behind ActorCritic.evaluate) as one
call: `mms_trpo_heads` (include/mms.h: csrc/trpo_loss_kernels.hip on the GPU, the CPU build for CPU tensors).

    res = trpo_heads(log_std, mu=..., rmu=..., stored=StoredRows(storage, indices), old_logp=None, want=("out", "logp", ...))

`want` names the outputs: "out" (a 2-vector {a_loss, kl} on the device), "logp" [M], "gsur", "gkl", "gn" [M, A]; `res` maps each to a
new tensor.  `stored` holds the flat views of a RolloutStorage's fields and the minibatch's index vector: the entry reads them where
they lie.  `old_logp` (a dense [M] vector) replaces the stored log-probabilities, as the reference's line search does from its second
evaluation on.  Nothing here is differentiable: TRPO takes its derivatives by hand (trpo.py's `fused_update` and `fvp="direct"`)."""
import ctypes

import torch

from .... import _lib
from ..ppo.loss import MAX_A, _p, _workspace

OUTPUTS = ("out", "logp", "gsur", "gkl", "gn")


class StoredRows:
    """The flat views of the rollout's fields that the head reads through `indices` (a list or an int64 tensor of the minibatch's rows)."""

    def __init__(self, storage, indices):
        s = storage
        A = s.actions.size(-1)
        dev = s.actions.device
        if not torch.is_tensor(indices):
            indices = torch.as_tensor(indices, dtype=torch.int64, device=dev)       # a list of indices: one copy to the device
        self.indices = indices
        self.actions, self.old_mu, self.old_sigma = s.actions.view(-1, A), s.mu.view(-1, A), s.sigma.view(-1, A)
        self.old_logp, self.adv = s.actions_log_prob.view(-1), s.advantages.view(-1)
        self.rows = indices.numel()

    def qualifies(self):
        ts = (self.actions, self.old_mu, self.old_sigma, self.old_logp, self.adv)
        dev = self.actions.device
        return (all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in ts) and self.indices.dtype == torch.int64
                and self.indices.is_contiguous() and self.indices.device == dev and 1 <= self.actions.shape[1] <= MAX_A and self.rows >= 1)


def trpo_heads(log_std, mu=None, rmu=None, stored=None, old_logp=None, want=("out", "logp")):
    """See the module docstring.  Raises on inputs the entry does not take: a missing kernel path is an error, not a torch fallback."""
    lead = mu if mu is not None else rmu
    M, A = lead.shape
    dev = lead.device
    dense = [t for t in (mu, rmu, old_logp, log_std) if t is not None]
    if not all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in dense) or (stored is not None and not stored.qualifies()):
        raise ValueError("trpo_heads: inputs must be contiguous float32 tensors on one device, indices int64, at most %d actions" % MAX_A)
    if stored is not None and stored.rows != M:
        raise ValueError("trpo_heads: mu has %d rows, the minibatch %d" % (M, stored.rows))
    L, idx, stream = _lib.for_device(dev)
    shapes = {"out": (2,), "logp": (M,), "gsur": (M, A), "gkl": (M, A), "gn": (M, A)}
    res = {k: torch.empty(shapes[k], device=dev) for k in want}
    s = stored
    head = (idx, M, A, _p(mu), _p(log_std), _p(rmu), _p(s.indices if s else None), _p(s.actions if s else None), _p(s.adv if s else None),
            _p(s.old_mu if s else None), _p(s.old_sigma if s else None), _p(old_logp if old_logp is not None else (s.old_logp if s else None)),
            1 if old_logp is not None else 0, *[_p(res.get(k)) for k in OUTPUTS])
    nbytes = ctypes.c_int64(-1)
    _lib.check(L.mms_trpo_heads(*head, None, ctypes.byref(nbytes), stream), None, "mms_trpo_heads size query", L)
    ws = _workspace(nbytes.value, dev)
    _lib.check(L.mms_trpo_heads(*head, ctypes.c_void_p(ws), ctypes.byref(nbytes), stream), None, "mms_trpo_heads", L)
    return res
