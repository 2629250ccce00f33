"""`FusedAdam`: gradient-norm clip + Adam + polyak as one call of the C ABI (`mms_param_step`, include/mms.h): two launches in
place of `nn.utils.clip_grad_norm_` + `torch.optim.Adam.step()` + the per-parameter polyak loop that end every learner's minibatch
(agents/algorithms/rl/sac/sac.py:325-349, rl/ppo/ppo.py, marl/mappo_trainer.py, marl/maddpg/module.py:280-292).

It is a `torch.optim.Optimizer` with the state keys and layout of `torch.optim.Adam` (`step`, `exp_avg`, `exp_avg_sq` per parameter),
so `state_dict()` / `load_state_dict()` go to and from `torch.optim.Adam` in both directions, and `FusedAdam.from_torch(opt)` adopts
a constructed one.  One param group.  The rule is Adam's default (no amsgrad, no maximize, coupled weight decay).  Unlike
`clip_grad_norm_`, `clip_and_step` does NOT rewrite the gradients: the clip coefficient is applied as they are read.

Where the call goes: through `_lib.for_device` to the library of the parameters' device -- the HIP build on "cuda", the CPU build on
"cpu" (when it has been built).  The C entry never falls back by itself.  These cases run THE SAME RULE in torch ops, in the same
order, inside this wrapper (`_torch_path`), and that is all they are:
  * CPU parameters without the CPU library built;
  * a parameter, gradient, moment or target that is not dense fp32 on the group's device;
  * more than 48 entries (MMS_PARAM_MAX_TENSORS) in one call;
  * parameters whose step counts differ (one of them had no gradient at an earlier step): the entry takes one step number."""
import ctypes
import os

import torch

from . import _lib

MAX_TENSORS = 48         # include/mms.h: MMS_PARAM_MAX_TENSORS
_vp = ctypes.c_void_p


def _dense(t, dev):
    return t.dtype == torch.float32 and t.device == dev and t.is_contiguous() and t.layout == torch.strided


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid betas: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        # the group carries torch.optim.Adam's own keys (whatever this torch version's are, at their defaults: the rule implemented
        # here), so that a state_dict loads on either side
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdam takes one param group (got %d)" % len(self.param_groups))
        self._partials = None

    def add_param_group(self, param_group):
        if len(self.param_groups) >= 1:
            raise ValueError("FusedAdam takes one param group")
        super().add_param_group(param_group)

    @classmethod
    def from_torch(cls, opt):
        """Adopt a constructed `torch.optim.Adam`: the same parameter objects, its hyperparameters, its state (moved, not copied)."""
        if type(opt) is not torch.optim.Adam:
            raise TypeError("FusedAdam.from_torch takes a torch.optim.Adam, not %s" % type(opt).__name__)
        if len(opt.param_groups) != 1:
            raise ValueError("FusedAdam takes one param group (got %d)" % len(opt.param_groups))
        g = opt.param_groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdam implements neither amsgrad nor maximize")
        if torch.is_tensor(g["lr"]):
            raise ValueError("FusedAdam reads lr as a host scalar (got a tensor lr)")
        new = cls(g["params"], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
        for p in g["params"]:
            if p in opt.state:
                st = opt.state.pop(p)
                step = st["step"]
                new.state[p] = {"step": step.detach().to("cpu", torch.float32) if torch.is_tensor(step) else torch.tensor(float(step)),
                                "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
        return new

    # ---- the step ----

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0)                   # torch.optim.Adam's layout: a float32 scalar on the host
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._run(None, (), None, None, False)
        return loss

    @torch.no_grad()
    def clip_and_step(self, max_norm=None, also_norm=(), targets=None, polyak=None):
        """Clip (max_norm None or <= 0: no clipping), Adam step, polyak -- one `mms_param_step`.
        also_norm: parameters outside this optimizer whose `.grad` enters the norm and nothing else.
        targets: an iterable parallel to the params (entries may be None) with `polyak`: target = target polyak + (1 - polyak) p_new,
        also for a parameter without a gradient.
        Returns a 0-d tensor on the parameters' device: the total norm BEFORE clipping (what clip_grad_norm_ / get_gard_norm return),
        over the params with a gradient and also_norm -- also when nothing is clipped.  `step()` is this without the norm."""
        return self._run(max_norm, also_norm, targets, polyak, True)

    def _run(self, max_norm, also_norm, targets, polyak, want_norm):
        group = self.param_groups[0]
        params = group["params"]
        targets = [None] * len(params) if targets is None else [None if t is None else (t.data if isinstance(t, torch.nn.Parameter) else t) for t in targets]
        if len(targets) != len(params):
            raise ValueError("targets must be parallel to the params (%d against %d)" % (len(targets), len(params)))
        if any(t is not None for t in targets) and polyak is None:
            raise ValueError("targets need polyak")
        if group.get("amsgrad") or group.get("maximize"):
            raise ValueError("FusedAdam implements neither amsgrad nor maximize")
        extra = [q for q in also_norm if q.grad is not None]
        dev = params[0].device if params else (extra[0].device if extra else torch.device("cpu"))
        # rows: (param, grad, exp_avg, exp_avg_sq, target, state)
        rows = []
        for p, t in zip(params, targets):
            if p.grad is None and t is None:
                continue
            if p.grad is not None and p.grad.is_sparse:
                raise RuntimeError("FusedAdam does not support sparse gradients")
            st = self._state_of(p) if p.grad is not None else None
            rows.append((p.data, p.grad, st["exp_avg"] if st else None, st["exp_avg_sq"] if st else None, t, st))
        rows += [(None, q.grad, None, None, None, None) for q in extra]
        stepped = [r[5] for r in rows if r[5] is not None]
        for st in stepped:
            st["step"] += 1
        steps = {int(st["step"]) for st in stepped}
        lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        mn = 0.0 if max_norm is None else float(max_norm)
        pk = 0.0 if polyak is None else float(polyak)
        native = len(rows) <= MAX_TENSORS and len(steps) <= 1 and all(x is None or _dense(x, dev) for r in rows for x in r[:5])
        if native and dev.type == "cpu" and not os.path.exists(_lib.LIB_CPU_PATH):
            native = False
        if not native:
            return self._torch_path(rows, dev, lr, beta1, beta2, eps, wd, mn, pk, want_norm)
        if not rows:
            return torch.zeros((), device=dev)
        L, idx, stream = _lib.for_device(dev)
        n = len(rows)
        numel = (ctypes.c_int64 * n)(*[(r[0] if r[0] is not None else r[1]).numel() for r in rows])
        table = lambda k: (_vp * n)(*[None if r[k] is None else r[k].data_ptr() for r in rows])
        norm = partials = None
        if want_norm:
            need = L.mms_param_step_partials(n, numel)
            if self._partials is None or self._partials.device != dev or self._partials.numel() < need:
                self._partials = torch.empty(need, dtype=torch.float64, device=dev)
            partials = _vp(self._partials.data_ptr())
            norm = torch.empty((), device=dev)
        _lib.check(L.mms_param_step(idx, n, numel, table(0), table(1), table(2), table(3), table(4), lr, beta1, beta2, eps, wd,
                                    steps.pop() if steps else 1, mn, pk, 0, partials, None if norm is None else _vp(norm.data_ptr()), stream),
                   None, "mms_param_step", L)
        return norm if norm is not None else torch.zeros((), device=dev)

    @staticmethod
    def _torch_path(rows, dev, lr, beta1, beta2, eps, wd, max_norm, polyak, want_norm):
        """mms_param_step's rule in torch ops, in its order: the norm over every gradient, the coefficient, then per tensor Adam on the
        clipped gradient (the stored gradient stays as it is) and the polyak statements."""
        total = torch.zeros((), device=dev)
        coef = None
        if want_norm:
            norms = [torch.linalg.vector_norm(r[1].to(torch.float64)) for r in rows if r[1] is not None]
            if norms:
                total = torch.linalg.vector_norm(torch.stack([v.to(dev) for v in norms])).to(torch.float32)
            if max_norm > 0.0:
                coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for p, g, m, v, t, st in rows:
            if p is not None and g is not None:
                step = int(st["step"])
                gc = g if coef is None else g * coef.to(g.device, g.dtype)
                if wd != 0.0:
                    gc = gc + wd * p
                m.add_((gc - m) * (1.0 - beta1))
                v.mul_(beta2).add_(((1.0 - beta2) * gc) * gc)
                denom = (v.sqrt() / (1.0 - beta2 ** step) ** 0.5).add_(eps)
                p.sub_((lr / (1.0 - beta1 ** step)) * (m / denom))
            if t is not None:
                t.mul_(polyak)
                t.add_((1 - polyak) * p)
        return total
