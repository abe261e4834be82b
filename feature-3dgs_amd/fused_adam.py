"""`FusedAdam`: torch.optim.Adam for the Gaussian parameters as ONE HIP launch over all tensors.

A `torch.optim.Optimizer` with torch.optim.Adam's param_groups and STATE LAYOUT (`step`, `exp_avg`, `exp_avg_sq`), so the
reference's densification code, which edits the optimizer state directly (scene/gaussian_model.py:285-382:
`replace_tensor_to_optimizer`, `_prune_optimizer`, `cat_tensors_to_optimizer`), works on it unchanged:

    self.optimizer = FusedAdam(l, lr=0.0, eps=1e-15)        # instead of torch.optim.Adam(l, lr=0.0, eps=1e-15)

No weight decay, no amsgrad (the reference uses neither).  HIP tensors only.

`capturable=True` keeps everything a step needs on the DEVICE, so that `step()` can be captured in a HIP graph and
replayed: `state["step"]` is a float32 scalar tensor on the parameter's device (torch.optim.Adam(capturable=True)'s layout; it
counts exactly up to 2^24 steps), the base rates live in a device fp64 table, and a group's rate may follow the reference's
exponential schedule (`set_lr_schedule`), evaluated on the device at the optimizer's own iteration word.  A step is then two
launches per table of up to 16 tensors - one wave that advances the step words and forms the rates and bias corrections, and
the update itself - with no host read and no host-side increment.
"""
from __future__ import annotations

import torch

from diff_gaussian_rasterization import _C

_C_MAX_TENSORS = 16     # include/f3dgs.h: F3DGS_ADAM_MAX_TENSORS


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, multi_tensor=True, capturable=False):
        defaults = dict(lr=lr, betas=betas, eps=eps)
        if capturable:
            defaults["capturable"] = True       # torch's load_state_dict then keeps `step` a float32 on the parameter's device
        super().__init__(params, defaults)
        self.multi_tensor = multi_tensor     # False: one launch per tensor (f3dgs_adam_step), as in round 2
        self.capturable = bool(capturable)
        if self.capturable:
            for group in self.param_groups:
                for p in group["params"]:
                    if not p.is_cuda:
                        raise ValueError("FusedAdam(capturable=True): HIP tensors only; got a parameter on " + str(p.device))
            self._schedules = {}        # group name -> (lr_init, lr_final, lr_delay_steps, lr_delay_mult, max_steps)
            self.schedule_epoch = 0     # bumped by set_lr_schedule: a captured step holds the schedule's constants
            self._lr_table = None       # device fp64, one base rate per param group
            self._lr_host = None        # what the table holds
            self._iteration = None      # device int64: iterations stepped so far
            self._consts = []           # per table of a step: device fp64 (16, 2) - rate used | the two fp32 constants
            self._last = []             # per table of the last step: the group index of each entry

    # ---- capturable=True: the device side --------------------------------------------------------------------------------------
    def _device(self):
        for group in self.param_groups:
            for p in group["params"]:
                return p.device
        raise RuntimeError("FusedAdam: no parameters")

    def _tables(self, n_tables=0):
        capturing = torch.cuda.is_current_stream_capturing()
        if self._lr_table is None or self._lr_table.numel() != len(self.param_groups) or len(self._consts) < n_tables:
            if capturing:
                raise RuntimeError("FusedAdam(capturable=True): the first step() must run eagerly (it allocates the optimizer's "
                                   "state and device tables); capture after a warm-up step")
            dev = self._device()
            if self._lr_table is None or self._lr_table.numel() != len(self.param_groups):
                self._lr_table = torch.zeros(len(self.param_groups), dtype=torch.float64, device=dev)
                self._lr_host = None
            if self._iteration is None:
                self._iteration = torch.zeros((), dtype=torch.int64, device=dev)
            while len(self._consts) < n_tables:
                self._consts.append(torch.zeros(_C_MAX_TENSORS, 2, dtype=torch.float64, device=dev))
        if not capturing and self._lr_host != [float(g["lr"]) for g in self.param_groups]:
            self.push_lrs()

    def push_lrs(self):
        """Uploads every group's `param_group["lr"]` into the device table of base rates.  An eager `step()` does this by itself
        when a rate changed; a captured step uploads nothing, so after changing a base rate between replays call this."""
        if not self.capturable:
            raise RuntimeError("push_lrs(): FusedAdam(capturable=True) only")
        if self._lr_table is None or self._lr_table.numel() != len(self.param_groups):
            self._lr_host = None
            self._tables()
            if self._lr_host is not None:
                return
        host = [float(g["lr"]) for g in self.param_groups]
        self._lr_table.copy_(torch.tensor(host, dtype=torch.float64))
        self._lr_host = host

    def set_lr_schedule(self, group_name, lr_init, lr_final=None, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
        """The group's rate follows the reference's exponential schedule (utils/general_utils.py:29-61: get_expon_lr_func,
        applied by update_learning_rate every iteration) instead of `param_group["lr"]`: at iteration i

            0 if lr_init == lr_final == 0, else delay(i) * exp(log(lr_init) (1 - u) + log(lr_final) u),  u = clip(i / max_steps, 0, 1)
            delay(i) = lr_delay_mult + (1 - lr_delay_mult) sin(pi/2 clip(i / lr_delay_steps, 0, 1)) if lr_delay_steps > 0, else 1

        evaluated in fp64 on the device; i is the optimizer's iteration word (`set_iteration`) plus one, i.e. the step being taken,
        as train.py calls update_learning_rate(iteration) before the step.  `lr_init=None` clears the schedule.  A captured step
        holds the schedule's constants: change them and capture again (`schedule_epoch` counts the changes)."""
        if not self.capturable:
            raise RuntimeError("set_lr_schedule(): FusedAdam(capturable=True) only")
        if not any(g.get("name") == group_name for g in self.param_groups):
            raise KeyError(f"no param_group named {group_name!r}")
        if lr_init is None:
            self._schedules.pop(group_name, None)
        else:
            lr_init, lr_final = float(lr_init), float(lr_final)
            if not (lr_init >= 0 and lr_final >= 0) or (lr_init == 0) != (lr_final == 0):
                raise ValueError(f"rates {lr_init} -> {lr_final}: both positive or both zero")
            if int(max_steps) <= 0 or int(lr_delay_steps) < 0:
                raise ValueError(f"max_steps = {max_steps}, lr_delay_steps = {lr_delay_steps}")
            self._schedules[group_name] = (lr_init, lr_final, float(int(lr_delay_steps)), float(lr_delay_mult), float(int(max_steps)))
        self.schedule_epoch += 1

    def set_iteration(self, i):
        """The number of iterations stepped so far: the next step evaluates the schedules at i + 1."""
        if not self.capturable:
            raise RuntimeError("set_iteration(): FusedAdam(capturable=True) only")
        self._tables()
        self._iteration.fill_(int(i))

    def iteration(self):
        """Iterations stepped so far; synchronises."""
        if not self.capturable:
            raise RuntimeError("iteration(): FusedAdam(capturable=True) only")
        self._tables()
        return int(self._iteration.item())

    def current_lrs(self):
        """{group name or index: the rate its last step used}; synchronises, and writes the values into `param_groups` like
        update_learning_rate does (a group that was not stepped yet reports its `lr` as it is)."""
        if not self.capturable:
            raise RuntimeError("current_lrs(): FusedAdam(capturable=True) only")
        used = {}
        for consts, groups in zip(self._consts, self._last):
            col = consts[:, 0].tolist()
            for k, gi in enumerate(groups):
                used[gi] = col[k]
        out = {}
        for gi, g in enumerate(self.param_groups):
            if gi in used:
                g["lr"] = used[gi]
            out[g.get("name", gi)] = float(g["lr"])
        return out

    def device_state(self):
        """Every device tensor a step writes apart from the parameters: step words, moments, the iteration word.  What a caller
        saves before warm-up steps it wants to undo (train_step.CapturedTrainer)."""
        if not self.capturable:
            raise RuntimeError("device_state(): FusedAdam(capturable=True) only")
        self._tables()
        out = [self._iteration]
        for st in self.state.values():
            out += [v for v in st.values() if torch.is_tensor(v) and v.is_cuda]
        return out

    def _step_capturable(self, visibility):
        capturing = torch.cuda.is_current_stream_capturing()
        work = {}      # (betas, eps, masked) -> [(param, group index)]
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise ValueError("FusedAdam(capturable=True): HIP tensors only")
                st = self.state[p]
                if "exp_avg" not in st:
                    if capturing:
                        raise RuntimeError("FusedAdam(capturable=True): the first step() of a parameter must run eagerly (it "
                                           "allocates the state); capture after a warm-up step")
                    st.setdefault("step", torch.zeros((), dtype=torch.float32, device=p.device))
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                s = st["step"]
                if not (torch.is_tensor(s) and s.is_cuda and s.dtype == torch.float32):      # state from a non-capturable run
                    if capturing:
                        raise RuntimeError("FusedAdam(capturable=True): state['step'] must be a float32 tensor on the device")
                    st["step"] = torch.as_tensor(float(s), dtype=torch.float32).to(p.device)
                masked = visibility is not None and p.dim() >= 1 and p.shape[0] == visibility.shape[0]
                work.setdefault((tuple(group["betas"]), group["eps"], masked), []).append((p, gi))
        tables = [(key, items[i:i + _C_MAX_TENSORS]) for key, items in work.items() for i in range(0, len(items), _C_MAX_TENSORS)]
        if not tables:
            return
        self._tables(len(tables))
        self._last = []
        for j, ((betas, eps, masked), items) in enumerate(tables):
            ps = [p for p, _ in items]
            sts = [self.state[p] for p in ps]
            sched = [list(self._schedules.get(self.param_groups[gi].get("name"), ())) for _, gi in items]
            _C.adam_step_multi_device(ps, [p.grad for p in ps], [s["exp_avg"] for s in sts], [s["exp_avg_sq"] for s in sts],
                                      [s["step"] for s in sts], self._lr_table, [gi for _, gi in items], sched, betas[0], betas[1],
                                      eps, self._iteration, j == 0, self._consts[j], visibility if masked else None)
            self._last.append([gi for _, gi in items])

    @torch.no_grad()
    def step(self, closure=None, visibility=None):
        """`visibility` (optional, (P,) HIP tensor: bool, uint8 or a wider integer such as `radii` itself - any non-zero
        entry means visible): an EXTENSION beyond the reference -
        only those rows of every (P, ...) tensor are stepped, the others keep parameter and moments (torch.optim.Adam
        would still move a never-visible Gaussian by its decaying first moment).  Default: the reference's dense Adam."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            self._step_capturable(visibility)
            return loss
        work = []      # (param, group) with a gradient, state initialised and stepped
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                work.append((p, group))
        # ONE launch over every tensor that shares betas / eps and (with a visibility mask) the row count - the seven
        # per-Gaussian tensors of the reference's model; whatever does not fit that takes the per-tensor entry point
        if self.multi_tensor and work:
            g0 = work[0][1]
            same = [pg for pg in work if pg[1]["betas"] == g0["betas"] and pg[1]["eps"] == g0["eps"] and pg[0].is_contiguous()
                    and (visibility is None or (pg[0].dim() >= 1 and pg[0].shape[0] == visibility.shape[0]))]
            same = same[:_C_MAX_TENSORS]
            if len(same) > 1:
                ps = [p for p, _ in same]
                _C.adam_step_multi(ps, [p.grad for p in ps], [self.state[p]["exp_avg"] for p in ps],
                                   [self.state[p]["exp_avg_sq"] for p in ps], [float(g["lr"]) for _, g in same],
                                   g0["betas"][0], g0["betas"][1], g0["eps"], [int(self.state[p]["step"]) for p in ps], visibility)
                done = {id(p) for p in ps}
                work = [pg for pg in work if id(pg[0]) not in done]
        for p, group in work:
            b1, b2 = group["betas"]
            st = self.state[p]
            mask = visibility if visibility is not None and p.dim() >= 1 and p.shape[0] == visibility.shape[0] else None
            _C.adam_step(p, p.grad, st["exp_avg"], st["exp_avg_sq"], float(group["lr"]), b1, b2, group["eps"], int(st["step"]), mask)
        return loss
