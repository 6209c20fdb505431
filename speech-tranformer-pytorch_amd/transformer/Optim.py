"""Noam-scheduled Adam (drop-in for reference transformer/Optim.py:6-45)."""
import contextlib

import torch
import torch.optim as optim

from transformer.Utils import learn_rate


class ScheduledOptim(object):
    """Adam(betas=(0.9, 0.98), eps=1e-9) whose rate is set from the global step
    before every update: ``lr = d_model^-0.5 * min(step^-0.5, step * warmup^-1.5)``.

    ``state_dict()`` / ``load_state_dict()`` speak the REFERENCE's checkpoint format (Optim.py:26-30 saves the
    state of ``Adam(model.parameters())``: one ``exp_avg`` / ``exp_avg_sq`` / ``step`` entry per parameter in
    ``model.parameters()`` order, a float learning rate) although the HIP path keeps ONE flat state over the
    parameter arena: the arena offsets give the mapping, so a checkpoint written by the reference (or by this
    class on the CPU path) resumes here and vice versa (train.py:110-114).

    Two options of the flat-arena update, both off by default (then the step launches exactly what it launched before they
    existed), both without a host read:
      * ``enable_nonfinite_guard()`` (config key ``skip_nonfinite``): a step whose gradient norm is NaN or infinite is SKIPPED -
        parameters, both moments and Adam's step count keep their bits.  ``found_inf`` (the last step's verdict) and
        ``skipped`` (the running count) are device scalars: read them when you choose, e.g. once per epoch.
      * ``enable_averaging(decay, warmup)`` (config keys ``ema_decay``, ``ema_warmup``): an exponential moving average of the
        weights, kept by the update kernel in the same pass; ``with optimizer.averaged():`` puts it under the model.
    With either enabled ``state_dict()`` carries one extra top-level key, ``"averaging"``.

    ``step_captured(..., window=win)`` is the update of a gradient-accumulation window (``st_amd.trainer.TrainStep(accumulate=K)``):
    the gradient buffer holds a sum whose denominator is the device scalar ``win[0]``; both options work inside it."""

    _allow_cpu_arena = False     # tests/_emul.py: exercise the arena path with emulated kernels on the CPU

    def __init__(self, model, d_model, config):
        self.lr = 0
        params = list(model.parameters())
        self._params = params
        self.arena = None
        self._norm_scratch = None
        if params and (all(p.is_cuda for p in params) or ScheduledOptim._allow_cpu_arena):
            # HIP path: every parameter is a view of one flat buffer (st_amd.arena), so Adam runs as a
            # single fused kernel over it instead of one multi-tensor launch chain over 258 tensors.
            # Same per-element arithmetic as the reference's per-tensor Adam; alignment gaps carry
            # zero gradients and therefore never move.
            from st_amd.arena import arena_of
            self.arena = arena_of(model)
            # the rate lives in a device scalar and the step counter on the device (capturable), so the
            # whole update can be replayed from a HIP graph while the Noam rate still changes per step
            self.lr_tensor = torch.zeros((), dtype=torch.float32, device=self.arena.device)
            on_gpu = self.arena.device.type == "cuda"
            self.optimizer = optim.Adam([self.arena.flat_parameter()], lr=self.lr_tensor, betas=(0.9, 0.98), eps=1e-9,
                                        fused=on_gpu, capturable=on_gpu, foreach=False if not on_gpu else None)
        else:
            self.optimizer = optim.Adam(params, lr=self.lr, betas=(0.9, 0.98), eps=1e-9)
        self.d_model = d_model
        self.n_warmup_steps = config.n_warmup_steps
        self._guard = None           # device f32 [2]: (verdict of the last step, number of skipped steps)
        self._avg_opts = None        # (decay, warmup) once averaging is on; the buffer is arena.avg
        self._avg_extra = []         # [(tensor, its average)] outside the arena (JointTrainStep: the CTC head)
        self._in_averaged = False
        self._state_loads = 0        # load_state_dict() calls (an accumulating TrainStep starts a fresh window after one)
        # optional keys: a reference config without them builds exactly the object above
        if getattr(config, "skip_nonfinite", None):
            self.enable_nonfinite_guard()
        if getattr(config, "ema_decay", None) is not None:
            warm = getattr(config, "ema_warmup", None)
            self.enable_averaging(decay=config.ema_decay, warmup=True if warm is None else bool(warm))

    # ---- options of the flat-arena update ----------------------------------------------------------------
    def _plain(self):
        group = self.optimizer.param_groups[0]
        return not (group["weight_decay"] or group["amsgrad"] or group["maximize"])

    def _require_hip_update(self, what):
        if self.arena is None:
            raise ValueError("ScheduledOptim.%s: needs the flat-arena path (the model on the GPU)" % what)
        if not self._plain():
            raise ValueError("ScheduledOptim.%s: weight decay / amsgrad / maximize take torch's own Adam, which has neither "
                             "the guard nor the average" % what)

    def enable_nonfinite_guard(self):
        """Skip every update whose gradient norm is not finite (see the class docstring).  Before the first capture."""
        self._require_hip_update("enable_nonfinite_guard")
        if self._guard is None:
            self._guard = torch.zeros(2, dtype=torch.float32, device=self.arena.device)

    def enable_averaging(self, decay=0.999, warmup=True):
        """Keep avg += (1 - d) * (p - avg) after every applied update; d = decay, or with warmup min(decay, (1 + t) / (10 + t))
        at Adam step count t.  The average starts as a copy of the parameters as they are now.  Before the first capture."""
        self._require_hip_update("enable_averaging")
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError("ScheduledOptim.enable_averaging: decay must lie in [0, 1], got %r" % (decay,))
        self.arena.enable_avg()
        self._avg_opts = (float(decay), bool(warmup))

    @property
    def found_inf(self):
        """Device scalar: 1 when the last step was skipped for a non-finite gradient norm, else 0 (None: guard off)."""
        return None if self._guard is None else self._guard[0]

    @property
    def skipped(self):
        """Device scalar: how many steps the guard has skipped so far (None: guard off)."""
        return None if self._guard is None else self._guard[1]

    def options_token(self):
        """What a captured step depends on: TrainStep records it at capture and refuses to replay after a change."""
        return (self._guard is not None, self._avg_opts, len(self._avg_extra))

    def averaging_weight(self):
        """Device scalar w of this step's average update, 0 on a skipped step - for tensors outside the arena, whose
        average JointTrainStep keeps with torch ops (call AFTER step_captured: the step count is already advanced)."""
        decay, warmup = self._avg_opts
        t = self._flat_state()[1]["step"]
        d = torch.clamp((1.0 + t) / (10.0 + t), max=decay) if warmup else torch.full_like(t, decay)
        w = 1.0 - d
        return w if self._guard is None else w * (1.0 - self._guard[0])

    def register_averaged(self, tensors):
        """Tensors outside the arena whose average the caller keeps (their averages start as copies): averaged() swaps
        them with the arena.  -> the list of average tensors, in order."""
        if self._avg_opts is None:
            raise ValueError("ScheduledOptim.register_averaged: averaging is not enabled")
        self._avg_extra = [(t, t.detach().clone()) for t in tensors]
        return [a for _, a in self._avg_extra]

    def _swap_averaged(self):
        from st_amd import native as nv
        nv.swap_(self.arena.flat, self.arena.avg)
        with torch.no_grad():
            for t, a in self._avg_extra:
                tmp = t.detach().clone()
                t.copy_(a)
                a.copy_(tmp)

    @contextlib.contextmanager
    def averaged(self):
        """Inside the context the model holds the averaged weights (one launch swaps ``arena.flat`` and ``arena.avg`` in
        place - parameter views and captured graphs hold addresses into the arena, so the pointers cannot be exchanged);
        the exit swaps back.  The bf16 shadow and the weight-fragment layouts are rebuilt by every outermost forward
        (``arena.scope()``), so eval forwards and Decode see the weights that are in ``flat`` at that moment.  No update may
        run inside; nesting raises."""
        if self._avg_opts is None:
            raise RuntimeError("ScheduledOptim.averaged: averaging is not enabled")
        if self._in_averaged:
            raise RuntimeError("ScheduledOptim.averaged: already inside averaged()")
        self._swap_averaged()
        self._in_averaged = True
        try:
            yield self
        finally:
            self._in_averaged = False
            self._swap_averaged()

    def step(self, global_step):
        self.update_learning_rate(global_step)
        if self._guard is not None or self._avg_opts is not None:
            self.step_captured(grad_norm=True, max_norm=float("inf"))      # (the HIP update; an infinite bound clips nothing)
            return
        self.optimizer.step()

    def _flat_state(self):
        """The flat Adam state over the arena, created the way torch.optim.Adam does lazily on its first step."""
        p = self.optimizer.param_groups[0]["params"][0]
        st = self.optimizer.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return p, st

    def norm_scratch(self, device):
        """st_grad_norm's zeroed block partials + ticket, one per optimizer; TrainStep asks for it before a graph capture."""
        if self._norm_scratch is None or self._norm_scratch.device != torch.device(device):
            from st_amd import native as nv
            self._norm_scratch = nv.grad_norm_scratch(device)
        return self._norm_scratch

    def _step_window(self, grad_norm, max_norm, grad_scale, win):
        """The update of an accumulation window: ``st_grad_norm`` + ``st_adam_clip`` with their ``win`` pointer.  The flat gradient buffer holds
        the SUM over the window's micro-batches and ``win`` (device f32 [4]) its denominator in win[0]: the norm returned and
        the gradient Adam consumes are those of ``grad_scale * g / win[0]``.  With the guard on, a non-finite norm or a
        denominator <= 0 skips the update.  Either way the gradient buffer holds ZEROS afterwards, not the clipped gradient."""
        if self.arena is None or not self._plain():
            raise ValueError("ScheduledOptim.step_captured(window=): needs the flat-arena HIP update (the model on the GPU, no "
                             "weight decay / amsgrad / maximize)")
        if grad_norm is not True or max_norm is None:
            raise ValueError("ScheduledOptim.step_captured(window=): takes grad_norm=True and a max_norm (the norm of a window "
                             "is computed here, over the divided sum)")
        if self._in_averaged:
            raise RuntimeError("ScheduledOptim.step_captured: inside averaged() the model holds the averaged weights")
        from st_amd import native as nv
        group = self.optimizer.param_groups[0]
        p, st = self._flat_state()
        self.norm_scratch(p.device)
        out = torch.empty((), dtype=torch.float32, device=p.device)
        gnorm = nv.grad_norm_win(p.grad, self._norm_scratch, out, st["step"], self._guard, win, grad_scale=grad_scale)
        averaging = self._avg_opts is not None
        decay, warmup = self._avg_opts if averaging else (1.0, False)
        beta1, beta2 = group["betas"]
        nv.adam_clip_win(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], self.lr_tensor, st["step"], gnorm, max_norm, beta1, beta2,
                         group["eps"], win, grad_scale=grad_scale, found_inf=self.found_inf,
                         avg=self.arena.avg if averaging else None, decay=decay, decay_warmup=warmup)
        return gnorm

    def step_captured(self, grad_norm=None, max_norm=None, grad_scale=1.0, window=None):
        """The update alone (rate already set with update_learning_rate) - what a HIP graph captures.
        With ``grad_norm`` and ``max_norm`` on the flat-arena path, gradient clipping (train.py:45) and the Adam update are
        two launches over the buffers: ``st_grad_norm`` (the global norm; also advances the step count) and
        ``st_adam_clip`` (clip + the arithmetic of torch's fused Adam, on this optimizer's own state tensors).
        grad_norm: True = compute it here (returned as a device scalar), or a device scalar already computed.
        grad_scale: the gradient buffer still has to be multiplied by this (st_amd.dp.GradReducer.synchronize(divide=False)
        leaves the rank SUM and returns 1 / world): folded into the norm and the clip coefficient - no pass of its own.
        With the guard or the average enabled the two launches are ``st_grad_norm`` with its guard and ``st_adam_clip`` with ``found_inf`` / ``avg``; a norm
        handed in (the joint step) gives the verdict through torch ops on that scalar - no host read either way.
        window: the device f32 [4] state of a gradient-accumulation window - see :meth:`_step_window`."""
        if window is not None:
            return self._step_window(grad_norm, max_norm, grad_scale, window)
        group = self.optimizer.param_groups[0]
        plain = not (group["weight_decay"] or group["amsgrad"] or group["maximize"])
        guard, averaging = self._guard is not None, self._avg_opts is not None
        if guard or averaging:
            if self._in_averaged:
                raise RuntimeError("ScheduledOptim.step_captured: inside averaged() the model holds the averaged weights")
            if guard and grad_norm is None:
                raise ValueError("ScheduledOptim.step_captured: the non-finite guard needs a norm (grad_norm=True or a scalar)")
            if grad_norm is None or max_norm is None or not plain:
                raise ValueError("ScheduledOptim.step_captured: the guard / the average exist in the HIP update only "
                                 "(grad_norm and max_norm given, no weight decay / amsgrad / maximize)")
        if self.arena is None or grad_norm is None:
            if grad_scale != 1.0:
                for q in self.optimizer.param_groups[0]["params"]:
                    if q.grad is not None:
                        q.grad.mul_(grad_scale)
            self.optimizer.step()
            return None
        if not plain:
            # weight decay / amsgrad / maximize: torch's own Adam does the update, the clipping still happens here (train.py:45
            # clips whatever optimizer follows) - the norm over the flat gradient, the gradient scaled in place, no host sync
            g = self._flat_state()[0].grad
            if grad_scale != 1.0:
                g.mul_(grad_scale)
            if grad_norm is True:
                grad_norm = torch.linalg.vector_norm(g.float())
            if max_norm is not None:
                g.mul_(torch.clamp(float(max_norm) / (grad_norm + 1e-6), max=1.0))
            self.optimizer.step()
            return grad_norm
        from st_amd import native as nv
        p, st = self._flat_state()
        if grad_norm is True:
            self.norm_scratch(p.device)
            out = torch.empty((), dtype=torch.float32, device=p.device)
            if guard:
                grad_norm = nv.grad_norm_guard(p.grad, self._norm_scratch, out, st["step"], self._guard, grad_scale=grad_scale)
            else:
                grad_norm = nv.grad_norm(p.grad, self._norm_scratch, out, step=st["step"], grad_scale=grad_scale)
        elif guard:
            found = (~torch.isfinite(grad_norm)).to(torch.float32).reshape(())
            self._guard[0].copy_(found)
            self._guard[1].add_(found)
            st["step"].add_(1.0 - found)
        else:
            st["step"].add_(1)
        beta1, beta2 = group["betas"]
        if guard or averaging:
            decay, warmup = self._avg_opts if averaging else (1.0, False)
            nv.adam_clip_avg(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], self.lr_tensor, st["step"], grad_norm, max_norm,
                             beta1, beta2, group["eps"], grad_scale=grad_scale, found_inf=self.found_inf,
                             avg=self.arena.avg if averaging else None, decay=decay, decay_warmup=warmup)
        else:
            nv.adam_clip(p.data, p.grad, st["exp_avg"], st["exp_avg_sq"], self.lr_tensor, st["step"], grad_norm, max_norm,
                         beta1, beta2, group["eps"], grad_scale=grad_scale)
        return grad_norm

    def zero_grad(self):
        if self.arena is not None:
            self.arena.zero_grads()
        else:
            self.optimizer.zero_grad()

    # ---- checkpoint format: the reference's (one entry per parameter, float rate) ----------------------------
    def state_dict(self):
        if self.arena is None:
            return self.optimizer.state_dict()
        group = self.optimizer.param_groups[0]
        flat_p = group["params"][0]
        st = self.optimizer.state.get(flat_p, {})
        state = {}
        if len(st):
            step = st["step"].detach().to("cpu", torch.float32).reshape(())
            for i, p in enumerate(self._params):
                off, n = self.arena.offset[id(p)], p.numel()
                state[i] = {"step": step.clone(),
                            "exp_avg": st["exp_avg"][off:off + n].detach().view(p.shape).clone(),
                            "exp_avg_sq": st["exp_avg_sq"][off:off + n].detach().view(p.shape).clone()}
        # the hyper-parameters a plain ``optim.Adam(model.parameters(), ...)`` saves (Optim.py:11-16)
        g = {k: v for k, v in group.items() if k != "params"}
        g.update(lr=float(self.lr), fused=None, capturable=False, foreach=None, params=list(range(len(self._params))))
        out = {"state": state, "param_groups": [g]}
        if self._guard is not None or self._avg_opts is not None:
            # the one key beyond the reference's format; absent when nothing is enabled
            extra = {"skipped": 0.0 if self._guard is None else float(self._guard[1])}
            if self._avg_opts is not None:
                extra.update(decay=self._avg_opts[0], warmup=self._avg_opts[1],
                             avg=[self.arena.avg_view(p).detach().clone() for p in self._params],
                             extra=[a.detach().clone() for _, a in self._avg_extra])
            out["averaging"] = extra
        return out

    def load_state_dict(self, optimizer_state_dict):
        self._state_loads += 1
        if self.arena is None:
            return self.optimizer.load_state_dict(optimizer_state_dict)
        groups = optimizer_state_dict["param_groups"]
        n_saved = sum(len(g["params"]) for g in groups)
        if n_saved == 1 and len(self._params) != 1:
            # round-1 format of this class: one flat tensor over the same arena layout
            self.optimizer.load_state_dict(optimizer_state_dict)
            lr = self.optimizer.param_groups[0]["lr"]
            self.lr = float(lr)
        elif n_saved == len(self._params) and len(groups) == 1:
            p, st = self._flat_state()
            saved = optimizer_state_dict["state"]
            keys = groups[0]["params"]
            step = None
            with torch.no_grad():
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
                for key, q in zip(keys, self._params):
                    ent = saved.get(key)
                    if not ent:
                        continue
                    off, n = self.arena.offset[id(q)], q.numel()
                    if ent["exp_avg"].numel() != n:
                        raise ValueError("ScheduledOptim.load_state_dict: state %r does not match parameter shape %s"
                                         % (key, tuple(q.shape)))
                    st["exp_avg"][off:off + n].copy_(ent["exp_avg"].reshape(-1))
                    st["exp_avg_sq"][off:off + n].copy_(ent["exp_avg_sq"].reshape(-1))
                    step = float(ent["step"]) if step is None else max(step, float(ent["step"]))
                st["step"].fill_(0.0 if step is None else step)
            g = self.optimizer.param_groups[0]
            for k in ("betas", "eps", "weight_decay", "amsgrad", "maximize"):
                if k in groups[0]:
                    g[k] = groups[0][k]
            self.lr = float(groups[0]["lr"])
        else:
            raise ValueError("ScheduledOptim.load_state_dict: checkpoint holds %d parameter states in %d groups; "
                             "this model has %d parameters" % (n_saved, len(groups), len(self._params)))
        # torch's load_state_dict rebuilds param_groups from the saved dict: re-attach the device-resident rate,
        # or every later update would keep the checkpoint's last learning rate (the Noam schedule frozen on resume)
        self.lr_tensor.fill_(self.lr)
        for g in self.optimizer.param_groups:
            g["lr"] = self.lr_tensor
        self._load_averaging(optimizer_state_dict.get("averaging"))

    def _load_averaging(self, extra):
        """The "averaging" key of a checkpoint into whatever is enabled HERE (decay / warmup stay as enabled); a checkpoint
        without the key - or without averages - re-seeds the average from the parameters."""
        extra = extra or {}
        if self._guard is not None:
            self._guard.zero_()
            self._guard[1].fill_(float(extra.get("skipped", 0.0)))
        if self._avg_opts is None:
            return
        saved = extra.get("avg")
        with torch.no_grad():
            if saved is None:
                self.arena.avg.copy_(self.arena.flat)
            else:
                if len(saved) != len(self._params) or any(a.numel() != p.numel() for a, p in zip(saved, self._params)):
                    raise ValueError("ScheduledOptim.load_state_dict: the checkpoint's averaged tensors do not match the model")
                for a, p in zip(saved, self._params):
                    self.arena.avg_view(p).copy_(a.reshape(p.shape))
            more = extra.get("extra") or []
            for i, (t, a) in enumerate(self._avg_extra):
                a.copy_(more[i] if len(more) == len(self._avg_extra) else t)

    def update_learning_rate(self, global_step):
        self.lr = learn_rate(self.d_model, self.n_warmup_steps, global_step)
        if self.arena is not None:
            self.lr_tensor.fill_(self.lr)
            return
        for group in self.optimizer.param_groups:
            group['lr'] = self.lr
