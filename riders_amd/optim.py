"""Flat-arena fused Adam: every parameter (and its gradient and both moments) lives in ONE contiguous fp32
buffer, so an optimizer step is a single rd_adam_step launch and data-parallel gradient exchange can all-reduce
arena slices in place (no bucket copies).

Reference: torch.optim.Adam(parameters, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0) at
RCNet/rcnet_main.py:233-238 and train_zju.py:205-211; same update arithmetic, same `param_groups[0]['lr']`
handle for the learning-rate schedule (rcnet_main.py:246-252, train_zju.py:231-237), and the same
`state_dict()` layout ({'state': {index: {step, exp_avg, exp_avg_sq}}, 'param_groups': [...]}) so the
`radarnet_optimizer_state_dict` entry of a checkpoint (RCNet/rcnet_model.py:224-257) is exchangeable with the
reference's torch.optim.Adam in both directions.

torch skips a parameter whose `.grad` is None (no moment update, no step increment).  The same holds here: a slot
that no backward kernel wrote since `zero_grad()` is left out of the step.  A slot that has NEVER been written
holds zero gradient and zero moments, for which the update is exactly zero, so the common case -- the reference's
never-used `projection` convolutions (utils/net_utils.py:300-307) -- still runs as one launch over the arena.

Parameter groups.  The reference's three training loops pass a list of group dictionaries
(`[{'params': parameters, 'weight_decay': w_weight_decay}]`, RCNet/rcnet_main.py:233-238); that form, per-group `lr` / `betas` / `eps` /
`weight_decay` and torch 2.10's `decoupled_weight_decay` (what AdamW is) are accepted.  The arena is laid out group after group, so a group is
one contiguous range and rd_adam_step_groups updates all of them in one launch (the group table travels in the kernel arguments).  One group
with coupled decay -- every optimizer built the flat way -- launches rd_adam_step exactly as before.

Gradient clipping by global norm.  `FlatAdam.set_grad_clip(max_norm, norm_type)` (persistent) and `clip_grad_norm_` below (torch's signature, for
the unchanged caller) form torch.nn.utils.clip_grad_norm_'s norm and coefficient on the device from one read of the arena and apply the
coefficient inside the Adam launch (rd_grad_norm_partial, rd_grad_clip_finalize, rd_adam_step_groups_clipped): the gradients are not rewritten
and nothing waits for the host.  Off -- the default -- step() launches exactly what it launched before.
"""
import ctypes

import torch
from torch.nn.utils.clip_grad import clip_grad_norm_ as _torch_clip_grad_norm_      # torch's own, bound once: the fallback of clip_grad_norm_ below,
#                                                                                   whatever torch.nn.utils.clip_grad_norm_ is aliased to later

from . import _lib, engine

_HYPER = ('lr', 'betas', 'eps', 'weight_decay', 'decoupled_weight_decay')
_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                       decoupled_weight_decay=False)


class DynamicLossScale(object):
    """torch.amp.GradScaler's loss scale for the fp16 mode, kept entirely on the device: 32 bytes (rd_loss_scale_state) that the backward's
    seed, the finite check, the Adam launches and the update kernel read and write in stream order, so no step synchronises with the host and
    a captured step (rcnet_main.GraphedStep) reads the scale of the replay, not of the capture.

    Hand it to `loss_scale=` of train_step / compute_gradients / staged_gradients / GraphedStep / GraphedTrainStep (or assign it to
    `FlatAdam.loss_scale` and seed the backward with `scale_tensor`).  FlatAdam.step() then runs rd_grad_finite_check on the arena, every Adam
    launch through rd_adam_step_groups_scaled (nothing is written while the flag is up; the gradient is divided by the live scale), and
    rd_loss_scale_update, which is torch._amp_update_scale_: backoff on a non-finite gradient, growth after `growth_interval` finite steps in
    a row.  One departure: a backoff that would take the scale below the smallest normal fp32 is not taken.

    Several ranks: the finite check runs in step(), i.e. on the REDUCED arena after the all-reducer's join, and an inf or NaN of one rank
    survives the sum, so every rank raises the same flag, skips the same step and keeps the same scale without exchanging anything more.

    One scaler serves one optimizer.  get_scale() / skipped_steps() / stats() synchronise; state_dict() / load_state_dict() have GradScaler's
    layout, so a checkpoint moves between the two."""

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, device=None):
        if not growth_factor > 1.0:
            raise ValueError("The growth factor must be > 1.0.")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError("The backoff factor must be in (0, 1).")
        if int(growth_interval) < 1:
            raise ValueError("The growth interval must be >= 1.")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._state = torch.zeros(ctypes.sizeof(_lib.LossScaleState) // 4, dtype=torch.int32, device=device)
        self.scale_tensor = self._state[0:1].view(torch.float32)      # the `scale` word itself: what the backward is seeded with
        self._flag = self._state[2:4]                                  # (found_inf, skipped): the flag pair of rd_grad_finite_check
        self._carry = 0      # skips counted before the last load_state_dict (which zeroes the device counters)
        self._init(init_scale, 0)

    def _init(self, scale, tracker):
        engine._chk(engine.L().rd_loss_scale_init(engine._p(self._state), ctypes.c_float(scale), int(tracker), engine._stream(self._state)),
                    "rd_loss_scale_init")

    def update(self):
        """the step's last launch: found_inf -> backoff and one more skipped step, otherwise the growth tracker; clears found_inf"""
        engine._chk(engine.L().rd_loss_scale_update(engine._p(self._state), ctypes.c_float(self.growth_factor), ctypes.c_float(self.backoff_factor),
                                                    self.growth_interval, engine._stream(self._state)), "rd_loss_scale_update")

    def stats(self):
        """-> dict of the state's fields (synchronises)"""
        raw = self._state.detach().cpu()
        f = raw[0:2].view(torch.float32)
        names = [n for n, _ in _lib.LossScaleState._fields_]
        out = dict(zip(names, [float(f[0]), float(f[1])] + [int(v) for v in raw[2:]]))
        out.pop("reserved")
        return out

    def get_scale(self):
        return float(self.scale_tensor.item())

    def skipped_steps(self):
        return self._carry + int(self._state[3].item())

    def state_dict(self):
        s = self.stats()
        return dict(scale=s["scale"], growth_factor=self.growth_factor, backoff_factor=self.backoff_factor, growth_interval=self.growth_interval,
                    _growth_tracker=s["growth_tracker"])

    def load_state_dict(self, sd):
        if len(sd) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance of GradScaler.")
        self._carry = self.skipped_steps()
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self._init(float(sd["scale"]), int(sd["_growth_tracker"]))


class FlatAdam(object):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False):
        params = [p for p in params]
        if len(params) == 0:
            raise ValueError("optimizer got an empty parameter list")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay)
        if not isinstance(params[0], dict):      # the flat form: one group
            params = [dict(params=params)]
        if len(params) > _lib.RD_ADAM_MAX_GROUPS:
            raise ValueError("FlatAdam supports at most %d parameter groups (got %d)" % (_lib.RD_ADAM_MAX_GROUPS, len(params)))
        self.param_groups, seen = [], set()
        for src in params:
            if not isinstance(src, dict):
                raise TypeError("param group must be a dict")
            ps = src['params']
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            if len(ps) == 0:
                raise ValueError("optimizer got an empty parameter list")
            if any(id(p) in seen for p in ps) or len(set(id(p) for p in ps)) != len(ps):
                raise ValueError("some parameters appear in more than one parameter group")
            seen.update(id(p) for p in ps)
            if bool(src.get('amsgrad', False)) or bool(src.get('maximize', False)):
                raise ValueError("amsgrad / maximize Adam are not supported (the reference uses neither)")
            g = {k: v for k, v in src.items() if k != 'params'}
            for k, v in defaults.items():
                g.setdefault(k, v)
            g['params'] = ps
            self.param_groups.append(g)
        params = [p for g in self.param_groups for p in g['params']]      # torch's state indices: the groups in order
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FlatAdam needs fp32 parameters on one device")
        self.params = params
        self._group_slots, k = [], 0      # [first, end) parameter indices of every group
        for g in self.param_groups:
            self._group_slots.append((k, k + len(g['params'])))
            k += len(g['params'])
        # 16-byte aligned slots so the vectorised kernel and RCCL see aligned slices
        self.offsets, n = [], 0
        for p in params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.numel = n
        self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self._gviews = {}
        self._index = {}
        self._owner = frozenset(id(p) for p in params)      # engine.refresh_packed: whose cached operands this optimizer's step re-packs
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(params, self.offsets)):
                view = self.flat_param[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
                self._gviews[id(p)] = self.flat_grad[o:o + p.numel()].view(p.shape)
                self._index[id(p)] = i
        self.steps = [0] * len(params)          # per-parameter step count (torch keeps `step` per parameter)
        self._touched = [False] * len(params)   # slot written by a backward kernel since zero_grad()
        self._ever = [False] * len(params)      # slot has received a gradient at least once (torch: has optimizer state)
        self.grad_scale = 1.0      # 1 / world size, set by parallel.GradientAllReducer (the all-reduce sums)
        self._loss_scale = 1.0     # loss scale of the fp16 mode: gradients arrive multiplied by it and are divided here (float or DynamicLossScale)
        self._overflow = None      # device int32[2] (flag, skipped steps) of the guarded fp16 step, allocated on first use
        self._skips_reconciled = 0  # skipped steps already taken back out of the host step counters (reconcile_skipped)
        self._dyn_reconciled = 0    # ... of those the attached DynamicLossScale counted
        self._clip = None           # (max_norm, norm kind) of set_grad_clip; None: no clipping, step() launches what it always launched
        self._clip_armed = False    # clip_grad_norm_ formed the coefficient already: the next step() uses it and runs no norm pass
        self._clipping = False      # inside step(): this step's Adam launches go through the clipped entry
        self._clip_state = None     # device int32[8]: rd_grad_clip_state, allocated with the partial rows on first use
        self._clip_partial = None
        self._reducer_attached = False
        engine.set_param_grad_allocator(self._grad_view)

    @property
    def loss_scale(self):
        """A float: the static loss scale (1.0: none).  A DynamicLossScale: the scale lives on the device and follows torch.amp.GradScaler; step()
        then launches rd_grad_finite_check, rd_adam_step_groups_scaled and rd_loss_scale_update and never synchronises.  The host step counters
        still advance before the device decides to skip, but the scaled launch subtracts the skips not yet reconciled, so every applied update has
        the bias correction of the number of updates applied.  A parameter that was not written during a skipped step keeps the approximation
        reconcile_skipped() already has: the skip is taken off its count too."""
        return self._loss_scale

    @loss_scale.setter
    def loss_scale(self, value):
        if isinstance(value, DynamicLossScale):
            if value is not self._loss_scale:      # attaching synchronises once: skips counted so far belong to whoever counted them
                self.reconcile_skipped()
                self._dyn_reconciled = value.skipped_steps()
            self._loss_scale = value
            return
        if isinstance(self._loss_scale, DynamicLossScale):
            self.reconcile_skipped()
        self._loss_scale = float(value)

    def _scaler(self):
        return self._loss_scale if isinstance(self._loss_scale, DynamicLossScale) else None

    # kept for callers that read the global step (all parameters that train share it)
    @property
    def step_count(self):
        return max(self.steps) if self.steps else 0

    def _grad_view(self, p):
        i = self._index.get(id(p))
        if i is None:
            return None
        self._touched[i] = True
        return self._gviews[id(p)]

    def mark_touched(self, indices):
        """Declare these slots written since zero_grad().  A hipGraph REPLAY of the backward writes the arena without going through the
        gradient allocator (which is what sets the flags in an eager backward): rcnet_main.GraphedStep records the slots its capture pass
        touched and re-marks them before every step(), so `optimizer.zero_grad()` between replays -- the reference loop's habit -- cannot
        turn the optimizer step into a silent no-op."""
        for i in indices:
            self._touched[i] = True

    def touched_indices(self):
        return [i for i, t in enumerate(self._touched) if t]

    def skipped_steps(self):
        """fp16 mode: optimizer steps dropped because a scaled gradient was not finite (synchronises).  The host-side step counters (bias
        correction) are advanced before the device decides to skip, so after k skipped steps they run k ahead of the moments until
        `reconcile_skipped()` (called by state_dict()) takes them back -- torch's GradScaler likewise does not advance `step` on a skip."""
        return self._static_skips() + self._dyn_skips()

    def _static_skips(self):
        return 0 if self._overflow is None else int(self._overflow[1].item())

    def _dyn_skips(self):
        """skips counted by the attached DynamicLossScale since it was attached (plus those reconciled under an earlier one)"""
        sc = self._scaler()
        return self._dyn_reconciled if sc is None else sc.skipped_steps()

    def reconcile_skipped(self, warn_after=8):
        """Subtract the device-side skip count from the host step counters (synchronises; with a static loss scale a persistent overflow
        skips EVERY step: more than `warn_after` skips since the last call raise a warning naming the remedy.  Under a DynamicLossScale skips
        are routine -- a few while the scale backs off, then one per growth interval -- and nothing is warned).  -> skips taken back."""
        ks, kd = self._static_skips(), self._dyn_skips()
        new_static = ks - self._skips_reconciled
        new = new_static + kd - self._dyn_reconciled
        if new > 0:
            self.steps = [max(0, s - new) if e else s for s, e in zip(self.steps, self._ever)]
            self._skips_reconciled, self._dyn_reconciled = ks, kd
            if new_static > warn_after and self._scaler() is None:
                import warnings
                warnings.warn("FlatAdam: %d optimizer steps were skipped because the scaled fp16 gradient was not finite; lower loss_scale "
                              "(now %g)" % (new_static, self.loss_scale))
        return max(new, 0)

    def slot_range(self, params):
        """-> sorted, merged [(start, end)] arena element ranges covering `params` (used to bucket the gradient all-reduce)."""
        spans = sorted((self.offsets[self._index[id(p)]], self.offsets[self._index[id(p)]] + (p.numel() + 3) // 4 * 4) for p in params)
        out = []
        for s, e in spans:
            if out and s <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], e))
            else:
                out.append((s, e))
        return out

    def zero_grad(self, set_to_none=True):
        """Gradients are (re)written by the backward kernels into arena views; a slot nobody writes before step() is skipped by it."""
        for p in self.params:
            p.grad = None
        self._touched = [False] * len(self.params)
        self._clip_armed = False      # a coefficient formed by clip_grad_norm_ belongs to the gradients it was formed from

    def _gather_foreign_grads(self):
        # gradients produced outside the arena (user-assigned tensors): copy in with a HIP kernel
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None:
                continue
            view = self._gviews[id(p)]
            self._touched[i] = True
            if g.data_ptr() != view.data_ptr():
                gc = g if g.is_contiguous() else g.contiguous()
                engine._chk(engine.L().rd_cast(engine._p(gc), engine._p(view), gc.numel(), engine.rd_of(gc), 0, 1.0,
                                               engine._stream(gc)), "rd_cast")

    def add_param_group(self, param_group):
        raise NotImplementedError("FlatAdam: the arena is sized at construction; pass every parameter group to the constructor")

    # ------------------------------------------------------------------ global-norm gradient clipping
    def set_grad_clip(self, max_norm, norm_type=2.0):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type) as part of every step(), on the device: one norm pass over the slots
        written since zero_grad() (rd_grad_norm_partial), one single-block launch that forms torch's coefficient min(1, max_norm / (norm + 1e-6))
        (rd_grad_clip_finalize), and every Adam launch of the step through rd_adam_step_groups_clipped, which multiplies the gradient by it.
        Nothing synchronises and the gradients are not rewritten, so train_step, GraphedStep and GraphedTrainStep use it unchanged.  None turns
        clipping off (the default): step() then launches exactly what it launched before.  norm_type is 2 or inf.

        The norm is taken of the gradient Adam sees: multiplied by grad_scale (1 / world under a GradientAllReducer, on the reduced arena) and
        divided by the loss scale -- what `scaler.unscale_(opt); clip_grad_norm_(...)` gives.  Under a DynamicLossScale (or a static scale) the
        norm pass raises the finite flag from the same read and rd_grad_finite_check is not launched.  A non-finite norm: without a loss scale the
        NaN coefficient reaches the parameters, as torch's error_if_nonfinite=False lets it; with one the step is skipped as it always is."""
        if max_norm is None:
            self._clip = None
            return
        kind = _norm_kind(norm_type)
        if kind is None:
            raise ValueError("FlatAdam.set_grad_clip: norm_type must be 2 or inf (got %r)" % (norm_type,))
        max_norm = float(max_norm)
        if not 0.0 < max_norm < float("inf"):
            raise ValueError("FlatAdam.set_grad_clip: max_norm must be a finite positive number (got %r)" % (max_norm,))
        self._clip = (max_norm, kind)
        self._clip_buffers()

    def _clip_buffers(self):
        if self._clip_state is None:
            dev = self.flat_param.device
            self._clip_state = torch.zeros(ctypes.sizeof(_lib.GradClipState) // 4, dtype=torch.int32, device=dev)
            self._clip_partial = torch.zeros(_lib.RD_GRAD_NORM_ROWS, dtype=torch.float64, device=dev)
            engine._chk(engine.L().rd_grad_clip_init(engine._p(self._clip_state), engine._stream(self.flat_param)), "rd_grad_clip_init")
        return self._clip_state

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the total norm of the last clipped step (a view of the device state: reading it enqueues, it does not wait)"""
        return self._clip_buffers()[0:1].view(torch.float32)[0]

    def clip_stats(self):
        """-> dict(total_norm, coef, passes, clipped, nonfinite) of the clipping state (synchronises)"""
        raw = self._clip_buffers().detach().cpu()
        f = raw[0:2].view(torch.float32)
        return dict(total_norm=float(f[0]), coef=float(f[1]), passes=int(raw[2]), clipped=int(raw[3]), nonfinite=int(raw[4]))

    def _touched_runs(self):
        """[(start, end)] arena element ranges of consecutive slots written since zero_grad()"""
        runs, n, i = [], len(self.params), 0
        while i < n:
            if not self._touched[i]:
                i += 1
                continue
            j = i
            while j + 1 < n and self._touched[j + 1]:
                j += 1
            runs.append((self.offsets[i], self.offsets[j + 1] if j + 1 < n else self.numel))
            i = j + 1
        return runs

    def _clip_pass(self, max_norm, kind, flag):
        """the norm of the written slots (stale slots do not count) and the coefficient, into the device state"""
        self._clip_buffers()
        st = engine._stream(self.flat_param)
        sc = self._scaler()
        pre = self.grad_scale if sc is not None else self.grad_scale / self.loss_scale
        state = engine._p(sc._state) if sc is not None else None
        for k, (a, b) in enumerate(self._touched_runs()):
            rc = engine._tb("optimizer", 4 * (b - a), lambda: engine.L().rd_grad_norm_partial(
                engine._p(self.flat_grad[a:b]), b - a, ctypes.c_float(pre), state, kind, engine._p(self._clip_partial), _lib.RD_GRAD_NORM_ROWS,
                1 if k else 0, flag, st), "grad_norm")
            engine._chk(rc, "rd_grad_norm_partial")
        engine._chk(engine.L().rd_grad_clip_finalize(engine._p(self._clip_partial), _lib.RD_GRAD_NORM_ROWS, ctypes.c_float(max_norm), kind,
                                                     engine._p(self._clip_state), st), "rd_grad_clip_finalize")

    def _clip_now(self, max_norm, kind):
        """riders_amd.clip_grad_norm_'s fast path: the norm pass and the finalize at once; the next step() multiplies by the coefficient"""
        self._gather_foreign_grads()
        if not any(self._touched):
            return None
        self._clip_pass(max_norm, kind, None)
        self._clip_armed = True
        return self.grad_norm

    def _launch(self, start, end, step):
        g = self.param_groups[0]
        if self._scaler() is not None or self._clipping:      # one coupled group under a dynamic scale or clipped: a table of one
            self._launch_groups(start, end, [(g, end, step)])
            return
        sl = slice(start, end)
        args = (engine._p(self.flat_param[sl]), engine._p(self.flat_grad[sl]), engine._p(self.exp_avg[sl]), engine._p(self.exp_avg_sq[sl]), end - start,
                ctypes.c_float(g['lr']), ctypes.c_float(g['betas'][0]), ctypes.c_float(g['betas'][1]), ctypes.c_float(g['eps']),
                ctypes.c_float(g['weight_decay']), step, ctypes.c_float(self.grad_scale / self.loss_scale))
        st = engine._stream(self.flat_param)
        if self._overflow is not None:
            rc = engine._tb("optimizer", 28 * (end - start), lambda: engine.L().rd_adam_step_guarded(*args, engine._p(self._overflow), st), "adam")
        else:
            rc = engine._tb("optimizer", 28 * (end - start), lambda: engine.L().rd_adam_step(*args, st), "adam")
        engine._chk(rc, "rd_adam_step")

    def _group_end(self, gi):
        """arena element where group gi ends"""
        j = self._group_slots[gi][1]
        return self.offsets[j] if j < len(self.params) else self.numel

    def _launch_groups(self, start, end, entries):
        """One rd_adam_step_groups launch over arena elements [start, end).  entries: [(param group, end element, step or None = inactive)]."""
        t = _lib.AdamGroups()
        t.count = len(entries)
        live = 0
        prev = start
        for k, (g, e, step) in enumerate(entries):
            t.end[k] = e - start
            t.flags[k] = (_lib.ADAM_DECOUPLED if g['decoupled_weight_decay'] else 0) | (_lib.ADAM_INACTIVE if step is None else 0)
            t.step[k] = 1 if step is None else step
            t.lr[k], t.beta1[k], t.beta2[k], t.eps[k], t.weight_decay[k] = g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay']
            live += 0 if step is None else e - prev
            prev = e
        sl = slice(start, end)
        ptrs = (engine._p(self.flat_param[sl]), engine._p(self.flat_grad[sl]), engine._p(self.exp_avg[sl]), engine._p(self.exp_avg_sq[sl]))
        st = engine._stream(self.flat_param)
        sc = self._scaler()
        if self._clipping:
            skip = engine._p(self._overflow) if (sc is None and self._overflow is not None) else None
            gscale = self.grad_scale if sc is not None else self.grad_scale / self.loss_scale
            rc = engine._tb("optimizer", 28 * live, lambda: engine.L().rd_adam_step_groups_clipped(
                *ptrs, end - start, t, ctypes.c_float(gscale), skip, engine._p(sc._state) if sc is not None else None,
                self._dyn_reconciled - sc._carry if sc is not None else 0, engine._p(self._clip_state), st), "adam")
            engine._chk(rc, "rd_adam_step_groups_clipped")
            return
        if sc is not None:
            # the host counters run ahead of the moments by the skips not yet reconciled: the kernel takes state->skipped - base off every step
            base = self._dyn_reconciled - sc._carry
            rc = engine._tb("optimizer", 28 * live, lambda: engine.L().rd_adam_step_groups_scaled(*ptrs, end - start, t, ctypes.c_float(self.grad_scale),
                                                                                                  engine._p(sc._state), base, st), "adam")
            engine._chk(rc, "rd_adam_step_groups_scaled")
            return
        skip = engine._p(self._overflow) if self._overflow is not None else None
        rc = engine._tb("optimizer", 28 * live, lambda: engine.L().rd_adam_step_groups(*ptrs, end - start, t, ctypes.c_float(self.grad_scale / self.loss_scale),
                                                                                       skip, st), "adam")
        engine._chk(rc, "rd_adam_step_groups")

    def _step_groups(self):
        """Several groups, or decoupled decay: ONE launch when every group is inactive (no slot written since zero_grad()) or uniform (its written
        slots share a step count, and every slot not written this step has never been written while the group decays nothing: zero gradient and
        zero moments, the update is exactly zero); otherwise one one-group launch per run of consecutive written slots that share a step count,
        runs split at group boundaries."""
        n = len(self.params)
        entries, one = [], True
        for gi, (g, (a, b)) in enumerate(zip(self.param_groups, self._group_slots)):
            live = set(self.steps[i] for i in range(a, b) if self._touched[i])
            if not live:
                entries.append((g, self._group_end(gi), None))
                continue
            idle_ok = g['weight_decay'] == 0 and not any(self._ever[i] for i in range(a, b) if not self._touched[i])
            if len(live) != 1 or not (idle_ok or all(self._touched[a:b])):
                one = False
                break
            entries.append((g, self._group_end(gi), live.pop()))
        if one:
            self._launch_groups(0, self.numel, entries)
            return
        for gi, (g, (a, b)) in enumerate(zip(self.param_groups, self._group_slots)):
            i = a
            while i < b:
                if not self._touched[i]:
                    i += 1
                    continue
                j = i
                while j + 1 < b and self._touched[j + 1] and self.steps[j + 1] == self.steps[i]:
                    j += 1
                end = self.offsets[j + 1] if j + 1 < n else self.numel
                self._launch_groups(self.offsets[i], end, [(g, end, self.steps[i])])
                i = j + 1

    def step(self):
        self._gather_foreign_grads()
        n = len(self.params)
        for i in range(n):
            if self._touched[i]:
                self.steps[i] += 1
                self._ever[i] = True
        live = [s for s, t in zip(self.steps, self._touched) if t]
        if not live:
            self._clip_armed = False
            return
        try:
            self._clipping = self._clip is not None or self._clip_armed
            self._step_launches(n, live)
        finally:
            self._clipping = self._clip_armed = False

    def _step_launches(self, n, live):
        scaler = self._scaler()
        guarded = scaler is None and self.loss_scale != 1.0     # fp16 mode: a non-finite scaled gradient skips the whole update (device-side, no host sync)
        if scaler is not None:      # the dynamic scale: the flag pair is the scaler's own (found_inf, skipped)
            if scaler._state.device != self.flat_param.device:
                raise ValueError("FlatAdam: the DynamicLossScale lives on %s, the arena on %s" % (scaler._state.device, self.flat_param.device))
        if guarded and self._overflow is None:
            self._overflow = torch.zeros(2, dtype=torch.int32, device=self.flat_param.device)
        flag = scaler._flag if scaler is not None else self._overflow if guarded else None
        if self._clip is not None and not self._clip_armed:      # the norm pass raises the flag from the same read: no finite check of its own
            self._clip_pass(self._clip[0], self._clip[1], engine._p(flag) if flag is not None else None)
        elif flag is not None:
            engine._chk(engine.L().rd_grad_finite_check(engine._p(self.flat_grad), self.numel, engine._p(flag),
                                                        engine._stream(self.flat_param)), "rd_grad_finite_check")
        if len(self.param_groups) > 1 or self.param_groups[0]['decoupled_weight_decay']:
            self._step_groups()
        else:
            # one launch when every slot is either written this step (all at the same step count) or has never been written (zero gradient and
            # zero moments: the update is exactly zero); otherwise one launch per run of consecutive written slots that share a step count
            uniform = len(set(live)) == 1 and all(t or not e for t, e in zip(self._touched, self._ever)) and self.param_groups[0]['weight_decay'] == 0
            if uniform:
                self._launch(0, self.numel, live[0])
            else:
                i = 0
                while i < n:
                    if not self._touched[i]:
                        i += 1
                        continue
                    j = i
                    while j + 1 < n and self._touched[j + 1] and self.steps[j + 1] == self.steps[i]:
                        j += 1
                    end = self.offsets[j + 1] if j + 1 < n else self.numel
                    self._launch(self.offsets[i], end, self.steps[i])
                    i = j + 1
        if guarded:
            engine._chk(engine.L().rd_adam_skip_count(engine._p(self._overflow), engine._stream(self.flat_param)), "rd_adam_skip_count")
        if scaler is not None:
            scaler.update()
        engine.refresh_packed(self._owner)   # one launch re-packs every cached MFMA operand of the rewritten parameters (this optimizer's only)

    # ------------------------------------------------------------------ checkpoint interchange with torch.optim.Adam
    def state_dict(self):
        """torch.optim.Adam's layout: per-parameter `step` / `exp_avg` / `exp_avg_sq` (copies sliced out of the arena) for every parameter
        that has received a gradient, and every param group with its hyperparameters and its parameter indices."""
        state = {}
        engine.check_roi_overflow()   # (the host waits here anyway) a checkpoint must not be written from NaN-poisoned moments
        self.reconcile_skipped()      # `step` = updates actually applied (fp16 mode: not the skipped ones)
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if not self._ever[i]:
                continue
            state[i] = dict(step=torch.tensor(float(self.steps[i])),
                            exp_avg=self.exp_avg[o:o + p.numel()].view(p.shape).clone(),
                            exp_avg_sq=self.exp_avg_sq[o:o + p.numel()].view(p.shape).clone())
        groups = []
        for src, (a, b) in zip(self.param_groups, self._group_slots):
            g = {k: v for k, v in src.items() if k != 'params'}
            for k, v in _GROUP_DEFAULTS.items():
                g.setdefault(k, v)
            g['params'] = list(range(a, b))      # consecutive indices running through the groups, as torch writes them
            groups.append(g)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        """Accepts a torch.optim.Adam state_dict (the reference's `radarnet_optimizer_state_dict`), this class's own output, and the
        flat {'step','exp_avg','exp_avg_sq'} form written by round-1 checkpoints."""
        if 'state' not in sd:      # round-1 private layout
            self.steps = [int(sd['step'])] * len(self.params)
            self._ever = [True] * len(self.params)
            self.exp_avg.copy_(sd['exp_avg'])
            self.exp_avg_sq.copy_(sd['exp_avg_sq'])
            self.param_groups[0].update({k: v for k, v in sd['param_groups'][0].items() if k != 'params'})
            self._skips_reconciled, self._dyn_reconciled = self._static_skips(), self._dyn_skips()
            return
        groups = sd['param_groups']
        if len(groups) != len(self.param_groups):
            raise ValueError("loaded state dict has a different number of parameter groups (%d, the optimizer has %d)" % (len(groups), len(self.param_groups)))
        if any(len(g['params']) != b - a for g, (a, b) in zip(groups, self._group_slots)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        order = [i for g in groups for i in g['params']]
        if any(bool(g.get('amsgrad', False)) or bool(g.get('maximize', False)) for g in groups):
            raise ValueError("amsgrad / maximize Adam states are not supported (the reference uses neither)")
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            self.steps = [0] * len(self.params)
            self._ever = [False] * len(self.params)
            for pos, key in enumerate(order):
                st = sd['state'].get(key)
                if st is None:
                    continue
                p, o = self.params[pos], self.offsets[pos]
                if tuple(st['exp_avg'].shape) != tuple(p.shape):
                    raise ValueError("optimizer state %r has shape %s, parameter %d has %s" % (key, tuple(st['exp_avg'].shape), pos, tuple(p.shape)))
                self.exp_avg[o:o + p.numel()].view(p.shape).copy_(st['exp_avg'])
                self.exp_avg_sq[o:o + p.numel()].view(p.shape).copy_(st['exp_avg_sq'])
                self.steps[pos] = int(float(st['step']))
                self._ever[pos] = True
        # the loaded `step` values are updates actually applied: skips counted on the device so far belong to the state that was replaced
        self._skips_reconciled, self._dyn_reconciled = self._static_skips(), self._dyn_skips()
        for mine, theirs in zip(self.param_groups, groups):
            hp = {k: v for k, v in theirs.items() if k in _HYPER}
            if 'betas' in hp:
                hp['betas'] = tuple(hp['betas'])
            mine.update(hp)


def _norm_kind(norm_type):
    """-> the C ABI's norm kind for 2 and inf, None for anything else"""
    try:
        v = float(norm_type)
    except (TypeError, ValueError):
        return None
    return _lib.GRAD_NORM_L2 if v == 2.0 else _lib.GRAD_NORM_INF if v == float("inf") else None


def _flat_owner(params):
    """the one live FlatAdam whose parameters with gradients are exactly `params` with gradients, or None"""
    for ref in reversed(engine._grad_allocs):
        fn = ref()
        opt = getattr(fn, "__self__", None)
        if not isinstance(opt, FlatAdam):
            continue
        has = lambda p: p.grad is not None or opt._touched[opt._index[id(p)]]      # noqa: E731
        if any(id(p) not in opt._index for p in params if p.grad is not None):
            continue
        given = set(id(p) for p in params if id(p) in opt._index and has(p))
        if given and given == set(id(p) for p in opt.params if has(p)):
            return opt
    return None


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """torch.nn.utils.clip_grad_norm_ for the unchanged caller (`loss.backward(); clip_grad_norm_(model.parameters(), 1.0); optimizer.step()`).

    When `parameters` are exactly the parameters with gradients of one live FlatAdam, error_if_nonfinite is false, norm_type is 2 or inf and no
    GradientAllReducer is attached to that optimizer, nothing is rewritten: the norm pass and the finalize run at once on the arena (gradients
    assigned outside it are gathered first; a loss scale attached to the optimizer is divided out, as after `scaler.unscale_`), the optimizer's
    next step() multiplies the gradient by the coefficient inside its Adam launch, and the device tensor FlatAdam.grad_norm is returned without
    a synchronisation.  The coefficient serves that one step.  Every other call is torch.nn.utils.clip_grad_norm_ itself.  With a
    GradientAllReducer the norm belongs to the REDUCED arena, which exists only inside step(): use FlatAdam.set_grad_clip there."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    kind = _norm_kind(norm_type)
    try:
        mn = float(max_norm)
    except (TypeError, ValueError):
        mn = -1.0
    if kind is not None and not error_if_nonfinite and 0.0 < mn < float("inf"):
        opt = _flat_owner(parameters)
        if opt is not None and not opt._reducer_attached:
            out = opt._clip_now(mn, kind)
            if out is not None:
                return out
    return _torch_clip_grad_norm_(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite, foreach=foreach)


class FlatAdamW(FlatAdam):
    """torch.optim.AdamW: FlatAdam with decoupled weight decay and AdamW's default weight_decay = 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super(FlatAdamW, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True)
