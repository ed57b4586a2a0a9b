"""optimizerG of the reference's training loop (/root/reference/apps/train_SuRS.py:54-72, :146-148) on SuRSNet's device masters.

    optimizerG = optim.from_options(netG, opt)          # --optimizer SGD | ADAM | RMSprop | AMSgrad
    ...
    optimizerG.zero_grad()
    res_hr, error, res_lr, grads = netG.forward_backward(...)
    optimizerG.step(grads)                              # one launch over every tensor, then netG.commit()
    optimizerG.step(grads, guard=True)                  # the same unless a gradient is non-finite: then nothing is touched

Optimizer steps the plain fp32 masters behind mlp_parameters(), sr_parameters() and hg_parameters() - about 330 tensors, 18.4 M values
at the released options - by ONE launch of surs_optim_step over a device table (native.optim_step; the arithmetic is torch.optim's
single-tensor path, csrc/surs_optim_update.h), and then calls net.commit(), so that the next forward runs on the stepped values: a
step without its commit would train on stale packed weights.  Hyper-parameters are kernel arguments read from param_groups at every
step: train_util.adjust_learning_rate works on it unchanged and uploads nothing.  state_dict() / load_state_dict() use torch.optim's
layout, so a run moves between torch.optim on the three parameter dictionaries and this optimiser in either direction.

The step count t of the bias corrections is the OPTIMISER's, one per step() call that had a gradient.  torch counts per tensor: a key
that was skipped in some steps (no gradient) is bias-corrected with a larger t here than in torch; load_state_dict refuses a state
whose tensors carry unequal steps.  Not here: Nesterov, dampening, centred RMSprop or RMSprop with momentum, maximize, AdamW's
decoupled decay (ValueError where param_groups asks for one), per-group hyper-parameters (one group).
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import native, weights

KINDS = tuple(native.OPTIM_KINDS)


def _torch_group(kind, lr, momentum, betas, eps, weight_decay):
    """param_groups[0] of the torch.optim optimiser this one stands in for (without 'params'): torch's own keys and defaults, whatever
    its version, so that state_dict() loads there key for key."""
    dummy = [torch.nn.Parameter(torch.zeros(1))]
    if kind == "SGD":
        o = torch.optim.SGD(dummy, lr=lr, momentum=momentum, weight_decay=weight_decay)
    elif kind in ("ADAM", "AMSgrad"):
        o = torch.optim.Adam(dummy, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=kind == "AMSgrad")
    elif kind == "RMSprop":
        o = torch.optim.RMSprop(dummy, lr=lr, momentum=0, eps=eps, weight_decay=weight_decay)
    else:
        raise ValueError("optimizer %r: the kinds are %s (apps/train_SuRS.py:54-72)" % (kind, ", ".join(KINDS)))
    return {k: v for k, v in o.param_groups[0].items() if k != "params"}


def _check_group(kind, g):
    """ValueError for what param_groups can ask for and the kernel does not do."""
    bad = [k for k in ("maximize", "nesterov", "centered", "decoupled_weight_decay") if g.get(k)]
    if g.get("dampening", 0) != 0:
        bad.append("dampening")
    if kind == "RMSprop" and g.get("momentum", 0) != 0:
        bad.append("momentum (RMSprop)")
    if kind in ("ADAM", "AMSgrad") and bool(g.get("amsgrad")) != (kind == "AMSgrad"):
        bad.append("amsgrad (the kind is %s)" % kind)
    if bad:
        raise ValueError("Optimizer(%s): not supported: %s" % (kind, ", ".join(bad)))
    for k in ("lr", "weight_decay", "eps", "momentum", "alpha"):
        if k in g and not float(g[k]) >= 0.0:
            raise ValueError("Optimizer(%s): %s = %r" % (kind, k, g[k]))


class Optimizer:
    """Optimizer(net, kind="ADAM", which=None, lr=1e-3, momentum=0.9, betas=(0.9, 0.999), eps=1e-8, weight_decay=0).

    kind: SGD (momentum; dampening 0, no Nesterov) | ADAM | AMSgrad | RMSprop (alpha 0.99, momentum 0, not centred); weight decay is an L2
    term of the gradient for all four.  momentum is SGD's.  which: a subset of SuRSNet.SETS, default all three; the net is asked for
    those parameter sets and their masters are stepped ("hg" under --norm batch: NotImplementedError, as commit raises).  State: one
    zero-initialised fp32 device slab per state kind, sliced per key at 16-byte-aligned offsets."""

    def __init__(self, net, kind="ADAM", which=None, lr=1e-3, momentum=0.9, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        group = _torch_group(kind, lr, momentum, betas, eps, weight_decay)
        _check_group(kind, group)
        which = net.SETS if which is None else (which,) if isinstance(which, str) else tuple(which)
        for w in which:
            if w not in net.SETS:
                raise ValueError("Optimizer: unknown parameter set %r; the sets are %s" % (w, net.SETS))
        if "hg" in which and weights.check_norm(getattr(net.opt, "norm", "group")) == "batch":
            raise NotImplementedError("Optimizer(which 'hg'): --norm group only (a BatchNorm encoder has no backward and no commit)")
        self.net, self.kind, self.which = net, kind, tuple(w for w in net.SETS if w in which)
        self.param_groups = [group]
        self._params = OrderedDict()       # state-dict key -> torch.nn.Parameter (over the master), the sets' key orders concatenated
        for w in self.which:
            self._params.update(getattr(net, w + "_parameters")())
        self._owners = {w: net._masters()[w] for w in self.which}
        self._masters = OrderedDict((k, t) for w in self.which for k, t in self._owners[w].items())
        assert list(self._masters) == list(self._params)
        self._keys = list(self._masters)
        self.device = next(iter(self._masters.values())).device
        self._offset, total = {}, 0
        for k, t in self._masters.items():
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("Optimizer: master %s is not a contiguous float32 tensor" % k)
            self._offset[k] = total
            total += (t.numel() + 3) // 4 * 4
        self._total = total
        self._slabs = {}                   # torch.optim's state name -> the slab, made when a step first needs it
        self._t = 0                        # steps taken (the t of the next step's bias corrections is _t + 1)
        self._seen = set()                 # keys that have been stepped (or loaded): the ones state_dict() lists
        self._sig = self._table = self._n_items = None
        self._keep = None
        self.skipped = 0                   # steps step(guard=True) refused because a gradient was not finite
        self.last_skipped_key = None       # the first key (in parameter order) whose gradient was not finite in the last refused step
        self.last_skipped_rank = None      # step(ranks=..., guard=True): the lowest rank whose gathered slab was not finite
        self._guard_sig = self._guard_table = self._guard_ws = self._guard_total = None

    # ------------------------------------------------------------------ state
    def _state_names(self, group=None):
        g = self.param_groups[0] if group is None else group
        if self.kind == "SGD" and g.get("momentum", 0) == 0:
            return ()
        return native.OPTIM_STATES[self.kind]

    def _slab(self, name):
        if name not in self._slabs:
            self._slabs[name] = torch.zeros(self._total, dtype=torch.float32, device=self.device)
        return self._slabs[name]

    def _slice(self, name, k):
        t = self._masters[k]
        return self._slab(name)[self._offset[k]:self._offset[k] + t.numel()]

    def zero_grad(self, set_to_none=True):
        """Sets the Parameters' .grad to None (the masters' gradients handed to step() as a mapping are the caller's)."""
        for p in self._params.values():
            p.grad = None

    # ------------------------------------------------------------------ the step
    def _hyper(self):
        g = self.param_groups[0]
        _check_group(self.kind, g)
        return native.optim_hyper(self.kind, self._t + 1, g["lr"], g.get("weight_decay", 0.0), g.get("momentum", 0.0),
                                  g.get("betas", (0.9, 0.999)), g.get("eps", 1e-8), g.get("alpha", 0.99),
                                  first_step=self.kind == "SGD" and not self._seen)

    def _gradients(self, grads):
        """[(key, contiguous float32 device tensor of the master's element count)] of the keys that have a gradient, in the parameter
        order; ValueError for a wrong size, dtype or device - before anything is written."""
        out = []
        for k, p in self._params.items():
            g = p.grad if grads is None else grads.get(k)
            if g is None:
                continue
            if not torch.is_tensor(g) or g.dtype != torch.float32 or g.device != self.device or g.numel() != p.numel():
                raise ValueError("Optimizer.step: gradient of %s: %s against a float32 parameter of %d elements on %s" % (
                    k, "%s %s on %s" % (tuple(g.shape), g.dtype, g.device) if torch.is_tensor(g) else type(g).__name__, p.numel(),
                    self.device))
            out.append((k, g.detach() if g.is_contiguous() else g.detach().contiguous()))
        return out

    def _nonfinite(self, todo):
        """The index in `todo` of the first gradient that holds a NaN or an infinity, or -1: native.tensors_nonfinite over a device
        table of the gradients (rebuilt only when a pointer differs from the previous guarded step's), then the one read of its 4-byte
        result - a synchronisation with the current stream."""
        sig = tuple((k, g.data_ptr(), g.numel()) for k, g in todo)
        if sig != self._guard_sig:
            items, total = native.tensor_refs([(g.data_ptr(), g.numel()) for _, g in todo])
            nbytes = C.sizeof(items)
            host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            C.memmove(host.data_ptr(), C.addressof(items), nbytes)
            self._guard_table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._guard_table.copy_(host, non_blocking=True)
            self._guard_ws = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
            self._guard_sig, self._guard_total = sig, total
        return int(native.tensors_nonfinite(self._guard_table, len(todo), self._guard_total, workspace=self._guard_ws).item())

    def _step_ranks(self, grads, ranks, commit, guard, hyper):
        """step(ranks=(gathered, R)): see step()."""
        gathered, R = ranks
        R = int(R)
        if (not torch.is_tensor(gathered) or gathered.dtype != torch.float32 or gathered.device != self.device
                or tuple(gathered.shape) != (R, self._total) or not gathered.is_contiguous() or gathered.data_ptr() % 16):
            raise ValueError("Optimizer.step(ranks=): a contiguous 16-byte-aligned float32 [%d, %d] tensor on %s is expected, got %s" % (
                R, self._total, self.device, "%s %s" % (tuple(gathered.shape), gathered.dtype) if torch.is_tensor(gathered)
                else type(gathered).__name__))
        keys = self._keys if grads is None else [k for k in self._keys if k in grads and grads[k] is not None]
        if not keys:
            return None
        if guard:
            sig = ("ranks", gathered.data_ptr(), R)
            if sig != self._guard_sig:
                items, total = native.tensor_refs([(gathered.data_ptr() + 4 * r * self._total, self._total) for r in range(R)])
                self._guard_table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.device)
                self._guard_ws = torch.empty(max(total, 1), dtype=torch.int32, device=self.device)
                self._guard_sig, self._guard_total = sig, total
            hit = int(native.tensors_nonfinite(self._guard_table, R, self._guard_total, workspace=self._guard_ws).item())
            if hit >= 0:
                self.skipped += 1
                self.last_skipped_rank, self.last_skipped_key = hit, None
                return False
        names = self._state_names()
        sig = ("ranks", names, gathered.data_ptr(), R, tuple(keys) if grads is not None else None)
        if sig != self._sig:
            rows = []
            for k in keys:
                s = [self._slice(n, k).data_ptr() for n in names] + [None] * (3 - len(names))
                rows.append((self._masters[k].data_ptr(), gathered.data_ptr() + 4 * self._offset[k], s[0], s[1], s[2],
                             self._masters[k].numel()))
            items = native.optim_items(rows)
            native.optim_check(items, len(rows), hyper)
            nbytes = C.sizeof(items)
            host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            C.memmove(host.data_ptr(), C.addressof(items), nbytes)
            self._table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._table.copy_(host, non_blocking=True)
            self._sig, self._n_items = sig, len(rows)
        self._keep = [gathered]
        native.optim_step_ranks(self._table, self._n_items, hyper, R, self._total, C.c_float(1.0 / R).value)
        self._t += 1
        self._seen.update(keys)
        if commit:
            self.net.commit(self.which)
        return True if guard else None

    def step(self, grads=None, commit=True, guard=False, ranks=None):
        """One step of every key that has a gradient, in one launch on the current stream, then net.commit(which) unless commit=False.
        grads: a mapping state-dict key -> device tensor - the OrderedDicts classifier_grads() / forward_backward(),
        super_res_backward() and filter_lr_backward() return, or a merge of them; any shape with the right element count; keys of other
        sets are ignored - or None: the .grad of the Parameters (autograd.point_loss and the other Functions leave them).  A key without
        a gradient is skipped, as torch skips grad is None (see the module docstring for its bias correction).  The device table is
        rebuilt only when a pointer differs from the previous step's and uploaded from pinned memory without synchronisation.
        guard=True: the gradients about to be applied are first searched for a NaN or an infinity (surs_tensors_nonfinite) and the
        4-byte answer is read - ONE synchronisation per step, which guard=False does not have.  The fp32-grade forward runs on two f16
        operand parts: an activation beyond the f16 range gives non-finite features and gradients, and one such step would poison every
        master.  On a hit nothing is launched: parameters, optimiser state and the step count stay bit for bit as they were, `skipped`
        counts the step, `last_skipped_key` names the first offending key, and the call returns False; otherwise it returns True after
        the step guard=False would have taken (the same bits).  Returns None with guard=False, as before.
        ranks=(gathered, R): the data-parallel step (dist.TrainGroup makes the buffer).  gathered is a contiguous float32 [R, total]
        device tensor, row r the gradient slab of rank r with key k at this optimiser's own offset _offset[k] (zeros where a rank had
        no gradient); the table's g points into row 0 and ONE launch of surs_optim_step_ranks applies ((g_0 + g_1) + ... + g_{R-1}) *
        fp32(1 / R) - sums in rank order, never written.  grads then only NAMES the keys to step (a mapping; None: every key) - the
        keys any rank had a gradient for, which in a data-parallel run is every rank's own set.  guard=True searches the R rows
        (surs_tensors_nonfinite over R refs): on a hit nothing is launched, `skipped` counts it and `last_skipped_rank` is the lowest
        offending rank - the same answer on every rank, from the same bytes.  R = 1 gives the plain step's bits."""
        for w in self.which:
            if self.net._masters().get(w) is not self._owners[w]:
                raise RuntimeError("Optimizer.step: the net's %r masters were replaced (load_state_dict() / to()): make a new Optimizer "
                                   "and load_state_dict() this one's state_dict()" % w)
        hyper = self._hyper()
        if ranks is not None:
            return self._step_ranks(grads, ranks, commit, guard, hyper)
        todo = self._gradients(grads)
        if not todo:
            return None
        if guard:
            hit = self._nonfinite(todo)
            if hit >= 0:
                self.skipped += 1
                self.last_skipped_key = todo[hit][0]
                return False
        names = self._state_names()
        sig = (names,) + tuple((k, g.data_ptr()) for k, g in todo)
        if sig != self._sig:
            rows = []
            for k, g in todo:
                s = [self._slice(n, k).data_ptr() for n in names] + [None] * (3 - len(names))
                rows.append((self._masters[k].data_ptr(), g.data_ptr(), s[0], s[1], s[2], self._masters[k].numel()))
            items = native.optim_items(rows)
            native.optim_check(items, len(rows), hyper)
            nbytes = C.sizeof(items)
            host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
            C.memmove(host.data_ptr(), C.addressof(items), nbytes)
            self._table = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._table.copy_(host, non_blocking=True)
            self._sig, self._n_items = sig, len(rows)
        self._keep = [g for _, g in todo]
        native.optim_step(self._table, self._n_items, hyper)
        self._t += 1
        self._seen.update(k for k, _ in todo)
        if commit:
            self.net.commit(self.which)
        return True if guard else None

    # ------------------------------------------------------------------ torch.optim's state_dict
    def state_dict(self):
        """torch.optim's layout: {'state': {index: {...}}, 'param_groups': [{..., 'params': [0 .. N-1]}]}, index in the concatenation of
        the sets' key orders; per index 'step' (ADAM, AMSgrad, RMSprop: a float32 scalar) and exp_avg, exp_avg_sq, max_exp_avg_sq |
        momentum_buffer | square_avg as clones of the parameter's shape.  Only keys that have been stepped are listed, as in torch."""
        names = self._state_names()
        state = {}
        for i, k in enumerate(self._keys):
            if k not in self._seen or (self.kind == "SGD" and not names):
                continue
            s = {} if self.kind == "SGD" else {"step": torch.tensor(float(self._t))}
            for n in names:
                s[n] = self._slice(n, k).clone().reshape(self._params[k].shape)
            state[i] = s
        group = dict(self.param_groups[0])
        group["params"] = list(range(len(self._keys)))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        """Takes a torch.optim (or this class's) state_dict of the same kind over the same parameters in the same order.  ValueError for
        another layout, for unsupported hyper-parameters, and for per-tensor steps that are not all equal (the step count here is the
        optimiser's)."""
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._keys):
            raise ValueError("Optimizer.load_state_dict: one group of %d parameters expected, got %s" % (
                len(self._keys), [len(g["params"]) for g in groups]))
        group = {k: v for k, v in groups[0].items() if k != "params"}
        _check_group(self.kind, group)
        names = self._state_names(group)
        index = {p: i for i, p in enumerate(groups[0]["params"])}
        steps, loaded = set(), []
        for pid, s in sd["state"].items():
            if pid not in index:
                raise ValueError("Optimizer.load_state_dict: state of parameter %r, which is in no group" % (pid,))
            k = self._keys[index[pid]]
            if "step" in s:
                steps.add(float(s["step"]))
            vals = {}
            for n in names:
                v = s.get(n)
                if v is None:
                    continue
                if not torch.is_tensor(v) or v.numel() != self._masters[k].numel():
                    raise ValueError("Optimizer.load_state_dict: %s of %s does not have the parameter's %d elements" % (
                        n, k, self._masters[k].numel()))
                vals[n] = v
            if vals and len(vals) != len(names):
                raise ValueError("Optimizer.load_state_dict: %s has %s of %s" % (k, sorted(vals), list(names)))
            if vals or "step" in s:
                loaded.append((k, vals))
        if len(steps) > 1:
            raise ValueError("Optimizer.load_state_dict: unequal per-tensor steps %s: the step count here is the optimiser's" % sorted(steps)[:4])
        # nothing was written so far
        self.param_groups = [group]
        for slab in self._slabs.values():
            slab.zero_()
        self._seen = set()
        for k, vals in loaded:
            for n, v in vals.items():
                self._slice(n, k).copy_(v.detach().reshape(-1).to(self.device, torch.float32))
            self._seen.add(k)
        self._t = int(steps.pop()) if steps else (1 if loaded else 0)
        self._sig = None
        return self


def from_options(net, opt, which=None):
    """The optimiser apps/train_SuRS.py:54-72 builds from --optimizer SGD | ADAM | RMSprop | AMSgrad: --learning_rate and --weight_decay
    for all, --momentum for SGD, --beta1 --beta2 --epsilon for ADAM and AMSgrad; RMSprop with momentum 0 and torch's default alpha and
    eps.  Any other name: ValueError (the reference would fail at its first use of optimizerG)."""
    name = opt.optimizer
    if name not in KINDS:
        raise ValueError("--optimizer %r: the choices are %s (apps/train_SuRS.py:54-72)" % (name, ", ".join(KINDS)))
    kw = dict(lr=opt.learning_rate, weight_decay=opt.weight_decay)
    if name == "SGD":
        kw["momentum"] = opt.momentum
    elif name in ("ADAM", "AMSgrad"):
        kw.update(betas=(opt.beta1, opt.beta2), eps=opt.epsilon)
    return Optimizer(net, name, which, **kw)
