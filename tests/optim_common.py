"""Shared by tests/test_optim_host.py and tests/test_gpu_optim.py: the seeded table, torch.optim's single-tensor path on the CPU as
truth (float64) and yardstick (float32), the host entry's results, and the bound every compared tensor must meet:

    d = max|ours - f64|,  d32 = max|torch_f32 - f64|,  d <= 4 d32 + 2^-22 max|f64|

An fp32 restatement with another valid order of operations stays inside it (ratio to d32 1.0 .. 1.5 on tensors of 257 values and more; on
1- and 3-value tensors, where d32 is down to chance, the floor term carries it); AdamW-style decay lands 10^4 .. 10^5 times outside.
Everything is computed once and kept: the references are never changed by a test."""
import numpy as np
import torch

SIZES = (1, 3, 4, 257, 4096, 4099)      # ONE table: below a vector, a vector, odd, one chunk exactly, one chunk and a scalar tail
STEPS = 5
LR = 1e-2
DECAYS = (0.0, 1e-2)
# name -> (kind of surs_amd.native.OPTIM_KINDS, momentum)
CASES = {"SGD": ("SGD", 0.9), "SGD_m0": ("SGD", 0.0), "ADAM": ("ADAM", 0.0), "AMSgrad": ("AMSgrad", 0.0), "RMSprop": ("RMSprop", 0.0)}
BETAS, EPS, ALPHA = (0.9, 0.999), 1e-8, 0.99

_cache = {}


def initial(sizes=SIZES, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.normal(0.0, 1.0, n).astype(np.float32) for n in sizes]


def gradients(step, sizes=SIZES, seed=2):
    """Fresh gradients of step `step` (0-based): normal, a few exact zeros and a few tiny values (sqrt(v) near eps) where there is room."""
    rng = np.random.default_rng(seed * 1000 + step)
    out = []
    for n in sizes:
        g = rng.normal(0.0, 1.0, n).astype(np.float32)
        if n >= 16:
            g[rng.permutation(n)[:4]] = [0.0, -0.0, 1e-9, -3e-7]
        out.append(g)
    return out


def state_names(kind, momentum):
    from surs_amd import native
    return () if (kind == "SGD" and momentum == 0) else native.OPTIM_STATES[kind]


def torch_optimizer(kind, params, lr=LR, wd=0.0, momentum=0.0, betas=BETAS, eps=EPS, **kw):
    """torch.optim as apps/train_SuRS.py:54-72 builds it, on its single-tensor path (foreach=False) unless kw says otherwise."""
    kw.setdefault("foreach", False)
    if kind == "SGD":
        return torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=wd, **kw)
    if kind in ("ADAM", "AMSgrad"):
        return torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, amsgrad=kind == "AMSgrad", **kw)
    return torch.optim.RMSprop(params, lr=lr, momentum=0, weight_decay=wd, **kw)


def run_torch(kind, p0, grads_per_step, dtype, names, **hyper):
    """torch.optim on the CPU in `dtype` over the tensors p0 with the given gradients: per step, ([p], {state name: [tensor]}) as
    numpy arrays of that dtype."""
    params = [torch.nn.Parameter(torch.from_numpy(np.asarray(p)).to(dtype).clone()) for p in p0]
    o = torch_optimizer(kind, params, **hyper)
    out = []
    for gs in grads_per_step:
        for p, g in zip(params, gs):
            p.grad = torch.from_numpy(np.asarray(g)).to(dtype).reshape(p.shape).clone()
        o.step()
        out.append(([p.detach().numpy().copy() for p in params],
                    {n: [o.state[p][n].detach().numpy().copy() for p in params] for n in names}))
    return out


def run_host(kind, p0, grads_per_step, names, lr=LR, wd=0.0, momentum=0.0, betas=BETAS, eps=EPS):
    """surs_optim_step_host over the same table: per step, ([p], {state name: [tensor]}) - copies."""
    from surs_amd import native
    p = [np.array(x, np.float32) for x in p0]
    st = [[np.zeros_like(x) for x in p] for _ in names]
    out = []
    for t, gs in enumerate(grads_per_step):
        h = native.optim_hyper(kind, t + 1, lr, wd, momentum, betas, eps, ALPHA, first_step=t == 0)
        rows = [(p[i], np.ascontiguousarray(gs[i], np.float32)) + tuple(s[i] for s in st) + (None,) * (3 - len(names)) for i in range(len(p))]
        native.optim_step_host(rows, h)
        out.append(([x.copy() for x in p], {n: [x.copy() for x in s] for n, s in zip(names, st)}))
    return out


def table(case, wd):
    """The shared table of one case and weight decay: dict(f64=, f32=, host=) of run_torch / run_host results, computed once."""
    key = (case, wd)
    if key not in _cache:
        kind, momentum = CASES[case]
        names = state_names(kind, momentum)
        p0, gs = initial(), [gradients(s) for s in range(STEPS)]
        hyper = dict(wd=wd, momentum=momentum)
        _cache[key] = dict(kind=kind, momentum=momentum, names=names, p0=p0, grads=gs,
                           f64=run_torch(kind, p0, gs, torch.float64, names, **hyper),
                           f32=run_torch(kind, p0, gs, torch.float32, names, **hyper),
                           host=run_host(kind, p0, gs, names, **hyper))
    return _cache[key]


def excess(ours, f64, f32):
    """(d, allowed, d / d32) of one tensor."""
    f64 = np.asarray(f64, np.float64).reshape(-1)
    d = float(np.max(np.abs(np.asarray(ours, np.float64).reshape(-1) - f64)))
    d32 = float(np.max(np.abs(np.asarray(f32, np.float64).reshape(-1) - f64)))
    allowed = 4.0 * d32 + 2.0 ** -22 * float(np.max(np.abs(f64)))
    return d, allowed, (d / d32 if d32 > 0 else float("inf") if d > 0 else 0.0)


def check_step(ours, f64, f32, what, report=None):
    """Asserts the bound on p and every state tensor of one step's ([p], {name: [tensor]}) triple; prints every figure first and
    returns the largest d / d32 among tensors of 257 values and more."""
    worst = 0.0
    rows = [("p", ours[0], f64[0], f32[0])] + [(n, ours[1][n], f64[1][n], f32[1][n]) for n in f64[1]]
    for name, a, b, c in rows:
        for i, (x, y, z) in enumerate(zip(a, b, c)):
            d, allowed, ratio = excess(x, y, z)
            print("%s %s[%d] n=%d d=%.3e allowed=%.3e d/d32=%.3f" % (what, name, i, np.size(y), d, allowed, ratio))
            assert d <= allowed, (what, name, i, d, allowed)
            if np.size(y) >= 257:
                worst = max(worst, ratio)
    if report is not None:
        report[what] = max(report.get(what, 0.0), worst)
    return worst


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
