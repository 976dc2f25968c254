"""What tests/test_norm_stats_host.py (no GPU) and tests/test_gpu_norm_stats.py (MI355X) share: the off-centre input builder, the
float64 references of BatchNorm / GroupNorm / LayerNorm, and the judge that holds a result against the project's bounds.

Every normalisation kernel of csrc/ takes its variance as E[x^2] - E[x]^2 in fp32 (bn.hip, groupnorm.hip) or in two passes
(tfm.hip).  The first form loses about (mean / std)^2 ulps, so the inputs here are built per SLAB -- a BatchNorm channel, a
GroupNorm (sample, group), a LayerNorm row -- with a prescribed |mean| / std.

Classes (slab i takes CLASSES[i % len(CLASSES)]):
    c0, c2, c8, c32, c128   |mean| / std = 0, 2, 8, 32, 128 (the 'n' twins carry a negative mean)
    dead                    every element exactly 0 (dead_value: another constant, for the host test's fault)
    tiny                    std 1e-3 about 0: var = 1e-6, far below eps = 1e-5

Bounds (fp32 / bf16; the error of a tensor is conftest.rel_err over the class's slabs, of a statistic the largest per-slab error):
    c0, c2, c8, tiny   output 1e-4 / 2e-2, statistics 1e-4 / 1e-4, gradients 4e-4 / 8e-2      (the per-kernel tolerances of
                       tests/test_gpu_kernels.py; bf16 statistics are fp32 arithmetic on bf16 values, hence still 1e-4)
    c32                output 1e-3 / 2e-2, variance and running_var 1e-3, mean and running_mean 1e-4, gradients 4e-3 / 8e-2
                       (the 1e-3 north star; the mean is a plain sum and keeps 1e-4)
    c128               finite, var >= 0, invstd <= 1 / sqrt(eps); the error is recorded, not asserted
    dead               output = beta within 1e-6, dx / dgamma finite, dbeta = sum dz within the gradient tolerance
How the statistics' errors are scaled (a relative error of a quantity that may be 0 needs a scale):
    mean, running_mean   |d| / max(|ref|, sqrt(var_ref + eps))   -- the mean only acts through (x - mean) / std
    variance             var = invstd^-2 - eps, |d| / (var_ref + eps)   -- what invstd = rsqrt(var + eps) can resolve
    running_var          |d| / max(|ref|, eps)
"""
import math

import torch

EPS = 1e-5
CLASSES = (('c0', 0.0, 1), ('c2', 2.0, 1), ('c2n', 2.0, -1), ('c8', 8.0, 1), ('c8n', 8.0, -1), ('c32', 32.0, 1), ('c32n', 32.0, -1),
           ('c128', 128.0, 1), ('c128n', 128.0, -1), ('dead', None, 0), ('tiny', 0.0, 0))
NCLS = len(CLASSES)
TINY_STD = 1e-3
# the bound classes the ledger reports (a class and its negative twin share a row)
GROUPS = ('c0', 'c2', 'c8', 'c32', 'c128', 'dead', 'tiny')


def group_of(i):
    return CLASSES[i % NCLS][0].rstrip('n')


def slab_classes(n):
    """-> the bound class name of each of n slabs"""
    return [group_of(i) for i in range(n)]


def slab_params(n):
    """-> (mean, std) float64 [n] of the slabs before rounding; std cycles 0.5, 1, 2 so an offset is not one magnitude"""
    mean, std = torch.zeros(n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
    for i in range(n):
        name, ratio, sign = CLASSES[i % NCLS]
        s = 2.0 ** ((i // NCLS) % 3 - 1)
        if name == 'dead':
            s = 0.0
        elif name == 'tiny':
            s = TINY_STD
        std[i] = s
        mean[i] = sign * (ratio or 0.0) * s
    return mean, std


def build_slabs(nslab, length, dtype, seed, dead_value=0.0, generator=None):
    """-> (x [nslab][length] rounded to dtype, x64 the same before rounding).  Built in float64: standard normal noise made exactly
    zero-mean / unit-variance per slab (so that a slab of 8 elements still has its class's ratio), scaled and shifted, rounded."""
    g = generator or torch.Generator().manual_seed(seed)
    z = torch.randn(nslab, length, dtype=torch.float64, generator=g)
    if length > 1:
        z = z - z.mean(1, keepdim=True)
        z = z / z.pow(2).mean(1, keepdim=True).sqrt()
    mean, std = slab_params(nslab)
    x64 = mean[:, None] + std[:, None] * z
    for i in range(nslab):
        if CLASSES[i % NCLS][0] == 'dead':
            x64[i] = dead_value
    return x64.to(dtype), x64


def realised(x):
    """-> (mean, biased var) float64 per slab of x [nslab][length]"""
    x = x.double()
    m = x.mean(1)
    return m, (x - m[:, None]).pow(2).mean(1)


def assert_ratios(x, what='', dead_value=0.0):
    """The realised |mean| / std of every slab of x [nslab][length] (any dtype, taken in float64) is within 25 % of its class's target:
    the inputs cannot silently drift back to centred."""
    m, v = realised(x)
    for i in range(x.shape[0]):
        name, ratio, _ = CLASSES[i % NCLS]
        if name == 'dead':
            assert bool((x[i].double() == dead_value).all()), f'{what}: dead slab {i} is not constant'
            continue
        r = abs(float(m[i])) / math.sqrt(float(v[i]))
        if name == 'tiny':
            assert 0.75 * TINY_STD ** 2 <= float(v[i]) <= 1.25 * TINY_STD ** 2, f'{what}: tiny slab {i} has var {float(v[i]):.3e}'
        if ratio == 0.0:
            assert r < 0.25, f'{what}: slab {i} ({name}) realised ratio {r:.3f}, target 0'
        else:
            assert 0.75 * ratio <= r <= 1.25 * ratio, f'{what}: slab {i} ({name}) realised ratio {r:.3f}, target {ratio}'


# ------------------------------------------------------------------------------ float64 references
def bn_ref(x, gamma=None, beta=None, eps=EPS, momentum=0.1, running_mean=None, running_var=None, res=None, gate=None):
    """Training-mode BatchNorm over x [M][C] in float64 (biased variance normalises, the unbiased one goes to running_var).
    gate: 0/1 [M][C] standing for the ReLU decisions of the run it is compared with.  -> dict"""
    x = x.double()
    M = x.shape[0]
    mean = x.mean(0)
    var = (x - mean).pow(2).mean(0)
    invstd = (var + eps).rsqrt()
    out = (x - mean) * invstd
    if gamma is not None:
        out = out * gamma.double()
    if beta is not None:
        out = out + beta.double()
    if res is not None:
        out = out + res.double()
    if gate is not None:
        out = out * gate.double()
    r = {'mean': mean, 'var': var, 'invstd': invstd, 'out': out}
    if running_mean is not None:
        unbiased = var * M / (M - 1) if M > 1 else var
        r['running_mean'] = (1 - momentum) * running_mean.double() + momentum * mean
        r['running_var'] = (1 - momentum) * running_var.double() + momentum * unbiased
    return r


def bn_bwd_ref(x, dz, gamma, mean, invstd, gate=None):
    """BatchNorm backward in float64 from the SAVED statistics: -> dx, dgamma, dbeta, dres (= the gated dz)"""
    x, g = x.double(), dz.double()
    if gate is not None:
        g = g * gate.double()
    mean, invstd = mean.double(), invstd.double()
    xhat = (x - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    M = x.shape[0]
    a = invstd * (gamma.double() if gamma is not None else 1.0)
    dx = a * (g - dbeta / M - xhat * dgamma / M)
    return {'dx': dx, 'dgamma': dgamma, 'dbeta': dbeta, 'dres': g}


# ------------------------------------------------------------------------------ bounds and the judge
def bounds(group, dtype):
    """-> dict(out, mean, var, grad) of the class, None where nothing but finiteness is asserted"""
    f32 = dtype == torch.float32
    if group == 'c128':
        return None
    if group == 'c32':
        return {'out': 1e-3 if f32 else 2e-2, 'mean': 1e-4, 'var': 1e-3, 'grad': 4e-3 if f32 else 8e-2}
    return {'out': 1e-4 if f32 else 2e-2, 'mean': 1e-4, 'var': 1e-4, 'grad': 4e-4 if f32 else 8e-2}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))          # conftest.rel_err


class Ledger:
    """Collects (route, class, quantity, error, bound) and every violated assertion; check() fails with all of them at once."""

    def __init__(self):
        self.rows, self.bad = [], []

    def add(self, route, group, qty, err, bound):
        self.rows.append((route, group, qty, float(err), bound))
        if not math.isfinite(err) or (bound is not None and not err <= bound):
            self.bad.append(f'{route} [{group}] {qty}: {err:.3e} > {bound}')

    def require(self, ok, msg):
        if not ok:
            self.bad.append(msg)

    def worst(self):
        """-> {(route, class, quantity): largest error}"""
        w = {}
        for route, group, qty, err, _ in self.rows:
            k = (route, group, qty)
            w[k] = max(w.get(k, 0.0), err)
        return w

    def report(self):
        return '\n'.join(f'NORMSTAT {r} {g} {q} {e:.3e} {b}' for r, g, q, e, b in self.rows)

    def check(self):
        assert not self.bad, '\n'.join(self.bad)


def _sel(classes, group):
    return [i for i, c in enumerate(classes) if c == group]


def judge_stats(led, route, dtype, classes, ref, got, eps=EPS):
    """Saved mean / invstd and the running statistics (1-d over slabs) against float64."""
    std = (ref['var'] + eps).sqrt()
    for group in GROUPS:
        idx = _sel(classes, group)
        if not idx:
            continue
        b = bounds(group, dtype)
        gm, gi = got['mean'].double().cpu()[idx], got['invstd'].double().cpu()[idx]
        rm, rv, sd = ref['mean'][idx], ref['var'][idx], std[idx]
        led.require(bool(torch.isfinite(gm).all() and torch.isfinite(gi).all()), f'{route} [{group}] mean / invstd not finite')
        led.require(bool((gi > 0).all() and (gi <= (1.0 + 1e-6) / math.sqrt(eps)).all()), f'{route} [{group}] invstd outside (0, 1/sqrt(eps)]')
        gv = gi.pow(-2) - eps
        led.require(bool((gv >= -1e-6 * (rv + eps)).all()), f'{route} [{group}] negative variance')
        led.add(route, group, 'mean', ((gm - rm).abs() / torch.maximum(rm.abs(), sd)).max(), b and b['mean'])
        led.add(route, group, 'var', ((gv - rv).abs() / (rv + eps)).max(), b and b['var'])
        if 'running_mean' in ref:
            a, r = got['running_mean'].double().cpu()[idx], ref['running_mean'][idx]
            led.add(route, group, 'running_mean', ((a - r).abs() / torch.maximum(r.abs(), sd)).max(), b and b['mean'])
            a, r = got['running_var'].double().cpu()[idx], ref['running_var'][idx]
            led.add(route, group, 'running_var', ((a - r).abs() / r.abs().clamp_min(eps)).max(), b and b['var'])


def judge_out(led, route, dtype, classes, ref_out, got_out, beta=None, slab_dim=1, qty='out'):
    """A normalised output: slabs along slab_dim of the (2-d) tensors.  The dead class must equal beta within 1e-6 (beta: per slab)."""
    for group in GROUPS:
        idx = _sel(classes, group)
        if not idx:
            continue
        r, a = ref_out.double().cpu().index_select(slab_dim, torch.tensor(idx)), got_out.double().cpu().index_select(slab_dim, torch.tensor(idx))
        led.require(bool(torch.isfinite(a).all()), f'{route} [{group}] {qty} not finite')
        if group == 'dead' and beta is not None:
            bt = beta.double().cpu()[idx]
            d = (a - (bt[None, :] if slab_dim == 1 else bt[:, None])).abs().max()
            led.add(route, group, qty + '-beta', d, 1e-6 if dtype == torch.float32 else None)
        b = bounds(group, dtype)
        led.add(route, group, qty, _rel(a, r), b and b['out'])


def judge_grads(led, route, dtype, classes, ref, got, slab_dim=1):
    """dx / dres [.. slabs ..] and dgamma / dbeta [slabs] of a backward route fed its own forward's saved statistics."""
    for group in GROUPS:
        idx = _sel(classes, group)
        if not idx:
            continue
        b = bounds(group, dtype)
        it = torch.tensor(idx)
        for k in ('dx', 'dres'):
            if got.get(k) is None:
                continue
            a, r = got[k].double().cpu().index_select(slab_dim, it), ref[k].index_select(slab_dim, it)
            led.require(bool(torch.isfinite(a).all()), f'{route} [{group}] {k} not finite')
            led.add(route, group, k, _rel(a, r), None if group == 'dead' and k == 'dx' else b and b['grad'])
        for k in ('dgamma', 'dbeta'):
            if got.get(k) is None:
                continue
            a, r = got[k].double().cpu()[idx], ref[k][idx]
            led.require(bool(torch.isfinite(a).all()), f'{route} [{group}] {k} not finite')
            led.add(route, group, k, _rel(a, r), None if group == 'dead' and k == 'dgamma' else b and b['grad'])
