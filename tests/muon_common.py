"""Shared by the Muon tests (not a conftest): a float64 restatement of the Newton-Schulz iteration and of the optimizer rules
of reference tools/muon_optimizer.py, the reference's own bf16 arithmetic written out with torch on the CPU, the judge built
from the two, and the matrix generators."""
import math

import torch

COEFFS = (3.4445, -4.7750, 2.0315)
EXACT_SHAPES = [(33, 75), (40, 96), (96, 40), (130, 1030), (7, 150), (64, 64)]
ACCURACY_SHAPES = EXACT_SHAPES + [(200, 264), (300, 136)]
EXACT_SEED = 131        # test_muon_host checks that every intermediate of the exact test is an integer <= 256 at this seed


def ns_stages_f64(x, coeffs=COEFFS, normalize=True):
    """One Newton-Schulz step in float64 with every intermediate: -> dict(A, AA, B, BX, out), all in the wide orientation."""
    a, b, c = coeffs
    X = x.double()
    if normalize:
        X = X / (X.norm() + 1e-7)
    A = X @ X.T
    AA = A @ A
    B = b * A + c * AA
    BX = B @ X
    return {'A': A, 'AA': AA, 'B': B, 'BX': BX, 'out': a * X + BX}


def ns_f64(x, steps=5, coeffs=COEFFS, normalize=True):
    """NS(x) in float64: transpose if rows > cols, X /= |X|_F + 1e-7, `steps` times A = X X^T, B = b A + c A A,
    X = a X + B X, transpose back."""
    X = x.double()
    tr = X.shape[0] > X.shape[1]
    if tr:
        X = X.T
    if normalize:
        X = X / (X.norm() + 1e-7)
    for _ in range(steps):
        X = ns_stages_f64(X, coeffs, normalize=False)['out']
    return X.T if tr else X


def ns_reference_bf16(x, steps=5, coeffs=COEFFS):
    """The reference's arithmetic (zeropower_via_newtonschulz5 without its compiler): bf16 tensors through torch on the CPU."""
    a, b, c = coeffs
    X = x.to(torch.bfloat16)
    tr = X.size(-2) > X.size(-1)
    if tr:
        X = X.mT
    X = X / (X.norm(dim=(-2, -1), keepdim=True) + 1e-7)
    for _ in range(steps):
        A = X @ X.mT
        B = b * A + c * A @ A
        X = a * X + B @ X
    return X.mT if tr else X


def fro_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())


def judge(u_kernel, x_bf16, steps=5):
    """-> (e_k, e_r): relative Frobenius error against float64 of the kernel's result and of the reference's own bf16
    arithmetic, both from the same bf16-rounded input."""
    want = ns_f64(x_bf16, steps)
    return fro_err(u_kernel, want), fro_err(ns_reference_bf16(x_bf16, steps), want)


def sparse_sign_matrix(shape, gen):
    """Entries in {-1, 0, 1}, 3-4 non-zeros per row, spread evenly over the columns (three rounds, and a fourth for a random
    half of the rows, each dealing the columns out in shuffled order): even column counts keep the products of the exact test
    small for a tall matrix too."""
    r, c = shape
    x = torch.zeros(r, c)
    rows = torch.arange(r)
    for rnd in range(4):
        order = torch.cat([torch.randperm(c, generator=gen) for _ in range(-(-r // c))])[:r]
        keep = torch.randint(0, 2, (r,), generator=gen).bool() if rnd == 3 else torch.ones(r, dtype=torch.bool)
        sign = (torch.randint(0, 2, (r,), generator=gen) * 2 - 1).float()
        m = keep & (x[rows, order] == 0)
        x[rows[m], order[m]] = sign[m]
    for i in range(r):                                      # a row whose rounds collided is topped up to three
        while int((x[i] != 0).sum()) < 3:
            j = int(torch.randint(0, c, (1,), generator=gen))
            if x[i, j] == 0:
                x[i, j] = float(int(torch.randint(0, 2, (1,), generator=gen)) * 2 - 1)
    return x


def exact_inputs(seed=EXACT_SEED):
    gen = torch.Generator().manual_seed(seed)
    return [sparse_sign_matrix(s, gen) for s in EXACT_SHAPES]


def exact_expected(x):
    """One step with coeffs (1, 1, 1), no normalisation, in float64 -> (output in x's orientation, largest |intermediate|,
    all intermediates integral)."""
    tr = x.shape[0] > x.shape[1]
    st = ns_stages_f64(x.T if tr else x, (1.0, 1.0, 1.0), normalize=False)
    worst = max(float(v.abs().max()) for v in st.values())
    integral = all(bool((v == v.round()).all()) for v in st.values())
    out = st['out']
    return (out.T if tr else out), worst, integral


def accuracy_inputs(seed):
    """Well-conditioned inputs: randn, and randn + 3, alternating over ACCURACY_SHAPES."""
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen) + (3.0 if k % 2 else 0.0) for k, s in enumerate(ACCURACY_SHAPES)]


def muon_ratio(shape):
    return 0.2 * math.sqrt(max(shape[0], shape[1]))


class MuonRestated:
    """The optimizer rules in the arithmetic of the tensors it is given (fp32 on the CPU in the tests).  Muon parameters: only the momentum buffer and v are
    restated (the orthogonalised update is judged separately); backup parameters: the reference's own AdamW in full."""

    def __init__(self, lr, wd, momentum=0.95, nesterov=True, betas=(0.9, 0.999), eps=1e-8):
        self.lr, self.wd, self.momentum, self.nesterov, self.betas, self.eps = lr, wd, momentum, nesterov, betas, eps
        self.state = {}

    def muon_v(self, name, g):
        """buf = momentum buf + g; -> v = g + momentum buf (nesterov) or buf, as [size(0), -1]"""
        g = g.reshape(g.shape[0], -1)
        st = self.state.setdefault(name, {'momentum_buffer': torch.zeros_like(g)})
        buf = st['momentum_buffer']
        buf.mul_(self.momentum).add_(g)
        return g.add(buf, alpha=self.momentum) if self.nesterov else buf.clone()

    def muon_update(self, p, u):
        """p (1 - lr wd) - lr ratio u"""
        return p * (1 - self.lr * self.wd) - self.lr * muon_ratio(p.shape) * u.reshape(p.shape).to(p.dtype)

    def adamw_step(self, name, p, g):
        st = self.state.setdefault(name, {'step': 0, 'moment1': torch.zeros_like(g), 'moment2': torch.zeros_like(g)})
        st['step'] += 1
        b1, b2 = self.betas
        st['moment1'].lerp_(g, 1 - b1)
        st['moment2'].lerp_(g.square(), 1 - b2)
        upd = st['moment1'] / (self.eps + st['moment2'].sqrt())
        scale = (1 - b1 ** st['step']) / (1 - b2 ** st['step']) ** 0.5
        p.mul_(1 - self.lr * self.wd)
        p.add_(upd, alpha=-self.lr / scale)
        return p
