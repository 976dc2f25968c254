"""Muon on the GPU (csrc/muon.hip, ops.muon_newton_schulz, engine.Muon, build_optimizer) against the float64 restatement of
tests/muon_common.py.

The parity scheme: a bf16 Newton-Schulz iteration has no tight bound against exact arithmetic (the reference's own bf16 result is
2-4e-2 from float64), so the kernels are judged against the reference's own error: with e_k / e_r the relative Frobenius distance
to float64 of the kernel's result / of the reference's arithmetic (bf16 tensors through torch on the CPU) from the same
bf16-rounded input, e_k <= e_r must hold.  A schedule with bf16 operands, fp32 accumulation and one rounding per stored matrix
sits at about half of e_r; a structural mistake (coefficient, tile, transpose) is of order 1.  Structure itself is pinned bit for
bit by integer operands."""
import copy
import logging

import pytest
import torch
import torch.nn as nn

import muon_common as M
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-6


def _ns(tensors, **kw):
    from simpleaicv_pytorch_training_examples_amd import ops
    out = ops.muon_newton_schulz([t.cuda() for t in tensors], **kw)
    torch.cuda.synchronize()
    assert all(o.dtype == torch.bfloat16 and o.shape == t.shape for o, t in zip(out, tensors))
    return [o.cpu() for o in out]


def test_one_step_on_integer_operands_is_bit_exact():
    """Entries in {-1, 0, 1}, coefficients (1, 1, 1), no normalisation, one step: every intermediate is an integer of magnitude
    <= 256 (asserted in float64 first), which bf16 holds exactly and fp32 accumulates exactly in any order, so the kernels'
    output must EQUAL the float64 one.  Ragged shapes, a tall one, m = 7, several tiles per side, all in one grouped call:
    lost edge tiles, the mirrored tiles of A and B, the transposed LDS read and the problem-table lookup show up exactly."""
    xs = M.exact_inputs()
    want = []
    for x in xs:
        out, worst, integral = M.exact_expected(x)
        assert integral and worst <= 256, (tuple(x.shape), worst)
        want.append(out)
    got = _ns(xs, steps=1, coeffs=(1.0, 1.0, 1.0), normalize=False)
    for x, g, w in zip(xs, got, want):
        bad = (g.double() != w).nonzero()
        assert bad.numel() == 0, (tuple(x.shape), bad.shape[0], bad[:4].tolist())


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_five_steps_are_no_further_from_float64_than_the_reference_arithmetic(seed):
    xs = [x.to(torch.bfloat16) for x in M.accuracy_inputs(seed)]
    got = _ns([x.float() for x in xs])
    ratios = []
    for x, g in zip(xs, got):
        e_k, e_r = M.judge(g, x)
        ratios.append(e_k / e_r)
        print(f'[muon ns] seed {seed} {tuple(x.shape)}: e_k {e_k:.3e} e_r {e_r:.3e} ratio {e_k / e_r:.2f}')
        assert 1e-2 < e_r < 6e-2, (tuple(x.shape), e_r)            # the regime the bound was derived in
        assert e_k <= e_r, (tuple(x.shape), e_k, e_r)
    print(f'[muon ns] seed {seed}: e_k / e_r between {min(ratios):.2f} and {max(ratios):.2f}')


def test_zero_matrix_gives_zeros_and_leaves_its_neighbours_alone():
    xs = M.accuracy_inputs(5)[:4]
    zero = torch.zeros(50, 70)
    with_zero = _ns(xs[:2] + [zero] + xs[2:])
    without = _ns(xs)
    assert bool((with_zero[2] == 0).all()) and not bool(torch.isnan(with_zero[2].float()).any())
    for a, b in zip(with_zero[:2] + with_zero[3:], without):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ engine.Muon
class _Net(nn.Module):
    """Parameters of every layout the arenas hold (the net of tests/test_gpu_optim.py, restated): a channels_last conv weight,
    2-d weights of several optimizer blocks, 1-d parameters, a layer that receives no gradient in some steps."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.conv = nn.Conv2d(8, 24, 3, bias=False)
        self.conv.weight.data = self.conv.weight.data.contiguous(memory_format=torch.channels_last)
        self.bn = nn.BatchNorm2d(24)
        self.fc1 = nn.Linear(300, 1500)
        self.fc2 = nn.Linear(1500, 7)
        self.unused = nn.Linear(33, 5)
        with torch.no_grad():
            self.bn.weight.uniform_(0.5, 1.5)
            self.bn.bias.uniform_(-0.2, 0.2)


def _build(nesterov=True, lr=0.02, wd=0.01):
    from simpleaicv_pytorch_training_examples_amd import engine
    net = _Net().cuda()
    muon = [p for p in net.parameters() if p.ndim >= 2]
    rest = [p for p in net.parameters() if p.ndim < 2]
    opt = engine.Muon(net, muon, rest, lr=lr, wd=wd, momentum=0.95, nesterov=nesterov, ns_steps=5)
    assert net.conv.weight.is_contiguous(memory_format=torch.channels_last) and not net.conv.weight.is_contiguous()
    return net, opt


def _write_grads(net, arena, seed, skip=(), poison=False):
    g = torch.Generator().manual_seed(seed)
    arena.zero_grad()
    grads = {}
    for n, p in net.named_parameters():
        grad = torch.randn(p.shape, generator=g)
        if any(n.startswith(s) for s in skip):
            continue
        if poison and n == 'fc1.weight':
            grad.view(-1)[17] = float('inf')
        p.grad.copy_(grad.cuda())
        arena.arrived[arena.names.index(n)] = True
        grads[n] = grad
    return grads


def _snapshot(opt):
    return [t.clone() for t in (opt.arena.flat_param, opt.state1, opt.state2, opt.step_blk)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('nesterov', [True, False], ids=['nesterov', 'plain'])
def test_muon_steps_match_the_restated_rules(nesterov):
    net, opt = _build(nesterov)
    arena = opt.arena
    ref = M.MuonRestated(lr=0.02, wd=0.01, momentum=0.95, nesterov=nesterov)
    params = dict(net.named_parameters())
    cpu = {n: p.detach().cpu().clone() for n, p in params.items()}
    assert opt.param_groups[0]['lr'] == 0.02 and set(opt.param_groups[0]) == {'params', 'lr', 'wd', 'momentum', 'nesterov', 'ns_steps',
                                                                             'adamw_betas', 'adamw_eps'}
    for step in range(4):
        skip = ('unused',) if step in (1, 2) else ()
        grads = _write_grads(net, arena, 100 + step, skip=skip)
        if step == 2:                                       # the Scheduler rewrites lr every iteration
            opt.param_groups[0]['lr'] = ref.lr = 0.01
        before = {n: p.detach().cpu().clone() for n, p in params.items()}
        state_before = {n: (opt._param_view(opt.state1, p).clone(), opt._param_view(opt.state2, p).clone()) for n, p in params.items()}
        opt.step()
        torch.cuda.synchronize()
        for n, p in params.items():
            after = p.detach().cpu()
            s1, s2 = opt._param_view(opt.state1, p), opt._param_view(opt.state2, p)
            if n not in grads:                              # no gradient: parameter and state bit-identical
                assert torch.equal(after, before[n]) and torch.equal(s1, state_before[n][0]) and torch.equal(s2, state_before[n][1]), (step, n)
                continue
            if p.ndim >= 2:
                v = ref.muon_v(n, grads[n])
                buf = ref.state[n]['momentum_buffer']
                assert rel_err(s1.reshape(p.shape[0], -1), buf) < TOL, (step, n)
                # the orthogonalised update, recovered from the parameter: the ratio comes from shape[:2] -- max(24, 8) for the
                # conv weight, not max(24, 72)
                u_hat = (before[n].double() * (1 - ref.lr * ref.wd) - after.double()) / (ref.lr * M.muon_ratio(p.shape))
                e_k, e_r = M.judge(u_hat.reshape(p.shape[0], -1), v.to(torch.bfloat16))
                print(f'[muon step {step}] {n} {tuple(p.shape)}: e_k {e_k:.3e} e_r {e_r:.3e} ratio {e_k / e_r:.2f}')
                assert e_k <= e_r, (step, n, e_k, e_r)
            else:
                cpu[n] = ref.adamw_step(n, cpu[n], grads[n])
                assert rel_err(after, cpu[n]) < TOL, (step, n)
                assert rel_err(s1, ref.state[n]['moment1']) < TOL and rel_err(s2, ref.state[n]['moment2']) < TOL, (step, n)
        for n, p in params.items():                         # step counts advance only where a parameter was really updated
            b0 = arena.offsets[arena.names.index(n)] // 1024
            want = ref.state[n]['step'] if p.ndim < 2 and n in ref.state else 0
            assert float(opt.step_blk[b0]) == want, (step, n)
    # a step with a poisoned gradient and found_inf set leaves parameters and all state untouched
    snap = _snapshot(opt)
    _write_grads(net, arena, 999, poison=True)
    opt.step(None, torch.ones(1, device='cuda'))
    torch.cuda.synchronize()
    assert _same(snap, _snapshot(opt))
    assert bool(torch.isfinite(arena.flat_param).all())


def test_state_dict_round_trip():
    net, opt = _build()
    for step in range(2):
        _write_grads(net, opt.arena, 300 + step, skip=('unused',))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd) == {'state', 'param_groups'} and len(sd['param_groups']) == 1
    group = sd['param_groups'][0]
    assert {k: group[k] for k in group if k != 'params'} == dict(lr=0.02, wd=0.01, momentum=0.95, nesterov=True, ns_steps=5,
                                                                adamw_betas=(0.9, 0.999), adamw_eps=1e-8)
    order = [p for p in net.parameters() if p.ndim >= 2] + [p for p in net.parameters() if p.ndim < 2]
    names = {id(p): n for n, p in net.named_parameters()}
    assert group['params'] == list(range(len(order)))
    index = {id(p): i for i, p in enumerate(order)}
    for i, p in enumerate(order):
        entry, n = sd['state'][i], names[id(p)]
        if p.ndim >= 2:
            assert set(entry) == {'use_muon', 'momentum_buffer'} and entry['use_muon'] is True
            assert entry['momentum_buffer'].shape == (p.shape[0], p.numel() // p.shape[0])
        elif n.startswith('unused'):
            assert entry == {'use_muon': False}             # never stepped: no moments yet
        else:
            assert set(entry) == {'use_muon', 'step', 'moment1', 'moment2'} and entry['use_muon'] is False and entry['step'] == 2
            assert entry['moment1'].shape == p.shape
    # the conv momentum buffer: [24, 72] in logical (NCHW) element order, whatever the storage order
    conv_buf = sd['state'][0]['momentum_buffer']
    logical = opt._param_view(opt.state1, net.conv.weight).contiguous().reshape(24, 72)
    assert conv_buf.shape == (24, 72) and conv_buf.is_contiguous() and torch.equal(conv_buf, logical) and float(conv_buf.abs().max()) > 0
    assert float(sd['state'][index[id(net.unused.weight)]]['momentum_buffer'].abs().max()) == 0

    net2, opt2 = _build()
    with torch.no_grad():
        for a, b in zip(net2.parameters(), net.parameters()):
            a.copy_(b)
    opt2.load_state_dict(sd)
    assert _same(_snapshot(opt), _snapshot(opt2))
    for n_, o_ in ((net, opt), (net2, opt2)):
        _write_grads(n_, o_.arena, 400)
        o_.step()
    torch.cuda.synchronize()
    assert _same(_snapshot(opt), _snapshot(opt2))
    assert opt2.state_dict()['state'][index[id(net.bn.weight)]]['step'] == 3


# ------------------------------------------------------------------------------------------------ product path
def test_build_optimizer_muon_trains_the_tiny_vit_reproducibly(deterministic):
    """build_optimizer(('Muon', ...)) -> engine.Muon and the two-entry summary; four iterations through train_classification in
    deterministic mode, twice eagerly and once with the step captured into a hipGraph: losses and final parameters bit-equal."""
    from simpleaicv_pytorch_training_examples_amd import engine
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification import backbones, common
    from simpleaicv_pytorch_training_examples_amd.tools import scripts, utils
    from test_gpu_train_loop import SyntheticSet, _config, _loader
    fx = load_golden('vit_tiny_b3_64')

    def run(use_graph):
        config = _config(SyntheticSet(n=64, size=64, seed=3), batch=16)
        torch.manual_seed(fx['model_seed'])
        config.model = backbones.vit._vit(16, 192, 3, 3, 4, **fx['kwargs'])
        config.optimizer = ('Muon', {'lr': 4e-4, 'weight_decay': 1e-3, 'exclude_muon_layer_name_list': []})
        config.scheduler = ('CosineLR', {'warm_up_epochs': 1, 'min_lr': 1e-6})      # lr moves every iteration
        config.use_step_graph, config.step_graph_warmup = use_graph, 2
        model = config.model.cuda()
        optimizer, summary = utils.build_optimizer(config, model)
        assert isinstance(optimizer, engine.Muon)
        assert [s['optimizer'] for s in summary] == ['Muon', 'AdamW']
        muon_names, adamw_names = utils._muon_split(config, model)
        assert summary == [{'name': muon_names, 'optimizer': 'Muon', 'lr': 4e-4, 'weight_decay': 1e-3},
                           {'name': adamw_names, 'optimizer': 'AdamW', 'lr': 4e-4, 'weight_decay': 1e-3}]
        scheduler = utils.Scheduler(config, optimizer)
        model, config.ema_model, config.scaler = utils.build_training_mode(config, model)
        got, orig = [], common.AverageMeter.update

        def spy(self, val, n=1):
            got.append(float(val))
            return orig(self, val, n)
        common.AverageMeter.update = spy
        try:
            scripts.train_classification(_loader(config), model, config.train_criterion, optimizer, scheduler, 1,
                                         logging.getLogger('saicv_muon'), config)
        finally:
            common.AverageMeter.update = orig
        torch.cuda.synchronize()
        return got, optimizer.arena.flat_param.clone(), getattr(config, '_saicv_step_graphs', {})

    eager, p_eager, _ = run(False)
    eager2, p_eager2, _ = run(False)
    graph, p_graph, graphs = run(True)
    assert len(graphs) == 1 and next(iter(graphs.values())).graph is not None       # really captured and replayed
    assert len(eager) == 4 and all(l == l and l > 0 for l in eager)
    assert eager == eager2 and torch.equal(p_eager, p_eager2), 'two eager runs differ in deterministic mode'
    assert graph == eager, [(i, a, b) for i, (a, b) in enumerate(zip(eager, graph)) if a != b]
    assert torch.equal(p_eager, p_graph), float((p_eager - p_graph).norm() / p_eager.norm())
