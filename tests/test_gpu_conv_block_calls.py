"""The launch plan of the host layer: which C-ABI entry points ops.conv_bn_act / ops.conv2d call, in which order, for every
path through ConvBnActFn and ConvFn (ordinary, inline / partial-row statistics, eval, fused BatchNorm-backward reduction,
residual join with a deferred shortcut, pooled space-to-depth stem, strided / arena weights, biased and padded-K plain
convolutions).  The numbers these paths produce are pinned elsewhere (test_gpu_kernels.py, test_gpu_r04.py, the deterministic
trajectories); this file pins the SEQUENCE, so that a restructuring of ops.py cannot quietly add, drop or reorder a launch.

Every expected list below was recorded by running this file at commit 227facba1fd3 -- the parent of the change that split
ConvBnActFn into stages -- and checked against a reading of that commit's ops.py; none of them comes from the code under test.
Names are entry points of include/saicv_hip.h without the `saicv_` prefix.  `saicv_pack_weight*` calls are left out: whether a
weight is (re)packed depends on what earlier tests left alive in ops._PackRegistry.

Shapes: N = 2, 12 x 12, 32 / 64 channels, fp32; channels_last weights unless a case says otherwise.  Two cases run in bf16: the
repeat of the plain block under autocast (the cast in conv_bn_act), and ConvFn with K = 36 -- 36 output channels are whole
16-byte chunks of fp32 (4 per chunk) but not of bf16 (8 per chunk), so only there does K = 36 reach the zero-padded branch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, HW = 2, 12


class _Recorder:
    """Stands in for ops.lib(): notes the name of every entry point fetched for a call and hands out the real function."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._real, name)

    def take(self):
        """Names recorded since the last take(), without the prefix and without the weight-packing launches."""
        out = [n[len('saicv_'):] for n in self.names if not n.startswith('saicv_pack_weight')]
        self.names = []
        return out


@pytest.fixture
def env(monkeypatch):
    from simpleaicv_pytorch_training_examples_amd import ops
    rec = _Recorder(ops.lib())
    monkeypatch.setattr(ops, 'lib', lambda: rec)
    for name in ('BN_FUSE', 'BN_INLINE', 'DS_JOIN_FUSE'):
        monkeypatch.setattr(ops, name, True)
    torch.manual_seed(0)
    return ops, rec, monkeypatch


def _x(c, h=HW, w=HW, grad=True):
    return torch.randn(N, c, h, w, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(grad)


def _block(cin, cout, k=3, stride=1, pad=1, act=True, channels_last=True):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import ConvBnActBlock
    blk = ConvBnActBlock(cin, cout, k, stride, pad, has_act=act).cuda()
    if channels_last:
        blk.layer[0].weight.data = blk.layer[0].weight.data.contiguous(memory_format=torch.channels_last)
    return blk


def _run(rec, fn, x):
    """-> (names of the forward, names of the backward) of z = fn(x) and z.backward(a dense gradient laid out like z: the
    gated shortcut gradient and the fused reductions pass the very tensor they were handed on, never a copy)"""
    rec.take()
    z = fn(x)
    fwd = rec.take()
    z.backward(torch.randn_like(z))
    torch.cuda.synchronize()
    return fwd, rec.take()


FWD_INLINE = ['conv2d_stat_rows', 'conv2d_fwd_stats', 'bn_act_fwd_stats']
FWD_ROWS = ['conv2d_stat_rows', 'conv2d_fwd', 'bn_ws_floats', 'bn_finalize_fwd', 'bn_act_fwd']
BWD_PLAIN = ['bn_bwd_ws_floats', 'bn_act_bwd', 'conv2d_dgrad', 'conv2d_wgrad']


@pytest.mark.parametrize('inline, autocast, fwd', [(True, False, FWD_INLINE), (False, False, FWD_ROWS), (True, True, FWD_INLINE)],
                         ids=['inline', 'partial_rows', 'inline_bf16_autocast'])
def test_conv_bn_relu_train(env, inline, autocast, fwd):
    ops, rec, mp = env
    mp.setattr(ops, 'BN_INLINE', inline)
    blk = _block(32, 64)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        got = _run(rec, blk, _x(32))
    print(got)
    assert got == (fwd, BWD_PLAIN)


def test_conv_bn_relu_eval(env):
    ops, rec, mp = env
    blk = _block(32, 64).eval()
    rec.take()
    with torch.no_grad():
        blk(_x(32))
    fwd = rec.take()
    print(fwd)
    assert fwd == ['conv2d_fwd', 'bn_eval_coeffs', 'bn_act_fwd']
    z = blk(_x(32))
    with pytest.raises(NotImplementedError):
        z.sum().backward()


@pytest.mark.parametrize('fuse, inline', [(True, True), (True, False), (False, True)], ids=['fused_inline', 'fused_partials', 'three_pass'])
def test_two_chained_blocks(env, fuse, inline):
    """The second block's data gradient leaves the partial sums of the first block's BatchNorm backward behind."""
    ops, rec, mp = env
    mp.setattr(ops, 'BN_FUSE', fuse)
    mp.setattr(ops, 'BN_INLINE', inline)
    a, b = _block(32, 64), _block(64, 64)
    got = _run(rec, lambda x: b(a(x)), _x(32))
    print(got)
    one = FWD_INLINE if inline else FWD_ROWS
    second = (['bn_bwd_ws_floats', 'bn_act_bwd', 'conv2d_dgrad_stat_rows', 'conv2d_dgrad_fused', 'conv2d_wgrad'] if fuse
              else BWD_PLAIN)
    first = ['bn_bwd_ws_floats', 'bn_act_bwd_inline' if inline else 'bn_act_bwd_from_partials', 'conv2d_dgrad', 'conv2d_wgrad']
    assert got == (one + one, second + (first if fuse else BWD_PLAIN))


JOIN = {
    # BasicBlock(32, 64, stride=2): conv1 (+ alias of its input), the 1 x 1 stride-2 shortcut, conv2 joining the two
    True: (FWD_INLINE
           + ['conv2d_stat_rows', 'conv2d_fwd_stats', 'bn_ws_floats', 'bn_finalize_fwd']        # shortcut: raw output + coefficients
           + ['conv2d_stat_rows', 'conv2d_fwd_stats', 'bn_act_fwd_join']),
    False: FWD_INLINE + FWD_INLINE + FWD_INLINE,
}
JOIN_BWD = (['bn_bwd_ws_floats', 'bn_act_bwd', 'conv2d_dgrad_stat_rows', 'conv2d_dgrad_fused', 'conv2d_wgrad']      # conv2; dres = (dz, mask)
            + ['bn_bwd_ws_floats', 'bn_act_bwd', 'conv2d_dgrad', 'conv2d_wgrad']                                  # shortcut applies the gate
            + ['bn_bwd_ws_floats', 'bn_act_bwd_inline', 'conv2d_dgrad_add', 'conv2d_wgrad'])                      # conv1 + the alias' gradient


@pytest.mark.parametrize('join', [True, False], ids=['deferred_shortcut', 'materialised_shortcut'])
def test_basic_block_with_shortcut_convolution(env, join):
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import BasicBlock
    ops, rec, mp = env
    mp.setattr(ops, 'DS_JOIN_FUSE', join)
    blk = BasicBlock(32, 64, stride=2).cuda()
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    got = _run(rec, blk, _x(32))
    print(got)
    assert got == (JOIN[join], JOIN_BWD)
    assert ops._GateLedger.pending == 0


def test_basic_block_with_identity_shortcut(env):
    """The alias' gradient arrives as (dz, ReLU mask) and joins, gated, in conv1's data-gradient epilogue."""
    from simpleaicv_pytorch_training_examples_amd.SimpleAICV.classification.backbones.resnet import BasicBlock
    ops, rec, mp = env
    blk = BasicBlock(64, 64).cuda()
    for p in blk.parameters():
        if p.dim() == 4:
            p.data = p.data.contiguous(memory_format=torch.channels_last)
    got = _run(rec, blk, _x(64))
    print(got)
    assert got == (FWD_INLINE + FWD_INLINE,
                   ['bn_bwd_ws_floats', 'bn_act_bwd', 'conv2d_dgrad_stat_rows', 'conv2d_dgrad_fused', 'conv2d_wgrad',
                    'bn_bwd_ws_floats', 'bn_act_bwd_inline', 'conv2d_dgrad_fused', 'conv2d_wgrad'])
    assert ops._GateLedger.pending == 0


def test_pooled_space_to_depth_stem(env):
    ops, rec, mp = env
    blk = _block(3, 64, 7, 2, 3)
    xp = ops.pack_stem_input(torch.randn(N, 3, 33, 47, device='cuda'), blk.layer[0])
    assert getattr(xp, '_saicv_s2d', None) is not None
    got = _run(rec, lambda x: blk(x, pool=(3, 2, 1)), xp)
    print(got)
    assert got == (['conv2d_stat_rows', 'conv2d_fwd', 'bn_ws_floats', 'bn_finalize_fwd', 'bn_relu_maxpool_fwd'],
                   ['bn_relu_maxpool_bwd_ws_floats', 'bn_relu_maxpool_bwd', 'conv2d_wgrad', 'unpack_wgrad_s2d'])


def test_weight_that_is_not_channels_last(env):
    ops, rec, mp = env
    blk = _block(32, 64, channels_last=False)
    assert not blk.layer[0].weight.is_contiguous(memory_format=torch.channels_last)
    got = _run(rec, blk, _x(32))
    print(got)
    assert got == (FWD_INLINE, BWD_PLAIN + ['unpack_wgrad'])


def _returns_of(mp, fn_cls):
    """Wraps fn_cls.backward; -> the list its return tuples are appended to."""
    seen, real = [], fn_cls.backward

    def backward(ctx, *grads):
        out = real(ctx, *grads)
        seen.append(out)
        return out

    mp.setattr(fn_cls, 'backward', staticmethod(backward))
    return seen


def _assert_arena_filled(arena):
    torch.cuda.synchronize()
    assert all(arena.arrived)
    for n, p in zip(arena.names, arena.params):
        assert float(p.grad.abs().sum()) > 0, n


def test_parameters_in_a_flat_arena(env):
    """Kernels accumulate straight into p.grad and the node returns None: autograd's AccumulateGrad still signals completion."""
    from simpleaicv_pytorch_training_examples_amd import engine
    ops, rec, mp = env
    blk = _block(32, 64)
    arena = engine.FlatArena(list(blk.named_parameters()), torch.device('cuda'))
    assert blk.layer[0].weight.is_contiguous(memory_format=torch.channels_last)
    seen = _returns_of(mp, ops.ConvBnActFn)
    got = _run(rec, blk, _x(32))
    print(got)
    assert got == (FWD_INLINE, BWD_PLAIN)
    (out,) = seen
    assert out[0] is not None and out[1] is None and out[2] is None and out[3] is None
    _assert_arena_filled(arena)


CONV_BWD = {'k32': ['conv2d_dgrad', 'conv2d_wgrad_bias'], 'k36_padded': ['conv2d_dgrad', 'conv2d_wgrad'],
            'frozen_weight': ['conv2d_dgrad', 'colsum'], 'arena': ['conv2d_dgrad', 'conv2d_wgrad_bias']}


@pytest.mark.parametrize('variant', list(CONV_BWD))
def test_plain_convolution_with_bias(env, variant):
    from simpleaicv_pytorch_training_examples_amd import engine
    ops, rec, mp = env
    k = 36 if variant == 'k36_padded' else 32
    conv = torch.nn.Conv2d(32, k, 3, padding=1).cuda()
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    if variant == 'frozen_weight':
        conv.weight.requires_grad_(False)
    arena = engine.FlatArena(list(conv.named_parameters()), torch.device('cuda')) if variant == 'arena' else None
    seen = _returns_of(mp, ops.ConvFn)
    # (K = 36 is zero-padded only where a 16-byte chunk holds 8 channels: bf16)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=variant == 'k36_padded'):
        got = _run(rec, lambda x: ops.conv2d(x, conv.weight, conv.bias, 1, 1), _x(32))
    print(got)
    assert got == (['conv2d_fwd'], CONV_BWD[variant])
    (out,) = seen
    assert out[0] is not None
    if arena is not None:
        assert out[1] is None and out[2] is None
        _assert_arena_filled(arena)
    else:
        assert out[2].shape == (k,) and conv.bias.grad.shape == (k,)
        assert (out[1] is None) == (variant == 'frozen_weight')
