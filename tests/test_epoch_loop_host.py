"""The per-iteration state machine of the training loops in tools/, on the CPU with stubs: accumulation phase, the carried skip
flag, the lagged host read that logs "skip this batch!" and moves the logged / scheduled iteration index back, the scheduler
arguments, the log lines and the parameter trajectory.  Five public loops are driven -- train_classification (scalar loss),
train_semantic_segmentation (dict, two terms), train_detection with a six-term criterion (stacked sum), train_sam_segmentation and
train_sam_matting (fixed key order, iteration width 6) -- each with accumulation 1 and 2 and host_sync_lag 0 and 2.

Expected values come from `reference_run` below: a plain eager loop (forward, backward, skip the window if anything in it was
non-finite, SGD) with the documented bookkeeping written out -- a skipped iteration is not counted, but the host learns of it only
`host_sync_lag` boundaries late.  Nothing expected is read from the code under test."""
import collections
import contextlib
import copy
import types

import pytest
import torch

BATCH, BATCHES = 8, 6
LR0 = 0.05
SAM_KEYS = ('focal_loss', 'dice_loss', 'iou_predict_loss')
MATTING_KEYS = ('global_pred_trimap_ce_loss', 'global_pred_trimap_iou_loss', 'local_pred_alpha_loss', 'local_pred_laplacian_loss',
                'fusion_pred_alpha_loss', 'fusion_pred_laplacian_loss', 'composition_loss', 'iou_predict_loss')
DET_KEYS = ('cls_loss', 'reg_loss', 'center_loss', 'aux_a', 'aux_b', 'aux_c')


def lr_at(progress):
    return LR0 * (1.0 - 0.1 * progress)


# ------------------------------------------------------------------------------------------------ stubs
class Net(torch.nn.Module):
    """Linear(4, 3) with a counting no_sync(); `.module` is the net itself, with the two SAM forward entry points"""

    def __init__(self, outputs_of=None):
        super().__init__()
        torch.manual_seed(3)
        self.lin = torch.nn.Linear(4, 3)
        self.no_sync_entered = 0
        self.outputs_of = outputs_of

    @property
    def module(self):
        return self

    def forward(self, x):
        return self.lin(x)

    @contextlib.contextmanager
    def no_sync(self):
        self.no_sync_entered += 1
        yield

    def finish_gradient_sync(self):
        pass

    def forward_image_encoder(self, images):
        return images * 1.0

    def forward_prompt_encoder_mask_decoder(self, embeddings, prompts, mask_out_idxs=None):
        assert prompts['prompt_point'] is not None and prompts['prompt_box'] is not None and prompts['prompt_mask'] is None
        return self.outputs_of(self.lin(embeddings))


class SGD:
    """records every step(inv_scale, skip_flag); plain SGD at `lr` unless the flag is set"""

    def __init__(self, model):
        self.params = list(model.parameters())
        self.lr = LR0
        self.found_inf = torch.zeros(1)
        self.flags, self.snapshots = [], []

    def check_finite(self):
        pass

    def clip_grad_value_(self, value, inv_scale=None):
        pass

    def clip_grad_norm_(self, norm, inv_scale=None):
        pass

    def refresh_hyper(self):
        pass

    def step(self, inv_scale, skip_flag):
        assert inv_scale is None
        skip = bool(skip_flag.reshape(-1)[0] != 0)
        self.flags.append(int(skip))
        if not skip:
            with torch.no_grad():
                for p in self.params:
                    p -= self.lr * p.grad
        self.snapshots.append([p.detach().clone() for p in self.params])

    def zero_grad(self):
        for p in self.params:
            p.grad = None


class Scheduler:
    def __init__(self):
        self.current_lr = LR0
        self.calls = []

    def step(self, optimizer, progress):
        self.calls.append(progress)
        self.current_lr = optimizer.lr = lr_at(progress)


class Logger:
    def __init__(self):
        self.lines = []

    def info(self, line):
        self.lines.append(line)


class Loader(list):
    dataset = range(BATCH * BATCHES)


def make_config(acc, lag, **extra):
    return types.SimpleNamespace(local_rank=0, total_rank=0, gpus_num=1, group=None, batch_size=BATCH, accumulation_steps=acc,
                                 host_sync_lag=lag, print_interval=1, use_amp=False, use_ema_model=False, **extra)


# ------------------------------------------------------------------------------------------------ the five loops
def _mse(a, b):
    return ((a - b) ** 2).mean()


def _tensors(seed, poisoned):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(BATCHES):
        x = torch.randn(BATCH, 4, generator=g)
        if i == poisoned:
            x[2, 1] = float('inf')
        out.append((x, torch.randn(BATCH, 3, generator=g), torch.randint(0, 3, (BATCH,), generator=g)))
    return out


class Shape:
    """One public loop: how to call it, its batches, and -- for the reference -- inputs, forward + loss in plain torch"""
    total_name, width, keys, print_terms, stacked, extra = 'loss', 5, None, True, False, {}

    def net(self):
        return Net()


class Classification(Shape):
    print_terms = False

    def batches(self, poisoned):
        return [{'image': x, 'label': y} for x, _, y in _tensors(11, poisoned)]

    def call(self, loader, model, optimizer, scheduler, epoch, logger, config):
        from simpleaicv_pytorch_training_examples_amd.tools.scripts import train_classification
        return train_classification(loader, model, torch.nn.functional.cross_entropy, optimizer, scheduler, epoch, logger, config)

    def inputs(self, data):
        return [data['image']]

    def loss(self, model, data):
        return torch.nn.functional.cross_entropy(model.lin(data['image']), data['label'])


class SemanticSegmentation(Shape):
    keys = ('CELoss', 'DiceLoss')
    extra = {'loss_ratio': {'CELoss': 1.0, 'DiceLoss': 0.5}}

    def batches(self, poisoned):
        return [{'image': x, 'mask': t} for x, t, _ in _tensors(12, poisoned)]

    def call(self, loader, model, optimizer, scheduler, epoch, logger, config):
        from simpleaicv_pytorch_training_examples_amd.tools.scripts import train_semantic_segmentation
        criterion = collections.OrderedDict([('CELoss', _mse), ('DiceLoss', lambda o, m: (o - m).abs().mean())])
        return train_semantic_segmentation(loader, model, criterion, optimizer, scheduler, epoch, logger, config)

    def inputs(self, data):
        return [data['image'], data['mask']]

    def loss(self, model, data):
        out = model.lin(data['image'])
        return {'CELoss': 1.0 * _mse(out, data['mask']), 'DiceLoss': 0.5 * (out - data['mask']).abs().mean()}


def _six_terms(out, target):
    return {k: (i + 1) * 0.25 * _mse(out, target) if i % 2 else (out - target).abs().mean() * (i + 1) for i, k in enumerate(DET_KEYS)}


class Detection(Shape):
    total_name, keys, stacked = 'total_loss', DET_KEYS, True
    extra = {'network': 'resnet50_retinanet'}

    def batches(self, poisoned):
        return [{'image': x, 'annots': t} for x, t, _ in _tensors(13, poisoned)]

    def call(self, loader, model, optimizer, scheduler, epoch, logger, config):
        from simpleaicv_pytorch_training_examples_amd.tools.scripts import train_detection
        return train_detection(loader, model, _six_terms, optimizer, scheduler, epoch, logger, config)

    def inputs(self, data):
        return [data['image'], data['annots']]

    def loss(self, model, data):
        return _six_terms(model.lin(data['image']), data['annots'])


_SAM_EXTRA = {'decoder_iters': 0, 'mask_out_idxs': [0], 'use_single_prompt': False, 'frozen_image_encoder': False,
              'frozen_prompt_encoder': False, 'frozen_mask_decoder': False,
              'prompt_probs': {'prompt_point': 1.0, 'prompt_box': 1.0, 'prompt_mask': 0.0}}


def _prompts():
    return {'prompt_point': torch.zeros(BATCH, 1, 3), 'prompt_box': torch.zeros(BATCH, 4), 'prompt_mask': torch.zeros(BATCH, 1, 2, 2)}


def _sam_terms(mask_preds, iou_preds, masks):
    # returned in another order than SAM_KEYS: the loop logs in the order of its own tuple
    return {'iou_predict_loss': 0.5 * (iou_preds ** 2).mean(), 'focal_loss': _mse(mask_preds, masks),
            'dice_loss': (mask_preds - masks).abs().mean()}


class SamSegmentation(Shape):
    width, keys, extra = 6, SAM_KEYS, _SAM_EXTRA

    def net(self):
        return Net(lambda out: (out, out.mean(dim=1, keepdim=True)))

    def batches(self, poisoned):
        return [dict(_prompts(), image=x, mask=t) for x, t, _ in _tensors(14, poisoned)]

    def call(self, loader, model, optimizer, scheduler, epoch, logger, config):
        from simpleaicv_pytorch_training_examples_amd.tools.interactive_segmentation_scripts import train_sam_segmentation

        def criterion(preds, masks):
            (mask_preds,), (iou_preds,) = preds
            return _sam_terms(mask_preds, iou_preds, masks)
        return train_sam_segmentation(loader, model, criterion, optimizer, scheduler, epoch, logger, config)

    def inputs(self, data):
        return [data['image']]

    def loss(self, model, data):
        out = model.lin(data['image'] * 1.0)
        return _sam_terms(out, out.mean(dim=1, keepdim=True), data['mask'])


def _matting_terms(images, outs, targets):
    global_pred, local_pred, fused_pred, iou_pred = outs
    mask, trimap, fg_map, bg_map = targets
    values = [_mse(global_pred, trimap), (global_pred - trimap).abs().mean(), _mse(local_pred, mask), (local_pred - mask).abs().mean(),
              _mse(fused_pred, mask), (fused_pred - mask).abs().mean(), _mse(fused_pred * fg_map + (1 - fused_pred) * bg_map, mask),
              0.5 * (iou_pred ** 2).mean() + 0. * images.sum()]
    terms = dict(zip(MATTING_KEYS, values))
    return {k: terms[k] for k in reversed(MATTING_KEYS)}         # again not the logged order


class SamMatting(Shape):
    width, keys, extra = 6, MATTING_KEYS, _SAM_EXTRA

    def net(self):
        return Net(lambda out: (out, out * 0.5, out * 0.25 + 0.1, out.mean(dim=1, keepdim=True)))

    def batches(self, poisoned):
        return [dict(_prompts(), image=x, mask=t, trimap=t * 0.5, fg_map=t + 1.0, bg_map=t - 1.0) for x, t, _ in _tensors(15, poisoned)]

    def call(self, loader, model, optimizer, scheduler, epoch, logger, config):
        from simpleaicv_pytorch_training_examples_amd.tools.interactive_matting_scripts import train_sam_matting

        def criterion(images, all_iter, targets):
            return _matting_terms(images, [o[0] for o in all_iter], targets)
        return train_sam_matting(loader, model, criterion, optimizer, scheduler, epoch, logger, config)

    def inputs(self, data):
        return [data['image']]

    def loss(self, model, data):
        out = model.lin(data['image'] * 1.0)
        outs = (out, out * 0.5, out * 0.25 + 0.1, out.mean(dim=1, keepdim=True))
        return _matting_terms(data['image'], outs, [data[k] for k in ('mask', 'trimap', 'fg_map', 'bg_map')])


SHAPES = {'classification': Classification(), 'semantic_segmentation': SemanticSegmentation(), 'detection': Detection(),
          'sam_segmentation': SamSegmentation(), 'sam_matting': SamMatting()}


# ------------------------------------------------------------------------------------------------ the reference
Expected = collections.namedtuple('Expected', 'lines averages scheduler flags snapshots no_sync')


def reference_run(shape, batches, acc, lag, epochs=1):
    """Plain eager loop.  A window of `acc` micro-batches is skipped as a whole when any input, the total or a term of any of its
    micro-batches is inf / nan (or the total is 0); the host meters and logs the LAST micro-batch of a window, `lag` host reads
    late, and takes the iteration index back by one when the window it reads turns out skipped."""
    model = shape.net()
    params = list(model.parameters())
    lr = LR0
    iters = BATCH * BATCHES // BATCH
    lines, averages, scheduler, flags, snapshots, no_sync = [], [], [], [], [], 0
    for epoch in range(1, epochs + 1):
        lines.append('use_amp: False, amp_type: torch.bfloat16!')
        index, pending, meter_sum, meter_n, window_bad = 1, collections.deque(), 0., 0, False

        def drain(keep):
            nonlocal index, meter_sum, meter_n
            while len(pending) > keep:
                skipped, total, terms, n, head = pending.popleft()
                if skipped:
                    lines.append('skip this batch!')
                    index -= 1
                    continue
                meter_sum, meter_n = meter_sum + total * n, meter_n + n
                if head is not None:
                    line = head + f'{shape.total_name}: {total * acc:.4f}'
                    if shape.print_terms:
                        line += ', ' + ''.join(f'{k}: {v * acc:.4f}, ' for k, v in zip(shape.keys, terms))
                    lines.append(line)

        for micro, data in enumerate(batches, 1):
            value = shape.loss(model, data)
            terms = []
            if isinstance(value, dict):
                if shape.stacked:                      # above four terms: one stack + one sum (except SAM matting, chained)
                    total = torch.stack([value[k].float() for k in shape.keys]).sum()
                else:
                    total = sum(value.values())
                terms = [float(value[k].detach().float() / acc) for k in shape.keys]
            else:
                total = value
            bad = any(not bool(torch.isfinite(t).all()) for t in shape.inputs(data))
            bad = bad or not bool(torch.isfinite(total)) or float(total.detach()) == 0. or any(t != t or abs(t) == float('inf') for t in terms)
            window_bad = window_bad or bad
            (total / acc).backward()
            if micro % acc == 0:
                if not window_bad:
                    with torch.no_grad():
                        for p in params:
                            p -= lr * p.grad
                flags.append(int(window_bad))
                snapshots.append([p.detach().clone() for p in params])
                for p in params:
                    p.grad = None
                progress = index / iters + (epoch - 1)
                scheduler.append(progress)
                lr = lr_at(progress)
                head = None
                if index % acc == 0:
                    head = (f'train: epoch {epoch:0>4d}, iter [{index // acc:0>{shape.width}d}, {iters // acc:0>{shape.width}d}], '
                            f'lr: {lr:.6f}, ')
                pending.append((window_bad, float((total / acc).detach().float()), terms, BATCH, head))
                window_bad = False
            else:
                no_sync += 1
            drain(lag)
            index += 1
        drain(0)
        averages.append(meter_sum / meter_n * acc)
    return Expected(lines, averages, scheduler, flags, snapshots, no_sync)


def run_loop(shape, batches, acc, lag, epochs=1):
    model = shape.net()
    optimizer, scheduler, logger = SGD(model), Scheduler(), Logger()
    config = make_config(acc, lag, **copy.deepcopy(shape.extra))
    averages = [shape.call(Loader(batches), model, optimizer, scheduler, epoch, logger, config) for epoch in range(1, epochs + 1)]
    return Expected(logger.lines, averages, scheduler.calls, optimizer.flags, optimizer.snapshots, model.no_sync_entered)


def assert_same(got, want):
    assert got.lines == want.lines
    assert got.scheduler == want.scheduler
    assert got.flags == want.flags
    assert got.no_sync == want.no_sync
    assert got.averages == pytest.approx(want.averages, rel=1e-6)
    assert len(got.snapshots) == len(want.snapshots)
    for step, (a, b) in enumerate(zip(got.snapshots, want.snapshots)):
        for p, q in zip(a, b):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-7), step


GRID = [(name, acc, lag) for name in SHAPES for acc in (1, 2) for lag in (0, 2)]
IDS = [f'{name}-acc{acc}-lag{lag}' for name, acc, lag in GRID]


@pytest.mark.parametrize('name,acc,lag', GRID, ids=IDS)
def test_clean_epoch_logs_schedules_and_steps_like_the_plain_loop(name, acc, lag):
    shape = SHAPES[name]
    batches = shape.batches(poisoned=None)
    got, want = run_loop(shape, batches, acc, lag), reference_run(shape, batches, acc, lag)
    assert_same(got, want)
    # literal anchors, independent of the reference loop as well
    steps = BATCHES // acc
    assert got.flags == [0] * steps and got.no_sync == BATCHES - steps
    assert got.scheduler == [k * acc / BATCHES for k in range(1, steps + 1)]
    assert len(got.lines) == 1 + steps
    w = shape.width
    assert got.lines[1].startswith(f'train: epoch 0001, iter [{1:0>{w}d}, {steps:0>{w}d}], lr: {lr_at(acc / BATCHES):.6f}, {shape.total_name}: ')
    if shape.print_terms:
        assert [part.split(': ')[0] for part in got.lines[1].split(', ')[4:-1]] == [shape.total_name] + list(shape.keys)
        assert got.lines[1].endswith(', ')
    else:
        assert got.lines[1].count(', ') == 4 and not got.lines[1].endswith(' ')


@pytest.mark.parametrize('name,acc,lag', GRID, ids=IDS)
def test_poisoned_batch_skips_its_window_and_the_index_moves_back_when_drained(name, acc, lag):
    shape = SHAPES[name]
    batches = shape.batches(poisoned=3)           # accumulation 2: the SECOND (boundary) micro-batch of the second window
    got, want = run_loop(shape, batches, acc, lag), reference_run(shape, batches, acc, lag)
    assert_same(got, want)
    assert got.lines.count('skip this batch!') == 1
    assert got.flags == ([0, 1, 0] if acc == 2 else [0, 0, 0, 1, 0, 0])
    k = got.flags.index(1)
    assert all(torch.equal(p, q) for p, q in zip(got.snapshots[k], got.snapshots[k - 1]))
    assert not any(torch.equal(p, q) for p, q in zip(got.snapshots[k + 1], got.snapshots[k]))
    numbers = [int(line.split('iter [')[1].split(',')[0]) if line.startswith('train:') else line for line in got.lines[1:]]
    literal = {(1, 0): [1, 2, 3, 'skip this batch!', 4, 5], (1, 2): [1, 2, 3, 'skip this batch!', 5, 6],
               (2, 0): [1, 'skip this batch!'], (2, 2): [1, 'skip this batch!', 3]}[(acc, lag)]
    assert numbers == literal


@pytest.mark.parametrize('name,acc,lag', GRID, ids=IDS)
def test_poisoned_first_micro_batch_is_carried_to_the_window_boundary(name, acc, lag):
    shape = SHAPES[name]
    batches = shape.batches(poisoned=2)           # accumulation 2: the FIRST micro-batch of the second window
    got, want = run_loop(shape, batches, acc, lag), reference_run(shape, batches, acc, lag)
    assert_same(got, want)
    assert got.lines.count('skip this batch!') == 1
    assert got.flags == ([0, 1, 0] if acc == 2 else [0, 0, 1, 0, 0, 0])
    k = got.flags.index(1)
    assert all(torch.equal(p, q) for p, q in zip(got.snapshots[k], got.snapshots[k - 1]))


@pytest.mark.parametrize('name,acc,lag', [g for g in GRID if g[0] != 'classification'], ids=[i for i in IDS if not i.startswith('classification')])
def test_second_epoch_on_the_same_config_still_prints_the_term_names(name, acc, lag):
    shape = SHAPES[name]
    batches = shape.batches(poisoned=None)
    got, want = run_loop(shape, batches, acc, lag, epochs=2), reference_run(shape, batches, acc, lag, epochs=2)
    assert_same(got, want)
    second = [line for line in got.lines if line.startswith('train: epoch 0002')]
    assert len(second) == BATCHES // acc
    for line in second:
        assert [part.split(': ')[0] for part in line.split(', ')[4:-1]] == [shape.total_name] + list(shape.keys)
