"""bench.py's command line: a plain run times exactly --steps steps and prints the headline line only, --full adds the
measurements that take runs of their own, --dump-outputs DIR writes what the timed path computed as DIR/<name>.npy."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

FULL_ONLY = ('roofline', 'power', 'kernel_breakdown_ms_per_step', 'secondary', 'sam_b_encoder', 'resnet50_detr_config', 'sam_b',
             'cpu_baseline')


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module('bench')


class _Wrapped(torch.nn.Module):
    """Stands in for engine.DistributedDataParallel: the trained network is `.module`."""

    def __init__(self, module):
        super().__init__()
        self.module = module


def _net():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 64, 3), torch.nn.BatchNorm2d(64), torch.nn.Flatten(), torch.nn.Linear(64, 10))


def test_plain_is_the_default_and_the_new_options_parse(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert (a.full, a.atomics, a.dump_outputs, a.steps, a.warmup) == (False, False, None, 7, 2)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full and a.dump_outputs == 'out'


def test_dump_outputs_writes_every_parameter_and_buffer_as_float_arrays(tmp_path, monkeypatch):
    """Small tensors whole, larger ones as a fixed sample of their share of the budget: the same elements in every run."""
    bench = _bench()
    net = _net()
    monkeypatch.setattr(bench, 'DUMP_BYTES', 8 * 900)           # 9 tensors -> 100 elements each
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), _Wrapped(net), {'loss': 2.5})
    tensors = {'param.' + n: p for n, p in net.named_parameters()}
    tensors.update({'buffer.' + n: b for n, b in net.named_buffers()})
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(['loss.npy'] + [n + '.npy' for n in tensors])
    loss = np.load(tmp_path / 'a' / 'loss.npy')
    assert loss.dtype == np.float64 and float(loss) == 2.5
    for name, t in tensors.items():
        got = np.load(tmp_path / 'a' / (name + '.npy'))
        assert np.array_equal(got, np.load(tmp_path / 'b' / (name + '.npy'))), name
        assert got.dtype == (np.float32 if t.is_floating_point() else np.float64), name
        flat = t.detach().reshape(-1).double().numpy()
        if flat.size <= 100:
            assert np.array_equal(got.astype(np.float64), flat), name
        else:
            assert got.size == 100 and np.isin(got.astype(np.float64), flat).all(), name


def test_dump_outputs_stays_within_64_mb():
    """A model of 80 MB of fp32 weights is sampled down to the budget."""
    import tempfile
    bench = _bench()
    net = torch.nn.Linear(5000, 4000)
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, net, {'loss': 1.0})
        total = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
    assert total <= 64 * 2 ** 20


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_times_exactly_its_steps_and_dumps_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one timed window of K steps in the deterministic mode, the headline
    fields only, and the loss and trained weights of the timed path in DIR -- bit for bit the same in a second process."""
    lines = []
    for d in ('a', 'b'):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1',
                              '--dump-outputs', str(tmp_path / d)], capture_output=True, text=True, timeout=400)
        assert out.returncode == 0, out.stderr[-3000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1]))
    line = lines[0]
    assert (line['metric'], line['unit'], line['higher_is_better'], line['dtype']) == ('training images/sec/node', 'images/s', True, 'bf16')
    assert line['steps'] == 3 and len(line['windows_ms_per_step']) == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert line['ms_per_step'] == line['windows_ms_per_step'][0]
    assert line['config']['deterministic'] is True and line['config']['bn_statistics'] == 'fixed-order partial rows'
    assert not set(FULL_ONLY) & set(line), sorted(set(FULL_ONLY) & set(line))
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert {'loss.npy', 'param.fc.weight.npy', 'buffer.conv1.layer.1.running_mean.npy'} <= set(files)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64 * 2 ** 20
    assert abs(float(np.load(tmp_path / 'a' / 'loss.npy')) - line['config']['final_loss']) < 1e-4
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
